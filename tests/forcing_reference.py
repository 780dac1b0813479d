"""NumPy restatement of core/forcing.f90, line for line: spng_init's widths (:124-140), spng_set
(:157-237), mth_stepf (:239-251), activate_sponge's mask (:101-104), nekStab_forcing (:2-52) and
nekStab_forcing_temp (:54-79).  Independent of the product: it shares no arithmetic with
nekstab_next_amd.forcing.  Every elementwise NumPy operation is one IEEE f64 operation per point in the
source's left-to-right order (NumPy never contracts); ``exp``, ``cos`` and ``sin`` are the C library's
(``math``), called per point, so their error bound is glibc's."""
import math

import numpy as np

XDMIN, XDMAX = 0.0010, 0.9990      # parameter(xdmin=0.0010d0, xdmax=0.9990d0), :243
EXP_OVERFLOW = 709.78              # exp of an f64 overflows above this argument


def mth_stepf(x, stats=None):
    """real function mth_stepf(x), :239-251.  ``stats['max_exp_arg']`` records the largest argument of exp,
    ``stats['near_overflow']`` counts the arguments within 1 of the f64 overflow threshold."""
    if x <= XDMIN:
        return 0.0
    elif x <= XDMAX:
        arg = 1.0 / (x - 1.0) + 1.0 / x
        if stats is not None:
            stats["max_exp_arg"] = max(stats.get("max_exp_arg", -math.inf), arg)
            stats["near_overflow"] = stats.get("near_overflow", 0) + int(abs(arg - EXP_OVERFLOW) <= 1.0)
        try:
            e = math.exp(arg)
        except OverflowError:          # Fortran's exp returns +Inf above 709.78: 1/(1 + Inf) = 0
            e = math.inf
        return 1.0 / (1.0 + e)
    else:
        return 1.0


def spng_init(acc_spg, lengths, ndim):
    """The widths of spng_init, :124-140.  lengths: [(xLspg, xRspg), (yLspg, yRspg), (zLspg, zRspg)]."""
    acc_spg = abs(acc_spg)
    spng_wl = [(1.0 - acc_spg) * lengths[il][0] for il in range(ndim)]   # left section width
    spng_wr = [(1.0 - acc_spg) * lengths[il][1] for il in range(ndim)]   # right section width
    spng_dl = [(acc_spg) * lengths[il][0] for il in range(ndim)]         # left drop/rise section width
    spng_dr = [(acc_spg) * lengths[il][1] for il in range(ndim)]         # right drop/rise section width
    return spng_wl, spng_wr, spng_dl, spng_dr


def spng_set(coords, bmin, bmax, spng_wl, spng_wr, spng_dl, spng_dr, stats=None):
    """subroutine spng_set, :157-229.  coords: [XM1, YM1[, ZM1]] (ntot points each).  Returns spng_fn.
    ``stats``: 'too_wide' lists the skipped dimensions, 'max_exp_arg' as mth_stepf."""
    ndim = len(coords)
    ntot = coords[0].size
    spng_fn = np.zeros(ntot)                                   # call rzero(spng_fn, ntot)
    for il in range(ndim):
        if spng_wl[il] > 0.0 or spng_wr[il] > 0.0:
            xxmax = bmax[il] - spng_wr[il]                     # sponge beginning (rise at xmax; right)
            xxmin = bmin[il] + spng_wl[il]                     # end (drop at xmin; left)
            xxmax_c = xxmax + spng_dr[il]                      # beginning of constant part (right)
            xxmin_c = xxmin - spng_dl[il]                      # beginning of constant part (left)
            if xxmax <= xxmin:
                if stats is not None:
                    stats.setdefault("too_wide", []).append(il)   # write (6, *) 'Sponge too wide'
            else:
                lcoord = coords[il]
                out = np.empty(ntot)
                const_l = lcoord <= xxmin_c
                fall = ~const_l & (lcoord < xxmin)
                zero = ~const_l & ~fall & (lcoord <= xxmax)
                rise = ~const_l & ~fall & ~zero & (lcoord < xxmax_c)
                const_r = ~const_l & ~fall & ~zero & ~rise
                out[const_l] = 1.0
                out[zero] = 0.0
                out[const_r] = 1.0
                for jl in np.nonzero(fall)[0]:
                    arg = (xxmin - lcoord[jl]) / spng_wl[il]
                    out[jl] = mth_stepf(arg, stats)
                for jl in np.nonzero(rise)[0]:
                    arg = (lcoord[jl] - xxmax) / spng_wr[il]
                    out[jl] = mth_stepf(arg, stats)
                spng_fn = np.maximum(spng_fn, out)             # spng_fn(jl) = max(spng_fn(jl), rtmp)
    return spng_fn


def sponge_function(coords, bmin, bmax, lengths, acc_spg=0.333, stats=None):
    """spng_init's widths followed by spng_set."""
    return spng_set(coords, bmin, bmax, *spng_init(acc_spg, lengths, len(coords)), stats=stats)


def activate_sponge(bm1, spng_fn):
    """if (spng_fn(i) /= 0) bm1s(i) = 0, :102-104."""
    bm1s = bm1.copy()
    bm1s[spng_fn != 0] = 0.0
    return bm1s


def _zeros_like_rows(lay):
    return np.zeros(lay.rows)


def nekstab_forcing(lay, ff, v, fc=None, omega_t=0.0, fR_Re=None, fR_Im=None, spng_st=0.0, spng_fn=None,
                    spng_vr=None, jp=0):
    """nekStab_forcing (:2-52) at every point of the ldim velocity fields, then nekStab_forcing_temp (:54-79)
    at every point of the remaining weighted fields.  All vectors are ``lay.rows`` long (the device layout
    without the time slot); ``ff`` holds userf / userq on entry (zeros for a case without its own force) and
    is updated in place on the live rows only.  ``v``: vx.. / t (jp = 0) or vxp.. / tp (jp /= 0)."""
    n, sv = lay.n_v, lay.sv
    fc = _zeros_like_rows(lay) if fc is None else fc
    for c in range(lay.ldim):
        s = slice(c * sv, c * sv + n)
        f = ff[s]
        f = f + fc[s]                                                              # :14-16
        if omega_t != 0.0:                                                         # :19
            if omega_t > 0.0:                                                      # real part
                f = f + fR_Re[s] * math.cos(omega_t) - fR_Im[s] * math.sin(omega_t)
            else:                                                                  # imag part
                f = f + fR_Re[s] * math.sin(omega_t) + fR_Im[s] * math.cos(omega_t)
        if spng_st != 0:                                                           # :35
            if jp == 0:                                                            # dns
                f = f + spng_fn * (spng_vr[s] - v[s]) * spng_st
            else:                                                                  # perturbation
                f = f - spng_fn * v[s]
        ff[s] = f
    for m in range(lay.ldim, lay.n_wf):                                            # nekStab_forcing_temp
        s = slice(m * sv, m * sv + n)
        temp = ff[s]
        if jp == 0:
            temp = temp + fc[s]                                                    # :64
        if spng_st != 0:                                                           # :66
            if jp == 0:
                temp = temp + spng_fn * (spng_vr[s] - v[s])                        # :72
            else:
                temp = temp - spng_fn * v[s]                                       # :74
        ff[s] = temp
    return ff
