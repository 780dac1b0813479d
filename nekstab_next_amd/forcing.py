"""The sponge layer and the body-force assembly on the device (core/forcing.f90:2-251).

Two things hang on that file:

* ``activate_sponge`` (:82-115) builds the sponge function ``spng_fn`` (``spng_init`` / ``spng_set`` /
  ``mth_stepf``, :117-251) and zeroes the dot weights ``bm1s`` inside it: :class:`Sponge`, one streaming
  kernel (``nkv_sponge_fn``) for the function and the mask together;
* ``nekStab_forcing`` / ``nekStab_forcing_temp`` (:2-79) hand the time stepper, once per time step, the
  SFD / TDF forcing ``fc``, the harmonic resolvent forcing and the sponge term: :class:`BodyForce`, ONE
  streaming kernel (``nkv_body_force``) instead of more than 20 vector sweeps.

The host keeps the section constants, the phase of the harmonic forcing and the mode switches; all
arithmetic on fields is in the library (csrc/forcing.hip).  No CPU path.
"""
from __future__ import annotations

import math
import os
import warnings
from ctypes import c_double
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .fixedp import TWO_PI, _refuse_pair, _volume
from .vector import NekContext, NekVector


# ---- host logic (pure functions: tested without a GPU) ------------------------------------------

@dataclass
class SpongeConfig:
    """``xLspg .. zRspg``: the sponge lengths left / right per dimension, ``acc_spg``: the fraction of
    each taken by the drop / rise, ``spng_st``: the strength (0: no sponge).  Defaults: main.f90:40-47.
    ``abs()`` of ``acc_spg`` (:124) and ``spng_st`` (:95-97), as the reference applies them."""

    xLspg: float = 0.0
    xRspg: float = 0.0
    yLspg: float = 0.0
    yRspg: float = 0.0
    zLspg: float = 0.0
    zRspg: float = 0.0
    acc_spg: float = 0.333
    spng_st: float = 0.0

    def __post_init__(self):
        self.acc_spg = abs(float(self.acc_spg))
        self.spng_st = abs(float(self.spng_st))

    def lengths(self, ldim: int) -> list:
        return [(float(self.xLspg), float(self.xRspg)), (float(self.yLspg), float(self.yRspg)),
                (float(self.zLspg), float(self.zRspg))][:ldim]


@dataclass(frozen=True)
class SpongeSection:
    """One dimension of ``spng_set``: the four breakpoints (:192-195), the section widths ``wl, wr``
    (:126-132), the drop / rise widths ``dl, dr`` (:134-140) and ``active`` (``wl > 0 or wr > 0``, :186)."""

    xxmin_c: float
    xxmin: float
    xxmax: float
    xxmax_c: float
    wl: float
    wr: float
    dl: float
    dr: float
    active: bool

    def constants(self) -> tuple:
        return (self.xxmin_c, self.xxmin, self.xxmax, self.xxmax_c, self.wl, self.wr)


def sponge_sections(cfg: SpongeConfig, bmin, bmax, ldim: int) -> list:
    """The per-dimension constants of ``spng_init`` / ``spng_set`` in the reference's arithmetic order
    (:126-140, :192-195) for the global extents ``bmin``, ``bmax`` (Nek's xmn/xmx, ymn/ymx, zmn/zmx).
    An active dimension with ``xxmax <= xxmin`` raises ValueError (the reference prints "Sponge too wide"
    and skips the dimension, :198-199); ``wl < dl`` or ``wr < dr`` warns "Wrong sponge parameters!" and
    continues, as the reference does (:188-190)."""
    acc = cfg.acc_spg
    out = []
    for il, (left, right) in enumerate(cfg.lengths(ldim)):
        wl = (1.0 - acc) * left
        wr = (1.0 - acc) * right
        dl = acc * left
        dr = acc * right
        active = wl > 0.0 or wr > 0.0
        xxmax = float(bmax[il]) - wr
        xxmin = float(bmin[il]) + wl
        xxmax_c = xxmax + dr
        xxmin_c = xxmin - dl
        if active:
            if wl < dl or wr < dr:
                warnings.warn(f"Wrong sponge parameters! (dimension {il + 1}: section width below the drop width)")
            if xxmax <= xxmin:
                raise ValueError(f"Sponge too wide: dimension {il + 1} has xxmax={xxmax} <= xxmin={xxmin}")
        out.append(SpongeSection(xxmin_c, xxmin, xxmax, xxmax_c, wl, wr, dl, dr, active))
    return out


def harmonic_phase(time: float, fintim: float) -> tuple:
    """``(omega_t, cos(omega_t), sin(omega_t))`` with ``omega_t = (2 pi / fintim) time``
    (linear_operators.f90:241-245).  ``omega_t == 0`` (the first step) means no harmonic term."""
    omega_t = (TWO_PI / float(fintim)) * float(time)
    return omega_t, math.cos(omega_t), math.sin(omega_t)


# ---- device classes -------------------------------------------------------------------------------

class Sponge:
    """``spng_init`` + ``spng_set`` on this rank's points (:117-237): holds ``fn`` (one field of sv doubles)
    on the device.  ``coords``: this rank's GLL coordinates {"x", "y"[, "z"]} (host arrays of n_v values,
    the :class:`~.vortex.VortexCore` convention); the extents ``bmin`` / ``bmax`` are their global minima
    and maxima (``comm.min_scalar`` / ``max_scalar``: Nek's xmn/xmx).  Collective."""

    def __init__(self, ctx: NekContext, coords: dict, cfg: SpongeConfig):
        _refuse_pair(ctx, "Sponge")
        lay = ctx.layout
        self.ctx, self.cfg, self.coords = ctx, cfg, coords
        host = []
        for k in ("x", "y", "z")[: lay.ldim]:
            a = np.ascontiguousarray(coords[k], dtype=np.float64).reshape(-1)
            if a.size != lay.n_v:
                raise ValueError(f"coords[{k!r}]: {a.size} points, the layout has n_v={lay.n_v}")
            host.append(a)
        # every rank takes part in both reductions of every dimension (an empty shard offers -inf / +inf)
        self.bmin = [ctx.comm.min_scalar(float(a.min()) if a.size else math.inf, device=ctx.device) for a in host]
        self.bmax = [ctx.comm.max_scalar(float(a.max()) if a.size else -math.inf, device=ctx.device) for a in host]
        self.sections = sponge_sections(cfg, self.bmin, self.bmax, lay.ldim)
        self.xyz = [torch.as_tensor(a).to(ctx.device) if a.size else torch.zeros(2, dtype=torch.float64, device=ctx.device)
                    for a in host]
        self.fn = torch.zeros(max(lay.sv, 2), dtype=torch.float64, device=ctx.device)
        self.ref = None       # spng_vr / spng_vt: the snapshot of set_reference
        self.bm1 = None       # the unmasked weights, kept by activate
        self.volume = None    # their all-reduced sum (volvm1)
        self.compute()

    def compute(self, w: torch.Tensor | None = None) -> None:
        """One ``nkv_sponge_fn`` launch: writes ``fn`` (padding rows zero) and, given the weights ``w`` (sv
        doubles on the device), zeroes them where ``fn != 0``."""
        lay = self.ctx.layout
        w_ptr = None if w is None else w.data_ptr()
        sec = (c_double * 18)(*([0.0] * 18))
        active = 0
        for d, s in enumerate(self.sections):
            sec[6 * d: 6 * d + 6] = s.constants()
            active |= int(s.active) << d
        self.ctx.call("nkv_sponge_fn", lay.ldim, self.xyz[0].data_ptr(), self.xyz[1].data_ptr(),
                      self.xyz[2].data_ptr() if lay.ldim == 3 else None, sec, active, self.fn.data_ptr(), w_ptr,
                      self.ctx.stream)

    def set_reference(self, v: NekVector) -> None:
        """``spng_init``'s snapshot of the flow (:150-151), the target of the DNS-mode sponge.  The whole
        vector is kept: the reference copies only scalar 1 into ``spng_vt`` yet ``nekStab_forcing_temp``
        reads ``spng_vt(ip, m)`` for every m."""
        if self.ref is None:
            self.ref = self.ctx.vector()
        self.ref.copy_from(v, time=False)

    def activate(self, ctx: NekContext | None = None) -> None:
        """``activate_sponge``'s mask (:101-104): ``ctx.w`` is zeroed in place wherever ``fn != 0``, by the
        kernel that forms ``fn``.  ``sponge.bm1`` keeps a copy of the weights before masking and
        ``sponge.volume`` their all-reduced sum (``volvm1``: pass it as ``SFD(volume=...)``)."""
        ctx = self.ctx if ctx is None else ctx
        if ctx.layout.n_v != self.ctx.layout.n_v or ctx.layout.sv != self.ctx.layout.sv:
            raise ValueError("activate: the context's shard differs from the sponge's")
        self.bm1 = ctx.w.clone()
        self.volume = _volume(ctx)
        self.compute(ctx.w)

    def write_spg(self, outdir: str = ".", session: str = "nek", write_coords: bool = False, time: float = 0.0,
                  istep: int = 0) -> str:
        """The ``SPG<session>0.f00001`` set of :231-234: the reference snapshot as the velocity (zeros before
        ``set_reference``), ``fn`` as the temperature, no pressure.  Collective."""
        from . import fld
        from .vortex import _empty_file, _put_velocity

        lay = self.ctx.layout
        with fld.collective_output(self.ctx.comm) as write:
            write(os.makedirs, outdir, exist_ok=True)
            f = _empty_file(lay, time, istep)
            if write_coords:
                f.fields.update({k: np.asarray(self.coords[k], dtype=np.float64).reshape(lay.nelv, lay.pts_v)
                                 for k in ("x", "y", "z")[: lay.ldim]})
                f.rdcode += "X"
            rows = [] if self.ref is None else [self.ref.storage[c * lay.sv:] for c in range(lay.ldim)]
            _put_velocity(lay, f, rows)
            f.fields["t"] = self.fn[: lay.n_v].cpu().numpy().reshape(lay.nelv, lay.pts_v)
            f.rdcode += "T"
            path = os.path.join(outdir, fld.fld_name("SPG", session, lay.rank, 1))
            write(fld.write_fld, path, f)
        return path


class BodyForce:
    """``nekStab_forcing`` + ``nekStab_forcing_temp`` (:2-79) for the flow or perturbation held in a
    :class:`NekVector`.  ``sponge``: a :class:`Sponge`; its term is added when its strength is not zero
    (``spng_st /= 0``, :35, :66)."""

    def __init__(self, ctx: NekContext, sponge: Sponge | None = None):
        _refuse_pair(ctx, "BodyForce")
        self.ctx, self.sponge = ctx, sponge
        self.n_vel = ctx.layout.ldim

    def assemble(self, ff: NekVector, v: NekVector, fc: NekVector | None = None, harmonic=None,
                 perturbation: bool = False, accumulate: bool = False) -> None:
        """One ``nkv_body_force`` call: the weighted fields of ``ff`` receive the force on the flow (or, with
        ``perturbation``, on the perturbation, jp /= 0) ``v``.  ``fc``: the SFD / TDF forcing.
        ``harmonic``: ``(f_re, f_im, omega_t)``; the sign of ``omega_t`` picks the real (> 0) or the
        imaginary (< 0) branch and 0 leaves the term out (:19-33; :func:`harmonic_phase`).  ``accumulate``:
        start from the present content of ``ff`` (the case's own ``userf`` / ``userq``) instead of zero."""
        flags = _lib.NKV_BF_PERTURBATION if perturbation else 0
        f_re = f_im = None
        c = s = 0.0
        if harmonic is not None:
            h_re, h_im, omega_t = harmonic
            omega_t = float(omega_t)
            if omega_t != 0.0:
                f_re, f_im = h_re.ptr, h_im.ptr
                c, s = math.cos(omega_t), math.sin(omega_t)
                if omega_t < 0.0:
                    flags |= _lib.NKV_BF_IMAG
        fn = ref = None
        st = 0.0
        sp = self.sponge
        if sp is not None and sp.cfg.spng_st != 0.0:
            fn, st = sp.fn.data_ptr(), sp.cfg.spng_st
            if not perturbation:
                if sp.ref is None:
                    raise ValueError("BodyForce.assemble: the DNS-mode sponge needs Sponge.set_reference first")
                ref = sp.ref.ptr
        self.ctx.call("nkv_body_force", ff.ptr, ff.ptr if accumulate else None, None if fc is None else fc.ptr,
                      f_re, f_im, c, s, fn, ref, v.ptr, st, self.n_vel, flags, self.ctx.stream)


__all__ = ["SpongeConfig", "SpongeSection", "sponge_sections", "harmonic_phase", "Sponge", "BodyForce"]
