"""nkv_sponge_fn / nkv_body_force and the Sponge / BodyForce classes on the device against the line-for-line
restatement of core/forcing.f90 (tests/forcing_reference.py).

Gates:

1. ``fn`` against the restatement: identical wherever the restatement is exactly 0 or 1, the set ``fn != 0``
   identical, and on the ramps |fn_dev - fn_ref| <= (U_dev + U_host + 2) eps fn_ref.  Everything but ``exp`` is
   bit-identical IEEE arithmetic; ``exp`` enters as 1/(1 + E), so a relative error in E is at most that in fn;
   the 2 covers the add and the divide on each side.  U_dev = 3 (no ULP table ships with the HIP headers
   here; the OpenCL f64 bound for exp is 3 ulp), U_host = 1 (glibc's exp, which the restatement calls per
   point through ``math.exp``), as test_gpu_vortex.py gate 3 takes its cbrt bounds.  Condition, asserted: no
   test point has an exp argument within 1 of the f64 overflow threshold 709.78 (there the two sides could
   disagree on Inf, i.e. on ``fn != 0``).  Padding rows of fn are 0 (pre-filled with NaN).
2. After ``activate`` the context's weights are bit-identical to the restatement's bm1s, ``sponge.bm1`` is
   the untouched bm1 and k_norm of a vector supported only inside the sponge is exactly 0.
3. ``nkv_body_force`` on the device's own fn is bit-identical (``==``) to the restatement: each term alone and
   all together, DNS and perturbation, both harmonic branches, 2-D and 3-D, with scalars, accumulate in and
   out of place; pressure, padding and time of ff unchanged (sentinel).
4. Relaxation with the stepper v <- v + dt ff for 20 steps, bit-identical to the restatement stepped alike.
5. ``write_spg`` read back with oracle/nekio; two shards give the same data and the same fn bits as one.
6. Hygiene: argument checks, the empty shard, the PairLayout refusal.
"""
import functools
import math
from ctypes import c_double

import numpy as np
import pytest
import torch

import forcing_reference as fref
import nekio
from test_bf_sensitivity import _cyl, deformed_box
from test_forcing import BFS_CFG, bfs_mesh

from nekstab_next_amd import _lib, forcing
from nekstab_next_amd import synthetic as syn
from nekstab_next_amd.layout import NekLayout, pair_layout
from nekstab_next_amd.vector import NekContext, k_norm

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
U_DEV, U_HOST = 3, 1
SENTINEL = -12345.678
DT = 0.25


def _tiny_coords(lay):
    from seed_helpers import box_mesh_coords

    return box_mesh_coords(lay, (1, 1, 1))


# name -> (global layout, coordinates of the whole mesh, sponge parameters)
CASES = {
    "tiny3d": (NekLayout(3, 3, 1, 1), _tiny_coords,
               dict(xRspg=2.0, zLspg=0.5, spng_st=1.5)),   # x = 0: the right-only quirk, x = 1: on the rise
    "cyl": (NekLayout(2, 6, 4, 1996, n_scalars=1), lambda lay: _cyl(),
            dict(xLspg=4.0, xRspg=12.0, yLspg=3.0, yRspg=3.0, spng_st=2.0)),
    "box3d": (NekLayout(3, 5, 3, 12, n_scalars=2), lambda lay: deformed_box(lay, (3, 2, 2)),
              dict(xRspg=0.7, yLspg=0.3, zLspg=0.8, zRspg=0.5, spng_st=0.75)),
    "bfs": (NekLayout(2, 6, 4, 1670), lambda lay: bfs_mesh(), dict(BFS_CFG)),
}


def _lengths(par):
    return [(par.get("xLspg", 0.0), par.get("xRspg", 0.0)), (par.get("yLspg", 0.0), par.get("yRspg", 0.0)),
            (par.get("zLspg", 0.0), par.get("zRspg", 0.0))]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(layout, coords, weights, restated fn over the whole mesh, its stats): computed once, never modified."""
    lay, make, par = CASES[name]
    co = make(lay)
    keys = ("x", "y", "z")[: lay.ldim]
    assert lay.n_v == co["x"].size
    bmin, bmax = [float(co[k].min()) for k in keys], [float(co[k].max()) for k in keys]
    stats = {}
    fn = fref.sponge_function([co[k] for k in keys], bmin, bmax, _lengths(par)[: lay.ldim],
                              par.get("acc_spg", 0.333), stats=stats)
    fn.setflags(write=False)
    w = syn.mass_weights(lay)
    w.setflags(write=False)
    return lay, co, w, fn, stats, (bmin, bmax)


def _setup(name):
    lay, co, w, fn_ref, stats, _ = _reference(name)
    ctx = NekContext(lay, weights=np.array(w), max_cols=4)
    sp = forcing.Sponge(ctx, co, forcing.SpongeConfig(**CASES[name][2]))
    return ctx, sp, lay, co, w, fn_ref, stats


def _host(lay, seed):
    return syn.hash_vector(lay, seed)[:lay.rows].copy()


def _vector(ctx, seed):
    v = ctx.vector()
    v.fill_hash(seed)
    return v


def _live_mask(lay, weighted_only=True):
    m = np.zeros(lay.ld, dtype=bool)
    for nm, s, n in lay.field_slices():
        if nm != "pr" or not weighted_only:
            m[s:s + n] = True
    return m


# ---- 1. fn -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_fn_matches_restatement(gpu, name):
    ctx, sp, lay, co, w, fn_ref, stats = _setup(name)
    n = lay.n_v
    assert lay.sv > n                                           # there are padding rows to check
    assert stats.get("near_overflow", 0) == 0, stats            # the condition of the ramp bound
    sp.fn.fill_(float("nan"))
    sp.compute()
    got = sp.fn.cpu().numpy()
    assert got.size == lay.sv and not got[n:].any()             # padding rows: written, zero
    fn = got[:n]
    exact = (fn_ref == 0.0) | (fn_ref == 1.0)
    ramp = ~exact
    assert np.array_equal(fn[exact], fn_ref[exact])
    assert np.array_equal(fn != 0.0, fn_ref != 0.0)
    err = np.abs(fn[ramp] - fn_ref[ramp])
    worst = float(np.max(err / (EPS * fn_ref[ramp]))) if ramp.any() else 0.0
    print(f"{name}: {int(np.count_nonzero(fn_ref))} of {n} sponge points, {int(ramp.sum())} on a ramp, "
          f"{int(np.count_nonzero(fn_ref == 1.0))} at 1; largest exp argument {stats.get('max_exp_arg')}; "
          f"worst ramp error {worst:.2f} eps fn (bound {U_DEV + U_HOST + 2})")
    assert ramp.sum() > 0 and np.count_nonzero(fn_ref == 1.0) > 0
    assert np.count_nonzero(fn_ref == 0.0) > 0 or name == "tiny3d"   # three points per line: ends 1, middle ramp
    assert np.all(err <= (U_DEV + U_HOST + 2) * EPS * fn_ref[ramp])
    if name == "bfs":
        assert (np.count_nonzero(fn), np.count_nonzero(fn == 1.0)) == (3120, 1560)


# ---- 2. the masked weights ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_activate_masks_the_weights(gpu, name):
    ctx, sp, lay, co, w, fn_ref, _ = _setup(name)
    n = lay.n_v
    w_before = ctx.w.cpu().numpy().copy()
    sp.activate(ctx)
    got = ctx.w.cpu().numpy()
    assert np.array_equal(got[:n], fref.activate_sponge(np.asarray(w), fn_ref))
    assert np.array_equal(got[n:], w_before[n:])                # rows beyond n_v: untouched
    assert np.array_equal(sp.bm1.cpu().numpy(), w_before) and sp.bm1.data_ptr() != ctx.w.data_ptr()
    assert sp.volume == pytest.approx(float(np.sum(w)), rel=1e-13)
    # a vector supported only inside the sponge has norm exactly 0; one point outside is seen
    inside = (fn_ref != 0.0).astype(np.float64)
    fields = {nm: _host(lay, 70 + i)[s:s + k] * (inside if nm != "pr" else 1.0)
              for i, (nm, s, k) in enumerate(lay.field_slices())}
    v = ctx.vector().from_fields(fields)
    assert np.count_nonzero(v.to_packed()) > lay.n_wf * np.count_nonzero(inside) // 2
    assert k_norm(v) == 0.0
    outside = np.nonzero(fn_ref == 0.0)[0]
    if outside.size:                                            # (tiny3d has no point outside its sponge)
        j = int(outside[0])
        fields["vy"] = fields["vy"].copy()
        fields["vy"][j] = 2.0
        assert k_norm(v.from_fields(fields)) == pytest.approx(2.0 * math.sqrt(w[j]), rel=1e-14)


# ---- 3. the force ------------------------------------------------------------------------------------------

OMEGA = 0.9          # > 0: the real branch; -OMEGA: the imaginary one

# name -> (fc, harmonic omega_t or None, sponge, perturbation, accumulate: False | "in" | "out")
COMBOS = {
    "nothing": (False, None, False, False, False),
    "fc": (True, None, False, False, False),
    "fc_pert": (True, None, False, True, False),
    "harmonic_re": (False, OMEGA, False, False, False),
    "harmonic_im": (False, -OMEGA, False, False, False),
    "harmonic_zero": (False, 0.0, False, False, False),
    "sponge_dns": (False, None, True, False, False),
    "sponge_pert": (False, None, True, True, False),
    "all_dns_re": (True, OMEGA, True, False, False),
    "all_dns_im": (True, -OMEGA, True, False, False),
    "all_pert_re": (True, OMEGA, True, True, False),
    "all_pert_im": (True, -OMEGA, True, True, False),
    "all_dns_acc_in": (True, OMEGA, True, False, "in"),
    "all_pert_acc_in": (True, -OMEGA, True, True, "in"),
    "all_dns_acc_out": (True, -OMEGA, True, False, "out"),
    "sponge_pert_acc_out": (False, None, True, True, "out"),
}


@pytest.mark.parametrize("name", ["tiny3d", "cyl", "box3d"])
def test_body_force_is_bitwise_the_restatement(gpu, name):
    ctx, sp, lay, co, w, fn_ref, _ = _setup(name)
    n = lay.n_v
    fn_dev = sp.fn.cpu().numpy()[:n].copy()                     # the device's own fn
    v, fc, fre, fim, ref, f0 = (_vector(ctx, 200 + i) for i in range(6))
    hv, hfc, hre, him, href, h0 = (_host(lay, 200 + i) for i in range(6))
    sp.set_reference(ref)
    st = sp.cfg.spng_st
    bf_on, bf_off = forcing.BodyForce(ctx, sp), forcing.BodyForce(ctx, None)
    weighted = _live_mask(lay)
    for combo, (use_fc, omega, use_sp, pert, acc) in COMBOS.items():
        ff = ctx.vector()
        start = np.zeros(lay.ld)
        if acc == "in":
            ff.copy_from(f0, time=False)
            ff.time = 3.5
            start[:lay.rows] = h0
            start[lay.time_offset] = 3.5
        else:
            ff.storage.fill_(SENTINEL)
            start[:] = SENTINEL
        harmonic = None if omega is None else (fre, fim, omega)
        if acc == "out":                                         # ff0 a separate vector: the entry itself
            flags = (_lib.NKV_BF_PERTURBATION if pert else 0) | (_lib.NKV_BF_IMAG if (omega or 0.0) < 0 else 0)
            ctx.call("nkv_body_force", ff.ptr, f0.ptr, fc.ptr if use_fc else None, fre.ptr if omega else None,
                     fim.ptr if omega else None, math.cos(omega or 0.0), math.sin(omega or 0.0),
                     sp.fn.data_ptr() if use_sp else None, ref.ptr if (use_sp and not pert) else None, v.ptr, st,
                     lay.ldim, flags, ctx.stream)
        else:
            (bf_on if use_sp else bf_off).assemble(ff, v, fc=fc if use_fc else None, harmonic=harmonic,
                                                   perturbation=pert, accumulate=acc == "in")
        want = h0.copy() if acc else np.zeros(lay.rows)          # userf / userq, or the zero
        fref.nekstab_forcing(lay, want, hv, fc=hfc if use_fc else None, omega_t=omega or 0.0, fR_Re=hre, fR_Im=him,
                             spng_st=st if use_sp else 0.0, spng_fn=fn_dev, spng_vr=href, jp=1 if pert else 0)
        got = ff.to_packed()
        bad = int(np.count_nonzero(got[:lay.rows][weighted[:lay.rows]] != want[weighted[:lay.rows]]))
        assert bad == 0, (name, combo, bad)
        assert np.array_equal(got[~weighted], start[~weighted]), (name, combo)   # pressure, padding, time, tail
        if combo in ("nothing", "harmonic_zero"):
            assert not got[weighted].any()
        else:
            assert got[weighted].any(), combo
    ctx.synchronize()


# ---- 4. relaxation end to end ----------------------------------------------------------------------------------

def _step(v, ff, dt):
    """v <- v + dt ff as two roundings (a product, then a sum): no fused multiply-add."""
    tmp = ff.storage * dt
    v.storage += tmp


@pytest.mark.parametrize("pert", [True, False], ids=["perturbation", "dns"])
def test_relaxation(gpu, pert):
    ctx, sp, lay, co, w, fn_ref, _ = _setup("cyl")
    n, sv, st = lay.n_v, lay.sv, sp.cfg.spng_st
    fn_dev = sp.fn.cpu().numpy()[:n].copy()
    v, ref = _vector(ctx, 300), _vector(ctx, 301)
    hv, href = _host(lay, 300), _host(lay, 301)
    h0 = hv.copy()
    sp.set_reference(ref)
    bf = forcing.BodyForce(ctx, sp)
    ff = ctx.vector()
    for _ in range(20):
        bf.assemble(ff, v, perturbation=pert)
        _step(v, ff, DT)
        hf = fref.nekstab_forcing(lay, np.zeros(lay.rows), hv, spng_st=st, spng_fn=fn_dev, spng_vr=href,
                                  jp=1 if pert else 0)
        hv = hv + hf * DT
    got = v.to_packed()[:lay.rows]
    assert np.array_equal(got, hv)                              # bit-identical to the restatement stepped alike
    one, zero = fn_dev == 1.0, fn_dev == 0.0
    assert one.sum() > 0 and zero.sum() > 0
    for c in range(lay.n_wf):
        g, g0, r = got[c * sv:c * sv + n], h0[c * sv:c * sv + n], href[c * sv:c * sv + n]
        assert np.array_equal(g[zero], g0[zero])                # outside the sponge: untouched
        if pert:
            # v - dt v with dt = 1/4 is the correctly rounded 0.75 v: twenty exact-factor multiplications
            decay = g0[one].copy()
            for _ in range(20):
                decay = decay * (1.0 - DT)
            assert np.array_equal(g[one], decay)
            assert np.allclose(g[one], g0[one] * (1.0 - DT) ** 20, rtol=40 * EPS, atol=0.0)
        else:
            rate = (1.0 - DT * st) if c < lay.ldim else (1.0 - DT)     # the scalars carry no strength factor
            d0, d = np.abs(g0[one] - r[one]), np.abs(g[one] - r[one])
            assert np.all(d <= d0 * abs(rate) ** 20 + 64 * EPS * (np.abs(r[one]) + np.abs(g0[one])))
    assert np.array_equal(got[lay.n_wf * sv:], h0[lay.n_wf * sv:])   # the pressure never moves


# ---- 5. the SPG file and shards ----------------------------------------------------------------------------------

class _ShardComm:
    """Stand-in for comm.Comm of rank r of `world`, run one rank after the other: the extent reductions
    return the global extents of the mesh, the all-reduce leaves the local partial in place."""

    def __init__(self, rank, world, bmin, bmax):
        self.rank, self.world = rank, world
        self._min, self._max = list(bmin), list(bmax)

    def allreduce_(self, t):
        return t

    def min_scalar(self, x, device=None):
        return min(x, self._min.pop(0))

    def max_scalar(self, x, device=None):
        return max(x, self._max.pop(0))

    def raise_if_any(self, err):
        if err is not None:
            raise err

    def barrier(self):
        pass


def _shard_sponge(name, rank, world):
    glob, co, w, fn_ref, _, (bmin, bmax) = _reference(name)
    lay = glob.shard(rank, world)
    e0, e1 = lay.elem_range()
    sl = slice(e0 * lay.pts_v, e1 * lay.pts_v)
    ctx = NekContext(lay, weights=np.array(w)[sl], comm=_ShardComm(rank, world, bmin, bmax), max_cols=4)
    local = {k: a[sl] for k, a in co.items()}
    return ctx, forcing.Sponge(ctx, local, forcing.SpongeConfig(**CASES[name][2])), sl


def test_write_spg_and_two_shards(gpu, tmp_path):
    name = "box3d"
    ctx, sp, lay, co, w, fn_ref, _ = _setup(name)
    n = lay.n_v
    ref = _vector(ctx, 400)
    sp.set_reference(ref)
    one = tmp_path / "one"
    path = sp.write_spg(str(one), session="bfs", write_coords=True)
    assert path.endswith("SPGbfs0.f00001")
    tok, ids, fields = nekio.read_std(path)
    assert tok[11] == "XUT" and list(ids) == list(range(1, lay.nelgv + 1))
    fn_one = sp.fn.cpu().numpy()[:n]
    assert np.array_equal(fields["t"].reshape(-1), fn_one)
    href = _host(lay, 400)
    for c, nm in enumerate(("vx", "vy", "vz")):
        assert np.array_equal(fields[nm].reshape(-1), href[c * lay.sv:c * lay.sv + n])
        assert np.array_equal(fields["xyz"[c]].reshape(-1), co["xyz"[c]])
    assert "pr" not in fields
    # without a snapshot the velocity is zero; without coordinates there is no X group
    ctx0, sp0, *_ = _setup(name)
    tok0, _, f0 = nekio.read_std(sp0.write_spg(str(tmp_path / "bare"), session="bfs"))
    assert tok0[11] == "UT" and not f0["vx"].any() and np.array_equal(f0["t"].reshape(-1), fn_one)
    # two shards, one after the other
    two = tmp_path / "two"
    parts = {k: [] for k in ("t", "vx", "vy", "vz")}
    all_ids = []
    for rank in range(2):
        cx, sx, sl = _shard_sponge(name, rank, 2)
        assert np.array_equal(sx.fn.cpu().numpy()[:cx.layout.n_v], fn_one[sl])      # the same fn bits
        sx.activate(cx)
        assert np.array_equal(cx.w.cpu().numpy()[:cx.layout.n_v], fref.activate_sponge(np.asarray(w), fn_ref)[sl])
        r = cx.vector()
        r.fill_hash(400)                                        # shard-independent data
        sx.set_reference(r)
        p = sx.write_spg(str(two), session="bfs")
        assert p.endswith(f"SPGbfs{rank}.f00001")
        tk, idr, fr_ = nekio.read_std(p)
        assert (int(tk[9]), int(tk[10])) == (rank, 2)
        all_ids += list(idr)
        for k in parts:
            parts[k].append(fr_[k])
    assert all_ids == list(ids)
    for k in parts:
        assert np.array_equal(np.concatenate(parts[k]), fields[k]), k


# ---- 6. hygiene ------------------------------------------------------------------------------------------------------

def test_empty_shard(gpu):
    name = "tiny3d"                                             # one element, two ranks: rank 0 owns none
    ctx, sp, _ = _shard_sponge(name, 0, 2)
    lay = ctx.layout
    assert lay.n_v == 0 and lay.sv == 0
    assert [s.active for s in sp.sections] == [True, False, True]     # the extents came from the peers
    w0 = ctx.w.clone()
    sp.activate(ctx)
    assert torch.equal(ctx.w, w0) and not sp.fn.any() and sp.volume == float(w0.sum())
    v, ff = ctx.vector(), ctx.vector()
    ff.storage.fill_(SENTINEL)
    sp.set_reference(v)
    forcing.BodyForce(ctx, sp).assemble(ff, v, fc=v, harmonic=(v, v, 0.3))
    assert np.all(ff.to_packed() == SENTINEL)
    # and rank 1 holds the whole mesh
    ctx1, sp1, sl = _shard_sponge(name, 1, 2)
    assert np.array_equal(sp1.fn.cpu().numpy()[:ctx1.layout.n_v], _reference(name)[3])


def test_argument_checks(gpu):
    ctx, sp, lay, co, w, fn_ref, _ = _setup("cyl")
    vs = [ctx.vector() for _ in range(7)]
    ff, f0, fc, fre, fim, ref, v = (x.ptr for x in vs)
    fn = sp.fn.data_ptr()

    def call(ff=ff, f0=f0, fc=fc, fre=fre, fim=fim, fn=fn, ref=ref, v=v, n_vel=2, flags=0):
        return ctx.lib.nkv_body_force(ctx._Lp, ff, f0, fc, fre, fim, 0.5, 0.5, fn, ref, v, 1.0, n_vel, flags, ctx.stream)

    assert call() == _lib.NKV_OK
    assert call(ff=None) == _lib.NKV_EINVAL and "ff is NULL" in _lib.last_error()
    for n_vel in (1, 4, 3, 0, -1):                              # 3 > ldim + 0 velocities... n_wf = 3 here
        rc = call(n_vel=n_vel)
        if n_vel == 3:
            assert rc == _lib.NKV_OK                            # the scalar then counts as a velocity (as nkv_sfd_step)
        else:
            assert rc == _lib.NKV_EINVAL and "n_vel" in _lib.last_error()
    ctx2 = NekContext(NekLayout(2, 4, 2, 6), max_cols=4)
    x2 = [ctx2.vector() for _ in range(2)]
    assert ctx2.lib.nkv_body_force(ctx2._Lp, x2[0].ptr, None, x2[1].ptr, None, None, 0.0, 0.0, None, None, None, 0.0, 3,
                                   0, ctx2.stream) == _lib.NKV_EINVAL and "n_vel" in _lib.last_error()
    for kw in ("fc", "fre", "fim", "fn", "ref", "v"):           # ff may alias ff0 only
        assert call(**{kw: ff}) == _lib.NKV_EINVAL and "alias" in _lib.last_error(), kw
    assert call(f0=ff) == _lib.NKV_OK
    assert call(flags=_lib.NKV_BF_PERTURBATION, ref=ff) == _lib.NKV_OK      # ref is not read in perturbation mode
    assert call(fim=None) == _lib.NKV_EINVAL and "both or neither" in _lib.last_error()
    assert call(v=None) == _lib.NKV_EINVAL and "v is NULL" in _lib.last_error()
    assert call(ref=None) == _lib.NKV_EINVAL and "ref is NULL" in _lib.last_error()
    assert call(ref=None, flags=_lib.NKV_BF_PERTURBATION) == _lib.NKV_OK
    assert call(f0=None, fc=None, fre=None, fim=None, fn=None, ref=None, v=None) == _lib.NKV_OK
    # nkv_sponge_fn
    sec = (c_double * 18)(*([0.0] * 18))
    sec[0:6] = sp.sections[0].constants()
    x, y = sp.xyz[0].data_ptr(), sp.xyz[1].data_ptr()

    def spfn(ldim=2, x=x, y=y, z=None, sec=sec, active=1, fn=fn, w=None):
        return ctx.lib.nkv_sponge_fn(ctx._Lp, ldim, x, y, z, sec, active, fn, w, ctx.stream)

    assert spfn() == _lib.NKV_OK
    assert spfn(ldim=4) == _lib.NKV_EINVAL and "ldim" in _lib.last_error()
    assert spfn(sec=None) == _lib.NKV_EINVAL and "sections" in _lib.last_error()
    assert spfn(active=4) == _lib.NKV_EINVAL and "active" in _lib.last_error()
    assert spfn(fn=None) == _lib.NKV_EINVAL and "fn is NULL" in _lib.last_error()
    assert spfn(x=None) == _lib.NKV_EINVAL and "xm is NULL" in _lib.last_error()
    assert spfn(y=None) == _lib.NKV_OK                          # an inactive dimension is not read
    assert spfn(w=fn) == _lib.NKV_EINVAL and "alias" in _lib.last_error()
    wide = (c_double * 18)(*([0.0] * 18))
    wide[0:6] = (1.0, 2.0, 2.0, 3.0, 1.0, 1.0)                  # xxmax == xxmin
    assert spfn(sec=wide) == _lib.NKV_EINVAL and "too wide" in _lib.last_error()
    sp.compute()                                                # leave fn as it was
    ctx.synchronize()
    # the classes
    with pytest.raises(ValueError, match="set_reference"):
        forcing.BodyForce(ctx, forcing.Sponge(ctx, co, sp.cfg)).assemble(vs[0], vs[6])
    with pytest.raises(ValueError, match="n_v"):
        forcing.Sponge(ctx, {"x": co["x"][:-1], "y": co["y"][:-1]}, sp.cfg)
    with pytest.raises(ValueError, match="too wide"):
        forcing.Sponge(ctx, co, forcing.SpongeConfig(xLspg=1e3, spng_st=1.0))


def test_zero_strength_leaves_the_sponge_out(gpu):
    """spng_st == 0 (:35, :66): no sponge term, whatever fn holds."""
    lay, co, w, fn_ref, _, _ = _reference("tiny3d")
    ctx = NekContext(lay, weights=np.array(w), max_cols=4)
    par = dict(CASES["tiny3d"][2], spng_st=0.0)
    sp = forcing.Sponge(ctx, co, forcing.SpongeConfig(**par))
    assert sp.fn.any()
    v, fc, ff = _vector(ctx, 1), _vector(ctx, 2), ctx.vector()
    forcing.BodyForce(ctx, sp).assemble(ff, v, fc=fc)
    want = fref.nekstab_forcing(lay, np.zeros(lay.rows), _host(lay, 1), fc=_host(lay, 2))
    assert np.array_equal(ff.to_packed()[:lay.rows], want)


def test_pair_layout_is_refused(gpu):
    ctx = NekContext(pair_layout(NekLayout(2, 4, 2, 6)), max_cols=4)
    with pytest.raises(ValueError, match="PairLayout"):
        forcing.BodyForce(ctx)
    with pytest.raises(ValueError, match="PairLayout"):
        forcing.Sponge(ctx, {"x": np.zeros(ctx.layout.n_v), "y": np.zeros(ctx.layout.n_v)}, forcing.SpongeConfig())
