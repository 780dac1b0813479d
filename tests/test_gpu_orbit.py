"""The time-periodic Burgers flow on the device (nkv_burgers_tangent_rhs, nkv_orbit_stage in csrc/advdiff.hip;
nekstab_next_amd/orbit.py) against its NumPy restatement (tests/orbit_reference.py), and the workflow it is there
for: Newton for a forced periodic orbit, then its Floquet multipliers, their adjoint and the intracycle growth.

"The gate" is test_gpu_burgers.py's: with e_ref = max |f64 - long double| of the restatement, the device is held
to max(8 e_ref, 1e-12 max|ref|).  The fused right-hand side against the two kernels it restates, nkv_orbit_stage
against its NumPy expression and nkv_rk4_stage, the two storage modes, repeated calls, element sub-ranges and
shards are compared bit for bit."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import advdiff_reference as ar
import burgers_reference as br
import orbit_reference as orf
import test_gpu_advdiff as ga
import test_gpu_burgers as gb

from nekstab_next_amd import _lib
from nekstab_next_amd.layout import NekLayout

ROOT = ga.ROOT
pytestmark = pytest.mark.gpu

E2E = "orbit-e2e"
E2E_LAY = dict(ldim=2, lx1=5, lx2=3, nelgv=4)
NSTEPS = 3


def _nan(count):
    return torch.full((count,), float("nan"), dtype=torch.float64, device="cuda")


# ---- nkv_burgers_tangent_rhs -------------------------------------------------------------------------
class _Raw(gb._Raw):
    def fused(self, u, u_stride, rB, rB_stride, ru, ru_stride, kappa, e0=0, e1=None):
        """nkv_burgers_tangent_rhs on elements [e0, e1): every per-point pointer moved by e0 elements."""
        lay = self.lay
        e1 = self.n // self.pts if e1 is None else e1
        L = lay.c_struct()
        L.n_v = (e1 - e0) * self.pts
        off = 8 * e0 * self.pts
        xyz = [t.data_ptr() + off for t in self.xyz] + ([None] if lay.ldim == 2 else [])
        rc = self.ctx.lib.nkv_burgers_tangent_rhs(ctypes.byref(L), lay.lx1, lay.ldim, self.D.data_ptr(), self.w.data_ptr(),
                                                  *xyz, self.B.data_ptr() + off, self.n, kappa.data_ptr(),
                                                  u.data_ptr() + off, lay.n_wf, u_stride, rB.data_ptr() + off, rB_stride,
                                                  ru.data_ptr() + off, ru_stride, self.st)
        assert rc == _lib.NKV_OK, _lib.last_error()


@pytest.mark.parametrize("name", ["cyl"] + gb.CASES_3D, ids=str)
def test_fused_rhs_equals_the_two_kernels(gpu, name):
    """r_B carries the bits of nkv_advdiff_rhs(u = B, U = B), r_u those of the forward nkv_linconv_rhs; output
    strides above n_v leave the NaN gap untouched; a second call and element sub-ranges give the same bits."""
    raw = _Raw(name)
    lay, n, pts = raw.lay, raw.n, raw.pts
    nf = lay.n_wf
    fields = ga._fields(lay, raw.co)
    su, sb, sr = n + 24, n + 8, n + 40
    u = _nan(nf * su)
    for f in range(nf):
        u[f * su: f * su + n] = ga._dev(fields[f])
    kd = ga._dev(raw.kap)
    E = n // pts
    wantB, wantu = _nan(nf * sb), _nan(nf * sr)
    raw.rhs(raw.B, nf, n, wantB, sb, kd, False, U=raw.B, U_stride=n)
    raw.lin(u, su, wantu, sr, kd, False)
    wB, wu = wantB.cpu().numpy().reshape(nf, sb), wantu.cpu().numpy().reshape(nf, sr)
    assert np.all(np.isfinite(wB[:, :n])) and np.all(np.isfinite(wu[:, :n])) and np.any(wB[:, :n] != 0.0)
    rB, ru = _nan(nf * sb), _nan(nf * sr)
    raw.fused(u, su, rB, sb, ru, sr, kd)
    gB, gu = rB.cpu().numpy().reshape(nf, sb), ru.cpu().numpy().reshape(nf, sr)
    print(f"{name}: max |r_B - advdiff| {np.max(np.abs(gB[:, :n] - wB[:, :n])):.2e}, "
          f"max |r_u - linconv| {np.max(np.abs(gu[:, :n] - wu[:, :n])):.2e}")
    assert np.array_equal(gB[:, :n], wB[:, :n])
    assert np.array_equal(gu[:, :n], wu[:, :n])
    assert np.all(np.isnan(gB[:, n:])) and np.all(np.isnan(gu[:, n:]))       # the gaps are untouched
    aB, au = _nan(nf * sb), _nan(nf * sr)
    raw.fused(u, su, aB, sb, au, sr, kd)
    assert np.array_equal(aB.cpu().numpy().reshape(nf, sb)[:, :n], gB[:, :n])
    assert np.array_equal(au.cpu().numpy().reshape(nf, sr)[:, :n], gu[:, :n])
    for e0, e1 in {(0, max(E // 2, 1)), (E // 2, E), (E - 1, E)}:
        pB, pu = _nan(nf * sb), _nan(nf * sr)
        raw.fused(u, su, pB, sb, pu, sr, kd, e0, e1)
        for part, got, s in ((pB, gB, sb), (pu, gu, sr)):
            p = part.cpu().numpy().reshape(nf, s)
            assert np.array_equal(p[:, e0 * pts:e1 * pts], got[:, e0 * pts:e1 * pts])
            assert np.all(np.isnan(p[:, :e0 * pts])) and np.all(np.isnan(p[:, e1 * pts:]))


def test_entry_checks(gpu):
    """Every NKV_EINVAL of nkv_burgers_tangent_rhs and nkv_orbit_stage with its message, nothing launched; an empty
    shard returns NKV_OK and reads no pointer."""
    lay = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=3, n_scalars=1)
    n, nf = lay.n_v, lay.n_wf
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.full((24 * n,), 7.0, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    L = lay.c_struct()
    u, B, rB, ru = p + 8 * 4 * n, p + 8 * 8 * n, p + 8 * 12 * n, p + 8 * 16 * n
    far = 8 * (nf - 1) * n + 8 * (n - 1)
    V = dict(L=ctypes.byref(L), lx1=4, ldim=3, D=p, w=p, xm=p, ym=p, zm=p, B=B, B_stride=n, kappa=p, u=u, nfld=nf,
             u_stride=n, r_B=rB, rB_stride=n, r_u=ru, ru_stride=n, stream=st)
    bad = [("ldim", 4, "ldim"), ("lx1", 11, "lx1"), ("zm", None, "zm"), ("u_stride", n - 1, "stride"),
           ("B_stride", n - 1, "stride"), ("rB_stride", n - 1, "stride"), ("ru_stride", n - 1, "stride"),
           ("nfld", 2, "nfld=2 < ldim=3"), ("D", None, "D is NULL"), ("w", None, "w is NULL"), ("xm", None, "xm is NULL"),
           ("ym", None, "ym is NULL"), ("B", None, "B is NULL"), ("u", None, "u is NULL"), ("kappa", None, "kappa is NULL"),
           ("r_B", None, "r_B is NULL"), ("r_u", None, "r_u is NULL"),
           ("r_u", rB, "r_B overlaps r_u"), ("r_u", rB + far, "r_B overlaps r_u"), ("r_B", ru - far, "r_B overlaps r_u"),
           ("r_B", u, "r_B overlaps u or B"), ("r_B", u + far, "r_B overlaps u or B"), ("r_B", B - far, "r_B overlaps u or B"),
           ("r_u", u - far, "r_u overlaps u or B"), ("r_u", B, "r_u overlaps u or B"), ("r_u", B - far, "r_u overlaps u or B"),
           ("r_u", B + far, "r_B overlaps r_u")]
    for key, val, msg in bad:
        assert lib.nkv_burgers_tangent_rhs(*{**V, key: val}.values()) == _lib.NKV_EINVAL, key
        assert "burgers_tangent_rhs" in _lib.last_error() and msg in _lib.last_error(), (key, _lib.last_error())
    a = [p + 8 * 2 * k * n for k in range(12)]                       # twelve disjoint spans of 2 n
    S = dict(L=ctypes.byref(L), minv=a[0], v=a[1], v_stride=n, r=a[2], r_stride=n, g0=None, gc=None, gs=None, g_stride=n,
             c=0.5, s=0.5, a=0.5, b=0.25, first=1, acc=None, acc_stride=n, w=a[3], w_stride=n, acc_out=a[4], ao_stride=n,
             tv=a[5], tv_stride=n, tr=a[6], tr_stride=n, tacc=None, tacc_stride=n, tw=a[7], tw_stride=n, tacc_out=a[8],
             tao_stride=n, nfld=1, zero_rest=0, stream=st)
    none = dict(tv=None, tr=None, tw=None, tacc_out=None)
    cases = [dict(v_stride=n - 1), dict(r_stride=n - 1), dict(w_stride=n - 1), dict(ao_stride=n - 1), dict(tv_stride=n - 1),
             dict(tr_stride=n - 1), dict(tw_stride=n - 1), dict(tao_stride=n - 1), dict(g0=a[9], g_stride=n - 1),
             dict(gc=a[9], g_stride=n - 1), dict(gs=a[9], g_stride=n - 1), dict(minv=None), dict(r=None), dict(acc_out=None),
             dict(tacc_out=None), dict(tr=None), dict(nfld=0), dict(a=float("nan")), dict(b=float("inf")),
             dict(c=float("nan")), dict(s=float("inf")), dict(zero_rest=1), dict(zero_rest=2), dict(zero_rest=4),
             dict(none, zero_rest=2), dict(first=0), dict(first=0, acc=a[9]), dict(w=a[4]), dict(w=a[1]), dict(acc_out=a[0]),
             dict(acc_out=a[2]), dict(gc=a[4]), dict(tw=a[4]), dict(tacc_out=a[3]), dict(tacc_out=a[1]), dict(acc_out=a[5]),
             dict(tw=a[6]), dict(tacc_out=a[8] - 8 * (n - 1), tw=a[8])]
    for case in cases:
        assert lib.nkv_orbit_stage(*{**S, **case}.values()) == _lib.NKV_EINVAL, case
        assert "orbit_stage" in _lib.last_error(), (case, _lib.last_error())
    torch.cuda.synchronize()
    assert torch.all(buf == 7.0)                                     # nothing was launched
    Le = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=0, n_scalars=1).c_struct()
    assert lib.nkv_burgers_tangent_rhs(*{**V, "L": ctypes.byref(Le), "D": None, "B": None, "u": None, "r_B": None,
                                         "r_u": None}.values()) == _lib.NKV_OK
    assert lib.nkv_orbit_stage(*{**S, "L": ctypes.byref(Le), "minv": None, "r": None, "v": None, "acc_out": None}.values()) \
        == _lib.NKV_OK
    # what the checks allow: acc_out on the acc or the v of its own half
    assert lib.nkv_orbit_stage(*{**S, "acc_out": a[1], "tacc_out": a[5]}.values()) == _lib.NKV_OK
    assert lib.nkv_orbit_stage(*{**S, "first": 0, "acc": a[4], "tacc": a[8]}.values()) == _lib.NKV_OK
    torch.cuda.synchronize()


# ---- nkv_orbit_stage ---------------------------------------------------------------------------------
def _stage_numpy(v, m, r, g0, gc, gs, c, s, a, b, first, acc):
    k = m * r
    if g0 is not None:
        k = k + g0
    if gc is not None:
        k = k + c * gc
    if gs is not None:
        k = k + s * gs
    return v + a * k, (v if first else acc) + b * k


@pytest.mark.parametrize("lay", [NekLayout(ldim=3, lx1=4, lx2=2, nelgv=5, n_scalars=1), NekLayout(ldim=2, lx1=3, lx2=1, nelgv=9)],
                         ids=["3d-n320", "2d-n81"])
def test_orbit_stage_bits(gpu, lay):
    """nkv_orbit_stage equals the NumPy expression bit for bit: even strides from aligned bases (the 16-byte path;
    with n_v = 81 its odd last point) and odd strides (the scalar path); every combination of g0 / gc / gs, with
    and without the tangent half, first or not; the NaN gaps stay NaN.  With gc = gs = NULL and no tangent half:
    the bits of nkv_rk4_stage.  zero_rest bit by bit on state vectors."""
    from nekstab_next_amd.vector import NekContext

    ctx = NekContext(lay, max_cols=4)
    lib = ctx.lib
    n, nf = lay.n_v, lay.n_wf
    assert (n % 2 == 1) == (lay.ldim == 2)
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)
    m = rng.uniform(0.5, 2.0, n)
    md = ga._dev(m)
    a, b = 0.05 / 2, 0.05 / 3
    c, s = orf.phase(1, 0.5, 20)
    L = lay.c_struct()

    def packed(rows, stride):
        h = np.full(nf * stride, np.nan)
        for f in range(nf):
            h[f * stride: f * stride + n] = rows[f]
        return ga._dev(h)

    def rows(t, stride):
        return t.cpu().numpy().reshape(nf, stride)

    for stride in (n + 7 + (n + 7) % 2, n + 6 + (n + 7) % 2):           # even, then odd
        H = {k: rng.standard_normal((nf, n)) for k in ("v", "r", "g0", "gc", "gs", "acc", "tv", "tr", "tacc")}
        Dv = {k: packed(t, stride) for k, t in H.items()}
        P = {k: t.data_ptr() for k, t in Dv.items()}
        for (w0, wc, ws), tan, first in itertools.product(itertools.product((False, True), repeat=3), (False, True),
                                                          (False, True)):
            wd, od, twd, tod = (_nan(nf * stride) for _ in range(4))
            rc = lib.nkv_orbit_stage(ctypes.byref(L), md.data_ptr(), P["v"], stride, P["r"], stride, P["g0"] if w0 else None,
                                     P["gc"] if wc else None, P["gs"] if ws else None, stride, c, s, a, b, int(first), P["acc"],
                                     stride, wd.data_ptr(), stride, od.data_ptr(), stride,
                                     P["tv"] if tan else None, stride, P["tr"] if tan else None, stride,
                                     P["tacc"] if tan else None, stride, twd.data_ptr() if tan else None, stride,
                                     tod.data_ptr() if tan else None, stride, nf, 0, st)
            assert rc == _lib.NKV_OK, _lib.last_error()
            what = (stride, w0, wc, ws, tan, first)
            ww, oo = _stage_numpy(H["v"], m, H["r"], H["g0"] if w0 else None, H["gc"] if wc else None,
                                  H["gs"] if ws else None, c, s, a, b, first, H["acc"])
            for got, want in ((wd, ww), (od, oo)):
                g = rows(got, stride)
                assert np.array_equal(g[:, :n], want), what
                assert np.all(np.isnan(g[:, n:])), what
            if tan:
                tw, to = _stage_numpy(H["tv"], m, H["tr"], None, None, None, c, s, a, b, first, H["tacc"])
                for got, want in ((twd, tw), (tod, to)):
                    g = rows(got, stride)
                    assert np.array_equal(g[:, :n], want), what
                    assert np.all(np.isnan(g[:, n:])), what
            else:
                assert np.all(np.isnan(rows(twd, stride))) and np.all(np.isnan(rows(tod, stride))), what
            if not (wc or ws or tan):                                   # the bits of nkv_rk4_stage
                w2, o2 = _nan(nf * stride), _nan(nf * stride)
                rc = lib.nkv_rk4_stage(ctypes.byref(L), P["v"], stride, md.data_ptr(), P["r"], stride,
                                       P["g0"] if w0 else None, stride, a, b, int(first), P["acc"], stride, w2.data_ptr(),
                                       stride, o2.data_ptr(), stride, nf, 0, st)
                assert rc == _lib.NKV_OK, _lib.last_error()
                assert np.array_equal(rows(w2, stride)[:, :n], rows(wd, stride)[:, :n]), what
                assert np.array_equal(rows(o2, stride)[:, :n], rows(od, stride)[:, :n]), what
        # v = NULL and w = NULL on both halves (a last stage), acc' in place
        ac, tac = Dv["acc"].clone(), Dv["tacc"].clone()
        rc = lib.nkv_orbit_stage(ctypes.byref(L), md.data_ptr(), None, stride, P["r"], stride, P["g0"], P["gc"], P["gs"],
                                 stride, c, s, 0.0, b, 0, ac.data_ptr(), stride, None, stride, ac.data_ptr(), stride, None,
                                 stride, P["tr"], stride, tac.data_ptr(), stride, None, stride, tac.data_ptr(), stride, nf,
                                 0, st)
        assert rc == _lib.NKV_OK, _lib.last_error()
        assert np.array_equal(rows(ac, stride)[:, :n],
                              _stage_numpy(0.0, m, H["r"], H["g0"], H["gc"], H["gs"], c, s, 0.0, b, False, H["acc"])[1])
        assert np.array_equal(rows(tac, stride)[:, :n],
                              _stage_numpy(0.0, m, H["tr"], None, None, None, c, s, 0.0, b, False, H["tacc"])[1])
    # the last stage into state vectors: bit 0 the base half's, bit 1 the tangent half's
    sv = lay.sv
    H = {k: rng.standard_normal((nf, n)) for k in ("r", "gc", "acc", "tr", "tacc")}
    P = {k: packed(t, sv) for k, t in H.items()}
    for bits in (1, 2, 3):
        y, ty = ga._sentinel(ctx), ga._sentinel(ctx)
        rc = lib.nkv_orbit_stage(ctypes.byref(L), md.data_ptr(), None, sv, P["r"].data_ptr(), sv, None, P["gc"].data_ptr(),
                                 None, sv, c, s, 0.0, b, 0, P["acc"].data_ptr(), sv, None, sv, y.ptr, sv, None, sv,
                                 P["tr"].data_ptr(), sv, P["tacc"].data_ptr(), sv, None, sv, ty.ptr, sv, nf, bits, st)
        assert rc == _lib.NKV_OK, _lib.last_error()
        for bit, vec, want in ((1, y, _stage_numpy(0.0, m, H["r"], None, H["gc"], None, c, s, 0.0, b, False, H["acc"])[1]),
                               (2, ty, _stage_numpy(0.0, m, H["tr"], None, None, None, c, s, 0.0, b, False, H["tacc"])[1])):
            got = vec.to_packed()
            assert np.array_equal(gb._rows(lay, got), want)
            if bits & bit:
                ga._check_rest(lay, got)
            else:
                assert np.all(got[nf * sv:] == 7.0)


# ---- the operators -----------------------------------------------------------------------------------
_OPS, _E2E = {}, {}


def _e2e():
    """The end-to-end case in f64 and long double, the f64 dense Newton from Pi target and the dense monodromy
    about what it found (built once)."""
    if not _E2E:
        c64, cld = orf.e2e_case(np.float64), orf.e2e_case(np.longdouble)
        ob = c64[2]
        q, hist = ob.newton(c64[3])
        orbit = ob.propagate(q)[1]
        _E2E.update(c64=c64, cld=cld, q=q, hist=hist, orbit=orbit, P=ob.monodromy(orbit))
    return _E2E


def _setup(name):
    """(ctx weighted by bm1, ViscousBurgers, OrbitFlow stored, OrbitFlow side by side, restatements, a state) of a
    case over NSTEPS steps with all three forcing parts set, built once."""
    if name not in _OPS:
        from nekstab_next_amd.burgers import ViscousBurgers
        from nekstab_next_amd.orbit import OrbitFlow
        from nekstab_next_amd.vector import NekContext

        if name == E2E:
            co, mask = orf.e2e_mesh()
            lay = NekLayout(**E2E_LAY)
            kap, dt = list(orf.E2E["kappa"]), orf.E2E["dt"]
            target, gc, gs = orf.e2e_forcing(co)
            g0 = None
        else:
            lay, co, _, mask, kap = gb._case(name)
            r64 = ga._refs(name)[0]
            dt = 1.5 / max(float(np.max(np.abs(np.linalg.eigvals(r64.dense(k))))) for k in kap)
            x, y, z = co["x"], co["y"], co["z"]
            g0 = np.stack([0.3 * np.sin(x + 0.2 * f) * np.cos(y) for f in range(lay.n_wf)])
            gc = np.stack([0.2 * np.cos(x) * np.sin(y + 0.1 * f) * (1.0 + 0.2 * z) for f in range(lay.n_wf)])
            gs = np.stack([0.1 * np.sin(2.0 * x + z) * np.cos(y - 0.3 * f) for f in range(lay.n_wf)])
        zero = [np.zeros(lay.n_v)] * lay.ldim
        obs = tuple(orf.Orbit(br.Burgers(ar.Reference(lay.lx1, lay.ldim, co, zero, mask=mask, dtype=t), kap, dt, NSTEPS),
                              g0=g0, gc=gc, gs=gs) for t in (np.float64, np.longdouble))
        ctx0 = NekContext(lay, max_cols=4)
        flow = ViscousBurgers(ctx0, co, kap, dt, NSTEPS, forcing=None if g0 is None else list(g0), mask=mask)
        if name == E2E:
            flow.steady_forcing(list(target))
            for ob in obs:
                ob.steady_g0(target)
        of = OrbitFlow(flow, cos=list(gc), sin=list(gs))
        sbs = OrbitFlow(flow, cos=list(gc), sin=list(gs), store=False)
        ctx = NekContext(lay, weights=flow.bm1, max_cols=32)
        q = np.stack(ga._fields(lay, co, seed=4))
        _OPS[name] = (ctx, flow, of, sbs, obs, q)
    return _OPS[name]


_CASES = [E2E, (5, (2, 2, 2))]


@pytest.mark.parametrize("name", _CASES, ids=str)
def test_flow_against_restatement(gpu, name):
    """OrbitFlow.propagate over 3 steps and every stored stage state against the restatement under the gate;
    pressure and time zeroed, padding untouched, deterministic; the two storage modes give the same bits; without
    cos and sin parts the bits of ViscousBurgers.propagate; time_derivative under the gate."""
    from nekstab_next_amd.orbit import OrbitFlow

    ctx, flow, of, sbs, (o64, old), q = _setup(name)
    lay = ctx.layout
    n, sv, nf = lay.n_v, lay.sv, lay.n_wf
    assert of.orbit_bytes == 4 * NSTEPS * nf * sv * 8 and sbs.orbit_bytes == 4 * nf * sv * 8
    x = gb._vector(ctx, q)
    y = ga._sentinel(ctx)
    of.propagate(x, y)
    got = y.to_packed()
    ga._check_rest(lay, got)
    (p64, orb64), (pld, orbld) = o64.propagate(q), old.propagate(q)
    gb._gate_rows(gb._rows(lay, got), p64, pld, f"{name} Phi_T")
    stages = of._orbit[: 4 * NSTEPS * nf * sv].cpu().numpy().reshape(NSTEPS, 4, nf, sv)[..., :n]
    for k in range(NSTEPS):
        for i in range(4):
            gb._gate_rows(stages[k, i], orb64[k][i], orbld[k][i], f"{name} step {k} stage {i + 1}")
    y2 = ga._sentinel(ctx)
    of.propagate(x, y2)
    assert torch.equal(y.storage, y2.storage)
    y3 = ga._sentinel(ctx)
    sbs.propagate(x, y3)
    assert torch.equal(y.storage, y3.storage)
    # the harmonic parts are in
    plain = OrbitFlow(flow)
    y4, y5 = ga._sentinel(ctx), ga._sentinel(ctx)
    plain.propagate(x, y4)
    flow.propagate(x, y5)
    assert torch.equal(y4.storage, y5.storage) and not torch.equal(y4.storage, y.storage)
    # compute_bvec at a step with cos and sin both away from 0 and 1
    b = ga._sentinel(ctx)
    of.time_derivative(x, b, step=1)
    gb._gate_rows(gb._rows(lay, b.to_packed()), o64.time_derivative(q, 1), old.time_derivative(q, 1), f"{name} bvec")
    assert b.time == 0.0 and np.all(b.to_packed()[nf * sv: nf * sv + lay.n_p] == 0.0)
    assert np.array_equal(                                            # (time_derivative left the orbit alone)
        of._orbit[: 4 * NSTEPS * nf * sv].cpu().numpy().reshape(NSTEPS, 4, nf, sv)[..., :n], stages)


@pytest.mark.parametrize("name", _CASES, ids=str)
def test_propagator_against_restatement(gpu, name):
    """OrbitPropagator.matvec / rmatvec over 3 steps against the restatement's tangent and adjoint under the gate
    (pressure and time zeroed, padding untouched, deterministic); matvec side by side gives the bits of matvec about
    the stored orbit, and its rmatvec raises; the adjoint defect |<A x, y> - <x, A^+ y>| / sum bm1 |A x| |y| for
    unprojected hash vectors within 4 times the restatement's own f64 defect (floor 1e-12)."""
    ctx, flow, of, sbs, (o64, old), q = _setup(name)
    lay = ctx.layout
    qv = gb._vector(ctx, q)
    fields = np.stack(ga._fields(lay, gb._case(name)[1] if name != E2E else orf.e2e_mesh()[0], seed=9))
    x = gb._vector(ctx, fields)
    op = of.linearized(qv)
    assert op is of.prop and of.linearized(qv) is op
    orb64, orbld = o64.propagate(q)[1], old.propagate(q)[1]
    for what, apply, ref in (("tangent", op.matvec, "tangent"), ("adjoint", op.rmatvec, "adjoint")):
        y = ga._sentinel(ctx)
        apply(x, y)
        got = y.to_packed()
        ga._check_rest(lay, got)
        gb._gate_rows(gb._rows(lay, got), getattr(o64, ref)(fields, orb64), getattr(old, ref)(fields, orbld),
                      f"{name} {what}")
        y2 = ga._sentinel(ctx)
        apply(x, y2)
        assert torch.equal(y.storage, y2.storage)
        if what == "tangent":
            mv = y
    ops = sbs.linearized(qv)
    y3 = ga._sentinel(ctx)
    ops.matvec(x, y3)
    assert torch.equal(mv.storage, y3.storage)
    y4 = ga._sentinel(ctx)
    ops.matvec(x, y4)
    assert torch.equal(y3.storage, y4.storage)
    with pytest.raises(RuntimeError, match="store=True"):
        ops.rmatvec(x, y4)
    # the frozen-base operator about q is something else
    yf = ctx.vector()
    flow.linearized(qv).matvec(x, yf)
    assert not torch.equal(yf.storage, mv.storage)
    a, b, Aa, Atb = ctx.vector(), ctx.vector(), ctx.vector(), ctx.vector()
    a.fill_hash(21)
    b.fill_hash(22)
    op.matvec(a, Aa)
    op.rmatvec(b, Atb)
    bm1 = flow.bm1.cpu().numpy()
    lhs, rhs = ctx.dot(b, Aa, time=False), ctx.dot(Atb, a, time=False)
    scale = float(np.sum(bm1 * np.abs(gb._rows(lay, Aa.to_packed())) * np.abs(gb._rows(lay, b.to_packed()))))
    defect = abs(lhs - rhs) / scale
    ah, bh = gb._rows(lay, a.to_packed()), gb._rows(lay, b.to_packed())
    Pa, Ptb = o64.tangent(ah, orb64), o64.adjoint(bh, orb64)
    w = o64.bg.ref.bm1
    own = abs(float(np.sum(w * bh * Pa) - np.sum(w * Ptb * ah))) / float(np.sum(w * np.abs(Pa) * np.abs(bh)))
    print(f"{name} adjoint defect: device {defect:.2e}, restatement {own:.2e}")
    assert scale > 0 and defect <= max(4 * own, 1e-12)


# ---- Newton for a forced periodic orbit, then Floquet ---------------------------------------------------
def test_forced_upo_newton_then_floquet_end_to_end(gpu):
    """The end-to-end case: newton_krylov(mode=2.2) from Pi target converges quadratically within 6 iterations onto
    the restatement's orbit; krylov_schur through LegacyMatvec(3.11) and (3.21) returns the three leading Floquet
    multipliers of the restatement's dense monodromy to 1e-10 relative, away from the frozen-base value; through
    (3.31) the leading intracycle gain; the bordered map of 2.1 fed from time_derivative under the gate."""
    from nekstab_next_amd.burgers import ViscousBurgers
    from nekstab_next_amd.config import GmresConfig, KrylovSchurConfig
    from nekstab_next_amd.krylov_schur import krylov_schur
    from nekstab_next_amd.newton import newton_krylov
    from nekstab_next_amd.operators import LegacyMatvec
    from nekstab_next_amd.orbit import OrbitFlow
    from nekstab_next_amd.vector import NekContext

    E = _e2e()
    co, mask, ob, qt, target, gc, gs = E["c64"]
    q_ref, hist = E["q"], E["hist"]
    lay = NekLayout(**E2E_LAY)
    c = orf.E2E
    ctx0 = NekContext(lay, max_cols=4)
    flow = ViscousBurgers(ctx0, co, c["kappa"], c["dt"], c["nsteps"], mask=mask)
    flow.steady_forcing(list(target))
    of = OrbitFlow(flow, cos=list(gc), sin=list(gs))
    ctx = NekContext(lay, weights=flow.bm1, max_cols=128)
    assert abs(of.tau - 1.0) < 1e-14
    nf, sv = lay.n_wf, lay.sv
    # Newton from Pi target
    q = gb._vector(ctx, target, time=0.0)
    flow.lin.project(q)
    res = newton_krylov(ctx, of.residual, of.linearized, q, tol=1e-20, maxiter=8, mode=2.2,
                        gmres=GmresConfig(k_dim=64, maxiter=100, tol=1e-24, mode="dcgs2-native"))
    r = res.residuals
    got = gb._rows(lay, q.to_packed())
    scale = float(np.max(np.abs(q_ref)))
    print("Newton ||F||^2:", r, "restatement:", hist, "GMRES iterations", [len(g.inner_residuals) for g in res.gmres],
          "max|q - q_ref|", np.max(np.abs(got - q_ref)))
    assert res.converged and len(r) <= 6 and r[-1] < 1e-20
    assert abs(r[0] - hist[0]) <= 1e-6 * hist[0]
    C2 = (2.0 * orf.NEWTON_C) ** 2                                   # the restatement's constant, doubled
    for k in range(len(r) - 1):
        if r[k] > 1e-12:
            assert r[k + 1] <= C2 * r[k] ** 2, (k, r)
    assert np.max(np.abs(got - q_ref)) <= 1e-10 * scale
    # Floquet: direct, adjoint, intracycle growth
    P = E["P"]
    mu = np.linalg.eigvals(P)
    lead = mu[np.argsort(-np.abs(mu))][:3]
    assert abs(lead[0] - orf.MULTIPLIERS[0]) < 1e-9
    sB = np.sqrt(ob.bg.mass())
    gain = float(np.linalg.svd(sB[:, None] * P / sB[None, :], compute_uv=False)[0] ** 2)
    assert abs(gain - orf.GAIN) < 1e-9
    op = of.linearized(q)
    tol = 1e-12
    cfg = KrylovSchurConfig(k_dim=48, schur_tgt=3, eigen_tol=tol)
    for mode in (3.11, 3.21):
        seed = ctx.vector()
        seed.fill_hash(11)
        ks = krylov_schur(ctx, LegacyMatvec(mode, op), seed, cfg)
        conv = np.flatnonzero(ks.residual < tol)
        assert conv.size >= 3, ks.residual
        worst = max(float(np.min(np.abs(ks.vals[conv] - m)) / abs(m)) for m in lead)
        print(f"uparam(1) = {mode}: {conv.size} converged, leading {ks.vals[0]:.12g}, worst relative error {worst:.2e}, "
              f"restarts {ks.schur_cnt}")
        assert worst <= 1e-10
        assert abs(ks.vals[0] - orf.FROZEN_BASE_MULTIPLIER) > 1e-3    # the orbit, not a frozen base, is in the operator
    seed = ctx.vector()
    seed.fill_hash(11)
    ks = krylov_schur(ctx, LegacyMatvec(3.31, op), seed, cfg)
    print(f"uparam(1) = 3.31: leading {ks.vals[0]:.12g}, sigma_1^2 {gain:.12g}")
    assert abs(ks.vals[0] - gain) <= 1e-10 * gain
    # the bordered map of 2.1 about the restatement's orbit (the same base state in every precision)
    old = E["cld"][2]
    ctx_t = NekContext(lay, weights=flow.bm1, max_cols=4, time_in_dot=True)
    qv = gb._vector(ctx_t, q_ref, time=0.0)
    qv.storage[nf * sv: nf * sv + lay.n_p] = 0.0
    b = ctx_t.vector()
    of.time_derivative(qv, b)
    b64, bld = ob.time_derivative(q_ref), old.time_derivative(q_ref)
    gb._gate_rows(gb._rows(lay, b.to_packed()), b64, bld, "bvec")
    A = LegacyMatvec(2.1, of.linearized(qv), b_fc=b, b_ic=b)
    x, f = ctx_t.vector(), ctx_t.vector()
    x.fill_hash(5)
    x.time = 0.7
    A.matvec(x, f)
    xh = gb._rows(lay, x.to_packed())
    want = [o.tangent(xh, o.propagate(q_ref)[1]) - xh.astype(o.dtype) + bb * o.dtype(0.7)
            for o, bb in ((ob, b64), (old, bld))]
    gb._gate_rows(gb._rows(lay, f.to_packed()), want[0], want[1], "bordered map")
    bm1 = flow.bm1.cpu().numpy().astype(np.longdouble)
    period = float(np.sum(bm1 * gb._rows(lay, b.to_packed()) * xh))
    print("period row", f.time, "want", period)
    assert abs(f.time - period) <= 1e-12 * abs(period)


# ---- shards ------------------------------------------------------------------------------------------
_SHARD_CASES = ((5, (3, 2, 2)), (8, (1, 1, 1)))


def _jobs(rank, world):
    """nkv_burgers_tangent_rhs, OrbitFlow.propagate and OrbitPropagator.matvec (about the stored orbit and side by
    side) / rmatvec over 2 steps with face_average="auto" on every case, this rank's slice."""
    from nekstab_next_amd.burgers import ViscousBurgers
    from nekstab_next_amd.comm import Comm
    from nekstab_next_amd.gs import GatherScatter
    from nekstab_next_amd.orbit import OrbitFlow
    from nekstab_next_amd.vector import NekContext

    comm = Comm()
    assert comm.world == world and comm.rank == rank
    res = {}
    for name in _SHARD_CASES:
        lay_g, co_g, B_g, mask_g, kap = gb._case(name)
        ctx = NekContext(lay_g, comm=comm, max_cols=4)
        lay = ctx.layout
        e0, e1 = lay.elem_range()
        sl = slice(e0 * lay.pts_v, e1 * lay.pts_v)
        co = {k: v[sl] for k, v in co_g.items()}
        g0, gc, gs = ([amp * np.sin(co["x"] + 0.2 * f + ph) * np.cos(co["y"]) for f in range(lay.n_wf)]
                      for amp, ph in ((0.3, 0.0), (0.2, 0.5), (0.1, 1.0)))
        flow = ViscousBurgers(ctx, co, kap, 1e-3, 2, forcing=g0, mask=mask_g[sl], face_average="auto")
        assert isinstance(flow.lin.face_average, GatherScatter) == (world > 1)
        of = OrbitFlow(flow, cos=gc, sin=gs)
        sbs = OrbitFlow(flow, cos=gc, sin=gs, store=False)
        lin = flow.lin
        q, x, y = ctx.vector(), ctx.vector(), ctx.vector()
        q.fill_hash(17)
        x.fill_hash(18)
        n, sv, nf = lay.n_v, lay.sv, lay.n_wf
        raw = torch.zeros(2 * nf * sv + 2, dtype=torch.float64, device=ctx.device)
        ctx.call("nkv_burgers_tangent_rhs", lay.lx1, lay.ldim, lin.D.data_ptr(), lin.w.data_ptr(), *lin._xyz_ptrs(), q.ptr,
                 sv, lin.kappa.data_ptr(), x.ptr, nf, sv, raw.data_ptr(), sv, raw.data_ptr() + 8 * nf * sv, sv, ctx.stream)
        both = raw.cpu().numpy()
        res[("rB", name)], res[("ru", name)] = gb._rows(lay, both[: nf * sv]), gb._rows(lay, both[nf * sv:])
        of.propagate(q, y)
        res[("phi", name)] = gb._rows(lay, y.to_packed())
        op = of.linearized(q)
        for key, apply in (("mv", op.matvec), ("rmv", op.rmatvec), ("sbs", sbs.linearized(q).matvec)):
            apply(x, y)
            res[(key, name)] = gb._rows(lay, y.to_packed())
    return res


def _rank_main(rank, world, port, out):
    import os
    import sys

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        out[rank] = _jobs(rank, world)
    finally:
        dist.destroy_process_group()


_RUNS = {}


def _world(world):
    """The results of every rank of ``world`` (spawned once per session; world 1 runs in this process)."""
    if world not in _RUNS:
        if world == 1:
            _RUNS[1] = {0: _jobs(0, 1)}
        else:
            out = mp.Manager().dict()
            ctx = mp.get_context("spawn")
            port = ga._free_port()
            procs = [ctx.Process(target=_rank_main, args=(r, world, port, out)) for r in range(world)]
            for p in procs:
                p.start()
            for p in procs:
                p.join()
            assert [p.exitcode for p in procs] == [0] * world
            _RUNS[world] = dict(out)
    return _RUNS[world]


@pytest.mark.parametrize("name", _SHARD_CASES, ids=str)
def test_shards_equal_one_rank(gpu, name):
    """Two gloo ranks sharing the GPU: the fused right-hand sides, the period map and the tangent (both modes) and
    adjoint over 2 steps equal the one-rank result bit for bit on every rank's slice.  The one-element case
    leaves rank 0 an empty shard, which takes part in every exchange and touches nothing."""
    one, got = _world(1)[0], _world(2)
    lay_g = gb._case(name)[0]
    keys = ("rB", "ru", "phi", "mv", "rmv", "sbs")
    for r in range(2):
        sh = lay_g.shard(r, 2)
        e0, e1 = sh.elem_range()
        sl = slice(e0 * sh.pts_v, e1 * sh.pts_v)
        for key in keys:
            np.testing.assert_array_equal(got[r][(key, name)], one[(key, name)][..., sl], err_msg=f"{key} rank {r}")
    for key in keys:
        assert np.any(one[(key, name)] != 0.0) and np.all(np.isfinite(one[(key, name)]))
    assert np.array_equal(one[("mv", name)], one[("sbs", name)])
    assert not np.array_equal(one[("mv", name)], one[("rmv", name)])
    assert not np.array_equal(one[("mv", name)], one[("phi", name)])
    if name == (8, (1, 1, 1)):
        assert lay_g.shard(0, 2).n_v == 0 and got[0][("mv", name)].shape == (lay_g.n_wf, 0)
