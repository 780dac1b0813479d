"""The viscous Burgers flow on the device (nkv_linconv_rhs, nkv_rk4_stage in csrc/advdiff.hip;
nekstab_next_amd/burgers.py) against its NumPy restatement (tests/burgers_reference.py), and the workflow it is
there for: Newton to a steady state, then the stability of that state and its adjoint spectrum.

Gate ("the gate" below), the project's for quantities differentiated twice (test_gpu_advdiff.py): with
e_ref = max |f64 - long double| of the restatement, the device is held to max(8 e_ref, 1e-12 max|ref|).
Element sub-ranges, repeated calls, shards and nkv_rk4_stage are compared bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import advdiff_reference as ar
import burgers_reference as br
import test_gpu_advdiff as ga

from nekstab_next_amd import _lib
from nekstab_next_amd.layout import NekLayout

ROOT = ga.ROOT
pytestmark = pytest.mark.gpu

CASES_3D = [(5, (3, 2, 2)), (8, (1, 1, 1)), (4, (7, 1, 1)), (10, (1, 2, 1)), (2, (3, 1, 1))]
E2E = "e2e"


# ---- meshes, base states, restatements ---------------------------------------------------------------
def _case(name):
    """(global layout, coordinates, base state of n_wf fields, wall mask, kappas) of a named case: the
    meshes and flows of test_gpu_advdiff.py, a smooth base scalar added in 3-D; "e2e": the end-to-end case
    about its Newton starting point (not a steady state)."""
    if name == E2E:
        co, mask, _, _, q0, *_ = _e2e()[0]
        return NekLayout(ldim=2, lx1=6, lx2=4, nelgv=9), co, [q0[0].copy(), q0[1].copy()], mask, list(br.E2E["kappa"])
    lay, co, U, mask = ga._mesh(name)
    B = [np.asarray(u, dtype=np.float64) for u in U]
    if lay.ldim == 3:
        B.append(np.cos(co["x"]) * np.sin(0.5 * co["y"] + 0.3 * co["z"]) + 0.1 * co["z"])
    assert len(B) == lay.n_wf
    return lay, co, B, mask, ga._kappas(lay)


_E2E, _BG = [], {}


def _e2e():
    """The end-to-end case of burgers_reference in f64 and long double (built once)."""
    if not _E2E:
        _E2E.extend(br.e2e_case(t) for t in (np.float64, np.longdouble))
    return _E2E


def _restatements(name, dt=None, nsteps=None):
    """The f64 and long double restatements of a case (their References are this module's own)."""
    key = (name, dt, nsteps)
    if key not in _BG:
        lay, co, B, mask, kap = _case(name)
        zero = [np.zeros(lay.n_v)] * lay.ldim
        _BG[key] = tuple(br.Burgers(ar.Reference(lay.lx1, lay.ldim, co, zero, mask=mask, dtype=t), kap, dt, nsteps)
                         for t in (np.float64, np.longdouble))
    return _BG[key]


def _rows(lay, packed):
    return np.stack([packed[f * lay.sv: f * lay.sv + lay.n_v] for f in range(lay.n_wf)])


def _gate_rows(got, a, b, what):
    for f in range(got.shape[0]):
        ga._gate(got[f], a[f], np.asarray(b[f]), f"{what} field {f}")


class _Raw(ga._Raw):
    """nkv_linconv_rhs on one mesh: the base state on the device with stride n_v."""

    def __init__(self, name):
        super().__init__(name if name != E2E else "cell")
        self.lay, self.co, B, _, self.kap = _case(name)
        self.xyz = [ga._dev(self.co[k]) for k in ("x", "y", "z")[: self.lay.ldim]]
        self.Bh = B
        self.B = ga._dev(np.concatenate(B))

    def lin(self, u, u_stride, r, r_stride, kappa, adjoint, e0=0, e1=None):
        lay = self.lay
        e1 = self.n // self.pts if e1 is None else e1
        L = lay.c_struct()
        L.n_v = (e1 - e0) * self.pts
        off = 8 * e0 * self.pts
        xyz = [t.data_ptr() + off for t in self.xyz] + ([None] if lay.ldim == 2 else [])
        rc = self.ctx.lib.nkv_linconv_rhs(ctypes.byref(L), lay.lx1, lay.ldim, self.D.data_ptr(), self.w.data_ptr(), *xyz,
                                          self.B.data_ptr() + off, self.n, kappa.data_ptr(), u.data_ptr() + off,
                                          lay.n_wf, u_stride, r.data_ptr() + off, r_stride, int(adjoint), self.st)
        assert rc == _lib.NKV_OK, _lib.last_error()


# ---- nkv_linconv_rhs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cyl"] + CASES_3D, ids=str)
def test_linconv_against_restatement(gpu, name):
    """Forward and adjoint coupled right-hand sides under the gate; r written with a stride above n_v leaves the
    NaN-filled gap untouched; a second call and element sub-ranges (pointer offset + shortened n_v) give the
    same bits."""
    raw = _Raw(name)
    lay, n, pts = raw.lay, raw.n, raw.pts
    b64, bld = _restatements(name)
    nf = lay.n_wf
    fields = ga._fields(lay, raw.co)
    stride = n + 24
    u = torch.full((nf * stride,), float("nan"), dtype=torch.float64, device="cuda")
    for f in range(nf):
        u[f * stride: f * stride + n] = ga._dev(fields[f])
    kd = ga._dev(raw.kap)
    E = n // pts
    for adjoint in (False, True):
        out = torch.full((nf * stride,), float("nan"), dtype=torch.float64, device="cuda")
        raw.lin(u, stride, out, stride, kd, adjoint)
        got = out.cpu().numpy().reshape(nf, stride)
        assert np.all(np.isnan(got[:, n:]))                             # the gap is untouched
        a, b = (bg.local(np.stack(fields), np.stack(raw.Bh), adjoint) for bg in (b64, bld))
        _gate_rows(got[:, :n], a, b, f"{name} adjoint={adjoint}")
        if not adjoint:
            fwd = got[:, :n].copy()
        again = torch.full_like(out, float("nan"))
        raw.lin(u, stride, again, stride, kd, adjoint)
        assert np.array_equal(again.cpu().numpy().reshape(nf, stride)[:, :n], got[:, :n])
        for e0, e1 in {(0, max(E // 2, 1)), (E // 2, E), (E - 1, E)}:
            part = torch.full_like(out, float("nan"))
            raw.lin(u, stride, part, stride, kd, adjoint, e0, e1)
            p = part.cpu().numpy().reshape(nf, stride)
            assert np.array_equal(p[:, e0 * pts:e1 * pts], got[:, e0 * pts:e1 * pts])
            assert np.all(np.isnan(p[:, :e0 * pts])) and np.all(np.isnan(p[:, e1 * pts:]))
    # the production term is in: the parent kernel about the same velocity gives something else
    par = torch.zeros(nf * stride, dtype=torch.float64, device="cuda")
    raw.rhs(u, nf, stride, par, stride, kd, False, U=raw.B, U_stride=n)
    assert np.max(np.abs(par.cpu().numpy().reshape(nf, stride)[:, :n] - fwd)) > 1e-3 * np.max(np.abs(fwd))


@pytest.mark.parametrize("name", [E2E, (5, (3, 2, 2))], ids=str)
def test_local_transpose_identity(gpu, name):
    """sum_p v . r_fwd(u) = sum_p u . r_adj(v) for random u, v, with no assembly: the two right-hand sides are
    transposes as matrices on the local points.  Held as test_rhs_constant_field_and_sum_identity holds the
    parent kernel's sum: to 1e-12 of the sum of the absolute terms."""
    raw = _Raw(name)
    n, nf = raw.n, raw.lay.n_wf
    rng = np.random.default_rng(31)
    u, v = rng.standard_normal((nf, n)), rng.standard_normal((nf, n))
    kd = ga._dev(raw.kap)
    rf = torch.zeros(nf * n, dtype=torch.float64, device="cuda")
    ra = torch.zeros(nf * n, dtype=torch.float64, device="cuda")
    raw.lin(ga._dev(u.ravel()), n, rf, n, kd, False)
    raw.lin(ga._dev(v.ravel()), n, ra, n, kd, True)
    rf, ra = rf.cpu().numpy().reshape(nf, n), ra.cpu().numpy().reshape(nf, n)
    lhs, rhs = float(np.sum(v * rf)), float(np.sum(u * ra))
    tol = 1e-12 * float(np.sum(np.abs(v * rf)))
    print(f"{name}: local transpose identity {abs(lhs - rhs):.3e}, tol {tol:.3e}")
    assert tol > 0 and abs(lhs - rhs) <= tol


def test_entry_checks(gpu):
    """Every NKV_EINVAL of nkv_linconv_rhs with its message, nothing launched; an empty shard returns NKV_OK and
    reads no pointer.  The same for nkv_rk4_stage."""
    lay = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=3, n_scalars=1)
    n, nf = lay.n_v, lay.n_wf
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.full((16 * n,), 7.0, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    L = lay.c_struct()
    u, B, r = p + 8 * 4 * n, p + 8 * 8 * n, p + 8 * 12 * n
    V = dict(L=ctypes.byref(L), lx1=4, ldim=3, D=p, w=p, xm=p, ym=p, zm=p, B=B, B_stride=n, kappa=p, u=u, nfld=nf,
             u_stride=n, r=r, r_stride=n, adjoint=0, stream=st)
    bad = [("ldim", 4, "ldim"), ("lx1", 11, "lx1"), ("zm", None, "zm"), ("u_stride", n - 1, "stride"),
           ("r_stride", n - 1, "stride"), ("B_stride", n - 1, "stride"), ("nfld", 2, "nfld=2 < ldim=3"),
           ("B", None, "B is NULL"), ("u", None, "u is NULL"), ("r", None, "r is NULL"), ("kappa", None, "kappa is NULL"),
           ("r", u, "r overlaps u or B"), ("r", u + 8 * (nf - 1) * n + 8 * (n - 1), "r overlaps u or B"),
           ("r", B, "r overlaps u or B"), ("r", B - 8 * (nf - 1) * n - 8 * (n - 1), "r overlaps u or B")]
    for adjoint in (0, 1):
        for key, val, msg in bad:
            assert lib.nkv_linconv_rhs(*{**V, "adjoint": adjoint, key: val}.values()) == _lib.NKV_EINVAL, key
            assert msg in _lib.last_error(), (key, _lib.last_error())
    S = dict(L=ctypes.byref(L), v=u, v_stride=n, minv=p, r=p + 8 * n, r_stride=n, g=None, g_stride=n, a=0.5, b=0.25,
             first=1, acc=None, acc_stride=n, w=B, w_stride=n, acc_out=r, ao_stride=n, nfld=1, zero_rest=0, stream=st)
    for key, val in (("v_stride", n - 1), ("r_stride", n - 1), ("w_stride", n - 1), ("ao_stride", n - 1), ("minv", None),
                     ("r", None), ("acc_out", None), ("nfld", 0), ("a", float("nan")), ("b", float("inf")),
                     ("zero_rest", 1), ("w", r), ("w", u), ("acc_out", p), ("first", 0)):
        assert lib.nkv_rk4_stage(*{**S, key: val}.values()) == _lib.NKV_EINVAL, (key, val)
        assert "rk4_stage" in _lib.last_error()
    assert lib.nkv_rk4_stage(*{**S, "g": u, "g_stride": n - 1}.values()) == _lib.NKV_EINVAL
    torch.cuda.synchronize()
    assert torch.all(buf == 7.0)                                     # nothing was launched
    Le = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=0, n_scalars=1).c_struct()
    assert lib.nkv_linconv_rhs(*{**V, "L": ctypes.byref(Le), "D": None, "B": None, "u": None, "r": None}.values()) \
        == _lib.NKV_OK
    assert lib.nkv_rk4_stage(*{**S, "L": ctypes.byref(Le), "minv": None, "r": None, "v": None, "acc_out": None}.values()) \
        == _lib.NKV_OK


# ---- nkv_rk4_stage -----------------------------------------------------------------------------------
def _rk4_numpy(v, m, r, g, a, b, first, acc):
    k = m * r
    if g is not None:
        k = k + g
    return v + a * k, (v if first else acc) + b * k


@pytest.mark.parametrize("lay", [NekLayout(ldim=3, lx1=4, lx2=2, nelgv=5, n_scalars=1), NekLayout(ldim=2, lx1=3, lx2=1, nelgv=9)],
                         ids=["3d-n320", "2d-n81"])
def test_rk4_stage_bits(gpu, lay):
    """nkv_rk4_stage equals the NumPy expression bit for bit: even strides from aligned bases (the 16-byte path;
    with n_v = 81 its odd last point) and odd strides (the scalar path); with and without g, with and without
    w, first or not; the NaN gaps between the rows stay NaN.  zero_rest on a state vector zeroes pressure and
    time and leaves the padding alone."""
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
    L = lay.c_struct()

    def packed(rows, stride):
        h = np.full(nf * stride, np.nan)
        for f in range(nf):
            h[f * stride: f * stride + n] = rows[f]
        return ga._dev(h)

    for stride in (n + 7 + (n + 7) % 2, n + 6 + (n + 7) % 2):           # even, then odd
        v, r, g, acc = (rng.standard_normal((nf, n)) for _ in range(4))
        vd, rd, gd, ad = (packed(t, stride) for t in (v, r, g, acc))
        for with_g in (False, True):
            for with_w in (False, True):
                for first in (False, True):
                    wd = torch.full((nf * stride,), float("nan"), dtype=torch.float64, device="cuda")
                    od = torch.full((nf * stride,), float("nan"), dtype=torch.float64, device="cuda")
                    rc = lib.nkv_rk4_stage(ctypes.byref(L), vd.data_ptr(), stride, md.data_ptr(), rd.data_ptr(), stride,
                                           gd.data_ptr() if with_g else None, stride, a, b, int(first), ad.data_ptr(),
                                           stride, wd.data_ptr() if with_w else None, stride, od.data_ptr(), stride, nf,
                                           0, st)
                    assert rc == _lib.NKV_OK, _lib.last_error()
                    ww, oo = _rk4_numpy(v, m, r, g if with_g else None, a, b, first, acc)
                    got_w, got_o = (t.cpu().numpy().reshape(nf, stride) for t in (wd, od))
                    what = (stride, with_g, with_w, first)
                    assert np.array_equal(got_o[:, :n], oo), what
                    assert np.all(np.isnan(got_o[:, n:])), what
                    assert np.array_equal(got_w[:, :n], ww) if with_w else np.all(np.isnan(got_w)), what
                    assert np.all(np.isnan(got_w[:, n:])), what
        # v = NULL stands for zero: w = a k, acc' = b k
        wd = torch.full((nf * stride,), float("nan"), dtype=torch.float64, device="cuda")
        od = torch.full((nf * stride,), float("nan"), dtype=torch.float64, device="cuda")
        rc = lib.nkv_rk4_stage(ctypes.byref(L), None, stride, md.data_ptr(), rd.data_ptr(), stride, gd.data_ptr(), stride,
                               a, b, 1, None, stride, wd.data_ptr(), stride, od.data_ptr(), stride, nf, 0, st)
        assert rc == _lib.NKV_OK, _lib.last_error()
        k = m * r + g
        assert np.array_equal(wd.cpu().numpy().reshape(nf, stride)[:, :n], a * k)
        assert np.array_equal(od.cpu().numpy().reshape(nf, stride)[:, :n], b * k)
        # in place: acc_out = acc
        ac = ad.clone()
        rc = lib.nkv_rk4_stage(ctypes.byref(L), vd.data_ptr(), stride, md.data_ptr(), rd.data_ptr(), stride, None, stride,
                               a, b, 0, ac.data_ptr(), stride, None, stride, ac.data_ptr(), stride, nf, 0, st)
        assert rc == _lib.NKV_OK, _lib.last_error()
        assert np.array_equal(ac.cpu().numpy().reshape(nf, stride)[:, :n], _rk4_numpy(v, m, r, None, a, b, False, acc)[1])
    # the last stage into a state vector
    sv = lay.sv
    v, r, g, acc = (rng.standard_normal((nf, n)) for _ in range(4))
    rd, gd, ad = (packed(t, sv) for t in (r, g, acc))
    y = ga._sentinel(ctx)
    rc = lib.nkv_rk4_stage(ctypes.byref(L), None, sv, md.data_ptr(), rd.data_ptr(), sv, gd.data_ptr(), sv, 0.0, b, 0,
                           ad.data_ptr(), sv, None, sv, y.ptr, sv, nf, 1, st)
    assert rc == _lib.NKV_OK, _lib.last_error()
    got = y.to_packed()
    ga._check_rest(lay, got)
    assert np.array_equal(_rows(lay, got), _rk4_numpy(v, m, r, g, 0.0, b, False, acc)[1])


# ---- the operators -----------------------------------------------------------------------------------
_OPS = {}
NSTEPS = 3


def _flow(name):
    """(ctx weighted by bm1, ViscousBurgers, restatements, base state, dt) of a case over NSTEPS steps, built
    once.  The 2-D case carries the steady forcing of its target, the 3-D case a smooth forcing."""
    if name not in _OPS:
        from nekstab_next_amd.burgers import ViscousBurgers
        from nekstab_next_amd.vector import NekContext

        lay, co, B, mask, kap = _case(name)
        if name == E2E:
            dt = br.E2E["dt"]
            forcing = None
        else:
            r64 = ga._refs(name)[0]
            dt = 1.5 / max(float(np.max(np.abs(np.linalg.eigvals(r64.dense(k))))) for k in kap)
            forcing = [0.3 * np.sin(co["x"] + 0.2 * f) * np.cos(co["y"]) for f in range(lay.n_wf)]
        b64, bld = _restatements(name, dt, NSTEPS)
        ctx0 = NekContext(lay, max_cols=4)
        flow = ViscousBurgers(ctx0, co, kap, dt, NSTEPS, forcing=forcing, mask=mask)
        if name == E2E:
            target = _e2e()[0][5]
            flow.steady_forcing(list(target))
            for bg in (b64, bld):
                bg.steady_forcing(target)
        else:
            for bg in (b64, bld):
                bg.g = bg.project(np.stack(forcing))
        ctx = NekContext(lay, weights=flow.bm1, max_cols=32)
        _OPS[name] = (ctx, flow, b64, bld, np.stack(B), dt)
    return _OPS[name]


def _vector(ctx, fields, time=3.0):
    lay = ctx.layout
    x = ctx.vector()
    x.from_fields({nm: (fields[i] if i < lay.n_wf else np.ones(m)) for i, (nm, _, m) in enumerate(lay.field_slices())},
                  time=time)
    return x


@pytest.mark.parametrize("name", [E2E, (5, (2, 2, 2))], ids=str)
def test_linearised_operator_against_restatement(gpu, name):
    """LinearisedConvection.matvec / rmatvec over 3 steps against the restatement's Horner propagators under the
    gate (pressure rows and time zeroed, padding untouched, deterministic), and the adjoint defect
    |<A x, y> - <x, A^+ y>| / sum bm1 |A x| |y| for unprojected hash vectors within 4 times the restatement's
    own f64 defect (floor 1e-12, as test_operator_against_restatement)."""
    ctx, flow, b64, bld, B, dt = _flow(name)
    lay = ctx.layout
    fields = np.stack(ga._fields(lay, _case(name)[1], seed=9))
    x = _vector(ctx, fields)
    op = flow.linearized(_vector(ctx, B))
    assert op is flow.lin
    assert np.array_equal(_rows(lay, op.B.cpu().numpy()), B)
    for adjoint, apply in ((False, op.matvec), (True, op.rmatvec)):
        y = ga._sentinel(ctx)
        apply(x, y)
        got = y.to_packed()
        ga._check_rest(lay, got)
        _gate_rows(_rows(lay, got), b64.propagate_lin(fields, B, adjoint), bld.propagate_lin(fields, B, adjoint),
                   f"{name} propagate_lin adjoint={adjoint}")
        y2 = ga._sentinel(ctx)
        apply(x, y2)
        assert torch.equal(y.storage, y2.storage)
    for adjoint in (False, True):
        y = ga._sentinel(ctx)
        op.rhs(x, y, adjoint)
        _gate_rows(_rows(lay, y.to_packed()), b64.L(fields, B, adjoint), bld.L(fields, B, adjoint), f"{name} L adjoint={adjoint}")
    a, b, Aa, Atb = ctx.vector(), ctx.vector(), ctx.vector(), ctx.vector()
    a.fill_hash(21)
    b.fill_hash(22)
    op.matvec(a, Aa)
    op.rmatvec(b, Atb)
    bm1 = flow.bm1.cpu().numpy()
    lhs, rhs = ctx.dot(b, Aa, time=False), ctx.dot(Atb, a, time=False)
    scale = float(np.sum(bm1 * np.abs(_rows(lay, Aa.to_packed())) * np.abs(_rows(lay, b.to_packed()))))
    defect = abs(lhs - rhs) / scale
    ah, bh = _rows(lay, a.to_packed()), _rows(lay, b.to_packed())
    Pa, Ptb = b64.propagate_lin(ah, B), b64.propagate_lin(bh, B, adjoint=True)
    own = abs(float(np.sum(b64.ref.bm1 * bh * Pa) - np.sum(b64.ref.bm1 * Ptb * ah))) / float(np.sum(b64.ref.bm1 * np.abs(Pa) * np.abs(bh)))
    print(f"{name} adjoint defect: device {defect:.2e}, restatement {own:.2e}")
    assert scale > 0 and defect <= max(4 * own, 1e-12)


@pytest.mark.parametrize("name", [E2E, (5, (2, 2, 2))], ids=str)
def test_flow_against_restatement(gpu, name):
    """ViscousBurgers.rhs (N(q), q as it is) and propagate (RK4^3 of the projected state) against the
    restatement under the gate; pressure rows and time zeroed, padding untouched, deterministic; residual is
    propagate minus q with time 0."""
    ctx, flow, b64, bld, B, dt = _flow(name)
    lay = ctx.layout
    fields = np.stack(ga._fields(lay, _case(name)[1], seed=4))
    x = _vector(ctx, fields)
    y = ga._sentinel(ctx)
    flow.rhs(x, y)
    got = y.to_packed()
    ga._check_rest(lay, got)
    _gate_rows(_rows(lay, got), b64.N(fields), bld.N(fields), f"{name} N")
    y = ga._sentinel(ctx)
    flow.propagate(x, y)
    got = y.to_packed()
    ga._check_rest(lay, got)
    _gate_rows(_rows(lay, got), b64.propagate(fields), bld.propagate(fields), f"{name} Phi")
    y2 = ga._sentinel(ctx)
    flow.propagate(x, y2)
    assert torch.equal(y.storage, y2.storage)
    f = ctx.vector()
    flow.residual(x, f)
    want = y.to_packed() - x.to_packed()
    assert np.array_equal(_rows(lay, f.to_packed()), _rows(lay, want)) and f.time == 0.0
    p0 = lay.n_wf * lay.sv
    assert np.array_equal(f.to_packed()[p0:p0 + lay.n_p], -x.to_packed()[p0:p0 + lay.n_p])


# ---- Newton, then stability, then the adjoint spectrum ------------------------------------------------
def test_newton_then_stability_end_to_end(gpu):
    """The end-to-end case: q_t is a steady state of the device's flow to rounding; newton_krylov from
    q_t + 0.02 Pi(pert) converges quadratically within 6 iterations onto q_t; krylov_schur about the converged
    state, direct and through LegacyMatvec(3.2, .), returns the five leading eigenvalues of the restatement's
    dense propagator to 1e-12 relative; one of them has |mu| > 1.1, which the operator without the production
    term (max |mu| = 0.866) cannot give."""
    from nekstab_next_amd.burgers import ViscousBurgers
    from nekstab_next_amd.config import GmresConfig, KrylovSchurConfig
    from nekstab_next_amd.krylov_schur import krylov_schur
    from nekstab_next_amd.newton import newton_krylov
    from nekstab_next_amd.operators import LegacyMatvec
    from nekstab_next_amd.vector import NekContext

    co, mask, bg, qt, q0, target, pert = _e2e()[0]
    lay = NekLayout(ldim=2, lx1=6, lx2=4, nelgv=9)
    c = br.E2E
    ctx0 = NekContext(lay, max_cols=4)
    flow = ViscousBurgers(ctx0, co, c["kappa"], c["dt"], c["nsteps"], mask=mask)
    flow.steady_forcing(list(target))
    ctx = NekContext(lay, weights=flow.bm1, max_cols=128)
    assert abs(flow.tau - 2.0) < 1e-14
    # the steady state
    x = _vector(ctx, target, time=0.0)
    flow.lin.project(x)
    steady = ctx.vector()
    flow.rhs(x, steady)
    nmax = float(np.max(np.abs(_rows(lay, steady.to_packed()))))
    print("max |N(q_t)| on the device:", nmax)
    assert nmax <= 1e-13 * float(np.max(np.abs(qt)))
    assert np.max(np.abs(_rows(lay, x.to_packed()) - qt)) <= 1e-14
    # Newton
    q = _vector(ctx, np.asarray(q0), time=0.0)
    q.storage[lay.n_wf * lay.sv: lay.n_wf * lay.sv + lay.n_p] = 0.0
    res = newton_krylov(ctx, flow.residual, flow.linearized, q, tol=1e-20, maxiter=8,
                        gmres=GmresConfig(k_dim=120, maxiter=100, tol=1e-24, mode="dcgs2-native"))
    r = res.residuals
    got = _rows(lay, q.to_packed())
    print("Newton ||F||^2:", r, "GMRES iterations", [len(g.inner_residuals) for g in res.gmres],
          "max|q - q_t|", np.max(np.abs(got - qt)))
    assert res.converged and len(r) <= 6 and r[-1] < 1e-20
    assert abs(r[0] - 3.3e-3) < 0.1e-3
    # quadratic until rounding: ||F_k+1|| <= C ||F_k||^2, C ~ 9 on the restatement, held as C^2 = 200 on ||F||^2
    for k in range(len(r) - 1):
        if r[k] > 1e-12:
            assert r[k + 1] <= 200.0 * r[k] ** 2, (k, r)
    assert r[2] < 1e-3 * r[1]
    assert np.max(np.abs(got - qt)) <= 1e-10 * np.max(np.abs(qt))
    # stability about the converged state
    P = bg.dense_propagator(qt)
    sB = np.sqrt(bg.mass())
    exact = np.linalg.eigvals(sB[:, None] * P / sB[None, :])
    lead = exact[np.argsort(-np.abs(exact))][:5]
    assert abs(lead[0] - 1.168724411411) < 1e-10
    op = flow.linearized(q)
    tol = 1e-12
    for what, A in (("direct", op), ("adjoint", LegacyMatvec(3.2, op))):
        seed = ctx.vector()
        seed.fill_hash(11)
        ks = krylov_schur(ctx, A, seed, KrylovSchurConfig(k_dim=24, schur_tgt=5, eigen_tol=tol))
        conv = np.flatnonzero(ks.residual < tol)
        assert conv.size >= 5, ks.residual
        worst = max(float(np.min(np.abs(ks.vals[conv] - mu)) / abs(mu)) for mu in lead)
        print(f"{what}: {conv.size} converged, leading {ks.vals[0]:.12g}, worst relative error {worst:.2e}, "
              f"restarts {ks.schur_cnt}")
        assert worst <= 1e-12
        assert np.max(np.abs(ks.vals[conv])) > 1.1


# ---- shards ------------------------------------------------------------------------------------------
_SHARD_CASES = ((5, (3, 2, 2)), (8, (1, 1, 1)))


def _jobs(rank, world):
    """nkv_linconv_rhs (forward and adjoint), ViscousBurgers.propagate and LinearisedConvection.matvec / rmatvec
    over 2 steps with face_average="auto" on every case, this rank's slice."""
    from nekstab_next_amd.burgers import ViscousBurgers
    from nekstab_next_amd.comm import Comm
    from nekstab_next_amd.gs import GatherScatter
    from nekstab_next_amd.vector import NekContext

    comm = Comm()
    assert comm.world == world and comm.rank == rank
    res = {}
    for name in _SHARD_CASES:
        lay_g, co_g, B_g, mask_g, kap = _case(name)
        ctx = NekContext(lay_g, comm=comm, max_cols=4)
        lay = ctx.layout
        e0, e1 = lay.elem_range()
        sl = slice(e0 * lay.pts_v, e1 * lay.pts_v)
        co = {k: v[sl] for k, v in co_g.items()}
        forcing = [0.3 * np.sin(co["x"] + 0.2 * f) * np.cos(co["y"]) for f in range(lay.n_wf)]
        flow = ViscousBurgers(ctx, co, kap, 1e-3, 2, forcing=forcing, mask=mask_g[sl], face_average="auto")
        assert isinstance(flow.lin.face_average, GatherScatter) == (world > 1)
        op = flow.lin.set_base([b[sl] for b in B_g])
        x, y = ctx.vector(), ctx.vector()
        x.fill_hash(17)
        n, sv, nf = lay.n_v, lay.sv, lay.n_wf
        raw = torch.zeros(nf * sv + 2, dtype=torch.float64, device=ctx.device)
        for key, adjoint in (("fwd", 0), ("adj", 1)):
            ctx.call("nkv_linconv_rhs", lay.lx1, lay.ldim, op.D.data_ptr(), op.w.data_ptr(), *op._xyz_ptrs(),
                     op.B.data_ptr(), sv, op.kappa.data_ptr(), x.ptr, nf, sv, raw.data_ptr(), sv, adjoint, ctx.stream)
            res[(key, name)] = _rows(lay, raw.cpu().numpy())
        for key, apply in (("phi", flow.propagate), ("mv", op.matvec), ("rmv", op.rmatvec)):
            apply(x, y)
            res[(key, name)] = _rows(lay, y.to_packed())
    return res


def _rank_main(rank, world, port, out):
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
    """Two gloo ranks sharing the GPU: the coupled right-hand sides, the nonlinear propagation and the
    linearised matvec / rmatvec over 2 steps equal the one-rank result bit for bit on every rank's slice.  The
    one-element case leaves rank 0 an empty shard, which takes part in every exchange and touches nothing."""
    one, got = _world(1)[0], _world(2)
    lay_g = _case(name)[0]
    for r in range(2):
        sh = lay_g.shard(r, 2)
        e0, e1 = sh.elem_range()
        sl = slice(e0 * sh.pts_v, e1 * sh.pts_v)
        for key in ("fwd", "adj", "phi", "mv", "rmv"):
            np.testing.assert_array_equal(got[r][(key, name)], one[(key, name)][..., sl], err_msg=f"{key} rank {r}")
    for key in ("fwd", "phi", "mv"):
        assert np.any(one[(key, name)] != 0.0) and np.all(np.isfinite(one[(key, name)]))
    assert not np.array_equal(one[("mv", name)], one[("rmv", name)])
    assert not np.array_equal(one[("mv", name)], one[("phi", name)])
    if name == (8, (1, 1, 1)):
        assert lay_g.shard(0, 2).n_v == 0 and got[0][("mv", name)].shape == (lay_g.n_wf, 0)
