"""The advection-diffusion operator on the device (csrc/advdiff.hip, nekstab_next_amd/advdiff.py) against its
NumPy restatement (tests/advdiff_reference.py).

Gate for everything differentiated twice, the project's convention (test_gpu_energy_budget.py): the
restatement runs in f64 and in long double from the same f64-rounded inputs; e_ref = max |f64 - long double|
is its own rounding error and the device — an equally valid f64 evaluation in another order — is held to
max(8 e_ref, 1e-12 max|ref|).  Element sub-ranges, repeated calls and shards are compared bit for bit."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import advdiff_reference as ar
from seed_helpers import box_mesh_coords
from test_bf_sensitivity import deformed_box

from nekstab_next_amd import _lib
from nekstab_next_amd import synthetic as syn
from nekstab_next_amd.layout import NekLayout, cylinder_layout
from nekstab_next_amd.sensitivity import gll_derivative

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
PI = np.pi
pytestmark = pytest.mark.gpu

CASES_3D = [(5, (3, 2, 2)), (8, (2, 3, 2)), (8, (1, 1, 1)), (4, (7, 1, 1)), (10, (1, 2, 1)), (2, (3, 1, 1))]


# ---- meshes, flows and fields ----------------------------------------------------------------------
def _mesh(name):
    """(global layout, coordinates, base flow components, wall mask) of a named case."""
    if name == "cyl":
        lay = cylinder_layout(1996)
        d = np.load(os.path.join(GOLD, "cyl_mesh_xy.npz"))
        co = {"x": d["x"], "y": d["y"]}
        bf = syn.from_reference_order(lay, np.load(os.path.join(GOLD, "bf_1cyl0_seed.npz"))["seed_ref"])
        U = [bf[c * lay.sv: c * lay.sv + lay.n_v].copy() for c in range(2)]
        return lay, co, U, ar.box_mask(co)
    if name == "cell":   # the 2-D case of tests/test_advdiff.py: one field layout (vx, vy), cellular flow
        lay = NekLayout(ldim=2, lx1=6, lx2=4, nelgv=9)
        co = ar.box_mesh_2d(6, (3, 3), (PI, PI), amp=0.04)
        x, y = co["x"], co["y"]
        U = [2.0 * np.sin(x) * np.cos(y) + 0.5, -2.0 * np.cos(x) * np.sin(y)]
        return lay, co, U, ar.box_mask(ar.box_mesh_2d(6, (3, 3), (PI, PI)))
    if name == "analytic":
        lay = NekLayout(ldim=2, lx1=8, lx2=6, nelgv=9)
        co = ar.box_mesh_2d(8, (3, 3), (PI, PI))
        n = co["x"].size
        return lay, co, [np.full(n, 0.3), np.zeros(n)], ar.box_mask(co)
    lx1, ne = name
    lay = NekLayout(ldim=3, lx1=lx1, lx2=max(lx1 - 2, 1), nelgv=int(np.prod(ne)), n_scalars=1)
    co = deformed_box(lay, ne)
    x, y, z = co["x"], co["y"], co["z"]
    U = [np.sin(y) + 0.3, 0.5 * np.cos(x), 0.2 * np.sin(x + z)]
    return lay, co, U, ar.box_mask(box_mesh_coords(lay, ne))


def _fields(lay, co, seed=5):
    """n_wf smooth functions of the coordinates plus 1e-3 noise."""
    rng = np.random.default_rng(seed)
    x, y = co["x"], co["y"]
    z = co["z"] if lay.ldim == 3 else 0.0 * x
    return [np.sin((1.0 + 0.1 * f) * x) * np.cos(0.8 * y + 0.2 * f) * (1.0 + 0.3 * z) + 1e-3 * rng.standard_normal(x.size)
            for f in range(lay.n_wf)]


def _kappas(lay):
    return [0.01 * (1 + f) for f in range(lay.n_wf)]


_REFS = {}


def _refs(name):
    """The f64 and long double restatements of a case (built once)."""
    if name not in _REFS:
        lay, co, U, mask = _mesh(name)
        _REFS[name] = tuple(ar.Reference(lay.lx1, lay.ldim, co, U, mask=mask, dtype=t) for t in (np.float64, np.longdouble))
    return _REFS[name]


def _gate(got, r64, rld, what):
    e_ref = float(np.max(np.abs(r64 - rld)))
    scale = float(np.max(np.abs(r64)))
    err = float(np.max(np.abs(got - r64)))
    print(f"{what}: e_ref/scale {e_ref / scale:.2e}, device-f64 {err / scale:.2e}, "
          f"device-longdouble {float(np.max(np.abs(got - rld))) / scale:.2e}")
    assert scale > 0 and e_ref > 0
    assert err <= max(8 * e_ref, 1e-12 * scale), (what, err, e_ref, scale)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")


class _Raw:
    """The raw entries on one mesh: D, w, coordinates and base flow on the device."""

    def __init__(self, name):
        from nekstab_next_amd.vector import NekContext

        self.lay, self.co, U, _ = _mesh(name)
        lay = self.lay
        self.ctx = NekContext(lay, max_cols=4)
        self.n, self.pts = lay.n_v, lay.pts_v
        self.D, self.w = _dev(gll_derivative(lay.lx1)), _dev(syn.gll_weights(lay.lx1))
        self.xyz = [_dev(self.co[k]) for k in ("x", "y", "z")[: lay.ldim]]
        self.U = _dev(np.concatenate(U))
        self.st = torch.cuda.current_stream().cuda_stream

    def rhs(self, u, nfld, u_stride, r, r_stride, kappa, adjoint, e0=0, e1=None, U=None, U_stride=None):
        """nkv_advdiff_rhs on elements [e0, e1): every per-point pointer moved by e0 elements."""
        lay = self.lay
        e1 = self.n // self.pts if e1 is None else e1
        L = lay.c_struct()
        L.n_v = (e1 - e0) * self.pts
        off = 8 * e0 * self.pts
        xyz = [t.data_ptr() + off for t in self.xyz] + ([None] if lay.ldim == 2 else [])
        U = self.U if U is None else U
        rc = self.ctx.lib.nkv_advdiff_rhs(ctypes.byref(L), lay.lx1, lay.ldim, self.D.data_ptr(), self.w.data_ptr(), *xyz,
                                          U.data_ptr() + off, self.n if U_stride is None else U_stride, kappa.data_ptr(),
                                          u.data_ptr() + off, nfld, u_stride, r.data_ptr() + off, r_stride,
                                          int(adjoint), self.st)
        assert rc == _lib.NKV_OK, _lib.last_error()


# ---- nkv_advdiff_rhs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cyl"] + CASES_3D, ids=str)
def test_rhs_against_restatement(gpu, name):
    """Forward and adjoint right-hand sides of n_wf fields with distinct kappa in one launch and of one field,
    with strides above n_v (the NaN-filled padding stays NaN), twice (same bits), and over element sub-ranges
    (pointer offset + shortened n_v: the bits of the whole)."""
    raw = _Raw(name)
    lay, n, pts = raw.lay, raw.n, raw.pts
    r64, rld = _refs(name)
    nf = lay.n_wf
    fields, kap = _fields(lay, raw.co), _kappas(lay)
    stride = n + 24
    u = torch.full((nf * stride,), float("nan"), dtype=torch.float64, device="cuda")
    for f in range(nf):
        u[f * stride: f * stride + n] = _dev(fields[f])
    kd = _dev(kap)
    E = n // pts
    for adjoint in (False, True):
        out = torch.full((nf * stride,), float("nan"), dtype=torch.float64, device="cuda")
        raw.rhs(u, nf, stride, out, stride, kd, adjoint)
        got = out.cpu().numpy().reshape(nf, stride)
        assert np.all(np.isnan(got[:, n:]))                             # the padding is untouched
        for f in range(nf):
            a, b = (r.local_rhs(fields[f], kap[f], adjoint) for r in (r64, rld))
            _gate(got[f, :n], a, np.asarray(b), f"{name} adjoint={adjoint} field {f}")
        again = torch.full_like(out, float("nan"))
        raw.rhs(u, nf, stride, again, stride, kd, adjoint)
        assert torch.equal(out[:n], again[:n]) and np.array_equal(again.cpu().numpy().reshape(nf, stride)[:, :n], got[:, :n])
        # one field, its own kappa: the bits of the batched launch
        one = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        f = nf - 1
        raw.rhs(u[f * stride:], 1, n, one, n, kd[f:], adjoint)
        assert np.array_equal(one.cpu().numpy(), got[f, :n])
        # element sub-ranges
        for e0, e1 in {(0, max(E // 2, 1)), (E // 2, E), (E - 1, E)}:
            part = torch.full_like(out, float("nan"))
            raw.rhs(u, nf, stride, part, stride, kd, adjoint, e0, e1)
            p = part.cpu().numpy().reshape(nf, stride)
            assert np.array_equal(p[:, e0 * pts:e1 * pts], got[:, e0 * pts:e1 * pts])
            assert np.all(np.isnan(p[:, :e0 * pts])) and np.all(np.isnan(p[:, e1 * pts:]))


def test_rhs_constant_field_and_sum_identity(gpu):
    """u = 1: the diffusion part of the forward right-hand side is rounding, and sum r = -sum bm1 U.grad 1 = 0.
    u = x with the cellular flow: sum_p r_forward = -sum bm1 U_x, since 1^T D_a^T F = (D_a 1)^T F = 0 and an
    isoparametric element differentiates x exactly."""
    raw = _Raw("cell")
    lay, n = raw.lay, raw.n
    r64, rld = _refs("cell")
    kd = _dev([0.02])
    ones, x = np.ones(n), raw.co["x"]
    out = torch.zeros(n, dtype=torch.float64, device="cuda")

    def run(u, U=None):
        raw.rhs(_dev(u), 1, n, out, n, kd, False, U=U, U_stride=n)
        return out.cpu().numpy().copy()

    rx = run(x)
    r1_diff = run(ones, U=torch.zeros(2 * n, dtype=torch.float64, device="cuda"))
    print("constant field, diffusion only: max|r| / max|r(x)|", np.max(np.abs(r1_diff)) / np.max(np.abs(rx)))
    assert np.max(np.abs(r1_diff)) <= 1e-12 * np.max(np.abs(rx))
    r1 = run(ones)
    a, b = r64.local_rhs(ones, 0.02), np.asarray(rld.local_rhs(ones, 0.02))
    gate = max(8 * float(np.max(np.abs(a - b))), 1e-12 * float(np.max(np.abs(a))))
    assert gate > 0 and np.max(np.abs(r1 - a)) <= gate
    assert abs(np.sum(r1)) <= n * gate                               # every point within the gate of ~0
    want = -np.sum(r64.bm1 * r64.U[0].reshape(-1))
    tol = 1e-12 * np.sum(np.abs(r64.local_rhs(x, 0.02)))
    print("sum r(x) + sum bm1 U_x", np.sum(rx) - want, "tol", tol)
    assert abs(np.sum(rx) - want) <= tol


def test_entry_checks(gpu):
    """Bad ldim, lx1 = 11, a missing zm in 3-D, a stride below n_v and a NULL pointer return NKV_EINVAL with a
    message and launch nothing; an empty shard returns NKV_OK and reads no pointer."""
    lay = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=3)
    n = lay.n_v
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.full((6 * n,), 7.0, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    L = lay.c_struct()
    V = dict(L=ctypes.byref(L), lx1=4, ldim=3, D=p, w=p, xm=p, ym=p, zm=p, U=p, U_stride=n, kappa=p, u=p, nfld=1,
             u_stride=n, r=p + 8 * 3 * n, r_stride=n, adjoint=0, stream=st)
    bad = [("ldim", 4, "ldim"), ("lx1", 11, "lx1"), ("zm", None, "zm"), ("u_stride", n - 1, "stride"),
           ("r_stride", n - 1, "stride"), ("U_stride", n - 1, "stride"), ("D", None, "D is NULL"),
           ("w", None, "w is NULL"), ("kappa", None, "kappa is NULL"), ("u", None, "u is NULL"),
           ("r", None, "r is NULL"), ("nfld", 0, "nfld"), ("r", p, "in place")]
    for key, val, msg in bad:
        assert lib.nkv_advdiff_rhs(*{**V, key: val}.values()) == _lib.NKV_EINVAL, key
        assert msg in _lib.last_error(), (key, _lib.last_error())
    Lb = lay.c_struct()
    Lb.n_v = n - 1                                                   # lx1^3 does not divide n_v
    assert lib.nkv_advdiff_rhs(*{**V, "L": ctypes.byref(Lb)}.values()) == _lib.NKV_EINVAL
    B = dict(L=ctypes.byref(L), lx1=4, ldim=3, D=p, w=p, xm=p, ym=p, zm=p, bm1=p + 8 * 3 * n, stream=st)
    for key, val in (("ldim", 1), ("lx1", 1), ("zm", None), ("bm1", None), ("w", None)):
        assert lib.nkv_advdiff_bm1(*{**B, key: val}.values()) == _lib.NKV_EINVAL, key
    Lv = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=3).c_struct()
    S = dict(L=ctypes.byref(Lv), v=p, v_stride=n, minv=p, r=p, r_stride=n, c=1.0, w=p + 8 * 3 * n, w_stride=n, nfld=1,
             zero_rest=0, stream=st)
    for key, val in (("v_stride", n - 1), ("r_stride", 0), ("w_stride", n - 1), ("minv", None), ("r", None),
                     ("w", None), ("nfld", 0), ("c", float("nan")), ("zero_rest", 1)):
        assert lib.nkv_advdiff_stage(*{**S, key: val}.values()) == _lib.NKV_EINVAL, key
    torch.cuda.synchronize()
    assert torch.all(buf == 7.0)                                     # nothing was launched
    E = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=0).c_struct()
    assert lib.nkv_advdiff_rhs(*{**V, "L": ctypes.byref(E), "D": None, "u": None, "r": None}.values()) == _lib.NKV_OK
    assert lib.nkv_advdiff_bm1(*{**B, "L": ctypes.byref(E), "bm1": None}.values()) == _lib.NKV_OK
    assert lib.nkv_advdiff_stage(*{**S, "L": ctypes.byref(E), "w": None}.values()) == _lib.NKV_OK


# ---- the operator ------------------------------------------------------------------------------------
_OPS = {}


def _operator(name, nsteps=3, equal_kappa=None, dt_rho=2.0):
    """(ctx weighted by op.bm1, op, f64 reference, long double reference, kappas, dt) of a case, built once."""
    key = (name, nsteps, equal_kappa, dt_rho)
    if key not in _OPS:
        from nekstab_next_amd.advdiff import AdvectionDiffusion
        from nekstab_next_amd.vector import NekContext

        lay, co, U, mask = _mesh(name)
        r64, rld = _refs(name)
        kap = [equal_kappa] * lay.n_wf if equal_kappa is not None else _kappas(lay)
        rho = max(float(np.max(np.abs(np.linalg.eigvals(r64.dense(k))))) for k in sorted(set(kap)))
        dt = dt_rho / rho
        ctx0 = NekContext(lay, max_cols=32)
        op = AdvectionDiffusion(ctx0, co, U, kap, dt, nsteps, mask=mask)
        ctx = NekContext(lay, weights=op.bm1, max_cols=32)   # the same layout: dots in the bm1 inner product
        _OPS[key] = (ctx, op, r64, rld, kap, dt)
    return _OPS[key]


def _field_rows(lay, packed):
    return [packed[f * lay.sv: f * lay.sv + lay.n_v] for f in range(lay.n_wf)]


def _sentinel(ctx, value=7.0):
    v = ctx.vector()
    v.storage.fill_(value)
    return v


def _check_rest(lay, packed, value=7.0):
    """Pressure rows and time are zero; every padding row still holds the sentinel."""
    for f in range(lay.n_wf):
        assert np.all(packed[f * lay.sv + lay.n_v:(f + 1) * lay.sv] == value)
    p0 = lay.n_wf * lay.sv
    assert np.all(packed[p0:p0 + lay.n_p] == 0.0) and lay.n_p > 0
    assert np.all(packed[p0 + lay.n_p:lay.time_offset] == value)
    assert packed[lay.time_offset] == 0.0
    assert np.all(packed[lay.time_offset + 1:] == value)


@pytest.mark.parametrize("name", ["cell", (5, (2, 2, 2))], ids=str)
def test_operator_against_restatement(gpu, name):
    """op.bm1, op.rhs, op.project and matvec / rmatvec over 3 steps against the restatement; pressure rows and
    time zeroed, padding untouched; the adjoint identity with ctx.dot in the bm1 inner product."""
    ctx, op, r64, rld, kap, dt = _operator(name)
    lay = ctx.layout
    n = lay.n_v
    bm1 = op.bm1.cpu().numpy()
    assert np.max(np.abs(bm1 - r64.bm1)) <= 1e-14 * np.max(r64.bm1)
    assert np.array_equal(op.mask.cpu().numpy(), r64.mask)
    assert abs(op.tau - 3 * dt) <= 1e-15 * op.tau
    fields = _fields(lay, _mesh(name)[1], seed=9)
    x = ctx.vector()
    x.from_fields({nm: (fields[i] if i < lay.n_wf else np.ones(m)) for i, (nm, _, m) in enumerate(lay.field_slices())},
                  time=3.0)
    for adjoint in (False, True):
        y = _sentinel(ctx)
        op.rhs(x, y, adjoint)
        got = y.to_packed()
        _check_rest(lay, got)
        for f, row in enumerate(_field_rows(lay, got)):
            # continuous input for L: the restatement's L takes the field as it is, like the device
            _gate(row, r64.L(fields[f], kap[f], adjoint), np.asarray(rld.L(fields[f], kap[f], adjoint)),
                  f"{name} L adjoint={adjoint} field {f}")
    y = _sentinel(ctx)
    op.project(x, y)
    got = y.to_packed()
    _check_rest(lay, got)
    for f, row in enumerate(_field_rows(lay, got)):
        _gate(row, r64.project(fields[f]), np.asarray(rld.project(fields[f])), f"{name} project field {f}")
    z = ctx.vector()
    z.copy_from(x)
    op.project(z)                                                    # in place
    assert np.array_equal(z.to_packed()[: lay.n_wf * lay.sv], np.where(got == 7.0, 0.0, got)[: lay.n_wf * lay.sv])
    for adjoint, apply in ((False, op.matvec), (True, op.rmatvec)):
        y = _sentinel(ctx)
        apply(x, y)
        got = y.to_packed()
        _check_rest(lay, got)
        for f, row in enumerate(_field_rows(lay, got)):
            _gate(row, r64.propagate(fields[f], kap[f], dt, 3, adjoint),
                  np.asarray(rld.propagate(fields[f], kap[f], dt, 3, adjoint)), f"{name} propagate adjoint={adjoint} field {f}")
        y2 = _sentinel(ctx)
        apply(x, y2)
        assert torch.equal(y.storage, y2.storage)                    # deterministic
    # <y, P x> = <P^T y, x> for unprojected hash vectors, in the bm1 inner product
    a, b, Pa, Ptb = ctx.vector(), ctx.vector(), ctx.vector(), ctx.vector()
    a.fill_hash(21)
    b.fill_hash(22)
    op.matvec(a, Pa)
    op.rmatvec(b, Ptb)
    lhs, rhs = ctx.dot(b, Pa, time=False), ctx.dot(Ptb, a, time=False)
    scale = sum(np.sum(bm1 * np.abs(q) * np.abs(p)) for q, p in zip(_field_rows(lay, b.to_packed()),
                                                                    _field_rows(lay, Pa.to_packed())))
    print(f"{name} adjoint identity: {abs(lhs - rhs) / scale:.2e}")
    assert scale > 0 and abs(lhs - rhs) <= 1e-12 * scale


def test_legacy_matvec_dispatch(gpu):
    """LegacyMatvec(3.0 / 3.2 / 3.3, op) applies matvec / rmatvec / rmatvec(matvec)."""
    from nekstab_next_amd.operators import LegacyMatvec

    ctx, op, *_ = _operator("cell")
    q = ctx.vector()
    q.fill_hash(3)
    want, got, mid = ctx.vector(), ctx.vector(), ctx.vector()
    op.matvec(q, want)
    LegacyMatvec(3.0, op).matvec(q, got)
    assert torch.equal(got.storage, want.storage) and float(want.storage.abs().max()) > 0
    op.rmatvec(q, want)
    LegacyMatvec(3.2, op).matvec(q, got)
    assert torch.equal(got.storage, want.storage)
    op.matvec(q, mid)
    op.rmatvec(mid, want)
    LegacyMatvec(3.3, op).matvec(q, got)
    assert torch.equal(got.storage, want.storage)


# ---- eigenvalues and singular values end to end --------------------------------------------------------
def _dense_propagator(r64, kappa, dt, nsteps):
    """B^(1/2) P B^(-1/2) on the free unique points: its eigenvalues are P's, its singular values those of P in
    the bm1 inner product."""
    sB = np.sqrt(r64.mass())
    return sB[:, None] * r64.dense_propagator(kappa, dt, nsteps) / sB[None, :]


@pytest.mark.parametrize("name,nsteps,tol", [("cell", 40, 1e-12), ((5, (2, 2, 2)), 60, 1e-14)], ids=str)
def test_krylov_schur_eigenvalues(gpu, name, nsteps, tol):
    """krylov_schur (k_dim = 24, schur_tgt = 2) driven by the propagator: every converged Ritz value within 1e-10
    relative of an eigenvalue of the restatement's dense P = p(dt L)^n.  With equal kappa the fields are
    uncoupled copies, so each eigenvalue may be found up to n_wf times.  eigen_tol: a Ritz value's error is at
    most its residual times the eigenvalue's condition number (<= 4 for the leading ones here, measured on
    the dense matrix), so a residual below 1e-12 (1e-14 where |lambda| ~ 1e-3) is well inside 1e-10 relative."""
    from nekstab_next_amd.config import KrylovSchurConfig
    from nekstab_next_amd.krylov_schur import krylov_schur

    kappa = 0.02 if name == "cell" else 0.05
    ctx, op, r64, _, _, dt = _operator(name, nsteps=nsteps, equal_kappa=kappa)
    lay = ctx.layout
    exact = np.linalg.eigvals(_dense_propagator(r64, kappa, dt, nsteps))
    seed = ctx.vector()
    seed.fill_hash(11)
    res = krylov_schur(ctx, op, seed, KrylovSchurConfig(k_dim=24, schur_tgt=2, eigen_tol=tol))
    conv = np.flatnonzero(res.residual < tol)
    assert conv.size >= 2, res.residual
    used = np.zeros(exact.size, dtype=int)
    worst = 0.0
    for v in res.vals[conv]:
        order = np.argsort(np.abs(exact - v))
        j = next(int(j) for j in order if used[j] < lay.n_wf)
        used[j] += 1
        worst = max(worst, abs(exact[j] - v) / abs(v))
    print(f"{name}: {conv.size} converged Ritz values, leading {res.vals[0]:.12g}, worst relative error {worst:.2e}, "
          f"restarts {res.schur_cnt}")
    assert worst <= 1e-10
    assert abs(abs(res.vals[0]) - np.max(np.abs(exact))) <= 1e-10 * np.max(np.abs(exact))


def test_analytic_growth_rate_through_the_device(gpu):
    """[0, pi]^2, U = (0.3, 0), kappa = 0.05, Dirichlet walls: log(leading Ritz value) / tau against
    log p(dt lambda) / dt at the exact lambda = -kappa (1 + 1) - c^2 / (4 kappa) = -0.55.  Gate 1e-7, the
    margin of test_advdiff.py's (a) (spatial error of the leading eigenvalue: 1.06e-9)."""
    from nekstab_next_amd.config import KrylovSchurConfig
    from nekstab_next_amd.krylov_schur import krylov_schur

    nsteps = 160
    ctx, op, r64, _, _, dt = _operator("analytic", nsteps=nsteps, equal_kappa=0.05, dt_rho=2.5)
    seed = ctx.vector()
    seed.fill_hash(5)
    res = krylov_schur(ctx, op, seed, KrylovSchurConfig(k_dim=24, schur_tgt=2, eigen_tol=1e-10))
    mu = res.vals[0]
    assert res.residual[0] < 1e-10 and abs(mu.imag) <= 1e-12
    got = np.log(mu.real) / op.tau
    want = np.log(ar.rk4_symbol(dt * -0.55)) / dt
    print(f"growth rate {got:.12f} against {want:.12f} (difference {abs(got - want):.2e}), tau {op.tau:.4f}")
    assert abs(got - want) <= 1e-7


def test_singular_values_and_transient_growth(gpu, tmp_path):
    """lightkrylov.svds on the 2-D case: sigma_1 (and every further converged value) within 1e-10 relative of
    the dense SVD of B^(1/2) P B^(-1/2), and sigma_1 > rho(P): the operator is non-normal, which is what the
    direct / adjoint path is tested for.  transient_growth_analysis runs on it and writes its files."""
    from nekstab_next_amd.drivers import transient_growth_analysis
    from nekstab_next_amd.krylov_schur import prepare_seed
    from nekstab_next_amd.lightkrylov import svds

    ctx, op, r64, _, _, dt = _operator("cell", nsteps=40, equal_kappa=0.02)
    S = _dense_propagator(r64, 0.02, dt, 40)
    sv = np.linalg.svd(S, compute_uv=False)
    rho = float(np.max(np.abs(np.linalg.eigvals(S))))
    seed = ctx.vector()
    seed.fill_hash(13)
    U, V = ctx.basis(25), ctx.basis(25)
    prepare_seed(seed, V[0])
    r = svds(ctx, op, U, V, nev=2, tolerance=1e-11)
    conv = np.flatnonzero(r.residuals < 1e-11)
    assert r.info == 0 and 0 in conv
    worst = max(float(np.min(np.abs(sv - s)) / s) for s in r.sigma[conv])
    print(f"sigma_1 {r.sigma[0]:.12f} (dense {sv[0]:.12f}), rho(P) {rho:.12f}, {conv.size} converged, worst {worst:.2e}")
    assert abs(r.sigma[0] - sv[0]) <= 1e-10 * sv[0] and worst <= 1e-10
    assert r.sigma[0] > rho * (1.0 + 1e-3)
    out = transient_growth_analysis(ctx, op, seed, k_dim=24, nev=2, tolerance=1e-11, outdir=str(tmp_path))
    assert out["info"] == 0 and abs(out["gain"][0] - sv[0] ** 2) <= 1e-9 * sv[0] ** 2
    names = sorted(os.listdir(tmp_path))
    assert "Spectrum_Sp.dat" in names and sum(nm.startswith("pU") for nm in names) == 2 \
        and sum(nm.startswith("pV") for nm in names) == 2


# ---- shards ------------------------------------------------------------------------------------------
_SHARD_CASES = ("cyl", (5, (3, 2, 2)), (8, (1, 1, 1)))


def _jobs(rank, world):
    """matvec and rmatvec over 2 steps with face_average="auto" on every case, this rank's slice."""
    from nekstab_next_amd.advdiff import AdvectionDiffusion, box_boundary_mask
    from nekstab_next_amd.comm import Comm
    from nekstab_next_amd.gs import GatherScatter
    from nekstab_next_amd.vector import NekContext

    comm = Comm()
    assert comm.world == world and comm.rank == rank
    res = {}
    for name in _SHARD_CASES:
        lay_g, co_g, U_g, mask_g = _mesh(name)
        ctx = NekContext(lay_g, comm=comm, max_cols=4)
        lay = ctx.layout
        e0, e1 = lay.elem_range()
        sl = slice(e0 * lay.pts_v, e1 * lay.pts_v)
        co = {k: v[sl] for k, v in co_g.items()}
        mask = mask_g[sl]
        if name == "cyl":   # the undeformed mesh: the walls are the bounding box, extents all-reduced
            assert np.array_equal(box_boundary_mask(co, comm, device=ctx.device), mask)
        op = AdvectionDiffusion(ctx, co, [u[sl] for u in U_g], _kappas(lay), 1e-3, 2, mask=mask, face_average="auto")
        assert isinstance(op.face_average, GatherScatter) == (world > 1)
        x, y = ctx.vector(), ctx.vector()
        x.fill_hash(17)
        for key, apply in (("mv", op.matvec), ("rmv", op.rmatvec)):
            apply(x, y)
            p = y.to_packed()
            res[(key, name)] = np.stack([p[f * lay.sv: f * lay.sv + lay.n_v] for f in range(lay.n_wf)])
        res[("bm1", name)] = op.bm1.cpu().numpy()
    return res


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


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
            port = _free_port()
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
    """Two gloo ranks sharing the GPU: matvec and rmatvec over 2 steps equal the one-rank result bit for bit on
    every rank's slice (the right-hand side is element-local, the average exchanges member values).  The
    one-element case leaves rank 0 an empty shard, which takes part in every exchange and touches nothing."""
    one, got = _world(1)[0], _world(2)
    lay_g = _mesh(name)[0]
    for r in range(2):
        sh = lay_g.shard(r, 2)
        e0, e1 = sh.elem_range()
        sl = slice(e0 * sh.pts_v, e1 * sh.pts_v)
        for key in ("mv", "rmv", "bm1"):
            np.testing.assert_array_equal(got[r][(key, name)], one[(key, name)][..., sl], err_msg=f"{key} rank {r}")
    assert np.any(one[("mv", name)] != 0.0) and np.all(np.isfinite(one[("mv", name)]))
    assert not np.array_equal(one[("mv", name)], one[("rmv", name)])
    if name == (8, (1, 1, 1)):
        assert lay_g.shard(0, 2).n_v == 0 and got[0][("mv", name)].shape == (lay_g.n_wf, 0)
