"""The two-system pressure CG and the incompressible resolvent on the device (nkv_pressure_div2 / _gradt2 /
_cg_update2 in csrc/pressure.hip, DivergenceFreeProjector.project_pair_ptr, IncompressibleResolventOperator in
nekstab_next_amd/resolvent.py).

The two-system entries are compared bit for bit with two calls of their single-system entries, and
``project_pair_ptr`` with two ``project_ptr``: no tolerance.  Runs of the stepper are held to the flow gate of
tests/test_gpu_incompressible.py (``_flow_gate``: max(8 e_ref, cond(E~) tol scale)).  The operator is held to the
dense answer: 4 times the distance of the f64 restatement of the same algorithm from it
(incompressible_resolvent_reference.DENSE_DISTANCE, measured by tests/test_incompressible_resolvent.py on the CPU),
floor 1e-11 relative; the adjoint identity to 4 times ADJOINT_DEFECT, same floor: the margins of
tests/test_gpu_coupled_resolvent.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import incompressible_resolvent_reference as irr
import test_gpu_advdiff as ga
import test_gpu_burgers as gb
import test_gpu_incompressible as gi
from test_gpu_resolvent import _check_zeroed, _download, _random_complex, _upload

from nekstab_next_amd import _lib
from nekstab_next_amd.layout import NekLayout

ROOT = ga.ROOT
pytestmark = pytest.mark.gpu

KERNEL_MESHES = ["odd2d", (3, (3, 2, 2)), (7, (2, 1, 2)), (10, (1, 2, 1))]
GATE = max(4 * irr.DENSE_DISTANCE, 1e-11)
ADJOINT_GATE = max(4 * irr.ADJOINT_DEFECT, 1e-11)
TOL = irr.CG_TOL
PB = 1024                                                            # NKV_PRESSURE_PARTIALS


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _same(a, b):
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def _ok(rc):
    assert rc == _lib.NKV_OK, _lib.last_error()


# ---- the two-system entries against two calls of the single-system entries ---------------------------------
class _Pair(gi._Raw):
    """The six pressure entries on pair buffers of one mesh: field f of system 0 at f * stride, of system 1 n_v
    doubles behind it (stride = 2 n_v + 24: gaps that must stay untouched; n_v = 81 on "odd2d")."""

    def __init__(self, name):
        super().__init__(name)
        self.stride = 2 * self.n + 24
        self.d = self.lay.ldim

    def fields(self, rng):
        """A pair buffer of ldim fields, NaN in the gaps."""
        u = _nan(self.d * self.stride)
        for c in range(self.d):
            u[c * self.stride: c * self.stride + 2 * self.n] = ga._dev(rng.standard_normal(2 * self.n))
        return u

    def pvec(self, rng):
        """(2, npz + 8) pressure vectors, NaN behind the npz values."""
        p = _nan(2, self.npz + 8)
        p[:, : self.npz] = ga._dev(rng.standard_normal((2, self.npz)))
        return p

    def div1(self, s, u, mult, out, pv, part, e0=0, e1=None):
        L, off, poff, head = self._head(e0, self.nel if e1 is None else e1)
        _ok(self.lib.nkv_pressure_div(ctypes.byref(L), *head, u.data_ptr() + 8 * s * self.n + off, self.stride,
                                      None if mult is None else mult.data_ptr() + off, out[s].data_ptr() + poff,
                                      None if pv is None else pv[s].data_ptr() + poff,
                                      None if pv is None else part[s].data_ptr(), self.st))

    def div2(self, active, u, mult, out, pv, part, e0=0, e1=None):
        L, off, poff, head = self._head(e0, self.nel if e1 is None else e1)
        ptr = lambda t, s, o: None if t is None or not active >> s & 1 else t[s].data_ptr() + o   # noqa: E731
        up = [u.data_ptr() + 8 * s * self.n + off if active >> s & 1 else None for s in range(2)]
        _ok(self.lib.nkv_pressure_div2(ctypes.byref(L), *head, *up, self.stride,
                                       None if mult is None else mult.data_ptr() + off, ptr(out, 0, poff),
                                       ptr(out, 1, poff), ptr(pv, 0, poff), ptr(pv, 1, poff),
                                       None if pv is None else part.data_ptr(), active, self.st))

    def gradt1(self, s, p, res, rr, first, t, e0=0, e1=None):
        L, off, poff, head = self._head(e0, self.nel if e1 is None else e1)
        _ok(self.lib.nkv_pressure_gradt(ctypes.byref(L), *head, p[s].data_ptr() + poff,
                                        None if res is None else res[s].data_ptr() + poff,
                                        None if res is None else rr[0][s].data_ptr(),
                                        None if res is None else rr[1][s].data_ptr(), PB, int(first),
                                        t.data_ptr() + 8 * s * self.n + off, self.stride, self.st))

    def gradt2(self, active, p, res, rr, first, t, e0=0, e1=None):
        L, off, poff, head = self._head(e0, self.nel if e1 is None else e1)
        ptr = lambda v, s: None if v is None or not active >> s & 1 else v[s].data_ptr() + poff   # noqa: E731
        tp = [t.data_ptr() + 8 * s * self.n + off if active >> s & 1 else None for s in range(2)]
        _ok(self.lib.nkv_pressure_gradt2(ctypes.byref(L), *head, ptr(p, 0), ptr(p, 1), ptr(res, 0), ptr(res, 1),
                                         None if res is None else rr[0].data_ptr(),
                                         None if res is None else rr[1].data_ptr(), PB, int(first), *tp, self.stride,
                                         active, self.st))


@pytest.mark.parametrize("name", KERNEL_MESHES, ids=str)
def test_div2_bits(gpu, name):
    """nkv_pressure_div2 against nkv_pressure_div on each system: outputs and partial rows, with and without the
    multiplier, with and without pv / partials, active = 1, 2, 3 (the inactive system's output and partial rows
    keep their NaN), an element sub-range, a second call."""
    raw = _Pair(name)
    rng = np.random.default_rng(11)
    u, pv = raw.fields(rng), raw.pvec(rng)
    mult = ga._dev(rng.uniform(0.5, 2.0, raw.n))
    E, pp = raw.nel, raw.ppts
    for m in (None, mult):
        for with_pv in (False, True):
            want, wpart = _nan(2, raw.npz + 8), _nan(2, 3 * PB)
            for s in range(2):
                raw.div1(s, u, m, want, pv if with_pv else None, wpart)
            assert torch.isfinite(want[:, : raw.npz]).all() and torch.isnan(want[:, raw.npz:]).all()
            assert not with_pv or torch.isfinite(wpart[:, 0]).all()
            for active in (1, 2, 3):
                got, part = _nan(2, raw.npz + 8), _nan(2, 3 * PB)
                raw.div2(active, u, m, got, pv if with_pv else None, part)
                for s in range(2):
                    if active >> s & 1:
                        assert _same(got[s], want[s]) and _same(part[s], wpart[s]), (name, active, s)
                    else:
                        assert torch.isnan(got[s]).all() and torch.isnan(part[s]).all(), (name, active, s)
                again, part2 = _nan(2, raw.npz + 8), _nan(2, 3 * PB)
                raw.div2(active, u, m, again, pv if with_pv else None, part2)
                assert _same(again, got) and _same(part2, part)
    full = _nan(2, raw.npz + 8)
    raw.div2(3, u, mult, full, None, None)
    for e0, e1 in {(0, max(E // 2, 1)), (E // 2, E), (E - 1, E)}:
        got = _nan(2, raw.npz + 8)
        raw.div2(3, u, mult, got, None, None, e0=e0, e1=e1)
        assert _same(got[:, e0 * pp: e1 * pp], full[:, e0 * pp: e1 * pp])
        assert torch.isnan(got[:, : e0 * pp]).all() and torch.isnan(got[:, e1 * pp:]).all()


@pytest.mark.parametrize("name", KERNEL_MESHES, ids=str)
def test_gradt2_bits(gpu, name):
    """nkv_pressure_gradt2 against nkv_pressure_gradt on each system: plain, with res on the first iteration and
    with res and each system's own beta; the gaps of the strided pair fields and the inactive system's t and p stay
    untouched; an element sub-range; a second call."""
    raw = _Pair(name)
    rng = np.random.default_rng(12)
    E, pts, n, d, stride = raw.nel, raw.pts, raw.n, raw.d, raw.stride
    p0, res = raw.pvec(rng), raw.pvec(rng)
    rr = [ga._dev(rng.uniform(0.5, 2.0, (2, PB))) for _ in range(2)]      # every system its own beta
    beta = (rr[0].sum(dim=1) / rr[1].sum(dim=1)).cpu().numpy()
    assert abs(beta[0] - beta[1]) > 1e-6

    def view(t):
        return t.view(d, stride)

    for mode in ("plain", "first", "beta"):
        r = None if mode == "plain" else res
        wp, wt = p0.clone(), _nan(d * stride)
        for s in range(2):
            raw.gradt1(s, wp, r, rr, mode != "beta", wt)
        assert torch.isnan(view(wt)[:, 2 * n:]).all() and torch.isfinite(view(wt)[:, : 2 * n]).all()
        assert (mode == "plain") == _same(wp, p0)
        for active in (1, 2, 3):
            gp, gt = p0.clone(), _nan(d * stride)
            raw.gradt2(active, gp, r, rr, mode != "beta", gt)
            for s in range(2):
                half = slice(s * n, (s + 1) * n)
                if active >> s & 1:
                    assert _same(gp[s], wp[s]) and _same(view(gt)[:, half], view(wt)[:, half]), (name, mode, active, s)
                else:
                    assert _same(gp[s], p0[s]) and torch.isnan(view(gt)[:, half]).all(), (name, mode, active, s)
            assert torch.isnan(view(gt)[:, 2 * n:]).all()
            if mode != "beta":                                       # (with beta a second call is another p)
                gp2, gt2 = p0.clone(), _nan(d * stride)
                raw.gradt2(active, gp2, r, rr, True, gt2)
                assert _same(gp2, gp) and _same(gt2, gt)
    full = _nan(d * stride)
    raw.gradt2(3, p0, None, rr, True, full)
    for e0, e1 in {(0, max(E // 2, 1)), (E // 2, E), (E - 1, E)}:
        got = _nan(d * stride)
        raw.gradt2(3, p0, None, rr, True, got, e0=e0, e1=e1)
        for s in range(2):
            lo, hi = s * n + e0 * pts, s * n + e1 * pts
            assert _same(view(got)[:, lo:hi], view(full)[:, lo:hi])
            assert torch.isnan(view(got)[:, s * n: lo]).all() and torch.isnan(view(got)[:, hi: (s + 1) * n]).all()


@pytest.mark.parametrize("n", [1, 81, 1000, 300001], ids=str)
def test_cg_update2_bits(gpu, n):
    """nkv_pressure_cg_update2 against nkv_pressure_cg_update on each system (one value, an odd count, several
    workgroups, more values than the grid covers in one pass): init and the update, closed and open, partial rows
    of NKV_PRESSURE_PARTIALS and reduced ones (Br = Bo = 1); active = 1, 2, 3."""
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(13)
    x0, r0, p, Ep = (ga._dev(rng.standard_normal((2, n + 3))) for _ in range(4))
    for B in (PB, 1):
        red, rr_old = ga._dev(rng.uniform(0.5, 2.0, (2, 3 * B))), ga._dev(rng.uniform(0.5, 2.0, (2, B)))
        for closed in (0, 1):
            for init in (0, 1):
                wx, wr, wout = x0.clone(), r0.clone(), _nan(2, PB)
                for s in range(2):
                    _ok(lib.nkv_pressure_cg_update(n, wx[s].data_ptr(), wr[s].data_ptr(), p[s].data_ptr(), Ep[s].data_ptr(),
                                                   red[s].data_ptr(), B, rr_old[s].data_ptr(), B, 1.0 / n, closed, init,
                                                   wout[s].data_ptr(), st))
                assert _same(wx[:, n:], x0[:, n:]) and not _same(wx[:, :n], x0[:, :n])
                for active in (1, 2, 3):
                    gx, gr_, gout = x0.clone(), r0.clone(), _nan(2, PB)
                    ptr = lambda t, s: t[s].data_ptr() if active >> s & 1 else None   # noqa: E731
                    _ok(lib.nkv_pressure_cg_update2(n, ptr(gx, 0), ptr(gx, 1), ptr(gr_, 0), ptr(gr_, 1), ptr(p, 0), ptr(p, 1),
                                                    ptr(Ep, 0), ptr(Ep, 1), red.data_ptr(), B, rr_old.data_ptr(), B, 1.0 / n,
                                                    closed, init, gout.data_ptr(), active, st))
                    for s in range(2):
                        if active >> s & 1:
                            assert _same(gx[s], wx[s]) and _same(gr_[s], wr[s]) and _same(gout[s], wout[s]), (B, closed, init, s)
                        else:
                            assert _same(gx[s], x0[s]) and _same(gr_[s], r0[s]) and torch.isnan(gout[s]).all()


def test_entry_checks(gpu):
    """NKV_EINVAL with a message: lx1 outside 3..10, active outside 1..3, a NULL operand of an active system,
    written spans that meet each other or an input; nothing is launched.  An empty shard returns NKV_OK and
    reads no pointer."""
    lay = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=3)
    n, npz = lay.n_v, 3 * 8
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    buf = torch.full((40 * n,), 7.0, dtype=torch.float64, device="cuda")
    b = buf.data_ptr()
    at = lambda k: b + 8 * k * n                                      # noqa: E731
    L = lay.c_struct()
    head = dict(L=ctypes.byref(L), lx1=4, ldim=3, D=b, interp=b, gw=b, xm=b, ym=b, zm=b)
    div = {**head, "u0": at(1), "u1": at(4), "u_stride": n, "mult": at(7), "out0": at(8), "out1": at(9), "pv0": at(10),
           "pv1": at(11), "partials": at(12), "active": 3, "stream": st}
    gradt = {**head, "p0": at(8), "p1": at(9), "res0": at(10), "res1": at(11), "rr_new": at(12), "rr_old": at(20), "B": 4,
             "first": 0, "t0": at(1), "t1": at(4), "t_stride": n, "active": 3, "stream": st}
    upd = dict(n=npz, x0=at(1), x1=at(2), r0=at(3), r1=at(4), p0=at(5), p1=at(6), Ep0=at(7), Ep1=at(8), red=at(9), Br=4,
               rr_old=at(10), Bo=4, inv_n=1.0 / npz, closed=1, init=0, rr_out=at(12), active=3, stream=st)
    last = 8 * (npz - 1)
    cases = [
        (lib.nkv_pressure_div2, div, [("lx1", 2, "lx1=2"), ("lx1", 11, "lx1=11"), ("ldim", 4, "ldim"), ("active", 0, "active=0"),
                                      ("active", 4, "active=4"), ("u1", None, "u1 is NULL"), ("out0", None, "out0 is NULL"),
                                      ("pv1", None, "pv1 and partials"), ("partials", None, "partials"),
                                      ("u_stride", n - 1, "u_stride"), ("zm", None, "zm"), ("D", None, "D is NULL"),
                                      ("out1", at(8) + last, "out0 overlaps out1"), ("out0", at(1), "out0 overlaps u0"),
                                      ("out1", at(3) + 8 * (n - 1), "out1 overlaps u0"), ("out0", at(6), "out0 overlaps u1"),
                                      ("out1", at(7), "out1 overlaps mult"), ("out0", at(11), "out0 overlaps pv1"),
                                      ("partials", at(8), "out0 overlaps partials")]),
        (lib.nkv_pressure_gradt2, gradt, [("lx1", 2, "lx1=2"), ("lx1", 11, "lx1=11"), ("active", -1, "active=-1"),
                                          ("active", 4, "active=4"), ("p1", None, "p1 is NULL"), ("t0", None, "t0 is NULL"),
                                          ("res1", None, "res0 and res1"), ("rr_new", None, "rr_new is NULL"),
                                          ("rr_old", None, "rr_old is NULL"), ("B", 0, "B=0"), ("B", PB + 1, "B=1025"),
                                          ("t_stride", n - 1, "t_stride"), ("t1", at(1) + 8 * (n - 1), "t0 overlaps t1"),
                                          ("t0", at(8), "t0 overlaps p0"), ("t1", at(10), "t1 overlaps res0"),
                                          ("p1", at(8) + last, "p0 overlaps p1"), ("p0", at(11), "p0 overlaps res1"),
                                          ("res0", at(8), "p0 overlaps res0")]),
        (lib.nkv_pressure_cg_update2, upd, [("n", -1, "n=-1"), ("active", 0, "active=0"), ("active", 7, "active=7"),
                                            ("x1", None, "x1 is NULL"), ("r0", None, "r0 is NULL"), ("p1", None, "p1 is NULL"),
                                            ("Ep0", None, "Ep0 is NULL"), ("red", None, "red is NULL"),
                                            ("rr_old", None, "rr_old is NULL"), ("rr_out", None, "rr_out is NULL"),
                                            ("Br", 0, "Br=0"), ("Bo", PB + 1, "Bo=1025"), ("inv_n", float("inf"), "inv_n"),
                                            ("x1", at(1) + last, "x0 overlaps x1"), ("r1", at(1), "x0 overlaps r1"),
                                            ("x0", at(5), "x0 overlaps p0"), ("r1", at(7), "r1 overlaps Ep0"),
                                            ("rr_out", at(9), "rr_out overlaps red")]),
    ]
    for fn, good, bad in cases:
        for key, val, msg in bad:
            assert fn(*{**good, key: val}.values()) == _lib.NKV_EINVAL, (fn.__name__, key)
            assert msg in _lib.last_error() and fn.__name__[4:] in _lib.last_error(), (key, _lib.last_error())
    # the halves of a pair vector interleave: accepted at t1 = t0 + n_v, refused one double closer
    pair = {**gradt, "t_stride": 2 * n, "t1": at(1) + 8 * (n - 1), "t0": at(1)}
    assert lib.nkv_pressure_gradt2(*pair.values()) == _lib.NKV_EINVAL and "t0 overlaps t1" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.all(buf == 7.0)                                     # nothing was launched
    Le = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=0).c_struct()
    for fn, good in ((lib.nkv_pressure_div2, div), (lib.nkv_pressure_gradt2, gradt)):
        empty = {k: (None if isinstance(v, int) and v >= b else v) for k, v in good.items()}
        empty.update(L=ctypes.byref(Le), stream=st)
        assert fn(*empty.values()) == _lib.NKV_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert torch.all(buf == 7.0)


# ---- project_pair_ptr --------------------------------------------------------------------------------------
def _pair_states(ctx, ref, pr, seed):
    """Two state vectors whose solves need clearly different iteration counts: a random Pi-projected velocity, and
    the correction minv dsavg(D^T phi) of a multiplier phi that is a combination of 12 eigenvectors of E~ (those of
    its largest eigenvalues, which are well separated): its right-hand side E~ phi lies in an invariant subspace of
    dimension 12, where CG ends within 12 iterations, at the check after 16.  (A projected velocity plus a small
    random perturbation does not do it: the stop is relative to the system's own right-hand side and the count is
    set by the spectrum the right-hand side excites, measured 104 against 104 on the 2-D mesh.)"""
    lay = ctx.layout
    a, _ = gi._state(ctx, ref, seed)
    E = pr.dense_E().astype(np.float64)
    Zm = np.eye(pr.npz) - (1.0 / pr.npz if pr.closed else 0.0)
    lam, V = np.linalg.eigh(Zm @ (0.5 * (E + E.T)) @ Zm)
    phi = V[:, -12:] @ (1.0 + np.arange(12))
    rng = np.random.default_rng(seed + 1)
    rows = list(pr.correction(phi)) + [rng.standard_normal(ref.n) for _ in range(lay.n_wf - lay.ldim)]
    return a, gb._vector(ctx, rows)


@pytest.mark.parametrize("name", gi.PROJECTOR_CASES, ids=str)
def test_project_pair_ptr(gpu, name):
    """Both results equal project_ptr on each input alone, bit for bit, with the same iteration counts, which
    differ (the freeze is exercised), in either order of the systems, in place and out of place; a zero second
    system returns untouched with count 0; maxiter = 3 raises."""
    from nekstab_next_amd.pressure import DivergenceFreeProjector

    ctx, proj, ref, pr, co, mask = gi._projector(name)
    lay = ctx.layout
    a, b = _pair_states(ctx, ref, pr, 21)
    want, its = [], []
    for v in (a, b):
        y = ctx.vector()
        proj.apply(v, y)
        want.append(y)
        its.append(proj.last_iterations)
    print(f"{name}: single iteration counts {its}")
    assert its[0] >= 2 * its[1] > 0
    sv = lay.sv
    for order in ((0, 1), (1, 0)):
        src = [(a, b)[k] for k in order]
        ya, yb = ga._sentinel(ctx), ga._sentinel(ctx)
        proj.project_pair_ptr(src[0].ptr, src[1].ptr, sv, ya.ptr, yb.ptr)
        assert proj.last_iterations_each == tuple(its[k] for k in order) and proj.last_iterations == max(its)
        for got, k in ((ya, order[0]), (yb, order[1])):
            assert torch.equal(got.storage[: lay.ldim * sv].view(lay.ldim, sv)[:, : lay.n_v],
                               want[k].storage[: lay.ldim * sv].view(lay.ldim, sv)[:, : lay.n_v])
            assert torch.all(got.storage[lay.ldim * sv:] == 7.0)     # nothing but the velocity rows is written
    ia, ib = ctx.vector(), ctx.vector()
    ia.copy_from(a)
    ib.copy_from(b)
    proj.project_pair_ptr(ia.ptr, ib.ptr, sv)                          # in place
    assert torch.equal(ia.storage, want[0].storage) and torch.equal(ib.storage, want[1].storage)
    zero = ctx.vector()
    ia.copy_from(a)
    proj.project_pair_ptr(ia.ptr, zero.ptr, sv)
    assert proj.last_iterations_each == (its[0], 0) and float(zero.storage.abs().max()) == 0.0
    assert torch.equal(ia.storage, want[0].storage)
    if name == "closed2d":
        short = DivergenceFreeProjector(ctx, co, mask=mask, tol=gi.TOL, maxiter=3)
        ia.copy_from(a)
        ib.copy_from(b)
        with pytest.raises(RuntimeError, match="maxiter=3"):
            short.project_pair_ptr(ia.ptr, ib.ptr, sv)
        assert short.last_iterations == 3


# ---- the operator ------------------------------------------------------------------------------------------
LAYOUTS = {"case2d": dict(ldim=2, lx1=5, lx2=3, nelgv=9), "box3d": dict(ldim=3, lx1=4, lx2=2, nelgv=8, n_scalars=1)}
# dt and nsteps of the operator tests against the dense answer, which depends on neither: three long steps over about
# the cases' own tau, so that an inner solve is some hundred GMRES iterations of three steps and not of eight
# (dt (rho + omega) = 2.33 and 2.36 with rho = 15.93 and 18.15 of tests/test_incompressible_resolvent.py: inside RK4's
# region, whose left half reaches 2.78).  The runs against the restatement use the cases' own dt.
SOLVE_STEPS = {"case2d": (0.13, 3), "box3d": (0.12, 3)}
_CASES, _OPS = {}, {}


def _case(name, dtype=np.float64):
    if (name, dtype) not in _CASES:
        _CASES[(name, dtype)] = irr.CASES[name](dtype)
    return _CASES[(name, dtype)]


def _build(name, dt=None, nsteps=None, comm=None, max_cols=64):
    """(LinearisedNavierStokes at CG tol 1e-13 with a batched dsavg, pair context) of a case or this rank's shard."""
    from nekstab_next_amd.gs import GatherScatter
    from nekstab_next_amd.incompressible import LinearisedNavierStokes
    from nekstab_next_amd.resolvent import pair_context
    from nekstab_next_amd.vector import NekContext

    co, mask, ns, B, dt0, nsteps0 = _case(name)
    lay_g = NekLayout(**LAYOUTS[name])
    ctx = NekContext(lay_g, max_cols=4) if comm is None else NekContext(lay_g, comm=comm, max_cols=4)
    e0, e1 = ctx.layout.elem_range() if comm is not None else (0, lay_g.nelv)
    sl = slice(e0 * lay_g.pts_v, e1 * lay_g.pts_v)
    co = {k: v[sl] for k, v in co.items()}
    lns = LinearisedNavierStokes(ctx, co, [b[sl] for b in np.asarray(B, dtype=np.float64)], ns.kappa, dt0 if dt is None else dt,
                                 nsteps0 if nsteps is None else nsteps, mask=mask[sl], face_average=GatherScatter(ctx, co),
                                 tol=TOL)
    return lns, pair_context(lns, max_cols=max_cols)


def _solver(name):
    """(lns, pctx) with SOLVE_STEPS, built once; the tests that change the base state build their own."""
    if name not in _OPS:
        _OPS[name] = _build(name, *SOLVE_STEPS[name], max_cols=200)
    return _OPS[name]


def _dense(name, omega):
    co, mask, ns, B, dt, nsteps = _case(name)
    return irr.IncompressibleResolvent(ns, B, dt, nsteps, omega)


@pytest.mark.parametrize("name", ["case2d", "box3d"])
def test_runs_against_restatement(gpu, name):
    """project, one forced and one unforced run over 2 steps, direct and adjoint, against the restatement in f64 and
    long double under the flow gate; pressure and time zeroed; batched=False gives the same bits."""
    from nekstab_next_amd.resolvent import IncompressibleResolventOperator

    lns, pctx = _build(name, nsteps=2)
    omega = irr.OMEGAS[name][1]
    op = IncompressibleResolventOperator(pctx, lns, omega)
    seq = IncompressibleResolventOperator(pctx, lns, omega, batched=False)
    lay = lns.ctx.layout
    r64, rld = (irr.IncompressibleResolvent(c[2], c[3], c[4], 2, omega) for c in (_case(name), _case(name, np.longdouble)))
    cond = gi._cond(r64.ns)
    assert gi.FLOW_TOL == TOL                                        # the flow gate is stated for this CG tolerance

    def gate(got, a, b, what):
        for part in ("real", "imag"):
            gi._flow_gate(getattr(got, part), getattr(a, part), np.asarray(getattr(b, part)), cond, f"{name} {what} {part}")

    xz = _random_complex(lay.n_wf, lay.n_v, 7)
    x = _upload(pctx, xz, pressure=1.0, time=3.0)
    f = _upload(pctx, 0 * xz, pressure=7.0, time=7.0)
    op.project(x, f)
    _check_zeroed(pctx.layout, f.to_packed())
    fz = _download(pctx, f)
    gate(fz, r64.project(xz), rld.project(xz), "project")
    assert op.projector.last_iterations_each[0] > 0 and op.projector.last_iterations_each[1] > 0
    f2 = pctx.vector()
    seq.project(x, f2)
    assert torch.equal(f2.storage, f.storage)
    for adjoint in (False, True):
        b, b2 = _upload(pctx, 0 * xz, pressure=7.0, time=7.0), pctx.vector()
        op.forced_run(f, b, adjoint)
        _check_zeroed(pctx.layout, b.to_packed())
        gate(_download(pctx, b), r64.forced_run(fz, adjoint), rld.forced_run(fz, adjoint), f"forced_run adjoint={adjoint}")
        seq.forced_run(f, b2, adjoint)
        assert torch.equal(b2.storage, b.storage)
        y, y2 = _upload(pctx, 0 * xz, pressure=7.0, time=7.0), pctx.vector()
        op.propagate(f, y, adjoint)
        _check_zeroed(pctx.layout, y.to_packed())
        gate(_download(pctx, y), r64.propagate(fz, adjoint), rld.propagate(fz, adjoint), f"propagate adjoint={adjoint}")
        seq.propagate(f, y2, adjoint)
        assert torch.equal(y2.storage, y.storage)
        assert np.array_equal(_download(pctx, f), fz)               # the forcing is read only


def _against_dense(op, pctx, lns, dense, what, adjoint=True):
    """matvec / rmatvec of random unprojected f, g against the dense answer under GATE, the adjoint identity in the
    pair bm1 product under ADJOINT_GATE, pressure and time zeroed, Z D y of both halves at the level of the CG
    tolerance.  Returns the downloaded matvec (``adjoint=False``: the matvec alone)."""
    lay = lns.ctx.layout
    fz, gz = _random_complex(lay.n_wf, lay.n_v, 4), _random_complex(lay.n_wf, lay.n_v, 5)
    f, g = _upload(pctx, fz, pressure=1.0, time=2.0), _upload(pctx, gz)
    y, ya = _upload(pctx, 0 * fz, pressure=7.0, time=7.0), pctx.vector()
    op.matvec(f, y)
    info = op.last_gmres
    assert info["info"] == 0 and info["adjoint"] is False and info["residuals"][-1] <= 1e-13 * info["residuals"][0]
    _check_zeroed(pctx.layout, y.to_packed())
    yz = _download(pctx, y)
    sides = [(yz, lambda: dense.dense_apply(fz), "matvec")]
    if adjoint:
        op.rmatvec(g, ya)
        assert op.last_gmres["info"] == 0 and op.last_gmres["adjoint"] is True
        sides.append((_download(pctx, ya), lambda: dense.dense_apply(gz, adjoint=True), "rmatvec"))
    for got, answer, side in sides:
        want = answer()
        d = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f"{what} {side}: distance from the dense answer {d:.2e} (gate {GATE:.1e})")
        assert np.max(np.abs(want)) > 0 and d <= GATE, (what, side, d)
    if adjoint:
        lhs, rhs = pctx.dot(y, g, time=False), pctx.dot(f, ya, time=False)
        scale = float(np.sum(lns.bm1.cpu().numpy() * (np.abs(yz.real * gz.real) + np.abs(yz.imag * gz.imag))))
        print(f"{what} adjoint identity: {abs(lhs - rhs) / scale:.2e} (gate {ADJOINT_GATE:.1e})")
        assert scale > 0 and abs(lhs - rhs) <= ADJOINT_GATE * scale
    # Z D y against Z D of a field of y's size that is not projected: cond(E~) tol, cond(E~) < 1e3
    # (tests/test_incompressible_resolvent.py)
    pif = dense.ns.ref.project(fz.real) + 1j * dense.ns.ref.project(fz.imag)
    unprojected = float(np.max(np.abs(dense.divergence(pif))) * np.max(np.abs(yz)) / np.max(np.abs(pif)))
    div = float(np.max(np.abs(dense.divergence(yz)))) / unprojected
    print(f"{what}: |Z D y| against an unprojected field {div:.2e}")
    assert div <= 1e3 * TOL
    return yz


@pytest.mark.parametrize("name,k", [("case2d", 0), ("case2d", 1), ("box3d", 0), ("box3d", 1)], ids=str)
def test_operator_against_dense_answer(gpu, name, k):
    """matvec / rmatvec at inner tol = 1e-13 against the dense answer on range(P Pi) (gate: module docstring), at the
    frequency near a weakly damped eigenfrequency (k = 0) and away from it (k = 1)."""
    from nekstab_next_amd.resolvent import IncompressibleResolventOperator

    lns, pctx = _solver(name)
    omega = irr.OMEGAS[name][k]
    op = IncompressibleResolventOperator(pctx, lns, omega, tol=1e-13, kdim=200, maxiter=4)
    _against_dense(op, pctx, lns, _dense(name, omega), f"{name} omega {omega}")
    print(f"{name} omega {omega}: inner GMRES cycles of at most 200 iterations: {len(op.last_gmres['residuals']) - 1}")


def test_batched_equals_sequential(gpu):
    """One matvec with batched=True and with batched=False on one rank: the same bits."""
    from nekstab_next_amd.resolvent import IncompressibleResolventOperator

    lns, pctx = _solver("box3d")
    lay = lns.ctx.layout
    omega = irr.OMEGAS["box3d"][1]
    f = _upload(pctx, _random_complex(lay.n_wf, lay.n_v, 4))
    out = []
    for batched in (True, False):
        op = IncompressibleResolventOperator(pctx, lns, omega, tol=1e-6, kdim=200, maxiter=4, batched=batched)
        y = pctx.vector()
        op.matvec(f, y)
        out.append((y, op.last_gmres["residuals"]))
    assert torch.equal(out[0][0].storage, out[1][0].storage) and out[0][1] == out[1][1]
    assert float(out[0][0].storage.abs().max()) > 0


def test_set_base_takes_effect_and_refusals(gpu):
    """lns.B is bound at construction: after lns.set_base(0.5 B) the same operator object gives the dense answer for
    0.5 B under the same gate, and another answer than before.  The new operator refuses a LinearisedConvection and a
    plain AdvectionDiffusion by name; the two parent classes still refuse a LinearisedNavierStokes; OrbitFlow still
    refuses the incompressible flow."""
    import test_gpu_coupled_resolvent as gc
    import test_gpu_resolvent as gr
    from nekstab_next_amd.orbit import OrbitFlow
    from nekstab_next_amd.resolvent import CoupledResolventOperator, IncompressibleResolventOperator, ResolventOperator

    name, omega = "box3d", irr.OMEGAS["box3d"][1]
    lns, pctx = _build(name, *SOLVE_STEPS[name], max_cols=200)        # its own: the base state changes
    co, mask, ns, B, dt, nsteps = _case(name)
    op = IncompressibleResolventOperator(pctx, lns, omega, tol=1e-13, kdim=200, maxiter=4)
    before = _against_dense(op, pctx, lns, _dense(name, omega), "box3d B", adjoint=False)
    assert lns.set_base([0.5 * b for b in B]) is lns
    after = _against_dense(op, pctx, lns, irr.IncompressibleResolvent(ns, 0.5 * B, dt, nsteps, omega), "box3d B/2",
                           adjoint=False)
    assert np.max(np.abs(after - before)) > 1e-3 * np.max(np.abs(after))
    lin, lpctx = gc._lin("odd")
    with pytest.raises(ValueError, match="IncompressibleResolventOperator.*LinearisedNavierStokes.*LinearisedConvection"):
        IncompressibleResolventOperator(lpctx, lin, omega)
    adv, apctx = gr._adv("odd")
    with pytest.raises(ValueError, match="IncompressibleResolventOperator.*LinearisedNavierStokes.*AdvectionDiffusion"):
        IncompressibleResolventOperator(apctx, adv, omega)
    with pytest.raises(ValueError, match="ResolventOperator.*LinearisedNavierStokes"):
        ResolventOperator(pctx, lns, omega)
    with pytest.raises(ValueError, match="CoupledResolventOperator.*LinearisedNavierStokes"):
        CoupledResolventOperator(pctx, lns, omega)
    flow = gi._flow(4)[1]
    with pytest.raises(ValueError, match="OrbitFlow.*IncompressibleFlow"):
        OrbitFlow(flow)


def test_resolvent_analysis_on_the_incompressible_stepper(gpu, tmp_path):
    """drivers.resolvent_analysis, unchanged, on the 2-D case at omega = 2, inner tol 1e-13: the leading gain within
    1e-10 relative of the dense singular value.  k_dim = 2 and a seed that is the dense leading right singular vector
    plus 1e-6 of a hashed vector keep it to four inner solves: the Ritz value's error is the square of the seed's
    (1e-12) times (sigma_2 / sigma_1)^2 = 0.53 per step.  (Next to the eigenfrequency, omega = 0.56, the inner
    GMRES stalls at 2.7e-13 relative for this seed and the operator raises, as it must.)"""
    from nekstab_next_amd.drivers import resolvent_analysis
    from nekstab_next_amd.resolvent import IncompressibleResolventOperator

    name = "case2d"
    lns, pctx = _solver(name)
    omega = irr.OMEGAS[name][1]
    dense = _dense(name, omega)
    Q, A = dense.reduced()
    _, s, Vh = np.linalg.svd(np.linalg.inv(1j * omega * np.eye(A.shape[0]) - A))
    assert s[1] / s[0] < 0.8
    v = dense.ns.expand(Q @ Vh[0].conj())
    op = IncompressibleResolventOperator(pctx, lns, omega, tol=1e-13, kdim=200, maxiter=4)
    noise, seed = pctx.vector(), _upload(pctx, v / np.sqrt(float(dense.dot(v, v))))
    noise.fill_hash(17)
    seed.axpby(1.0, noise, 1e-6 / float(np.sqrt(pctx.dot(noise, noise, time=False))))
    out = resolvent_analysis(pctx, op, seed, k_dim=2, nev=1, tolerance=1e-6, outdir=str(tmp_path))
    print("gains", out["sigma2"][:2], "dense", s[:2] ** 2, "relative distance", abs(out["sigma2"][0] - s[0] ** 2) / s[0] ** 2,
          "residuals", out["residuals"][:2])
    np.testing.assert_allclose(out["sigma2"][0], s[0] ** 2, rtol=1e-10)
    assert np.loadtxt(tmp_path / "Spectrum_Sr.dat").shape == (2, 2)


# ---- two ranks -------------------------------------------------------------------------------------------
def _job(rank, world, fz):
    """One matvec of the forcing ``fz`` (global complex fields) on this rank's slice of the 2-D case: (the complex
    fields, the element range, the counts of the last pair projection)."""
    from nekstab_next_amd.comm import Comm
    from nekstab_next_amd.resolvent import IncompressibleResolventOperator

    comm = Comm()
    assert comm.world == world and comm.rank == rank
    name = "case2d"
    lns, pctx = _build(name, *SOLVE_STEPS[name], comm=comm, max_cols=64)
    lay = lns.ctx.layout
    e0, e1 = lay.elem_range()
    sl = slice(e0 * lay.pts_v, e1 * lay.pts_v)
    op = IncompressibleResolventOperator(pctx, lns, irr.OMEGAS[name][1], tol=1e-13, kdim=60, maxiter=2)
    f, y = _upload(pctx, fz[:, sl]), pctx.vector()
    op.matvec(f, y)
    return _download(pctx, y), (e0, e1), op.projector.last_iterations_each


def _rank_main(rank, world, port, out, fz):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        out[rank] = _job(rank, world, fz)
    finally:
        dist.destroy_process_group()


def test_two_ranks_against_dense_answer(gpu):
    """Two gloo ranks sharing the GPU (the 2-D mesh split 5 + 4 elements): the matvec equals the dense answer, and
    so the one-rank answer, under the dense gate.  Bits are not asked for: the all-reduce sums in another order.
    Every CG iteration is two all-reduces through the host here, so the forcing is a combination of six
    eigenvectors of P L_B, for which the inner GMRES ends within about twelve iterations."""
    name = "case2d"
    dense = _dense(name, irr.OMEGAS[name][1])
    fz = dense.modal_forcing(6)
    want = dense.dense_apply(fz)
    out = mp.Manager().dict()
    ctx = mp.get_context("spawn")
    port = ga._free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, out, fz)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join()
    assert [p.exitcode for p in procs] == [0, 0]
    pts, sizes = NekLayout(**LAYOUTS[name]).pts_v, []
    for r in range(2):
        got, (e0, e1), its = out[r]
        sizes.append(e1 - e0)
        d = float(np.max(np.abs(got - want[:, e0 * pts: e1 * pts])) / np.max(np.abs(want)))
        print(f"rank {r}: elements {e0}..{e1}, distance from the dense answer {d:.2e} (gate {GATE:.1e}), last CG counts {its}")
        assert d <= GATE and min(its) > 0
    assert sorted(sizes) == [4, 5] and np.max(np.abs(want)) > 0
