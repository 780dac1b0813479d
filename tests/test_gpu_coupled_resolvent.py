"""The coupled time-stepper resolvent on the device (nkv_linconv_crhs in csrc/advdiff.hip, CoupledResolventOperator
in nekstab_next_amd/resolvent.py) against the two nkv_linconv_rhs launches it replaces, its NumPy restatement
(tests/coupled_resolvent_reference.py) and the dense (i omega - J)^-1 of the linearised convection.

The fused right-hand side is compared bit for bit with nkv_linconv_rhs on each half.  Runs of the stepper are held
to the project's gate for everything differentiated twice (tests/test_gpu_advdiff.py: ``_gate``, max(8 e_ref,
1e-12 scale) with e_ref the distance of the f64 from the long double restatement).  The operator is held to the
dense solve: 4 times the distance of the f64 restatement of the same algorithm from that solve
(coupled_resolvent_reference.DENSE_DISTANCE, measured by tests/test_coupled_resolvent.py on the CPU), with 1e-11
relative as the floor; the adjoint identity to 4 times ADJOINT_DEFECT: the margins of tests/test_gpu_resolvent.py."""
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
import coupled_resolvent_reference as cr
import test_gpu_advdiff as ga
import test_gpu_burgers as gb
import test_gpu_resolvent as gr
from test_gpu_resolvent import _check_rest, _check_zeroed, _download, _gate_complex, _random_complex, _upload

from nekstab_next_amd import _lib
from nekstab_next_amd import synthetic as syn
from nekstab_next_amd.layout import NekLayout
from nekstab_next_amd.sensitivity import gll_derivative

ROOT = ga.ROOT
pytestmark = pytest.mark.gpu

BOX3D = cr.BOX3D
SHAPES = ["cell", "odd", BOX3D]
GATE = max(4 * cr.DENSE_DISTANCE, 1e-11)


# ---- cases -------------------------------------------------------------------------------------------
def _case(name):
    """(global layout, coordinates, base state of n_wf fields, wall mask, kappas, dt, nsteps): the cases of
    test_gpu_resolvent.py; the base state is the case's own flow, in 3-D with test_gpu_burgers.py's scalar."""
    lay, co, U, mask, kap, dt, nsteps = gr._case(name)
    B = [np.asarray(u, dtype=np.float64) for u in U] if lay.ldim == 2 else gb._case(name)[2]
    assert len(B) == lay.n_wf
    return lay, co, B, mask, kap, dt, nsteps


_BG, _LINS = {}, {}


def _restatements(name):
    """The f64 and long double Burgers restatements of a case (built once)."""
    if name not in _BG:
        lay, co, B, mask, kap, dt, nsteps = _case(name)
        zero = [np.zeros(lay.n_v)] * lay.ldim
        _BG[name] = tuple(br.Burgers(ar.Reference(lay.lx1, lay.ldim, co, zero, mask=mask, dtype=t), kap, dt, nsteps)
                          for t in (np.float64, np.longdouble))
    return _BG[name]


def _build(name, batched=False, nsteps=None, comm=None):
    """(LinearisedConvection, pair context) of a case, or of this rank's shard of it."""
    from nekstab_next_amd.burgers import LinearisedConvection
    from nekstab_next_amd.gs import GatherScatter
    from nekstab_next_amd.resolvent import pair_context
    from nekstab_next_amd.vector import NekContext

    lay_g, co, B, mask, kap, dt, ns = _case(name)
    ctx = NekContext(lay_g, max_cols=4) if comm is None else NekContext(lay_g, comm=comm, max_cols=4)
    e0, e1 = ctx.layout.elem_range() if comm is not None else (0, lay_g.nelv)
    sl = slice(e0 * lay_g.pts_v, e1 * lay_g.pts_v)
    co = {k: v[sl] for k, v in co.items()}
    lin = LinearisedConvection(ctx, co, [b[sl] for b in B], kap, dt, ns if nsteps is None else nsteps,
                               mask=mask[sl], face_average=GatherScatter(ctx, co) if batched else "auto")
    return lin, pair_context(lin)


def _lin(name, batched=False):
    """Built once per case on one rank; the tests that change the base state build their own."""
    if (name, batched) not in _LINS:
        _LINS[(name, batched)] = _build(name, batched)
    return _LINS[(name, batched)]


# ---- nkv_linconv_crhs against two nkv_linconv_rhs ------------------------------------------------------
class _Raw(gb._Raw):
    """nkv_linconv_rhs and nkv_linconv_crhs on one mesh; "odd" (not a mesh of test_gpu_advdiff.py) is built here."""

    def __init__(self, name):
        if name != "odd":
            super().__init__(name)
            return
        from nekstab_next_amd.vector import NekContext

        lay, co, B, _, kap = _case(name)[:5]
        self.lay, self.co, self.kap, self.Bh = lay, co, list(kap), B
        self.ctx = NekContext(lay, max_cols=4)
        self.n, self.pts = lay.n_v, lay.pts_v
        self.D, self.w = ga._dev(gll_derivative(lay.lx1)), ga._dev(syn.gll_weights(lay.lx1))
        self.xyz = [ga._dev(co[k]) for k in ("x", "y")]
        self.B = ga._dev(np.concatenate(B))
        self.st = torch.cuda.current_stream().cuda_stream

    def clin(self, u, u_stride, r, r_stride, kappa, adjoint, e0=0, e1=None):
        """nkv_linconv_crhs on elements [e0, e1) of pair buffers: the im half n_v doubles behind the re half."""
        lay, n = self.lay, self.n
        e1 = n // self.pts if e1 is None else e1
        L = lay.c_struct()
        L.n_v = (e1 - e0) * self.pts
        off = 8 * e0 * self.pts
        xyz = [t.data_ptr() + off for t in self.xyz] + ([None] if lay.ldim == 2 else [])
        rc = self.ctx.lib.nkv_linconv_crhs(ctypes.byref(L), lay.lx1, lay.ldim, self.D.data_ptr(), self.w.data_ptr(), *xyz,
                                           self.B.data_ptr() + off, n, kappa.data_ptr(), u.data_ptr() + off,
                                           u.data_ptr() + 8 * n + off, lay.n_wf, u_stride, r.data_ptr() + off,
                                           r.data_ptr() + 8 * n + off, r_stride, int(adjoint), self.st)
        assert rc == _lib.NKV_OK, _lib.last_error()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", ["odd", "cell", "cyl"] + gb.CASES_3D, ids=str)
def test_crhs_bits(gpu, name):
    """Forward and adjoint: both halves of the fused pass carry the bits of nkv_linconv_rhs on that half ("odd":
    n_v = 81, the im half only 8-byte aligned; lx1 = 10, the LDS limit; lx1 = 2; one- and seven-element groups with
    a partial last group).  The pair stride is above 2 n_v and the NaN gap stays untouched; a second call and
    element sub-ranges give the same bits; the inputs are unchanged bit for bit."""
    raw = _Raw(name)
    lay, n, pts = raw.lay, raw.n, raw.pts
    nf = lay.n_wf
    stride = 2 * n + 25
    rng = np.random.default_rng(11)
    fields = ga._fields(lay, raw.co)
    host = np.full(nf * stride, np.nan)
    for f in range(nf):
        host[f * stride: f * stride + n] = fields[f]
        host[f * stride + n: f * stride + 2 * n] = fields[(f + 1) % nf][::-1] + 0.1 * rng.standard_normal(n)
    u = ga._dev(host)
    kd = ga._dev(raw.kap)
    B0 = raw.B.clone()
    E = n // pts
    nan = lambda: torch.full((nf * stride,), float("nan"), dtype=torch.float64, device="cuda")   # noqa: E731
    if n % 2:
        assert (u.data_ptr() + 8 * n) % 16 == 8
    for adjoint in (False, True):
        want = nan()
        raw.lin(u, stride, want, stride, kd, adjoint)                  # the re half
        raw.lin(u[n:], stride, want[n:], stride, kd, adjoint)          # the im half
        want = want.cpu().numpy().reshape(nf, stride)
        assert np.all(np.isfinite(want[:, :2 * n])) and np.all(np.isnan(want[:, 2 * n:]))
        assert np.max(np.abs(want[:, :n] - want[:, n:2 * n])) > 0      # the halves differ
        out = nan()
        raw.clin(u, stride, out, stride, kd, adjoint)
        got = out.cpu().numpy().reshape(nf, stride)
        assert _same(got[:, :n], want[:, :n]), f"{name} adjoint={adjoint}: re half"
        assert _same(got[:, n:2 * n], want[:, n:2 * n]), f"{name} adjoint={adjoint}: im half"
        assert np.all(np.isnan(got[:, 2 * n:]))                         # the gap is untouched
        again = nan()
        raw.clin(u, stride, again, stride, kd, adjoint)
        assert _same(again.cpu().numpy().reshape(nf, stride), got)
        for e0, e1 in {(0, max(E // 2, 1)), (E // 2, E), (E - 1, E)}:
            part = nan()
            raw.clin(u, stride, part, stride, kd, adjoint, e0, e1)
            p = part.cpu().numpy().reshape(nf, stride)
            for h in (0, n):
                assert np.array_equal(p[:, h + e0 * pts:h + e1 * pts], got[:, h + e0 * pts:h + e1 * pts])
                assert np.all(np.isnan(p[:, h:h + e0 * pts])) and np.all(np.isnan(p[:, h + e1 * pts:h + n]))
            assert np.all(np.isnan(p[:, 2 * n:]))
    assert _same(u.cpu().numpy(), host) and torch.equal(raw.B, B0)     # the inputs are read only


def test_crhs_entry_checks(gpu):
    """Every NKV_EINVAL of nkv_linconv_crhs names its argument and launches nothing; an empty shard returns
    NKV_OK and reads no pointer."""
    lay = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=3, n_scalars=1)
    n, nf = lay.n_v, lay.n_wf
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.full((28 * n,), 7.0, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    L = lay.c_struct()
    u_re, u_im, B, r_re, r_im = (p + 8 * k * n for k in (4, 8, 12, 16, 20))
    last = 8 * (nf - 1) * n + 8 * (n - 1)                             # the last double of a span
    V = dict(L=ctypes.byref(L), lx1=4, ldim=3, D=p, w=p, xm=p, ym=p, zm=p, B=B, B_stride=n, kappa=p, u_re=u_re, u_im=u_im,
             nfld=nf, u_stride=n, r_re=r_re, r_im=r_im, r_stride=n, adjoint=0, stream=st)
    bad = [("ldim", 4, "ldim"), ("lx1", 11, "lx1"), ("zm", None, "zm"), ("u_stride", n - 1, "u_stride"),
           ("r_stride", n - 1, "r_stride"), ("B_stride", n - 1, "B_stride"), ("nfld", 2, "nfld=2 < ldim=3"),
           ("D", None, "D is NULL"), ("w", None, "w is NULL"), ("xm", None, "xm is NULL"), ("ym", None, "ym is NULL"),
           ("B", None, "B is NULL"), ("kappa", None, "kappa is NULL"), ("u_re", None, "u_re is NULL"),
           ("u_im", None, "u_im is NULL"), ("r_re", None, "r_re is NULL"), ("r_im", None, "r_im is NULL"),
           ("r_re", r_im, "r_re overlaps r_im"), ("r_im", r_re + last, "r_re overlaps r_im"),
           ("r_im", r_re - last, "r_re overlaps r_im"),
           ("r_re", u_re, "r_re overlaps"), ("r_re", u_im + last, "r_re overlaps"), ("r_re", B - last, "r_re overlaps"),
           ("r_im", u_re + last, "r_im overlaps"), ("r_im", u_im, "r_im overlaps"), ("r_im", B, "r_im overlaps")]
    for adjoint in (0, 1):
        for key, val, msg in bad:
            assert lib.nkv_linconv_crhs(*{**V, "adjoint": adjoint, key: val}.values()) == _lib.NKV_EINVAL, key
            assert msg in _lib.last_error() and "linconv_crhs" in _lib.last_error(), (key, _lib.last_error())
    # the halves of a pair vector interleave: accepted at im = re + n_v, refused one double closer
    pair = {**V, "r_stride": 2 * n, "r_im": r_re + 8 * (n - 1)}
    assert lib.nkv_linconv_crhs(*pair.values()) == _lib.NKV_EINVAL and "r_re overlaps r_im" in _lib.last_error()
    Lbad = lay.c_struct()
    Lbad.n_v = n - 1                                                  # not whole elements
    assert lib.nkv_linconv_crhs(*{**V, "L": ctypes.byref(Lbad)}.values()) == _lib.NKV_EINVAL
    torch.cuda.synchronize()
    assert torch.all(buf == 7.0)                                     # nothing was launched
    Le = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=0, n_scalars=1).c_struct()
    empty = {**V, "L": ctypes.byref(Le), "D": None, "w": None, "xm": None, "ym": None, "zm": None, "B": None,
             "kappa": None, "u_re": None, "u_im": None, "r_re": None, "r_im": None}
    assert lib.nkv_linconv_crhs(*empty.values()) == _lib.NKV_OK
    torch.cuda.synchronize()
    assert torch.all(buf == 7.0)


# ---- the stepper against the restatement -------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES, ids=str)
def test_runs_against_restatement(gpu, name):
    """project, forced_run and propagate, direct and adjoint, at omega = 1 (0 on the 3-D case) against the
    restatement in f64 and long double; pressure rows and time zeroed, padding untouched; in place equals out of
    place; the forcing is read only."""
    from nekstab_next_amd.resolvent import CoupledResolventOperator

    lin, pctx = _lin(name)
    lay, _, B, _, _, dt, nsteps = _case(name)
    omega = 0.0 if name == BOX3D else 1.0
    op = CoupledResolventOperator(pctx, lin, omega)
    r64, rld = (cr.CoupledResolvent(bg, np.stack(B), dt, nsteps, omega) for bg in _restatements(name))
    assert abs(op.tau - nsteps * dt) <= 1e-15 * op.tau
    x = _upload(pctx, _random_complex(lay.n_wf, lay.n_v, 7), pressure=1.0, time=3.0)
    xz = _download(pctx, x)
    f = _upload(pctx, 0 * xz, pressure=7.0, time=7.0, fill=7.0)
    op.project(x, f)
    _check_rest(pctx.layout, f.to_packed())
    fz = _download(pctx, f)
    _gate_complex(fz, r64.project(xz), rld.project(xz), f"{name} project")
    inplace = pctx.vector()
    inplace.copy_from(x)
    op.project(inplace)
    assert np.array_equal(_download(pctx, inplace), fz)
    for adjoint in (False, True):
        b = _upload(pctx, 0 * xz, pressure=7.0, time=7.0)
        op.forced_run(f, b, adjoint)
        _check_zeroed(pctx.layout, b.to_packed())
        _gate_complex(_download(pctx, b), r64.forced_run(fz, adjoint), rld.forced_run(fz, adjoint),
                      f"{name} forced_run adjoint={adjoint}")
        y = _upload(pctx, 0 * xz, pressure=7.0, time=7.0, fill=7.0)
        y.copy_from(x)                                               # pressure 1, time 3 in x
        op.propagate(x, y, adjoint)
        _check_zeroed(pctx.layout, y.to_packed())
        op.propagate(f, y, adjoint)
        got = _download(pctx, y)
        _gate_complex(got, r64.propagate(fz, adjoint), rld.propagate(fz, adjoint), f"{name} propagate adjoint={adjoint}")
        y2 = pctx.vector()
        y2.copy_from(f)
        op.propagate(y2, y2, adjoint)                                # in place
        assert np.array_equal(_download(pctx, y2), got)
        assert np.array_equal(_download(pctx, f), fz)               # the forcing is read only
    with pytest.raises(ValueError):
        op.forced_run(f, f)


# ---- the operator against the dense inverse ------------------------------------------------------------
def _against_dense(op, pctx, lin, dense, lay, what, identity=True):
    """matvec / rmatvec of random unprojected f, g against the dense solves under GATE and, with ``identity``
    (the cases ADJOINT_DEFECT was measured on), the adjoint identity in the pair bm1 product of the context under
    4 ADJOINT_DEFECT.  Returns the downloaded matvec."""
    fz, gz = _random_complex(lay.n_wf, lay.n_v, 4), _random_complex(lay.n_wf, lay.n_v, 5)
    f, g = _upload(pctx, fz, pressure=1.0, time=2.0), _upload(pctx, gz)
    y, ya = _upload(pctx, 0 * fz, pressure=7.0, time=7.0), pctx.vector()
    op.matvec(f, y)
    info = op.last_gmres
    assert info["info"] == 0 and info["adjoint"] is False and info["residuals"][-1] <= 1e-13 * info["residuals"][0]
    _check_zeroed(pctx.layout, y.to_packed())
    op.rmatvec(g, ya)
    assert op.last_gmres["info"] == 0 and op.last_gmres["adjoint"] is True
    for got, want, side in ((_download(pctx, y), dense.dense_apply(fz), "matvec"),
                            (_download(pctx, ya), dense.dense_apply(gz, adjoint=True), "rmatvec")):
        d = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f"{what} {side}: distance from the dense solve {d:.2e} (gate {GATE:.1e})")
        assert np.max(np.abs(want)) > 0 and d <= GATE, (what, side, d)
    lhs, rhs = pctx.dot(y, g, time=False), pctx.dot(f, ya, time=False)
    yz = _download(pctx, y)
    scale = float(np.sum(lin.bm1.cpu().numpy() * (np.abs(yz.real * gz.real) + np.abs(yz.imag * gz.imag))))
    print(f"{what} adjoint identity: {abs(lhs - rhs) / scale:.2e} (gate {4 * cr.ADJOINT_DEFECT:.1e})")
    assert scale > 0 and (abs(lhs - rhs) <= 4 * cr.ADJOINT_DEFECT * scale or not identity)
    return yz


@pytest.mark.parametrize("name,omega", [("cell", 0.0), ("cell", 1.0), ("odd", 0.0), ("odd", 1.0)], ids=str)
def test_operator_against_dense_inverse(gpu, name, omega):
    """matvec / rmatvec at inner tol = 1e-13 against the dense (±i omega - J)^-1 Pi f on all fields (gate: module
    docstring), and <R f, g> = <f, R† g>."""
    from nekstab_next_amd.resolvent import CoupledResolventOperator

    lin, pctx = _lin(name)
    lay, _, B, _, _, dt, nsteps = _case(name)
    op = CoupledResolventOperator(pctx, lin, omega, tol=1e-13)
    dense = cr.CoupledResolvent(_restatements(name)[0], np.stack(B), dt, nsteps, omega)
    _against_dense(op, pctx, lin, dense, lay, f"{name} omega {omega}")


def test_set_base_takes_effect_and_refusals(gpu):
    """lin.B is bound at construction: after lin.set_base(0.5 B) the same operator object gives the dense answer
    for 0.5 B under the same gate, and another answer than before.  CoupledResolventOperator refuses a plain
    AdvectionDiffusion; ResolventOperator still refuses the linearised convection."""
    from nekstab_next_amd.resolvent import CoupledResolventOperator, ResolventOperator

    name, omega = "odd", 1.0
    lin, pctx = _build(name)                                          # its own: the base state changes
    lay, _, B, _, _, dt, nsteps = _case(name)
    op = CoupledResolventOperator(pctx, lin, omega, tol=1e-13)
    bg = _restatements(name)[0]
    before = _against_dense(op, pctx, lin, cr.CoupledResolvent(bg, np.stack(B), dt, nsteps, omega), lay, "odd B")
    assert lin.set_base([0.5 * b for b in B]) is lin
    after = _against_dense(op, pctx, lin, cr.CoupledResolvent(bg, 0.5 * np.stack(B), dt, nsteps, omega), lay, "odd B/2",
                           identity=False)
    assert np.max(np.abs(after - before)) > 0.1 * np.max(np.abs(after))
    adv, apctx = gr._adv(name)
    with pytest.raises(ValueError, match="LinearisedConvection"):
        CoupledResolventOperator(apctx, adv, omega)
    with pytest.raises(ValueError, match="production term") as info:
        ResolventOperator(pctx, lin, omega)
    assert "CoupledResolventOperator" in str(info.value)


def test_resolvent_analysis_on_the_coupled_stepper(gpu, tmp_path):
    """drivers.resolvent_analysis, unchanged, on "odd" at omega = 1 with inner tol = 1e-13: the two leading
    distinct gains (287.90, 40.33), each twice, within GAIN_GATE of the dense weighted SVD and Spectrum_Sr.dat
    written with k_dim rows.  k_dim = ANALYSIS_KDIM and the gate are argued on the CPU
    (tests/test_coupled_resolvent.py).  ``info`` is taken at the driver's default tolerance 1e-6: at this k_dim
    the residual estimates of the leading four are at most 4.7e-8 over the 40 seeds of that study (the values
    converge as the square of the residuals).  The averages are batched (a one-rank GatherScatter): the launch
    count is what costs."""
    from nekstab_next_amd.drivers import resolvent_analysis
    from nekstab_next_amd.resolvent import CoupledResolventOperator

    lin, pctx = _lin("odd", batched=True)
    lay, _, B, _, _, dt, nsteps = _case("odd")
    op = CoupledResolventOperator(pctx, lin, 1.0, tol=1e-13)
    gains = cr.CoupledResolvent(_restatements("odd")[0], np.stack(B), dt, nsteps, 1.0).gains()
    for got, want in zip(gains, (287.90, 40.33, 7.17)):
        assert abs(got - want) <= 1e-3 * want
    seed = pctx.vector()
    seed.fill_hash(17)
    k_dim = cr.ANALYSIS_KDIM
    out = resolvent_analysis(pctx, op, seed, k_dim=k_dim, nev=4, tolerance=1e-6, outdir=str(tmp_path))
    exact = np.repeat(gains[:2], 2)
    print("gains", out["sigma2"][:4], "dense", exact, "relative distance", np.abs(out["sigma2"][:4] - exact) / exact,
          "residuals", out["residuals"][:4], "gate", cr.GAIN_GATE)
    assert out["info"] == 0
    np.testing.assert_allclose(out["sigma2"][:4], exact, rtol=cr.GAIN_GATE)
    data = np.loadtxt(tmp_path / "Spectrum_Sr.dat")
    assert data.shape == (k_dim, 2)
    np.testing.assert_allclose(data[:4, 0], exact, rtol=1e-6)


# ---- shards ------------------------------------------------------------------------------------------
def _jobs(rank, world):
    """On "cell", this rank's slice: nkv_linconv_crhs of the uploaded pair vector and propagate over 2 steps,
    direct and adjoint, and one matvec at inner tol 1e-13."""
    from nekstab_next_amd.comm import Comm
    from nekstab_next_amd.resolvent import CoupledResolventOperator

    comm = Comm()
    assert comm.world == world and comm.rank == rank
    lay_g = _case("cell")[0]
    lin2, pctx2 = _build("cell", nsteps=2, comm=comm)
    lin, pctx = _build("cell", comm=comm)
    lay = lin.ctx.layout
    e0, e1 = lay.elem_range()
    sl = slice(e0 * lay.pts_v, e1 * lay.pts_v)
    xz = _random_complex(lay_g.n_wf, lay_g.n_v, 9)[:, sl]
    op2 = CoupledResolventOperator(pctx2, lin2, 1.0)
    x, r, y = _upload(pctx2, xz), pctx2.vector(), pctx2.vector()
    out = {}
    psv, n = pctx2.layout.sv, lay.n_v
    for adjoint in (False, True):
        r.zero()
        lin2.ctx.call("nkv_linconv_crhs", *op2._crhs_head, x.ptr, x.ptr + 8 * n, lay.n_wf, psv, r.ptr, r.ptr + 8 * n, psv,
                      int(adjoint), pctx2.stream)
        out[f"r{int(adjoint)}"] = _download(pctx2, r)
        op2.propagate(x, y, adjoint)
        out[f"p{int(adjoint)}"] = _download(pctx2, y)
    op = CoupledResolventOperator(pctx, lin, 1.0, tol=1e-13)
    f, ym = _upload(pctx, xz), pctx.vector()
    op.matvec(f, ym)
    out["y"] = _download(pctx, ym)
    return out


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


def test_shards_equal_one_rank(gpu):
    """Two gloo ranks sharing the GPU: the fused right-hand side and propagate over 2 steps, direct and adjoint,
    equal the one-rank result bit for bit on every rank's slice; the matvec of each is within the operator gate
    of the dense solve."""
    one = _jobs(0, 1)
    out = mp.Manager().dict()
    ctx = mp.get_context("spawn")
    port = ga._free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join()
    assert [p.exitcode for p in procs] == [0, 0]
    got = dict(out)
    lay_g, _, B, _, _, dt, nsteps = _case("cell")
    want = cr.CoupledResolvent(_restatements("cell")[0], np.stack(B), dt, nsteps, 1.0).dense_apply(
        _random_complex(lay_g.n_wf, lay_g.n_v, 9))
    scale = float(np.max(np.abs(want)))
    assert scale > 0 and all(np.any(one[k] != 0) and np.all(np.isfinite(one[k])) for k in one)
    assert np.max(np.abs(one["y"] - want)) <= GATE * scale
    for r in range(2):
        sh = lay_g.shard(r, 2)
        e0, e1 = sh.elem_range()
        sl = slice(e0 * sh.pts_v, e1 * sh.pts_v)
        for k in ("r0", "r1", "p0", "p1"):
            np.testing.assert_array_equal(got[r][k], one[k][:, sl], err_msg=f"{k} rank {r}")
        d = float(np.max(np.abs(got[r]["y"] - want[:, sl]))) / scale
        print(f"rank {r}: matvec differs from the dense solve by {d:.2e} (gate {GATE:.1e})")
        assert d <= GATE
