"""The fast-diagonalisation preconditioner of the pressure CG on the device (nkv_pressure_precond, _precond2,
_pgradt, _pgradt2 in csrc/pressure.hip; DivergenceFreeProjector(preconditioner="fdm")) against its NumPy
restatement (tests/pressure_precond_reference.py).

Gates.  ``precondition`` against ``M(r)``: both apply 2 ldim line contractions of m terms and one scale whose
denominator is a sum of ldim products; to first order either differs from the exact ``M r`` by at most
(2 ldim m + ldim + 3) u times ``|S| .. diag(1/den) .. |S^T| |r|`` componentwise (u the unit roundoff), so the two
differ by at most twice that; the gate takes u = 2^-52.  The projector: 8 times the restatement's records for PCG
(``pressure_precond_reference.PROJECTOR``), the count within 1.25 times the restatement's.  The flow and one
resolvent matvec: 8 times the restatement's own CG-against-PCG difference (``FLOW_DIFFERENCE``,
``RESOLVENT_DIFFERENCE``).  Sub-ranges, repeated runs and the two-system solve are compared bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import advdiff_reference as ar
import incompressible_reference as ir
import pressure_precond_reference as pp
import test_gpu_advdiff as ga
import test_gpu_burgers as gb
import test_gpu_incompressible as gi

from nekstab_next_amd import _lib
from nekstab_next_amd.layout import NekLayout

pytestmark = pytest.mark.gpu
PI = np.pi
ROOT = ga.ROOT
TOL = 1e-13
EPS = 2.0 ** -52

APPLY_CASES = ["closed2d", "closed3d", "two3d_lx8", "odd2d", "thirty2d"]
_APPLY, _PROJ = {}, {}


def _apply_mesh(name):
    """(lx1, ldim, coords, mask) of an apply case: two meshes of ``projector_case`` (m = 3: 28 elements a workgroup,
    9 here; m = 2: 32 a workgroup, 8 here), 2 x 1 x 1 elements of lx1 = 8 deformed by 0.04 (m = 6, one element a
    workgroup), 3 x 3 elements of lx1 = 3 (m = 1: a pure scale) and 6 x 5 elements of lx1 = 5 (two workgroups,
    28 + 2 elements)."""
    if name in ("closed2d", "closed3d"):
        lx1, ldim, co, mask, _ = ir.projector_case(name)
        return lx1, ldim, co, mask
    if name == "two3d_lx8":
        from test_bf_sensitivity import deformed_box

        lay = NekLayout(ldim=3, lx1=8, lx2=6, nelgv=2)
        return 8, 3, deformed_box(lay, (2, 1, 1), amp=0.04), None
    if name == "odd2d":
        return 3, 2, ar.box_mesh_2d(3, (3, 3), (PI, PI), amp=0.04), None
    if name == "thirty2d":
        return 5, 2, ar.box_mesh_2d(5, (6, 5), (PI, PI), amp=0.04), None
    raise KeyError(name)


def _apply_case(name):
    """(projector with "fdm", PressureFDM) of an apply case, built once."""
    if name not in _APPLY:
        from nekstab_next_amd.pressure import DivergenceFreeProjector
        from nekstab_next_amd.vector import NekContext

        lx1, ldim, co, mask = _apply_mesh(name)
        n = co["x"].size
        lay = NekLayout(ldim=ldim, lx1=lx1, lx2=lx1 - 2, nelgv=n // lx1 ** ldim)
        ctx = NekContext(lay, max_cols=4)
        proj = DivergenceFreeProjector(ctx, co, mask=mask, closed=False, preconditioner="fdm")
        ref = ar.Reference(lx1, ldim, co, [np.zeros(n)] * ldim, mask=mask)
        _APPLY[name] = (proj, pp.PressureFDM(ref, co, closed=False))
    return _APPLY[name]


def _nan(size):
    return torch.full((size,), float("nan"), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name", APPLY_CASES)
def test_precondition_against_restatement(gpu, name):
    """``precondition`` under the gate of the module docstring; S, lambda and c are the restatement's; the partials of
    r.z and sum z add up; a second call and every element sub-range give the same bits and touch nothing else."""
    proj, pr = _apply_case(name)
    lay = proj.ctx.layout
    m, d, npz = lay.lx1 - 2, lay.ldim, pr.npz
    S, lam, c = pr.fdm_data()
    assert np.array_equal(proj.fdm_lambda.cpu().numpy(), lam) and np.array_equal(proj.fdm_S.cpu().numpy(), S)
    assert np.allclose(proj.fdm_c.cpu().numpy(), c, rtol=1e-14, atol=0) and np.all(lam > 0) and np.all(c > 0)
    r = np.random.default_rng(11).standard_normal(npz)
    rd, out = ga._dev(r), _nan(npz + 8)
    proj.precondition(rd, out)
    got = out.cpu().numpy()
    assert np.all(np.isnan(got[npz:]))
    want, bound = pr.M(r), pr.M(r, absolute=True)
    gate = 2 * (2 * d * m + d + 3) * EPS * bound
    err = np.abs(got[:npz] - want)
    print(f"{name}: max |device - M r| / gate {float(np.max(err / gate)):.3f}, max |M r| {float(np.max(np.abs(want))):.3e}")
    assert np.all(gate > 0) and np.all(err <= gate)
    again = _nan(npz + 8)
    proj.precondition(rd, again)
    assert np.array_equal(again.cpu().numpy()[:npz], got[:npz])
    # the raw entry: partials, sub-ranges
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    PB = lib.nkv_pressure_partials()
    pm, E = m ** d, npz // m ** d
    head = (lay.lx1, d, proj.fdm_S.data_ptr(), proj.fdm_lambda.data_ptr())

    def raw(e0, e1, z, part):
        rc = lib.nkv_pressure_precond(e1 - e0, *head, proj.fdm_c.data_ptr() + 8 * d * e0, rd.data_ptr() + 8 * pm * e0,
                                      z.data_ptr() + 8 * pm * e0, None if part is None else part.data_ptr(), st)
        assert rc == _lib.NKV_OK, _lib.last_error()

    part, z = torch.zeros(2 * PB, dtype=torch.float64, device="cuda"), _nan(npz)
    raw(0, E, z, part)
    assert np.array_equal(z.cpu().numpy(), got[:npz])
    sums = part.view(2, PB).sum(dim=1).cpu().numpy()
    assert abs(sums[0] - r @ got[:npz]) <= 1e-13 * float(np.abs(r) @ np.abs(got[:npz]))
    assert abs(sums[1] - got[:npz].sum()) <= 1e-13 * float(np.abs(got[:npz]).sum())
    for e0, e1 in {(0, max(E // 2, 1)), (E // 2, E), (E - 1, E), (1, E)}:
        z = _nan(npz)
        raw(e0, e1, z, None)
        g = z.cpu().numpy()
        assert np.array_equal(g[e0 * pm:e1 * pm], got[e0 * pm:e1 * pm])
        assert np.all(np.isnan(g[:e0 * pm])) and np.all(np.isnan(g[e1 * pm:]))
    # refusals
    assert lib.nkv_pressure_precond(E, *head, proj.fdm_c.data_ptr(), rd.data_ptr(), rd.data_ptr(), None, st) == _lib.NKV_EINVAL
    assert lib.nkv_pressure_precond(E, 11, d, *head[2:], proj.fdm_c.data_ptr(), rd.data_ptr(), z.data_ptr(), None,
                                    st) == _lib.NKV_EINVAL


# ---- the projector -----------------------------------------------------------------------------------
def _projector(name):
    """(ctx, the projector with "fdm" at tol 1e-13, Reference, PressureFDM, coordinates, mask), built once."""
    if name not in _PROJ:
        from nekstab_next_amd.pressure import DivergenceFreeProjector
        from nekstab_next_amd.vector import NekContext

        lx1, ldim, co, mask, ref, pr = pp.projector_pressure(name)
        lay = NekLayout(ldim=ldim, lx1=lx1, lx2=lx1 - 2, nelgv=ref.n // lx1 ** ldim, n_scalars=1 if ldim == 3 else 0)
        ctx = NekContext(lay, max_cols=4)
        proj = DivergenceFreeProjector(ctx, co, mask=mask, tol=TOL, preconditioner="fdm")
        _PROJ[name] = (ctx, proj, ref, pr, co, mask)
    return _PROJ[name]


@pytest.mark.parametrize("name", gi.PROJECTOR_CASES, ids=str)
def test_projector_fdm(gpu, name):
    """``test_gpu_incompressible.test_projector`` with the preconditioner: every figure within 8 times the
    restatement's PCG record, 0 < iterations <= 1.25 times the restatement's; the same bits again; b = 0 gives 0
    iterations and the input back; a non-finite input raises."""
    ctx, proj, ref, pr, co, mask = _projector(name)
    lay = ctx.layout
    d, n = lay.ldim, lay.n_v
    rec = pp.PROJECTOR[name]
    assert proj.closed == pr.closed == (name != "open2d") and proj.preconditioner == "fdm"
    x, v = gi._state(ctx, ref, 5)
    dense = pr.project(v)
    scale = float(np.max(np.abs(v)))
    y = ga._sentinel(ctx)
    proj.apply(x, y)
    its = proj.last_iterations
    got, xin = y.to_packed(), x.to_packed()
    Pv = gb._rows(lay, got)[:d]
    assert np.array_equal(got[d * lay.sv: lay.time_offset + 1], xin[d * lay.sv: lay.time_offset + 1])
    dist_ = float(np.max(np.abs(Pv - dense))) / scale
    print(f"{name}: distance to the dense projection {dist_:.3e} (record {rec['dist']:.1e}), iterations {its} "
          f"(record {rec['iterations']})")
    div0, div1 = proj.divergence(x).cpu().numpy(), proj.divergence(y).cpu().numpy()
    ratio = float(np.max(np.abs(div1)) / np.max(np.abs(div0)))
    print(f"{name}: |Z D P v| / |Z D v| {ratio:.3e} (record {rec['div']:.1e})")
    y2 = ga._sentinel(ctx)
    proj.apply(y, y2)
    twice = float(np.max(np.abs(gb._rows(lay, y2.to_packed())[:d] - Pv))) / scale
    print(f"{name}: second projection moves {twice:.3e} (record {rec['twice']:.1e}), iterations {proj.last_iterations}")
    xw, w = gi._state(ctx, ref, 6)
    yw = ctx.vector()
    proj.apply(xw, yw)
    Pw = gb._rows(lay, yw.to_packed())[:d]
    bm = ref.bm1
    sa = abs(float(np.sum(bm * w * Pv) - np.sum(bm * Pw * v))) / float(np.sum(bm * np.abs(w) * np.abs(Pv)))
    print(f"{name}: self-adjointness defect {sa:.3e} (record {rec['selfadj']:.1e})")
    assert dist_ <= 8 * rec["dist"]
    assert 0 < its <= 1.25 * rec["iterations"]
    assert ratio <= 8 * rec["div"]
    assert twice <= 8 * rec["twice"]
    assert sa <= 8 * rec["selfadj"]
    # the same bits again
    y3 = ga._sentinel(ctx)
    proj.apply(x, y3)
    assert torch.equal(y3.storage, y.storage) and proj.last_iterations == its
    # b = 0; a non-finite input
    zero = ctx.vector()
    proj.apply(zero)
    assert proj.last_iterations == 0 and float(zero.storage.abs().max()) == 0.0
    bad = ctx.vector()
    bad.copy_from(x)
    bad.storage[3] = float("inf")
    with pytest.raises(RuntimeError, match="not finite"):
        proj.apply(bad)


def test_maxiter_raises_fdm(gpu):
    from nekstab_next_amd.pressure import DivergenceFreeProjector

    ctx, _, ref, _, co, mask = _projector("closed2d")
    proj = DivergenceFreeProjector(ctx, co, mask=mask, tol=TOL, maxiter=3, preconditioner="fdm")
    x, _ = gi._state(ctx, ref, 5)
    with pytest.raises(RuntimeError, match="maxiter=3"):
        proj.apply(x)
    assert proj.last_iterations == 3
    with pytest.raises(ValueError, match="preconditioner"):
        DivergenceFreeProjector(ctx, co, mask=mask, preconditioner="jacobi")
    with pytest.raises(RuntimeError, match="preconditioner=None"):
        gi._projector("closed2d")[1].precondition(proj._r, proj._x)


@pytest.mark.parametrize("name", ["big2d", "big3d"])
def test_fdm_halves_the_iterations(gpu, name):
    """On 6 x 6 elements of lx1 = 6 and on 3 x 3 x 3 of lx1 = 6 (closed, deformed by 0.04) the device's PCG needs at
    most half the iterations of the device's CG (tol = 1e-12, tested every 8), and both land within 1.25 times the
    restatement's counts."""
    from nekstab_next_amd.pressure import DivergenceFreeProjector
    from nekstab_next_amd.vector import NekContext

    lx1, ldim, ne, co, mask, ref = pp.iteration_case(name)
    lay = NekLayout(ldim=ldim, lx1=lx1, lx2=lx1 - 2, nelgv=int(np.prod(ne)))
    ctx = NekContext(lay, max_cols=4)
    x, _ = gi._state(ctx, ref, 5)
    its = []
    for pre in (None, "fdm"):
        proj = DivergenceFreeProjector(ctx, co, mask=mask, tol=1e-12, preconditioner=pre)
        assert proj.closed
        proj.apply(x, ctx.vector())
        its.append(proj.last_iterations)
    print(f"{name}: device iterations CG {its[0]}, PCG {its[1]} (restatement {pp.ITERATIONS[name]})")
    assert 0 < its[1] <= 0.5 * its[0]
    assert its[0] <= 1.25 * pp.ITERATIONS[name][0] and its[1] <= 1.25 * pp.ITERATIONS[name][1]


# ---- the two-system solve ------------------------------------------------------------------------------
def _pair_states(ctx, ref, pr, seed):
    """Two states whose preconditioned solves stop at different checks: a random Pi-projected velocity, and the
    correction of a multiplier that combines 6 eigenvectors of (Z M Z) E~ (largest eigenvalues): the Krylov space of
    the preconditioned iteration on its right-hand side has dimension 6, so PCG ends at the first check."""
    lay = ctx.layout
    a, _ = gi._state(ctx, ref, seed)
    E = pr.dense_E().astype(np.float64)
    Zm = np.eye(pr.npz) - (1.0 / pr.npz if pr.closed else 0.0)
    Et, Mt = Zm @ (0.5 * (E + E.T)) @ Zm, Zm @ pr.dense_M() @ Zm
    Mt = 0.5 * (Mt + Mt.T)
    # (Z M Z) E~ v = mu v  <=>  E~ v = mu (Z M Z)^+ v; on the mean-free space both are definite: solve it as the
    # symmetric problem of L^T E~ L with Z M Z = L L^T
    lamM, Q = np.linalg.eigh(Mt)
    keep = lamM > 1e-10 * lamM.max()
    L = Q[:, keep] * np.sqrt(lamM[keep])
    mu, W = np.linalg.eigh(L.T @ Et @ L)
    V = L @ W[:, -6:]
    phi = V @ (1.0 + np.arange(6))
    rng = np.random.default_rng(seed + 1)
    rows = list(pr.correction(phi)) + [rng.standard_normal(ref.n) for _ in range(lay.n_wf - lay.ldim)]
    return a, gb._vector(ctx, rows)


@pytest.mark.parametrize("name", gi.PROJECTOR_CASES, ids=str)
def test_project_pair_ptr_fdm(gpu, name):
    """Both halves equal ``project_ptr`` with "fdm" on each alone, bit for bit, with the same counts, which differ
    (the freeze is exercised), in either order, in place and out of place; a zero half is frozen from the start."""
    ctx, proj, ref, pr, co, mask = _projector(name)
    lay = ctx.layout
    a, b = _pair_states(ctx, ref, pr, 21)
    want, its = [], []
    for v in (a, b):
        y = ctx.vector()
        proj.apply(v, y)
        want.append(y)
        its.append(proj.last_iterations)
    print(f"{name}: single iteration counts {its}")
    assert its[0] > its[1] > 0
    sv = lay.sv
    for order in ((0, 1), (1, 0)):
        src = [(a, b)[k] for k in order]
        ya, yb = ga._sentinel(ctx), ga._sentinel(ctx)
        proj.project_pair_ptr(src[0].ptr, src[1].ptr, sv, ya.ptr, yb.ptr)
        assert proj.last_iterations_each == tuple(its[k] for k in order) and proj.last_iterations == max(its)
        for got, k in ((ya, order[0]), (yb, order[1])):
            assert torch.equal(got.storage[: lay.ldim * sv].view(lay.ldim, sv)[:, : lay.n_v],
                               want[k].storage[: lay.ldim * sv].view(lay.ldim, sv)[:, : lay.n_v])
            assert torch.all(got.storage[lay.ldim * sv:] == 7.0)
    ia, ib = ctx.vector(), ctx.vector()
    ia.copy_from(a)
    ib.copy_from(b)
    proj.project_pair_ptr(ia.ptr, ib.ptr, sv)
    assert torch.equal(ia.storage, want[0].storage) and torch.equal(ib.storage, want[1].storage)
    zero = ctx.vector()
    ia.copy_from(a)
    proj.project_pair_ptr(zero.ptr, ia.ptr, sv)
    assert proj.last_iterations_each == (0, its[0]) and float(zero.storage.abs().max()) == 0.0
    assert torch.equal(ia.storage, want[0].storage)


# ---- the flow ------------------------------------------------------------------------------------------
def test_flow_with_fdm_against_plain(gpu):
    """``IncompressibleFlow.propagate`` over 2 steps from the Newton starting point of ``case2d`` with "fdm" against
    the same flow with None, within 8 times the restatement's own CG-against-PCG difference; the linearisation the
    flow builds carries the preconditioner."""
    from nekstab_next_amd.incompressible import IncompressibleFlow
    from nekstab_next_amd.vector import NekContext

    c = ir.CASE
    co, mask, n64, qt, q0, target, pert = ir.case2d(np.float64, 2)
    lay = NekLayout(ldim=2, lx1=c["lx1"], lx2=c["lx1"] - 2, nelgv=9)
    ctx = NekContext(lay, max_cols=4)
    out = []
    for pre in (None, "fdm"):
        flow = IncompressibleFlow(ctx, co, c["kappa"], c["dt"], 2, mask=mask, tol=pp.FLOW_TOL, preconditioner=pre)
        assert flow.projector.preconditioner == pre and flow.lin.projector is flow.projector
        flow.steady_forcing(list(target))
        y = ga._sentinel(ctx)
        flow.propagate(gb._vector(ctx, q0), y)
        out.append(gb._rows(lay, y.to_packed()))
    diff = float(np.max(np.abs(out[0] - out[1])) / np.max(np.abs(out[0])))
    print(f"flow: |None - fdm| / |None| {diff:.3e} (record {pp.FLOW_DIFFERENCE:.1e})")
    assert 0 < np.max(np.abs(out[0])) and diff <= 8 * pp.FLOW_DIFFERENCE


def test_resolvent_matvec_with_fdm_against_plain(gpu):
    """One ``IncompressibleResolventOperator`` matvec on ``case2d`` (omega = 2.0, three steps of 0.13, CG and inner
    GMRES at 1e-13) over a ``LinearisedNavierStokes`` with "fdm" against the same with None, within 8 times the
    restatement's own CG-against-PCG difference; the operator reaches the preconditioner through ``lns.projector``."""
    import incompressible_resolvent_reference as irr
    from test_gpu_resolvent import _download, _random_complex, _upload

    from nekstab_next_amd.gs import GatherScatter
    from nekstab_next_amd.incompressible import LinearisedNavierStokes
    from nekstab_next_amd.resolvent import IncompressibleResolventOperator, pair_context
    from nekstab_next_amd.vector import NekContext

    co, mask, ns, B = irr.CASES["case2d"]()[:4]
    dt, nsteps = pp.RESOLVENT_STEPS
    omega = irr.OMEGAS["case2d"][1]
    lay = NekLayout(ldim=2, lx1=5, lx2=3, nelgv=9)
    fz = _random_complex(lay.n_wf, lay.n_v, 4)
    out = []
    for pre in (None, "fdm"):
        ctx = NekContext(lay, max_cols=4)
        lns = LinearisedNavierStokes(ctx, co, list(np.asarray(B, dtype=np.float64)), ns.kappa, dt, nsteps, mask=mask,
                                     face_average=GatherScatter(ctx, co), tol=irr.CG_TOL, preconditioner=pre)
        pctx = pair_context(lns, max_cols=200)
        op = IncompressibleResolventOperator(pctx, lns, omega, tol=1e-13, kdim=200, maxiter=4)
        assert op.projector is lns.projector and op.projector.preconditioner == pre
        y = pctx.vector()
        op.matvec(_upload(pctx, fz), y)
        assert op.last_gmres["info"] == 0
        out.append(_download(pctx, y))
        print(f"preconditioner {pre}: pair projection iterations {op.projector.last_iterations_each}")
    diff = float(np.max(np.abs(out[0] - out[1])) / np.max(np.abs(out[0])))
    print(f"resolvent matvec: |None - fdm| / |None| {diff:.3e} (record {pp.RESOLVENT_DIFFERENCE:.1e})")
    assert np.max(np.abs(out[0])) > 0 and diff <= 8 * pp.RESOLVENT_DIFFERENCE


# ---- two gloo ranks ------------------------------------------------------------------------------------
def _job(rank, world):
    """``precondition`` of a fixed vector and one projection of a hashed state with "fdm" on this rank's slice of
    the fixed 2-D mesh."""
    from nekstab_next_amd.comm import Comm
    from nekstab_next_amd.pressure import DivergenceFreeProjector
    from nekstab_next_amd.vector import NekContext

    comm = Comm()
    assert comm.world == world and comm.rank == rank
    lx1, ldim, co_g, mask_g, _ = ir.projector_case("closed2d")
    ctx = NekContext(NekLayout(ldim=2, lx1=lx1, lx2=lx1 - 2, nelgv=9), comm=comm, max_cols=4)
    lay = ctx.layout
    e0, e1 = lay.elem_range()
    sl = slice(e0 * lay.pts_v, e1 * lay.pts_v)
    co = {k: v[sl] for k, v in co_g.items()}
    proj = DivergenceFreeProjector(ctx, co, mask=mask_g[sl], tol=TOL, preconditioner="fdm")
    pm = (lx1 - 2) ** 2
    r = np.cos(1.0 + 0.37 * np.arange(9 * pm))[e0 * pm:e1 * pm]
    z = torch.zeros(max(proj.npz, 2), dtype=torch.float64, device=ctx.device)
    proj.precondition(ga._dev(np.concatenate([r, np.zeros(2)])), z)
    x, y = ctx.vector(), ctx.vector()
    x.fill_hash(17)
    proj.op.project(x)
    proj.apply(x, y)
    rows = np.stack([y.to_packed()[f * lay.sv: f * lay.sv + lay.n_v] for f in range(lay.n_wf)])
    return rows, z[: proj.npz].cpu().numpy(), proj.last_iterations, (e0, e1)


def _rank_main(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        out[rank] = _job(rank, world)
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_one_rank_fdm(gpu):
    """Two spawned gloo ranks (5 + 4 elements): ``precondition`` is bit for bit the one-rank result on the rank's
    elements; the projection agrees with one rank within 8 times the restatement's distance record."""
    one, z1, its1, _ = _job(0, 1)
    out = mp.Manager().dict()
    ctx = mp.get_context("spawn")
    port = ga._free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join()
    assert [p.exitcode for p in procs] == [0, 0]
    scale = float(np.max(np.abs(one)))
    pts, pm = one.shape[1] // 9, z1.size // 9
    for r in range(2):
        rows, z, its, (e0, e1) = out[r]
        assert np.array_equal(z, z1[e0 * pm:e1 * pm])
        err = float(np.max(np.abs(rows - one[:, e0 * pts:e1 * pts]))) / scale
        print(f"rank {r}: elements {e0}..{e1}, iterations {its} (one rank {its1}), distance to one rank {err:.3e}")
        assert err <= 8 * pp.PROJECTOR["closed2d"]["dist"]
        assert abs(its - its1) <= 8
