"""The divergence-free projection on two gloo ranks sharing the GPU: the fixed 2-D mesh split 5 + 4 elements.
The reductions of the CG then go through ``ctx.comm.allreduce_`` and run in another order than on one rank, so
the result equals the one-rank projection to 100 tol, not bit for bit.  Launcher: the one of
test_gpu_burgers.py (spawned ranks, results through a manager)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import incompressible_reference as ir
import test_gpu_advdiff as ga

from nekstab_next_amd.layout import NekLayout

ROOT = ga.ROOT
pytestmark = pytest.mark.gpu
TOL = 1e-12


def _job(rank, world):
    """One projection of a hashed state on this rank's slice of the fixed 2-D mesh: (velocity rows, iterations,
    closed, the global pressure count)."""
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
    proj = DivergenceFreeProjector(ctx, co, mask=mask_g[sl], tol=TOL)
    x, y = ctx.vector(), ctx.vector()
    x.fill_hash(17)
    proj.op.project(x)                     # a continuous, masked field
    proj.apply(x, y)
    rows = np.stack([y.to_packed()[f * lay.sv: f * lay.sv + lay.n_v] for f in range(lay.n_wf)])
    return rows, proj.last_iterations, proj.closed, proj.npz_global, (e0, e1)


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


def test_two_ranks_equal_one_rank(gpu):
    one, its1, closed1, npz1, _ = _job(0, 1)
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
    pts = one.shape[1] // 9
    sizes = []
    for r in range(2):
        rows, its, closed, npz, (e0, e1) = out[r]
        sizes.append(e1 - e0)
        err = float(np.max(np.abs(rows - one[:, e0 * pts:e1 * pts]))) / scale
        print(f"rank {r}: elements {e0}..{e1}, iterations {its} (one rank {its1}), distance to one rank {err:.3e}")
        assert closed == closed1 is True and npz == npz1 == 81
        assert err <= 100 * TOL
        assert abs(its - its1) <= 8
    assert sorted(sizes) == [4, 5] and scale > 0
