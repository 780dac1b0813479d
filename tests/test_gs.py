"""The sharded gather-scatter's host half (CPU): the plans of nekstab_next_amd/gs.py, driven for every
rank of a simulated world in one process (local setup, a list as the all-gather, plan), then pack,
exchange and average carried out in NumPy with the kernels' arithmetic.  The concatenated shards must
equal the oracle's one-rank average bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest

import oracle as orc
from seed_helpers import box_mesh_coords

from nekstab_next_amd import gs
from nekstab_next_amd.layout import NekLayout

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cyl():
    d = np.load(os.path.join(GOLD, "cyl_mesh_xy.npz"))
    return {"x": d["x"], "y": d["y"]}, 6, 2


def _box(ne, lx1, shuffled):
    lay = NekLayout(ldim=3, lx1=lx1, lx2=max(lx1 - 2, 1), nelgv=int(np.prod(ne)))
    co = box_mesh_coords(lay, ne)
    if shuffled:
        perm = np.random.default_rng(7).permutation(lay.nelgv)
        co = {k: v.reshape(lay.nelgv, -1)[perm].ravel() for k, v in co.items()}
    return co, lx1, 3


def _split(nel, world):
    """Element ranges of the layout's element-contiguous shards."""
    lay = NekLayout(ldim=2, lx1=2, lx2=1, nelgv=nel)
    return [lay.shard(r, world).elem_range() for r in range(world)]


def simulate(co, lx1, ldim, world, rel_tol=1e-9, ranges=None):
    """Every rank's (local setup, plan) over the global coordinates ``co``."""
    names = ("x", "y", "z")[:ldim]
    pts = lx1 ** ldim
    nel = co["x"].size // pts
    ranges = ranges or _split(nel, world)
    ext = max(float(np.ptp(co[k])) for k in names) or 1.0   # min/max over all ranks
    tol = rel_tol * ext
    locs = []
    for e0, e1 in ranges:
        sh = {k: co[k][e0 * pts:e1 * pts] for k in names}
        locs.append(gs.local_setup(sh, lx1, ldim, tol, e0 * pts))
    gathered = [(l["xyz"], l["gnum"]) for l in locs]
    plans = [gs.build_plan(r, locs[r], gathered) for r in range(world)]
    return ranges, locs, plans


def run_plans(q, ranges, plans, pts):
    """Pack, exchange and average in NumPy: the sum in entry order from 0.0, times 1.0 / count."""
    shards = [q[e0 * pts:e1 * pts].copy() for e0, e1 in ranges]
    sent = [s[p.send] for s, p in zip(shards, plans)]
    for s, p in zip(shards, plans):
        vals = np.empty(p.local.size)
        loc = p.local >= 0
        vals[loc] = s[p.local[loc]]
        for i in np.flatnonzero(~loc):
            vals[i] = sent[p.rank[i]][p.pos[i]]
        cnt = np.diff(p.start)
        acc = np.zeros(p.n_groups)
        for k in range(int(cnt.max()) if cnt.size else 0):
            m = cnt > k
            acc[m] = acc[m] + vals[p.start[:-1][m] + k]
        mean = acc * (1.0 / cnt)
        per_entry = np.repeat(mean, cnt)
        s[p.local[loc]] = per_entry[loc]
    return np.concatenate(shards) if shards else q.copy()


CASES = [("cyl", w) for w in (2, 3, 8)]
CASES += [(f"box{tag}{'s' if sh else ''}", w) for tag in ("234", "333") for sh in (False, True) for w in (2, 3, 5)]
CASES += [("six", 8)]


def _mesh(name):
    if name == "cyl":
        return _cyl()
    if name == "six":
        return _box((3, 2, 1), 3, False)
    ne, lx1 = ((2, 3, 4), 5) if "234" in name else ((3, 3, 3), 2)
    return _box(ne, lx1, name.endswith("s"))


_SIM = {}


def _sim(name, world):
    if (name, world) not in _SIM:
        co, lx1, ldim = _mesh(name)
        _SIM[(name, world)] = (co, lx1, ldim) + simulate(co, lx1, ldim, world)
    return _SIM[(name, world)]


def _global_gid(co, ldim, rel_tol=1e-9):
    from nekstab_next_amd.seeds import group_ids

    xs = [co[k] for k in ("x", "y", "z")[:ldim]]
    return group_ids(xs, rel_tol * (max(float(np.ptp(x)) for x in xs) or 1.0))


@pytest.mark.parametrize("name,world", CASES)
def test_plans_reproduce_the_one_rank_average(name, world):
    """Every rank's plan from its shard's coordinates plus the simulated all-gather; pack, exchange and
    average in NumPy; the concatenated shards equal oracle.coincident_average on the whole mesh.
    ("six", 8): 6 elements on 8 ranks, two empty shards with empty plans."""
    co, lx1, ldim, ranges, locs, plans = _sim(name, world)
    q = np.random.default_rng(5).standard_normal(co["x"].size)
    got = run_plans(q, ranges, plans, lx1 ** ldim)
    np.testing.assert_array_equal(got, orc.coincident_average(q, co))
    if name == "six":
        empty = [p for (e0, e1), p in zip(ranges, plans) if e0 == e1]
        assert len(empty) == 2 and all(p.n_groups == 0 and p.send.size == 0 for p in empty)
    assert any(p.send.size for p in plans)


@pytest.mark.parametrize("name,world", CASES)
def test_candidates_cover_every_cross_rank_point(name, world):
    """Each point with a copy on another rank is a candidate, and the send list is exactly those
    points; every group's entries ascend in global point number on every rank that holds a member."""
    co, lx1, ldim, ranges, locs, plans = _sim(name, world)
    pts = lx1 ** ldim
    gid = _global_gid(co, ldim)
    owner = np.zeros(gid.size, np.int64)
    for r, (e0, e1) in enumerate(ranges):
        owner[e0 * pts:e1 * pts] = r
    lo, hi = np.full(gid.max() + 1, world), np.full(gid.max() + 1, -1)
    np.minimum.at(lo, gid, owner)
    np.maximum.at(hi, gid, owner)
    cross = (lo != hi)[gid]
    for r, (e0, e1) in enumerate(ranges):
        want = np.flatnonzero(cross[e0 * pts:e1 * pts])
        assert np.all(np.isin(want, locs[r]["cand"])), (name, world, r)
        np.testing.assert_array_equal(plans[r].send, want)
        p = plans[r]
        first = np.array([e0 * pts for e0, _ in ranges])
        gn = np.where(p.local >= 0, p.local + e0 * pts, 0)
        rem = p.local < 0
        gn[rem] = first[p.rank[rem]] + np.array([plans[s].send[k] for s, k in zip(p.rank[rem], p.pos[rem])],
                                                 dtype=np.int64)
        for a, b in zip(p.start[:-1], p.start[1:]):
            assert b - a >= 2 and np.all(np.diff(gn[a:b]) > 0)
            assert np.all(gid[gn[a:b]] == gid[gn[a]])                       # one global group ...
            assert b - a == np.count_nonzero(gid == gid[gn[a]])            # ... and all of it
        firsts = np.array([p.local[a:b][p.local[a:b] >= 0].min() for a, b in zip(p.start[:-1], p.start[1:])])
        assert np.all(np.diff(firsts) > 0)                                  # groups ascend with their first member


def test_exposed_faces_only_on_boundary_and_cut():
    """4 x 4 x 4 elements at lx1=4 split in two along z: every candidate lies on the domain boundary or
    on the cut plane — 1,744 of 4,096 points — where 'any point on an element face' would send 3,584."""
    co, lx1, ldim = _box((4, 4, 4), 4, False)
    ranges, locs, plans = simulate(co, lx1, ldim, 2)
    L = (2.0, 1.0, 3.0)
    total = 0
    for (e0, e1), loc in zip(ranges, locs):
        idx = loc["cand"] + e0 * lx1 ** 3
        on_bnd = np.zeros(idx.size, bool)
        for k, ext in zip("xyz", L):
            on_bnd |= (co[k][idx] == 0.0) | (co[k][idx] == ext)
        on_cut = np.abs(co["z"][idx] - 1.5) < 1e-12
        assert np.all(on_bnd | on_cut)
        total += idx.size
    assert total == 1744
    assert sum(p.send.size for p in plans) == 2 * 16 * 16               # the cut plane's face points: 16 elements x 16 per side


def test_rounding_half_step_across_ranks():
    """Two copies of one point a few ulps apart on either side of a half-step of the grouping grid, on
    DIFFERENT ranks, form one group (the construction of test_coincident_groups_across_a_rounding_
    half_step: in x, in y and in both); two points 0.01 cells apart across the half-step, one per rank,
    stay apart.  One 2-D lx1=2 element per
    rank; the remaining corners keep the extent at 1."""
    ext = 1.0
    tol = 1e-9 * ext
    c = (123456 + 0.5) * tol
    lo, hi = np.nextafter(c, -1.0), np.nextafter(np.nextafter(c, 2.0), 2.0)
    assert int(np.round(lo / tol)) != int(np.round(hi / tol))
    far = c + 0.01 * tol
    #            element 0 (rank 0)      element 1 (rank 1)
    x = np.array([lo, 0.3, lo, far,      hi, 0.3, hi, lo])
    y = np.array([0.5, lo, lo, 0.9,      0.5, hi, hi, 0.9])
    x = np.r_[x, [0.0, ext, 0.7, 0.2]]   # a third element (rank 2) sets the extent
    y = np.r_[y, [0.0, ext, 0.1, 0.6]]
    co = {"x": x, "y": y}
    ranges, locs, plans = simulate(co, 2, 2, 3, ranges=[(0, 1), (1, 2), (2, 3)])
    for r in (0, 1):
        p = plans[r]
        assert p.n_groups == 3 and np.all(np.diff(p.start) == 2)
        np.testing.assert_array_equal(p.send, [0, 1, 2])
        np.testing.assert_array_equal(np.sort(p.local[p.local >= 0]), [0, 1, 2])
        np.testing.assert_array_equal(p.rank[p.local < 0], [1 - r] * 3)
    assert plans[2].n_groups == 0
    q = np.random.default_rng(3).standard_normal(x.size)
    np.testing.assert_array_equal(run_plans(q, ranges, plans, 4), orc.coincident_average(q, co))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _allgather_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist

    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from nekstab_next_amd.comm import Comm

        comm = Comm()
        send = torch.tensor([-0.0, float(rank), float("inf")], dtype=torch.float64)
        got = comm.allgather_(send, torch.empty(3 * world, dtype=torch.float64))
        ids = comm.allgather_(torch.tensor([rank, -1], dtype=torch.int64), torch.empty(2 * world, dtype=torch.int64))
        out[rank] = (got.numpy().copy(), ids.numpy().copy())
    finally:
        dist.destroy_process_group()


def test_comm_allgather_rank_order_and_bits():
    """Comm.allgather_ over gloo: rank order, any dtype, and the bytes unchanged (-0.0 keeps its sign);
    a plain copy at world 1; a wrong output size is refused."""
    import torch
    import torch.multiprocessing as mp

    from nekstab_next_amd.comm import Comm

    world = 3
    out = mp.Manager().dict()
    mp.spawn(_allgather_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    want = np.concatenate([[-0.0, float(r), np.inf] for r in range(world)])
    for r in range(world):
        got, ids = out[r]
        np.testing.assert_array_equal(got, want)
        assert np.all(np.signbit(got[0::3]))
        np.testing.assert_array_equal(ids, np.array([[s, -1] for s in range(world)]).ravel())
    one = Comm()
    a = torch.arange(4, dtype=torch.float64)
    assert torch.equal(one.allgather_(a, torch.empty(4, dtype=torch.float64)), a)
    with pytest.raises(ValueError, match="allgather_"):
        one.allgather_(a, torch.empty(5, dtype=torch.float64))
