"""The sharded gather-scatter on the device (nkv_gs_pack / nkv_gs_average, gs.GatherScatter): against
seeds.FaceAverage (nkv_group_average) on one rank, and on 2, 3 and 8 gloo ranks sharing the GPU against
the one-rank results' slices — bit for bit, as ranks exchange member values and every group is summed in
ascending global point number.  Each world's ranks are spawned once and run every job of that world."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from seed_helpers import box_mesh_coords

from nekstab_next_amd import _lib, seeds
from nekstab_next_amd.layout import NekLayout, cylinder_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = pytest.mark.gpu


def _mesh(name):
    if name == "cyl":
        d = np.load(os.path.join(GOLD, "cyl_mesh_xy.npz"))
        return cylinder_layout(1996), {"x": d["x"], "y": d["y"]}
    if name == "six":   # more ranks than elements at world 8
        lay = NekLayout(ldim=3, lx1=3, lx2=1, nelgv=6)
        return lay, box_mesh_coords(lay, (3, 2, 1))
    lay = NekLayout(ldim=3, lx1=6, lx2=4, nelgv=3 * 2 * 4, n_scalars=1)
    return lay, box_mesh_coords(lay, (3, 2, 4))


def _hash(gnum, seg):
    """A value per GLOBAL point number and segment in [-0.5, 0.5): the same on any sharding."""
    h = (gnum.astype(np.uint64) + np.uint64(1 + 7919 * seg)) * np.uint64(2654435761) % np.uint64(2 ** 32)
    return h.astype(np.float64) / 2.0 ** 32 - 0.5


def _shard_coords(lay, co):
    e0, e1 = lay.elem_range()
    return {k: v[e0 * lay.pts_v:e1 * lay.pts_v] for k, v in co.items()}


def _segments(lay, nseg):
    e0, e1 = lay.elem_range()
    gnum = np.arange(e0 * lay.pts_v, e1 * lay.pts_v)
    dev = torch.device("cuda", 0)
    return [torch.as_tensor(_hash(gnum, s)).to(dev) if gnum.size else torch.zeros(1, dtype=torch.float64, device=dev)
            for s in range(nseg)]


def _jobs(rank, world):
    """Everything one rank of ``world`` computes (world 1: the references, with FaceAverage)."""
    from nekstab_next_amd import synthetic as syn
    from nekstab_next_amd.comm import Comm
    from nekstab_next_amd.gs import GatherScatter, auto_average
    from nekstab_next_amd.postproc import energy_budget_fields
    from nekstab_next_amd.sensitivity import Gradm1, bf_sensitivity_fields, velocity_layout
    from nekstab_next_amd.vector import NekContext
    from nekstab_next_amd.vortex import VortexCore

    comm = Comm()
    assert comm.world == world and comm.rank == rank
    res = {}
    for name in ("cyl", "box") + (("six",) if world in (1, 8) else ()):
        lay_g, co_g = _mesh(name)
        ctx = NekContext(lay_g, comm=comm, max_cols=4)
        lay = ctx.layout
        co = _shard_coords(lay, co_g)
        segs = _segments(lay, lay.ldim + 1)
        if world == 1:
            fa = seeds.FaceAverage(ctx, co)
            for s in segs:
                fa.apply(s.data_ptr())
        else:
            g = GatherScatter(ctx, co)
            g.apply_many([s.data_ptr() for s in segs])
            res[("counts", name)] = (g.n_groups, g.n_send, g.stride, g.n_candidates)
        res[("avg", name)] = np.stack([s[: lay.n_v].cpu().numpy() for s in segs])
        if world in (1, 3) and name != "six":
            avg = seeds.FaceAverage(ctx, co) if world == 1 else GatherScatter(ctx, co)
            seed = seeds.noise_seed(ctx, co, face_average=avg).to_packed()
            res[("seed", name)] = np.stack([seed[c * lay.sv: c * lay.sv + lay.n_v] for c in range(lay.n_wf)])
    if world in (1, 2):
        lay_g, co_g = _mesh("box")
        sh = velocity_layout(lay_g).shard(rank, world)
        ctx = NekContext(sh, weights=syn.mass_weights(sh), comm=comm, max_cols=4)
        co = _shard_coords(sh, co_g)
        vecs = []
        for sd in (3, 4, 5, 6, 7):
            v = ctx.vector()
            v.fill_hash(sd)
            vecs.append(v)
        n, d, sv = sh.n_v, sh.ldim, sh.sv
        core = VortexCore(ctx, co)
        res["vort"] = core.comp_vort3(vecs[0], "auto")[:, :n].cpu().numpy()
        fa = auto_average(ctx, co)                      # what "auto" builds in the drivers
        assert isinstance(fa, GatherScatter) == (world > 1)
        grad_op = Gradm1(ctx, co)
        out, grad = bf_sensitivity_fields(ctx, *vecs[:4], grad_op, fa)
        res["bf_out"] = out.view(6 * d, sv)[:, :n].cpu().numpy()
        res["bf_grad"] = grad.view(4 * d * d, sv)[:, :n].cpu().numpy()
        prod, diss, integ = energy_budget_fields(ctx, vecs[4], vecs[0], vecs[1], grad_op, fa, 0.02)
        ctx.check_nan()
        res["pke_prod"] = prod.view(d * d, sv)[:, :n].cpu().numpy()
        res["pke_diss"] = diss[:n].cpu().numpy()
        res["pke_int"] = integ.cpu().numpy()
    return res


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, out):
    sys.path.insert(0, ROOT)
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


def _slice(lay_g, rank, world, a):
    sh = lay_g.shard(rank, world)
    e0, e1 = sh.elem_range()
    return a[..., e0 * sh.pts_v:e1 * sh.pts_v]


# ---- world 1 -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cyl", "box"])
def test_world1_equals_face_average(gpu, name):
    """apply_many over 1, 3 and 7 segments equals that many FaceAverage.apply calls bit for bit, and so do
    apply on one segment and __call__ on a vector's fields (cylinder: vertices shared by 4 and 5 elements;
    3 x 2 x 4 box at lx1=6: corners shared by 8)."""
    from nekstab_next_amd.gs import GatherScatter
    from nekstab_next_amd.vector import NekContext

    lay, co = _mesh(name)
    ctx = NekContext(lay, max_cols=4)
    fa, g = seeds.FaceAverage(ctx, co), GatherScatter(ctx, co)
    assert g.n_groups == fa.n_groups and g.n_send == 0 and g.stride == 0
    for nseg in (1, 3, 7):
        a, b = _segments(lay, nseg), _segments(lay, nseg)
        for s in a:
            fa.apply(s.data_ptr())
        g.apply_many([s.data_ptr() for s in b])
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert not torch.equal(a[0], _segments(lay, 1)[0])      # the average did move the shared points
    a, b = _segments(lay, 1)[0], _segments(lay, 1)[0]
    fa.apply(a.data_ptr())
    g.apply(b.data_ptr())
    assert torch.equal(a, b)
    va, vb = ctx.vector(), ctx.vector()
    va.fill_hash(9)
    vb.fill_hash(9)
    fa(va, range(lay.ldim))
    g(vb, range(lay.ldim))
    assert torch.equal(va.storage, vb.storage)
    g.apply_many([])
    with pytest.raises(ValueError, match="points"):
        GatherScatter(ctx, {k: v[:-1] for k, v in co.items()})


def test_entry_checks(gpu):
    """NULL and out-of-range arguments return NKV_EINVAL; zero groups / points return NKV_OK untouched."""
    lib = _lib.load()
    q = torch.ones(64, dtype=torch.float64, device="cuda")
    i32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    one = (ctypes.c_void_p * 1)(q.data_ptr())
    null1 = (ctypes.c_void_p * 1)(None)
    many = (ctypes.c_void_p * (_lib.NKV_GS_MAX_FIELDS + 1))(*([q.data_ptr()] * (_lib.NKV_GS_MAX_FIELDS + 1)))
    st = torch.cuda.current_stream().cuda_stream
    ip, qp = i32.data_ptr(), q.data_ptr()
    ok, bad = _lib.NKV_OK, _lib.NKV_EINVAL
    # average(nf, q, n_v, n_groups, start, src, recv, stride, n_ranks, stream)
    assert lib.nkv_gs_average(1, one, 64, 0, None, None, None, 0, 1, st) == ok
    assert lib.nkv_gs_average(1, None, 64, 0, None, None, None, 0, 1, st) == ok
    assert lib.nkv_gs_average(1, one, 64, -1, ip, ip, None, 0, 1, st) == bad
    assert lib.nkv_gs_average(1, one, -1, 1, ip, ip, None, 0, 1, st) == bad
    assert lib.nkv_gs_average(0, one, 64, 1, ip, ip, None, 0, 1, st) == bad
    assert lib.nkv_gs_average(_lib.NKV_GS_MAX_FIELDS + 1, many, 64, 1, ip, ip, None, 0, 1, st) == bad
    assert lib.nkv_gs_average(1, None, 64, 1, ip, ip, None, 0, 1, st) == bad
    assert lib.nkv_gs_average(1, null1, 64, 1, ip, ip, None, 0, 1, st) == bad
    assert lib.nkv_gs_average(1, one, 64, 1, None, ip, None, 0, 1, st) == bad
    assert lib.nkv_gs_average(1, one, 64, 1, ip, None, None, 0, 1, st) == bad
    assert lib.nkv_gs_average(1, one, 64, 1, ip, ip, None, 4, 2, st) == bad          # recv NULL with a stride
    assert lib.nkv_gs_average(1, one, 64, 1, ip, ip, qp, 4, 0, st) == bad            # no ranks
    assert lib.nkv_gs_average(1, one, 2 ** 31, 1, ip, ip, None, 0, 1, st) == bad     # n_v beyond 32-bit indices
    assert lib.nkv_gs_average(1, one, 64, 1, ip, ip, qp, 2 ** 30, 2, st) == bad      # ranks x stride beyond them
    assert "32-bit" in _lib.last_error()
    # pack(nf, q, n_v, n_send, send_idx, stride, send, stream)
    assert lib.nkv_gs_pack(1, one, 64, 0, None, 0, None, st) == ok
    assert lib.nkv_gs_pack(1, one, 64, -1, ip, 8, qp, st) == bad
    assert lib.nkv_gs_pack(1, one, 64, 9, ip, 8, qp, st) == bad                      # n_send > stride
    assert lib.nkv_gs_pack(1, one, 4, 8, ip, 8, qp, st) == bad                       # n_send > n_v
    assert lib.nkv_gs_pack(0, one, 64, 8, ip, 8, qp, st) == bad
    assert lib.nkv_gs_pack(_lib.NKV_GS_MAX_FIELDS + 1, many, 64, 8, ip, 8, qp, st) == bad
    assert lib.nkv_gs_pack(1, None, 64, 8, ip, 8, qp, st) == bad
    assert lib.nkv_gs_pack(1, null1, 64, 8, ip, 8, qp, st) == bad
    assert lib.nkv_gs_pack(1, one, 64, 8, None, 8, qp, st) == bad
    assert lib.nkv_gs_pack(1, one, 64, 8, ip, 8, None, st) == bad
    assert lib.nkv_gs_pack(1, one, 2 ** 31, 8, ip, 8, qp, st) == bad
    torch.cuda.synchronize()
    assert torch.all(q == 1.0)
    # one real launch of each by hand: two groups over local points and "received" values
    src = torch.tensor([0, 3, -(1 + 1), 5, -(1 + 4 + 2)], dtype=torch.int32, device="cuda")   # stride 4
    start = torch.tensor([0, 3, 5], dtype=torch.int32, device="cuda")
    recv = torch.arange(100.0, 116.0, dtype=torch.float64, device="cuda")                     # 2 ranks x 2 segments x 4
    a = torch.arange(8.0, dtype=torch.float64, device="cuda")
    b = a * 10
    two = (ctypes.c_void_p * 2)(a.data_ptr(), b.data_ptr())
    assert lib.nkv_gs_average(2, two, 8, 2, start.data_ptr(), src.data_ptr(), recv.data_ptr(), 4, 2, st) == ok
    wa = ((0.0 + 0.0) + 3.0 + 101.0) * (1.0 / 3.0), ((0.0 + 5.0) + 110.0) * 0.5
    wb = ((0.0 + 0.0) + 30.0 + 105.0) * (1.0 / 3.0), ((0.0 + 50.0) + 114.0) * 0.5
    assert a.tolist() == [wa[0], 1.0, 2.0, wa[0], 4.0, wa[1], 6.0, 7.0]
    assert b.tolist() == [wb[0], 10.0, 20.0, wb[0], 40.0, wb[1], 60.0, 70.0]
    idx = torch.tensor([1, 5, 7], dtype=torch.int32, device="cuda")
    send = torch.zeros(8, dtype=torch.float64, device="cuda")
    assert lib.nkv_gs_pack(2, two, 8, 3, idx.data_ptr(), 4, send.data_ptr(), st) == ok
    assert send.tolist() == [1.0, wa[1], 7.0, 0.0, 10.0, wb[1], 70.0, 0.0]


_RCCL_SCRIPT = r'''
import sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
torch.cuda.set_device(0)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:" + sys.argv[2], rank=0, world_size=1,
                        device_id=torch.device("cuda", 0))
from nekstab_next_amd.comm import Comm
comm = Comm(force_collectives=True)   # world 1, the gather through RCCL's all_gather all the same
assert comm.backend == "nccl" and comm.world == 1
a = torch.tensor([-0.0, 1.5, float("inf"), 3.0], dtype=torch.float64, device="cuda")
out = comm.allgather_(a, torch.full((4,), 7.0, dtype=torch.float64, device="cuda"))
assert torch.equal(out, a) and bool(torch.signbit(out[0]))
i = torch.tensor([5, -1, 2 ** 40], dtype=torch.int64, device="cuda")
assert torch.equal(comm.allgather_(i, torch.zeros(3, dtype=torch.int64, device="cuda")), i)
dist.destroy_process_group()
print("RCCL allgather ok")
'''


def test_allgather_rccl_path_single_gpu(gpu, tmp_path):
    """Comm.allgather_ through the nccl (= RCCL) backend on the real device: a world-1 group with the
    collectives forced on, device buffers gathered in place of the plain copy (the 8-GPU path minus the
    peers), bytes unchanged.  In a child process, so the test process holds no process group."""
    import subprocess

    script = tmp_path / "rccl_allgather.py"
    script.write_text(_RCCL_SCRIPT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(script), ROOT, str(_free_port())], capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "RCCL allgather ok" in p.stdout


# ---- several ranks ---------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3, 8])
def test_sharded_average_equals_one_rank(gpu, world):
    """apply_many over ldim + 1 segments (values: a hash of the global point number) on 2, 3 (ragged:
    665/665/666 elements) and 8 ranks equals this shard's slice of the one-rank FaceAverage result, on the
    cylinder and on the 24-element box; at world 8 also 6 elements on 8 ranks (two empty shards, which
    still take part in the exchange)."""
    one, got = _world(1)[0], _world(world)
    for name in ("cyl", "box") + (("six",) if world == 8 else ()):
        lay_g, _ = _mesh(name)
        sends = 0
        for r in range(world):
            np.testing.assert_array_equal(got[r][("avg", name)], _slice(lay_g, r, world, one[("avg", name)]))
            n_groups, n_send, stride, n_cand = got[r][("counts", name)]
            assert n_send <= stride and n_send <= n_cand <= lay_g.shard(r, world).n_v
            sends += n_send
        assert sends > 0
        if name == "six":
            empty = [r for r in range(world) if lay_g.shard(r, world).n_v == 0]
            assert len(empty) == 2 and [got[r][("counts", name)][:2] for r in empty] == [(0, 0)] * 2


@pytest.mark.parametrize("name", ["cyl", "box"])
def test_sharded_default_seed_equals_one_rank(gpu, name):
    """The reference's default seed (ifseed_nois: op_add_noise / add_noise_scal with dssum + vmult and
    dsavg) on 3 ranks with a GatherScatter equals the one-rank noise_seed with FaceAverage, bit for bit."""
    one, got = _world(1)[0], _world(3)
    lay_g, _ = _mesh(name)
    for r in range(3):
        np.testing.assert_array_equal(got[r][("seed", name)], _slice(lay_g, r, 3, one[("seed", name)]))
    assert np.any(one[("seed", name)] != 0.0)


def test_sharded_consumers_with_auto(gpu):
    """comp_vort3("auto"), bf_sensitivity_fields and energy_budget_fields with what "auto" builds, on 2
    ranks: the FIELDS equal the one-rank fields' slices bit for bit (gradm1 is element-local, the average
    bit-identical).  The all-reduced integrals only regroup the partial sums of the same n = 5,184 terms
    bm1 * field per integral: any two summation orders differ by at most 2 n u sum|terms| (u = 2^-53),
    which is the gate; every rank holds the same all-reduced bits."""
    from nekstab_next_amd import synthetic as syn
    from nekstab_next_amd.sensitivity import velocity_layout

    one, got = _world(1)[0], _world(2)
    lay_g, _ = _mesh("box")
    w = syn.mass_weights(velocity_layout(lay_g))
    fields = list(one["pke_prod"]) + [one["pke_diss"]]
    gate = np.array([2 * w.size * 2.0 ** -53 * np.sum(w * np.abs(f)) for f in fields])
    for r in range(2):
        for key in ("vort", "bf_out", "bf_grad", "pke_prod", "pke_diss"):
            np.testing.assert_array_equal(got[r][key], _slice(lay_g, r, 2, one[key]), err_msg=key)
        assert np.all(np.abs(got[r]["pke_int"] - one["pke_int"]) <= gate), (got[r]["pke_int"], one["pke_int"])
        np.testing.assert_array_equal(got[r]["pke_int"], got[0]["pke_int"])
    assert np.any(one["vort"] != 0.0) and np.any(one["pke_diss"] != 0.0) and np.all(gate > 0)
