"""nkv_sfd_step / nkv_tdf_step and the SFD / TDF classes on the device against the op-for-op
restatement of core/fixedp.f90 (tests/fixedp_reference.py).

Tolerances: every state vector and fc to 1e-12 max|field| after every step (DESIGN.md §7's gate; one
step rounds fewer than 10 times at 1.1e-16 and the kernel evaluates in the reference's order without
contraction), the residual to 1e-12 relative (its summation order differs from numpy's)."""
import math

import numpy as np
import pytest
import torch

import fixedp_reference as fr
from nekstab_next_amd import _lib, fixedp
from nekstab_next_amd import synthetic as syn
from nekstab_next_amd.layout import NekLayout, pair_layout

pytestmark = pytest.mark.gpu

LAYOUTS = {
    "2d": NekLayout(2, 6, 4, 300),
    "3d_scalar": NekLayout(3, 5, 3, 37, n_scalars=1),
    "2d_nopr": NekLayout(2, 6, 4, 150, ifpo=False),
}
UP4, UP5, DT = 0.3, 0.2, 0.05
AB3 = (23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0)


def _weights(lay):
    """Mass weights with every second point zeroed (the sponge case, core/forcing.f90:101-104)."""
    w = syn.mass_weights(lay)
    w[::2] = 0.0
    return w


def _context(lay, comm=None):
    from nekstab_next_amd.vector import NekContext

    w = _weights(lay)
    return NekContext(lay, weights=w, comm=comm, max_cols=4), w


def _host(lay, seed):
    return syn.hash_vector(lay, seed)[:lay.rows].copy()


def _live_mask(lay):
    m = np.zeros(lay.ld, dtype=bool)
    for _, s, n in lay.field_slices():
        m[s:s + n] = True
    return m


def _check_vector(lay, dev_vec, ref, what):
    """Stored rows to 1e-12 max|field|; padding rows and the time slot exactly 0."""
    got = dev_vec.to_packed()
    scale = float(np.max(np.abs(ref))) if ref.size else 0.0
    err = float(np.max(np.abs(got[:lay.rows] - ref))) if ref.size else 0.0
    assert err <= 1e-12 * scale, (what, err, scale)
    assert not got[~_live_mask(lay)].any(), what          # padding, time slot, tail


def _check_sfd_state(lay, sfd, ref, fc, fc_ref, tag):
    _check_vector(lay, sfd.v_old, ref.oldV, tag + " v_old")
    _check_vector(lay, sfd.qbar, ref.oldQ, tag + " qbar")
    for dev, r, nm in zip(sfd._q, (ref.qa, ref.qb, ref.qc), ("qa", "qb", "qc")):
        _check_vector(lay, dev, r, f"{tag} {nm}")
    _check_vector(lay, fc, fc_ref, tag + " fc")


def _sfd_pair(ctx, lay, w, monitor=False):
    up5 = 0.0 if monitor else UP5
    vol = float(np.sum(w)) + 1.0          # not the default: the volume argument is used
    sfd = fixedp.SFD(ctx, UP4, up5, DT, 1e-10, volume=vol)
    cutoff, gain = fixedp.sfd_coefficients(UP4, up5)
    return sfd, fr.SFDReference(lay, w, cutoff, gain, DT, vol, monitor=monitor)


# ---- 1. trajectory ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(LAYOUTS))
def test_sfd_trajectory_matches_restatement(gpu, name):
    lay = LAYOUTS[name]
    ctx, w = _context(lay)
    sfd, ref = _sfd_pair(ctx, lay, w)
    v, fc = ctx.vector(), ctx.vector()
    v.fill_hash(100)
    fc.fill_hash(99)                                       # fc starts nonzero
    fc_ref = _host(lay, 99)
    sfd.start(v)
    ref.start(_host(lay, 100))
    old = 0.0
    for istep in range(1, 13):                             # Euler, AB2, then AB3
        v.fill_hash(100 + istep)
        res, rate, conv = sfd.step(v, fc)
        res_ref, rate_ref = ref.step(_host(lay, 100 + istep), fc_ref, fixedp.ab3_coefficients(istep))
        print(f"{name} step {istep}: res {res:.17e} ref {res_ref:.17e}")
        assert abs(res - res_ref) <= 1e-12 * res_ref, (istep, res, res_ref)
        assert rate == (res - old) / DT and not conv
        old = res
        _check_sfd_state(lay, sfd, ref, fc, fc_ref, f"{name} step {istep}")
    ctx.check_nan()


# ---- 2. velocity-only residual ------------------------------------------------------------------------

def test_residual_sums_velocities_only(gpu):
    lay = LAYOUTS["3d_scalar"]
    ctx, w = _context(lay)
    sfd, _ = _sfd_pair(ctx, lay, w)
    v = ctx.vector()
    v.fill_hash(7)
    sfd.start(v)
    host = v.to_packed()
    other = syn.hash_vector(lay, 8)
    changed = host.copy()
    changed[3 * lay.sv:] = other[3 * lay.sv:]              # the scalar and the pressure only
    zero_w = np.nonzero(_weights(lay) == 0.0)[0]
    for c in range(3):                                     # and the velocities where the weight is 0
        changed[c * lay.sv + zero_w] = other[c * lay.sv + zero_w]
    assert np.count_nonzero(changed != host) > lay.n_v
    v.from_packed(changed)
    fc = ctx.vector()
    res, _, _ = sfd.step(v, fc)
    assert sfd.res2 == 0.0 and res == 0.0
    np.testing.assert_array_equal(sfd.v_old.to_packed(), changed)
    # and a change at one weighted velocity point is seen
    i = int(np.nonzero(_weights(lay))[0][0])
    changed[2 * lay.sv + i] += 0.5
    v.from_packed(changed)
    sfd.step(v, fc)
    assert sfd.res2 == pytest.approx(_weights(lay)[i] * 0.25, rel=1e-14)


# ---- 3. more chunks than workgroups -------------------------------------------------------------------

def test_sfd_grid_stride(gpu):
    lay = NekLayout(3, 8, 6, 1500)
    assert lay.rows > 1024 * 2048                          # more chunks than any grid (<= NKV_MAXB workgroups)
    ctx, w = _context(lay)
    sfd, ref = _sfd_pair(ctx, lay, w)
    v, fc = ctx.vector(), ctx.vector()
    v.fill_hash(1)
    sfd.start(v)
    ref.start(_host(lay, 1))
    for i, (dev, r) in enumerate(zip(sfd._q, (ref.qa, ref.qb, ref.qc))):   # nonzero histories
        dev.fill_hash(20 + i)
        r[:] = _host(lay, 20 + i)
    sfd.qbar.fill_hash(30)
    ref.oldQ[:] = _host(lay, 30)
    fc.fill_hash(31)
    fc_ref = _host(lay, 31)
    v.fill_hash(2)
    res, _, _ = sfd.step(v, fc, ab=AB3)
    res_ref, _ = ref.step(_host(lay, 2), fc_ref, AB3)
    assert abs(res - res_ref) <= 1e-12 * res_ref, (res, res_ref)
    _check_sfd_state(lay, sfd, ref, fc, fc_ref, "grid-stride")


# ---- 4. monitor mode ------------------------------------------------------------------------------------

def test_monitor_mode(gpu):
    lay = LAYOUTS["2d"]
    ctx, w = _context(lay)
    sfd, ref = _sfd_pair(ctx, lay, w, monitor=True)
    assert sfd.monitor and not hasattr(sfd, "qbar")
    v = ctx.vector()
    v.fill_hash(100)
    sfd.start(v)
    ref.start(_host(lay, 100))
    for istep in (1, 2):
        v.fill_hash(100 + istep)
        res, _, _ = sfd.step(v, None)
        res_ref, _ = ref.step(_host(lay, 100 + istep), None, None)
        assert abs(res - res_ref) <= 1e-12 * res_ref
        _check_vector(lay, sfd.v_old, ref.oldV, "monitor v_old")
    # the entry itself, given filter state and a forcing: none of them is read or written
    others = [ctx.vector() for _ in range(5)]
    for i, o in enumerate(others):
        o.fill_hash(40 + i)
    before = [o.to_packed() for o in others]
    r2 = torch.zeros(1, dtype=torch.float64, device=ctx.device)
    v.fill_hash(200)
    ctx.call("nkv_sfd_step", ctx.w.data_ptr(), v.ptr, sfd.v_old.ptr, *[o.ptr for o in others], 1.5, -0.5, 0.25, 0.1,
             -0.4, 2, r2.data_ptr(), ctx.ws.data_ptr(), _lib.NKV_SFD_MONITOR, ctx.stream)
    res_ref, _ = ref.step(_host(lay, 200), None, None)
    assert abs(math.sqrt(float(r2.item()) / ref.volume) - res_ref) <= 1e-12 * res_ref
    for o, b in zip(others, before):
        np.testing.assert_array_equal(o.to_packed(), b)
    _check_vector(lay, sfd.v_old, ref.oldV, "monitor v_old (entry)")


# ---- 5. TDF ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["2d", "3d_scalar"])
def test_tdf_matches_shifting_history(gpu, name):
    lay = LAYOUTS[name]
    ctx, w = _context(lay)
    vol = float(np.sum(w))
    tdf = fixedp.TDF(ctx, period=5.0, dt_target=1.0, tol=1e-10)
    assert tdf.norbit == 5 and tdf.dt == 1.0 and tdf.volume == pytest.approx(vol, rel=1e-13)
    ref = fr.TDFReference(lay, w, 5, tdf.gain, tdf.volume)
    v, fc = ctx.vector(), ctx.vector()
    fc.fill_hash(99)
    fc_ref = _host(lay, 99)
    nw = lay.n_wf * lay.sv
    prev = 0.0
    for istep in range(1, 14):
        v.fill_hash(300 + istep)
        l2, rate, conv = tdf.step(v, fc)
        l2_ref, rate_ref = ref.step(_host(lay, 300 + istep), fc_ref)
        if istep <= 5:
            assert (l2, rate, conv) == (0.0, 0.0, False)
        else:
            print(f"{name} step {istep}: l2 {l2:.17e} ref {l2_ref:.17e}")
            assert abs(l2 - l2_ref) <= 1e-12 * l2_ref and rate == l2 - prev and not conv
            prev = l2
        _check_vector(lay, fc, fc_ref, f"tdf fc step {istep}")
        if istep >= 5:                                     # the ring holds the reference's history
            ring = tdf.ring.storage.cpu().numpy()
            for i in range(5):
                slot = ring[(istep - 5 + i) % 5]
                np.testing.assert_array_equal(slot[:nw], ref.hist[i])
                assert not slot[nw:].any()                 # pressure, time: never written
    ctx.check_nan()


def test_tdf_periodic_flow_is_unforced(gpu):
    lay = LAYOUTS["3d_scalar"]
    ctx, _ = _context(lay)
    tdf = fixedp.TDF(ctx, period=5.0, dt_target=1.0, tol=1e-10)
    v, fc = ctx.vector(), ctx.vector()
    fc.fill_hash(99)
    fc0 = fc.to_packed()
    for istep in range(1, 14):
        v.fill_hash(400 + (istep - 1) % 5)                 # exactly norbit-periodic
        l2, rate, conv = tdf.step(v, fc)
        assert l2 == 0.0 and rate == 0.0 and not conv      # l2 = 0 is not convergence (:105)
    np.testing.assert_array_equal(fc.to_packed(), fc0)


# ---- 6. end to end ------------------------------------------------------------------------------------------

def _device_oscillator(ctx, lay, b, v0, uparam4, steps, forced=True):
    """The loop of fixedp_reference.run_oscillator with the flow, the forcing and the time stepping
    (torch ops on the field slices) on the device.  Returns (first step reported converged, final v)."""
    sv = lay.sv
    E, G = (complex(z) for z in fr.oscillator_maps(0.1))   # python floats for the torch ops
    v, fc, bb = ctx.vector(), ctx.vector(), ctx.vector()
    pad = np.zeros(lay.ld)
    pad[:lay.rows] = v0
    v.from_packed(pad)
    pad[:lay.rows] = b
    bb.from_packed(pad)
    x, y = v.storage[:sv], v.storage[sv:2 * sv]
    bx, by = bb.storage[:sv], bb.storage[sv:2 * sv]
    fx, fy = fc.storage[:sv], fc.storage[sv:2 * sv]
    sfd = fixedp.SFD(ctx, uparam4, 0.25, 0.1, 1e-10)
    sfd.start(v)
    first = None
    for istep in range(1, steps + 1):
        rx, ry = bx + fx, by + fy
        xn = E.real * x - E.imag * y + G.real * rx - G.imag * ry
        yn = E.imag * x + E.real * y + G.imag * rx + G.real * ry
        x.copy_(xn)
        y.copy_(yn)
        fc.storage.zero_()
        if forced:
            _, _, conv = sfd.step(v, fc)
            if conv and first is None:
                first = istep
    return first, v.to_packed()[:lay.rows]


@pytest.mark.parametrize("uparam4", [1.0 / (2.0 * math.pi), -1.0 / (2.0 * math.pi)], ids=["akervik", "casacuberta"])
def test_sfd_stabilises_the_oscillator_on_the_device(gpu, uparam4):
    from nekstab_next_amd.vector import NekContext

    lay = NekLayout(2, 4, 2, 6)
    w = syn.mass_weights(lay)
    b, v0 = _host(lay, 41), _host(lay, 42)
    b[2 * lay.sv:] = 0.0
    v0[2 * lay.sv:] = 0.0
    ustar = -(b[:lay.sv] + 1j * b[lay.sv:2 * lay.sv]) / fr.LAMBDA
    k_ref, _, _ = fr.run_oscillator(lay, w, b, v0, uparam4, 0.25, 0.1, 1e-10, 1500)
    assert k_ref is not None
    ctx = NekContext(lay, weights=w, max_cols=4)
    first, v = _device_oscillator(ctx, lay, b, v0, uparam4, k_ref + 100)
    print(f"converged at step {first}, restatement {k_ref}")
    assert first is not None and abs(first - k_ref) <= 2, (first, k_ref)
    err = float(np.max(np.abs(v[:lay.sv] + 1j * v[lay.sv:2 * lay.sv] - ustar)))
    assert err < 1e-9, err


def test_unforced_oscillator_diverges_on_the_device(gpu):
    from nekstab_next_amd.vector import NekContext

    lay = NekLayout(2, 4, 2, 6)
    b, v0 = _host(lay, 41), _host(lay, 42)
    b[2 * lay.sv:] = 0.0
    v0[2 * lay.sv:] = 0.0
    ustar = -(b[:lay.sv] + 1j * b[lay.sv:2 * lay.sv]) / fr.LAMBDA
    ctx = NekContext(lay, weights=syn.mass_weights(lay), max_cols=4)
    _, v = _device_oscillator(ctx, lay, b, v0, 1.0 / (2.0 * math.pi), 1500, forced=False)
    assert float(np.max(np.abs(v[:lay.sv] + 1j * v[lay.sv:2 * lay.sv] - ustar))) > 1e5


# ---- 7. shards in one process ------------------------------------------------------------------------------------

class _ShardComm:
    """Stand-in for comm.Comm of rank r of `world`, run one rank after the other: the all-reduce
    leaves the local partial in place and records it, the test does the sum."""

    def __init__(self, rank, world):
        self.rank, self.world, self.seen = rank, world, []

    def allreduce_(self, t):
        self.seen.append(t.clone())
        return t


def _run_sfd(lay, comm, steps=3):
    ctx, _ = _context(lay, comm=comm)
    lay = ctx.layout
    sfd = fixedp.SFD(ctx, UP4, UP5, DT, 1e-10, volume=1.0)
    v, fc = ctx.vector(), ctx.vector()
    v.fill_hash(100)
    fc.fill_hash(99)
    sfd.start(v)
    res2 = []
    for istep in range(1, steps + 1):
        v.fill_hash(100 + istep)
        sfd.step(v, fc)
        res2.append(sfd.res2)
    tdf = fixedp.TDF(ctx, period=2.0, dt_target=1.0, tol=1e-10, volume=1.0)
    for istep in range(1, 4):
        v.fill_hash(100 + istep)
        tdf.step(v, fc)
    res2.append(tdf.res2)
    ctx.check_nan()
    vecs = [sfd.v_old, sfd.qbar, *sfd._q, fc, tdf.ring[0], tdf.ring[1]]
    return lay, res2, [x.to_packed() for x in vecs]


@pytest.mark.parametrize("nelgv", [7, 1])
def test_shards_equal_one_rank(gpu, nelgv):
    """nelgv = 1 with two ranks: rank 0 owns no element (an empty shard launches nothing)."""
    glob = NekLayout(2, 6, 4, nelgv)
    one, res2_one, vecs_one = _run_sfd(glob, None)
    total = np.zeros(len(res2_one))
    for rank in range(2):
        comm = _ShardComm(rank, 2)
        lay, res2, vecs = _run_sfd(glob.shard(rank, 2), comm)
        assert (lay.rank, lay.world) == (rank, 2) and len(comm.seen) == len(res2)
        if lay.n_v == 0:
            assert res2 == [0.0] * len(res2)
        total += res2
        for a, g in zip(vecs, vecs_one):
            for (_, s, n), (_, sg, _) in zip(lay.field_slices(), one.field_slices()):
                pts = n // max(lay.nelv, 1)
                off = lay.elem_range()[0] * pts
                np.testing.assert_array_equal(a[s:s + n], g[sg + off:sg + off + n])   # bit for bit
    assert glob.shard(0, 2).n_v == 0 or nelgv > 1
    np.testing.assert_allclose(total, res2_one, rtol=1e-12, atol=0.0)


# ---- 8. error paths ------------------------------------------------------------------------------------------------

def test_error_paths(gpu):
    lay = LAYOUTS["2d"]
    ctx, _ = _context(lay)
    vs = [ctx.vector() for _ in range(7)]
    r2 = torch.zeros(1, dtype=torch.float64, device=ctx.device)
    w, ws = ctx.w.data_ptr(), ctx.ws.data_ptr()

    def sfd(n_vel, ptrs=None, flags=0):
        p = [x.ptr for x in vs] if ptrs is None else ptrs
        return ctx.lib.nkv_sfd_step(ctx._Lp, w, *p, 1.0, 0.0, 0.0, 0.1, -0.4, n_vel, r2.data_ptr(), ws, flags, ctx.stream)

    def tdf(n_vel, ptrs=None, flags=0):
        p = [x.ptr for x in vs[:3]] if ptrs is None else ptrs
        return ctx.lib.nkv_tdf_step(ctx._Lp, w, *p, -0.1, n_vel, r2.data_ptr(), ws, flags, ctx.stream)

    for call in (sfd, tdf):
        for n_vel in (1, 4, 3, 0, -1):                     # 3 > n_wf = 2 on this layout
            assert call(n_vel) == _lib.NKV_EINVAL
            assert "n_vel" in _lib.last_error()
        assert call(2) == _lib.NKV_OK
    for k in range(7):                                     # a null vector
        p = [x.ptr for x in vs]
        p[k] = None
        assert sfd(2, p) == _lib.NKV_EINVAL and "NULL" in _lib.last_error(), k
    for k in range(3):
        p = [x.ptr for x in vs[:3]]
        p[k] = None
        assert tdf(2, p) == _lib.NKV_EINVAL and "NULL" in _lib.last_error(), k
    assert ctx.lib.nkv_sfd_step(ctx._Lp, w, *[x.ptr for x in vs], 1.0, 0.0, 0.0, 0.1, -0.4, 2, None, ws, 0,
                                ctx.stream) == _lib.NKV_EINVAL
    p = [x.ptr for x in vs]
    p[5] = p[3]                                            # qd aliases qa
    assert sfd(2, p) == _lib.NKV_EINVAL and "alias" in _lib.last_error()
    # a 3-D layout takes n_vel = 3, and 2 (its third field then counts as a scalar)
    ctx3, _ = _context(LAYOUTS["3d_scalar"])
    v3 = [ctx3.vector() for _ in range(3)]
    for n_vel in (2, 3):
        assert ctx3.lib.nkv_tdf_step(ctx3._Lp, ctx3.w.data_ptr(), *[x.ptr for x in v3], -0.1, n_vel, r2.data_ptr(),
                                     ctx3.ws.data_ptr(), 0, ctx3.stream) == _lib.NKV_OK
    assert ctx3.lib.nkv_tdf_step(ctx3._Lp, ctx3.w.data_ptr(), *[x.ptr for x in v3], -0.1, 4, r2.data_ptr(),
                                 ctx3.ws.data_ptr(), 0, ctx3.stream) == _lib.NKV_EINVAL
    ctx.synchronize()


def test_pair_layout_is_refused(gpu):
    from nekstab_next_amd.vector import NekContext

    ctx = NekContext(pair_layout(NekLayout(2, 4, 2, 6)), max_cols=4)
    with pytest.raises(ValueError, match="PairLayout"):
        fixedp.SFD(ctx, UP4, UP5, DT, 1e-10)
    with pytest.raises(ValueError, match="PairLayout"):
        fixedp.TDF(ctx, 5.0, 1.0, 1e-10)


def test_residu_file(gpu, tmp_path):
    lay = NekLayout(2, 4, 2, 6)
    ctx, _ = _context(lay)
    sfd = fixedp.SFD(ctx, UP4, UP5, DT, 1e-10, residu=tmp_path / "residu.dat")
    v, fc = ctx.vector(), ctx.vector()
    v.fill_hash(1)
    sfd.start(v)
    v.fill_hash(2)
    res, rate, _ = sfd.step(v, fc)
    sfd.close()
    assert (tmp_path / "residu.dat").read_text() == fixedp.residu_line(DT, res, rate, 1e-10) + "\n"
