"""The checkpointed adjoint of the periodic-orbit tangent on the device: nkv_burgers_backward_rhs
(csrc/advdiff.hip) against the two kernels it restates, and OrbitFlow(checkpoint=c) / OrbitPropagator.rmatvec
(nekstab_next_amd/orbit.py), sequential and pipelined, against the stored orbit.

Every comparison is bit for bit: the recomputed stage states come from the launches of ``propagate`` on the same
inputs, and the fused right-hand side keeps the operand order of its parents.  Only the adjoint identity carries a
gate, the one of test_gpu_orbit.py: 4 times the restatement's own f64 defect (floor 1e-12)."""
import ctypes

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
import test_gpu_orbit as go

from nekstab_next_amd import _lib
from nekstab_next_amd import synthetic as syn
from nekstab_next_amd.layout import NekLayout
from nekstab_next_amd.sensitivity import gll_derivative

ROOT = ga.ROOT
pytestmark = pytest.mark.gpu

ODD = "odd-2d"            # lx1 = 3 in 2-D, 9 elements: n_v = 81
NSTEPS = 7
CS = (1, 2, 3, 4, 7, 9)
CASE_3D = (5, (2, 2, 2))
_nan = go._nan


# ---- nkv_burgers_backward_rhs ------------------------------------------------------------------------
class _Raw(gb._Raw):
    def __init__(self, name):
        if name != ODD:
            super().__init__(name)
            return
        from nekstab_next_amd.vector import NekContext

        lay = self.lay = NekLayout(ldim=2, lx1=3, lx2=1, nelgv=9)
        self.co = ar.box_mesh_2d(3, (3, 3), (ga.PI, ga.PI), amp=0.04)
        x, y = self.co["x"], self.co["y"]
        self.Bh = [2.0 * np.sin(x) * np.cos(y) + 0.5, -2.0 * np.cos(x) * np.sin(y)]
        self.kap = ga._kappas(lay)
        self.ctx = NekContext(lay, max_cols=4)
        self.n, self.pts = lay.n_v, lay.pts_v
        self.D, self.w = ga._dev(gll_derivative(lay.lx1)), ga._dev(syn.gll_weights(lay.lx1))
        self.xyz = [ga._dev(self.co[k]) for k in ("x", "y")]
        self.B = self.U = ga._dev(np.concatenate(self.Bh))
        self.st = torch.cuda.current_stream().cuda_stream

    def backward(self, X, X_stride, S, S_stride, u, u_stride, rX, rX_stride, ru, ru_stride, kappa, e0=0, e1=None):
        """nkv_burgers_backward_rhs on elements [e0, e1): every per-point pointer moved by e0 elements."""
        lay = self.lay
        e1 = self.n // self.pts if e1 is None else e1
        L = lay.c_struct()
        L.n_v = (e1 - e0) * self.pts
        off = 8 * e0 * self.pts
        xyz = [t.data_ptr() + off for t in self.xyz] + ([None] if lay.ldim == 2 else [])
        rc = self.ctx.lib.nkv_burgers_backward_rhs(ctypes.byref(L), lay.lx1, lay.ldim, self.D.data_ptr(),
                                                   self.w.data_ptr(), *xyz, X.data_ptr() + off, X_stride,
                                                   S.data_ptr() + off, S_stride, kappa.data_ptr(), u.data_ptr() + off,
                                                   lay.n_wf, u_stride, rX.data_ptr() + off, rX_stride,
                                                   ru.data_ptr() + off, ru_stride, self.st)
        assert rc == _lib.NKV_OK, _lib.last_error()


def _strided(rows, n, stride):
    t = _nan(len(rows) * stride)
    for f, row in enumerate(rows):
        t[f * stride: f * stride + n] = ga._dev(row)
    return t


@pytest.mark.parametrize("name", ["cyl", ODD] + gb.CASES_3D, ids=str)
def test_backward_rhs_equals_the_two_kernels(gpu, name):
    """r_X carries the bits of nkv_advdiff_rhs(u = U = X), r_u those of the adjoint nkv_linconv_rhs(u; S), with X
    and S two states and with X aliasing S; output strides above n_v leave the NaN gap untouched; a second call
    and element sub-ranges give the same bits."""
    raw = _Raw(name)
    lay, n, pts = raw.lay, raw.n, raw.pts
    nf = lay.n_wf
    assert (n % 2 == 1) == (name == ODD)
    E = n // pts
    kd = ga._dev(raw.kap)
    su, sx, sb, sr = n + 24, n + 16, n + 8, n + 40
    u = _strided(ga._fields(lay, raw.co), n, su)
    other = _strided(ga._fields(lay, raw.co, seed=11), n, sx)          # a second state, on a stride of its own
    base = raw.B                                                         # the case's base state, stride n
    for what, X, xs, S in (("X != S", other, sx, base), ("X is S", base, n, base)):
        wantX, wantu = _nan(nf * sb), _nan(nf * sr)
        raw.rhs(X, nf, xs, wantX, sb, kd, False, U=X, U_stride=xs)
        keep, raw.B = raw.B, S                                           # (lin reads raw.B with stride n)
        raw.lin(u, su, wantu, sr, kd, True)
        raw.B = keep
        wX, wu = wantX.cpu().numpy().reshape(nf, sb), wantu.cpu().numpy().reshape(nf, sr)
        assert np.all(np.isfinite(wX[:, :n])) and np.all(np.isfinite(wu[:, :n]))
        assert np.any(wX[:, :n] != 0.0) and np.any(wu[:, :n] != 0.0)
        rX, ru = _nan(nf * sb), _nan(nf * sr)
        raw.backward(X, xs, S, n, u, su, rX, sb, ru, sr, kd)
        gX, gu = rX.cpu().numpy().reshape(nf, sb), ru.cpu().numpy().reshape(nf, sr)
        print(f"{name} {what}: max |r_X - advdiff| {np.max(np.abs(gX[:, :n] - wX[:, :n])):.2e}, "
              f"max |r_u - linconv adjoint| {np.max(np.abs(gu[:, :n] - wu[:, :n])):.2e}")
        assert np.array_equal(gX[:, :n], wX[:, :n]), what
        assert np.array_equal(gu[:, :n], wu[:, :n]), what
        assert np.all(np.isnan(gX[:, n:])) and np.all(np.isnan(gu[:, n:]))   # the gaps are untouched
        aX, au = _nan(nf * sb), _nan(nf * sr)
        raw.backward(X, xs, S, n, u, su, aX, sb, au, sr, kd)
        assert np.array_equal(aX.cpu().numpy().reshape(nf, sb)[:, :n], gX[:, :n])
        assert np.array_equal(au.cpu().numpy().reshape(nf, sr)[:, :n], gu[:, :n])
        for e0, e1 in {(0, max(E // 2, 1)), (E // 2, E), (E - 1, E)}:
            pX, pu = _nan(nf * sb), _nan(nf * sr)
            raw.backward(X, xs, S, n, u, su, pX, sb, pu, sr, kd, e0, e1)
            for part, got, s in ((pX, gX, sb), (pu, gu, sr)):
                p = part.cpu().numpy().reshape(nf, s)
                assert np.array_equal(p[:, e0 * pts:e1 * pts], got[:, e0 * pts:e1 * pts])
                assert np.all(np.isnan(p[:, :e0 * pts])) and np.all(np.isnan(p[:, e1 * pts:]))


def test_entry_checks(gpu):
    """Every NKV_EINVAL of nkv_burgers_backward_rhs with its message, nothing launched; an empty shard returns
    NKV_OK and reads no pointer."""
    lay = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=3, n_scalars=1)
    n, nf = lay.n_v, lay.n_wf
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.full((24 * n,), 7.0, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    L = lay.c_struct()
    u, X, S, rX, ru = (p + 8 * k * n for k in (4, 8, 12, 16, 20))
    far = 8 * (nf - 1) * n + 8 * (n - 1)
    V = dict(L=ctypes.byref(L), lx1=4, ldim=3, D=p, w=p, xm=p, ym=p, zm=p, X=X, X_stride=n, S=S, S_stride=n, kappa=p,
             u=u, nfld=nf, u_stride=n, r_X=rX, rX_stride=n, r_u=ru, ru_stride=n, stream=st)
    assert len(V) == len(_lib._SIGNATURES["nkv_burgers_backward_rhs"][1])
    both, rx, rU = "r_X overlaps r_u", "r_X overlaps X, S or u", "r_u overlaps X, S or u"
    bad = [("ldim", 4, "ldim"), ("lx1", 11, "lx1"), ("lx1", 5, "do not divide"), ("zm", None, "zm"),
           ("X_stride", n - 1, "stride"), ("S_stride", n - 1, "stride"), ("u_stride", n - 1, "stride"),
           ("rX_stride", n - 1, "stride"), ("ru_stride", n - 1, "stride"), ("nfld", 2, "nfld=2 < ldim=3"),
           ("D", None, "D is NULL"), ("w", None, "w is NULL"), ("xm", None, "xm is NULL"), ("ym", None, "ym is NULL"),
           ("X", None, "X is NULL"), ("S", None, "S is NULL"), ("kappa", None, "kappa is NULL"), ("u", None, "u is NULL"),
           ("r_X", None, "r_X is NULL"), ("r_u", None, "r_u is NULL"),
           ("r_u", rX, both), ("r_u", rX + far, both), ("r_X", ru - far, both),
           ("r_X", X, rx), ("r_X", S + far, rx), ("r_X", u - far, rx), ("r_X", S - far, rx),
           ("r_u", X, rU), ("r_u", S, rU), ("r_u", u + far, rU), ("r_u", u - far, rU), ("r_u", S - far, rU)]
    for key, val, msg in bad:
        assert lib.nkv_burgers_backward_rhs(*{**V, key: val}.values()) == _lib.NKV_EINVAL, (key, val)
        assert "burgers_backward_rhs" in _lib.last_error() and msg in _lib.last_error(), (key, _lib.last_error())
    torch.cuda.synchronize()
    assert torch.all(buf == 7.0)                                     # nothing was launched
    Le = NekLayout(ldim=3, lx1=4, lx2=2, nelgv=0, n_scalars=1).c_struct()
    assert lib.nkv_burgers_backward_rhs(*{**V, "L": ctypes.byref(Le), "D": None, "X": None, "S": None, "u": None,
                                          "r_X": None, "r_u": None}.values()) == _lib.NKV_OK
    torch.cuda.synchronize()
    assert torch.all(buf == 7.0)


# ---- the storage modes -------------------------------------------------------------------------------
_FLOWS = {}


def _flows(name):
    """(ctx weighted by bm1, ViscousBurgers over 7 steps, the stored OrbitFlow, the checkpointed ones by c, two
    states, a vector to apply to, the f64 restatement or None) of a case with cos and sin forcing, built once."""
    if name not in _FLOWS:
        from nekstab_next_amd.burgers import ViscousBurgers
        from nekstab_next_amd.orbit import OrbitFlow
        from nekstab_next_amd.vector import NekContext

        o64 = None
        if name == go.E2E:
            co, mask = orf.e2e_mesh()
            lay = NekLayout(**go.E2E_LAY)
            kap, dt = list(orf.E2E["kappa"]), orf.E2E["dt"]
            target, gc, gs = orf.e2e_forcing(co)
            g0 = None
        else:
            lay, co, _, mask, kap = gb._case(name)
            dt = 2e-3
            x, y, z = co["x"], co["y"], co["z"]
            g0 = np.stack([0.3 * np.sin(x + 0.2 * f) * np.cos(y) for f in range(lay.n_wf)])
            gc = np.stack([0.2 * np.cos(x) * np.sin(y + 0.1 * f) * (1.0 + 0.2 * z) for f in range(lay.n_wf)])
            gs = np.stack([0.1 * np.sin(2.0 * x + z) * np.cos(y - 0.3 * f) for f in range(lay.n_wf)])
        ctx0 = NekContext(lay, max_cols=4)
        flow = ViscousBurgers(ctx0, co, kap, dt, NSTEPS, forcing=None if g0 is None else list(g0), mask=mask)
        if name == go.E2E:
            flow.steady_forcing(list(target))
            zero = [np.zeros(lay.n_v)] * lay.ldim
            o64 = orf.Orbit(br.Burgers(ar.Reference(lay.lx1, lay.ldim, co, zero, mask=mask, dtype=np.float64), kap, dt,
                                       NSTEPS), g0=None, gc=gc, gs=gs)
            o64.steady_g0(target)
        stored = OrbitFlow(flow, cos=list(gc), sin=list(gs))
        ck = {c: OrbitFlow(flow, cos=list(gc), sin=list(gs), checkpoint=c) for c in CS}
        ctx = NekContext(lay, weights=flow.bm1, max_cols=64)
        q = gb._vector(ctx, np.stack(ga._fields(lay, co, seed=4)))
        q2 = gb._vector(ctx, np.stack(ga._fields(lay, co, seed=6)))
        x = gb._vector(ctx, np.stack(ga._fields(lay, co, seed=9)))
        _FLOWS[name] = (ctx, flow, stored, ck, q, q2, x, o64)
    return _FLOWS[name]


_WANT = {}


def _want(name):
    """The stored mode's propagate, matvec and rmatvec of a case (computed once, left unchanged)."""
    if name not in _WANT:
        ctx, flow, stored, ck, q, q2, x, _ = _flows(name)
        phi, mv, rmv = ga._sentinel(ctx), ga._sentinel(ctx), ga._sentinel(ctx)
        stored.propagate(q, phi)
        stored.prop.matvec(x, mv)
        stored.prop.rmatvec(x, rmv)
        assert not torch.equal(mv.storage, rmv.storage) and bool(torch.all(torch.isfinite(rmv.storage)))
        _WANT[name] = (phi, mv, rmv)
    return _WANT[name]


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("name", [go.E2E, CASE_3D], ids=str)
def test_storage_modes_give_the_same_bits(gpu, name, c):
    """Over 7 steps with c steps per segment: propagate, matvec and rmatvec (sequential, pipelined and by default)
    equal the stored mode's; orbit_bytes is what was allocated, within the bound, and below the stored mode's at
    c = 2."""
    ctx, flow, stored, ck, q, q2, x, _ = _flows(name)
    phi, mv, rmv = _want(name)
    of = ck[c]
    lay = ctx.layout
    seg = lay.n_wf * lay.sv
    J, W = -(-NSTEPS // c), min(c, NSTEPS)
    assert of.checkpoint == c and of.orbit_bytes == 8 * (of._orbit.numel() - 2) == 8 * seg * (J + 8 * W + 4)
    assert of.orbit_bytes <= 8 * lay.n_wf * lay.sv * (J + 8 * min(c, NSTEPS) + 4)
    assert stored.orbit_bytes == 8 * (stored._orbit.numel() - 2) == 4 * NSTEPS * seg * 8
    if c == 2:
        assert of.orbit_bytes < stored.orbit_bytes
    y = ga._sentinel(ctx)
    of.propagate(q, y)
    assert torch.equal(y.storage, phi.storage)
    op = of.linearized(q)
    assert op is of.prop
    y = ga._sentinel(ctx)
    op.matvec(x, y)
    assert torch.equal(y.storage, mv.storage)
    for fused in (False, True, None):
        y = ga._sentinel(ctx)
        if fused is None:
            op.rmatvec(x, y)
        else:
            op.rmatvec(x, y, fused=fused)
        assert torch.equal(y.storage, rmv.storage), (c, fused)
        ga._check_rest(lay, y.to_packed())
    # a fresh propagate, then the pipelined walk first: the windows hold the last two segments, every segment
    # before them is recomputed next to the adjoint of the one after it, c steps of four stages each
    of.propagate(q, ga._sentinel(ctx))
    calls = []
    real = of.ctx.call
    of.ctx.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        y = ga._sentinel(ctx)
        op.rmatvec(x, y, fused=True)
    finally:
        del of.ctx.call
    assert torch.equal(y.storage, rmv.storage)
    assert calls.count("nkv_burgers_backward_rhs") == 4 * c * max(J - 2, 0)
    assert calls.count("nkv_linconv_rhs") == 4 * (NSTEPS - c * max(J - 2, 0))
    assert calls.count("nkv_advdiff_rhs") == 0


@pytest.mark.parametrize("fused", [False, True], ids=["sequential", "pipelined"])
def test_call_sequences(gpu, fused):
    """At c = 3: two rmatvec in a row, rmatvec right after propagate (the last segment's window is hit), after
    matvec, after linearized(q2) with another state, with time_derivative in between: every result equals the
    stored mode's under the same sequence."""
    ctx, flow, stored, ck, q, q2, x, _ = _flows(go.E2E)
    of = ck[3]

    def sequence(f, **kw):
        out = []

        def run(fn, *a, **k):
            y = ga._sentinel(ctx)
            fn(*a, y, **k)
            out.append(y.storage.clone())

        run(f.propagate, q)
        run(f.prop.rmatvec, x, **kw)                 # right after propagate
        run(f.prop.rmatvec, x, **kw)                 # twice in a row
        run(f.prop.matvec, x)
        run(f.prop.rmatvec, x, **kw)                 # after matvec
        op = f.linearized(q2)                        # another state: the orbit is run again
        run(op.rmatvec, x, **kw)
        run(f.time_derivative, q)
        run(op.rmatvec, x, **kw)                     # time_derivative left the windows alone
        run(op.matvec, x)
        op = f.linearized(q2)                        # the same state: nothing is run again
        run(op.rmatvec, x, **kw)
        op = f.linearized(q)
        run(op.rmatvec, x, **kw)
        return out

    want = sequence(stored)
    hits = []
    real = of._recompute

    def counted(j, k0=0):
        hits.append((j, k0, of._holds(j)))
        real(j, k0)

    of._recompute = counted
    try:
        got = sequence(of, fused=fused)
    finally:
        del of._recompute
    assert len(got) == len(want) == 11
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), k
    assert torch.equal(got[1], got[2]) and torch.equal(got[5], got[7]) and not torch.equal(got[1], got[5])
    assert hits[0] == (2, 0, True)                   # the first walk found the last segment in its window
    assert any(h == (2, 0, False) for h in hits)     # and a later one had to fill it


def test_adjoint_identity(gpu):
    """<A x, y> = <x, A^+ y> in the bm1 inner product for the checkpointed operator (c = 3, pipelined), under the
    gate of test_gpu_orbit.py: the defect over sum bm1 |A x| |y| within 4 times the restatement's own (floor
    1e-12)."""
    ctx, flow, stored, ck, q, q2, x, o64 = _flows(go.E2E)
    lay = ctx.layout
    op = ck[3].linearized(q)
    a, b, Aa, Atb = ctx.vector(), ctx.vector(), ctx.vector(), ctx.vector()
    a.fill_hash(21)
    b.fill_hash(22)
    op.matvec(a, Aa)
    op.rmatvec(b, Atb, fused=True)
    bm1 = flow.bm1.cpu().numpy()
    lhs, rhs = ctx.dot(b, Aa, time=False), ctx.dot(Atb, a, time=False)
    scale = float(np.sum(bm1 * np.abs(gb._rows(lay, Aa.to_packed())) * np.abs(gb._rows(lay, b.to_packed()))))
    defect = abs(lhs - rhs) / scale
    ah, bh = gb._rows(lay, a.to_packed()), gb._rows(lay, b.to_packed())
    orb64 = o64.propagate(gb._rows(lay, q.to_packed()))[1]
    Pa, Ptb = o64.tangent(ah, orb64), o64.adjoint(bh, orb64)
    w = o64.bg.ref.bm1
    own = abs(float(np.sum(w * bh * Pa) - np.sum(w * Ptb * ah))) / float(np.sum(w * np.abs(Pa) * np.abs(bh)))
    print(f"adjoint defect: device {defect:.2e}, restatement {own:.2e}")
    assert scale > 0 and defect <= max(4 * own, 1e-12)


def test_adjoint_floquet_workflow(gpu):
    """krylov_schur through LegacyMatvec(3.21, .) on the checkpointed operator, sequential and pipelined, returns
    the stored mode's Ritz values and residuals exactly (k_dim = 48, as the orbit end-to-end test)."""
    from nekstab_next_amd.config import KrylovSchurConfig
    from nekstab_next_amd.krylov_schur import krylov_schur
    from nekstab_next_amd.operators import LegacyMatvec
    from nekstab_next_amd.orbit import OrbitPropagator

    ctx, flow, stored, ck, q, q2, x, _ = _flows(go.E2E)
    cfg = KrylovSchurConfig(k_dim=48, schur_tgt=3, eigen_tol=1e-12)

    def ritz(of):
        seed = ctx.vector()
        seed.fill_hash(11)
        return krylov_schur(ctx, LegacyMatvec(3.21, of.linearized(q)), seed, cfg)

    want = ritz(stored)
    assert np.all(np.isfinite(want.vals)) and abs(want.vals[0]) > 0
    keep = OrbitPropagator.FUSED_DEFAULT
    try:
        for fused in (False, True):
            OrbitPropagator.FUSED_DEFAULT = fused     # the drivers call rmatvec(x, y)
            got = ritz(ck[3])
            assert np.array_equal(got.vals, want.vals) and np.array_equal(got.residual, want.residual), fused
            assert got.schur_cnt == want.schur_cnt
    finally:
        OrbitPropagator.FUSED_DEFAULT = keep


def test_argument_errors(gpu):
    from nekstab_next_amd.orbit import OrbitFlow

    flow = _flows(go.E2E)[1]
    with pytest.raises(ValueError, match="store=True"):
        OrbitFlow(flow, store=False, checkpoint=2)
    for bad in (0, -2, 1.5, "sqrt"):
        with pytest.raises(ValueError, match="checkpoint"):
            OrbitFlow(flow, checkpoint=bad)
    auto = OrbitFlow(flow, checkpoint="auto")
    assert auto.checkpoint == max(1, round((NSTEPS / 8) ** 0.5)) == 1
    with pytest.raises(RuntimeError, match="no orbit yet"):
        auto.prop.rmatvec(_flows(go.E2E)[6], ga._sentinel(_flows(go.E2E)[0]))


# ---- shards ------------------------------------------------------------------------------------------
_SHARD_CASES = go._SHARD_CASES


def _jobs(rank, world):
    """OrbitPropagator.rmatvec over 5 steps about a stored orbit and about a checkpointed one (c = 2: a shorter
    last segment), sequential and pipelined, with face_average="auto" on every case, this rank's slice."""
    from nekstab_next_amd.burgers import ViscousBurgers
    from nekstab_next_amd.comm import Comm
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
        flow = ViscousBurgers(ctx, co, kap, 1e-3, 5, forcing=g0, mask=mask_g[sl], face_average="auto")
        q, x, y = ctx.vector(), ctx.vector(), ctx.vector()
        q.fill_hash(17)
        x.fill_hash(18)
        for key, kw in (("stored", {}), ("ck", dict(checkpoint=2))):
            of = OrbitFlow(flow, cos=gc, sin=gs, **kw)
            op = of.linearized(q)
            for fused in ((None,) if key == "stored" else (False, True)):
                if fused is None:
                    op.rmatvec(x, y)
                else:
                    op.rmatvec(x, y, fused=fused)
                res[(key, fused, name)] = gb._rows(lay, y.to_packed())
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
    """Two gloo ranks sharing the GPU: the checkpointed rmatvec, pipelined and sequential, equals the one-rank
    result bit for bit on every rank's slice, and that equals the stored mode's.  The one-element case leaves
    rank 0 an empty shard, which takes part in every exchange and touches nothing."""
    one, got = _world(1)[0], _world(2)
    lay_g = gb._case(name)[0]
    want = one[("stored", None, name)]
    assert np.any(want != 0.0) and np.all(np.isfinite(want))
    for fused in (False, True):
        assert np.array_equal(one[("ck", fused, name)], want), fused
    for r in range(2):
        sh = lay_g.shard(r, 2)
        e0, e1 = sh.elem_range()
        sl = slice(e0 * sh.pts_v, e1 * sh.pts_v)
        for key in (("stored", None, name), ("ck", False, name), ("ck", True, name)):
            np.testing.assert_array_equal(got[r][key], want[..., sl], err_msg=f"{key} rank {r}")
    if name == (8, (1, 1, 1)):
        assert lay_g.shard(0, 2).n_v == 0 and got[0][("ck", True, name)].shape == (lay_g.n_wf, 0)
