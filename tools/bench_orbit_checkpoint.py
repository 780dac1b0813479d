"""Time the checkpointed adjoint of the periodic-orbit tangent (nkv_burgers_backward_rhs, csrc/advdiff.hip;
orbit.OrbitFlow(checkpoint=c)): the fused right-hand side next to the two launches it replaces (nkv_advdiff_rhs
with u = U = X, then the adjoint nkv_linconv_rhs of u about S); one paired step of the pipelined backward sweep next
to one unfused base step plus one unfused adjoint step; and OrbitPropagator.rmatvec over a short orbit about the
stored orbit and about a checkpointed one, sequential (fused=False) and pipelined (fused=True), at the same nsteps.

  python tools/bench_orbit_checkpoint.py [--elements 22088] [--nsteps 8] [--checkpoint 2] [--reps 5] [--rounds 5]
                                         [--lib path/to/libnekkrylov.so] [--out profiles/orbit_checkpoint_bench.json]

The case, the process and the shape are bench_orbit.py's: the box of bench_advdiff.py, 3-D, lx1=8, E=22,088 (11.3M
points per field), vx vy vz t (n_wf = 4).  The legs alternate inside each round in ONE process (only numbers of
one process compare); per leg the median and the minimum over the rounds go out as one JSON line.  The yardstick of
every comparison is the unfused sequence of kernels, not the fused code.  Bytes are the algorithmic streams per
point, in doubles: 2 ldim + 2 n_wf for nkv_advdiff_rhs, ldim + 3 n_wf for nkv_linconv_rhs, ldim + 5 n_wf for the
fused pass (coordinates; X, S, u in; r_X, r_u out): 14 + 15 = 29 against 23; GB/s against the 8 TB/s HBM3E peak.
The fused results are compared with the pair's bit for bit first, and the three rmatvec with each other.  With
nsteps = 8 and c = 2 there are four segments, so every checkpointed rmatvec recomputes all of them (a window never
still holds what the next walk needs first).  --lib times another build of the library, e.g. one compiled with
-DNKV_BWD_WAVES=0.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from nekstab_next_amd import _lib  # noqa: E402

PEAK = 8.0e12


def bench(a):
    import numpy as np

    from bench_advdiff import _mesh
    from nekstab_next_amd.burgers import ViscousBurgers
    from nekstab_next_amd.orbit import OrbitFlow
    from nekstab_next_amd.vector import NekContext

    lay, co, U = _mesh("box", a.elements)
    ctx = NekContext(lay, max_cols=4)
    n, sv, nf, d = lay.n_v, lay.sv, lay.n_wf, lay.ldim
    N, c = a.nsteps, a.checkpoint
    part = lambda amp, ph: [amp * np.sin(co["x"] + 0.2 * f + ph) * np.cos(co["y"]) for f in range(nf)]   # noqa: E731
    flow = ViscousBurgers(ctx, co, [0.01 * (1 + f) for f in range(nf)], 1e-4, N, forcing=part(0.3, 0.0))
    stored = OrbitFlow(flow, cos=part(0.2, 0.5), sin=part(0.1, 1.0))
    ck = OrbitFlow(flow, cos=part(0.2, 0.5), sin=part(0.1, 1.0), checkpoint=c)
    assert ck._nseg >= 3, "fewer than three segments: a walk would find segments still in the windows"
    op = flow.lin
    q, s, x, y, ys, yf, yp = (ctx.vector() for _ in range(7))
    q.zero()                    # the base state of bench_burgers.py: the box flow and a smooth scalar
    for f, b in enumerate(list(U) + [np.cos(co["x"]) * np.sin(0.5 * co["y"] + 0.3 * co["z"])]):
        q.storage[f * sv: f * sv + n] = torch.as_tensor(np.ascontiguousarray(b, dtype=np.float64)).to(ctx.device)
    s.fill_hash(5)              # a second state to linearise about
    s.storage.mul_(0.1).add_(q.storage)
    x.fill_hash(3)
    op.project(x)
    f64 = dict(dtype=torch.float64, device=ctx.device)
    rX, ru, fX, fu = (torch.zeros(nf * sv, **f64) for _ in range(4))
    st = ctx.stream
    head = (lay.lx1, d, op.D.data_ptr(), op.w.data_ptr(), *op._xyz_ptrs())
    kap = op.kappa.data_ptr()

    def self_advection():
        ctx.call("nkv_advdiff_rhs", *head, q.ptr, sv, kap, q.ptr, nf, sv, rX.data_ptr(), sv, 0, st)

    def linconv_adjoint():
        ctx.call("nkv_linconv_rhs", *head, s.ptr, sv, kap, x.ptr, nf, sv, ru.data_ptr(), sv, 1, st)

    def pair():
        self_advection()
        linconv_adjoint()

    def fused():
        ctx.call("nkv_burgers_backward_rhs", *head, q.ptr, sv, s.ptr, sv, kap, x.ptr, nf, sv, fX.data_ptr(), sv,
                 fu.data_ptr(), sv, st)

    stored.propagate(q, y)
    ck.propagate(q, y)
    so, co_ = stored.linearized(q), ck.linearized(q)
    # one step of the backward sweep: the adjoint of the orbit's last step, base step m of the segment before its own
    na = N - 1
    m = ck._span(na // c - 1)[0]
    slots = [ck._slot(m, i) for i in range(4)]

    def unfused_step():
        ck._wtag = [None, None]   # (the step writes into a window behind its tag)
        ck._base_step(m, slots, ck._next(m), 0)
        co_._adjoint_steps((na,), yp)

    def paired_step():
        ck._wtag = [None, None]
        co_._paired_step(na, m, yp)

    yp.copy_from(x)
    legs = {
        f"advdiff_rhs_self_{nf}": (self_advection, 2 * d + 2 * nf),
        f"linconv_rhs_adjoint_{nf}": (linconv_adjoint, d + 3 * nf),
        f"pair_{nf}": (pair, 3 * d + 5 * nf),
        f"fused_{nf}": (fused, d + 5 * nf),
        "unfused_base_plus_adjoint_step": (unfused_step, 0),
        "paired_step": (paired_step, 0),
        "rmatvec_stored": (lambda: so.rmatvec(x, ys), 0),
        "rmatvec_checkpoint_sequential": (lambda: co_.rmatvec(x, y, fused=False), 0),
        "rmatvec_checkpoint_pipelined": (lambda: co_.rmatvec(x, yf, fused=True), 0),
    }
    for fn, _ in legs.values():   # warm every shape
        fn()
    torch.cuda.synchronize()
    bits = dict(r_X=bool(torch.equal(rX.view(nf, sv)[:, :n], fX.view(nf, sv)[:, :n])),
                r_u=bool(torch.equal(ru.view(nf, sv)[:, :n], fu.view(nf, sv)[:, :n])),
                rmatvec_sequential=bool(torch.equal(ys.storage, y.storage)),
                rmatvec_pipelined=bool(torch.equal(ys.storage, yf.storage)))
    times = {k: [] for k in legs}
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, (fn, _) in legs.items():
            t0.record()
            for _ in range(a.reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / a.reps)
    lines = [dict(case="box", E=lay.nelv, lx1=lay.lx1, ldim=d, n_wf=nf, n_v=n, sv=sv, reps=a.reps, rounds=a.rounds,
                  nsteps=N, checkpoint=c, segments=ck._nseg, same_bits=bits,
                  orbit_bytes=dict(stored=stored.orbit_bytes, checkpoint=ck.orbit_bytes),
                  device=torch.cuda.get_device_properties(ctx.device).gcnArchName.split(":")[0])]
    print(f"orbit_bytes: stored {stored.orbit_bytes}, checkpoint={c} {ck.orbit_bytes} (sequential and pipelined share it)",
          file=sys.stderr)
    out = {}
    for name, (_, doubles) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        byts = 8 * doubles * n
        out[name] = dict(case="box", leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), GB=round(byts / 1e9, 4),
                         gbs_median=round(byts / (med * 1e-3) / 1e9, 1), frac_peak=round(byts / (med * 1e-3) / PEAK, 3))
        lines.append(out[name])
    ms = {k: v["ms_median"] for k, v in out.items()}
    lines.append(dict(case="box", fused_over_pair=round(ms[f"fused_{nf}"] / ms[f"pair_{nf}"], 3),
                      byte_model=round((d + 5 * nf) / (3 * d + 5 * nf), 3),
                      paired_over_unfused_step=round(ms["paired_step"] / ms["unfused_base_plus_adjoint_step"], 3),
                      pipelined_over_sequential=round(ms["rmatvec_checkpoint_pipelined"] /
                                                      ms["rmatvec_checkpoint_sequential"], 3),
                      sequential_over_stored=round(ms["rmatvec_checkpoint_sequential"] / ms["rmatvec_stored"], 3),
                      pipelined_over_stored=round(ms["rmatvec_checkpoint_pipelined"] / ms["rmatvec_stored"], 3)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=22088)
    ap.add_argument("--nsteps", type=int, default=8)
    ap.add_argument("--checkpoint", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    _lib.load(a.lib)
    _lib.require_gpu()
    lines = []
    for ln in bench(a):
        print(json.dumps(ln), flush=True)
        lines.append(ln)
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
