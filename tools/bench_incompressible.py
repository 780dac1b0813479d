"""Time one divergence-free projection (pressure.DivergenceFreeProjector) and the three kernels of its CG
iteration (nkv_pressure_gradt, nkv_pressure_div, nkv_pressure_cg_update; csrc/pressure.hip).

  python tools/bench_incompressible.py [--elements 22088] [--tol 1e-12] [--reps 5] [--rounds 5]
                                       [--lib path/to/libnekkrylov.so] [--out profiles/incompressible_bench.json]

The case is bench_advdiff.py's box: 3-D, lx1=8, E=22,088 (11.3M GLL points per field, 4.8M pressure values), no
mask (an open domain: E is positive definite, no deflation).  The legs alternate inside each round in ONE process
(only numbers of one process compare); per leg the median and the minimum over the rounds go out as one JSON
line.  Bytes are the algorithmic streams, in doubles per GLL point n and per pressure value m:
  gradt (p = r + beta p on the load):  2 ldim n (coordinates in, D^T p out) + 3 m (r, p in; p out)
  div (minv on the load, partials):    (2 ldim + 1) n (coordinates, velocity, minv in) + 2 m (p in; E p out)
  cg_update:                           6 m (x, r in and out; p, E p in)
GB/s against the 8 TB/s HBM3E peak.  The dsavg batch of ldim segments between gradt and div has no byte model
here (gs.py's).  The last line: the CG iterations of one projection of a hashed continuous field, its time and
the time per iteration.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from nekstab_next_amd import _lib  # noqa: E402

PEAK = 8.0e12


def bench(a):
    from bench_advdiff import _mesh
    from nekstab_next_amd.gs import average_segments
    from nekstab_next_amd.pressure import DivergenceFreeProjector
    from nekstab_next_amd.vector import NekContext

    lay, co, _ = _mesh("box", a.elements)
    ctx = NekContext(lay, max_cols=4)
    n, d = lay.n_v, lay.ldim
    proj = DivergenceFreeProjector(ctx, co, tol=a.tol, maxiter=a.maxiter, closed=False)
    m = proj.npz
    x, y = ctx.vector(), ctx.vector()
    x.fill_hash(3)
    proj.op.project(x)
    # one projection: iterations and time
    proj.apply(x, y)                      # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    proj.apply(x, y)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    its = proj.last_iterations
    B = proj.PARTIALS
    minv = proj.op._minv

    def gradt():
        proj.ctx.call("nkv_pressure_gradt", *proj._head, proj._p.data_ptr(), proj._r.data_ptr(), proj._rr[0].data_ptr(),
                      proj._rr[1].data_ptr(), B, 0, proj._t.data_ptr(), lay.sv, ctx.stream)

    def dsavg():
        average_segments(proj.op.face_average, proj._t_ptrs)

    def div():
        proj._div(proj._t.data_ptr(), minv, proj._Ep, pv=proj._p)

    def update():
        proj._update(proj._red, B, proj._rr[0], B, proj._rr[1], init=False)

    def iteration():
        gradt()
        dsavg()
        div()
        update()

    legs = {
        "pressure_gradt": (gradt, 2 * d * n + 3 * m),
        "dsavg_batch": (dsavg, 0),
        "pressure_div": (div, (2 * d + 1) * n + 2 * m),
        "pressure_cg_update": (update, 6 * m),
        "cg_iteration": (iteration, (4 * d + 1) * n + 11 * m),
    }
    for fn, _ in legs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, (fn, _) in legs.items():
            s.record()
            for _ in range(a.reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / a.reps)
    lines = [dict(case="box", E=lay.nelv, lx1=lay.lx1, ldim=d, n_v=n, npz=m, reps=a.reps, rounds=a.rounds, tol=a.tol,
                  device=torch.cuda.get_device_properties(ctx.device).gcnArchName.split(":")[0])]
    for name, (_, doubles) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        byts = 8 * doubles
        lines.append(dict(case="box", leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), GB=round(byts / 1e9, 4),
                          gbs_median=round(byts / (med * 1e-3) / 1e9, 1), frac_peak=round(byts / (med * 1e-3) / PEAK, 3)))
    lines.append(dict(case="box", leg="projection", cg_iterations=its, ms=round(1e3 * wall, 2),
                      ms_per_iteration=round(1e3 * wall / max(its, 1), 4)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=22088)
    ap.add_argument("--tol", type=float, default=1e-12)
    ap.add_argument("--maxiter", type=int, default=20000)
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
