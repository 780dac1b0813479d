"""Time the divergence-free projection (pressure.DivergenceFreeProjector) with and without the fast-diagonalisation
preconditioner, and the kernels of either CG iteration (csrc/pressure.hip), in ONE process.

  python tools/bench_pressure_precond.py [--elements 22088] [--tol 1e-12] [--reps 5] [--rounds 3]
                                         [--lib path/to/libnekkrylov.so] [--out profiles/pressure_precond_bench.json]

The case is bench_incompressible.py's: the 3-D box, lx1 = 8, E = 22,088 (11.3M GLL points per field, 4.77M pressure
values), no mask.  Per setting (preconditioner None and "fdm") the legs of one iteration alternate inside each round;
per leg the median and the minimum over the rounds go out as one JSON line.  Bytes are the algorithmic streams of
bench_incompressible.py, in doubles per GLL point n and per pressure value m, and for the new kernels
  pgradt (p = (z - zeta) + beta p on the load):  2 ldim n + 3 m     (the stream of gradt: z in for r)
  precond (z = M r, partials):                   2 m                (r in, z out; c is ldim doubles an element)
GB/s against the 8 TB/s HBM3E peak.  Then one projection of a hashed continuous field per setting, the settings
alternating over --rounds rounds: the iterations, the median and minimum time and the time per iteration, and the
ratio of the two whole-projection times.
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


def _legs(proj, pre):
    """{leg: (callable, doubles moved)} of one iteration of ``proj``."""
    from nekstab_next_amd.gs import average_segments

    ctx, lay = proj.ctx, proj.ctx.layout
    n, d, m, B = lay.n_v, lay.ldim, proj.npz, proj.PARTIALS
    minv = proj.op._minv

    def dsavg():
        average_segments(proj.op.face_average, proj._t_ptrs)

    def div():
        proj._div(proj._t.data_ptr(), minv, proj._Ep, pv=proj._p)

    if pre is None:
        def gradt():
            ctx.call("nkv_pressure_gradt", *proj._head, proj._p.data_ptr(), proj._r.data_ptr(), proj._rr[0].data_ptr(),
                     proj._rr[1].data_ptr(), B, 0, proj._t.data_ptr(), lay.sv, ctx.stream)

        def update():
            proj._update(proj._red, B, proj._rr[0], B, proj._rr[1], init=False)

        def iteration():
            gradt()
            dsavg()
            div()
            update()

        return {"pressure_gradt": (gradt, 2 * d * n + 3 * m), "dsavg_batch": (dsavg, 0),
                "pressure_div": (div, (2 * d + 1) * n + 2 * m), "pressure_cg_update": (update, 6 * m),
                "cg_iteration": (iteration, (4 * d + 1) * n + 11 * m)}

    a, b = (t.data_ptr() for t in proj._pz)

    def pgradt():
        ctx.call("nkv_pressure_pgradt", *proj._head, proj._p.data_ptr(), proj._z.data_ptr(), a + 8 * B, b + 8 * B, None, B,
                 0.0, 0, proj._t.data_ptr(), lay.sv, ctx.stream)

    def update():
        ctx.call_nl("nkv_pressure_cg_update", m, proj._x.data_ptr(), proj._r.data_ptr(), proj._p.data_ptr(),
                    proj._Ep.data_ptr(), proj._red.data_ptr(), B, a + 8 * B, B, 1.0 / max(proj.npz_global, 1), 0, 0, b,
                    ctx.stream)

    def precond():
        ctx.call_nl("nkv_pressure_precond", *proj._fdm_head, proj._r.data_ptr(), proj._z.data_ptr(), b + 8 * B, ctx.stream)

    def iteration():
        pgradt()
        dsavg()
        div()
        update()
        precond()

    return {"pressure_pgradt": (pgradt, 2 * d * n + 3 * m), "dsavg_batch": (dsavg, 0),
            "pressure_div": (div, (2 * d + 1) * n + 2 * m), "pressure_cg_update": (update, 6 * m),
            "pressure_precond": (precond, 2 * m), "pcg_iteration": (iteration, (4 * d + 1) * n + 13 * m)}


def bench(a):
    from bench_advdiff import _mesh
    from nekstab_next_amd.pressure import DivergenceFreeProjector
    from nekstab_next_amd.vector import NekContext

    lay, co, _ = _mesh("box", a.elements)
    ctx = NekContext(lay, max_cols=4)
    n, d = lay.n_v, lay.ldim
    settings = (None, "fdm")
    projs = {pre: DivergenceFreeProjector(ctx, co, tol=a.tol, maxiter=a.maxiter, closed=False, preconditioner=pre)
             for pre in settings}
    x, y = ctx.vector(), ctx.vector()
    x.fill_hash(3)
    projs[None].op.project(x)
    lines = [dict(case="box", E=lay.nelv, lx1=lay.lx1, ldim=d, n_v=n, npz=projs[None].npz, reps=a.reps, rounds=a.rounds,
                  tol=a.tol, device=torch.cuda.get_device_properties(ctx.device).gcnArchName.split(":")[0])]
    # whole projections, the settings alternating (the first round warms and is dropped)
    wall, its = {pre: [] for pre in settings}, {}
    for rnd in range(a.rounds + 1):
        for pre in settings:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            projs[pre].apply(x, y)
            torch.cuda.synchronize()
            if rnd:
                wall[pre].append(time.perf_counter() - t0)
            its[pre] = projs[pre].last_iterations
    # the legs of one iteration (the CG vectors hold the state the last solve left)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for pre in settings:
        legs = _legs(projs[pre], pre)
        for fn, _ in legs.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for name, (fn, _) in legs.items():
                s.record()
                for _ in range(a.reps):
                    fn()
                e.record()
                torch.cuda.synchronize()
                times[name].append(s.elapsed_time(e) / a.reps)
        for name, (_, doubles) in legs.items():
            med, mn = statistics.median(times[name]), min(times[name])
            byts = 8 * doubles
            lines.append(dict(case="box", preconditioner=pre, leg=name, ms_median=round(med, 4), ms_min=round(mn, 4),
                              GB=round(byts / 1e9, 4), gbs_median=round(byts / (med * 1e-3) / 1e9, 1),
                              frac_peak=round(byts / (med * 1e-3) / PEAK, 3)))
    med = {}
    for pre in settings:
        med[pre] = statistics.median(wall[pre])
        lines.append(dict(case="box", preconditioner=pre, leg="projection", iterations=its[pre],
                          ms_median=round(1e3 * med[pre], 2), ms_min=round(1e3 * min(wall[pre]), 2),
                          ms_per_iteration=round(1e3 * med[pre] / max(its[pre], 1), 4)))
    lines.append(dict(case="box", leg="fdm_over_none", time_ratio=round(med["fdm"] / med[None], 4),
                      iteration_ratio=round(its["fdm"] / max(its[None], 1), 4)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=22088)
    ap.add_argument("--tol", type=float, default=1e-12)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
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
