"""Time one pair projection (pressure.DivergenceFreeProjector.project_pair_ptr: the two-system CG over
nkv_pressure_div2 / _gradt2 / _cg_update2; csrc/pressure.hip) next to the two project_ptr solves it replaces, and one
Horner pass of resolvent.IncompressibleResolventOperator with batched=True next to the same pass with batched=False.

  python tools/bench_incompressible_resolvent.py [--elements 22088] [--tol 1e-12] [--reps 1] [--rounds 3]
                                                 [--lib path/to/libnekkrylov.so]
                                                 [--out profiles/incompressible_resolvent_bench.json]

The case and the shape are bench_incompressible.py's: the box of bench_advdiff.py, 3-D, lx1=8, E=22,088 (11.3M GLL
points per half and field, 4.77M pressure values per system), no mask (an open domain), vx vy vz t (n_wf = 4), the
base state of bench_coupled_resolvent.py, omega = 1.  The two halves projected are hashed continuous fields of
different seeds.  The legs alternate inside each round in ONE process (only numbers of one process compare); per leg
the median and the minimum over the rounds go out as one JSON line, then the iteration counts and the ratios
batched / sequential.  The results of the two paths are compared bit for bit first.  A projection at this size is
thousands of CG iterations: one repetition per round is seconds.
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


def bench(a):
    import numpy as np

    from bench_advdiff import _mesh
    from nekstab_next_amd.incompressible import LinearisedNavierStokes
    from nekstab_next_amd.resolvent import IncompressibleResolventOperator, pair_context
    from nekstab_next_amd.vector import NekContext

    lay, co, U = _mesh("box", a.elements)
    n, nf, d = lay.n_v, lay.n_wf, lay.ldim
    base = list(U) + [np.cos(co["x"]) * np.sin(0.5 * co["y"] + 0.3 * co["z"])]
    lns = LinearisedNavierStokes(NekContext(lay, max_cols=4), co, base, [0.01 * (1 + f) for f in range(nf)], 1e-4, 1,
                                 tol=a.tol, maxiter=a.maxiter, closed=False)
    pctx = pair_context(lns, max_cols=4)
    ops = {True: IncompressibleResolventOperator(pctx, lns, 1.0, kdim=4, batched=True),
           False: IncompressibleResolventOperator(pctx, lns, 1.0, kdim=4, batched=False)}
    x, f, w = (pctx.vector() for _ in range(3))
    x.fill_hash(3)
    ops[True].project(x)
    f.fill_hash(5)
    ops[True].project(f)
    outs = {True: pctx.vector(), False: pctx.vector()}
    its = {}

    def projection(batched):
        w.copy_from(x0)
        ops[batched]._project_velocity(w.ptr, w.storage)

    def horner(batched):
        op = ops[batched]
        op._pass(x.ptr, x.ptr, f.ptr, op.omega, op.dt / 4, outs[batched].ptr, False)

    x0 = pctx.vector()
    x0.fill_hash(7)                                                   # unprojected: two full solves
    super(IncompressibleResolventOperator, ops[True]).project(x0)     # continuous and masked, not divergence-free
    bits = {}
    res = {}
    for batched in (True, False):                                     # (also warms every shape)
        projection(batched)
        torch.cuda.synchronize()
        res[batched] = w.storage.clone()
        its[batched] = (lns.projector.last_iterations_each if batched else None, lns.projector.last_iterations)
        horner(batched)
    torch.cuda.synchronize()
    bits["projection"] = bool(torch.equal(res[True], res[False]))
    bits["horner_pass"] = bool(torch.equal(outs[True].storage, outs[False].storage))
    legs = {"pair_projection_batched": lambda: projection(True), "pair_projection_sequential": lambda: projection(False),
            "horner_pass_batched": lambda: horner(True), "horner_pass_sequential": lambda: horner(False)}
    times = {k: [] for k in legs}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, fn in legs.items():
            s.record()
            for _ in range(a.reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / a.reps)
    lines = [dict(case="box", E=lay.nelv, lx1=lay.lx1, ldim=d, n_wf=nf, n_v=n, npz=lns.projector.npz, tol=a.tol, reps=a.reps,
                  rounds=a.rounds, same_bits=bits, cg_iterations_each=its[True][0], cg_iterations_last_sequential=its[False][1],
                  lib=os.path.basename(a.lib),
                  device=torch.cuda.get_device_properties(pctx.device).gcnArchName.split(":")[0])]
    ms = {}
    for name in legs:
        ms[name] = statistics.median(times[name])
        lines.append(dict(case="box", leg=name, ms_median=round(ms[name], 3), ms_min=round(min(times[name]), 3)))
    lines.append(dict(case="box",
                      projection_batched_over_sequential=round(ms["pair_projection_batched"] / ms["pair_projection_sequential"], 3),
                      pass_batched_over_sequential=round(ms["horner_pass_batched"] / ms["horner_pass_sequential"], 3)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=22088)
    ap.add_argument("--tol", type=float, default=1e-12)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=1)
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
