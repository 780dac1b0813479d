"""Time the fused pair right-hand side of the coupled resolvent (nkv_linconv_crhs; csrc/advdiff.hip) next to the two
nkv_linconv_rhs launches it replaces, forward and adjoint, and one forced RK4 step of
resolvent.CoupledResolventOperator next to the same step with the two-launch right-hand side.

  python tools/bench_coupled_resolvent.py [--elements 22088] [--reps 5] [--rounds 5] [--lib path/to/libnekkrylov.so]
                                          [--out profiles/coupled_resolvent_bench.json]

The case, the process and the shape are bench_burgers.py's: the box of bench_advdiff.py, 3-D, lx1=8, E=22,088
(11.3M points per half and field), vx vy vz t (n_wf = 4), the box flow and a smooth scalar as base state, omega = 1.
The legs alternate inside each round in ONE process (only numbers of one process compare); per leg the median and
the minimum over the rounds go out as one JSON line.  Bytes are the algorithmic streams per point, in doubles:
ldim + 3 n_wf for one nkv_linconv_rhs (coordinates; B, u in; r out), so 2 ldim + 6 n_wf = 30 for the two launches,
and ldim + 5 n_wf = 23 for the fused pass (coordinates and B once; u_re, u_im in; r_re, r_im out); GB/s against the
8 TB/s HBM3E peak.  The fused results are compared with the pair's bit for bit first, and so are the two steps.
--lib times another build of the library, e.g. one compiled with -DNKV_CRHS_WAVES=0 (no waves-per-SIMD request in
the launch bounds of k_linconv_crhs).
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
    from nekstab_next_amd.burgers import LinearisedConvection
    from nekstab_next_amd.gs import average_segments
    from nekstab_next_amd.resolvent import CoupledResolventOperator, pair_context
    from nekstab_next_amd.vector import NekContext

    lay, co, U = _mesh("box", a.elements)
    n, nf, d = lay.n_v, lay.n_wf, lay.ldim
    base = list(U) + [np.cos(co["x"]) * np.sin(0.5 * co["y"] + 0.3 * co["z"])]   # the base state of bench_burgers.py
    lin = LinearisedConvection(NekContext(lay, max_cols=4), co, base, [0.01 * (1 + f) for f in range(nf)], 1e-4, 1)
    pctx = pair_context(lin, max_cols=4)
    op = CoupledResolventOperator(pctx, lin, 1.0, kdim=4)
    psv, st, call = pctx.layout.sv, pctx.stream, lin.ctx.call
    x, f, y, y2 = (pctx.vector() for _ in range(4))
    x.fill_hash(3)
    op.project(x)
    f.fill_hash(5)
    op.project(f)
    r1, r2 = torch.zeros_like(op._r), torch.zeros_like(op._r)
    head = op._crhs_head

    def two(src, dst, adjoint):
        for h in (0, 8 * n):
            call("nkv_linconv_rhs", *head, src + h, nf, psv, dst + h, psv, int(adjoint), st)

    def fused(src, dst, adjoint):
        call("nkv_linconv_crhs", *head, src, src + 8 * n, nf, psv, dst, dst + 8 * n, psv, int(adjoint), st)

    def local_two(src, adjoint, stream):
        """CoupledResolventOperator._local_rhs with the two launches."""
        two(src, op._r.data_ptr(), adjoint)
        average_segments(lin.face_average, op._avg_ptrs)

    def step(local_rhs, out):
        """One forced RK4 step from x into ``out``: the four Horner passes of ResolventOperator._steps."""
        out.copy_from(x)
        src, rp = out.ptr, op._r.data_ptr()
        for s, w in ((4, op._wa), (3, op._wb), (2, op._wa)):
            local_rhs(src, False, st)
            op._cstage(out.ptr, lin._minv, rp, src, f.ptr, op.omega, op.dt / s, w.data_ptr(), st)
            src = w.data_ptr()
        local_rhs(src, False, st)
        op._cstage(out.ptr, lin._minv, rp, src, f.ptr, op.omega, op.dt, out.ptr, st, zero_rest=True)

    legs = {}
    for adjoint, tag in ((False, "forward"), (True, "adjoint")):
        legs[f"two_linconv_rhs_{tag}"] = (lambda adjoint=adjoint: two(x.ptr, r2.data_ptr(), adjoint), 2 * d + 6 * nf)
        legs[f"linconv_crhs_{tag}"] = (lambda adjoint=adjoint: fused(x.ptr, r1.data_ptr(), adjoint), d + 5 * nf)
    legs["step_two_launches"] = (lambda: step(local_two, y2), 0)
    legs["step_fused"] = (lambda: step(op._local_rhs, y), 0)
    bits = {}
    live = slice(0, nf * psv)
    for adjoint, tag in ((False, "forward"), (True, "adjoint")):   # (also warms every shape)
        two(x.ptr, r2.data_ptr(), adjoint)
        fused(x.ptr, r1.data_ptr(), adjoint)
        torch.cuda.synchronize()
        bits[tag] = bool(torch.equal(r1[live], r2[live])) and bool(torch.any(r1[live] != 0))
    step(local_two, y2)
    step(op._local_rhs, y)
    torch.cuda.synchronize()
    bits["step"] = bool(torch.equal(y.storage, y2.storage))
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
    lines = [dict(case="box", E=lay.nelv, lx1=lay.lx1, ldim=d, n_wf=nf, n_v=n, pair_sv=psv, omega=op.omega, reps=a.reps,
                  rounds=a.rounds, same_bits=bits, lib=os.path.basename(a.lib),
                  device=torch.cuda.get_device_properties(pctx.device).gcnArchName.split(":")[0])]
    out = {}
    for name, (_, doubles) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        byts = 8 * doubles * n
        out[name] = dict(case="box", leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), GB=round(byts / 1e9, 4),
                         gbs_median=round(byts / (med * 1e-3) / 1e9, 1), frac_peak=round(byts / (med * 1e-3) / PEAK, 3))
        lines.append(out[name])
    ms = {k: v["ms_median"] for k, v in out.items()}
    lines.append(dict(case="box", byte_model=round((d + 5 * nf) / (2 * d + 6 * nf), 3),
                      fused_over_two_forward=round(ms["linconv_crhs_forward"] / ms["two_linconv_rhs_forward"], 3),
                      fused_over_two_adjoint=round(ms["linconv_crhs_adjoint"] / ms["two_linconv_rhs_adjoint"], 3),
                      step_fused_over_two=round(ms["step_fused"] / ms["step_two_launches"], 3)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=22088)
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
