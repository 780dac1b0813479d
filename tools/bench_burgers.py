"""Time the viscous Burgers entries (nkv_linconv_rhs, nkv_rk4_stage; csrc/advdiff.hip), one nonlinear step of
burgers.ViscousBurgers and one linearised step of burgers.LinearisedConvection, next to nkv_advdiff_rhs at the
same size (the byte floor: the new kernel reads n_wf more fields) and to the coupled right-hand side composed
from what predates it: nkv_gradm1 of the base state, torch pointwise operations and nkv_advdiff_rhs.

  python tools/bench_burgers.py [--elements 22088] [--reps 5] [--rounds 5] [--lib path/to/libnekkrylov.so]
                                [--out profiles/burgers_bench.json]

The case is bench_advdiff.py's box: 3-D, lx1=8, E=22,088 (11.3M points per field), vx vy vz t (n_wf = 4).
The legs alternate inside each round in ONE process (only numbers of one process compare); per leg the median
and the minimum over the rounds go out as one JSON line.  Bytes are the algorithmic streams per point, in
doubles: ldim + 3 n_wf for the coupled right-hand side (coordinates; B, u in; r out), 2 ldim + 2 n_wf for the
parent's (coordinates, U; u in; r out), 6 n_wf + 1 for a middle RK4 stage with forcing (v, r, g, acc in; w, acc
out; minv); GB/s against the 8 TB/s HBM3E peak.  The composed leg is held to the fused result first (max
difference over the result's scale is printed).
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
    from nekstab_next_amd.sensitivity import Gradm1
    from nekstab_next_amd.vector import NekContext

    lay, co, U = _mesh("box", a.elements)
    ctx = NekContext(lay, max_cols=4)
    n, sv, nf, d = lay.n_v, lay.sv, lay.n_wf, lay.ldim
    forcing = [0.3 * np.sin(co["x"] + 0.2 * f) * np.cos(co["y"]) for f in range(nf)]
    flow = ViscousBurgers(ctx, co, [0.01 * (1 + f) for f in range(nf)], 1e-4, 1, forcing=forcing)
    op = flow.lin.set_base(list(U) + [np.cos(co["x"]) * np.sin(0.5 * co["y"] + 0.3 * co["z"])])
    x, y = ctx.vector(), ctx.vector()
    x.fill_hash(3)
    op.project(x)
    f64 = dict(dtype=torch.float64, device=ctx.device)
    r = torch.zeros(nf * sv, **f64)
    st = ctx.stream
    xyz = op._xyz_ptrs()

    def rhs(entry, adjoint):
        ctx.call(entry, lay.lx1, d, op.D.data_ptr(), op.w.data_ptr(), *xyz, op.B.data_ptr(), sv, op.kappa.data_ptr(),
                 x.ptr, nf, sv, r.data_ptr(), sv, int(adjoint), st)

    def stage():
        ctx.call("nkv_rk4_stage", x.ptr, sv, op._minv.data_ptr(), r.data_ptr(), sv, flow._g.data_ptr(), sv, 0.5e-4,
                 0.33e-4, 0, flow._acc.data_ptr(), sv, op._w.data_ptr(), sv, flow._acc.data_ptr(), sv, nf, 0, st)

    def linear_step():   # the four Horner passes of one step of the linearised operator
        src = x.ptr
        for s in (4, 3, 2):
            op._local_rhs(src, False)
            op._stage(x.ptr, op._minv, op._r.data_ptr(), op.dt / s, op._w.data_ptr())
            src = op._w.data_ptr()
        op._local_rhs(src, False)
        op._stage(x.ptr, op._minv, op._r.data_ptr(), op.dt, y.ptr, zero_rest=True)

    def nonlinear_step():   # the four stages of one classical RK4 step (x is continuous: the projection is not in)
        dt, wp, ap = flow.dt, op._w.data_ptr(), flow._acc.data_ptr()
        flow._nonlinear_rhs(x.ptr)
        flow._rk4(x.ptr, dt / 2, dt / 6, True, wp, ap)
        flow._nonlinear_rhs(wp)
        flow._rk4(x.ptr, dt / 2, dt / 3, False, wp, ap)
        flow._nonlinear_rhs(wp)
        flow._rk4(x.ptr, dt, dt / 3, False, wp, ap)
        flow._nonlinear_rhs(wp)
        flow._rk4(None, 0.0, dt / 6, False, None, y.ptr, zero_rest=True)

    # the composition of what predates the fused entry: grad B by nkv_gradm1, the production term in torch,
    # the advection-diffusion part by nkv_advdiff_rhs
    grad_op = Gradm1.__new__(Gradm1)
    grad_op.ctx, grad_op.D, grad_op.xyz = ctx, op.D, op.xyz
    grad = torch.zeros(nf * d * n, **f64)
    rc = torch.zeros(nf * sv, **f64)
    uvel = [x.storage[c * sv: c * sv + n] for c in range(d)]

    def composed():
        grad_op(op.B.data_ptr(), grad.data_ptr(), nfld=nf, u_stride=sv, g_stride=n)
        ctx.call("nkv_advdiff_rhs", lay.lx1, d, op.D.data_ptr(), op.w.data_ptr(), *xyz, op.B.data_ptr(), sv,
                 op.kappa.data_ptr(), x.ptr, nf, sv, rc.data_ptr(), sv, 0, st)
        for f in range(nf):
            prod = uvel[0] * grad[(f * d) * n:(f * d + 1) * n]
            for c in range(1, d):
                prod = prod + uvel[c] * grad[(f * d + c) * n:(f * d + c + 1) * n]
            rc[f * sv: f * sv + n].sub_(op.bm1 * prod)

    legs = {
        f"advdiff_rhs_forward_{nf}": (lambda: rhs("nkv_advdiff_rhs", False), 2 * d + 2 * nf),
        f"advdiff_rhs_adjoint_{nf}": (lambda: rhs("nkv_advdiff_rhs", True), 2 * d + 2 * nf),
        f"linconv_rhs_forward_{nf}": (lambda: rhs("nkv_linconv_rhs", False), d + 3 * nf),
        f"linconv_rhs_adjoint_{nf}": (lambda: rhs("nkv_linconv_rhs", True), d + 3 * nf),
        f"composed_forward_{nf}": (composed, d + 3 * nf),
        "rk4_stage": (stage, 6 * nf + 1),
        "nonlinear_step": (nonlinear_step, 0),
        "linearised_step": (linear_step, 0),
    }
    for fn, _ in legs.values():   # warm every shape
        fn()
    torch.cuda.synchronize()
    rhs("nkv_linconv_rhs", False)
    composed()
    torch.cuda.synchronize()
    fused, comp = r.view(nf, sv)[:, :n], rc.view(nf, sv)[:, :n]
    dev = float(torch.max(torch.abs(fused - comp)).item()) / float(torch.max(torch.abs(fused)).item())
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
    lines = [dict(case="box", E=lay.nelv, lx1=lay.lx1, ldim=d, n_wf=nf, n_v=n, reps=a.reps, rounds=a.rounds,
                  composed_vs_fused_rel_max=dev,
                  device=torch.cuda.get_device_properties(ctx.device).gcnArchName.split(":")[0])]
    out = {}
    for name, (_, doubles) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        byts = 8 * doubles * n
        out[name] = dict(case="box", leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), GB=round(byts / 1e9, 4),
                         gbs_median=round(byts / (med * 1e-3) / 1e9, 1), frac_peak=round(byts / (med * 1e-3) / PEAK, 3))
        lines.append(out[name])
    ms = {k: v["ms_median"] for k, v in out.items()}
    lines.append(dict(case="box",
                      linconv_over_advdiff_forward=round(ms[f"linconv_rhs_forward_{nf}"] / ms[f"advdiff_rhs_forward_{nf}"], 2),
                      linconv_over_advdiff_adjoint=round(ms[f"linconv_rhs_adjoint_{nf}"] / ms[f"advdiff_rhs_adjoint_{nf}"], 2),
                      composed_over_fused=round(ms[f"composed_forward_{nf}"] / ms[f"linconv_rhs_forward_{nf}"], 2),
                      nonlinear_over_linearised_step=round(ms["nonlinear_step"] / ms["linearised_step"], 2)))
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
