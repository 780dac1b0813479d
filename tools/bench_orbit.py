"""Time the orbit entries (nkv_burgers_tangent_rhs, nkv_orbit_stage; csrc/advdiff.hip): the fused right-hand side
next to the two launches it replaces (nkv_advdiff_rhs with u = U = B, then the forward nkv_linconv_rhs), and one
side-by-side step of orbit.OrbitPropagator (store=False: the base and the perturbation advance together) next to
one step about a stored orbit (the tangent alone) and to the base step that fills the orbit.

  python tools/bench_orbit.py [--elements 22088] [--reps 5] [--rounds 5] [--lib path/to/libnekkrylov.so]
                              [--out profiles/orbit_bench.json]

The case, the process and the shape are bench_burgers.py's: the box of bench_advdiff.py, 3-D, lx1=8, E=22,088
(11.3M points per field), vx vy vz t (n_wf = 4).  The legs alternate inside each round in ONE process (only
numbers of one process compare); per leg the median and the minimum over the rounds go out as one JSON line.
Bytes are the algorithmic streams per point, in doubles: 2 ldim + 2 n_wf for nkv_advdiff_rhs (coordinates, U; u
in; r out), ldim + 3 n_wf for nkv_linconv_rhs (coordinates; B, u in; r out), ldim + 4 n_wf for the fused pass
(coordinates; B, u in; r_B, r_u out): 14 + 15 = 29 against 19; GB/s against the 8 TB/s HBM3E peak.  The fused
results are compared with the pair's bit for bit first, and the side-by-side step with the stored one.
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
    part = lambda amp, ph: [amp * np.sin(co["x"] + 0.2 * f + ph) * np.cos(co["y"]) for f in range(nf)]   # noqa: E731
    flow = ViscousBurgers(ctx, co, [0.01 * (1 + f) for f in range(nf)], 1e-4, 1, forcing=part(0.3, 0.0))
    of = OrbitFlow(flow, cos=part(0.2, 0.5), sin=part(0.1, 1.0))
    sbs = OrbitFlow(flow, cos=part(0.2, 0.5), sin=part(0.1, 1.0), store=False)
    op = flow.lin
    q, x, y, y2 = ctx.vector(), ctx.vector(), ctx.vector(), ctx.vector()
    q.zero()                    # the base state of bench_burgers.py: the box flow and a smooth scalar
    for f, b in enumerate(list(U) + [np.cos(co["x"]) * np.sin(0.5 * co["y"] + 0.3 * co["z"])]):
        q.storage[f * sv: f * sv + n] = torch.as_tensor(np.ascontiguousarray(b, dtype=np.float64)).to(ctx.device)
    x.fill_hash(3)
    op.project(x)
    f64 = dict(dtype=torch.float64, device=ctx.device)
    rB, ru, fB, fu = (torch.zeros(nf * sv, **f64) for _ in range(4))
    st = ctx.stream
    xyz = op._xyz_ptrs()
    head = (lay.lx1, d, op.D.data_ptr(), op.w.data_ptr(), *xyz, q.ptr, sv, op.kappa.data_ptr())

    def self_advection():
        ctx.call("nkv_advdiff_rhs", *head, q.ptr, nf, sv, rB.data_ptr(), sv, 0, st)

    def linconv():
        ctx.call("nkv_linconv_rhs", *head, x.ptr, nf, sv, ru.data_ptr(), sv, 0, st)

    def pair():
        self_advection()
        linconv()

    def fused():
        ctx.call("nkv_burgers_tangent_rhs", *head, x.ptr, nf, sv, fB.data_ptr(), sv, fu.data_ptr(), sv, st)

    of.propagate(q, y)          # the stored orbit of one step (nsteps = 1)
    stored, side = of.linearized(q), sbs.linearized(q)
    legs = {
        f"advdiff_rhs_self_{nf}": (self_advection, 2 * d + 2 * nf),
        f"linconv_rhs_forward_{nf}": (linconv, d + 3 * nf),
        f"pair_{nf}": (pair, 3 * d + 5 * nf),
        f"fused_{nf}": (fused, d + 4 * nf),
        "base_step": (lambda: of.propagate(q, y), 0),
        "stored_tangent_step": (lambda: stored.matvec(x, y), 0),
        "side_by_side_step": (lambda: side.matvec(x, y2), 0),
    }
    for fn, _ in legs.values():   # warm every shape
        fn()
    torch.cuda.synchronize()
    bits = dict(r_B=bool(torch.equal(rB.view(nf, sv)[:, :n], fB.view(nf, sv)[:, :n])),
                r_u=bool(torch.equal(ru.view(nf, sv)[:, :n], fu.view(nf, sv)[:, :n])),
                step=bool(torch.equal(y.storage, y2.storage)))
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
    lines = [dict(case="box", E=lay.nelv, lx1=lay.lx1, ldim=d, n_wf=nf, n_v=n, sv=sv, reps=a.reps, rounds=a.rounds,
                  same_bits=bits, orbit_bytes_per_step=of.orbit_bytes // of.nsteps,
                  device=torch.cuda.get_device_properties(ctx.device).gcnArchName.split(":")[0])]
    out = {}
    for name, (_, doubles) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        byts = 8 * doubles * n
        out[name] = dict(case="box", leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), GB=round(byts / 1e9, 4),
                         gbs_median=round(byts / (med * 1e-3) / 1e9, 1), frac_peak=round(byts / (med * 1e-3) / PEAK, 3))
        lines.append(out[name])
    ms = {k: v["ms_median"] for k, v in out.items()}
    lines.append(dict(case="box", fused_over_pair=round(ms[f"fused_{nf}"] / ms[f"pair_{nf}"], 3),
                      byte_model=round((d + 4 * nf) / (3 * d + 5 * nf), 3),
                      side_by_side_over_base_plus_stored=round(ms["side_by_side_step"] /
                                                               (ms["base_step"] + ms["stored_tangent_step"]), 3),
                      side_by_side_over_stored=round(ms["side_by_side_step"] / ms["stored_tangent_step"], 3)))
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
