"""Time the energy-budget entries (nkv_pke_production, nkv_divm1, nkv_pke_dissipation;
csrc/postproc.hip) and the whole per-mode chain at config 5's mesh (3-D, lx1=8, E=22,088: 11.3M points
per field), next to the same production result composed from entries that predate them: three
nkv_gradm1, the pointwise products in torch and nine nkv_dot.

  python tools/bench_energy_budget.py [--elements 22088] [--reps 5] [--rounds 5] [--no-average]
                                      [--lib path/to/libnekkrylov.so]

The legs alternate inside each round in ONE process (boxes differ by 1.5-3 %: only numbers of one
process compare); per leg the median and the minimum over the rounds are printed as one JSON line.
Bytes are the algorithmic streams in doubles per point n_v (8 bytes each), 3-D:
  production         13 read (x, y, z, 3 base, 3 re, 3 im, bm1) + 9 written                      = 22
  production_nofld   13 read, integrals only (prod = NULL)                                       = 13
  composed           3 gradm1 (4 read + 3 written each) = 21; the products as single passes
                     (6 mode + 9 gradients read, 9 written) = 24; 9 dots (bm1, P, ones) = 27     = 72
                     (torch runs the products as 36 elementwise kernels: what a caller without the
                     fused entry writes; the byte model counts them as the single passes they could be)
  divm1              3 coordinates + 18 first derivatives read, 6 Laplacians written             = 27
  dissipation        6 mode + 6 Laplacians + bm1 read, 1 written                                 = 14
  chain              energy_budget_fields: production 22 + 2 gradm1 of 3 fields (3 + 3 + 9 = 15 each)
                     + divm1 27 + dissipation 14 = 93, plus dsavg of 18 + 6 segments over the shared
                     points only (not counted; --no-average leaves dsavg out)
and GB/s is bytes over the event-timed call, against the 8 TB/s HBM3E peak.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from nekstab_next_amd import _lib  # noqa: E402

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=22088)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-average", action="store_true")
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    a = ap.parse_args()
    _lib.load(a.lib)
    _lib.require_gpu()
    from seed_helpers import box_mesh_coords

    from nekstab_next_amd import synthetic as syn
    from nekstab_next_amd.layout import NekLayout, _roundup
    from nekstab_next_amd.postproc import energy_budget_fields
    from nekstab_next_amd.seeds import FaceAverage
    from nekstab_next_amd.sensitivity import Gradm1, velocity_layout
    from nekstab_next_amd.vector import NekContext

    lx1, d, nel = 8, 3, a.elements
    nz = -(-nel // 484)
    full = NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=22 * 22 * nz)
    box = box_mesh_coords(full, (22, 22, nz), L=(1.0, 1.0, 2.0))
    co = {k: box[k][: nel * lx1 ** 3] for k in ("x", "y", "z")}
    del box
    lay = velocity_layout(NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=nel))
    ctx = NekContext(lay, weights=syn.mass_weights(lay), max_cols=4)
    sv, n = lay.sv, lay.n_v
    op = Gradm1(ctx, co)
    avg = None if a.no_average else FaceAverage(ctx, co).apply
    base, re, im = (ctx.vector() for _ in range(3))
    for i, v in enumerate((base, re, im)):
        v.fill_hash(20 + i)
    f64 = dict(dtype=torch.float64, device=ctx.device)
    w, ws, st = ctx.w.data_ptr(), ctx.ws.data_ptr(), ctx.stream
    D, (xm, ym, zm) = op.D.data_ptr(), [t.data_ptr() for t in op.xyz]
    prod = torch.zeros(9 * sv, **f64)
    grads = torch.zeros(18 * sv, **f64)
    lap = torch.zeros(6 * sv, **f64)
    diss = torch.zeros(sv, **f64)
    integ = torch.zeros(16, **f64)

    def production():
        ctx.call("nkv_pke_production", lx1, d, D, xm, ym, zm, base.ptr, sv, re.ptr, im.ptr, sv, w, prod.data_ptr(), sv,
                 integ.data_ptr(), ws, st)

    def production_nofld():
        ctx.call("nkv_pke_production", lx1, d, D, xm, ym, zm, base.ptr, sv, re.ptr, im.ptr, sv, w, None, sv,
                 integ.data_ptr(), ws, st)

    # the composed leg: entries that predate postproc.hip
    L1 = lay.c_struct()
    L1.n_wf, L1.n_p, L1.sp, L1.ld = 1, 0, 0, _roundup(sv + 1, 4096)
    ones = torch.zeros(L1.ld, **f64)
    ones[:n] = 1.0
    G = torch.zeros(9 * sv, **f64)
    P = torch.zeros(9 * sv + 4096, **f64)   # + the time slot the last one-field dot may address
    Gv, Pv = G.view(3, 3, sv), P[: 9 * sv].view(3, 3, sv)
    R, I = re.storage[: 3 * sv].view(3, sv), im.storage[: 3 * sv].view(3, sv)
    integ2 = torch.zeros(9, **f64)

    def composed():
        for c in range(3):
            op(base.ptr + 8 * c * sv, G.data_ptr() + 8 * 3 * c * sv, nfld=1, g_stride=sv)
        for c in range(3):
            for k in range(3):
                m2 = R[c] * R[c] + I[c] * I[c] if c == k else R[c] * R[k] + I[k] * I[c]
                torch.mul(-0.5 * m2, Gv[c, k], out=Pv[c, k])
        for q in range(9):
            _lib.check(ctx.lib.nkv_dot(ctypes.byref(L1), w, P.data_ptr() + 8 * q * sv, ones.data_ptr(),
                                       integ2.data_ptr() + 8 * q, ws, 0, st), "nkv_dot")

    def divm1():
        ctx.call("nkv_divm1", lx1, d, D, xm, ym, zm, grads.data_ptr(), 6, sv, lap.data_ptr(), sv, st)

    def dissipation():
        ctx.call("nkv_pke_dissipation", re.ptr, im.ptr, sv, lap.data_ptr(), sv, d, 0.02, w, diss.data_ptr(),
                 integ.data_ptr() + 8 * 12, ws, st)

    def chain():
        energy_budget_fields(ctx, base, re, im, op, avg, 0.02)

    legs = {
        "production": (production, 22),
        "production_nofld": (production_nofld, 13),
        "composed": (composed, 72),
        "divm1": (divm1, 27),
        "dissipation": (dissipation, 14),
        "chain": (chain, 93),
    }
    for fn, _ in legs.values():   # warm every shape
        fn()
    torch.cuda.synchronize()
    # the two production results agree (the composed one is not in the reference's operand order)
    production()
    torch.cuda.synchronize()
    dev = float(torch.max(torch.abs(prod.view(9, sv)[:, :n] - P[: 9 * sv].view(9, sv)[:, :n])).item())
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
    ctx.check_nan()
    info = dict(E=nel, lx1=lx1, n_v=n, reps=a.reps, rounds=a.rounds, dsavg=not a.no_average,
                fused_vs_composed_max_abs=dev,
                device=torch.cuda.get_device_properties(ctx.device).gcnArchName.split(":")[0])
    print(json.dumps(info), flush=True)
    out = {}
    for name, (_, doubles) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        byts = 8 * doubles * n
        out[name] = dict(leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), GB=round(byts / 1e9, 3),
                         gbs_median=round(byts / (med * 1e-3) / 1e9, 1), frac_peak=round(byts / (med * 1e-3) / PEAK, 3))
        print(json.dumps(out[name]), flush=True)
    print(json.dumps(dict(composed_over_fused=round(out["composed"]["ms_median"] / out["production"]["ms_median"], 2))),
          flush=True)


if __name__ == "__main__":
    main()
