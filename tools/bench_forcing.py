"""Time the body-force kernels (nkv_body_force, nkv_sponge_fn; csrc/forcing.hip) at the BASELINE layout,
each next to the same result composed from torch ops on the same tensors, and next to nkv_tdf_step (the
nearest existing kernel shape) and nkv_axpby from the same run.

  python tools/bench_forcing.py [--elements 44176] [--reps 5] [--rounds 5] [--lib path/to/libnekkrylov.so]

The legs alternate inside each round in ONE process (boxes differ by 1.5-3 %: only numbers of one process
compare); per leg the median and the minimum over the rounds are printed as one JSON line.  Bytes are the
algorithmic streams of n_v doubles (8 bytes each) of the kernel's header comment:
  force_dns    fc + harmonic + sponge on the userf zero: per velocity 5 reads + 1 write, per scalar 3 reads
               (fc, ref, t) + 1 write, fn once: (5 ldim + 1) reads and ldim writes on a flow without scalars
  force_pert   the perturbation sponge alone: per weighted field 1 read + 1 write, fn once
  sponge_fn    ldim coordinate reads (every dimension sponged) + 1 write
  *_torch      the same result from torch ops; timed, and rated with the bytes of the fused leg (the
               rate a user sees for the same work)
  tdf_step     (3 reads + 2 writes + w) over the velocity fields, 1 read + 1 write per scalar
  axpby        2 reads + 1 write of the stored rows
and GB/s is bytes over the event-timed call, against the 8 TB/s HBM3E peak.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nekstab_next_amd import _lib  # noqa: E402

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=44176)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    a = ap.parse_args()
    _lib.load(a.lib)
    _lib.require_gpu()

    from nekstab_next_amd import forcing
    from nekstab_next_amd import synthetic as syn
    from nekstab_next_amd.layout import box3d_layout
    from nekstab_next_amd.vector import NekContext

    lay = box3d_layout(a.elements)
    ctx = NekContext(lay, weights=syn.mass_weights(lay), max_cols=2)
    d, nwf, nv, sv, N = lay.ldim, lay.n_wf, lay.n_v, lay.sv, lay.rows
    st_ = ctx.stream
    # coordinates in [0, 1)^3 from the hash (a sponge needs only per-point values, not a mesh)
    rng = np.random.default_rng(3)
    coords = {k: rng.random(nv) for k in ("x", "y", "z")}
    cfg = forcing.SpongeConfig(xLspg=0.15, xRspg=0.3, yLspg=0.1, yRspg=0.1, zLspg=0.2, zRspg=0.2, spng_st=2.0)
    sp = forcing.Sponge(ctx, coords, cfg)
    v, fc, fre, fim, ref, ff, tD, tM = (ctx.vector() for _ in range(8))
    for i, x in enumerate((v, fc, fre, fim, ref, tD, tM)):
        x.fill_hash(10 + i)
    sp.set_reference(ref)
    bf = forcing.BodyForce(ctx, sp)
    omega = 0.9
    co, si, strength = math.cos(omega), math.sin(omega), cfg.spng_st
    ring = ctx.basis(1)
    r2 = torch.zeros(1, dtype=torch.float64, device=ctx.device)

    def force_dns():
        bf.assemble(ff, v, fc=fc, harmonic=(fre, fim, omega))

    def force_pert():
        bf.assemble(ff, v, perturbation=True)

    def sponge_fn():
        sp.compute()

    # ---- the same results from torch ops on the same tensors ----
    def rows(x, f0, f1):
        return x.storage[f0 * sv:f1 * sv].view(f1 - f0, sv)[:, :nv]

    fn = sp.fn[:nv]
    t1 = torch.empty((d, nv), dtype=torch.float64, device=ctx.device)
    t2 = torch.empty_like(t1)
    s1 = torch.empty((max(nwf - d, 1), nv), dtype=torch.float64, device=ctx.device)

    def force_dns_torch():
        out = rows(ff, 0, d)
        torch.mul(rows(fre, 0, d), co, out=t1)
        torch.add(rows(fc, 0, d), t1, out=t2)
        torch.mul(rows(fim, 0, d), si, out=t1)
        torch.sub(t2, t1, out=t2)
        torch.sub(rows(ref, 0, d), rows(v, 0, d), out=t1)
        torch.mul(t1, fn, out=t1)
        torch.mul(t1, strength, out=t1)
        torch.add(t2, t1, out=out)
        if nwf > d:
            outs = rows(ff, d, nwf)
            torch.sub(rows(ref, d, nwf), rows(v, d, nwf), out=s1)
            torch.mul(s1, fn, out=s1)
            torch.add(rows(fc, d, nwf), s1, out=outs)

    def force_pert_torch():
        out = rows(ff, 0, nwf)
        torch.mul(rows(v, 0, nwf), fn, out=out)
        torch.neg(out, out=out)

    def stepf(arg):
        e = torch.exp(1.0 / (arg - 1.0) + 1.0 / arg)
        one = torch.ones_like(arg)
        return torch.where(arg <= 0.001, torch.zeros_like(arg), torch.where(arg <= 0.999, 1.0 / (1.0 + e), one))

    fn_t = torch.empty(nv, dtype=torch.float64, device=ctx.device)

    def sponge_fn_torch():
        fn_t.zero_()
        for x, s in zip(sp.xyz, sp.sections):
            one, zero = torch.ones_like(x), torch.zeros_like(x)
            fall = stepf((s.xxmin - x) / s.wl)
            rise = stepf((x - s.xxmax) / s.wr)
            r = torch.where(x <= s.xxmin_c, one, torch.where(x < s.xxmin, fall, torch.where(
                x <= s.xxmax, zero, torch.where(x < s.xxmax_c, rise, one))))
            torch.maximum(fn_t, r, out=fn_t)

    def tdf_step():
        ctx.call("nkv_tdf_step", ctx.w.data_ptr(), v.ptr, ring.col_ptr(0), fc.ptr, -0.5, d, r2.data_ptr(),
                 ctx.ws.data_ptr(), 0, st_)

    def axpby():
        ctx.call("nkv_axpby", tD.ptr, 1.0, tM.ptr, 0.5, 0, st_)

    b_dns = (6 * d + 4 * (nwf - d) + 1) * nv
    b_pert = (2 * nwf + 1) * nv
    b_spg = (d + 1) * nv
    legs = {
        "force_dns": (force_dns, b_dns),
        "force_dns_torch": (force_dns_torch, b_dns),
        "force_pert": (force_pert, b_pert),
        "force_pert_torch": (force_pert_torch, b_pert),
        "sponge_fn": (sponge_fn, b_spg),
        "sponge_fn_torch": (sponge_fn_torch, b_spg),
        "tdf_step": (tdf_step, 6 * d * nv + 2 * (nwf - d) * nv),
        "axpby": (axpby, 3 * N),
    }
    times = {k: [] for k in legs}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn_, _ in legs.values():   # warm every shape
        fn_()
    torch.cuda.synchronize()
    # the composed legs give the fused results (to rounding: torch may contract, the kernel does not)
    force_dns()
    want = ff.storage.clone()
    force_dns_torch()
    live = torch.zeros(lay.ld, dtype=torch.bool, device=ctx.device)
    for f in range(nwf):
        live[f * sv:f * sv + nv] = True
    scale = float(want[live].abs().max())
    dns_diff = float((ff.storage[live] - want[live]).abs().max()) / scale
    sponge_fn()
    sponge_fn_torch()
    fn_diff = float((fn_t - sp.fn[:nv]).abs().max())
    for _ in range(a.rounds):
        for name, (fn_, _) in legs.items():
            s.record()
            for _ in range(a.reps):
                fn_()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / a.reps)
    ctx.check_nan()
    info = dict(E=a.elements, rows=N, n_v=nv, n_wf=nwf, reps=a.reps, rounds=a.rounds,
                sponge_points=int(torch.count_nonzero(sp.fn).item()), composed_dns_rel_diff=dns_diff,
                composed_fn_abs_diff=fn_diff,
                device=torch.cuda.get_device_properties(ctx.device).gcnArchName.split(":")[0])
    print(json.dumps(info), flush=True)
    out = {}
    for name, (_, doubles) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        byts = 8 * doubles
        out[name] = dict(leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), GB=round(byts / 1e9, 3),
                         gbs_median=round(byts / (med * 1e-3) / 1e9, 1), frac_peak=round(byts / (med * 1e-3) / PEAK, 3))
        print(json.dumps(out[name]), flush=True)
    ratio = lambda p, q: round(out[p]["ms_median"] / out[q]["ms_median"], 2)   # noqa: E731
    print(json.dumps(dict(dns_composed_over_fused=ratio("force_dns_torch", "force_dns"),
                          pert_composed_over_fused=ratio("force_pert_torch", "force_pert"),
                          sponge_composed_over_fused=ratio("sponge_fn_torch", "sponge_fn"),
                          dns_gbs_over_tdf=round(out["force_dns"]["gbs_median"] / out["tdf_step"]["gbs_median"], 3),
                          pert_gbs_over_tdf=round(out["force_pert"]["gbs_median"] / out["tdf_step"]["gbs_median"], 3),
                          dns_gbs_over_axpby=round(out["force_dns"]["gbs_median"] / out["axpby"]["gbs_median"], 3))),
          flush=True)


if __name__ == "__main__":
    main()
