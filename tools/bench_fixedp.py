"""Time the fused fixed-point steps (nkv_sfd_step, nkv_tdf_step; csrc/fixedp.hip) at the BASELINE
layout, next to the same SFD step composed from the existing BLAS-1 entries in the reference's
order (fixedp.f90:157-189) and to nkv_axpby alone.

  python tools/bench_fixedp.py [--elements 44176] [--reps 5] [--rounds 5] [--lib path/to/libnekkrylov.so]

The legs alternate inside each round in ONE process (boxes differ by 1.5-3 %: only numbers of one
process compare); per leg the median and the minimum over the rounds are printed as one JSON line.
Bytes are the algorithmic streams over the stored rows N (8 bytes each), the weights on the
velocity rows included:
  sfd_step     6 reads + 4 writes of N, + n_vel n_v of w
  sfd_monitor  2 reads + 1 write of N, + n_vel n_v of w
  tdf_step     (3 reads + 2 writes + w) over the n_vel velocity fields, 1 read + 1 write per scalar
  sfd_composed the 20 sweeps of the reference: 8 copies (2 N), 5 cmults (2 N), 4 add2/sub2 (3 N),
               2 sub3 (3 N), one weighted dot (2 N_w + w per field)
  axpby        2 reads + 1 write of N
and GB/s is bytes over the event-timed call, against the 8 TB/s HBM3E peak.
"""
import argparse
import json
import os
import statistics
import sys

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

    from nekstab_next_amd import fixedp
    from nekstab_next_amd import synthetic as syn
    from nekstab_next_amd.layout import box3d_layout
    from nekstab_next_amd.vector import NekContext

    lay = box3d_layout(a.elements)
    ctx = NekContext(lay, weights=syn.mass_weights(lay), max_cols=2)
    n_vel, N, nv = lay.ldim, lay.rows, lay.sv
    w, ws, st = ctx.w.data_ptr(), ctx.ws.data_ptr(), ctx.stream
    v, v_old, qbar, qa, qb, qc, fc, tD, tM = (ctx.vector() for _ in range(9))
    for i, x in enumerate((v, v_old, qbar, qa, qb, qc, fc)):
        x.fill_hash(10 + i)
    ring = ctx.basis(2)
    r2 = torch.zeros(1, dtype=torch.float64, device=ctx.device)
    adt, bdt, cdt = fixedp.ab3_coefficients(3)
    cdtm, gain = 0.05, -0.5
    T = _lib.NKV_TIME

    def sfd_step():
        ctx.call("nkv_sfd_step", w, v.ptr, v_old.ptr, qbar.ptr, qa.ptr, qb.ptr, qc.ptr, fc.ptr, adt, bdt, cdt, cdtm, gain,
                 n_vel, r2.data_ptr(), ws, 0, st)

    def sfd_monitor():
        ctx.call("nkv_sfd_step", w, v.ptr, v_old.ptr, None, None, None, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, n_vel,
                 r2.data_ptr(), ws, _lib.NKV_SFD_MONITOR, st)

    def tdf_step():
        ctx.call("nkv_tdf_step", w, v.ptr, ring.col_ptr(0), fc.ptr, gain, n_vel, r2.data_ptr(), ws, 0, st)

    def copy(p, q):
        ctx.call("nkv_copy", p.ptr, q.ptr, T, st)

    def cmult(p, c):
        ctx.call("nkv_scal", p.ptr, c, T, st)

    def add2(p, q, s=1.0):
        ctx.call("nkv_axpby", p.ptr, 1.0, q.ptr, s, T, st)

    def sub3(p, q, r):
        ctx.call("nkv_sub3", p.ptr, q.ptr, r.ptr, T, st)

    def sfd_composed():   # fixedp.f90:158-189, sweep for sweep
        copy(qc, qb)
        copy(qb, qa)
        sub3(qa, v_old, qbar)
        copy(tD, qa)
        cmult(tD, adt)
        copy(tM, tD)
        copy(tD, qb)
        cmult(tD, bdt)
        add2(tM, tD)
        copy(tD, qc)
        cmult(tD, cdt)
        add2(tM, tD)
        cmult(tM, cdtm)
        add2(qbar, tM)
        sub3(tD, v_old, qbar)
        cmult(tD, gain)
        add2(fc, tD)
        add2(v_old, v, -1.0)                                                   # nopsub2
        ctx.call("nkv_dot", w, v_old.ptr, v_old.ptr, r2.data_ptr(), ws, 0, st)  # normvc (all weighted fields)
        copy(v_old, v)

    def axpby():
        ctx.call("nkv_axpby", tD.ptr, 1.0, tM.ptr, 0.5, 0, st)

    wb = n_vel * nv
    nw = lay.n_wf * nv
    legs = {
        "sfd_step": (sfd_step, 10 * N + wb),
        "sfd_monitor": (sfd_monitor, 3 * N + wb),
        "tdf_step": (tdf_step, 6 * n_vel * nv + 2 * (lay.n_wf - n_vel) * nv),
        "sfd_composed": (sfd_composed, (8 * 2 + 5 * 2 + 4 * 3 + 2 * 3) * N + 3 * nw),
        "axpby": (axpby, 3 * N),
    }
    times = {k: [] for k in legs}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn, _ in legs.values():   # warm every shape
        fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (fn, _) in legs.items():
            s.record()
            for _ in range(a.reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / a.reps)
    ctx.check_nan()
    info = dict(E=a.elements, rows=N, n_v=lay.n_v, reps=a.reps, rounds=a.rounds,
                device=torch.cuda.get_device_properties(ctx.device).gcnArchName.split(":")[0])
    print(json.dumps(info), flush=True)
    out = {}
    for name, (_, doubles) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        byts = 8 * doubles
        out[name] = dict(leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), GB=round(byts / 1e9, 3),
                         gbs_median=round(byts / (med * 1e-3) / 1e9, 1), frac_peak=round(byts / (med * 1e-3) / PEAK, 3))
        print(json.dumps(out[name]), flush=True)
    print(json.dumps(dict(composed_over_fused=round(out["sfd_composed"]["ms_median"] / out["sfd_step"]["ms_median"], 2),
                          fused_gbs_over_axpby=round(out["sfd_step"]["gbs_median"] / out["axpby"]["gbs_median"], 3),
                          tdf_gbs_over_axpby=round(out["tdf_step"]["gbs_median"] / out["axpby"]["gbs_median"], 3))),
          flush=True)


if __name__ == "__main__":
    main()
