"""Time the batched direct-stiffness average (gs.GatherScatter.apply_many: nkv_gs_average; csrc/gs.hip)
over 1, 3, 9 and 24 field segments next to the same number of seeds.FaceAverage.apply calls
(nkv_group_average, one launch per segment), on a one-rank box at config 5's mesh (3-D, lx1=8, E=22,088:
11.3M points per segment), in the same process.

  python tools/bench_gs.py [--elements 22088] [--reps 5] [--rounds 5] [--lib path/to/libnekkrylov.so]

The legs alternate inside each round in ONE process (boxes differ by 1.5-3 %: only numbers of one process
compare); per leg the median and the minimum over the rounds are printed as one JSON line.  Bytes are the
algorithmic ones for G groups holding M entries in all (every shared point is an entry):
  separate   per segment: 8 M index bytes + 16 G offset bytes + 8 M read + 8 M written
  fused      once: 4 M index bytes + 8 G offset bytes; per segment: 8 M read + 8 M written
The values are gathered 8 bytes at a time from lines the other groups of the neighbourhood share, so the
traffic the memory system sees is a multiple of this; GB/s is the algorithmic bytes over the event-timed
call.  At world 1 there is no pack and no exchange: this is the average kernel alone.
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

from nekstab_next_amd import _lib  # noqa: E402

NF = (1, 3, 9, 24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=22088)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    a = ap.parse_args()
    _lib.load(a.lib)
    _lib.require_gpu()
    from seed_helpers import box_mesh_coords

    from nekstab_next_amd.gs import GatherScatter
    from nekstab_next_amd.layout import NekLayout
    from nekstab_next_amd.seeds import FaceAverage
    from nekstab_next_amd.sensitivity import velocity_layout
    from nekstab_next_amd.vector import NekContext

    lx1, nel = 8, a.elements
    nz = -(-nel // 484)
    full = NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=22 * 22 * nz)
    box = box_mesh_coords(full, (22, 22, nz), L=(1.0, 1.0, 2.0))
    co = {k: box[k][: nel * lx1 ** 3] for k in ("x", "y", "z")}
    del box
    lay = velocity_layout(NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=nel))
    ctx = NekContext(lay, max_cols=4)
    n = lay.n_v
    fa, gs = FaceAverage(ctx, co), GatherScatter(ctx, co)
    G, M = gs.n_groups, int(gs.plan.start[-1])
    assert G == fa.n_groups
    f64 = dict(dtype=torch.float64, device=ctx.device)
    base = torch.rand(max(NF) * n, **f64)
    work = torch.empty_like(base)
    ptrs = [work.data_ptr() + 8 * f * n for f in range(max(NF))]

    # the two paths give the same bits
    work.copy_(base)
    gs.apply_many(ptrs)
    fused = work.clone()
    work.copy_(base)
    for p in ptrs:
        fa.apply(p)
    same = bool(torch.equal(fused, work))
    del fused

    def separate(nf):
        for p in ptrs[:nf]:
            fa.apply(p)

    legs = {}
    for nf in NF:
        legs[f"fused_{nf}"] = (lambda nf=nf: gs.apply_many(ptrs[:nf]), 4 * M + 8 * G + nf * 16 * M)
        legs[f"separate_{nf}"] = (lambda nf=nf: separate(nf), nf * (8 * M + 16 * G + 16 * M))
    for fn, _ in legs.values():   # warm every shape
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
    info = dict(E=nel, lx1=lx1, n_v=n, groups=G, entries=M, candidates=gs.n_candidates, reps=a.reps, rounds=a.rounds,
                fused_equals_separate=same,
                device=torch.cuda.get_device_properties(ctx.device).gcnArchName.split(":")[0])
    print(json.dumps(info), flush=True)
    out = {}
    for name, (_, byts) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        out[name] = dict(leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), MB=round(byts / 1e6, 1),
                         gbs_median=round(byts / (med * 1e-3) / 1e9, 1))
        print(json.dumps(out[name]), flush=True)
    print(json.dumps({f"separate_over_fused_{nf}": round(out[f"separate_{nf}"]["ms_median"]
                                                         / out[f"fused_{nf}"]["ms_median"], 2) for nf in NF}), flush=True)


if __name__ == "__main__":
    main()
