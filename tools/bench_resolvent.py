"""Time the fused complex Horner stage (nkv_advdiff_cstage; csrc/advdiff.hip) and one forced RK4 step of
resolvent.ResolventOperator, next to the same stage composed from what predates it: nkv_advdiff_stage on the
re and on the im halves plus torch pointwise operations for the -i omega coupling and the forcing.

  python tools/bench_resolvent.py [--elements 22088] [--reps 5] [--rounds 5] [--lib path/to/libnekkrylov.so]
                                  [--out profiles/resolvent_bench.json]

3-D, lx1=8, E=22,088 (the size of tools/bench_advdiff.py: 11.3M points per half and field), vx vy vz t
(n_wf = 4), omega = 1.  The legs alternate inside each round in ONE process (only numbers of one process
compare); per leg the median and the minimum over the rounds go out as one JSON line.  Bytes of a stage are
the algorithmic streams: 8 n_v n_wf 11 (v, r, s, f in both halves and minv read, w written in both halves);
GB/s against the 8 TB/s HBM3E peak.  A step adds four right-hand sides per half and the averages, the same
in both legs, so its bytes are not modelled.  The composed stage is held to the fused result first (it rounds
in another order: the largest difference over the largest value is printed).
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


class ComposedStage:
    """w = v + c (minv r - i omega s + f) from nkv_advdiff_stage per half and four torch passes."""

    def __init__(self, op):
        self.op = op
        lay = op.ctx.layout
        self.n, self.psv, self.nf = lay.n_v // 2, lay.sv, lay.n_wf

    def _rows(self, t):
        """(re, im) views (n_wf, n) of a tensor laid out as the field segments of a pair vector."""
        seg = t[: self.nf * self.psv].view(self.nf, self.psv)
        return seg[:, : self.n], seg[:, self.n: 2 * self.n]

    def __call__(self, v, r, s, f, omega, c, w):
        """v, r, s, f, w: tensors (v may be w; f may be None)."""
        op, n, psv = self.op, self.n, self.psv
        actx = op.adv.ctx
        for h in (0, 8 * n):
            actx.call("nkv_advdiff_stage", v.data_ptr() + h, psv, op.adv._minv.data_ptr(), r.data_ptr() + h, psv, float(c),
                      w.data_ptr() + h, psv, self.nf, 0, actx.stream)
        w_re, w_im = self._rows(w)
        s_re, s_im = self._rows(s)
        w_re.add_(s_im, alpha=c * omega)
        w_im.add_(s_re, alpha=-c * omega)
        if f is not None:
            f_re, f_im = self._rows(f)
            w_re.add_(f_re, alpha=c)
            w_im.add_(f_im, alpha=c)


def bench(a):
    from bench_advdiff import _mesh
    from nekstab_next_amd.advdiff import AdvectionDiffusion
    from nekstab_next_amd.resolvent import ResolventOperator, pair_context
    from nekstab_next_amd.vector import NekContext

    lay, co, U = _mesh("box", a.elements)
    adv = AdvectionDiffusion(NekContext(lay, max_cols=4), co, U, [0.01 * (1 + f) for f in range(lay.n_wf)], 1e-4, 1)
    pctx = pair_context(adv, max_cols=4)
    op = ResolventOperator(pctx, adv, 1.0, kdim=4)
    n, nf = lay.n_v, lay.n_wf
    x, f, y, yc = (pctx.vector() for _ in range(4))
    x.fill_hash(3)
    op.project(x)
    f.fill_hash(5)
    op.project(f)
    comp = ComposedStage(op)
    c, st = op.dt / 3.0, pctx.stream

    def stage_fused():
        op._cstage(x.ptr, adv._minv, op._r.data_ptr(), op._wa.data_ptr(), f.ptr, op.omega, c, y.ptr, st)

    def stage_composed():
        comp(x.storage, op._r, op._wa, f.storage, op.omega, c, yc.storage)

    def step(stage, out):
        """One forced RK4 step from x into ``out``: the four Horner passes of ResolventOperator._steps."""
        out.copy_from(x)
        src, srct = out.ptr, out.storage
        for s, wt in ((4, op._wa), (3, op._wb), (2, op._wa)):
            op._local_rhs(src, False, st)
            stage(out, srct, op.dt / s, wt)
            src, srct = wt.data_ptr(), wt
        op._local_rhs(src, False, st)
        stage(out, srct, op.dt, out.storage)

    def fused(v, s, cc, w):
        op._cstage(v.ptr, adv._minv, op._r.data_ptr(), s.data_ptr(), f.ptr, op.omega, cc, w.data_ptr(), st)

    def composed(v, s, cc, w):
        comp(v.storage, op._r, s, f.storage, op.omega, cc, w)

    legs = {
        "cstage_fused": (stage_fused, 11 * nf),
        "cstage_composed": (stage_composed, 11 * nf),
        "step_fused": (lambda: step(fused, y), 0),
        "step_composed": (lambda: step(composed, yc), 0),
    }
    op._wa.copy_(x.storage[: op._wa.numel()])   # a source and a right-hand side with live values
    op._local_rhs(x.ptr, False, st)
    for fn, _ in legs.values():                  # warm every shape
        fn()
    torch.cuda.synchronize()
    op._wa.copy_(x.storage[: op._wa.numel()])
    op._local_rhs(x.ptr, False, st)
    stage_fused()
    stage_composed()
    torch.cuda.synchronize()
    live = slice(0, nf * pctx.layout.sv)
    dev = float(torch.max(torch.abs(y.storage[live] - yc.storage[live])).item()) / float(torch.max(torch.abs(y.storage[live])).item())
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
    lines = [dict(E=lay.nelv, lx1=lay.lx1, ldim=lay.ldim, n_wf=nf, n_v=n, omega=op.omega, reps=a.reps, rounds=a.rounds,
                  composed_vs_fused_rel_max=dev,
                  device=torch.cuda.get_device_properties(pctx.device).gcnArchName.split(":")[0])]
    out = {}
    for name, (_, doubles) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        byts = 8 * doubles * n
        out[name] = dict(leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), GB=round(byts / 1e9, 4),
                         gbs_median=round(byts / (med * 1e-3) / 1e9, 1), frac_peak=round(byts / (med * 1e-3) / PEAK, 3))
        lines.append(out[name])
    lines.append(dict(stage_composed_over_fused=round(out["cstage_composed"]["ms_median"] / out["cstage_fused"]["ms_median"], 2),
                      step_composed_over_fused=round(out["step_composed"]["ms_median"] / out["step_fused"]["ms_median"], 2)))
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
    lines = bench(a)
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
