"""Time the advection-diffusion entries (nkv_advdiff_rhs, nkv_advdiff_stage; csrc/advdiff.hip) and one full RK4
step of advdiff.AdvectionDiffusion, next to the same right-hand side composed from what predates them:
nkv_gradm1, the pointwise fluxes in torch and the transposed line sums as torch contractions.

  python tools/bench_advdiff.py [--case box|cyl|both] [--elements 22088] [--reps 5] [--rounds 5]
                                [--lib path/to/libnekkrylov.so] [--out profiles/advdiff_bench.json]

box: 3-D, lx1=8, E=22,088 (11.3M points per field, DESIGN §4's 3-D size), vx vy vz t (n_wf = 4).
cyl: the 2-D cylinder mesh of tests/golden (E=1,996, lx1=6, n_wf = 2) with its Re=50 base flow: 72k points,
     a launch-bound size.
The legs alternate inside each round in ONE process (boxes differ by 1.5-3 %: only numbers of one process
compare); per leg the median and the minimum over the rounds go out as one JSON line.  Bytes are the
algorithmic streams: 8 n_v (2 ldim + 2 nfld) for a right-hand side (coordinates, U, u in, r out),
8 n_v (3 nfld + 1) for a stage (v, r in, w out, minv); GB/s against the 8 TB/s HBM3E peak.  The composed
leg is held to the fused result first (max difference over the test gate's scale is printed).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from nekstab_next_amd import _lib  # noqa: E402

PEAK = 8.0e12


def _mesh(case, nel):
    from nekstab_next_amd import synthetic as syn
    from nekstab_next_amd.layout import NekLayout, cylinder_layout

    if case == "cyl":
        gold = os.path.join(ROOT, "tests", "golden")
        lay = cylinder_layout(1996)
        d = np.load(os.path.join(gold, "cyl_mesh_xy.npz"))
        bf = syn.from_reference_order(lay, np.load(os.path.join(gold, "bf_1cyl0_seed.npz"))["seed_ref"])
        return lay, {"x": d["x"], "y": d["y"]}, [bf[c * lay.sv: c * lay.sv + lay.n_v].copy() for c in range(2)]
    from seed_helpers import box_mesh_coords

    nz = -(-nel // 484)
    full = NekLayout(ldim=3, lx1=8, lx2=6, nelgv=22 * 22 * nz)
    box = box_mesh_coords(full, (22, 22, nz), L=(1.0, 1.0, 2.0))
    lay = NekLayout(ldim=3, lx1=8, lx2=6, nelgv=nel, n_scalars=1)
    co = {k: box[k][: lay.n_v] for k in ("x", "y", "z")}
    x, y, z = co["x"], co["y"], co["z"]
    return lay, co, [np.sin(y) + 0.3, 0.5 * np.cos(x), 0.2 * np.sin(x + z)]


class Composed:
    """The right-hand side from nkv_gradm1, torch pointwise operations and torch contractions.  The inverse
    metrics M[d][a] = g[d][a] / jac and bm1 are formed once (not timed), as a caller without the fused entry
    would keep them."""

    def __init__(self, op):
        from nekstab_next_amd.sensitivity import Gradm1

        ctx = op.ctx
        lay = ctx.layout
        self.op, self.lay = op, lay
        n, d, nx = lay.n_v, lay.ldim, lay.lx1
        self.shape = (lay.nelv,) + (nx,) * d                # (e, [k,] j, i)
        self.grad_op = Gradm1.__new__(Gradm1)
        self.grad_op.ctx, self.grad_op.D, self.grad_op.xyz = ctx, op.D, op.xyz
        D = op.D
        self.lines = ("im,...m->...i", "jm,...mi->...ji", "km,...mji->...kji")[:d]
        self.lines_t = ("mi,...m->...i", "mj,...mi->...ji", "mk,...mji->...kji")[:d]
        X = [t[:n].view(self.shape) for t in op.xyz]
        J = [[torch.einsum(self.lines[a], D, X[c]) for a in range(d)] for c in range(d)]   # dx_c / dr_a
        if d == 2:
            (xr, xs), (yr, ys) = J
            jac = xr * ys - xs * yr
            g = [[ys, -yr], [-xs, xr]]
        else:
            (xr, xs, xt), (yr, ys, yt), (zr, zs, zt) = J
            jac = xr * ys * zt + xt * yr * zs + xs * yt * zr - xr * yt * zs - xs * yr * zt - xt * ys * zr
            g = [[ys * zt - yt * zs, yt * zr - yr * zt, yr * zs - ys * zr],
                 [xt * zs - xs * zt, xr * zt - xt * zr, xs * zr - xr * zs],
                 [xs * yt - xt * ys, xt * yr - xr * yt, xr * ys - xs * yr]]
        self.M = [[(g[dd][a] / jac).contiguous() for a in range(d)] for dd in range(d)]
        self.bm1 = op.bm1.view(self.shape)
        self.U = [op.U[c * lay.sv: c * lay.sv + n].view(self.shape) for c in range(d)]
        self.grad = torch.zeros(lay.n_wf * d * n, dtype=torch.float64, device=ctx.device)

    def __call__(self, u_ptr, nfld, out, adjoint=False):
        """out[f] (views of n_v) <- the local right-hand side of the nfld fields at u_ptr (stride sv)."""
        lay, d, n = self.lay, self.lay.ldim, self.lay.n_v
        self.grad_op(u_ptr, self.grad.data_ptr(), nfld=nfld, u_stride=lay.sv, g_stride=n)
        kap = self.op.kappa
        for f in range(nfld):
            du = [self.grad[(f * d + dd) * n:(f * d + dd + 1) * n].view(self.shape) for dd in range(d)]
            G = [-(kap[f] * self.bm1) * du[dd] for dd in range(d)]
            r = 0
            for a in range(d):
                F = sum(self.M[dd][a] * G[dd] for dd in range(d))
                r = r + torch.einsum(self.lines_t[a], self.op.D, F)
            r = r - self.bm1 * sum(self.U[dd] * du[dd] for dd in range(d))
            out[f].copy_(r.reshape(-1))


def bench(case, a):
    from nekstab_next_amd.advdiff import AdvectionDiffusion
    from nekstab_next_amd.vector import NekContext

    lay, co, U = _mesh(case, a.elements)
    ctx = NekContext(lay, max_cols=4)
    n, sv, nf, d = lay.n_v, lay.sv, lay.n_wf, lay.ldim
    op = AdvectionDiffusion(ctx, co, U, [0.01 * (1 + f) for f in range(nf)], 1e-4, 1)
    x, y = ctx.vector(), ctx.vector()
    x.fill_hash(3)
    op.project(x)
    f64 = dict(dtype=torch.float64, device=ctx.device)
    r = torch.zeros(nf * sv, **f64)
    st = ctx.stream
    xyz = op._xyz_ptrs()

    def rhs(nfld, adjoint):
        ctx.call("nkv_advdiff_rhs", lay.lx1, d, op.D.data_ptr(), op.w.data_ptr(), *xyz, op.U.data_ptr(), sv,
                 op.kappa.data_ptr(), x.ptr, nfld, sv, r.data_ptr(), sv, int(adjoint), st)

    def stage():
        ctx.call("nkv_advdiff_stage", x.ptr, sv, op._minv.data_ptr(), r.data_ptr(), sv, 0.25e-4, y.ptr, sv, nf, 0, st)

    def step():   # the four Horner passes of one RK4 step: right-hand side, dsavg of n_wf segments, stage
        src = x.ptr
        for s in (4, 3, 2):
            op._local_rhs(src, False)
            op._stage(x.ptr, op._minv, op._r.data_ptr(), op.dt / s, op._w.data_ptr())
            src = op._w.data_ptr()
        op._local_rhs(src, False)
        op._stage(x.ptr, op._minv, op._r.data_ptr(), op.dt, y.ptr, zero_rest=True)

    comp = Composed(op)
    rc = torch.zeros(nf * n, **f64)
    rc_rows = [rc[f * n:(f + 1) * n] for f in range(nf)]
    legs = {
        "rhs_forward_1": (lambda: rhs(1, False), 2 * d + 2),
        "rhs_adjoint_1": (lambda: rhs(1, True), 2 * d + 2),
        f"rhs_forward_{nf}": (lambda: rhs(nf, False), 2 * d + 2 * nf),
        f"rhs_adjoint_{nf}": (lambda: rhs(nf, True), 2 * d + 2 * nf),
        "composed_forward_1": (lambda: comp(x.ptr, 1, rc_rows), 2 * d + 2),
        f"composed_forward_{nf}": (lambda: comp(x.ptr, nf, rc_rows), 2 * d + 2 * nf),
        "stage": (stage, 3 * nf + 1),
        "step": (step, 0),
    }
    for fn, _ in legs.values():   # warm every shape
        fn()
    torch.cuda.synchronize()
    rhs(nf, False)
    comp(x.ptr, nf, rc_rows)
    torch.cuda.synchronize()
    fused = r.view(nf, sv)[:, :n]
    dev = float(torch.max(torch.abs(fused - rc.view(nf, n))).item()) / float(torch.max(torch.abs(fused)).item())
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
    lines = [dict(case=case, E=lay.nelv, lx1=lay.lx1, ldim=d, n_wf=nf, n_v=n, reps=a.reps, rounds=a.rounds,
                  composed_vs_fused_rel_max=dev,
                  device=torch.cuda.get_device_properties(ctx.device).gcnArchName.split(":")[0])]
    out = {}
    for name, (_, doubles) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        byts = 8 * doubles * n
        out[name] = dict(case=case, leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), GB=round(byts / 1e9, 4),
                         gbs_median=round(byts / (med * 1e-3) / 1e9, 1), frac_peak=round(byts / (med * 1e-3) / PEAK, 3))
        lines.append(out[name])
    lines.append(dict(case=case,
                      composed_over_fused_1=round(out["composed_forward_1"]["ms_median"] / out["rhs_forward_1"]["ms_median"], 2),
                      **{f"composed_over_fused_{nf}": round(out[f"composed_forward_{nf}"]["ms_median"]
                                                            / out[f"rhs_forward_{nf}"]["ms_median"], 2)}))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("box", "cyl", "both"), default="both")
    ap.add_argument("--elements", type=int, default=22088)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    _lib.load(a.lib)
    _lib.require_gpu()
    lines = []
    for case in (("box", "cyl") if a.case == "both" else (a.case,)):
        for ln in bench(case, a):
            print(json.dumps(ln), flush=True)
            lines.append(ln)
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
