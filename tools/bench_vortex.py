"""Time the fused vortex-criteria launch (nkv_vortex_criteria; csrc/vortex.hip) producing lambda2, q and
omega — the velocity field of nekStab_outpost's ``vox`` file — at config 5's mesh (3-D, lx1=8, E=22,088:
11.3M points per field), next to the same result composed from nkv_gradm1, torch pointwise operations and
nkv_filter_s0, in the same process.

  python tools/bench_vortex.py [--elements 22088] [--reps 5] [--rounds 5] [--lib path/to/libnekkrylov.so]

The legs alternate inside each round in ONE process (boxes differ by 1.5-3 %: only numbers of one
process compare); per leg the median and the minimum over the rounds are printed as one JSON line.
Bytes are the algorithmic streams in doubles per point n_v (8 bytes each), 3-D:
  fused              3 coordinates + 3 velocities read, 3 criteria written                       = 9
  fused_q_omega      6 read, 2 written (no lambda2: the Jacobi sweeps are the arithmetic-heavy part) = 8
  composed           gradm1 of 3 fields (6 read, 9 written) = 15; the pointwise criteria as ONE pass
                     (9 read, 3 written) = 12; filter_s0 of q and omega (2 read, 2 written) = 4   = 31
                     (torch runs the pointwise part as hundreds of elementwise kernels, the Jacobi sweeps
                     of lambda2 above all: what a caller without the fused entry writes; the byte model
                     counts the single pass it could be)
  composed_q_omega   15 + (9 read, 2 written) + 4                                                  = 30
  filter_s0          2 fields read, 2 written                                                      = 4
  energy             nkv_energy_components: 3 components + weights read                            = 4
and TB/s is bytes over the event-timed call, against the 8 TB/s HBM3E peak.
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

PEAK = 8.0e12


def _jacobi_rotate(app, aqq, apq, arp, arq):
    nz = apq != 0
    den = torch.where(nz, apq, torch.ones_like(apq))
    theta = (aqq - app) / (2.0 * den)
    one = torch.ones_like(theta)
    t = torch.where(theta >= 0, one, -one) / (theta.abs() + torch.sqrt(theta * theta + 1.0))
    t = torch.where(nz, t, torch.zeros_like(t))
    c = 1.0 / torch.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    return app - h, aqq + h, 0.0 * apq, c * arp - s * arq, s * arp + c * arq


def torch_criteria(G, with_lambda2=True):
    """lambda2, q, omega from the gradient tensor G[i][j] (views of n points) in the kernel's operand order."""
    q = (G[1][1] * G[2][2] - G[1][2] * G[2][1]) + (G[0][0] * G[1][1] - G[0][1] * G[1][0])
    q = q + (G[2][2] * G[0][0] - G[0][2] * G[2][0])
    S = [[0.5 * (G[i][j] + G[j][i]) for j in range(3)] for i in range(3)]
    O = [[0.5 * (G[i][j] - G[j][i]) for j in range(3)] for i in range(3)]
    sa = torch.zeros_like(q)
    sb = torch.zeros_like(q)
    for j in range(3):
        for i in range(3):
            sa = sa + S[i][j] * S[i][j]
            sb = sb + O[i][j] * O[i][j]
    a, b = sa * sa, sb * sb
    omega = b / ((a + b) + 1.0e-5)
    if not with_lambda2:
        return None, q, omega

    def entry(i, j):
        acc = S[i][0] * S[0][j] + O[i][0] * O[0][j]
        for k in (1, 2):
            acc = acc + S[i][k] * S[k][j]
            acc = acc + O[i][k] * O[k][j]
        return acc

    a00, a01, a02, a11, a12, a22 = entry(0, 0), entry(0, 1), entry(0, 2), entry(1, 1), entry(1, 2), entry(2, 2)
    for _ in range(5):
        a00, a11, a01, a02, a12 = _jacobi_rotate(a00, a11, a01, a02, a12)
        a00, a22, a02, a01, a12 = _jacobi_rotate(a00, a22, a02, a01, a12)
        a11, a22, a12, a01, a02 = _jacobi_rotate(a11, a22, a12, a01, a02)
    lo, hi = torch.minimum(a00, a11), torch.maximum(a00, a11)
    return torch.maximum(lo, torch.minimum(hi, a22)), q, omega


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

    from nekstab_next_amd import synthetic as syn
    from nekstab_next_amd.layout import NekLayout
    from nekstab_next_amd.sensitivity import velocity_layout
    from nekstab_next_amd.vector import NekContext
    from nekstab_next_amd.vortex import VortexCore

    lx1, d, nel = 8, 3, a.elements
    nz = -(-nel // 484)
    full = NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=22 * 22 * nz)
    box = box_mesh_coords(full, (22, 22, nz), L=(1.0, 1.0, 2.0))
    co = {k: box[k][: nel * lx1 ** 3] for k in ("x", "y", "z")}
    del box
    lay = velocity_layout(NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=nel))
    ctx = NekContext(lay, weights=syn.mass_weights(lay), max_cols=4)
    sv, n = lay.sv, lay.n_v
    core = VortexCore(ctx, co)
    op = core.grad_op
    vel = ctx.vector()
    vel.fill_hash(20)
    f64 = dict(dtype=torch.float64, device=ctx.device)
    out3, out2 = torch.zeros(3 * sv, **f64), torch.zeros(2 * sv, **f64)
    G = torch.zeros(9 * sv, **f64)
    Gv = G.view(3, 3, sv)[:, :, :n]
    comp = torch.zeros(3 * sv, **f64)
    cv = comp.view(3, sv)
    sums = torch.zeros(4, **f64)

    def fused():
        core.launch(vel.ptr, sv, ["lambda2", "q", "omega"], True, out3.data_ptr(), sv)

    def fused_q_omega():
        core.launch(vel.ptr, sv, ["q", "omega"], True, out2.data_ptr(), sv)

    def composed(with_lambda2=True):
        op(vel.ptr, G.data_ptr(), nfld=3, u_stride=sv, g_stride=sv)
        l2, q, om = torch_criteria(Gv, with_lambda2)
        if with_lambda2:
            cv[0, :n] = l2
        cv[1, :n] = q
        cv[2, :n] = om
        core.filter(comp.data_ptr() + 8 * sv, nfld=2, stride=sv)

    def filter_s0():
        core.filter(out2.data_ptr(), nfld=2, stride=sv)

    def energy():
        ctx.call("nkv_energy_components", ctx.w.data_ptr(), vel.ptr, sv, 3, None, None, sums.data_ptr(),
                 ctx.ws.data_ptr(), ctx.stream)

    legs = {
        "fused": (fused, 9),
        "fused_q_omega": (fused_q_omega, 8),
        "composed": (composed, 31),
        "composed_q_omega": (lambda: composed(False), 30),
        "filter_s0": (filter_s0, 4),
        "energy": (energy, 4),
    }
    for fn, _ in legs.values():   # warm every shape
        fn()
    torch.cuda.synchronize()
    fused()
    composed()
    torch.cuda.synchronize()
    dev = float(torch.max(torch.abs(out3.view(3, sv)[:, :n] - cv[:, :n])).item())
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
    info = dict(E=nel, lx1=lx1, n_v=n, reps=a.reps, rounds=a.rounds, fused_vs_composed_max_abs=dev,
                device=torch.cuda.get_device_properties(ctx.device).gcnArchName.split(":")[0])
    print(json.dumps(info), flush=True)
    out = {}
    for name, (_, doubles) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        byts = 8 * doubles * n
        out[name] = dict(leg=name, ms_median=round(med, 4), ms_min=round(mn, 4), GB=round(byts / 1e9, 3),
                         tbs_median=round(byts / (med * 1e-3) / 1e12, 3), frac_peak=round(byts / (med * 1e-3) / PEAK, 3))
        print(json.dumps(out[name]), flush=True)
    print(json.dumps(dict(composed_over_fused=round(out["composed"]["ms_median"] / out["fused"]["ms_median"], 2),
                          composed_over_fused_q_omega=round(out["composed_q_omega"]["ms_median"]
                                                            / out["fused_q_omega"]["ms_median"], 2))), flush=True)


if __name__ == "__main__":
    main()
