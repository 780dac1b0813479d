"""Time the monitor kernels (nkv_torque, nkv_avg_step; csrc/monitors.hip) at the BASELINE layout, each next to
the same result composed from entries the library already had plus torch ops on the same tensors.

  python tools/bench_monitors.py [--ne 16 11 251] [--reps 5] [--rounds 5] [--lib path/to/libnekkrylov.so]

The mesh is a conforming ne[0] x ne[1] x ne[2] box (default 16 x 11 x 251 = 44,176 elements, lx1 = 8: the
layout of box3d_layout(44176)).  The legs alternate inside each round in ONE process (boxes differ by
1.5-3 %: only numbers of one process compare); per leg the median and the minimum over the rounds are
printed as one JSON line.
  torque_plane     the fused kernel, one boundary plane (x = 0) as the object
  torque_six       ... all six boundary planes as one object
  torque_composed_plane / _six
                   whole-volume nkv_gradm1 (ldim^2 gradient fields written), the mesh-2 -> mesh-1 pressure map
                   as three batched matmuls, then a torch gather at the face points (indices and nA
                   precomputed: the geometry is static) and the sums
  avg_step         avg and rms: per stored row 1 read + 2 read-modify-writes = 5 streams
  avg_step_cross   ... + uv, vw, wu: + 2 streams of n_v per cross moment
  avg_torch        avg and rms composed from torch ops (mul_, add_, addcmul_), rated with the fused bytes
The torque legs move O(faces) data and are latency-bound when the object has few faces: they are reported
in ms and in microseconds per face, not in GB/s.  GB/s of the avg legs is bytes over the event-timed call,
against the 8 TB/s HBM3E peak.
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

from nekstab_next_amd import _lib  # noqa: E402

PEAK = 8.0e12


def box_coords(lay, ne, L=(2.0, 1.0, 3.0)):
    from nekstab_next_amd.fld import gll_points

    n = lay.lx1
    g = 0.5 * (gll_points(n) + 1.0)
    e = np.arange(lay.nelgv)
    ex, ey, ez = e % ne[0], (e // ne[0]) % ne[1], e // (ne[0] * ne[1])
    kk, jj, ii = (a.ravel() for a in np.meshgrid(g, g, g, indexing="ij"))
    return {"x": ((ex[:, None] + ii[None, :]) * L[0] / ne[0]).ravel(),
            "y": ((ey[:, None] + jj[None, :]) * L[1] / ne[1]).ravel(),
            "z": ((ez[:, None] + kk[None, :]) * L[2] / ne[2]).ravel()}


def boundary(ne, planes):
    """(element, face) of the boundary faces on the listed planes (preprocessor face numbers)."""
    e = np.arange(int(np.prod(ne)))
    ex, ey, ez = e % ne[0], (e // ne[0]) % ne[1], e // (ne[0] * ne[1])
    on = {1: ey == 0, 2: ex == ne[0] - 1, 3: ey == ne[1] - 1, 4: ex == 0, 5: ez == 0, 6: ez == ne[2] - 1}
    return [(int(el), fc) for fc in planes for el in e[on[fc]]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, nargs=3, default=(16, 11, 251))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    a = ap.parse_args()
    _lib.load(a.lib)
    _lib.require_gpu()

    from nekstab_next_amd import fld
    from nekstab_next_amd import monitors as mon
    from nekstab_next_amd import synthetic as syn
    from nekstab_next_amd.layout import box3d_layout
    from nekstab_next_amd.sensitivity import Gradm1
    from nekstab_next_amd.vector import NekContext

    ne = tuple(a.ne)
    lay = box3d_layout(int(np.prod(ne)))
    ctx = NekContext(lay, weights=syn.mass_weights(lay), max_cols=2)
    d, n, nv, sv, nel = lay.ldim, lay.lx1, lay.n_v, lay.sv, lay.nelv
    dev = ctx.device
    co = box_coords(lay, ne)
    grad_op = Gradm1(ctx, co)
    v = ctx.vector()
    v.fill_hash(5)
    nu, x0, scale = 0.01, (0.3, -0.2, 0.1), 2.0
    objects = {"plane": [boundary(ne, (4,))], "six": [boundary(ne, (1, 2, 3, 4, 5, 6))]}
    tq = {k: mon.Torque(ctx, co, o, grad_op=grad_op) for k, o in objects.items()}

    # ---- the composed route: gradm1 over the volume, the pressure map, a gather and the sums ----
    G = torch.empty((d * d, nv), dtype=torch.float64, device=dev)
    Ip = torch.as_tensor(fld.interp_matrix(fld.gauss_points(lay.lx2), fld.gll_points(n))).to(dev)
    xyz = torch.stack([t[:nv] for t in grad_op.xyz])
    x0t = torch.tensor(x0, dtype=torch.float64, device=dev)
    static = {}
    for k, t in tq.items():
        t.compute(v, nu, x0=x0, scale=scale, distributions=True)       # nA of the fused kernel: static geometry
        idx = np.concatenate([e * lay.pts_v + mon.face_points(n, d, fc) for e, fc, _ in t.faces])
        static[k] = (torch.as_tensor(idx).to(dev), t.na.permute(1, 0, 2).reshape(d, -1).clone())

    def composed(kind):
        idx, na = static[kind]
        grad_op(v.ptr, G.data_ptr(), nfld=d, u_stride=sv, g_stride=nv)
        p2 = v.storage[lay.n_wf * sv: lay.n_wf * sv + lay.n_p].view(nel, lay.lx2, lay.lx2, lay.lx2)
        pm = torch.matmul(p2, Ip.T)                                                     # along r
        pm = torch.matmul(Ip, pm)                                                       # along s
        pm = torch.matmul(Ip, pm.reshape(nel, lay.lx2, n * n)).reshape(-1)              # along t
        g = G[:, idx].view(d, d, -1)
        s = g + g.transpose(0, 1)
        fp = pm[idx] * na                                                               # [d, points]
        fv = -nu * torch.einsum("cdp,dp->cp", s, na)
        r = xyz[:, idx] - x0t[:, None]
        out = torch.stack([fp.sum(1), fv.sum(1), torch.linalg.cross(r, fp, dim=0).sum(1),
                           torch.linalg.cross(r, fv, dim=0).sum(1)]) * scale
        return out

    # ---- statistics ----
    avg, rms, avg_t, rms_t = (ctx.vector() for _ in range(4))
    cross = torch.zeros(3 * sv, dtype=torch.float64, device=dev)
    alpha, beta = 0.9, 0.1
    rows = lay.rows

    def avg_step():
        ctx.call("nkv_avg_step", v.ptr, avg.ptr, rms.ptr, None, 0, alpha, beta, ctx.stream)

    def avg_step_cross():
        ctx.call("nkv_avg_step", v.ptr, avg.ptr, rms.ptr, cross.data_ptr(), 3, alpha, beta, ctx.stream)

    def avg_torch():
        x = v.storage[:rows]
        avg_t.storage[:rows].mul_(alpha).add_(x, alpha=beta)
        rms_t.storage[:rows].mul_(alpha).addcmul_(x, x, value=beta)

    legs = {
        "torque_plane": (lambda: tq["plane"].compute(v, nu, x0=x0, scale=scale), tq["plane"].nfaces),
        "torque_composed_plane": (lambda: composed("plane").cpu(), tq["plane"].nfaces),
        "torque_six": (lambda: tq["six"].compute(v, nu, x0=x0, scale=scale), tq["six"].nfaces),
        "torque_composed_six": (lambda: composed("six").cpu(), tq["six"].nfaces),
        "avg_step": (avg_step, 5 * lay.N),
        "avg_step_cross": (avg_step_cross, 5 * lay.N + 6 * nv),
        "avg_torch": (avg_torch, 5 * lay.N),
    }
    # the composed route gives the fused result (to rounding: another summation order, torch may contract)
    diffs = {}
    for k in tq:
        want = tq[k].compute(v, nu, x0=x0, scale=scale)[0]
        got = composed(k).cpu().numpy()
        diffs[k] = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    avg_step()
    avg_torch()
    live = slice(0, nv)
    avg_diff = float((avg.storage[live] - avg_t.storage[live]).abs().max())
    times = {k: [] for k in legs}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn_, _ in legs.values():
        fn_()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (fn_, _) in legs.items():
            s.record()
            for _ in range(a.reps):
                fn_()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / a.reps)
    info = dict(ne=list(ne), E=lay.nelgv, rows=rows, n_v=nv, reps=a.reps, rounds=a.rounds,
                faces_plane=tq["plane"].nfaces, faces_six=tq["six"].nfaces, composed_torque_rel_diff=diffs,
                composed_avg_abs_diff=avg_diff,
                device=torch.cuda.get_device_properties(dev).gcnArchName.split(":")[0])
    print(json.dumps(info), flush=True)
    out = {}
    for name, (_, work) in legs.items():
        med, mn = statistics.median(times[name]), min(times[name])
        rec = dict(leg=name, ms_median=round(med, 4), ms_min=round(mn, 4))
        if name.startswith("torque"):
            rec.update(faces=work, us_per_face=round(1e3 * med / work, 4))
        else:
            byts = 8 * work
            rec.update(GB=round(byts / 1e9, 3), gbs_median=round(byts / (med * 1e-3) / 1e9, 1),
                       frac_peak=round(byts / (med * 1e-3) / PEAK, 3))
        out[name] = rec
        print(json.dumps(rec), flush=True)
    ratio = lambda p, q: round(out[p]["ms_median"] / out[q]["ms_median"], 2)   # noqa: E731
    print(json.dumps(dict(torque_plane_composed_over_fused=ratio("torque_composed_plane", "torque_plane"),
                          torque_six_composed_over_fused=ratio("torque_composed_six", "torque_six"),
                          avg_composed_over_fused=ratio("avg_torch", "avg_step"))), flush=True)


if __name__ == "__main__":
    main()
