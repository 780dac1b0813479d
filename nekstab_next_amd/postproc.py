"""Eigenmode kinetic-energy budget on the device (nekStab's ``stability_energy_budget``,
core/postproc.f90:649-872; ``uparam(1) = 4.1``, the step between 3.1 and 3.2 of the reference's job
chain, which waits for its ``PKE_dRe<session>0.f00001``).

Per mode the reference forms (all pointwise, then ``glsc2`` with the mass matrix ``bm1``, :728-730)

* nine production terms P[c][d] = -0.5 (re_c re_d + im_d im_c) d(base_c)/dx_d (``compute_production``,
  :801-836; ``gradm1`` of the base flow without ``dsavg``) — here ONE tiled pass
  (``nkv_pke_production``) that differentiates the base flow in LDS and returns the nine fields and
  their nine integrals together;
* the dissipation 0.5 nu sum_c (re_c Lap re_c + im_c Lap im_c) (``compute_dissipation``, :761-799),
  each Laplacian being four ``gradm1`` + ``dsavg`` rounds of which it keeps a third (:853-872) — here one
  gradient of the 2 ldim mode components (``nkv_gradm1``), ``dsavg`` of every first derivative, one
  divergence (``nkv_divm1``), ``dsavg`` of the 2 ldim Laplacians and one fused term + integral
  (``nkv_pke_dissipation``).  On several ranks ``gs.GatherScatter`` averages each round in one batch: two
  exchanges per mode.  ``dsavg`` is linear, so averaging the sum d2x + d2y + d2z equals the reference's
  sum of the three averages to rounding.

The ten local integrals travel in one all-reduce.  In 2-D every term with a z factor (integrals 3, 6,
7, 8, 9 and d2z) is absent, i.e. zero: the reference reads never-set arrays there.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .newton import fortran_e
from .sensitivity import Gradm1, _out_file, _scal_velocity
from .vector import NekContext, NekVector


def _bm1_tensor(ctx: NekContext, bm1) -> torch.Tensor:
    """The mass-matrix weights on the device: the context's by default, else ``bm1`` (n_v values)."""
    if bm1 is None:
        return ctx.w
    if isinstance(bm1, torch.Tensor):
        t = bm1.to(device=ctx.device, dtype=torch.float64)
    else:
        t = torch.as_tensor(np.asarray(bm1, dtype=np.float64)).to(ctx.device)
    if t.numel() < ctx.layout.n_v:
        raise ValueError(f"bm1: {t.numel()} values, the layout has n_v={ctx.layout.n_v}")
    return t if t.numel() else torch.zeros(1, dtype=torch.float64, device=ctx.device)


def energy_budget_fields(ctx: NekContext, base: NekVector, dRe: NekVector, dIm: NekVector, grad_op: Gradm1,
                         face_average, nu: float, bm1=None):
    """postproc.f90:716-730 on velocity-only vectors (``base``: the base flow; ``dRe``/``dIm``: the
    mode, already scaled): returns (prod, diss, integrals) — ``prod`` ldim x ldim field segments
    [c][d] (``sv`` doubles each), ``diss`` one segment, ``integrals`` the ten ``glsc2(bm1, .)`` of the
    reference's ``energy_budget(:, 1..10)`` on the device, all-reduced (index 3c + d for P[c][d], 9 for
    the dissipation; the 2-D z entries stay zero).  ``face_average(ptr)`` is ``dsavg`` of one segment
    in place (a ``gs.GatherScatter`` averages each round's segments in one batch; None skips it);
    ``bm1`` defaults to the context's weights."""
    lay = ctx.layout
    d, sv = lay.ldim, lay.sv
    f64 = dict(dtype=torch.float64, device=ctx.device)
    w = _bm1_tensor(ctx, bm1)
    D, xyz = grad_op.D.data_ptr(), [t.data_ptr() for t in grad_op.xyz]
    zp = xyz[2] if d == 3 else None
    local = torch.zeros(16, **f64)       # [0, d*d): production, [12]: dissipation (this rank's partials)
    prod = torch.zeros(d * d * sv, **f64)
    ctx.call("nkv_pke_production", lay.lx1, d, D, xyz[0], xyz[1], zp, base.ptr, sv, dRe.ptr, dIm.ptr, sv,
             w.data_ptr(), prod.data_ptr(), sv, local.data_ptr(), ctx.ws.data_ptr(), ctx.stream)
    # Laplacians of the 2 d mode components: gradient, dsavg, divergence, dsavg
    grad = torch.zeros(2 * d * d * sv, **f64)   # [Re, Im][component][direction]
    gp = grad.data_ptr()
    grad_op(dRe.ptr, gp, nfld=d, u_stride=sv, g_stride=sv)
    grad_op(dIm.ptr, gp + 8 * d * d * sv, nfld=d, u_stride=sv, g_stride=sv)
    if face_average is not None:   # a GatherScatter: one batch (one exchange) per round, two per mode
        from .gs import average_segments

        average_segments(face_average, [gp + 8 * q * sv for q in range(2 * d * d)])
    lap = torch.zeros(2 * d * sv, **f64)        # [Re, Im][component]
    ctx.call("nkv_divm1", lay.lx1, d, D, xyz[0], xyz[1], zp, gp, 2 * d, sv, lap.data_ptr(), sv, ctx.stream)
    if face_average is not None:
        average_segments(face_average, [lap.data_ptr() + 8 * q * sv for q in range(2 * d)])
    diss = torch.zeros(sv, **f64)
    ctx.call("nkv_pke_dissipation", dRe.ptr, dIm.ptr, sv, lap.data_ptr(), sv, d, float(nu), w.data_ptr(),
             diss.data_ptr(), local.data_ptr() + 8 * 12, ctx.ws.data_ptr(), ctx.stream)
    integrals = torch.zeros(10, **f64)
    idx = torch.as_tensor([3 * c + k for c in range(d) for k in range(d)], device=ctx.device)
    integrals[idx] = local[: d * d]
    integrals[9] = local[12]
    ctx.comm.allreduce_(integrals)              # the ten glsc2 all-reduces of :729 as one
    return prod, diss, integrals


def pke_records(integrals) -> tuple[list, float, float]:
    """The twelve ``(1E15.7)`` records of ``PKE_dRe<session>0.f<mode>`` (postproc.f90:748-753): the ten
    integrals, sum(integrals(1:9)) and that sum minus integrals(10).  Returns (lines, total, balance)."""
    vals = [float(v) for v in integrals]
    if len(vals) != 10:
        raise ValueError(f"{len(vals)} integrals, the budget has 10")
    total = 0.0
    for v in vals[:9]:
        total = total + v
    balance = total - vals[9]
    return [fortran_e(v, 15, 7) for v in vals + [total, balance]], total, balance


def stability_energy_budget(ctx: NekContext, directory: str, coords: dict, session: str = "nek", nu: float = 1.0,
                            maxmodes: int = 20, normalize="reference", face_average="auto",
                            outdir: str | None = None, write_coords: bool = False, bm1=None) -> list:
    """``stability_energy_budget`` (postproc.f90:649-872) on a velocity-only context
    (``sensitivity.velocity_layout``): the velocity of ``BF_<session>0.f00001``, then for mode = 1 ..
    ``maxmodes`` (stopping at the first mode whose files are missing) ``dRe``/``dIm<session>0.f<mode>``,
    alpha = sqrt(norm(dRe)^2 + norm(dIm)^2) with the context's weights (``bm1s``, no time term), the
    scaling, the budget on the device, ``K<mode:02d><session><rank>.f0000{c+1}`` with the velocity
    (P[c][x], P[c][y][, P[c][z]]) for c < ldim, and on rank 0 the text file
    ``PKE_dRe<session>0.f<mode:05d>``.  ``nu`` is param(2)/param(1).

    ``normalize``: "reference" multiplies both parts by alpha as the reference does (``nopcmult``, :707-708,
    under a comment that says normalise); "unit" divides; None leaves the mode as loaded.
    ``face_average``: "auto" (``seeds.FaceAverage`` on one rank, ``gs.GatherScatter`` on several), a
    ``gs.GatherScatter``, a callable ``f(ptr)`` (dsavg of one field segment) or None.  ``bm1``: the mass
    matrix (n_v local values; default the context's weights, which differ from it only inside a sponge).
    Returns one dict per mode: integrals (10), total, balance, alpha, paths (and the fields of this rank's
    points: production [c][d], dissipation)."""
    from . import fld

    lay = ctx.layout
    if lay.n_scalars or lay.n_p or lay.n_wf != lay.ldim:
        raise ValueError("stability_energy_budget works on a velocity-only context (sensitivity.velocity_layout)")
    if normalize not in ("reference", "unit", None):
        raise ValueError("normalize: 'reference', 'unit' or None")
    if isinstance(face_average, str):
        if face_average != "auto":
            raise ValueError("face_average: 'auto', a callable f(ptr) or None")
        from .gs import auto_average

        face_average = auto_average(ctx, coords)
    grad_op = Gradm1(ctx, coords)
    w = _bm1_tensor(ctx, bm1)

    def load(prefix, num):
        files = fld.read_fld_set(directory, prefix, session, num, lay=lay, comm=ctx.comm)
        return ctx.vector().from_packed(fld.vector_from_fld(lay, files)), files[0]

    base, _ = load("BF_", 1)
    dst = outdir or directory
    os.makedirs(dst, exist_ok=True)
    d = lay.ldim
    results = []
    for mode in range(1, maxmodes + 1):
        try:
            dRe, _ = load("dRe", mode)
            dIm, last = load("dIm", mode)
        except FileNotFoundError:
            break
        a = math.sqrt(ctx.dot(dRe, dRe, time=False))   # norm (eigensolvers.f90:60-74)
        b = math.sqrt(ctx.dot(dIm, dIm, time=False))
        alpha = math.sqrt(a ** 2 + b ** 2)
        if normalize is not None:
            s = alpha if normalize == "reference" else 1.0 / alpha
            _scal_velocity(ctx, dRe, s)
            _scal_velocity(ctx, dIm, s)
        prod, _diss, integrals = energy_budget_fields(ctx, base, dRe, dIm, grad_op, face_average, nu, bm1=w)
        ctx.check_nan()
        host = prod.view(d, d, lay.sv)[:, :, : lay.n_v].cpu().numpy()
        vals = integrals.cpu().numpy()
        lines, total, balance = pke_records(vals)
        paths = []
        with fld.collective_output(ctx.comm):
            for c in range(d):
                f = _out_file(lay, last, coords if write_coords else None)
                for k, nm in enumerate(("vx", "vy", "vz")[:d]):
                    f.fields[nm] = host[c, k].reshape(lay.nelv, lay.pts_v)
                f.rdcode += "U"
                path = os.path.join(dst, fld.fld_name(f"K{mode:02d}", session, lay.rank, c + 1))
                fld.write_fld(path, f)
                paths.append(path)
            if ctx.comm.rank == 0:
                path = os.path.join(dst, f"PKE_dRe{session}0.f{mode:05d}")
                with open(path, "w") as fh:
                    fh.write("".join(ln + "\n" for ln in lines))
                paths.append(path)
        results.append(dict(integrals=vals, total=total, balance=balance, alpha=alpha, paths=paths,
                            production=[[host[c, k].copy() for k in range(d)] for c in range(d)],
                            dissipation=_diss[: lay.n_v].cpu().numpy()))
    return results
