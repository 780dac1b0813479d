"""Per-time-step monitors on the device: the lift / drag / torque record and the running statistics.

* ``nekStab_torque`` (core/utils.f90:718-879, ``lift_drag.dat``): :class:`Torque` integrates the pressure and
  viscous forces and their moments over the member faces of every object in ONE launch whose cost scales
  with the number of faces (``nkv_torque``, csrc/monitors.hip) and one all-reduce of the 12 (nobj + 1)
  partial sums; :class:`TorqueMonitor` writes the record.  Nek5000's ``comp_sij``, ``drgtrq``, ``mappr``
  and ``create_obj`` are not part of the reference tree: they are restated from their definitions
  (DESIGN.md §3).  :func:`wall_faces` plays ``nekStab_define_obj``'s role from the coordinates alone
  (no ``cbc``: reading ``.re2`` boundary conditions is out of scope).
* ``nekStab_avg`` (core/postproc.f90:524-646): :class:`Statistics` keeps the running mean, mean square and
  (opt-in) cross moments of a state vector with one streaming launch per step (``nkv_avg_step``) on the
  reference's schedule, and dumps the ``avt`` / ``avg`` / ``rms`` / ``rm2`` files.

Both follow the monitor protocol of ``SFD(monitors=...)`` / ``TDF(monitors=...)``: ``m(v, istep, time)``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import fld
from .fixedp import fortran_e
from .sensitivity import Gradm1
from .synthetic import gll_weights
from .vector import NekContext, NekVector, k_sub3

# preprocessor face number -> (reference direction 0 r, 1 s, 2 t; side -1 / +1)
FACES = {1: (1, -1), 2: (0, +1), 3: (1, +1), 4: (0, -1), 5: (2, -1), 6: (2, +1)}


def face_points(lx1: int, ldim: int, face: int) -> np.ndarray:
    """Indices (into the lx1^ldim points of an element, r fastest) of the GLL points of ``face`` in the
    kernel's face-point order: fp = a + lx1 b over the in-face directions in ascending order."""
    if face not in FACES or face > 2 * ldim:
        raise ValueError(f"face {face} outside 1..{2 * ldim}")
    d, side = FACES[face]
    n = lx1
    c0 = n - 1 if side > 0 else 0
    a = np.arange(n)
    if ldim == 2:
        i, j = (np.full(n, c0), a) if d == 0 else (a, np.full(n, c0))
        return i + n * j
    b, a = (g.ravel() for g in np.meshgrid(a, a, indexing="ij"))   # a fastest
    c = np.full(n * n, c0)
    i, j, k = {0: (c, a, b), 1: (a, c, b), 2: (a, b, c)}[d]
    return i + n * j + n * n * k


def wall_faces(lay, coords: dict, predicate) -> list:
    """The faces of this rank's elements whose GLL points ALL satisfy ``predicate(x, y[, z])`` (arrays in,
    a boolean array out), as ``(global element, face)`` pairs with 0-based elements and the
    preprocessor's face numbers, elements ascending and faces ascending within an element.
    ``nekStab_define_obj``'s role (utils.f90:881-), from the geometry instead of ``cbc``."""
    n, d = lay.lx1, lay.ldim
    e0, _ = lay.elem_range()
    xyz = [np.asarray(coords[k], dtype=np.float64).reshape(lay.nelv, lay.pts_v) for k in ("x", "y", "z")[:d]]
    out = []
    hit = {}
    for fc in range(1, 2 * d + 1):
        idx = face_points(n, d, fc)
        ok = np.asarray(predicate(*[c[:, idx] for c in xyz]), dtype=bool)
        hit[fc] = ok.reshape(lay.nelv, -1).all(axis=1)
    for e in range(lay.nelv):
        for fc in range(1, 2 * d + 1):
            if hit[fc][e]:
                out.append((e0 + e, fc))
    return out


def torque_record(istep: int, time: float, row, ldim: int) -> str:
    """One line of ``lift_drag.dat`` for one object (utils.f90:868-873).  ``row``: [4, 3] (pressure force,
    viscous force, pressure torque, viscous torque).  ``(i8,19E15.7)`` in 3-D: istep, time, then (total,
    pressure, viscous) of dragx, dragy, dragz, torqx, torqy, torqz; ``(i8,10E15.7)`` in 2-D: dragx, dragy
    and torqz."""
    r = np.asarray(row, dtype=np.float64).reshape(4, 3)
    trip = lambda p, v: (p + v, p, v)  # noqa: E731
    vals = [float(time)]
    for k in range(ldim):
        vals += trip(r[0, k], r[1, k])
    for k in (range(3) if ldim == 3 else (2,)):
        vals += trip(r[2, k], r[3, k])
    return f"{int(istep):8d}" + "".join(fortran_e(v, 15, 7) for v in vals)


class Torque:
    """The surface-force integrals of ``nekStab_torque`` on this rank's share of the objects.

    ``objects``: one list of ``(global element, face)`` pairs per object (0-based elements, preprocessor
    face numbers; :func:`wall_faces` makes one), every rank passing the same lists or only its own
    members: a rank keeps the members whose element lies in its ``elem_range()``, as ``gllnid(ieg) ==
    nid`` does (:808), in the order given.  ``grad_op`` reuses an existing :class:`~.sensitivity.Gradm1`
    (its D and coordinates)."""

    def __init__(self, ctx: NekContext, coords: dict, objects, grad_op: Gradm1 | None = None):
        lay = ctx.layout
        self.ctx = ctx
        self.grad_op = grad_op if grad_op is not None else Gradm1(ctx, coords)
        self.D, self.xyz = self.grad_op.D, self.grad_op.xyz
        self.nobj = len(objects)
        if self.nobj < 1:
            raise ValueError("Torque needs at least one object")
        e0, e1 = lay.elem_range()
        rows = []
        for o, members in enumerate(objects, start=1):
            for eg, fc in members:
                eg, fc = int(eg), int(fc)
                if not 0 <= eg < lay.nelgv:
                    raise ValueError(f"object {o}: element {eg} outside 0..{lay.nelgv - 1}")
                if not 1 <= fc <= 2 * lay.ldim:
                    raise ValueError(f"object {o}: face {fc} outside 1..{2 * lay.ldim}")
                if e0 <= eg < e1:
                    rows.append((eg - e0, fc, o))
        self.faces = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 3))
        self.nfaces = self.faces.shape[0]
        f64 = dict(dtype=torch.float64, device=ctx.device)
        self.faces_dev = torch.as_tensor(self.faces if self.nfaces else np.zeros((1, 3), np.int32)).to(ctx.device)
        self.wg = torch.as_tensor(gll_weights(lay.lx1)).to(ctx.device)
        self.Ipm = None
        if lay.ifpo:   # mappr: lx2 Gauss -> lx1 GLL points; lx1 == lx2: the pressure already lives on mesh 1
            I = (np.eye(lay.lx1) if lay.lx1 == lay.lx2 else
                 fld.interp_matrix(fld.gauss_points(lay.lx2), fld.gll_points(lay.lx1)))
            self.Ipm = torch.as_tensor(np.ascontiguousarray(I)).to(ctx.device)
        self.nfp = lay.lx1 ** (lay.ldim - 1)
        self.dgtq = torch.zeros((max(self.nfaces, 1), 12), **f64)      # per-face partials
        self.out = torch.zeros((self.nobj + 1, 12), **f64)
        self.sij = self.na = None

    def compute(self, vec: NekVector, visc, x0=(0.0, 0.0, 0.0), scale: float = 2.0, dp_mean=(0.0, 0.0, 0.0),
                pm1=None, distributions: bool = False) -> np.ndarray:
        """[nobj + 1, 4, 3]: (pressure force, viscous force, pressure torque, viscous torque) x (x, y, z)
        per object, row 0 their sum over the objects (:839-864).  ``visc``: ``param(2)`` or a field of n_v
        values (``vdiff``); ``scale``: the reference hard-codes 2 (:754); ``dp_mean``: the mean pressure
        gradient of :766-768; ``pm1``: a mesh-1 pressure of n_v values (device tensor or array) instead of
        the vector's mesh-2 pressure, e.g. after the host's own element-boundary averaging.
        ``distributions``: also keep ``self.sij`` [face][3 | 6][face point] and ``self.na``
        [face][ldim][face point] (the wall-shear distribution).  One all-reduce (the reference: twelve)."""
        ctx, lay = self.ctx, self.ctx.layout
        three = lay.ldim == 3
        f64 = dict(dtype=torch.float64, device=ctx.device)
        if pm1 is not None:
            pm1 = torch.as_tensor(pm1).to(**f64)
            if pm1.numel() < lay.n_v:
                raise ValueError(f"pm1: {pm1.numel()} values, the layout has n_v={lay.n_v}")
            pr_ptr, pm1_ptr = None, pm1.data_ptr()
        else:
            if self.nfaces and not lay.n_p:
                raise ValueError("the layout stores no pressure: pass pm1")
            pr_ptr, pm1_ptr = vec.ptr + 8 * lay.n_wf * lay.sv, None
        vf = None
        if not np.isscalar(visc):
            vf = torch.as_tensor(visc).to(**f64)
            if vf.numel() < lay.n_v:
                raise ValueError(f"visc: {vf.numel()} values, the layout has n_v={lay.n_v}")
        if distributions and self.sij is None:
            self.sij = torch.zeros((max(self.nfaces, 1), 6 if three else 3, self.nfp), **f64)
            self.na = torch.zeros((max(self.nfaces, 1), lay.ldim, self.nfp), **f64)
        c3 = ctypes.c_double * 3
        ctx.call("nkv_torque", lay.lx1, lay.lx2, lay.ldim, self.D.data_ptr(), self.wg.data_ptr(),
                 self.Ipm.data_ptr() if self.Ipm is not None else None, self.xyz[0].data_ptr(),
                 self.xyz[1].data_ptr(), self.xyz[2].data_ptr() if three else None, vec.ptr, lay.sv, pr_ptr, pm1_ptr,
                 vf.data_ptr() if vf is not None else None, 0.0 if vf is not None else float(visc),
                 self.faces.ctypes.data if self.nfaces else None, self.faces_dev.data_ptr(), self.nfaces, self.nobj,
                 c3(*(float(a) for a in x0)), c3(*(float(a) for a in dp_mean)), float(scale),
                 self.dgtq.data_ptr(), self.out.data_ptr(), self.sij.data_ptr() if distributions else None,
                 self.na.data_ptr() if distributions else None, ctx.stream)
        ctx.comm.allreduce_(self.out)
        vals = self.out.cpu().numpy().copy()
        if ctx.comm.world > 1:   # row 0 from the reduced object rows, in ascending order (:846-863)
            vals[0] = sum_objects(vals[1:])
        return vals.reshape(self.nobj + 1, 4, 3)


def sum_objects(rows: np.ndarray) -> np.ndarray:
    """Row 0 of the result: the object rows added one by one in ascending order onto 0.0."""
    acc = np.zeros(rows.shape[1:])
    for r in rows:
        acc = acc + r
    return acc


class TorqueMonitor:
    """``nekStab_torque(fname, skip)`` as a monitor ``m(v, istep, time)``: every ``skip`` steps one line per
    object in ``path`` (rank 0).  ``pm1``: None (the vector's mesh-2 pressure, interpolated at the face
    points) or a callable ``pm1(v)`` returning a mesh-1 pressure of n_v values.  The other arguments are
    :meth:`Torque.compute`'s."""

    def __init__(self, ctx: NekContext, torque: Torque, path="lift_drag.dat", skip: int = 1, visc=1.0,
                 x0=(0.0, 0.0, 0.0), scale: float = 2.0, dp_mean=(0.0, 0.0, 0.0), pm1=None):
        if skip < 1:
            raise ValueError(f"skip={skip} < 1")
        self.ctx, self.torque, self.skip = ctx, torque, int(skip)
        self.visc, self.x0, self.scale, self.dp_mean, self.pm1 = visc, tuple(x0), float(scale), tuple(dp_mean), pm1
        self.fh = open(path, "w") if (path is not None and ctx.comm.rank == 0) else None
        self.records = 0
        self.last = None

    def __call__(self, v: NekVector, istep: int, time: float):
        if istep % self.skip:
            return None
        vals = self.torque.compute(v, self.visc, self.x0, self.scale, self.dp_mean,
                                   None if self.pm1 is None else self.pm1(v))
        self.last = vals
        self.records += 1
        if self.fh is not None:
            for o in range(1, self.torque.nobj + 1):
                self.fh.write(torque_record(istep, time, vals[o], self.ctx.layout.ldim) + "\n")
            self.fh.flush()
        return vals

    def close(self) -> None:
        if self.fh is not None:
            self.fh.close()
            self.fh = None


class StatisticsSchedule:
    """The clock of ``nekStab_avg`` (postproc.f90:554-579, 613, 639-643), host only.  ``advance(time)``
    returns ``(alpha, beta)`` of this call's update or None when the call updates nothing (the first call,
    or dtime = 0 or atime = 0)."""

    def __init__(self, iastep: int = 500):
        if iastep < 1:
            raise ValueError(f"iastep={iastep} < 1")
        self.iastep = int(iastep)
        self.started = False
        self.atime = 0.0
        self.timel = 0.0

    def advance(self, time: float):
        time = float(time)
        if not self.started:          # icalld == 0 (:554-562)
            self.started = True
            self.atime = 0.0
            self.timel = time
        dtime = time - self.timel
        self.atime = self.atime + dtime
        self.timel = time             # :643 (nothing between reads it)
        if self.atime != 0.0 and dtime != 0.0:
            beta = dtime / self.atime
            return 1.0 - beta, beta
        return None

    def due(self, istep: int, last: bool = False) -> bool:
        """:613: ``(mod(istep, iastep) == 0 .and. istep > 1) .or. lastep == 1``."""
        return (istep % self.iastep == 0 and istep > 1) or bool(last)

    def dump(self, istep: int, last: bool = False) -> float:
        """The file time of a dump (atime, :616) and the reset of :639 (the next update has beta = 1).
        Refused at istep <= 1 unless ``last``, as :613 never dumps there."""
        if not (last or istep > 1):
            raise ValueError(f"nekStab_avg dumps at istep > 1 or at the last step (istep={istep})")
        t, self.atime = self.atime, 0.0
        return t


class Statistics:
    """``nekStab_avg(ifstatis)`` on the device as a monitor ``m(v, istep, time)``.

    Every call advances the reference's clock (:class:`StatisticsSchedule`), updates ``avg`` (and ``rms``,
    and with ``cross`` the moments uv[, vw, wu]) in one launch, and dumps on the reference's condition.  A
    dump writes, with the file time = atime and 64-bit fields, ``avt`` (avg - base, when ``base`` is
    given), ``avg``, ``rms`` and ``rm2`` (the cross moments as the velocity; zeros without ``cross``, as
    the reference writes) and resets atime; the accumulators are kept.  ``avg`` and ``rms`` are
    :class:`NekVector`\\ s.  ``ifpo`` / ``ifto``: write the pressure / scalar statistics when the layout
    stores them (the reference clears both flags before its dumps, :621)."""

    def __init__(self, ctx: NekContext, base: NekVector | None = None, ifstatis: bool = True, cross: bool = False,
                 iastep: int = 500, outdir: str = ".", session: str = "nek", ifpo: bool = True, ifto: bool = True):
        from .fixedp import _refuse_pair

        _refuse_pair(ctx, "Statistics")
        if cross and not ifstatis:
            raise ValueError("cross moments belong to the ifstatis block")
        lay = ctx.layout
        self.ctx, self.base, self.ifstatis, self.outdir, self.session = ctx, base, bool(ifstatis), outdir, session
        self.ifpo, self.ifto = bool(ifpo), bool(ifto)
        self.clock = StatisticsSchedule(iastep)
        self.avg = ctx.vector()
        self.rms = ctx.vector() if ifstatis else None
        self.ncross = (3 if lay.ldim == 3 else 1) if cross else 0
        self.cross = (torch.zeros(max(self.ncross * lay.sv, 2), dtype=torch.float64, device=ctx.device)
                      if cross else None)
        self._tmp = None
        self.updates = 0
        self.dumps = 0

    def update(self, v: NekVector, alpha: float, beta: float) -> None:
        ctx = self.ctx
        ctx.call("nkv_avg_step", v.ptr, self.avg.ptr, self.rms.ptr if self.rms is not None else None,
                 self.cross.data_ptr() if self.cross is not None else None, self.ncross, float(alpha), float(beta),
                 ctx.stream)
        self.updates += 1

    def __call__(self, v: NekVector, istep: int, time: float, last: bool = False):
        ab = self.clock.advance(time)
        if ab is not None:
            self.update(v, *ab)
        if self.clock.due(istep, last):
            return self.dump(istep)
        return None

    # ---- the four files ----
    def _file(self, vec_host, vel_rows, istep: int):
        lay = self.ctx.layout
        e0, e1 = lay.elem_range()
        f = fld.FldFile(lay.lx1, lay.lx1, lay.lx1 if lay.ldim == 3 else 1, lay.nelgv, float(self._file_time),
                        int(istep), lay.rank, lay.world, "U", np.arange(e0 + 1, e1 + 1, dtype=np.int32), {})
        for k, nm in enumerate(("vx", "vy", "vz")[: lay.ldim]):
            a = vel_rows[k] if k < len(vel_rows) else np.zeros(lay.n_v)
            f.fields[nm] = np.asarray(a[: lay.n_v]).reshape(lay.nelv, lay.pts_v)
        if vec_host is None:
            return f
        if self.ifpo and lay.n_p:
            s = lay.n_wf * lay.sv
            f.fields["pr"] = fld.map_pressure_to_mesh1(vec_host[s: s + lay.n_p].reshape(lay.nelv, lay.pts_p),
                                                       lay.lx1, lay.lx2, lay.ldim)
            f.rdcode += "P"
        if self.ifto:
            for sc in range(lay.n_scalars):
                k = lay.ldim + sc
                f.fields["t" if sc == 0 else f"s{sc:02d}"] = vec_host[k * lay.sv: k * lay.sv + lay.n_v].reshape(
                    lay.nelv, lay.pts_v).copy()
                f.rdcode += "T" if sc == 0 else f"S{sc:02d}"
        return f

    def _velocity(self, host):
        lay = self.ctx.layout
        return [host[k * lay.sv: k * lay.sv + lay.n_v] for k in range(lay.ldim)]

    def dump(self, istep: int = 0, last: bool = False) -> list:
        """Write the files of :613-640 and reset atime.  Refused at istep <= 1 unless ``last``."""
        ctx, lay = self.ctx, self.ctx.layout
        self._file_time = self.clock.dump(istep, last)
        self.dumps += 1
        num = self.dumps
        files = []
        if self.base is not None:
            if self._tmp is None:
                self._tmp = ctx.vector()
            k_sub3(self._tmp, self.avg, self.base)            # opsub3 (:622), every stored row
            h = self._tmp.to_packed()
            files.append(("avt", self._file(h, self._velocity(h), istep)))
        h = self.avg.to_packed()
        files.append(("avg", self._file(h, self._velocity(h), istep)))
        hr = self.rms.to_packed() if self.rms is not None else np.zeros(lay.ld)
        files.append(("rms", self._file(hr, self._velocity(hr), istep)))
        if self.cross is not None:
            c = self.cross.cpu().numpy()
            cr = [c[m * lay.sv: m * lay.sv + lay.n_v] for m in range(self.ncross)]
        else:
            cr = []
        files.append(("rm2", self._file(hr, cr, istep)))      # outpost(uvms, vwms, wums, prms, trms) (:627)
        paths = []
        with fld.collective_output(ctx.comm) as write:
            write(os.makedirs, self.outdir, exist_ok=True)
            for prefix, f in files:
                path = os.path.join(self.outdir, fld.fld_name(prefix, self.session, lay.rank, num))
                write(fld.write_fld, path, f)
                paths.append(path)
        return paths


__all__ = ["FACES", "face_points", "wall_faces", "torque_record", "Torque", "TorqueMonitor", "sum_objects",
           "StatisticsSchedule", "Statistics"]
