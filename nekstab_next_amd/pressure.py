"""The divergence-free projection of a velocity on the GLL mesh: the pressure solve of an incompressible flow
on the P_N–P_{N−2} pair, by conjugate gradients on the device.

Reference: Nek5000's ``opdiv`` / ``opgradt`` / ``cdabdtp`` (navier1.f), the operators behind the pressure ``pr``
that nekStab's state vector carries on the ``lx2`` mesh.  In the notation of :mod:`~nekstab_next_amd.advdiff`
(``bm1``, ``minv = mask / dsavg(bm1)``, ``Π``), with ``D`` the weak divergence onto the ``lx2 = lx1 − 2``
Gauss–Legendre points of every element (``nkv_pressure_div``) and ``Dᵀ`` its transpose (``nkv_pressure_gradt``,
include/nekkrylov.h):

    E φ = D( minv · dsavg( Dᵀ φ ) )                          (Nek's cdabdtp: D B⁻¹ Dᵀ)
    P v = v − minv · dsavg( Dᵀ E⁺ D v )                      (velocity rows of a continuous, masked field)

``P Π`` is the ``bm1``-orthogonal projector onto ``{v continuous, masked, D v = 0}``.  Scalars, pressure and
time of a state vector are not touched.

On a closed domain (every boundary point masked) the constant is a null vector of ``E`` — exactly in 2-D,
only nearly on a deformed 3-D mesh, where plain CG is hopeless — and a right-hand side that is rounding noise
(the divergence of a field that is already solenoidal) is inconsistent along it.  One rule handles both: solve
on the mean-free pressures, ``Ẽ = Z E Z`` with ``Z = I − 11ᵀ/n`` over all ranks, ``b = Z D v``; ``P`` is then
the orthogonal projector onto ``ker(Z D)``.  ``closed="auto"`` compares the Rayleigh quotient of the constant
with that of a fixed mean-free vector (closed below 1e-6 of it).

One CG iteration is three launches and one ``dsavg`` batch of ``ldim`` segments: ``nkv_pressure_gradt`` forms
``p = r + βp`` on its load, ``nkv_pressure_div`` applies ``minv`` and emits the partials of ``pᵀEp``, ``ΣEp`` and
``Σp``, ``nkv_pressure_cg_update`` forms ``α``, updates ``x`` and ``r`` and emits the partials of ``rᵀr``.
``α`` and ``β`` never leave the device; the host reads one scalar every ``check_every`` iterations.  The
reductions run in a fixed order without atomics: the same input gives the same bits.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .advdiff import AdvectionDiffusion
from .fld import gauss_points, gll_points, interp_matrix
from .gs import average_segments
from .layout import PairLayout
from .vector import NekContext, NekVector

CLOSED_RATIO = 1e-6


class DivergenceFreeProjector:
    """``P`` on the velocity rows (module docstring).

    ``coords``, ``mask``, ``face_average``: as for :class:`AdvectionDiffusion`; or pass ``operator=`` (an
    :class:`AdvectionDiffusion` on ``ctx``) to share its mesh, ``minv`` and ``face_average``.  ``tol``: CG stops at
    ``‖r‖ ≤ tol·‖b‖``, tested every ``check_every`` iterations; more than ``maxiter`` iterations (default
    ``2·npz_global + 20``) raise ``RuntimeError``.  ``closed``: ``"auto"``, True or False.

    ``apply(x, y)`` projects the velocity rows of a state vector; ``last_iterations`` is the count of the latest
    solve and ``phi`` its multiplier (this rank's ``nel·lx2^ldim`` values)."""

    def __init__(self, ctx: NekContext, coords: dict | None = None, mask=None, face_average="auto", tol: float = 1e-12,
                 maxiter: int | None = None, check_every: int = 8, closed="auto", operator: AdvectionDiffusion | None = None):
        lay = ctx.layout
        if isinstance(lay, PairLayout):
            raise ValueError("DivergenceFreeProjector: a PairLayout context is refused (project the halves of a pair "
                             "vector on the base layout)")
        if lay.lx1 < 3:
            raise ValueError(f"DivergenceFreeProjector: lx1={lay.lx1}: the pressure mesh has lx1 - 2 points per "
                             "direction, lx1 >= 3")
        if not tol > 0.0 or check_every < 1 or (maxiter is not None and maxiter < 1):
            raise ValueError(f"tol={tol}, check_every={check_every}, maxiter={maxiter}: need tol > 0, check_every >= 1, "
                             "maxiter >= 1")
        if closed not in ("auto", True, False):
            raise ValueError("closed: 'auto', True or False")
        if operator is None:
            zero = [np.zeros(lay.n_v) for _ in range(lay.ldim)]
            operator = AdvectionDiffusion(ctx, coords, zero, 0.0, 1.0, 1, mask=mask, face_average=face_average)
        elif operator.ctx is not ctx:
            raise ValueError("DivergenceFreeProjector: operator= must live on ctx")
        self.ctx, self.op = ctx, operator
        self.tol, self.check_every = float(tol), int(check_every)
        d, m = lay.ldim, lay.lx1 - 2
        self.npz = (lay.n_v // lay.lx1 ** d) * m ** d
        f64 = dict(dtype=torch.float64, device=ctx.device)
        self._world = ctx.comm.world
        self._offset = lay.elem_range()[0] * m ** d             # the global index of this rank's first pressure value
        self.npz_global = self.npz
        if self._world > 1:
            cnt = torch.tensor([float(self.npz)], **f64)
            self.npz_global = int(ctx.comm.allreduce_(cnt).item())
        self.maxiter = 2 * self.npz_global + 20 if maxiter is None else int(maxiter)
        self._interp = torch.as_tensor(interp_matrix(gll_points(lay.lx1), gauss_points(m))).to(ctx.device)
        self._gw = torch.as_tensor(np.polynomial.legendre.leggauss(m)[1]).to(ctx.device)
        self._head = (lay.lx1, d, operator.D.data_ptr(), self._interp.data_ptr(), self._gw.data_ptr(),
                      *operator._xyz_ptrs())
        B = self.PARTIALS = _lib.load().nkv_pressure_partials()
        npad = max(self.npz, 2)
        self._x, self._r, self._p, self._Ep = (torch.zeros(npad, **f64) for _ in range(4))
        self._t = torch.zeros(d * lay.sv + 2, **f64)                # D^T p, ldim segments
        self._red = torch.zeros(3 * B, **f64)                        # p.Ep, sum Ep, sum p: one slot per workgroup
        self._rr = [torch.zeros(B, **f64) for _ in range(2)]         # r.r, before and after an update
        self._t_ptrs = [self._t.data_ptr() + 8 * c * lay.sv for c in range(d)]
        self._chk = torch.zeros(1, **f64)                            # the scalar the host reads (allocated once)
        self.phi = self._x[: self.npz]
        self.last_iterations = 0
        self.closed_ratio = None
        self.closed = False
        if closed == "auto":
            self.closed = self._detect_closed()
        else:
            self.closed = bool(closed)

    # ---- the operators ----
    def _gradt(self, p: torch.Tensor, res=None, rr_new=None, rr_old=None, B: int = 1, first: bool = True) -> None:
        """t <- dsavg(D^T p); with ``res``, p <- first ? res : res + beta p on the way."""
        ctx, lay = self.ctx, self.ctx.layout
        ctx.call("nkv_pressure_gradt", *self._head, p.data_ptr(), None if res is None else res.data_ptr(),
                 None if rr_new is None else rr_new.data_ptr(), None if rr_old is None else rr_old.data_ptr(), B,
                 int(first), self._t.data_ptr(), lay.sv, ctx.stream)
        average_segments(self.op.face_average, self._t_ptrs)

    def _div(self, u_ptr: int, mult, out: torch.Tensor, pv=None) -> None:
        ctx, lay = self.ctx, self.ctx.layout
        ctx.call("nkv_pressure_div", *self._head, u_ptr, lay.sv, None if mult is None else mult.data_ptr(),
                 out.data_ptr(), None if pv is None else pv.data_ptr(), None if pv is None else self._red.data_ptr(),
                 ctx.stream)

    def _reduced(self, part: torch.Tensor, rows: int):
        """The partials a consumer kernel sums: as they are on one rank; summed here and all-reduced on several."""
        if self._world == 1:
            return part, self.PARTIALS
        s = part.view(rows, self.PARTIALS).sum(dim=1)
        self.ctx.comm.allreduce_(s)
        return s, 1

    def _host_sum(self, part: torch.Tensor) -> float:
        """The one scalar the host reads: the sum of the partials of r.r (no allocation on the device)."""
        torch.sum(part, dim=0, keepdim=True, out=self._chk)
        return float(self._chk.item())

    def apply_E(self, phi: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """``out = E phi`` on this rank's pressure values (collective through ``dsavg``); no deflation."""
        self._gradt(phi)
        self._div(self._t.data_ptr(), self.op._minv, out)
        return out

    def _detect_closed(self) -> bool:
        n, f64 = self.npz, dict(dtype=torch.float64, device=self.ctx.device)
        k = torch.arange(self._offset, self._offset + n, **f64)
        z = torch.zeros(max(n, 2), **f64)
        z[:n] = torch.cos(1.0 + 2.399963 * k)
        s = torch.zeros(1, **f64)
        s[0] = z[:n].sum()
        self.ctx.comm.allreduce_(s)
        z[:n] -= s[0] / self.npz_global
        one = torch.zeros(max(n, 2), **f64)
        one[:n] = 1.0
        q = torch.zeros(4, **f64)
        Ev = torch.zeros(max(n, 2), **f64)
        for i, v in enumerate((one, z)):
            self.apply_E(v, Ev)
            q[2 * i] = torch.dot(v[:n], Ev[:n])
            q[2 * i + 1] = torch.dot(v[:n], v[:n])
        self.ctx.comm.allreduce_(q)
        q1, d1, qz, dz = (float(a) for a in q.cpu())
        self.closed_ratio = (q1 / d1) / (qz / dz)
        return self.closed_ratio < CLOSED_RATIO

    # ---- the solve ----
    def _update(self, red, Br: int, rr_old, Bo: int, rr_out: torch.Tensor, init: bool) -> None:
        self.ctx.call_nl("nkv_pressure_cg_update", self.npz, self._x.data_ptr(), self._r.data_ptr(), self._p.data_ptr(),
                         self._Ep.data_ptr(), None if red is None else red.data_ptr(), Br,
                         None if rr_old is None else rr_old.data_ptr(), Bo, 1.0 / max(self.npz_global, 1),
                         int(self.closed), int(init), rr_out.data_ptr(), self.ctx.stream)

    def project_ptr(self, v_ptr: int, out_ptr: int | None = None) -> None:
        """``P`` on the ``ldim`` segments (stride ``sv``) at ``v_ptr``, into ``out_ptr`` (default: in place)."""
        ctx, lay = self.ctx, self.ctx.layout
        out_ptr = v_ptr if out_ptr is None else out_ptr
        minv = self.op._minv
        # b = Z D v; x = 0, r = b
        self._div(v_ptr, None, self._Ep, pv=self._p)
        red, Br = self._reduced(self._red, 3)
        self._update(red, Br, None, 1, self._rr[0], init=True)
        rr, Bo = self._reduced(self._rr[0], 1)
        bb = self._host_sum(rr)
        it = 0
        if bb > 0.0 and math.isfinite(bb):
            stop = (self.tol ** 2) * bb
            rr_prev, done = None, False
            while not done:
                if it >= self.maxiter:
                    self.last_iterations = it
                    raise RuntimeError(f"DivergenceFreeProjector: CG did not reach tol={self.tol:g} in maxiter={self.maxiter} "
                                       f"iterations (|r|/|b| = {math.sqrt(max(self._host_sum(rr), 0.0) / bb):.3e})")
                self._gradt(self._p, res=self._r, rr_new=rr, rr_old=rr_prev, B=Bo, first=(it == 0))
                self._div(self._t.data_ptr(), minv, self._Ep, pv=self._p)
                red, Br = self._reduced(self._red, 3)
                out = self._rr[(it + 1) % 2]
                self._update(red, Br, rr, Bo, out, init=False)
                rr_prev = rr
                rr, Bo = self._reduced(out, 1)
                it += 1
                if it % self.check_every == 0:
                    now = self._host_sum(rr)
                    if not math.isfinite(now):
                        raise RuntimeError("DivergenceFreeProjector: the CG residual is not finite")
                    done = now <= stop
        elif not math.isfinite(bb):
            raise RuntimeError("DivergenceFreeProjector: the divergence of the input is not finite")
        self.last_iterations = it
        # out = v - minv dsavg(D^T x)   (x = 0 when b = 0: out = v)
        self._gradt(self._x)
        ctx.call("nkv_advdiff_stage", v_ptr, lay.sv, minv.data_ptr(), self._t.data_ptr(), lay.sv, -1.0, out_ptr, lay.sv,
                 lay.ldim, 0, ctx.stream)

    def apply(self, x: NekVector, y: NekVector | None = None) -> NekVector:
        """``y = x`` with its velocity rows projected (in place when ``y`` is None); every other row is copied."""
        if y is not None and y is not x:
            y.copy_from(x)
        tgt = x if y is None else y
        self.project_ptr(tgt.ptr)
        return tgt

    def divergence(self, x: NekVector) -> torch.Tensor:
        """``Z D v`` of the velocity rows of ``x`` (this rank's values; a new tensor)."""
        out = torch.zeros(max(self.npz, 2), dtype=torch.float64, device=self.ctx.device)
        self._div(x.ptr, None, out)
        out = out[: self.npz]
        if self.closed:
            s = out.sum().reshape(1)
            self.ctx.comm.allreduce_(s)
            out = out - s[0] / self.npz_global
        return out


__all__ = ["DivergenceFreeProjector"]
