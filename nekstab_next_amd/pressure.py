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

``project_pair_ptr`` solves two systems on the mesh at once, the re and the im half of a pair vector (a resolvent
stage): the same iteration over ``nkv_pressure_gradt2``, ``nkv_pressure_div2`` and ``nkv_pressure_cg_update2``, which
stage the coordinates and form the factors once for both, one ``dsavg`` batch of ``2·ldim`` segments and one
all-reduce per reduced quantity.  Every system keeps its own scalars and its own stop; one that has met it is
frozen (dropped from the ``active`` mask of every later launch), so each result carries the bits and the iteration
count of ``project_ptr`` on it alone.

``preconditioner="fdm"`` runs the same solve as preconditioned CG with a non-overlapping element-block
preconditioner applied by fast diagonalisation (the local solve of Nek5000's Schwarz smoother without overlap or
coarse grid).  For ``n = lx1`` take the GLL weights ``ρ`` and derivative ``D̂``, the ``m = lx1 − 2`` Gauss weights ``w``
and the interpolation ``I`` (m × n); with ``ρ̃ = ρ``, its two end weights doubled (the mass an interior interface sees
after assembly), ``D̃ = diag(w) I D̂`` and ``J̃ = diag(w) I``:

    Â = D̃ diag(1/ρ̃) D̃ᵀ,   B̂ = J̃ diag(1/ρ̃) J̃ᵀ,   Â S = B̂ S Λ,   Sᵀ B̂ S = I        (``fdm_eigenpairs``)

Per element ``e`` and local direction ``d``, ``h[e,d]`` is half the distance between the centroids of the two opposite
faces and ``c[e,d] = (Π_k h[e,k]) / h[e,d]²`` (``fdm_element_scales``).  Then, with ``i_1`` along r,

    M_e = (S ⊗ … ⊗ S) · diag( 1 / Σ_d c[e,d] λ_{i_d} ) · (Sᵀ ⊗ … ⊗ Sᵀ)              (``nkv_pressure_precond``)

is the exact inverse of ``Σ_d c[e,d] (Â in slot d, B̂ elsewhere)`` on an undeformed rectilinear element, and
``M = blockdiag(M_e)`` is symmetric positive definite and element-local.  The iteration is

    z = Z M r,   p = z + (r·z / r·z_prev) p,   α = r·z / p·(Z E p)

with the stop rule, ``maxiter`` and the errors of the plain iteration (``‖r‖₂ ≤ tol·‖b‖₂`` every ``check_every``
iterations).  It is four launches: ``nkv_pressure_pgradt`` (``nkv_pressure_gradt`` that also takes the mean off ``z``
on its load), ``nkv_pressure_div``, ``nkv_pressure_cg_update`` (given the partials of ``r·z`` where the plain
iteration gives those of ``r·r``; it still emits ``r·r`` for the stop) and ``nkv_pressure_precond``, which emits the
partials of ``r·z`` and ``Σz``.  The three partial rows share one buffer, so several ranks reduce them in one
all-reduce.  ``preconditioner=None`` (the default) runs the plain iteration above, unchanged.
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


def fdm_eigenpairs(lx1: int):
    """``(S, lambda)`` of the 1-D reference problem of the fast-diagonalisation preconditioner (module docstring),
    in f64: ``A^ S = B^ S diag(lambda)``, ``S^T B^ S = I``."""
    from scipy.linalg import eigh

    from .sensitivity import gll_derivative
    from .synthetic import gll_weights

    m = lx1 - 2
    rho = np.array(gll_weights(lx1), dtype=np.float64)
    rho[0] *= 2.0                                                    # the mass an interior interface sees
    rho[-1] *= 2.0
    Jt = np.polynomial.legendre.leggauss(m)[1][:, None] * interp_matrix(gll_points(lx1), gauss_points(m))
    Dt = Jt @ gll_derivative(lx1)
    A, B = (Dt / rho) @ Dt.T, (Jt / rho) @ Jt.T
    lam, S = eigh(0.5 * (A + A.T), 0.5 * (B + B.T))
    return np.ascontiguousarray(S), lam


def fdm_element_scales(xyz, lx1: int, ldim: int) -> np.ndarray:
    """``c[e, d] = (prod_k h[e, k]) / h[e, d]^2`` (nel x ldim) from the GLL coordinates ``xyz`` (ldim arrays of
    ``nel·lx1^ldim``): ``h[e, d]`` is half the distance between the centroids of the two faces across ``d``."""
    X = np.stack([np.asarray(x, dtype=np.float64).reshape(-1, lx1 if ldim == 3 else 1, lx1, lx1) for x in xyz])
    h = []
    for d in range(ldim):
        lo, hi = (np.take(X, i, axis=4 - d) for i in (0, lx1 - 1))     # r is the last axis of (comp, e, k, j, i)
        lo, hi = (f.reshape(ldim, f.shape[1], -1).mean(axis=2) for f in (lo, hi))
        h.append(0.5 * np.sqrt(np.sum((hi - lo) ** 2, axis=0)))
    h = np.stack(h, axis=1)
    return np.ascontiguousarray(np.prod(h, axis=1, keepdims=True) / h ** 2)


class DivergenceFreeProjector:
    """``P`` on the velocity rows (module docstring).

    ``coords``, ``mask``, ``face_average``: as for :class:`AdvectionDiffusion`; or pass ``operator=`` (an
    :class:`AdvectionDiffusion` on ``ctx``) to share its mesh, ``minv`` and ``face_average``.  ``tol``: CG stops at
    ``‖r‖ ≤ tol·‖b‖``, tested every ``check_every`` iterations; more than ``maxiter`` iterations (default
    ``2·npz_global + 20``) raise ``RuntimeError``.  ``closed``: ``"auto"``, True or False.  ``preconditioner``: None
    (plain CG) or ``"fdm"`` (module docstring); with ``"fdm"``, ``precondition(r, out)`` applies ``M`` and ``fdm_S``,
    ``fdm_lambda``, ``fdm_c`` hold its data on the device.

    ``apply(x, y)`` projects the velocity rows of a state vector; ``last_iterations`` is the count of the latest
    solve and ``phi`` its multiplier (this rank's ``nel·lx2^ldim`` values).  ``project_pair_ptr`` projects two
    velocities in one CG loop; ``last_iterations_each`` holds its two counts and ``last_iterations`` their maximum
    (``phi`` stays the latest single solve's)."""

    def __init__(self, ctx: NekContext, coords: dict | None = None, mask=None, face_average="auto", tol: float = 1e-12,
                 maxiter: int | None = None, check_every: int = 8, closed="auto", operator: AdvectionDiffusion | None = None,
                 preconditioner: str | None = None):
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
        if preconditioner not in (None, "fdm"):
            raise ValueError(f"preconditioner={preconditioner!r}: None or 'fdm'")
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
        self.last_iterations_each = (0, 0)                           # of the latest two-system solve
        self._pair = None                                            # the buffers of project_pair_ptr
        self.preconditioner = preconditioner
        self.fdm_S = self.fdm_lambda = self.fdm_c = None
        if preconditioner == "fdm":
            self._build_fdm()
        self.closed_ratio = None
        self.closed = False
        if closed == "auto":
            self.closed = self._detect_closed()
        else:
            self.closed = bool(closed)

    # ---- the preconditioner ----
    def _build_fdm(self) -> None:
        """``S``, ``lambda`` (the same on every rank) and the scales ``c`` of this rank's elements, on the device;
        ``z`` and the two partial buffers of the preconditioned iteration: rows r.r, r.z, sum z."""
        ctx, lay, B = self.ctx, self.ctx.layout, self.PARTIALS
        f64 = dict(dtype=torch.float64, device=ctx.device)
        S, lam = fdm_eigenpairs(lay.lx1)
        c = fdm_element_scales([x[: lay.n_v].cpu().numpy() for x in self.op.xyz], lay.lx1, lay.ldim)
        self.fdm_S, self.fdm_lambda = torch.as_tensor(S).to(ctx.device), torch.as_tensor(lam).to(ctx.device)
        self.fdm_c = torch.zeros(max(c.shape[0], 1), lay.ldim, **f64)
        self.fdm_c[: c.shape[0]] = torch.as_tensor(c).to(ctx.device)
        self._nel = c.shape[0]
        self._z = torch.zeros(max(self.npz, 2), **f64)
        self._pz = [torch.zeros(3 * B, **f64) for _ in range(2)]
        self._fdm_head = (self._nel, lay.lx1, lay.ldim, self.fdm_S.data_ptr(), self.fdm_lambda.data_ptr(),
                          self.fdm_c.data_ptr())

    def precondition(self, r: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """``out = M r`` on this rank's pressure values (element-local: no communication, no deflation)."""
        if self.preconditioner != "fdm":
            raise RuntimeError("DivergenceFreeProjector.precondition: built with preconditioner=None")
        for t, name in ((r, "r"), (out, "out")):
            if t.dtype != torch.float64 or t.device != self._z.device or not t.is_contiguous() or t.numel() < self.npz:
                raise ValueError(f"precondition: {name} must be a contiguous f64 tensor of at least {self.npz} values "
                                 "on the projector's device")
        self.ctx.call_nl("nkv_pressure_precond", *self._fdm_head, r.data_ptr(), out.data_ptr(), None, self.ctx.stream)
        return out

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
        if self.preconditioner == "fdm":
            return self._project_ptr_fdm(v_ptr, out_ptr)
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

    def _project_ptr_fdm(self, v_ptr: int, out_ptr: int | None) -> None:
        """``project_ptr`` by preconditioned CG: ``z = Z M r``, ``p = z + (r.z / r.z_prev) p``, ``alpha = r.z /
        p.(Z E p)``; the stop rule, ``maxiter`` and the errors of the plain iteration.  Four launches an iteration:
        ``nkv_pressure_pgradt`` (takes the mean off ``z`` on its load), ``nkv_pressure_div``,
        ``nkv_pressure_cg_update`` (``r.z`` for ``r.r`` in ``alpha``; it still emits ``r.r``) and
        ``nkv_pressure_precond``.  The partials of ``r.r``, ``r.z`` and ``sum z`` share one buffer and one
        all-reduce."""
        ctx, lay, PB = self.ctx, self.ctx.layout, self.PARTIALS
        out_ptr = v_ptr if out_ptr is None else out_ptr
        minv, st = self.op._minv, ctx.stream
        inv_n, closed = 1.0 / max(self.npz_global, 1), int(self.closed)
        x, r, p, Ep, z = (a.data_ptr() for a in (self._x, self._r, self._p, self._Ep, self._z))

        def update_precond(red, Br, rz_ptr, Bo, buf, init):
            ctx.call_nl("nkv_pressure_cg_update", self.npz, x, r, p, Ep, None if red is None else red.data_ptr(), Br,
                        rz_ptr, Bo, inv_n, closed, int(init), buf.data_ptr(), st)
            ctx.call_nl("nkv_pressure_precond", *self._fdm_head, r, z, buf.data_ptr() + 8 * PB, st)
            return self._reduced(buf, 3)                             # rows r.r, r.z, sum z: Bo values each

        # b = Z D v; x = 0, r = b, z = M r
        self._div(v_ptr, None, self._Ep, pv=self._p)
        red, Br = self._reduced(self._red, 3)
        cur, Bo = update_precond(red, Br, None, 1, self._pz[0], True)
        bb = self._host_sum(cur[:Bo])
        it = 0
        if bb > 0.0 and math.isfinite(bb):
            stop = (self.tol ** 2) * bb
            prev, done = None, False
            while not done:
                if it >= self.maxiter:
                    self.last_iterations = it
                    raise RuntimeError(f"DivergenceFreeProjector: CG did not reach tol={self.tol:g} in maxiter={self.maxiter} "
                                       f"iterations (|r|/|b| = {math.sqrt(max(self._host_sum(cur[:Bo]), 0.0) / bb):.3e})")
                ctx.call("nkv_pressure_pgradt", *self._head, p, z, cur.data_ptr() + 8 * Bo,
                         None if prev is None else prev.data_ptr() + 8 * Bo,
                         cur.data_ptr() + 16 * Bo if closed else None, Bo, inv_n, int(it == 0), self._t.data_ptr(), lay.sv,
                         st)
                average_segments(self.op.face_average, self._t_ptrs)
                self._div(self._t.data_ptr(), minv, self._Ep, pv=self._p)
                red, Br = self._reduced(self._red, 3)
                prev = cur
                cur, Bo = update_precond(red, Br, cur.data_ptr() + 8 * Bo, Bo, self._pz[(it + 1) % 2], False)
                it += 1
                if it % self.check_every == 0:
                    now = self._host_sum(cur[:Bo])
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

    # ---- the solve of two systems at once ----
    def _pair_buffers(self):
        """The second set of CG vectors, allocated on first use: x, r, p, Ep, D^T p and the partial rows of both
        systems (system 0's too: the two-system entries take the rows of both from one buffer)."""
        if self._pair is None:
            lay, B = self.ctx.layout, self.PARTIALS
            f64 = dict(dtype=torch.float64, device=self.ctx.device)
            npad = max(self.npz, 2)
            x, r, p, Ep = (torch.zeros(2, npad, **f64) for _ in range(4))
            t = torch.zeros(2 * lay.ldim * lay.sv + 2, **f64)        # system s, component c at (s ldim + c) sv
            red = torch.zeros(2 * 3 * B, **f64)
            rr = [torch.zeros(2 * B, **f64) for _ in range(2)]
            t_ptrs = [t.data_ptr() + 8 * k * lay.sv for k in range(2 * lay.ldim)]
            t_sets = {1: t_ptrs[: lay.ldim], 2: t_ptrs[lay.ldim:], 3: t_ptrs}   # by ``active``
            self._pair = dict(x=x, r=r, p=p, Ep=Ep, t=t, red=red, rr=rr, t_sets=t_sets, chk=torch.zeros(2, **f64))
            if self.preconditioner == "fdm":     # z, and the rows r.r, r.z, sum z of both systems (system s: row 2q + s)
                self._pair.update(z=torch.zeros(2, npad, **f64), pz=[torch.zeros(6 * B, **f64) for _ in range(2)])
        return self._pair

    def _reduced2(self, part: torch.Tensor, rows: int):
        """``_reduced`` for the rows of both systems: one all-reduce covers them."""
        if self._world == 1:
            return part, self.PARTIALS
        s = part.view(2 * rows, self.PARTIALS).sum(dim=1)
        self.ctx.comm.allreduce_(s)
        return s, 1

    def _host_sums2(self, part: torch.Tensor, B: int):
        """The two scalars the host reads in one copy: the sums of both systems' partials of r.r."""
        w = self._pair["chk"]
        torch.sum(part.view(2, B), dim=1, out=w)
        a, b = w.tolist()
        return [a, b]

    def project_pair_ptr(self, v0_ptr: int, v1_ptr: int, stride: int, out0_ptr: int | None = None,
                         out1_ptr: int | None = None) -> None:
        """``P`` on the ``ldim`` segments at ``v0_ptr`` and on those at ``v1_ptr`` (stride ``stride`` doubles,
        ``n_v`` points of the base layout each: the halves of a pair vector), into ``out0_ptr`` / ``out1_ptr``
        (default: in place).  One CG loop over the two-system entries (``nkv_pressure_div2``, ``_gradt2``,
        ``_cg_update2``): one ``dsavg`` batch of ``2·ldim`` segments and one all-reduce per reduced quantity and
        iteration, both residuals read together every ``check_every`` iterations.  Each system has its own ``‖b‖``
        and stop; one that meets it at a check (or has ``b = 0``) is frozen, its bit cleared from ``active`` for
        every later launch, so each result is bit for bit ``project_ptr``'s for it alone on one rank, with the same
        count (``last_iterations_each``; ``last_iterations`` is their maximum)."""
        if self.preconditioner == "fdm":
            return self._project_pair_ptr_fdm(v0_ptr, v1_ptr, stride, out0_ptr, out1_ptr)
        ctx, lay = self.ctx, self.ctx.layout
        out0_ptr = v0_ptr if out0_ptr is None else out0_ptr
        out1_ptr = v1_ptr if out1_ptr is None else out1_ptr
        w, minv, d, sv, st = self._pair_buffers(), self.op._minv, lay.ldim, lay.sv, ctx.stream
        x, r, p, Ep = ([a[0].data_ptr(), a[1].data_ptr()] for a in (w["x"], w["r"], w["p"], w["Ep"]))
        tp = [w["t"].data_ptr(), w["t"].data_ptr() + 8 * d * sv]
        redp = w["red"].data_ptr()
        inv_n, closed = 1.0 / max(self.npz_global, 1), int(self.closed)

        def div2(u0, u1, ustride, mult, active):
            ctx.call("nkv_pressure_div2", *self._head, u0, u1, ustride, mult, *Ep, *p, redp, active, st)

        def gradt2(src, res, rr_new, rr_old, B, first, active):
            ctx.call("nkv_pressure_gradt2", *self._head, *src, *res, rr_new, rr_old, B, int(first), *tp, sv, active, st)
            average_segments(self.op.face_average, w["t_sets"][active])

        def update2(red, Br, rr_old, Bo, rr_out, init, active):
            ctx.call_nl("nkv_pressure_cg_update2", self.npz, *x, *r, *p, *Ep, None if red is None else red.data_ptr(),
                        Br, None if rr_old is None else rr_old.data_ptr(), Bo, inv_n, closed, int(init),
                        rr_out.data_ptr(), active, st)

        # b = Z D v; x = 0, r = b
        div2(v0_ptr, v1_ptr, stride, None, 3)
        red, Br = self._reduced2(w["red"], 3)
        update2(red, Br, None, 1, w["rr"][0], True, 3)
        rr, Bo = self._reduced2(w["rr"][0], 1)
        bb = self._host_sums2(rr, Bo)
        if not all(math.isfinite(b) for b in bb):
            raise RuntimeError("DivergenceFreeProjector: the divergence of the input is not finite")
        stop = [(self.tol ** 2) * b for b in bb]
        its = [0, 0]
        active = sum(1 << s for s in range(2) if bb[s] > 0.0)
        it, rr_prev = 0, None
        while active:
            if it >= self.maxiter:
                self.last_iterations_each, self.last_iterations = tuple(its), max(its)
                now = self._host_sums2(rr, Bo)
                rel = max(math.sqrt(max(now[s], 0.0) / bb[s]) for s in range(2) if active >> s & 1)
                raise RuntimeError(f"DivergenceFreeProjector: CG did not reach tol={self.tol:g} in maxiter={self.maxiter} "
                                   f"iterations (|r|/|b| = {rel:.3e})")
            gradt2(p, r, rr.data_ptr(), None if rr_prev is None else rr_prev.data_ptr(), Bo, it == 0, active)
            div2(*tp, sv, minv.data_ptr(), active)
            red, Br = self._reduced2(w["red"], 3)
            out = w["rr"][(it + 1) % 2]
            update2(red, Br, rr, Bo, out, False, active)
            rr_prev = rr
            rr, Bo = self._reduced2(out, 1)
            it += 1
            for s in range(2):
                if active >> s & 1:
                    its[s] = it
            if it % self.check_every == 0:
                now = self._host_sums2(rr, Bo)
                for s in range(2):
                    if not active >> s & 1:
                        continue
                    if not math.isfinite(now[s]):
                        raise RuntimeError("DivergenceFreeProjector: the CG residual is not finite")
                    if now[s] <= stop[s]:
                        active &= ~(1 << s)
        self.last_iterations_each, self.last_iterations = tuple(its), max(its)
        # out = v - minv dsavg(D^T x)   (x = 0 when b = 0: out = v)
        gradt2(x, (None, None), None, None, 1, True, 3)
        for v_ptr, t_ptr, o_ptr in ((v0_ptr, tp[0], out0_ptr), (v1_ptr, tp[1], out1_ptr)):
            ctx.call("nkv_advdiff_stage", v_ptr, stride, minv.data_ptr(), t_ptr, sv, -1.0, o_ptr, stride, d, 0, st)

    def _project_pair_ptr_fdm(self, v0_ptr: int, v1_ptr: int, stride: int, out0_ptr: int | None,
                              out1_ptr: int | None) -> None:
        """``project_pair_ptr`` by the preconditioned iteration of ``_project_ptr_fdm`` over the two-system entries
        (``nkv_pressure_pgradt2``, ``_div2``, ``_cg_update2``, ``_precond2``): each system carries the bits and the
        count of the single-system preconditioned solve."""
        ctx, lay, PB = self.ctx, self.ctx.layout, self.PARTIALS
        out0_ptr = v0_ptr if out0_ptr is None else out0_ptr
        out1_ptr = v1_ptr if out1_ptr is None else out1_ptr
        w, minv, d, sv, st = self._pair_buffers(), self.op._minv, lay.ldim, lay.sv, ctx.stream
        x, r, p, Ep, z = ([a[0].data_ptr(), a[1].data_ptr()] for a in (w["x"], w["r"], w["p"], w["Ep"], w["z"]))
        tp = [w["t"].data_ptr(), w["t"].data_ptr() + 8 * d * sv]
        redp = w["red"].data_ptr()
        inv_n, closed = 1.0 / max(self.npz_global, 1), int(self.closed)

        def div2(u0, u1, ustride, mult, active):
            ctx.call("nkv_pressure_div2", *self._head, u0, u1, ustride, mult, *Ep, *p, redp, active, st)

        def update_precond2(red, Br, rz_ptr, Bo, buf, init, active):
            ctx.call_nl("nkv_pressure_cg_update2", self.npz, *x, *r, *p, *Ep, None if red is None else red.data_ptr(),
                        Br, rz_ptr, Bo, inv_n, closed, int(init), buf.data_ptr(), active, st)
            ctx.call_nl("nkv_pressure_precond2", *self._fdm_head, *r, *z, buf.data_ptr() + 8 * 2 * PB, active, st)
            return self._reduced2(buf, 3)                            # rows r.r, r.z, sum z: 2 Bo values each

        # b = Z D v; x = 0, r = b, z = M r
        div2(v0_ptr, v1_ptr, stride, None, 3)
        red, Br = self._reduced2(w["red"], 3)
        cur, Bo = update_precond2(red, Br, None, 1, w["pz"][0], True, 3)
        bb = self._host_sums2(cur[: 2 * Bo], Bo)
        if not all(math.isfinite(b) for b in bb):
            raise RuntimeError("DivergenceFreeProjector: the divergence of the input is not finite")
        stop = [(self.tol ** 2) * b for b in bb]
        its = [0, 0]
        active = sum(1 << s for s in range(2) if bb[s] > 0.0)
        it, prev = 0, None
        while active:
            if it >= self.maxiter:
                self.last_iterations_each, self.last_iterations = tuple(its), max(its)
                now = self._host_sums2(cur[: 2 * Bo], Bo)
                rel = max(math.sqrt(max(now[s], 0.0) / bb[s]) for s in range(2) if active >> s & 1)
                raise RuntimeError(f"DivergenceFreeProjector: CG did not reach tol={self.tol:g} in maxiter={self.maxiter} "
                                   f"iterations (|r|/|b| = {rel:.3e})")
            ctx.call("nkv_pressure_pgradt2", *self._head, *p, *z, cur.data_ptr() + 8 * 2 * Bo,
                     None if prev is None else prev.data_ptr() + 8 * 2 * Bo,
                     cur.data_ptr() + 8 * 4 * Bo if closed else None, Bo, inv_n, int(it == 0), *tp, sv, active, st)
            average_segments(self.op.face_average, w["t_sets"][active])
            div2(*tp, sv, minv.data_ptr(), active)
            red, Br = self._reduced2(w["red"], 3)
            prev = cur
            cur, Bo = update_precond2(red, Br, cur.data_ptr() + 8 * 2 * Bo, Bo, w["pz"][(it + 1) % 2], False, active)
            it += 1
            for s in range(2):
                if active >> s & 1:
                    its[s] = it
            if it % self.check_every == 0:
                now = self._host_sums2(cur[: 2 * Bo], Bo)
                for s in range(2):
                    if not active >> s & 1:
                        continue
                    if not math.isfinite(now[s]):
                        raise RuntimeError("DivergenceFreeProjector: the CG residual is not finite")
                    if now[s] <= stop[s]:
                        active &= ~(1 << s)
        self.last_iterations_each, self.last_iterations = tuple(its), max(its)
        # out = v - minv dsavg(D^T x)   (x = 0 when b = 0: out = v)
        ctx.call("nkv_pressure_gradt2", *self._head, *x, None, None, None, None, 1, 1, *tp, sv, 3, st)
        average_segments(self.op.face_average, w["t_sets"][3])
        for v_ptr, t_ptr, o_ptr in ((v0_ptr, tp[0], out0_ptr), (v1_ptr, tp[1], out1_ptr)):
            ctx.call("nkv_advdiff_stage", v_ptr, stride, minv.data_ptr(), t_ptr, sv, -1.0, o_ptr, stride, d, 0, st)

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
