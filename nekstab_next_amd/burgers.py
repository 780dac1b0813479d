"""A pressure-free viscous Burgers flow on the GLL mesh, its exact linearisation and its exact discrete
adjoint: the first operator of the package whose base state is itself the solution of a nonlinear problem.

Reference: nekStab's workflow is Newton first, then stability about what Newton found (fixed point at
``uparam(1) = 2``, stability at ``3``, adjoint at ``3.2``; newton_krylov.f90:1-166 and
``newton_linearized_map``, matvec.f90:520-571), all of it a Nek5000 run.  Pressure and incompressibility stay
Nek5000's; here the velocity (the first ``ldim`` weighted fields) advects itself and every
scalar, which is enough to drive ``newton_krylov`` and then ``krylov_schur`` on one mesh.

In the notation of :mod:`~nekstab_next_amd.advdiff` (``bm1``, ``minv = mask / dsavg(bm1)``, ``Π``), with
``r(q; U)`` the forward right-hand side of ``nkv_advdiff_rhs``:

    N(q)    = minv · dsavg(r(q; U = q_vel)) + g                 (g: a constant forcing, already projected)
    L_B u   = minv · dsavg(r_fwd(u; B)),   L_B† u = minv · dsavg(r_adj(u; B))      (nkv_linconv_rhs)
      r_fwd,f = r_advdiff,f(u; U = B_vel)     − bm1 Σ_{d<ldim} u_d ∂_d B_f
      r_adj,f = r_advdiff,adj,f(u; U = B_vel) − [f < ldim] bm1 Σ_{f'<n_wf} u_f' ∂_f B_f'
    Φ(q)    = RK4^nsteps(Π q)              (classical four-stage RK4 of dq/dt = N(q), nkv_rk4_stage)
    matvec:  y = p(dt L_B)^nsteps Π x,     rmatvec:  y = p(dt L_B†)^nsteps Π x     (Horner, as the parent)

At a steady state (``N(q*) = 0``) every RK4 stage equals ``q*``, so the Jacobian of Φ there is exactly
``p(dt L_q*)^nsteps Π``; away from one the frozen-base operator differs from it by O(‖N(q)‖), which is what
``newton_linearized_map`` does for a steady base and keeps Newton quadratic.

A nonlinear step is four stages of one right-hand-side launch, one ``dsavg`` batch and one stage launch;
nothing synchronises with the host and the work vectors are allocated once.
"""
from __future__ import annotations

import numpy as np
import torch

from .advdiff import AdvectionDiffusion
from .vector import NekContext, NekVector


def _base_rows(ctx: NekContext, base, what: str = "base"):
    """The n_wf rows of a base state: a NekVector, or n_wf arrays of n_v values (checked)."""
    lay = ctx.layout
    if isinstance(base, NekVector):
        return base
    if len(base) != lay.n_wf:
        raise ValueError(f"{what}: {len(base)} fields, the layout has n_wf={lay.n_wf} weighted fields")
    rows = [np.asarray(b, dtype=np.float64).ravel() for b in base]
    for f, b in enumerate(rows):
        if b.size != lay.n_v:
            raise ValueError(f"{what}[{f}]: {b.size} points, the layout has n_v={lay.n_v}")
    return rows


class LinearisedConvection(AdvectionDiffusion):
    """``y = p(dt L_B)^nsteps Π x`` and its adjoint about a base state ``B`` of all ``n_wf`` weighted fields
    (module docstring): :class:`AdvectionDiffusion` with the production term ``(u'·∇)B`` and its adjoint
    ``(∇B)ᵀu'``.  ``base``: a :class:`NekVector` (its weighted rows are copied) or ``n_wf`` arrays of n_v
    values; the first ``ldim`` fields advect.  Everything else as in the parent; ``set_base`` replaces the
    base state in place."""

    def __init__(self, ctx: NekContext, coords: dict, base, kappa, dt: float, nsteps: int, mask=None,
                 face_average="auto"):
        lay = ctx.layout
        d, sv, nf = lay.ldim, lay.sv, lay.n_wf
        rows = _base_rows(ctx, base)
        super().__init__(ctx, coords, rows if isinstance(rows, NekVector) else rows[:d], kappa, dt, nsteps, mask=mask,
                         face_average=face_average)
        self.B = torch.zeros(nf * max(sv, 2), dtype=torch.float64, device=ctx.device)
        self.U = self.B[: d * max(sv, 2)]   # the advecting velocity: the first ldim rows of the base state
        self.set_base(rows)

    def set_base(self, q) -> "LinearisedConvection":
        """Copy the weighted rows of ``q`` (a NekVector, or n_wf arrays) into the base state; allocates
        nothing when ``q`` is a NekVector."""
        lay = self.ctx.layout
        n, sv, nf = lay.n_v, lay.sv, lay.n_wf
        rows = _base_rows(self.ctx, q)
        if isinstance(rows, NekVector):
            self.B[: nf * sv].copy_(rows.storage[: nf * sv])
        else:
            for f in range(nf):
                self.B[f * sv: f * sv + n] = torch.as_tensor(rows[f]).to(self.ctx.device)
        return self

    def _local_rhs(self, u_ptr: int, adjoint: bool) -> None:
        ctx, lay = self.ctx, self.ctx.layout
        ctx.call("nkv_linconv_rhs", lay.lx1, lay.ldim, self.D.data_ptr(), self.w.data_ptr(), *self._xyz_ptrs(),
                 self.B.data_ptr(), lay.sv, self.kappa.data_ptr(), u_ptr, lay.n_wf, lay.sv, self._r.data_ptr(), lay.sv,
                 int(adjoint), ctx.stream)
        self._average(self._r)


class ViscousBurgers:
    """The nonlinear flow ``dq/dt = N(q)`` and its time-``tau`` map ``Φ`` (module docstring).

    ``forcing``: None, a :class:`NekVector` or ``n_wf`` arrays of n_v values; it is projected by ``Π`` once.
    ``kappa``, ``mask``, ``face_average``: as for :class:`AdvectionDiffusion`.  ``residual`` and ``linearized``
    are the two callables of ``newton.newton_krylov``; ``linearized(q)`` returns the single
    :class:`LinearisedConvection` the flow owns (``self.lin``), re-based about ``q``."""

    def __init__(self, ctx: NekContext, coords: dict, kappa, dt: float, nsteps: int, forcing=None, mask=None,
                 face_average="auto"):
        lay = ctx.layout
        zero = [np.zeros(lay.n_v) for _ in range(lay.n_wf)]
        self.lin = self._make_lin(ctx, coords, zero, kappa, dt, nsteps, mask, face_average)
        self.ctx, self.dt, self.nsteps, self.tau = ctx, self.lin.dt, self.lin.nsteps, self.lin.tau
        self.bm1, self.mask, self.minv = self.lin.bm1, self.lin.mask, self.lin.minv
        f64 = dict(dtype=torch.float64, device=ctx.device)
        # the accumulator of a step and the forcing (n_wf segments each); the stage state and the right-hand
        # side are the linearised operator's work vectors (the two never run at once)
        self._acc = torch.zeros(lay.n_wf * lay.sv + 2, **f64)
        self._g = torch.zeros(lay.n_wf * lay.sv + 2, **f64)
        self._tmp = ctx.vector()
        self._forced = False
        if forcing is not None:
            self.set_forcing(forcing)

    def _make_lin(self, ctx, coords, base, kappa, dt, nsteps, mask, face_average) -> LinearisedConvection:
        """The linearised operator the flow owns (a subclass may own a subclass of it)."""
        return LinearisedConvection(ctx, coords, base, kappa, dt, nsteps, mask=mask, face_average=face_average)

    # ---- forcing ----
    def _load(self, rows, dst: NekVector) -> None:
        lay = self.ctx.layout
        rows = _base_rows(self.ctx, rows, "forcing")
        if isinstance(rows, NekVector):
            dst.copy_from(rows)
        else:
            dst.storage.zero_()
            for f in range(lay.n_wf):
                dst.storage[f * lay.sv: f * lay.sv + lay.n_v] = torch.as_tensor(rows[f]).to(self.ctx.device)

    def set_forcing(self, forcing) -> None:
        """``g = Π forcing`` (None: no forcing)."""
        lay = self.ctx.layout
        if forcing is None:
            self._forced = False
            return
        self._load(forcing, self._tmp)
        self.lin.project(self._tmp)
        self._g[: lay.n_wf * lay.sv].copy_(self._tmp.storage[: lay.n_wf * lay.sv])
        self._forced = True

    def steady_forcing(self, q_target) -> None:
        """``g = −N₀(Π q_target)``, N₀ the unforced generator: ``Π q_target`` is then an exact discrete steady
        state (``N(Π q_target)`` is ``−a + a`` point by point)."""
        lay = self.ctx.layout
        self._load(q_target, self._tmp)
        self.lin.project(self._tmp)
        self._nonlinear_rhs(self._tmp.ptr)
        self.lin._stage(None, self.lin._minv, self.lin._r.data_ptr(), -1.0, self._g.data_ptr())
        self._forced = True

    # ---- the flow ----
    def _nonlinear_rhs(self, q_ptr: int) -> None:
        """r <- dsavg of the forward advection-diffusion right-hand side of the fields at ``q_ptr`` advected by
        their own velocity rows."""
        lin, ctx, lay = self.lin, self.ctx, self.ctx.layout
        ctx.call("nkv_advdiff_rhs", lay.lx1, lay.ldim, lin.D.data_ptr(), lin.w.data_ptr(), *lin._xyz_ptrs(), q_ptr,
                 lay.sv, lin.kappa.data_ptr(), q_ptr, lay.n_wf, lay.sv, lin._r.data_ptr(), lay.sv, 0, ctx.stream)
        lin._average(lin._r)

    def _rk4(self, v_ptr, a: float, b: float, first: bool, w_ptr, out_ptr: int, zero_rest: bool = False) -> None:
        ctx, lay, lin = self.ctx, self.ctx.layout, self.lin
        sv = lay.sv
        ctx.call("nkv_rk4_stage", v_ptr, sv, lin._minv.data_ptr(), lin._r.data_ptr(), sv,
                 self._g.data_ptr() if self._forced else None, sv, float(a), float(b), int(first),
                 self._acc.data_ptr(), sv, w_ptr, sv, out_ptr, sv, lay.n_wf, int(zero_rest), ctx.stream)

    def rhs(self, q: NekVector, out: NekVector) -> None:
        """``out = N(q)`` on the weighted fields; ``q`` is taken as it is (not projected); pressure and time
        of ``out`` are zeroed."""
        self._nonlinear_rhs(q.ptr)
        self._rk4(None, 0.0, 1.0, True, None, out.ptr, zero_rest=True)   # v = NULL: acc' = 1 k

    def propagate(self, q: NekVector, out: NekVector) -> None:
        """``out = Φ(q) = RK4^nsteps(Π q)``; pressure and time of ``out`` are zeroed."""
        lin, dt = self.lin, self.dt
        lin.project(q, out)
        wp, ap = lin._w.data_ptr(), self._acc.data_ptr()
        for _ in range(self.nsteps):
            self._nonlinear_rhs(out.ptr)
            self._rk4(out.ptr, dt / 2, dt / 6, True, wp, ap)
            self._nonlinear_rhs(wp)
            self._rk4(out.ptr, dt / 2, dt / 3, False, wp, ap)
            self._nonlinear_rhs(wp)
            self._rk4(out.ptr, dt, dt / 3, False, wp, ap)
            self._nonlinear_rhs(wp)
            self._rk4(None, 0.0, dt / 6, False, None, out.ptr, zero_rest=True)

    def residual(self, q: NekVector, f: NekVector) -> None:
        """``f = Φ(q) − q`` with time 0: the ``nonlinear`` callable of ``newton_krylov``."""
        to = self.ctx.layout.time_offset
        self.propagate(q, f)
        f.storage[:to].sub_(q.storage[:to])

    def linearized(self, q: NekVector) -> LinearisedConvection:
        """The owned :class:`LinearisedConvection` about ``q``: the ``linearized`` callable of ``newton_krylov``."""
        return self.lin.set_base(q)


__all__ = ["LinearisedConvection", "ViscousBurgers"]
