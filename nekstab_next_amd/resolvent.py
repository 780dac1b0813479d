"""A time-stepper resolvent operator over the model propagator: the operator ``drivers.resolvent_analysis``
runs ``svds`` on, as a PDE on the GLL mesh.

Reference: nekStab's ``resolvent_op`` (core/linear_operators.f90:309-431): a harmonically forced Nek5000
integration, an inner GMRES on ``I - exp(tau A)`` and a quarter-period run, driven by ``resolvent_analysis``
(linear_stab.f90:121-163).  Here the stepper is :class:`~nekstab_next_amd.advdiff.AdvectionDiffusion`'s and
the formulation is the rotating frame: with the response ``u(t) = Re[y(t) e^{i omega t}]`` the forcing
``Re[f e^{i omega t}]`` (``forcing.BodyForce``, forcing.f90:18-33) becomes constant,

    dy/dt = G y + Pi f,    G = L - i omega,    steady state  y = (i omega - L)^-1 Pi f,

``L = minv · dsavg(r(·))`` and ``Pi`` of advdiff.py acting on the re and the im half of a complex (pair)
vector.  One RK4 step is the Horner form of advdiff.py with the forcing inside,

    w <- y + (dt / s) (G w + f)   for s = 4, 3, 2, 1 from w = y:     y+ = p(dt G) y + dt phi(dt G) f,
    phi(z) = (p(z) - 1) / z,

and over ``nsteps`` steps (``tau = nsteps · dt``), with ``Phi`` the unforced run and ``b`` the forced run from 0:

    matvec:  y = (I - Phi)^-1 b     by ``lightkrylov.gmres`` on the pair context, from y = 0.

Since ``p(z) - 1 = z phi(z)`` the fixed point is ``(i omega - L)^-1 Pi f`` exactly, for any stable ``dt`` and
any ``nsteps``: the time stepping only preconditions the solve and leaves no O(dt^4) error.  ``rmatvec`` is
the same algorithm on ``L†`` with ``-omega`` (``G† = L† + i omega``): the adjoint of ``matvec`` in the pair inner
product weighted by ``adv.bm1`` up to the inner tolerance, not up to a time-discretisation error.  The
deviations from the reference's real-state form are DESIGN §3's.

:class:`CoupledResolventOperator` is the same algorithm about a base state ``B``: ``L = L_B`` of
:class:`~nekstab_next_amd.burgers.LinearisedConvection`, production term ``(u'·∇)B`` included, the non-normal
part that makes resolvent gains large.  :class:`IncompressibleResolventOperator` is that operator over a
:class:`~nekstab_next_amd.incompressible.LinearisedNavierStokes`: ``L = P L_B`` on the divergence-free velocities,
the projection of both halves of every stage in one two-system pressure CG.

Stability: every ``dt · (lambda - i omega)``, lambda in the spectrum of L, inside RK4's region, roughly
``dt · rho(L - i omega) <~ 2.78``.  On the edge of that region phi vanishes (z = -2.785 and
z = -0.607 ± 2.872i), where ``I - Phi`` loses the forcing's component: keep ``dt`` inside.

Each Horner pass is ``nkv_advdiff_rhs`` on the re and on the im halves (coupled: one ``nkv_linconv_crhs`` for
both), one ``dsavg`` batch of the ``2 · n_wf`` segments and one fused complex stage (``nkv_advdiff_cstage``,
include/nekkrylov.h).  The work vectors are allocated once and nothing synchronises with the host outside GMRES.
"""
from __future__ import annotations

import math

import torch

from .advdiff import AdvectionDiffusion
from .gs import average_segments
from .layout import PairLayout, pair_layout
from .lightkrylov import gmres
from .operators import LinearOperator
from .vector import NekContext, NekVector


def pair_context(adv: AdvectionDiffusion, max_cols: int = 64, **kw) -> NekContext:
    """The context of the complex (re/im pair) vectors of ``adv``'s mesh: ``pair_layout`` of its layout,
    ``adv.bm1`` on both halves as weights, its communicator and device.  ``max_cols`` bounds the inner
    GMRES's ``kdim`` and the outer ``svds``'s basis."""
    return NekContext(pair_layout(adv.ctx.layout), weights=torch.cat([adv.bm1, adv.bm1]), comm=adv.ctx.comm,
                      max_cols=max_cols, device=adv.ctx.device, **kw)


class _OneMinusPhi(LinearOperator):
    """x -> x - Phi x, the operator of the inner solve."""

    def __init__(self, op: "ResolventOperator", adjoint: bool):
        self.op, self.adjoint = op, adjoint

    def matvec(self, x: NekVector, y: NekVector) -> None:
        self.op.propagate(x, y, self.adjoint)
        y.axpby(-1.0, x, 1.0)


class ResolventOperator(LinearOperator):
    """``y = (i omega - L)^-1 Pi x`` on complex pair vectors and its adjoint (module docstring).

    ``pctx``: a :class:`NekContext` on ``pair_layout(adv.ctx.layout)`` whose weights are ``adv.bm1`` on both
    halves (:func:`pair_context` builds it); anything else is refused.  ``adv`` lends its coordinates, base
    flow, kappa, ``minv``, ``face_average``, ``dt`` and ``nsteps`` (its tensors are bound at construction) and is
    not changed.  ``tol``: the inner GMRES stops at ``||b - (I - Phi) y|| <= tol ||b||``; ``kdim`` (at most ``pctx.max_cols``) and ``maxiter``
    are its basis size and restarts.  An inner solve that does not converge raises ``RuntimeError``.
    ``last_gmres``: ``{"info", "residuals", "adjoint"}`` of the latest solve."""

    # Whether the class projects every stage onto the divergence-free velocities: one that does not refuses the
    # incompressible models, whose projection it would silently skip.
    projects_stages = False

    def __init__(self, pctx: NekContext, adv: AdvectionDiffusion, omega: float, tol: float = 1e-10, kdim: int = 60,
                 maxiter: int = 20):
        if not self.projects_stages:
            from .incompressible import refuse_incompressible

            refuse_incompressible(type(self).__name__, adv)
        self._check_model(adv)
        base = adv.ctx.layout
        if not isinstance(pctx.layout, PairLayout) or pctx.layout != pair_layout(base):
            raise ValueError("ResolventOperator: pctx must be a context on pair_layout(adv.ctx.layout)")
        if pctx.device != adv.ctx.device or pctx.comm.world != adv.ctx.comm.world or pctx.comm.rank != adv.ctx.comm.rank:
            raise ValueError("ResolventOperator: pctx and adv.ctx differ in device or communicator")
        n = base.n_v
        if not (torch.equal(pctx.w[:n], adv.bm1) and torch.equal(pctx.w[n: 2 * n], adv.bm1)):
            raise ValueError("ResolventOperator: the weights of pctx must be adv.bm1 on both halves (pair_context)")
        if pctx.time_in_dot:
            raise ValueError("ResolventOperator: time_in_dot contexts are refused (the time slot is not a state)")
        if adv.nsteps < 1 or not adv.dt > 0.0:
            raise ValueError(f"dt={adv.dt}, nsteps={adv.nsteps}: need dt > 0 and nsteps >= 1")
        if not math.isfinite(omega) or not tol > 0.0 or maxiter < 1:
            raise ValueError(f"omega={omega}, tol={tol}, maxiter={maxiter}: need a finite omega, tol > 0, maxiter >= 1")
        if not 1 <= kdim <= pctx.max_cols:
            raise ValueError(f"kdim={kdim} outside 1..max_cols={pctx.max_cols} of pctx")
        self.ctx, self.adv, self.omega = pctx, adv, float(omega)
        self.dt, self.nsteps, self.tau = adv.dt, adv.nsteps, adv.nsteps * adv.dt
        self.tol, self.kdim, self.maxiter = float(tol), int(kdim), int(maxiter)
        self.bm1 = adv.bm1
        self.last_gmres = None
        # the work vectors of a step (n_wf pair segments each), the projected forcing and the right-hand side
        f64 = dict(dtype=torch.float64, device=pctx.device)
        size = pctx.layout.n_wf * pctx.layout.sv + 2
        self._r, self._wa, self._wb = (torch.zeros(size, **f64) for _ in range(3))
        self._f, self._b = pctx.vector(), pctx.vector()
        self._shifted = {False: _OneMinusPhi(self, False), True: _OneMinusPhi(self, True)}
        # A solve is tens of thousands of small launches and the host's time per call sets its duration: the
        # arguments that never change are formed once.  adv's tensors are bound here (and kept alive); writing
        # into them in place still takes effect.
        psv, nf = pctx.layout.sv, base.n_wf
        self._bound = (adv.D, adv.w, adv.xyz, adv.U, adv.kappa, adv._minv, adv._bm1)
        self._rhs_head = (base.lx1, base.ldim, adv.D.data_ptr(), adv.w.data_ptr(), *adv._xyz_ptrs(), adv.U.data_ptr(),
                          base.sv, adv.kappa.data_ptr())
        self._half = 8 * n
        rp = self._r.data_ptr()
        self._avg_ptrs = [h + 8 * k * psv for k in range(nf) for h in self._halves(rp)]

    # ---- plumbing ----
    @staticmethod
    def _check_model(adv) -> None:
        """The models this class steps: anything but a LinearisedConvection, whose production term
        ``nkv_advdiff_rhs`` does not have."""
        from .burgers import LinearisedConvection

        if isinstance(adv, LinearisedConvection):
            raise ValueError("ResolventOperator: a LinearisedConvection is refused: the resolvent steps with "
                             "nkv_advdiff_rhs and would silently drop the production term (u'.grad)B; "
                             "CoupledResolventOperator is the resolvent about a base state")

    def _halves(self, ptr: int):
        return ptr, ptr + self._half

    def _local_rhs(self, src: int, adjoint: bool, st: int) -> None:
        """r <- dsavg of the local right-hand sides of the re and im halves of the n_wf fields at ``src``."""
        call, psv, nf = self.adv.ctx.call, self.ctx.layout.sv, self.ctx.layout.n_wf
        for u, r in zip(self._halves(src), self._halves(self._r.data_ptr())):
            call("nkv_advdiff_rhs", *self._rhs_head, u, nf, psv, r, psv, int(adjoint), st)
        average_segments(self.adv.face_average, self._avg_ptrs)

    def _cstage(self, v, m: torch.Tensor, r: int, s: int, f, omega: float, c: float, w: int, st: int,
                zero_rest: bool = False) -> None:
        ctx, psv = self.ctx, self.ctx.layout.sv
        none = (None, None)
        ctx.call("nkv_advdiff_cstage", *(self._halves(v) if v else none), psv, m.data_ptr(), *self._halves(r), psv,
                 *self._halves(s), psv, *(self._halves(f) if f else none), psv, float(omega), float(c), *self._halves(w),
                 psv, ctx.layout.n_wf, int(zero_rest), st)

    def _steps(self, y: NekVector, f, adjoint: bool) -> None:
        """nsteps RK4 steps of dy/dt = G y [+ f] in place (G† if ``adjoint``)."""
        om = -self.omega if adjoint else self.omega
        minv, rp, st = self.adv._minv, self._r.data_ptr(), self.ctx.stream
        wa, wb = self._wa.data_ptr(), self._wb.data_ptr()
        for _ in range(self.nsteps):
            src = y.ptr
            for s, out in ((4, wa), (3, wb), (2, wa)):   # w is never its own source: two work vectors in turn
                self._local_rhs(src, adjoint, st)
                self._cstage(y.ptr, minv, rp, src, f, om, self.dt / s, out, st)
                src = out
            self._local_rhs(src, adjoint, st)
            self._cstage(y.ptr, minv, rp, src, f, om, self.dt, y.ptr, st, zero_rest=True)

    # ---- the pieces ----
    def project(self, f: NekVector, y: NekVector | None = None) -> NekVector:
        """``y = Pi f`` on both halves (in place when ``y`` is None); pressure and time of ``y`` are zeroed."""
        y = f if y is None else y
        rp, st = self._r.data_ptr(), self.ctx.stream
        self._cstage(None, self.adv._bm1, f.ptr, f.ptr, None, 0.0, 1.0, rp, st)                 # bm1 f
        average_segments(self.adv.face_average, self._avg_ptrs)
        self._cstage(None, self.adv._minv, rp, rp, None, 0.0, 1.0, y.ptr, st, zero_rest=True)   # minv dsavg(.)
        return y

    def forced_run(self, f: NekVector, b: NekVector, adjoint: bool = False) -> None:
        """``b`` = nsteps forced steps from 0 under the constant forcing ``f``, taken as it is (project it
        first): ``b = dt phi(dt G) sum_k p(dt G)^k f``.  ``b`` must not be ``f``."""
        if b.ptr == f.ptr:
            raise ValueError("forced_run: b must not be f")
        b.zero()
        self._steps(b, f.ptr, adjoint)

    def propagate(self, x: NekVector, y: NekVector, adjoint: bool = False) -> None:
        """``y = Phi x = p(dt G)^nsteps x``, the unforced run from ``x`` taken as it is; pressure and time of
        ``y`` are zeroed."""
        if y.ptr != x.ptr:
            y.copy_from(x)
        self._steps(y, None, adjoint)

    # ---- the operator ----
    def _apply(self, x: NekVector, y: NekVector, adjoint: bool) -> None:
        self.project(x, self._f)
        self.forced_run(self._f, self._b, adjoint)
        y.zero()
        info, hist = gmres(self.ctx, self._shifted[adjoint], self._b, y, atol=0.0, rtol=self.tol, kdim=self.kdim,
                           maxiter=self.maxiter)
        self.last_gmres = dict(info=info, residuals=hist, adjoint=adjoint)
        if info != 0:
            raise RuntimeError(f"{type(self).__name__}: the inner GMRES did not converge (omega={self.omega}, kdim={self.kdim}, "
                               f"maxiter={self.maxiter}, tol={self.tol}): residuals {hist}")

    def matvec(self, x: NekVector, y: NekVector) -> None:
        self._apply(x, y, False)

    def rmatvec(self, x: NekVector, y: NekVector) -> None:
        self._apply(x, y, True)


class CoupledResolventOperator(ResolventOperator):
    """``y = (i omega - L_B)^-1 Pi x`` on complex pair vectors and, as ``rmatvec``, ``(-i omega - L_B†)^-1 Pi x``:
    the resolvent about a base state ``B``, with ``L_B`` the linearised convection of
    :class:`~nekstab_next_amd.burgers.LinearisedConvection` (advection by ``B``'s velocity, diffusion and the
    production term ``(u'·∇)B``) and ``L_B†`` its exact discrete adjoint.

    Everything is :class:`ResolventOperator`'s (``project``, ``forced_run``, ``propagate``, the inner GMRES on
    ``I - Phi``, ``last_gmres``, the context checks, the zeroing of pressure and time) except the local
    right-hand side: ``B`` is real and does not mix the halves, so one ``nkv_linconv_crhs`` per Horner pass
    writes both (the bits of ``nkv_linconv_rhs`` on each half), followed by the same ``dsavg`` batch.
    ``pair_context(lin)`` builds ``pctx``.  ``lin.B`` is bound at construction: ``lin.set_base(q)`` afterwards
    writes into it in place and takes effect on the next product without rebuilding the operator.  Anything
    that is not a ``LinearisedConvection`` is refused."""

    def __init__(self, pctx: NekContext, lin, omega: float, tol: float = 1e-10, kdim: int = 60, maxiter: int = 20):
        super().__init__(pctx, lin, omega, tol=tol, kdim=kdim, maxiter=maxiter)
        base = lin.ctx.layout
        self.lin = lin
        self._bound = self._bound + (lin.B,)
        self._crhs_head = (base.lx1, base.ldim, lin.D.data_ptr(), lin.w.data_ptr(), *lin._xyz_ptrs(), lin.B.data_ptr(),
                           base.sv, lin.kappa.data_ptr())

    @staticmethod
    def _check_model(adv) -> None:
        from .burgers import LinearisedConvection

        if not isinstance(adv, LinearisedConvection):
            raise ValueError(f"CoupledResolventOperator: needs a LinearisedConvection (the base state and its production "
                             f"term), not a {type(adv).__name__}; ResolventOperator steps a plain AdvectionDiffusion")

    def _local_rhs(self, src: int, adjoint: bool, st: int) -> None:
        """r <- dsavg of the linearised local right-hand sides of both halves of the n_wf fields at ``src``."""
        psv, rp = self.ctx.layout.sv, self._r.data_ptr()
        self.adv.ctx.call("nkv_linconv_crhs", *self._crhs_head, *self._halves(src), self.ctx.layout.n_wf, psv,
                          *self._halves(rp), psv, int(adjoint), st)
        average_segments(self.adv.face_average, self._avg_ptrs)


class IncompressibleResolventOperator(CoupledResolventOperator):
    """The resolvent of the incompressible linearised Navier-Stokes operator about a base state ``B`` (nekStab's
    ``resolvent_op``, which integrates exactly this operator), on complex pair vectors:

        matvec:   y = (i omega - P L_B)^-1 P Pi x   on range(P Pi)
        rmatvec:  y = (-i omega - P L_B†)^-1 P Pi x

    with ``P`` the divergence-free projection of ``lns.projector`` (:mod:`~nekstab_next_amd.pressure`) and ``L_B``,
    ``L_B†`` of :class:`~nekstab_next_amd.incompressible.LinearisedNavierStokes`.  The rotating-frame Horner stepper
    and the inner GMRES on ``I - Phi`` are the parents'; a Horner pass is

        nkv_linconv_crhs, the dsavg batch            r   (both halves)
        nkv_advdiff_cstage, v = NULL, omega = 0       k = minv r
        lns.projector.project_pair_ptr                k_vel <- P k_vel on the re and the im half: ONE two-system CG
        nkv_advdiff_cstage, the mask for minv         w = y + c (k + omega-coupling + f)

    as ``LinearisedNavierStokes._propagate`` closes its stages; scalar rows (``n_wf > ldim``) pass unprojected.
    ``project`` gives ``P Pi f`` on both halves.

    Exactness: ``range(P Pi)`` (on both halves) is invariant under the stage, since ``P k``, the coupling term
    ``omega s`` of a source in the range and the projected forcing all lie in it.  On it the step is
    ``y+ = p(dt G) y + dt phi(dt G) f`` with ``G = P L_B - i omega`` restricted to the range, so the module
    docstring's argument (``p(z) - 1 = z phi(z)``) carries over: the fixed point of ``(I - Phi) y = b`` is
    ``(i omega - P L_B)^-1 P Pi f`` exactly, for any stable ``dt`` and any ``nsteps``.  ``P`` is self-adjoint in the
    ``bm1`` inner product, so the adjoint of ``P L_B`` restricted to the range is ``P L_B†`` restricted to it, and
    ``rmatvec`` is the adjoint of ``matvec`` in the pair inner product up to the CG tolerance of the
    projector and the tolerance of the inner GMRES, not up to a time-discretisation error.

    ``batched=False`` projects the halves one after the other with ``project_ptr`` (through a staging buffer on
    the base layout's stride): the path the tests and tools/bench_incompressible_resolvent.py compare with; on
    one rank it gives the same bits.  ``pair_context(lns)`` builds ``pctx``; ``lns.set_base(q)`` takes effect on
    the next product.  Anything that is not a ``LinearisedNavierStokes`` is refused."""

    projects_stages = True

    def __init__(self, pctx: NekContext, lns, omega: float, tol: float = 1e-10, kdim: int = 60, maxiter: int = 20,
                 batched: bool = True):
        super().__init__(pctx, lns, omega, tol=tol, kdim=kdim, maxiter=maxiter)
        base = lns.ctx.layout
        self.lns, self.projector, self.batched = lns, lns.projector, bool(batched)
        f64 = dict(dtype=torch.float64, device=pctx.device)
        self._k = torch.zeros(pctx.layout.n_wf * pctx.layout.sv + 2, **f64)
        self._stage_buf = None if self.batched else torch.zeros(base.ldim * base.sv + 2, **f64)
        self._bound = self._bound + (lns.mask,)

    @staticmethod
    def _check_model(adv) -> None:
        from .incompressible import LinearisedNavierStokes

        if not isinstance(adv, LinearisedNavierStokes):
            raise ValueError(f"IncompressibleResolventOperator: needs a LinearisedNavierStokes (the base state and the "
                             f"divergence-free projection), not a {type(adv).__name__}; CoupledResolventOperator is the "
                             f"resolvent of a LinearisedConvection, ResolventOperator of a plain AdvectionDiffusion")

    def _project_velocity(self, ptr: int, t: torch.Tensor) -> None:
        """``P`` in place on the velocity rows of both halves of the pair fields at ``ptr`` (the storage ``t``)."""
        psv = self.ctx.layout.sv
        if self.batched:
            self.projector.project_pair_ptr(ptr, ptr + self._half, psv)
            return
        base = self.adv.ctx.layout
        d, n, sv = base.ldim, base.n_v, base.sv
        off = (ptr - t.data_ptr()) // 8
        rows = t[off: off + d * psv].view(d, psv)
        buf = self._stage_buf[: d * sv].view(d, sv)
        for h in range(2):
            buf[:, :n].copy_(rows[:, h * n: (h + 1) * n])
            self.projector.project_ptr(self._stage_buf.data_ptr())
            rows[:, h * n: (h + 1) * n].copy_(buf[:, :n])

    def _pass(self, y: int, src: int, f, om: float, c: float, out: int, adjoint: bool, zero_rest: bool = False) -> None:
        """One Horner pass: ``out = y + c (P(minv dsavg r(src)) + om-coupling of src [+ f])``."""
        rp, kp, st = self._r.data_ptr(), self._k.data_ptr(), self.ctx.stream
        self._local_rhs(src, adjoint, st)
        self._cstage(None, self.adv._minv, rp, rp, None, 0.0, 1.0, kp, st)             # k = minv r
        self._project_velocity(kp, self._k)
        self._cstage(y, self.lns.mask, kp, src, f, om, c, out, st, zero_rest=zero_rest)

    def _steps(self, y: NekVector, f, adjoint: bool) -> None:
        """nsteps RK4 steps of dy/dt = (P L_B - i omega) y [+ f] in place (L_B†, +i omega if ``adjoint``)."""
        om = -self.omega if adjoint else self.omega
        wa, wb = self._wa.data_ptr(), self._wb.data_ptr()
        for _ in range(self.nsteps):
            src = y.ptr
            for s, out in ((4, wa), (3, wb), (2, wa)):   # w is never its own source: two work vectors in turn
                self._pass(y.ptr, src, f, om, self.dt / s, out, adjoint)
                src = out
            self._pass(y.ptr, src, f, om, self.dt, y.ptr, adjoint, zero_rest=True)

    def project(self, f: NekVector, y: NekVector | None = None) -> NekVector:
        """``y = P Pi f`` on both halves (in place when ``y`` is None); pressure and time of ``y`` are zeroed."""
        y = super().project(f, y)
        self._project_velocity(y.ptr, y.storage)
        return y


__all__ = ["CoupledResolventOperator", "IncompressibleResolventOperator", "ResolventOperator", "pair_context"]
