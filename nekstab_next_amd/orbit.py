"""A time-periodic base flow of the viscous Burgers flow on the device: the orbit of the discrete RK4 map under
a harmonic forcing, the exact tangent of that map and its exact discrete adjoint.

Reference: the periodic half of nekStab's workflow.  Forced and natural UPO Newton (``uparam(1) = 2.2`` / ``2.1``,
newton_krylov.f90:77-91,128-131,145-148), Floquet direct, adjoint and intracycle transient growth (``3.11`` /
``3.21`` / ``3.31``, matvec.f90:176-235,414-468, eigensolvers.f90:174-176), the stored orbit ``uor/vor/wor/tor``
(``ifstorebase``, on by default, main.f90:26) and the side-by-side mode ``ifbase = .true.`` in which the
nonlinear flow and the perturbation advance together; ``compute_bvec`` (matvec.f90:575-613) for the period row.

In the notation of :mod:`~nekstab_next_amd.burgers` (``N₀`` the unforced generator, ``L_B`` / ``L_B†`` the
linearisation about ``B`` and its adjoint, ``Π`` the projector), with ``T = nsteps·dt``, ``ω = 2π/T`` and step
``n`` starting at ``t_n = n·dt``:

    g(t)     = g0 + cos(ωt)·gc + sin(ωt)·gs                 (each part projected by Π once; each may be absent)
    stages     s1 = v, s2 = v + dt/2·k1, s3 = v + dt/2·k2, s4 = v + dt·k3,  k_i = N₀(s_i) + g(t_n + θ_i·dt),
               θ = (0, ½, ½, 1);   v' = v + dt/6·k1 + dt/3·k2 + dt/3·k3 + dt/6·k4
    Φ_T(q)   = RK4^nsteps(Π q)
    tangent    κ1 = L_s1 v, κ2 = L_s2(v + dt/2·κ1), κ3 = L_s3(v + dt/2·κ2), κ4 = L_s4(v + dt·κ3),
               y = v + dt/6·κ1 + dt/3·κ2 + dt/3·κ3 + dt/6·κ4   (the exact Jacobian of the step: g drops out)
    adjoint    u4 = λ, u3 = λ + dt/2·L†_s4 u4, u2 = λ + dt/2·L†_s3 u3, u1 = λ + dt·L†_s2 u2,
               v̄ = λ + dt/6·L†_s4 u4 + dt/3·L†_s3 u3 + dt/3·L†_s2 u2 + dt/6·L†_s1 u1;  steps nsteps−1 … 0, Π first

The phase of a stage is formed on the host in f64 as ``2.0*pi*(n + θ)/nsteps``; its cos and sin travel to
``nkv_orbit_stage`` as arguments.  A base stage writes the next stage state straight into the orbit buffer, so
storing the orbit costs no pass of its own.  Nothing synchronises with the host and the work vectors are
allocated once.

The chain, as nekStab runs it (forced UPO by Newton, then Floquet multipliers, adjoint and intracycle growth):

    flow = ViscousBurgers(ctx0, coords, kappa, dt, nsteps, mask=mask);  flow.steady_forcing(target)
    of = OrbitFlow(flow, cos=gc, sin=gs)
    newton_krylov(ctx, of.residual, of.linearized, q, tol=1e-20, mode=2.2, gmres=GmresConfig(...))
    op = of.linearized(q)
    krylov_schur(ctx, LegacyMatvec(3.11, op), seed, cfg)      # 3.21: adjoint, 3.31: intracycle growth

Checkpointed storage (``OrbitFlow(…, checkpoint=c)``).  The stored orbit takes ``4·nsteps`` stage states; with
``checkpoint=c`` the period is cut into ``J = ceil(nsteps/c)`` segments of ``c`` steps (the last may be shorter)
and only the start state of every segment is kept, next to two windows of the stage states of one segment each.
``rmatvec`` then walks the segments backwards: it re-runs the base flow over a segment from its checkpoint into
a window (the same launches on the same inputs as ``propagate``, so the same bits) and runs the adjoint steps
about that window.  :func:`checkpoint_schedule` is that walk as a list of operations.  Pipelined (``fused=True``)
the adjoint of segment ``j`` and the recomputation of segment ``j − 1`` advance in the same launches: per stage
one ``nkv_burgers_backward_rhs``, one ``dsavg`` batch of the ``2·n_wf`` segments and one ``nkv_orbit_stage`` with
both halves.  Stored, sequential and pipelined ``rmatvec`` give the same bits.

Out of scope: the natural UPO Newton loop of 2.1, whose period — and with it ``dt`` — changes per
iterate (``time_derivative`` feeds its period row; the pressure-free flow has no known autonomous cycle).
"""
from __future__ import annotations

import math

import torch

from .burgers import ViscousBurgers
from .gs import average_segments
from .operators import LinearOperator
from .vector import NekVector

THETA = (0.0, 0.5, 0.5, 1.0)


def auto_checkpoint(nsteps: int) -> int:
    """``checkpoint="auto"``: ``max(1, round(sqrt(nsteps/8)))``, the minimiser of the ``nsteps/c + 8c`` slots of
    checkpoints and windows."""
    return max(1, round(math.sqrt(nsteps / 8)))


def _segment_length(nsteps: int, c) -> int:
    if c == "auto":
        return auto_checkpoint(nsteps)
    if isinstance(c, bool) or not isinstance(c, int) or c < 1:
        raise ValueError(f'checkpoint={c!r}: the steps per segment, an int >= 1, or "auto"')
    return c


def checkpoint_schedule(nsteps: int, c, fused: bool = True) -> list:
    """The backward walk of a checkpointed ``rmatvec`` over ``J = ceil(nsteps/c)`` segments (segment ``j``: steps
    ``[j·c, min((j+1)·c, nsteps))``; its window is ``j & 1``), as a list of

        ("recompute", j, window)    re-run the base over segment j from checkpoint j into the window
        ("adjoint", j, window)      the adjoint steps end−1 … start of segment j about the window
        ("pair", ja, jr, k)         adjoint step end−1−t of segment ja (window ja & 1) with recompute step
                                    start+t of segment jr = ja − 1 (window jr & 1) for t < k; k is all of ja,
                                    and the steps of jr past k (only a last segment is shorter) follow unfused

    ``fused=False``: recompute then adjoint, segment by segment.  ``fused=True``: the last segment is recomputed
    alone, every other recomputation rides with the adjoint of the segment after it, and the adjoint of segment 0
    runs alone.  Pure: no device, no state."""
    if isinstance(nsteps, bool) or not isinstance(nsteps, int) or nsteps < 1:
        raise ValueError(f"nsteps={nsteps!r} must be an int >= 1")
    c = _segment_length(nsteps, c)
    J = -(-nsteps // c)
    ops = [("recompute", J - 1, (J - 1) & 1)]
    if fused:
        ops += [("pair", j, j - 1, min((j + 1) * c, nsteps) - j * c) for j in range(J - 1, 0, -1)]
        ops.append(("adjoint", 0, 0))
    else:
        for j in range(J - 1, -1, -1):
            if j < J - 1:
                ops.append(("recompute", j, j & 1))
            ops.append(("adjoint", j, j & 1))
    return ops


class OrbitFlow:
    """``Φ_T`` of a :class:`ViscousBurgers` under ``g(t) = g0 + cos(ωt)·cos + sin(ωt)·sin`` (module docstring);
    ``g0`` is the flow's own constant forcing.  ``cos`` / ``sin``: None, a :class:`NekVector` or ``n_wf`` arrays
    of n_v values, projected by ``Π`` once.

    ``store=True`` keeps every stage state of the last ``propagate`` in an orbit buffer ``[nsteps][4][n_wf][sv]``
    of ``4·nsteps·n_wf·sv·8`` bytes on the device (``self.orbit_bytes``; sv: the padded points per field of this
    rank); ``store=False`` keeps none and the propagator advances the base next to the perturbation.
    ``residual`` and ``linearized`` are the two callables of ``newton.newton_krylov``; with ``cos = sin = None``
    ``propagate`` equals ``ViscousBurgers.propagate`` bit for bit.  The flow itself is left as it is, except
    that its work vectors are used.

    ``checkpoint=c`` (an int >= 1, or ``"auto"`` for ``max(1, round(sqrt(nsteps/8)))``; only with ``store=True``)
    keeps, instead of the whole orbit, the start state of each of the ``J = ceil(nsteps/c)`` segments of ``c``
    steps, two windows of the ``4·min(c, nsteps)`` stage states of one segment each and the four slots of the
    side-by-side ``matvec``: ``(J + 8·min(c, nsteps) + 4)·n_wf·sv·8`` bytes (``self.orbit_bytes``), about
    ``5.7·sqrt(nsteps)`` stage states with ``"auto"``.  ``propagate`` fills the windows in turn and writes the end
    of a segment straight into the next checkpoint; each window remembers which segment of which run it holds,
    and a segment it still holds is not recomputed.  ``matvec`` advances the base next to the perturbation, as
    with ``store=False``; ``rmatvec`` recomputes segment by segment (module docstring).  When a segment is
    recomputed the end state of its last step, which the next checkpoint already holds, goes to the first of the
    ``matvec`` slots as scratch: no checkpoint is written twice.  Every result carries the bits of the stored
    mode."""

    def __init__(self, flow: ViscousBurgers, cos=None, sin=None, store: bool = True, checkpoint=None):
        from .incompressible import refuse_incompressible

        refuse_incompressible("OrbitFlow", flow)
        ctx, lay = flow.ctx, flow.ctx.layout
        self.flow, self.lin, self.ctx, self.store = flow, flow.lin, ctx, bool(store)
        self.dt, self.nsteps, self.tau = flow.dt, flow.nsteps, flow.tau
        self.bm1, self.mask, self.minv = flow.bm1, flow.mask, flow.minv
        if checkpoint is not None and not self.store:
            raise ValueError("checkpoint= cuts a stored orbit into segments: it needs store=True")
        self.checkpoint = None if checkpoint is None else _segment_length(self.nsteps, checkpoint)
        f64 = dict(dtype=torch.float64, device=ctx.device)
        self._seg = lay.n_wf * lay.sv                       # doubles of one stage state
        if self.checkpoint:
            c = self.checkpoint
            self._nseg = -(-self.nsteps // c)               # J
            self._wlen = min(c, self.nsteps)                # steps per window
            slots = self._nseg + 8 * self._wlen + 4         # checkpoints | window 0 | window 1 | matvec's slots
        else:
            slots = 4 * self.nsteps if self.store else 4
        self.orbit_bytes = 8 * slots * self._seg
        try:
            self._orbit = torch.empty(slots * self._seg + 2, **f64)
        except RuntimeError as e:   # (torch.OutOfMemoryError is one)
            what = (f"{slots}·n_wf·sv·8 (checkpoint={self.checkpoint})" if self.checkpoint else "4·nsteps·n_wf·sv·8")
            raise MemoryError(f"the orbit buffer needs {what} = {self.orbit_bytes} bytes on the device "
                              f"(nsteps={self.nsteps}, n_wf={lay.n_wf}, sv={lay.sv}); checkpoint= keeps the start of "
                              f"every segment and recomputes the rest, store=False keeps no orbit") from e
        self._gc = self._part(cos)
        self._gs = self._part(sin)
        self._q0 = torch.zeros(self._seg + 2, **f64)        # the weighted rows the orbit started from
        self._tacc = torch.zeros(self._seg + 2, **f64)      # the tangent's accumulator
        side = self.checkpoint or not self.store            # the base advances next to a perturbation
        self._r2 = torch.zeros(2 * self._seg + 2, **f64) if side else None   # r_B | r_u of the fused passes
        self._out = ctx.vector() if self.store else None    # where linearized() lets a re-run end
        self._td = None                                     # the stage states of time_derivative, on first use
        self._valid = False
        self._run = 0                                       # counts propagate: with a segment, a window's tag
        self._wtag = [None, None]                           # (run, segment) each window holds
        self._plan = {f: checkpoint_schedule(self.nsteps, self.checkpoint, fused=f)
                      for f in (False, True)} if self.checkpoint else None
        self.prop = OrbitPropagator(self)

    # ---- plumbing ----
    def _part(self, rows):
        if rows is None:
            return None
        flow, n = self.flow, self._seg
        flow._load(rows, flow._tmp)
        self.lin.project(flow._tmp)
        return torch.cat([flow._tmp.storage[:n], flow._tmp.storage.new_zeros(2)])

    def _slot(self, n: int, i: int) -> int:
        """The address of stage state i of step n (one step's four slots when nothing is stored).  Checkpointed:
        in the window of the step's segment, but the first state of a segment is its checkpoint."""
        if self.checkpoint:
            j, k = divmod(n, self.checkpoint)
            at = j if k == 0 and i == 0 else self._nseg + 4 * self._wlen * (j & 1) + 4 * k + i
        else:
            at = (4 * n if self.store else 0) + i
        return self._orbit.data_ptr() + 8 * at * self._seg

    def _side_slot(self, i: int) -> int:
        """Stage state i of the step the side-by-side ``matvec`` is at."""
        at = self._nseg + 8 * self._wlen + i if self.checkpoint else i
        return self._orbit.data_ptr() + 8 * at * self._seg

    def _span(self, j: int):
        """The steps [start, end) of segment j."""
        return j * self.checkpoint, min((j + 1) * self.checkpoint, self.nsteps)

    def _holds(self, j: int) -> bool:
        return self._wtag[j & 1] == (self._run, j)

    def _recompute(self, j: int, k0: int = 0) -> None:
        """Steps k0 … of segment j again from its checkpoint (or from step k0's first state) into the segment's
        window: the launches of ``propagate``; the end of the last step goes to scratch."""
        if k0 == 0 and self._holds(j):
            return
        start, end = self._span(j)
        self._wtag[j & 1] = None
        for n in range(start + k0, end):
            self._base_step(n, [self._slot(n, i) for i in range(4)], self._next(n), 0)
        self._wtag[j & 1] = (self._run, j)

    def _next(self, n: int) -> int:
        """Where a recomputed step n ends: the first state of step n + 1 in the window, or scratch."""
        return self._side_slot(0) if (n + 1) % self.checkpoint == 0 or n + 1 == self.nsteps else self._slot(n + 1, 0)

    def phase(self, n: int, theta: float):
        ph = 2.0 * math.pi * (n + theta) / self.nsteps
        return math.cos(ph), math.sin(ph)

    def _project(self, src: int, dst: int) -> None:
        """The weighted rows at ``dst`` <- Π of those at ``src``: the launches of ``lin.project``."""
        lin = self.lin
        lin._stage(None, lin._bm1, src, 1.0, lin._r.data_ptr())
        lin._average(lin._r)
        lin._stage(None, lin._minv, lin._r.data_ptr(), 1.0, dst)

    def _stage(self, n, i, v, r, acc_out, w, zero_rest=0, tan=None) -> None:
        """Stage i of step n: the base half from the averaged right-hand side at ``r``; ``tan``: the tangent
        half's (tv, tr, tw, tacc_out)."""
        ctx, lay, flow = self.ctx, self.ctx.layout, self.flow
        sv, dt = lay.sv, self.dt
        a, b = (dt / 2, dt / 2, dt, 0.0)[i], (dt / 6, dt / 3, dt / 3, dt / 6)[i]
        c, s = self.phase(n, THETA[i])
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        tv, tr, tw, tao = tan or (None, None, None, None)
        ctx.call("nkv_orbit_stage", self.lin._minv.data_ptr(), v, sv, r, sv,
                 flow._g.data_ptr() if flow._forced else None, ptr(self._gc), ptr(self._gs), sv, c, s, float(a), float(b),
                 int(i == 0), flow._acc.data_ptr(), sv, w, sv, acc_out, sv,
                 tv, sv, tr, sv, self._tacc.data_ptr() if tan else None, sv, tw, sv, tao, sv, lay.n_wf, zero_rest,
                 ctx.stream)

    def _base_step(self, n: int, src, end: int, zero_rest: int) -> None:
        """One RK4 step of the base flow from the stage states at ``src`` (src[0] = v; src[1:] are written)."""
        flow, rp, ap = self.flow, self.lin._r.data_ptr(), self.flow._acc.data_ptr()
        for i in range(3):
            flow._nonlinear_rhs(src[i])
            self._stage(n, i, src[0], rp, ap, src[i + 1])
        flow._nonlinear_rhs(src[3])
        self._stage(n, 3, None, rp, end, None, zero_rest)

    # ---- the flow ----
    def propagate(self, q: NekVector, out: NekVector) -> None:
        """``out = Φ_T(q)``; pressure and time of ``out`` are zeroed.  With ``store`` the orbit buffer then holds
        the stage states of this run."""
        N = self.nsteps
        self._q0[: self._seg].copy_(q.storage[: self._seg])
        self._run += 1
        self._wtag = [None, None]
        self._project(q.ptr, self._slot(0, 0))
        for n in range(N):
            last = n == N - 1
            self._base_step(n, [self._slot(n, i) for i in range(4)], out.ptr if last else self._slot(n + 1, 0), int(last))
            if self.checkpoint and (last or (n + 1) % self.checkpoint == 0):
                j = n // self.checkpoint
                self._wtag[j & 1] = (self._run, j)
        self._valid = True

    def residual(self, q: NekVector, f: NekVector) -> None:
        """``f = Φ_T(q) − q`` with time 0: the ``nonlinear`` callable of ``newton_krylov``."""
        to = self.ctx.layout.time_offset
        self.propagate(q, f)
        f.storage[:to].sub_(q.storage[:to])

    def linearized(self, q: NekVector) -> "OrbitPropagator":
        """The owned :class:`OrbitPropagator` about the orbit from ``q``: the ``linearized`` callable of
        ``newton_krylov``.  The orbit is run again only if the stored one did not start from ``q`` (one
        comparison on the device, the only host synchronisation here; over shards the ranks agree on the
        answer, so the call is collective)."""
        if not self.store:
            self._q0[: self._seg].copy_(q.storage[: self._seg])
            return self.prop
        same = float(self._valid and torch.equal(self._q0[: self._seg], q.storage[: self._seg]))
        comm = self.ctx.comm
        if comm.world > 1:
            same = comm.min_scalar(same, device=self.ctx.device)
        if not same:
            self.propagate(q, self._out)
        return self.prop

    def time_derivative(self, q: NekVector, out: NekVector, step: int = 0) -> None:
        """``out = (one RK4 step from q at t_step − q)/dt`` with time 0, ``q`` taken as it is: ``compute_bvec``
        (matvec.f90:575-613), the ``b_fc`` / ``b_ic`` of ``LegacyMatvec(2.1, …)``.  Pressure is zeroed; the stored
        orbit is left alone."""
        n = self._seg
        if self._td is None:
            self._td = torch.zeros(3 * n + 2, dtype=torch.float64, device=self.ctx.device)
        td = self._td.data_ptr()
        self._base_step(int(step), [q.ptr] + [td + 8 * i * n for i in range(3)], out.ptr, 1)
        out.storage[:n].sub_(q.storage[:n]).div_(self.dt)


class OrbitPropagator(LinearOperator):
    """``matvec``: the tangent of ``Φ_T`` over one period about the orbit of its :class:`OrbitFlow`, ``rmatvec``:
    its exact adjoint in the inner product weighted by ``bm1`` (module docstring).

    With the orbit stored each stage is ``nkv_linconv_rhs`` with the base state pointing into the orbit buffer,
    one ``dsavg`` batch and ``nkv_rk4_stage``.  With ``store=False`` (the reference's ``ifbase = .true.``)
    ``matvec`` advances the base from the state ``linearized`` was given next to the perturbation: one
    ``nkv_burgers_tangent_rhs``, one ``dsavg`` batch of the ``2·n_wf`` segments and one ``nkv_orbit_stage`` per
    stage, the same bits as the stored mode; ``rmatvec`` then has no orbit to run backwards through and raises.
    About a checkpointed orbit ``matvec`` is that side-by-side run and ``rmatvec`` follows
    :func:`checkpoint_schedule`: ``fused=False`` recomputes a segment, then runs its adjoint; ``fused=True``
    pairs the adjoint of a segment with the recomputation of the one before it (``nkv_burgers_backward_rhs``);
    ``fused=None`` takes ``FUSED_DEFAULT``.  All three give the bits of the stored mode; nothing synchronises
    with the host and nothing is allocated."""

    FUSED_DEFAULT = True

    def __init__(self, of: OrbitFlow):
        self.of, self.ctx, self.lin = of, of.ctx, of.lin
        self.dt, self.nsteps, self.tau = of.dt, of.nsteps, of.tau
        self.bm1 = of.bm1

    def _linconv(self, B: int, u: int, adjoint: bool) -> None:
        lin, ctx, lay = self.lin, self.ctx, self.ctx.layout
        ctx.call("nkv_linconv_rhs", lay.lx1, lay.ldim, lin.D.data_ptr(), lin.w.data_ptr(), *lin._xyz_ptrs(), B, lay.sv,
                 lin.kappa.data_ptr(), u, lay.n_wf, lay.sv, lin._r.data_ptr(), lay.sv, int(adjoint), ctx.stream)
        lin._average(lin._r)

    def _rk4(self, v, a: float, b: float, first: bool, w, out: int, zero_rest: bool = False) -> None:
        ctx, lay, lin = self.ctx, self.ctx.layout, self.lin
        sv = lay.sv
        ctx.call("nkv_rk4_stage", v, sv, lin._minv.data_ptr(), lin._r.data_ptr(), sv, None, sv, float(a), float(b),
                 int(first), self.of._tacc.data_ptr(), sv, w, sv, out, sv, lay.n_wf, int(zero_rest), ctx.stream)

    def _stored(self) -> None:
        if not self.of._valid:
            raise RuntimeError("no orbit yet: call OrbitFlow.propagate, residual or linearized first")

    def _side_by_side(self, y: NekVector) -> None:
        of, lin, ctx, lay = self.of, self.lin, self.ctx, self.ctx.layout
        sv, nf, seg = lay.sv, lay.n_wf, of._seg
        rB = of._r2.data_ptr()
        ru = rB + 8 * seg
        segments = [rB + 8 * f * sv for f in range(2 * nf)]
        wp, ap, tp = lin._w.data_ptr(), of.flow._acc.data_ptr(), of._tacc.data_ptr()
        s = [of._side_slot(i) for i in range(4)]
        of._project(of._q0.data_ptr(), s[0])
        for n in range(self.nsteps):
            for i in range(4):
                ctx.call("nkv_burgers_tangent_rhs", lay.lx1, lay.ldim, lin.D.data_ptr(), lin.w.data_ptr(),
                         *lin._xyz_ptrs(), s[i], sv, lin.kappa.data_ptr(), y.ptr if i == 0 else wp, nf, sv, rB, sv, ru, sv,
                         ctx.stream)
                average_segments(lin.face_average, segments)
                if i < 3:
                    of._stage(n, i, s[0], rB, ap, s[i + 1], tan=(y.ptr, ru, wp, tp))
                else:
                    of._stage(n, i, None, rB, s[0], None, zero_rest=2, tan=(None, ru, None, y.ptr))

    def matvec(self, x: NekVector, y: NekVector) -> None:
        of, dt = self.of, self.dt
        self.lin.project(x, y)
        if not of.store:
            self._side_by_side(y)
            return
        self._stored()
        if of.checkpoint:
            self._side_by_side(y)
            return
        wp, tp = self.lin._w.data_ptr(), of._tacc.data_ptr()
        for n in range(self.nsteps):
            self._linconv(of._slot(n, 0), y.ptr, False)
            self._rk4(y.ptr, dt / 2, dt / 6, True, wp, tp)
            self._linconv(of._slot(n, 1), wp, False)
            self._rk4(y.ptr, dt / 2, dt / 3, False, wp, tp)
            self._linconv(of._slot(n, 2), wp, False)
            self._rk4(y.ptr, dt, dt / 3, False, wp, tp)
            self._linconv(of._slot(n, 3), wp, False)
            self._rk4(None, 0.0, dt / 6, False, None, y.ptr, zero_rest=True)

    def _adjoint_steps(self, steps, y: NekVector) -> None:
        """The adjoint of the base steps ``steps`` (descending) about their stage states, in place in ``y``."""
        of, dt = self.of, self.dt
        wp, tp = self.lin._w.data_ptr(), of._tacc.data_ptr()
        for n in steps:
            self._linconv(of._slot(n, 3), y.ptr, True)
            self._rk4(y.ptr, dt / 2, dt / 6, True, wp, tp)
            self._linconv(of._slot(n, 2), wp, True)
            self._rk4(y.ptr, dt / 2, dt / 3, False, wp, tp)
            self._linconv(of._slot(n, 1), wp, True)
            self._rk4(y.ptr, dt, dt / 3, False, wp, tp)
            self._linconv(of._slot(n, 0), wp, True)
            self._rk4(None, 0.0, dt / 6, False, None, y.ptr, zero_rest=True)

    def _paired_step(self, n: int, m: int, y: NekVector) -> None:
        """The adjoint of step n about its window and base step m into the other window, stage by stage in the
        same launches.  The (a, b) of an adjoint stage are the base stage's, so ``nkv_orbit_stage`` serves both
        halves: its base half is stage i of step m, its tangent half adjoint stage i about s_{4−i}(n)."""
        of, lin, ctx, lay = self.of, self.lin, self.ctx, self.ctx.layout
        sv, nf = lay.sv, lay.n_wf
        rX = of._r2.data_ptr()
        ru = rX + 8 * of._seg
        segments = [rX + 8 * f * sv for f in range(2 * nf)]
        wp, ap, tp = lin._w.data_ptr(), of.flow._acc.data_ptr(), of._tacc.data_ptr()
        S = [of._slot(n, i) for i in range(4)]
        X = [of._slot(m, i) for i in range(4)]
        for i in range(4):
            ctx.call("nkv_burgers_backward_rhs", lay.lx1, lay.ldim, lin.D.data_ptr(), lin.w.data_ptr(), *lin._xyz_ptrs(),
                     X[i], sv, S[3 - i], sv, lin.kappa.data_ptr(), y.ptr if i == 0 else wp, nf, sv, rX, sv, ru, sv,
                     ctx.stream)
            average_segments(lin.face_average, segments)
            if i < 3:
                of._stage(m, i, X[0], rX, ap, X[i + 1], tan=(y.ptr, ru, wp, tp))
            else:   # (bit 0 is never set: the base half ends in the orbit buffer)
                of._stage(m, i, None, rX, of._next(m), None, zero_rest=2, tan=(None, ru, None, y.ptr))

    def _pair(self, ja: int, jr: int, k: int, y: NekVector) -> None:
        of = self.of
        start, end = of._span(ja)
        if of._holds(jr):           # nothing to recompute next to this adjoint
            self._adjoint_steps(range(end - 1, start - 1, -1), y)
            return
        of._wtag[jr & 1] = None
        first = of._span(jr)[0]
        for t in range(k):
            self._paired_step(end - 1 - t, first + t, y)
        of._wtag[jr & 1] = (of._run, jr)
        of._recompute(jr, k)        # the steps of jr without a partner (a shorter last segment)

    def rmatvec(self, x: NekVector, y: NekVector, fused=None) -> None:
        of = self.of
        if not of.store:
            raise RuntimeError("the adjoint runs backwards through the stored orbit: build the OrbitFlow with store=True")
        self._stored()
        self.lin.project(x, y)
        if not of.checkpoint:
            self._adjoint_steps(range(self.nsteps - 1, -1, -1), y)
            return
        for op in of._plan[bool(self.FUSED_DEFAULT if fused is None else fused)]:
            if op[0] == "recompute":
                of._recompute(op[1])
            elif op[0] == "adjoint":
                start, end = of._span(op[1])
                self._adjoint_steps(range(end - 1, start - 1, -1), y)
            else:
                self._pair(op[1], op[2], op[3], y)


__all__ = ["OrbitFlow", "OrbitPropagator", "auto_checkpoint", "checkpoint_schedule"]
