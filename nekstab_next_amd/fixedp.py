"""Selective frequency damping and time-delayed feedback on the device (core/fixedp.f90:2-216).

nekStab reaches a base flow by forcing the time stepper: ``SFD`` (uparam(1) = 1.1, fixedp.f90:124-216)
low-pass filters the flow and feeds the difference back, ``TDF`` (1.4, :2-121) feeds back the
difference to the flow one period ago; both are called once per time step from ``userchk``
(core/main.f90:156-176).  Here each step is ONE streaming kernel (``nkv_sfd_step`` /
``nkv_tdf_step``, csrc/fixedp.hip) with the residual norm out of the same pass:

    SFD, istep >= 1 (:157-189)                         reference sweeps
        d     = v_old - qbar                           k_sub3(qa, oldV, oldQ)
        m     = adt d + bdt qa + cdt qb                k_copy/k_cmult/k_add2 x 3 (qa, qb: previous d's)
        qbar += cutoff dt m                            k_cmult, k_add2
        fc   += gain (v_old - qbar)                    k_sub3, k_cmult, nopadd2 (the LAGGED flow v_old)
        res   = normvc(v_old - v);  v_old = v          nopsub2, normvc, nopcopy
    TDF, istep > norbit (:71-96)
        r = v - v(t - T);  fc += gain r;  l2 = normvc(r);  history <- v

The reference's ``qc <- qb <- qa`` copies (:158-159) are a rotation of three buffers, and TDF's
shift of the whole history every step (:77-89) is a ring: the slot of step ``istep`` is
``(istep - 1) mod norbit``.  The host keeps the step counter, the AB3 coefficients, the residual
bookkeeping and ``residu.dat``; all arithmetic on fields is in the library.  No CPU path.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .layout import PairLayout
from .vector import NekContext, NekVector

TWO_PI = 8.0 * math.atan(1.0)   # the reference's 8*atan(1.0d0) (:35, :134)


# ---- host logic (pure functions: tested without a GPU) ------------------------------------------

def sfd_coefficients(uparam4: float, uparam5: float) -> tuple[float, float]:
    """(cutoff, gain) of SFD from uparam(4) (Strouhal number; its sign picks the branch) and
    uparam(5) (growth rate), fixedp.f90:134-145: Åkervik when uparam4 > 0, Casacuberta otherwise."""
    frq = abs(uparam4) * TWO_PI
    sig = abs(uparam5)
    if uparam4 > 0:
        return 0.5 * frq, -2 * sig
    root = math.sqrt(frq ** 2 + sig ** 2)
    return 0.5 * (root - sig), -0.5 * (root + sig)


def ab3_coefficients(istep: int) -> tuple[float, float, float]:
    """(adt, bdt, cdt) of Nek5000's ``setab3`` (external to the reference tree; called at :157) for a
    constant time step: Euler at step 1, AB2 at step 2, AB3 from step 3 on."""
    if istep < 1:
        raise ValueError("istep >= 1")
    if istep == 1:
        return 1.0, 0.0, 0.0
    if istep == 2:
        return 1.5, -0.5, 0.0
    return 23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0


def sfd_is_monitor(uparam5: float) -> bool:
    """The continuation branch (:137, :178-183): uparam(5) <= 0 leaves filter and forcing out."""
    return not uparam5 > 0


def sfd_converged(istep: int, res: float, tol: float, min_steps: int = 100) -> bool:
    """``istep > 100 .and. res < dtol`` (:201)."""
    return istep > min_steps and res < tol


def tdf_parameters(period: float, dt_target: float) -> tuple[int, float, float]:
    """(norbit, dt, gain) of TDF: norbit = ceiling(porbit/dt), dt = porbit/norbit so that the orbit
    closes to machine accuracy (:24-27), gain = -0.04432 * 2 pi / porbit (:35)."""
    if not (period > 0 and dt_target > 0):
        raise ValueError("period and dt_target must be positive")
    norbit = int(math.ceil(period / dt_target))
    return norbit, period / norbit, -0.04432 * TWO_PI / period


def tdf_slot(istep: int, norbit: int) -> int:
    """Ring slot read and written at step ``istep`` (1-based): it holds the flow of step
    istep - norbit, the reference's ``uor(:, 1)`` after istep - norbit - 1 shifts (:77-90)."""
    if istep < 1:
        raise ValueError("istep >= 1")
    return (istep - 1) % norbit


def tdf_converged(l2: float, tol: float) -> bool:
    """``l2 > 0 .and. l2 < tol`` (:105)."""
    return 0.0 < l2 < tol


def fortran_e(x: float, width: int = 15, digits: int = 7) -> str:
    """One Fortran ``E15.7`` field: 0.dddddddE+ee, right-justified (the exponent letter is dropped for
    three-digit exponents, as the standard prescribes)."""
    x = float(x)
    if x != x:
        return "NaN".rjust(width)
    if math.isinf(x):
        return ("-Infinity" if x < 0 else "Infinity").rjust(width)
    mant, exp = f"{abs(x):.{digits - 1}E}".split("E")   # d.dddddd, correctly rounded
    e = 0 if x == 0 else int(exp) + 1
    s = ("-" if math.copysign(1.0, x) < 0 else "") + "0." + mant.replace(".", "")
    s += f"E{e:+03d}" if abs(e) < 100 else f"{e:+04d}"
    return s.rjust(width) if len(s) <= width else "*" * width


def residu_line(*values: float) -> str:
    """One ``residu.dat`` record: ``(4E15.7)`` time, res, rate, param(21) for SFD (:191),
    ``(3E15.7)`` time, l2, rate for TDF (:99)."""
    return "".join(fortran_e(v) for v in values)


# ---- device classes -------------------------------------------------------------------------------

def _volume(ctx: NekContext) -> float:
    """All-reduced sum of the context's weights (Nek5000's volvm1 when they are bm1)."""
    t = ctx.w.sum().reshape(1)
    ctx.comm.allreduce_(t)
    return float(t.item())


def _refuse_pair(ctx: NekContext, what: str) -> None:
    if isinstance(ctx.layout, PairLayout):
        raise ValueError(f"{what} forces a real flow: a PairLayout (re/im pair) context is refused")


class _ResiduFile:
    """``open (unit=10, file='residu.dat')`` on rank 0 (:52, :146, :180)."""

    def __init__(self, ctx: NekContext, path):
        self.fh = open(path, "w") if (path is not None and ctx.comm.rank == 0) else None

    def write(self, *values: float) -> None:
        if self.fh is not None:
            self.fh.write(residu_line(*values) + "\n")
            self.fh.flush()

    def close(self) -> None:
        if self.fh is not None:
            self.fh.close()
            self.fh = None


class SFD:
    """Selective frequency damping (fixedp.f90:124-216) of the flow held in a :class:`NekVector`.

    ``uparam4`` / ``uparam5``: Strouhal number and growth rate (:134-145; uparam5 <= 0: monitor
    mode, the reference's continuation branch — no filter, no forcing, only the residual);
    ``dt``: the time step; ``tol``: ``max(param(21), param(22))`` (:149); ``volume``: the domain
    volume ``volvm1`` of ``normvc``, default the all-reduced sum of the context's weights (exact when
    they are ``bm1``; with sponge-zeroed ``bm1s`` pass the full volume: ``Sponge.volume``).  ``normvc`` is Nek5000's, not
    part of the reference tree: its l2 is sqrt(sum_c glsc3(u_c, bm1, u_c) / volvm1) over the
    velocities, which is what ``step`` returns with the context's weights.  ``residu``: a path for the
    ``residu.dat`` records (rank 0).  ``monitors``: callables ``m(v, istep, time)`` run at the end of
    every step, e.g. ``vortex.EnergyMonitor`` / ``vortex.EnstrophyMonitor`` (the reference calls
    ``nekStab_energy`` / ``nekStab_enstrophy`` from every step, main.f90:152-163); default none, and
    then nothing changes.

    The time slots of the internal vectors are never touched (the reference's ``oldQ%time`` etc. are
    never set either).
    """

    def __init__(self, ctx: NekContext, uparam4: float, uparam5: float, dt: float, tol: float,
                 volume: float | None = None, min_steps: int = 100, residu=None, monitors=()):
        _refuse_pair(ctx, "SFD")
        self.ctx = ctx
        self.monitors = tuple(monitors)   # called as m(v, istep, time) after every step (main.f90:152-163)
        self.monitor = sfd_is_monitor(uparam5)
        self.cutoff, self.gain = sfd_coefficients(uparam4, uparam5)
        self.dt, self.tol, self.min_steps = float(dt), float(tol), int(min_steps)
        self.volume = _volume(ctx) if volume is None else float(volume)
        self.n_vel = ctx.layout.ldim
        self.v_old = ctx.vector()
        if not self.monitor:
            self.qbar = ctx.vector()                                  # oldQ: the filtered flow
            self._q = [ctx.vector(), ctx.vector(), ctx.vector()]      # qa, qb, qc (rotated, never copied)
        self._res2 = torch.zeros(1, dtype=torch.float64, device=ctx.device)
        self.istep = 0
        self.old_res = 0.0
        self.res2 = 0.0
        self._file = _ResiduFile(ctx, residu)

    def start(self, v: NekVector) -> None:
        """istep == 0 (:148-155): qa = qb = qc = 0, oldQ = oldV = v.  (The forcing the reference adds
        at this step, gain (oldV - oldQ), is exactly zero.)"""
        self.v_old.copy_from(v, time=False)
        if not self.monitor:
            self.qbar.copy_from(v, time=False)
            for q in self._q:
                q.zero()
        self.istep = 0
        self.old_res = 0.0

    def step(self, v: NekVector, fc: NekVector | None, ab=None, time: float | None = None):
        """One call of SFD at the next istep >= 1: updates the filter state and adds the forcing to
        ``fc`` (not in monitor mode, where ``fc`` may be None); returns ``(res, rate, converged)``
        with res = sqrt(allreduce(res2) / volume), rate = (res - old_res) / dt (:188) and
        converged = istep > min_steps and res < tol (:201).  ``ab``: explicit (adt, bdt, cdt) of
        ``setab3``, default :func:`ab3_coefficients`.  Synchronises the stream (res is a host value)."""
        ctx = self.ctx
        self.istep += 1
        adt, bdt, cdt = ab3_coefficients(self.istep) if ab is None else ab
        w, ws, st = ctx.w.data_ptr(), ctx.ws.data_ptr(), ctx.stream
        if self.monitor:
            ctx.call("nkv_sfd_step", w, v.ptr, self.v_old.ptr, None, None, None, None, None, 0.0, 0.0, 0.0, 0.0, 0.0,
                     self.n_vel, self._res2.data_ptr(), ws, _lib.NKV_SFD_MONITOR, st)
        else:
            if fc is None:
                raise ValueError("SFD.step needs the forcing vector fc")
            qa, qb, qc = self._q
            ctx.call("nkv_sfd_step", w, v.ptr, self.v_old.ptr, self.qbar.ptr, qa.ptr, qb.ptr, qc.ptr, fc.ptr,
                     float(adt), float(bdt), float(cdt), self.cutoff * self.dt, self.gain, self.n_vel,
                     self._res2.data_ptr(), ws, 0, st)
            self._q = [qc, qa, qb]   # qc <- qb <- qa <- d
        ctx.comm.allreduce_(self._res2)
        self.res2 = float(self._res2.item())
        if self.res2 != self.res2:
            ctx.check_nan()
        res = math.sqrt(self.res2 / self.volume)
        rate = (res - self.old_res) / self.dt
        self.old_res = res
        self._file.write(self.istep * self.dt if time is None else time, res, rate, self.tol)
        for m in self.monitors:
            m(v, self.istep, self.istep * self.dt if time is None else time)
        return res, rate, sfd_converged(self.istep, res, self.tol, self.min_steps)

    def close(self) -> None:
        self._file.close()


class TDF:
    """Time-delayed feedback (fixedp.f90:2-121): fc += gain (v(t) - v(t - T)) on the velocities.

    ``period``: the orbit's period 1/uparam(5) (:20); ``dt_target``: the CFL time step (:22-23);
    norbit, ``dt`` (the caller must step with it) and the gain follow :func:`tdf_parameters`.  The
    orbit history is a :class:`Basis` of norbit slots used as a ring (:func:`tdf_slot`) instead of
    the reference's shifted arrays.  ``volume``, ``residu`` and ``monitors`` as for :class:`SFD`.

    The reference computes l2 only from step norbit + 2 on but its ``rate = l2 - residu0`` runs at
    norbit + 1 on an undefined l2 (:72: the ``if`` guards the ``call normvc`` alone); here the
    residual is computed from the first forcing step on.
    """

    def __init__(self, ctx: NekContext, period: float, dt_target: float, tol: float, volume: float | None = None,
                 residu=None, monitors=()):
        _refuse_pair(ctx, "TDF")
        self.ctx = ctx
        self.monitors = tuple(monitors)   # called as m(v, istep, time) after every step (main.f90:152-163)
        self.period = float(period)
        self.norbit, self.dt, self.gain = tdf_parameters(period, dt_target)
        self.tol = float(tol)
        self.volume = _volume(ctx) if volume is None else float(volume)
        self.n_vel = ctx.layout.ldim
        self.ring = ctx.basis(self.norbit)
        self._res2 = torch.zeros(1, dtype=torch.float64, device=ctx.device)
        self.istep = 0
        self.residu0 = 0.0
        self.res2 = 0.0
        self._file = _ResiduFile(ctx, residu)

    def step(self, v: NekVector, fc: NekVector, time: float | None = None):
        """One call of TDF at the next istep >= 1.  The first norbit steps store the flow (:58-67) and
        return (0.0, 0.0, False); after that the forcing is added to ``fc`` and ``(l2, rate,
        converged)`` returned, rate = l2 - previous l2 (:72), converged = 0 < l2 < tol (:105)."""
        ctx = self.ctx
        self.istep += 1
        slot = self.ring.col_ptr(tdf_slot(self.istep, self.norbit))
        w, ws, st = ctx.w.data_ptr(), ctx.ws.data_ptr(), ctx.stream
        if self.istep <= self.norbit:
            ctx.call("nkv_tdf_step", w, v.ptr, slot, None, 0.0, self.n_vel, self._res2.data_ptr(), ws,
                     _lib.NKV_TDF_STORE, st)
            self._monitor(v, time)
            return 0.0, 0.0, False
        ctx.call("nkv_tdf_step", w, v.ptr, slot, fc.ptr, self.gain, self.n_vel, self._res2.data_ptr(), ws, 0, st)
        ctx.comm.allreduce_(self._res2)
        self.res2 = float(self._res2.item())
        if self.res2 != self.res2:
            ctx.check_nan()
        l2 = math.sqrt(self.res2 / self.volume)
        rate = l2 - self.residu0
        self.residu0 = l2
        self._file.write(self.istep * self.dt if time is None else time, l2, rate)
        self._monitor(v, time)
        return l2, rate, tdf_converged(l2, self.tol)

    def _monitor(self, v: NekVector, time: float | None) -> None:
        for m in self.monitors:
            m(v, self.istep, self.istep * self.dt if time is None else time)

    def close(self) -> None:
        self._file.close()


__all__ = ["SFD", "TDF", "sfd_coefficients", "ab3_coefficients", "sfd_is_monitor", "sfd_converged",
           "tdf_parameters", "tdf_slot", "tdf_converged", "fortran_e", "residu_line"]
