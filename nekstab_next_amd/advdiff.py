"""A spectral-element advection-diffusion propagator and its adjoint: the first operator of the package
whose matvec is a time integration over the GLL mesh.

Reference: LightKrylov's ``abstract_linop`` / nekStab's ``exponential_prop`` (core/linear_operators.f90:
17-23, 39-103), whose ``matvec`` / ``rmatvec`` advance the direct / adjoint equations over ``tau`` with
Nek5000.  The Navier–Stokes stepper and its pressure projection are Nek5000's and stay out;
this is the equation Nek5000 advances for a passive scalar (``ifheat``, ``t``): every weighted field of the
layout (``vx, vy, [vz], t…``) is advected by a frozen base flow ``U`` and diffused with its own ``kappa``,
independently of the others.  It couples the elements through direct-stiffness averaging and is non-normal,
so it exercises ``krylov_schur``, ``eigs``, ``svds``, ``transient_growth_analysis``, GMRES and
``LegacyMatvec`` the way a real stepper does.

With ``r`` the local weak-form right-hand side (``nkv_advdiff_rhs``, include/nekkrylov.h: forward or
adjoint), ``bm1`` the mass matrix and ``dsavg`` the direct-stiffness average,

    L u  = minv · dsavg(r(u)),          minv = mask / dsavg(bm1)        (Nek's binvm1 · dssum, by dsavg)
    Π x  = minv · dsavg(bm1 · x)                                        (the projector)
    matvec:  y = p(dt L)^nsteps Π x,    rmatvec:  y = p(dt L†)^nsteps Π x
    p(z) = 1 + z + z²/2 + z³/6 + z⁴/24  (RK4 of a linear autonomous system), in Horner form:
           w ← v + (dt / s) L w  for s = 4, 3, 2, 1 from w = v.

Π is the bm1-orthogonal projector onto the continuous fields that vanish where ``mask`` is 0; without it
every discontinuous component of a seed would be an eigenvector of eigenvalue exactly 1.  ``matvec`` and
``rmatvec`` are adjoints of each other to rounding, for arbitrary (unprojected) vectors, in the inner
product weighted by ``op.bm1``: build the context as ``NekContext(lay, weights=op.bm1)``.  A weight that a
sponge has zeroed (``forcing.Sponge``, forcing.f90:101-104) is another inner product and breaks the
identity.  The explicit step is stable for ``dt · ρ(L) ≲ 2.78`` (RK4's limit on the imaginary axis is
2.83, on the negative real axis 2.78).

Each Horner pass is one right-hand-side launch, one ``dsavg`` batch of the ``n_wf`` segments
(``gs.average_segments``) and one fused stage launch (``nkv_advdiff_stage``); nothing synchronises with the
host and the two work vectors are allocated once.
"""
from __future__ import annotations

import numpy as np
import torch

from .gs import auto_average, average_segments
from .operators import LinearOperator
from .sensitivity import gll_derivative
from .synthetic import gll_weights
from .vector import NekContext, NekVector

_NAMES = ("x", "y", "z")


def box_boundary_mask(coords: dict, comm=None, rel_tol: float = 1e-9, device=None) -> np.ndarray:
    """A Dirichlet mask for a box: 0 on the faces of the bounding box of the mesh, 1 elsewhere (one value
    per point of this rank).  The extents are all-reduced over ``comm`` as ``GatherScatter`` reduces its
    own, so every rank masks the faces of the whole mesh, not of its shard (collective when given)."""
    xs = [np.asarray(coords[k], dtype=np.float64).ravel() for k in _NAMES if k in coords]
    lo = [float(x.min()) if x.size else np.inf for x in xs]
    hi = [float(x.max()) if x.size else -np.inf for x in xs]
    if comm is not None and comm.world > 1:
        lo = [comm.min_scalar(v, device=device) for v in lo]
        hi = [comm.max_scalar(v, device=device) for v in hi]
    ext = max([h - l for l, h in zip(lo, hi) if h >= l] or [0.0])
    tol = rel_tol * (ext or 1.0)
    mask = np.ones(xs[0].size)
    for x, l, h in zip(xs, lo, hi):
        mask[(np.abs(x - l) <= tol) | (np.abs(x - h) <= tol)] = 0.0
    return mask


def mask_from_faces(lay, faces) -> np.ndarray:
    """A Dirichlet mask from a face table: 0 on every GLL point of the ``(global element, face)`` pairs of
    ``monitors.wall_faces`` (0-based elements, preprocessor face numbers), 1 elsewhere.  Members outside
    this rank's element range are skipped.  A wall point that another element touches only along an edge
    or at a vertex is not in that element's faces: pass the mask through ``dsavg`` and floor it, or let the
    operator do so (it masks a point when any of its copies is masked)."""
    from .monitors import face_points

    e0, e1 = lay.elem_range()
    mask = np.ones(lay.n_v).reshape(lay.nelv, lay.pts_v)
    for eg, fc in faces:
        if e0 <= int(eg) < e1:
            mask[int(eg) - e0, face_points(lay.lx1, lay.ldim, int(fc))] = 0.0
    return mask.reshape(-1)


class AdvectionDiffusion(LinearOperator):
    """``y = p(dt L)^nsteps Π x`` and its adjoint (module docstring).

    ``coords``: this rank's GLL coordinates {"x", "y"[, "z"]} (n_v each).  ``base``: the frozen flow, a
    :class:`NekVector` (its velocity rows are copied) or ldim arrays of n_v values.  ``kappa``: one
    diffusivity, or one per weighted field.  ``mask``: n_v values, 0 on Dirichlet points (default: natural
    boundaries); a point is masked when any of its coincident copies is (on any rank).  ``face_average``: ``"auto"``
    (``gs.auto_average``: ``FaceAverage`` on one rank, a ``GatherScatter`` over the shards on several), a
    ``GatherScatter`` or a callable ``f(ptr)`` averaging one segment in place.

    ``op.bm1`` is the mass matrix on the device (n_v values): the weights of the inner product in which
    ``rmatvec`` is the adjoint of ``matvec``.  ``op.tau = nsteps · dt``."""

    def __init__(self, ctx: NekContext, coords: dict, base, kappa, dt: float, nsteps: int, mask=None,
                 face_average="auto"):
        lay = ctx.layout
        n, d, sv, nf = lay.n_v, lay.ldim, lay.sv, lay.n_wf
        if nsteps < 1 or not dt > 0.0:
            raise ValueError(f"dt={dt}, nsteps={nsteps}: need dt > 0 and nsteps >= 1")
        self.ctx, self.dt, self.nsteps = ctx, float(dt), int(nsteps)
        self.tau = self.nsteps * self.dt
        f64 = dict(dtype=torch.float64, device=ctx.device)

        def dev(a, what):
            a = np.asarray(a, dtype=np.float64).ravel()
            if a.size != n:
                raise ValueError(f"{what}: {a.size} points, the layout has n_v={n}")
            return torch.as_tensor(a).to(ctx.device) if n else torch.zeros(2, **f64)

        self.D = torch.as_tensor(gll_derivative(lay.lx1)).to(ctx.device)
        self.w = torch.as_tensor(gll_weights(lay.lx1)).to(ctx.device)
        self.xyz = [dev(coords[k], f"coords[{k!r}]") for k in _NAMES[:d]]
        self.U = torch.zeros(d * max(sv, 2), **f64)
        if isinstance(base, NekVector):
            self.U[: d * sv].copy_(base.storage[: d * sv])
        else:
            if len(base) != d:
                raise ValueError(f"base: {len(base)} components, the layout has ldim={d}")
            for c in range(d):
                self.U[c * sv: c * sv + n] = dev(base[c], f"base[{c}]")[:n]
        k = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (nf,)) if np.ndim(kappa) == 0 else \
            np.asarray(kappa, dtype=np.float64).ravel()
        if k.size != nf or not np.all(np.isfinite(k)) or np.any(k < 0.0):
            raise ValueError(f"kappa: one non-negative value, or one per weighted field ({nf})")
        self.kappa = torch.as_tensor(np.ascontiguousarray(k)).to(ctx.device)
        self.face_average = auto_average(ctx, coords) if isinstance(face_average, str) else face_average
        if isinstance(face_average, str) and face_average != "auto":
            raise ValueError("face_average: 'auto', a GatherScatter or a callable f(ptr)")
        # the two work vectors of a step (n_wf segments each) and the pointwise operands, allocated once
        self._r = torch.zeros(nf * sv + 2, **f64)
        self._w = torch.zeros(nf * sv + 2, **f64)
        self._bm1 = torch.zeros(max(n, 2), **f64)
        self.bm1 = self._bm1[:n]
        ctx.call("nkv_advdiff_bm1", lay.lx1, d, self.D.data_ptr(), self.w.data_ptr(), *self._xyz_ptrs(),
                 self._bm1.data_ptr(), ctx.stream)
        den = self._bm1.clone()
        average_segments(self.face_average, [den.data_ptr()])
        m = torch.ones(max(n, 2), **f64)
        if mask is not None:   # (every rank passes a mask or none does: the average is collective)
            m[:n] = dev(mask, "mask")[:n]
            average_segments(self.face_average, [m.data_ptr()])
            m = (m > 0.95).to(torch.float64)   # one masked copy among k <= 8 lowers the mean to <= 7/8
        self.mask = m[:n]
        self._minv = m / den if n else m
        self.minv = self._minv[:n]

    # ---- plumbing ----
    def _xyz_ptrs(self):
        p = [t.data_ptr() for t in self.xyz]
        return p + [None] if len(p) == 2 else p

    def _average(self, t: torch.Tensor) -> None:
        sv = self.ctx.layout.sv
        average_segments(self.face_average, [t.data_ptr() + 8 * f * sv for f in range(self.ctx.layout.n_wf)])

    def _local_rhs(self, u_ptr: int, adjoint: bool) -> None:
        """r <- the local right-hand side of the n_wf fields at ``u_ptr`` (segments of sv), then its dsavg."""
        ctx, lay = self.ctx, self.ctx.layout
        ctx.call("nkv_advdiff_rhs", lay.lx1, lay.ldim, self.D.data_ptr(), self.w.data_ptr(), *self._xyz_ptrs(),
                 self.U.data_ptr(), lay.sv, self.kappa.data_ptr(), u_ptr, lay.n_wf, lay.sv, self._r.data_ptr(), lay.sv,
                 int(adjoint), ctx.stream)
        self._average(self._r)

    def _stage(self, v_ptr, m: torch.Tensor, r_ptr: int, c: float, w_ptr: int, zero_rest: bool = False) -> None:
        ctx, lay = self.ctx, self.ctx.layout
        ctx.call("nkv_advdiff_stage", v_ptr, lay.sv, m.data_ptr(), r_ptr, lay.sv, float(c), w_ptr, lay.sv, lay.n_wf,
                 int(zero_rest), ctx.stream)

    # ---- the operator ----
    def rhs(self, x: NekVector, y: NekVector, adjoint: bool = False) -> None:
        """One application of the generator: ``y = L x`` (``L†`` if ``adjoint``) on the weighted fields, for
        tests and for callers with their own integrator.  ``x`` is taken as it is (not projected); pressure
        and time of ``y`` are zeroed."""
        self._local_rhs(x.ptr, adjoint)
        self._stage(None, self._minv, self._r.data_ptr(), 1.0, y.ptr, zero_rest=True)

    def project(self, x: NekVector, y: NekVector | None = None) -> NekVector:
        """``y = Π x`` (in place when ``y`` is None); pressure and time of ``y`` are zeroed."""
        y = x if y is None else y
        self._stage(None, self._bm1, x.ptr, 1.0, self._r.data_ptr())
        self._average(self._r)
        self._stage(None, self._minv, self._r.data_ptr(), 1.0, y.ptr, zero_rest=True)
        return y

    def _propagate(self, x: NekVector, y: NekVector, adjoint: bool) -> None:
        self.project(x, y)
        rp, wp = self._r.data_ptr(), self._w.data_ptr()
        for _ in range(self.nsteps):
            src = y.ptr
            for s in (4, 3, 2):
                self._local_rhs(src, adjoint)
                self._stage(y.ptr, self._minv, rp, self.dt / s, wp)
                src = wp
            self._local_rhs(src, adjoint)
            self._stage(y.ptr, self._minv, rp, self.dt, y.ptr, zero_rest=True)

    def matvec(self, x: NekVector, y: NekVector) -> None:
        self._propagate(x, y, False)

    def rmatvec(self, x: NekVector, y: NekVector) -> None:
        self._propagate(x, y, True)


__all__ = ["AdvectionDiffusion", "box_boundary_mask", "mask_from_faces"]
