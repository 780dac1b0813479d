"""NumPy restatement of the time-periodic Burgers flow of ``nekstab_next_amd.orbit`` (nkv_burgers_tangent_rhs,
nkv_orbit_stage; csrc/advdiff.hip), built on ``burgers_reference.Burgers``: the oracle of its tests.

One period is T = nsteps dt; step n starts at t_n = n dt.  With N0 the unforced generator of ``Burgers``:

    g(t)   = g0 + cos(w t) gc + sin(w t) gs,  w = 2 pi / T         (each part projected once; each may be absent)
    stages   s1 = v, s2 = v + dt/2 k1, s3 = v + dt/2 k2, s4 = v + dt k3,  k_i = N0(s_i) + g(t_n + th_i dt),
             th = (0, 1/2, 1/2, 1);   v' = v + dt/6 k1 + dt/3 k2 + dt/3 k3 + dt/6 k4
    tangent  K1 = L_s1 v, K2 = L_s2(v + dt/2 K1), K3 = L_s3(v + dt/2 K2), K4 = L_s4(v + dt K3),
             y = v + dt/6 K1 + dt/3 K2 + dt/3 K3 + dt/6 K4       (the exact Jacobian of the discrete step)
    adjoint  u4 = l, u3 = l + dt/2 L+_s4 u4, u2 = l + dt/2 L+_s3 u3, u1 = l + dt L+_s2 u2,
             y = l + dt/6 L+_s4 u4 + dt/3 L+_s3 u3 + dt/3 L+_s2 u2 + dt/6 L+_s1 u1;  steps nsteps-1 down to 0
    Phi_T(q) = RK4^nsteps(Pi q);  P = d Phi_T / dq = (product of the step Jacobians) Pi

The phase of a stage is formed in f64 as ``2.0 * pi * (n + th) / nsteps`` and its cos / sin are taken in f64, as
the host of the device code does, then cast to ``dtype``: both precisions see the same forcing coefficients.

Records of tests/test_orbit.py on the end-to-end case (``e2e_case``), which holds each to 8 times these:"""
import math

import numpy as np

import advdiff_reference as ar
import burgers_reference as br

FD_LINEARISATION = 4.7e-8      # |central difference of Phi_T - P v| relative, eps = 1e-4 (truncation, O(eps^2))
DENSE_TRANSPOSE = 2.5e-15      # max |M P - (M P^+)^T| over the largest entry of M P
# the dense Newton's ||F||^2 history from Pi target, and its quadratic constant: ||F_k+1|| <= C ||F_k||^2, so
# r[k+1] <= C^2 r[k]^2 on r = ||F||^2; r[k+1] / r[k]^2 = 0.221, 13.26, 6.35 while r[k] > 1e-12: C = sqrt(13.26)
NEWTON_HISTORY = (7.3036e-3, 1.18e-5, 1.85e-9, 2.2e-17, 8e-31)
NEWTON_C = 3.65
MULTIPLIERS = (1.146982082393, complex(1.058001193650, 0.357999727895))
FROZEN_BASE_MULTIPLIER = 1.14385384
GAIN = 2.199205061548

PI = np.pi
THETA = (0.0, 0.5, 0.5, 1.0)


def phase(n, theta, nsteps):
    """(cos, sin) of the phase of stage time t_n + theta dt, in f64: the host side of nkv_orbit_stage."""
    ph = 2.0 * math.pi * (n + theta) / nsteps
    return math.cos(ph), math.sin(ph)


class Orbit:
    """The harmonic forcing, the step with its stages, the tangent and adjoint steps and their dense forms on top
    of a ``Burgers`` (whose own constant forcing is not used).  States: (n_wf, n_v)."""

    def __init__(self, bg: br.Burgers, g0=None, gc=None, gs=None):
        self.bg, self.dtype, self.nsteps, self.dt = bg, bg.dtype, bg.nsteps, bg.dt
        self.g0, self.gc, self.gs = (None if g is None else bg.project(g) for g in (g0, gc, gs))

    def steady_g0(self, q_target):
        """g0 = -N0(Pi q_target); returns Pi q_target."""
        qt = self.bg.project(q_target)
        self.g0 = -self.bg.N0(qt)
        return qt

    # ---- the forced generator: m r, + g0, + c gc, + s gs, in this order ----
    def k(self, s, n, theta):
        k = self.bg.N0(s)
        c, sn = phase(n, theta, self.nsteps)
        if self.g0 is not None:
            k = k + self.g0
        if self.gc is not None:
            k = k + self.dtype(c) * self.gc
        if self.gs is not None:
            k = k + self.dtype(sn) * self.gs
        return k

    def _ab(self):
        dt, t = self.dt, self.dtype
        return (dt / t(2), dt / t(2), dt), (dt / t(6), dt / t(3), dt / t(3), dt / t(6))

    def step(self, v, n):
        """(v', [s1, s2, s3, s4]) of step n."""
        a, b = self._ab()
        s, stages, acc = v, [], v
        for i in range(4):
            stages.append(s)
            k = self.k(s, n, THETA[i])
            acc = acc + b[i] * k
            if i < 3:
                s = v + a[i] * k
        return acc, stages

    def propagate(self, q):
        """(Phi_T(q), the stage states [nsteps][4])."""
        v = self.bg.project(q)
        orbit = []
        for n in range(self.nsteps):
            v, st = self.step(v, n)
            orbit.append(st)
        return v, orbit

    def time_derivative(self, q, step=0):
        """(one RK4 step from q at t_step - q) / dt: compute_bvec."""
        q = np.asarray(q).astype(self.dtype)
        return (self.step(q, step)[0] - q) / self.dt

    # ---- the tangent and the adjoint of one step ----
    def tangent_step(self, stages, v):
        a, b = self._ab()
        L = self.bg.L
        u, acc = v, v
        for i in range(4):
            kap = L(u, stages[i])
            acc = acc + b[i] * kap
            if i < 3:
                u = v + a[i] * kap
        return acc

    def adjoint_step(self, stages, lam):
        a, b = self._ab()
        L = self.bg.L
        u, acc = lam, lam
        for i, (ai, bi) in zip((3, 2, 1, 0), ((a[0], b[0]), (a[1], b[1]), (a[2], b[2]), (None, b[3]))):
            kap = L(u, stages[i], adjoint=True)
            acc = acc + bi * kap
            if ai is not None:
                u = lam + ai * kap
        return acc

    def tangent(self, x, orbit):
        v = self.bg.project(x)
        for st in orbit:
            v = self.tangent_step(st, v)
        return v

    def adjoint(self, x, orbit):
        v = self.bg.project(x)
        for st in reversed(orbit):
            v = self.adjoint_step(st, v)
        return v

    # ---- dense forms on the free unique points x n_wf ----
    def dense_step(self, stages, adjoint=False):
        a, b = self._ab()
        J = [self.bg.dense(s, adjoint) for s in stages]
        I = np.eye(J[0].shape[0], dtype=self.dtype)
        if not adjoint:
            U, S = I, I
            for i in range(4):
                K = J[i] @ U
                S = S + b[i] * K
                if i < 3:
                    U = I + a[i] * K
            return S
        U, S = I, I
        for i, (ai, bi) in zip((3, 2, 1, 0), ((a[0], b[0]), (a[1], b[1]), (a[2], b[2]), (None, b[3]))):
            K = J[i] @ U
            S = S + bi * K
            if ai is not None:
                U = I + ai * K
        return S

    def monodromy(self, orbit, adjoint=False):
        """The product of the dense step Jacobians (adjoint: of their adjoints, last step first)."""
        P = None
        for st in (reversed(orbit) if adjoint else orbit):
            S = self.dense_step(st, adjoint)
            P = S if P is None else S @ P
        return P

    def newton(self, q0, maxiter=8, tol=1e-20):
        """Dense Newton on F(q) = Phi_T(q) - q over the free unique points with the exact monodromy; returns
        (q, the history of ||F||^2 in the bm1 inner product)."""
        bg = self.bg
        c = bg.restrict(bg.project(q0))
        M = bg.mass()
        hist = []
        for _ in range(maxiter):
            q = bg.expand(c)
            phi, orbit = self.propagate(q)
            F = bg.restrict(phi) - c
            hist.append(float(np.sum(M * F * F)))
            if hist[-1] < tol:
                break
            J = self.monodromy(orbit).astype(np.float64) - np.eye(c.size)
            c = c - np.linalg.solve(J, F.astype(np.float64)).astype(self.dtype)
        return bg.expand(c), hist


# ---- the end-to-end case -----------------------------------------------------------------------------
E2E = dict(lx1=5, ne=(2, 2), kappa=(0.05, 0.03), dt=0.05, nsteps=20)


def e2e_mesh():
    co = ar.box_mesh_2d(5, (2, 2), (PI, PI), amp=0.04)
    return co, ar.box_mask(ar.box_mesh_2d(5, (2, 2), (PI, PI)))


def e2e_forcing(co):
    """(target, gc, gs) before projection."""
    x, y = co["x"], co["y"]
    target = np.stack([np.sin(x) * np.sin(2 * y), -0.7 * np.sin(2 * x) * np.sin(y)])
    gc = 0.5 * np.stack([np.sin(2 * x) * np.sin(y), np.sin(x) * np.sin(3 * y)])
    gs = 0.3 * np.stack([np.sin(x) * np.sin(y), np.sin(2 * x) * np.sin(2 * y)])
    return target, gc, gs


def e2e_case(dtype=np.float64, nsteps=None):
    """(coords, mask, Orbit, Pi target, target, gc, gs) of the 2-D case: lx1 = 5, 2 x 2 elements of [0, pi]^2
    deformed by 0.04, walls of the undeformed box, layout (vx, vy), T = nsteps dt = 1."""
    co, mask = e2e_mesh()
    x = co["x"]
    ref = ar.Reference(5, 2, co, [np.zeros_like(x), np.zeros_like(x)], mask=mask, dtype=dtype)
    bg = br.Burgers(ref, E2E["kappa"], E2E["dt"], E2E["nsteps"] if nsteps is None else nsteps)
    target, gc, gs = e2e_forcing(co)
    ob = Orbit(bg, gc=gc, gs=gs)
    qt = ob.steady_g0(target)
    return co, mask, ob, qt, target, gc, gs
