"""NumPy restatement of the viscous Burgers flow of ``nekstab_next_amd.burgers`` (nkv_linconv_rhs,
nkv_rk4_stage; csrc/advdiff.hip), built on ``advdiff_reference.Reference``: the oracle of its tests.

States are stacks of the ``n_wf`` weighted fields, shape (n_wf, [batch,] n_v); the first ``ldim`` are the
velocity.  With ``r(q; U)`` the forward local right-hand side of ``Reference.local_rhs``:

    N(q)    = minv dsavg(r(q; U = q_vel)) + g
    L_B u   = minv dsavg(r_fwd),   r_fwd,f = r_f(u; U = B_vel)     - bm1 sum_{d<ldim} u_d d_d B_f
    L_B^+ u = minv dsavg(r_adj),   r_adj,f = r_adj,f(u; U = B_vel) - [f < ldim] bm1 sum_{f'<n_wf} u_f' d_f B_f'
    Phi(q)  = RK4^nsteps(Pi q)     (classical: k = N(s); s' = v + a k; acc' = acc + b k)
    P x     = p(dt L_B)^nsteps Pi x   (Horner, as Reference.propagate)

Everything runs in the ``dtype`` of the ``Reference`` from the same f64-rounded inputs, so the distance between
the ``np.float64`` and the ``np.longdouble`` run is the restatement's own rounding error.

Records of tests/test_burgers.py on the end-to-end case (``e2e_case``), which holds each to 8 times these:"""
import numpy as np

import advdiff_reference as ar

DENSE_TRANSPOSE = 3.9e-16     # max |M J - (M J^+)^T| over the largest entry of M J
FD_LINEARISATION = 6.2e-14    # |central difference of N - L_B v| relative, eps = 1e-3

PI = np.pi


class Burgers:
    def __init__(self, ref: ar.Reference, kappa, dt=None, nsteps=None, forcing=None):
        self.ref, self.dtype, self.ldim = ref, ref.dtype, ref.ldim
        self.kappa = [float(k) for k in kappa]
        self.nf = len(self.kappa)
        self.dt = None if dt is None else self.dtype(dt)
        self.nsteps = nsteps
        self.g = self.dtype(0.0) if forcing is None else self.project(forcing)

    # ---- plumbing ----
    def _cast(self, q):
        return np.asarray(q).astype(self.dtype)

    def _tile(self, a):
        return a.reshape(a.shape[:-1] + self.ref.bm1_t.shape)

    def _advect_by(self, B):
        """The frozen flow of the Reference <- the velocity rows of B (one state, no batch axes)."""
        self.ref.U = [self._cast(B[d]).reshape(self.ref.shp) for d in range(self.ldim)]

    def project(self, x):
        return self.ref.project(self._cast(x))

    def assemble(self, r):
        return self.ref.minv * self.ref.dsavg(r)

    # ---- the nonlinear generator ----
    def N0(self, q):
        """The unforced generator; q: (n_wf, n_v)."""
        q = self._cast(q)
        self._advect_by(q)
        return self.assemble(np.stack([self.ref.local_rhs(q[f], self.kappa[f]) for f in range(self.nf)]))

    def N(self, q):
        return self.N0(q) + self.g

    def steady_forcing(self, q_target):
        """g = -N0(Pi q_target); returns Pi q_target, then an exact steady state."""
        qt = self.project(q_target)
        self.g = -self.N0(qt)
        return qt

    # ---- the linearisation and its adjoint ----
    def local(self, u, B, adjoint=False):
        """The unassembled coupled right-hand side; u: (n_wf, [batch,] n_v), B: (n_wf, n_v)."""
        u, B = self._cast(u), self._cast(B)
        ref, d = self.ref, self.ldim
        self._advect_by(B)
        gB = [ref.grad(B[f]) for f in range(self.nf)]           # gB[f][d]: tiles
        ut = [self._tile(u[f]) for f in range(self.nf)]
        out = []
        for f in range(self.nf):
            r = ref.local_rhs(u[f], self.kappa[f], adjoint)
            if not adjoint:
                prod = sum(ut[c] * gB[f][c] for c in range(d))
            elif f < d:
                prod = sum(ut[fp] * gB[fp][f] for fp in range(self.nf))
            else:
                prod = None
            if prod is not None:
                r = r - (ref.bm1_t * prod).reshape(u[f].shape)
            out.append(r)
        return np.stack(out)

    def L(self, u, B, adjoint=False):
        return self.assemble(self.local(u, B, adjoint))

    # ---- time stepping ----
    def step(self, v):
        dt = self.dt
        two, three, six = self.dtype(2), self.dtype(3), self.dtype(6)
        k = self.N(v)
        acc = v + dt / six * k
        k = self.N(v + dt / two * k)
        acc = acc + dt / three * k
        k = self.N(v + dt / two * k)
        acc = acc + dt / three * k
        k = self.N(v + dt * k)
        return acc + dt / six * k

    def propagate(self, q):
        """Phi(q) = RK4^nsteps(Pi q)."""
        v = self.project(q)
        for _ in range(self.nsteps):
            v = self.step(v)
        return v

    def propagate_lin(self, x, B, adjoint=False):
        """p(dt L_B)^nsteps Pi x in Horner form."""
        v = self.project(x)
        for _ in range(self.nsteps):
            w = v
            for s in (4, 3, 2, 1):
                w = v + self.dt / self.dtype(s) * self.L(w, B, adjoint)
            v = w
        return v

    # ---- dense forms on the free unique points x n_wf (field-major) ----
    def expand(self, c):
        """(n_wf, n_v) continuous fields from (n_wf * n_free) coefficients."""
        return self.ref.expand(np.asarray(c).reshape(self.nf, -1))

    def restrict(self, q):
        return self.ref.restrict(q).reshape(-1)

    def dense(self, B, adjoint=False):
        ref, nf = self.ref, self.nf
        m = ref.free.size
        nodal = ref.expand(np.eye(m, dtype=self.dtype))          # (m, n_v)
        J = np.zeros((nf * m, nf * m), dtype=self.dtype)
        for fb in range(nf):
            u = np.zeros((nf, m, ref.n), dtype=self.dtype)
            u[fb] = nodal
            cols = ref.restrict(self.L(u, B, adjoint))           # (nf, column, row)
            for f in range(nf):
                J[f * m:(f + 1) * m, fb * m:(fb + 1) * m] = cols[f].T
        return J

    def mass(self):
        return np.tile(self.ref.mass(), self.nf)

    def dense_propagator(self, B, adjoint=False):
        A = self.dense(B, adjoint) * self.dt
        I = np.eye(A.shape[0], dtype=self.dtype)
        step = I
        for s in (4, 3, 2, 1):
            step = I + A @ step / self.dtype(s)
        P = I
        for _ in range(self.nsteps):
            P = step @ P
        return P

    def newton(self, q0, maxiter=8, tol=1e-20):
        """Dense frozen-base Newton on F(q) = Phi(q) - q over the free unique points; returns (q, the history
        of ||F||^2 in the bm1 inner product)."""
        c = self.restrict(self.project(q0))
        M = self.mass()
        hist = []
        for _ in range(maxiter):
            q = self.expand(c)
            F = self.restrict(self.propagate(q)) - c
            hist.append(float(np.sum(M * F * F)))
            if hist[-1] < tol:
                break
            J = self.dense_propagator(q).astype(np.float64) - np.eye(c.size)
            c = c - np.linalg.solve(J, F.astype(np.float64)).astype(self.dtype)
        return self.expand(c), hist


# ---- the end-to-end case -----------------------------------------------------------------------------
E2E = dict(lx1=6, ne=(3, 3), kappa=(0.05, 0.03), dt=0.05, nsteps=40, offset=0.02)


def e2e_case(dtype=np.float64):
    """(coords, mask, Burgers with the steady forcing set, q_t, the Newton starting point) of the 2-D case:
    lx1 = 6, 3 x 3 elements of [0, pi]^2 deformed by 0.04, walls of the undeformed box, layout (vx, vy)."""
    co = ar.box_mesh_2d(6, (3, 3), (PI, PI), amp=0.04)
    mask = ar.box_mask(ar.box_mesh_2d(6, (3, 3), (PI, PI)))
    x, y = co["x"], co["y"]
    ref = ar.Reference(6, 2, co, [np.zeros_like(x), np.zeros_like(x)], mask=mask, dtype=dtype)
    bg = Burgers(ref, E2E["kappa"], E2E["dt"], E2E["nsteps"])
    target = np.stack([np.sin(x) * np.sin(2 * y), -0.7 * np.sin(2 * x) * np.sin(y)])
    pert = np.stack([np.sin(2 * x) * np.sin(y), np.sin(x) * np.sin(3 * y)])
    qt = bg.steady_forcing(target)
    q0 = qt + dtype(E2E["offset"]) * bg.project(pert)
    return co, mask, bg, qt, q0, target, pert
