"""NumPy restatement of the incompressible time-stepper resolvent of ``nekstab_next_amd.resolvent``
(``IncompressibleResolventOperator``; ``DivergenceFreeProjector.project_pair_ptr``, csrc/pressure.hip), built on
``incompressible_reference.Incompressible``, ``burgers_reference.Burgers`` and
``coupled_resolvent_reference.CoupledResolvent``: the oracle of its tests.

The algorithm is the coupled resolvent's with the divergence-free projection behind every right-hand side,

    k = minv dsavg(r(w; B))        k_vel <- P k_vel  (CG at ``tol`` on the re and on the im part)
    g_re = (k_re + omega w_im) [+ f_re]      g_im = (k_im - omega w_re) [+ f_im]      w <- y + (dt/s) g

and ``P Pi`` for ``Pi``; the step, ``forced_run``, ``propagate``, ``dot``, ``solve`` and ``apply`` are
``resolvent_reference.Resolvent``'s.  Scalar fields pass unprojected.

The dense answer does not go through the time stepper or the CG.  With ``J`` the dense ``P L_B`` on the free unique
points (``Burgers.dense`` over ``Incompressible.L``: column by column, the projection through the dense
pseudo-inverse of ``E~``), ``M`` the diagonal ``bm1`` mass and ``Q`` an ``M``-orthonormal basis of ``range(P Pi)``
(the eigenvectors at eigenvalue 1 of the symmetric ``M^1/2 P M^-1/2``):

    y = Q (i omega - Q^T M J Q)^-1 Q^T M Pi f                       (J†, -omega for the adjoint)

which is regular at omega = 0 as well, where ``i omega - P L_B P`` on all free points is not.

Records of tests/test_incompressible_resolvent.py, which prints what it measures in f64 and holds every run to 8
times these; tests/test_gpu_incompressible_resolvent.py holds the device to 4 times them (floor 1e-11):"""
import numpy as np

import burgers_reference as br
import coupled_resolvent_reference as cr
import incompressible_reference as ir

# max |fixed point - dense answer| / max |dense answer|, CG at 1e-13 and inner GMRES at 1e-13: the worst of the two
# cases at their two frequencies, direct and adjoint, random unprojected forcings (seeds 4 and 5).  The worst run is
# "case2d" at omega = 0.56, adjoint (124 GMRES iterations), next to the eigenvalue 0.386 + 0.562i where the leading
# gain is 2279; away from it (omega = 2) the same case gives 9.5e-14, and "box3d" at most 2.1e-13.
DENSE_DISTANCE = 8.7e-13
# |<R f, g> - <f, R† g>| / sum bm1 |R f| |g| of the same runs (one pair per case and frequency), the worst ("case2d"
# at omega = 0.56; 3.0e-15 at omega = 2, at most 7.7e-15 on "box3d").
ADJOINT_DEFECT = 4.1e-14

CG_TOL = 1e-13
RK4_EDGE = cr.RK4_EDGE
# The frequencies of each case: one near a weakly damped (here: weakly growing or decaying) eigenfrequency of the
# dense P L_B, where the gain peaks, and one away from every one of them.
OMEGAS = {"case2d": (0.56, 2.0), "box3d": (0.0, 1.5)}
BOX3D_PARAMS = dict(kappa=(0.05, 0.04, 0.03, 0.02), dt=0.04, nsteps=4)


def case2d(dtype=np.float64, nsteps=None):
    """(coordinates, mask, Incompressible, base state, dt, nsteps): the fixed closed 2-D case ``ir.CASE`` (9
    elements of lx1 = 5) about its steady state q_t."""
    co, mask, ns, qt, *_ = ir.case2d(dtype, nsteps)
    return co, mask, ns, qt, ir.CASE["dt"], ns.nsteps


def box3d(dtype=np.float64, nsteps=None):
    """(coordinates, mask, Incompressible, base state, dt, nsteps): the closed deformed 3-D box of the projector
    tests (2 x 2 x 2 elements of lx1 = 4) with one scalar (n_wf = 4 > ldim) about ``P Pi`` of a smooth state."""
    lx1, ldim, co, mask, ref = ir.projector_case("closed3d", dtype)
    p = BOX3D_PARAMS
    ns = ir.Incompressible(ref, p["kappa"], p["dt"], p["nsteps"] if nsteps is None else nsteps)
    x, y, z = co["x"], co["y"], co["z"]
    B = ns.project(np.stack([np.sin(x) * np.cos(2 * y) * np.sin(z), np.cos(x + z) * np.sin(2 * y), 0.5 * np.sin(x * y) + 0.2 * z,
                             np.cos(x) * np.cos(y) * np.cos(z)]))
    return co, mask, ns, B, p["dt"], ns.nsteps


CASES = {"case2d": case2d, "box3d": box3d}


class IncompressibleResolvent(cr.CoupledResolvent):
    """``cg=True``: the device's algorithm, every projection by ``Pressure.cg_project`` at ``tol``;
    ``cg=False``: the same with the dense pseudo-inverse projection (``Incompressible.P``)."""

    def __init__(self, ns: ir.Incompressible, B, dt, nsteps, omega, tol=CG_TOL, check_every=8, cg=True):
        super().__init__(ns, B, dt, nsteps, omega)
        self.ns, self.tol, self.check_every, self.cg = ns, tol, check_every, cg
        self._red, self._E = {}, None

    # ---- the algorithm ----
    def cg_project(self, v):
        """``Pressure.cg_project`` (the device's iteration: unpreconditioned CG from 0, the mean of every ``E p``
        removed, the residual tested every ``check_every`` iterations) with ``E`` applied as its dense matrix: an
        inner solve of the resolvent runs some 10^5 CG iterations, which the sum-factorised form does not give
        in the time of a test.  Returns (P v, iterations)."""
        pr = self.ns.pr
        if self._E is None:
            self._E = pr.dense_E()
        E, zero = self._E, self.dtype(0)
        mean = (lambda a: a.mean()) if pr.closed else (lambda a: zero)
        v = np.asarray(v).astype(self.dtype)
        b = pr.div(v)
        r = b - mean(b)
        x = np.zeros_like(r)
        rr = bb = r @ r
        it = 0
        if bb == 0:
            return v.copy(), 0
        p = r.copy()
        while True:
            Ep = E @ p
            mu = mean(Ep)
            den = p @ Ep - mu * p.sum()
            alpha = rr / den if den != 0 else zero
            x = x + alpha * p
            r = r - alpha * (Ep - mu)
            rr_new = r @ r
            it += 1
            if it % self.check_every == 0 and rr_new <= self.tol ** 2 * bb:
                break
            if it >= 2 * pr.npz + 20:
                raise RuntimeError(f"CG: {it} iterations, |r|/|b| = {float(np.sqrt(rr_new / bb)):.3e}")
            p = r + (rr_new / rr if rr != 0 else zero) * p
            rr = rr_new
        return v - pr.correction(x), it

    def P(self, q):
        """``P`` on the velocity rows of a real state (n_wf, n_v)."""
        if not self.cg:
            return self.ns.P(q)
        q = np.array(q, dtype=self.dtype)
        d = self.ns.ldim
        q[:d] = self.cg_project(q[:d])[0]
        return q

    def _halves(self, fn, x):
        x = np.asarray(x)
        return self._join(fn(x.real), fn(x.imag))

    def project(self, f):
        return self._halves(lambda u: self.P(self.ns.ref.project(u.astype(self.dtype))), f)

    def L(self, w, adjoint=False):
        ns = self.ns
        return self._halves(lambda u: self.P(br.Burgers.assemble(ns, ns.local(u, self.B, adjoint))), w)

    def divergence(self, y):
        """``Z D`` of the velocity rows of both parts: (2, npz)."""
        pr, d = self.ns.pr, self.ns.ldim
        y = np.asarray(y)
        return np.stack([pr.Z(pr.div(y.real[:d])), pr.Z(pr.div(y.imag[:d]))])

    # ---- the dense answer ----
    def reduced(self, adjoint=False):
        """(Q, A): the M-orthonormal basis of range(P Pi) on the free unique points and A = Q^T M J Q (f64)."""
        if adjoint not in self._red:
            ns = self.ns
            M = ns.mass().astype(np.float64)
            if "Q" not in self._red:
                sM = np.sqrt(M)
                S = sM[:, None] * ns.dense_P().astype(np.float64) / sM[None, :]
                lam, V = np.linalg.eigh(0.5 * (S + S.T))
                assert np.all((np.abs(lam) < 1e-8) | (np.abs(lam - 1.0) < 1e-8)), "dense_P is not a projector"
                self._red["Q"] = V[:, lam > 0.5] / sM[:, None]
            Q = self._red["Q"]
            J = br.Burgers.dense(ns, self.B, adjoint).astype(np.float64)      # P L_B, column by column
            self._red[adjoint] = Q.T @ (M[:, None] * (J @ Q))
        return self._red["Q"], self._red[adjoint]

    def dense_apply(self, f, adjoint=False):
        ns = self.ns
        Q, A = self.reduced(adjoint)
        M = ns.mass().astype(np.float64)
        om = float(-self.omega if adjoint else self.omega)
        pf = np.asarray(f)
        pf = self._join(ns.ref.project(pf.real.astype(self.dtype)), ns.ref.project(pf.imag.astype(self.dtype)))
        rhs = Q.T @ (M * ns.restrict(pf).astype(np.complex128))
        c = np.linalg.solve(1j * om * np.eye(A.shape[0]) - A, rhs)
        return ns.expand(Q @ c)

    def modal_forcing(self, k=6):
        """A forcing in range(P Pi) that is a combination of k eigenvectors of P L_B (those of largest real part):
        the right-hand side of the inner solve then lies in an invariant subspace of Phi of complex dimension k, and
        GMRES in the real pair space ends within about 2 k iterations."""
        Q, A = self.reduced()
        lam, V = np.linalg.eig(A)
        idx = np.argsort(-lam.real, kind="stable")[:k]
        return self.ns.expand(Q @ (V[:, idx] @ (1.0 + 0.5j * np.arange(k))))

    def spectrum(self):
        """The eigenvalues of P L_B on range(P Pi)."""
        return np.linalg.eigvals(self.reduced()[1])

    def gains(self):
        """The squared singular values of the operator in the bm1 inner product, descending, each once (in the
        pair space each counts twice): those of (i omega - A)^-1 in the M-orthonormal coordinates of Q."""
        A = self.reduced()[1]
        R = np.linalg.inv(1j * float(self.omega) * np.eye(A.shape[0]) - A)
        return np.linalg.svd(R, compute_uv=False) ** 2


def unprojected_gains(ns: ir.Incompressible, B, dt, nsteps, omega):
    """The dense gains of the ``CoupledResolventOperator`` of the same case: no projection anywhere."""
    bg = br.Burgers(ns.ref, ns.kappa, dt, nsteps)
    return cr.CoupledResolvent(bg, B, dt, nsteps, omega).gains()
