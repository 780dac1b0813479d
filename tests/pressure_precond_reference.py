"""NumPy restatement of the fast-diagonalisation preconditioner of the pressure CG
(``nekstab_next_amd.pressure`` with ``preconditioner="fdm"``, ``nkv_pressure_precond`` in csrc/pressure.hip),
built on ``incompressible_reference.Pressure``: the oracle of its tests.

1-D reference data for ``n = lx1``: the GLL weights ``rho`` and derivative ``D^``, the ``m = lx1 - 2`` Gauss weights
``w`` and the interpolation ``I`` (m x n).  With ``rho~ = rho``, its two end weights doubled (the mass an interior
interface sees after assembly), ``D~ = diag(w) I D^`` and ``J~ = diag(w) I``:

    A^ = D~ diag(1/rho~) D~^T,   B^ = J~ diag(1/rho~) J~^T,   A^ S = B^ S Lambda,  S^T B^ S = I

Per element ``e`` and local direction ``d`` (r fastest): ``h[e,d]`` half the distance between the centroids (plain
means of the GLL coordinates) of the two opposite faces, ``c[e,d] = (prod_k h[e,k]) / h[e,d]^2`` and

    M_e = (S x .. x S) diag( 1 / sum_d c[e,d] lambda_{i_d} ) (S^T x .. x S^T)

the exact inverse of ``sum_d c[e,d] (A^ in slot d, B^ elsewhere)``.  ``pcg_project`` is the device's iteration:
``z = Z M r``, ``p = z + (r.z / r.z_prev) p``, ``alpha = r.z / p.(Z E p)``, the stop rule of ``cg_project``
(``|r|_2 <= tol |b|_2`` every ``check_every`` iterations).

Records, measured in f64 by the functions below (seed 5), which tests/test_pressure_precond.py regenerates:"""
import numpy as np
import scipy.linalg

import advdiff_reference as ar
import incompressible_reference as ir
from nekstab_next_amd.fld import gauss_points, gll_points, interp_matrix
from nekstab_next_amd.sensitivity import gll_derivative
from nekstab_next_amd.synthetic import gll_weights

# the projector with PCG at tol = 1e-13 on the three meshes of ``incompressible_reference.projector_case``
# (``projector_records``): the figures of ``incompressible_reference.PROJECTOR``, by ``pcg_project``.  selfadj is the
# difference of two f64 sums over the sum of their absolute terms: one ulp of a sum, 2^-52 = 2.2e-16, is the
# resolution of that measure, and a smaller figure (1.1e-17 on open2d, exactly 0 on closed3d) is recorded as 2.2e-16
PROJECTOR = {
    "closed2d": dict(dist=7.2e-15, div=6.2e-15, twice=4.4e-15, selfadj=7.2e-16, iterations=64),
    "open2d": dict(dist=5.6e-15, div=1.5e-15, twice=9.0e-16, selfadj=2.2e-16, iterations=48),
    "closed3d": dict(dist=5.1e-15, div=1.2e-15, twice=6.9e-16, selfadj=2.2e-16, iterations=64),
}
# iterations to |r| <= 1e-12 |b| tested every 8, (CG, PCG), on the two larger meshes of ``iteration_case`` and on the
# three of ``projector_case`` (``iteration_records``)
ITERATIONS = {"big2d": (360, 144), "big3d": (552, 168), "closed2d": (96, 64), "open2d": (80, 40), "closed3d": (88, 64)}
# max |propagate with CG projections - propagate with PCG projections| / max |.| on ``case2d`` over 2 steps from q0,
# every projection solved to tol = 1e-13 (``flow_difference``)
FLOW_DIFFERENCE = 1.0e-15
FLOW_TOL = 1e-13
# the same for one matvec of the restatement's incompressible resolvent on ``case2d`` at omega = 2.0, three steps of
# 0.13 (the operator of tests/test_gpu_incompressible_resolvent.py), CG and inner GMRES at 1e-13 (``resolvent_difference``)
RESOLVENT_DIFFERENCE = 2.9e-14
RESOLVENT_STEPS = (0.13, 3)
PI = np.pi


def fdm_matrices(lx1):
    """(S, lambda, A^, B^) of the 1-D reference problem in f64."""
    m = lx1 - 2
    rho = np.array(gll_weights(lx1), dtype=np.float64)
    rho[0] *= 2.0
    rho[-1] *= 2.0
    w = np.polynomial.legendre.leggauss(m)[1]
    Jt = w[:, None] * interp_matrix(gll_points(lx1), gauss_points(m))
    Dt = Jt @ gll_derivative(lx1)
    A = (Dt / rho) @ Dt.T
    B = (Jt / rho) @ Jt.T
    A, B = 0.5 * (A + A.T), 0.5 * (B + B.T)
    lam, S = scipy.linalg.eigh(A, B)
    return S, lam, A, B


def element_scales(coords, lx1, ldim):
    """c[e, d] from the face centroids of every element."""
    nz = lx1 if ldim == 3 else 1
    X = np.stack([np.asarray(coords[k], dtype=np.float64).reshape(-1, nz, lx1, lx1) for k in ("x", "y", "z")[:ldim]])
    h = []
    for d in range(ldim):
        ax = 4 - d                                            # r is the last axis of (c, e, k, j, i)
        lo, hi = np.take(X, 0, axis=ax), np.take(X, lx1 - 1, axis=ax)
        lo, hi = (f.reshape(ldim, f.shape[1], -1).mean(axis=2) for f in (lo, hi))
        h.append(0.5 * np.sqrt(np.sum((hi - lo) ** 2, axis=0)))
    h = np.stack(h, axis=1)
    return np.prod(h, axis=1, keepdims=True) / h ** 2


class PressureFDM(ir.Pressure):
    """``Pressure`` with the preconditioner; ``coords``: the mesh the Reference was built on."""

    def __init__(self, ref, coords, closed="auto"):
        super().__init__(ref, closed=closed)
        self.coords = coords
        self._fdm = None

    def fdm_data(self):
        """(S, lambda, c): the generalised eigenvectors and eigenvalues, the element scales (nel, ldim)."""
        if self._fdm is None:
            S, lam, _, _ = fdm_matrices(self.ref.lx1)
            self._fdm = (S, lam, element_scales(self.coords, self.ref.lx1, self.ldim))
        return self._fdm

    def _denominator(self):
        S, lam, c = self.fdm_data()
        den = c[:, 0, None, None, None] * lam[None, None, None, :] + c[:, 1, None, None, None] * lam[None, None, :, None]
        if self.ldim == 3:
            den = den + c[:, 2, None, None, None] * lam[None, :, None, None]
        return den

    def M(self, r, absolute=False):
        """M r on ([batch,] npz); ``absolute``: |S| for S and |r| for r, the bound of the rounding analysis."""
        S = self.fdm_data()[0].astype(self.dtype)
        r = np.asarray(r).astype(self.dtype)
        if absolute:
            S, r = np.abs(S), np.abs(r)
        T = r.reshape(r.shape[:-1] + self.pshape)
        T = np.einsum("ia,...i->...a", S, T)
        T = np.einsum("jb,...ja->...ba", S, T)
        if self.ldim == 3:
            T = np.einsum("kc,...kba->...cba", S, T)
        T = T / self._denominator().astype(self.dtype)
        T = np.einsum("ia,...a->...i", S, T)
        T = np.einsum("jb,...ba->...ja", S, T)
        if self.ldim == 3:
            T = np.einsum("kc,...cba->...kba", S, T)
        return T.reshape(r.shape)

    def dense_M(self):
        return self.M(np.eye(self.npz, dtype=self.dtype)).T

    def pcg_project(self, v, tol=1e-12, maxiter=None, check_every=8):
        """(P v, iterations, phi): ``cg_project`` preconditioned by ``Z M``, the same stop rule."""
        v = np.asarray(v).astype(self.dtype)
        maxiter = 2 * self.npz + 20 if maxiter is None else maxiter
        zero = self.dtype(0)
        mean = (lambda a: a.mean()) if self.closed else (lambda a: zero)
        b = self.div(v)
        r = b - mean(b)
        x = np.zeros_like(r)
        bb = r @ r
        it = 0
        if bb == 0:
            return v.copy(), 0, x
        z = self.M(r)
        rz = r @ z
        p = z - mean(z)
        while True:
            Ep = self.E(p)
            mu = mean(Ep)
            den = p @ Ep - mu * p.sum()
            alpha = rz / den if den != 0 else zero
            x = x + alpha * p
            r = r - alpha * (Ep - mu)
            rr = r @ r
            it += 1
            if it % check_every == 0 and np.sqrt(rr) <= tol * np.sqrt(bb):
                break
            if it >= maxiter:
                raise RuntimeError(f"PCG: {it} iterations, |r|/|b| = {float(np.sqrt(rr / bb)):.3e}")
            z = self.M(r)
            rz_new = r @ z
            p = (z - mean(z)) + (rz_new / rz if rz != 0 else zero) * p
            rz = rz_new
        return v - self.correction(x), it, x


# ---- the cases -----------------------------------------------------------------------------------------
def projector_pressure(name):
    """(lx1, ldim, coords, mask, Reference, PressureFDM) of a mesh of ``incompressible_reference.projector_case``."""
    lx1, ldim, co, mask, ref = ir.projector_case(name)
    return lx1, ldim, co, mask, ref, PressureFDM(ref, co)


def iteration_case(name):
    """(lx1, ldim, ne, coords, mask, Reference) of the two larger closed meshes deformed by 0.04: "big2d", 6 x 6
    elements of lx1 = 6 on [0, pi]^2; "big3d", 3 x 3 x 3 elements of lx1 = 6 (the box of ``deformed_box``)."""
    if name == "big2d":
        lx1, ldim, ne = 6, 2, (6, 6)
        co = ar.box_mesh_2d(lx1, ne, (PI, PI), amp=0.04)
        mask = ar.box_mask(ar.box_mesh_2d(lx1, ne, (PI, PI)))
    elif name == "big3d":
        from nekstab_next_amd.layout import NekLayout
        from seed_helpers import box_mesh_coords
        from test_bf_sensitivity import deformed_box

        lx1, ldim, ne = 6, 3, (3, 3, 3)
        lay = NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=27)
        co = deformed_box(lay, ne, amp=0.04)
        mask = ar.box_mask(box_mesh_coords(lay, ne))
    else:
        raise KeyError(name)
    zero = [np.zeros(co["x"].size)] * ldim
    return lx1, ldim, ne, co, mask, ar.Reference(lx1, ldim, co, zero, mask=mask)


def iteration_records(name, tol=1e-12, seed=5, check_every=8):
    """(CG, PCG) iterations of a random masked continuous velocity on a mesh of ``iteration_case`` or of
    ``projector_case``."""
    if name in ("big2d", "big3d"):
        lx1, ldim, _, co, mask, ref = iteration_case(name)
    else:
        lx1, ldim, co, mask, ref = ir.projector_case(name)
    pr = PressureFDM(ref, co)
    v = ref.project(np.random.default_rng(seed).standard_normal((ldim, ref.n)))
    return (pr.cg_project(v, tol=tol, check_every=check_every)[1],
            pr.pcg_project(v, tol=tol, check_every=check_every)[1])


def projector_records(name, tol=1e-13, seed=5):
    """``incompressible_reference.projector_records`` with ``pcg_project`` for ``cg_project``."""
    lx1, ldim, co, mask, ref, pr = projector_pressure(name)
    rng = np.random.default_rng(seed)
    v, w = (ref.project(rng.standard_normal((ldim, ref.n))) for _ in range(2))
    Pv, it, _ = pr.pcg_project(v, tol=tol)
    Pw = pr.pcg_project(w, tol=tol)[0]
    dense = pr.project(v)
    scale = float(np.max(np.abs(v)))
    PPv = pr.pcg_project(Pv, tol=tol)[0]
    bm = ref.bm1
    lhs, rhs = float(np.sum(bm * w * Pv)), float(np.sum(bm * Pw * v))
    return dict(dist=float(np.max(np.abs(Pv - dense))) / scale,
                div=float(np.max(np.abs(pr.Z(pr.div(Pv)))) / np.max(np.abs(pr.Z(pr.div(v))))),
                twice=float(np.max(np.abs(PPv - Pv))) / scale,
                selfadj=abs(lhs - rhs) / float(np.sum(bm * np.abs(w) * np.abs(Pv))),
                iterations=it, closed=pr.closed, ratio=pr.closed_ratio)


class IterativeIncompressible(ir.Incompressible):
    """``Incompressible`` whose projection is the device's iteration: ``cg_project`` or ``pcg_project`` at ``tol``."""

    def __init__(self, ref, coords, kappa, dt, nsteps, preconditioned, tol=FLOW_TOL):
        super().__init__(ref, kappa, dt, nsteps)
        self.pr = PressureFDM(ref, coords, closed=self.pr.closed)
        self._solve = self.pr.pcg_project if preconditioned else self.pr.cg_project
        self._tol = tol

    def P(self, q):
        q = np.array(q, dtype=self.dtype)
        q[: self.ldim] = self._solve(q[: self.ldim], tol=self._tol)[0]
        return q


def flow_difference(nsteps=2, tol=FLOW_TOL):
    """max |CG flow - PCG flow| / max |CG flow| of ``propagate`` from the Newton starting point of ``case2d``."""
    co, mask, ns, qt, q0, target, pert = ir.case2d(np.float64, nsteps)
    out = []
    for pre in (False, True):
        it = IterativeIncompressible(ns.ref, co, ir.CASE["kappa"], ir.CASE["dt"], nsteps, pre, tol)
        it.g = ns.g
        out.append(it.propagate(q0))
    return float(np.max(np.abs(out[0] - out[1])) / np.max(np.abs(out[0])))


def resolvent_difference(name="case2d", k=1, seed=4, tol=1e-13, kdim=400, dt=RESOLVENT_STEPS[0], nsteps=RESOLVENT_STEPS[1]):
    """max |matvec with CG projections - matvec with PCG projections| / max |.| of the restatement's resolvent
    (``incompressible_resolvent_reference.IncompressibleResolvent``: forced run, then the inner GMRES) for a random
    unprojected forcing on a case of that file at its frequency ``k``, over ``nsteps`` steps of ``dt``."""
    import incompressible_resolvent_reference as irr

    co, mask, ns, B = irr.CASES[name]()[:4]
    omega = irr.OMEGAS[name][k]
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((ns.nf, ns.ref.n)) + 1j * rng.standard_normal((ns.nf, ns.ref.n))
    pr = PressureFDM(ns.ref, co, closed=ns.pr.closed)

    class Preconditioned(irr.IncompressibleResolvent):
        """``cg_project`` by the preconditioned iteration, E and M as their dense matrices."""

        def cg_project(self, v):
            if self._E is None:
                self._E, self._M = pr.dense_E(), pr.dense_M()
            E, M, zero = self._E, self._M, self.dtype(0)
            mean = (lambda a: a.mean()) if pr.closed else (lambda a: zero)
            v = np.asarray(v).astype(self.dtype)
            b = pr.div(v)
            r = b - mean(b)
            x = np.zeros_like(r)
            bb = r @ r
            it = 0
            if bb == 0:
                return v.copy(), 0
            z = M @ r
            rz = r @ z
            p = z - mean(z)
            while True:
                Ep = E @ p
                mu = mean(Ep)
                den = p @ Ep - mu * p.sum()
                alpha = rz / den if den != 0 else zero
                x = x + alpha * p
                r = r - alpha * (Ep - mu)
                rr = r @ r
                it += 1
                if it % self.check_every == 0 and rr <= self.tol ** 2 * bb:
                    break
                if it >= 2 * pr.npz + 20:
                    raise RuntimeError(f"PCG: {it} iterations, |r|/|b| = {float(np.sqrt(rr / bb)):.3e}")
                z = M @ r
                rz_new = r @ z
                p = (z - mean(z)) + (rz_new / rz if rz != 0 else zero) * p
                rz = rz_new
            return v - pr.correction(x), it

    out = []
    for cls in (irr.IncompressibleResolvent, Preconditioned):
        R = cls(ns, B, dt, nsteps, omega)
        out.append(R.solve(R.forced_run(R.project(f)), tol=tol, kdim=kdim)[0])
    return float(np.max(np.abs(out[0] - out[1])) / np.max(np.abs(out[0])))
