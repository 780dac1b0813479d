"""NumPy restatement of the coupled time-stepper resolvent of ``nekstab_next_amd.resolvent``
(``CoupledResolventOperator``, ``nkv_linconv_crhs``; csrc/advdiff.hip): ``resolvent_reference.Resolvent``'s
algorithm with ``L`` replaced by the linearised convection ``burgers_reference.Burgers.L(·, B, adjoint)`` about a
base state ``B`` of all fields, applied to the re and the im part.  ``B`` is real, so it does not mix the halves;
it couples the fields, so the dense forms are one matrix on all of them (field-major on the free unique points).

The step, ``forced_run``, ``propagate``, ``dot``, ``solve`` and ``apply`` are the parent's, in the ``dtype`` of the
``Burgers`` restatement (``np.float64`` or ``np.longdouble``).

Records of tests/test_coupled_resolvent.py, which prints what it measures in f64 and holds every run to 8 times
these (the margin ``_gate`` of tests/test_gpu_advdiff.py gives a rounding error); tests/test_gpu_coupled_resolvent.py
holds the device to 4 times them, the margins tests/test_gpu_resolvent.py gives the same quantities."""
import numpy as np

import advdiff_reference as ar
import burgers_reference as br
import resolvent_reference as rr

# max |fixed point - dense solve| / max |dense solve| at inner tolerance 1e-13: the worst of "cell" and "odd" at
# omega in {0, 1}, direct and adjoint, random unprojected forcings (seeds 4 and 5), the cases' own dt and nsteps.
# The worst run is "cell" at omega = 1, direct (43 GMRES iterations); "odd" at omega = 0, the most non-normal of
# the four (leading gain 3934), gives 6.2e-14.
DENSE_DISTANCE = 7.9e-14
# |<R f, g> - <f, R† g>| / sum bm1 |R f| |g| of the same eight runs (four pairs), the worst.
ADJOINT_DEFECT = 4.4e-15
# The leading four pair-space gains of "odd" at omega = 1 from a Golub-Kahan bidiagonalisation of the f64
# restatement's operator (inner tolerance 1e-13, k_dim = ANALYSIS_KDIM, the hashed seed 17 of the device test): the worst relative distance from
# the dense weighted SVD.  8 times this is above the project's 1e-10 when GAIN_GATE says so (see there).
GAIN_DISTANCE = 1.4e-14
# k_dim of the analysis test: the smallest for which a bidiagonalisation of the dense pair operator of "odd" at
# omega = 1 (real dimension 100) with 1e-13 relative noise in every product has the four leading values within
# 1e-12 of the dense SVD for each of 40 random seeds whatever noise is drawn (worst 8.3e-14).  16 is the edge: its
# worst seed lies between 7e-13 and 3e-11 with the noise; at 15 the worst is 2.6e-8.
ANALYSIS_KDIM = 17
# The gate of the analysis test on the leading four values: the project's 1e-10 relative if the restatement meets
# it with a factor 8 to spare, otherwise 8 times the restatement's own distance.
GAIN_GATE = 1e-10 if 8 * GAIN_DISTANCE <= 1e-10 else 8 * GAIN_DISTANCE

# The leading gains sigma_1^2 of the dense weighted SVD: (case, omega) -> (coupled, uncoupled).  The production
# term is what makes L_B non-normal: without it the gains are an order of magnitude smaller.
LEADING_GAINS = {("cell", 1.0): (54.01, 4.419), ("cell", 0.0): (338.77, 154.10),
                 ("odd", 1.0): (287.90, 8.493), ("odd", 0.0): (3934.0, 181.60)}
# max Re lambda(J), rho(J) of the dense L_B of the three cases: L_B is stable and dt (rho + omega) stays inside
# RK4's region (about 2.78) for omega <= 1.
MARGINS = {"cell": (-0.241, 32.4), "odd": (-0.023, 5.78), "box3d": (-1.86, 43.6)}
RK4_EDGE = 2.78

BOX3D = (5, (2, 2, 2))
BOX3D_PARAMS = dict(kappa=(0.05, 0.04, 0.03, 0.02), dt=0.04, nsteps=4)


def cell_case(name, dtype=np.float64):
    """(Burgers restatement, base state B, dt, nsteps) of a 2-D case of ``resolvent_reference.CASES``: the
    case's own cellular flow is the base state (taken as it is, not projected)."""
    c = rr.CASES[name]
    co, U, mask = rr.cell_mesh(c["lx1"])
    zero = [np.zeros_like(co["x"])] * 2
    bg = br.Burgers(ar.Reference(c["lx1"], 2, co, zero, mask=mask, dtype=dtype), c["kappa"], c["dt"], c["nsteps"])
    return bg, np.stack(U), c["dt"], c["nsteps"]


class CoupledResolvent(rr.Resolvent):
    def __init__(self, bg: br.Burgers, B, dt, nsteps, omega):
        super().__init__(bg.ref, bg.kappa, dt, nsteps, omega)
        self.bg, self.B = bg, np.asarray(B).astype(bg.dtype)

    def L(self, w, adjoint=False):
        """L_B (its adjoint) on the re and the im part of (n_wf, n_v) complex fields."""
        w = np.asarray(w)
        return self._join(self.bg.L(w.real, self.B, adjoint), self.bg.L(w.imag, self.B, adjoint))

    # ---- dense forms on the free unique points x n_wf (field-major) ----
    def dense_inverse(self, adjoint=False):
        """(i omega - J)^-1 with J = Burgers.dense(B) ((-i omega - J†)^-1 if ``adjoint``)."""
        J = self.bg.dense(self.B, adjoint).astype(np.float64)
        om = -self.omega if adjoint else self.omega
        return np.linalg.inv(1j * float(om) * np.eye(J.shape[0]) - J)

    def dense_apply(self, f, adjoint=False):
        """(±i omega - J)^-1 Pi f by one dense solve on all fields."""
        pf = self.project(f)
        J = self.bg.dense(self.B, adjoint).astype(np.float64)
        om = -self.omega if adjoint else self.omega
        z = 1j * float(om) * np.eye(J.shape[0]) - J
        return self.bg.expand(np.linalg.solve(z, self.bg.restrict(pf).astype(np.complex128)))

    def weighted(self, adjoint=False):
        """M^1/2 (±i omega - J)^-1 M^-1/2: the operator in the Euclidean product."""
        sB = np.sqrt(self.bg.mass().astype(np.float64))
        return sB[:, None] * self.dense_inverse(adjoint) / sB[None, :]

    def gains(self):
        """The squared singular values of the operator in the bm1 inner product of all fields, descending, each
        once (in the pair space each counts twice)."""
        return np.linalg.svd(self.weighted(), compute_uv=False) ** 2


def bidiagonal_gains(matvec, rmatvec, dot, seed, k_dim):
    """Squared singular values, descending, of the k_dim-step Golub-Kahan bidiagonalisation (full
    reorthogonalisation, twice) of an operator given by its products: what ``svds`` computes."""
    def norm(v):
        return np.sqrt(dot(v, v))

    def orth(v, Q):
        for _ in range(2):
            for q in Q:
                v = v - dot(q, v) * q
        return v

    V, U = [seed / norm(seed)], []
    alpha, beta = [], []
    for k in range(k_dim):
        u = matvec(V[k])
        if k > 0:
            u = u - beta[-1] * U[-1]
        u = orth(u, U)
        alpha.append(float(norm(u)))
        U.append(u / alpha[-1])
        v = rmatvec(U[k]) - alpha[-1] * V[k]
        v = orth(v, V)
        beta.append(float(norm(v)))
        V.append(v / beta[-1])
    Bk = np.diag(alpha) + np.diag(beta[:-1], 1)
    return np.linalg.svd(Bk, compute_uv=False) ** 2
