"""NumPy restatement of the rotating-frame time-stepper resolvent of ``nekstab_next_amd.resolvent``
(``nkv_advdiff_cstage``, csrc/advdiff.hip), built on ``advdiff_reference.Reference``: the oracle of its tests.

With ``u(t) = Re[y(t) e^{i omega t}]`` the harmonically forced problem is ``dy/dt = (L - i omega) y + Pi f``, a
constant forcing, with the steady state ``y = (i omega - L)^-1 Pi f``.  One RK4 step in Horner form, the
forcing inside, on the re / im halves (the order of the device, no contraction):

    g_re = (L w_re + omega w_im) [+ f_re]      g_im = (L w_im - omega w_re) [+ f_im]
    w_re <- y_re + (dt/s) g_re                  w_im <- y_im + (dt/s) g_im        s = 4, 3, 2, 1 from w = y

so ``y+ = p(dt G) y + dt phi(dt G) f`` with ``G = L - i omega`` and ``phi(z) = (p(z) - 1)/z``.  Over ``nsteps``
steps: ``b`` the forced run from 0, ``Phi x`` the unforced run from ``x``; the fixed point of
``(I - Phi) y = b`` is the steady state exactly, since ``p - 1 = z phi``.  The adjoint replaces ``L`` by its
adjoint and ``omega`` by ``-omega``.

Complex fields are arrays (n_wf, n_v) of ``np.complex128`` or ``np.clongdouble``: field f has its own
``kappa[f]``.  The inner product is the pair product ``sum bm1 (a_re b_re + a_im b_im)``, in which i x is
another direction than x: every singular value of the complex operator counts twice."""
import numpy as np

import advdiff_reference as ar


PI = np.pi
# The 2-D cases of the resolvent tests: 3 x 3 deformed elements of [0, pi]^2, fields (vx, vy), cellular flow.
# "odd": n_v = 81, so the im halves of a pair vector are only 8-byte aligned.
CASES = {"cell": dict(lx1=6, kappa=(0.05, 0.03), dt=0.06, nsteps=16),
         "odd": dict(lx1=3, kappa=(0.05, 0.03), dt=0.3, nsteps=16)}
# Measured by tests/test_resolvent.py on "cell" (omega in {0, 1}, dt in {0.06, 0.04}, nsteps in {16, 32}, inner
# tolerance 1e-13), recorded in DESIGN §9 item 13; the tests gate against them with the margins stated there.
DENSE_DISTANCE = 8.2e-14    # max |fixed point - dense solve| / max |dense solve|, the worst of the 16 runs
ADJOINT_DEFECT = 4.6e-15    # |<R f, g> - <f, R† g>| / sum bm1 |R f| |g|, the worst of the 8 pairs


def cell_mesh(lx1):
    """(coordinates, base flow, wall mask) of the deformed 3 x 3 mesh with the cellular flow of
    tests/test_advdiff.py; the walls are those of the box before the deformation."""
    co = ar.box_mesh_2d(lx1, (3, 3), (PI, PI), amp=0.04)
    x, y = co["x"], co["y"]
    U = [2.0 * np.sin(x) * np.cos(y) + 0.5, -2.0 * np.cos(x) * np.sin(y)]
    return co, U, ar.box_mask(ar.box_mesh_2d(lx1, (3, 3), (PI, PI)))


def _ctype(dtype):
    return np.clongdouble if dtype == np.longdouble else np.complex128


class Resolvent:
    def __init__(self, ref: ar.Reference, kappa, dt, nsteps, omega):
        self.ref, self.kappa = ref, [float(k) for k in kappa]
        self.dtype, self.ctype = ref.dtype, _ctype(ref.dtype)
        self.dt, self.nsteps, self.omega = ref.dtype(dt), int(nsteps), ref.dtype(omega)

    # ---- the pieces ----
    def _join(self, re, im):
        out = np.empty(re.shape, dtype=self.ctype)
        out.real, out.imag = re, im
        return out

    def _each(self, fn, x):
        """fn(field values, kappa) on both halves of every field."""
        x = np.asarray(x)
        re = np.stack([fn(x[f].real, k) for f, k in enumerate(self.kappa)])
        im = np.stack([fn(x[f].imag, k) for f, k in enumerate(self.kappa)])
        return self._join(re.astype(self.dtype), im.astype(self.dtype))

    def project(self, f):
        return self._each(lambda u, k: self.ref.project(u), f)

    def L(self, w, adjoint=False):
        return self._each(lambda u, k: self.ref.L(u, k, adjoint), w)

    def step(self, y, f=None, adjoint=False):
        """One RK4 step of dy/dt = (L - i omega) y + f  (L†, +i omega if ``adjoint``)."""
        om = -self.omega if adjoint else self.omega
        y = np.asarray(y).astype(self.ctype)
        w = y
        for s in (4, 3, 2, 1):
            Lw = self.L(w, adjoint)
            g_re = Lw.real + om * w.imag
            g_im = Lw.imag - om * w.real
            if f is not None:
                g_re = g_re + f.real
                g_im = g_im + f.imag
            c = self.dt / self.dtype(s)
            w = self._join(y.real + c * g_re, y.imag + c * g_im)
        return w

    def forced_run(self, f, adjoint=False):
        """nsteps forced steps from y = 0; ``f`` is taken as it is (project it first)."""
        f = np.asarray(f).astype(self.ctype)
        y = np.zeros_like(f)
        for _ in range(self.nsteps):
            y = self.step(y, f, adjoint)
        return y

    def propagate(self, x, adjoint=False):
        """nsteps unforced steps from ``x`` (taken as it is)."""
        y = np.asarray(x).astype(self.ctype)
        for _ in range(self.nsteps):
            y = self.step(y, None, adjoint)
        return y

    # ---- the pair inner product and the fixed point ----
    def dot(self, a, b):
        bm1 = self.ref.bm1
        return (bm1 * (a.real * b.real + a.imag * b.imag)).sum()

    def solve(self, b, adjoint=False, tol=1e-13, kdim=150):
        """(I - Phi) y = b by full GMRES (modified Gram-Schmidt, twice) in the pair inner product, from y = 0,
        to ||r|| <= tol ||b||.  Returns (y, iterations)."""
        beta = np.sqrt(self.dot(b, b))
        if beta == 0:
            return np.zeros_like(b), 0
        Q = [b / beta]
        H = np.zeros((kdim + 1, kdim), dtype=self.dtype)
        e1 = np.zeros(kdim + 1, dtype=np.float64)
        e1[0] = float(beta)
        for k in range(kdim):
            v = Q[k] - self.propagate(Q[k], adjoint)
            for _ in range(2):
                for i in range(k + 1):
                    h = self.dot(Q[i], v)
                    H[i, k] += h
                    v = v - h * Q[i]
            H[k + 1, k] = np.sqrt(self.dot(v, v))
            Hk = H[: k + 2, : k + 1].astype(np.float64)
            yk, *_ = np.linalg.lstsq(Hk, e1[: k + 2], rcond=None)
            res = np.linalg.norm(e1[: k + 2] - Hk @ yk)
            if res <= tol * float(beta) or H[k + 1, k] == 0:
                break
            Q.append(v / H[k + 1, k])
        else:
            raise RuntimeError(f"restatement GMRES: residual {res / float(beta):.2e} after {kdim} iterations")
        y = sum(self.dtype(c) * q for c, q in zip(yk, Q))
        return y, k + 1

    def apply(self, f, adjoint=False, tol=1e-13):
        """The operator: y = (I - Phi)^-1 [forced run of Pi f].  Returns (y, GMRES iterations)."""
        return self.solve(self.forced_run(self.project(f), adjoint), adjoint, tol)

    # ---- dense forms on the free unique points ----
    def dense_inverse(self, field, adjoint=False):
        """(i omega - L)^-1 of one field on the free unique points ((-i omega - L†)^-1 if ``adjoint``)."""
        A = self.ref.dense(self.kappa[field], adjoint).astype(np.float64)
        om = -self.omega if adjoint else self.omega
        return np.linalg.inv(1j * float(om) * np.eye(A.shape[0]) - A)

    def dense_apply(self, f, adjoint=False):
        """(±i omega - L)^-1 Pi f by a dense solve per field."""
        pf = self.project(f)
        om = -self.omega if adjoint else self.omega
        out = np.zeros(pf.shape, dtype=np.complex128)
        for k in range(len(self.kappa)):
            A = self.ref.dense(self.kappa[k], adjoint).astype(np.float64)
            z = 1j * float(om) * np.eye(A.shape[0]) - A
            out[k] = self.ref.expand(np.linalg.solve(z, self.ref.restrict(pf[k]).astype(np.complex128)))
        return out

    def gains(self, field=None):
        """The squared singular values of the operator in the bm1 inner product, descending, each once (in
        the pair space each counts twice): of one field, or of all of them together."""
        sB = np.sqrt(self.ref.mass().astype(np.float64))
        fields = range(len(self.kappa)) if field is None else [field]
        sv = [np.linalg.svd(sB[:, None] * self.dense_inverse(k).astype(np.complex128) / sB[None, :], compute_uv=False)
              for k in fields]
        return np.sort(np.concatenate(sv))[::-1] ** 2
