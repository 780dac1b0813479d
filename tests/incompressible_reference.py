"""NumPy restatement of the divergence-free projection and the incompressible flow of
``nekstab_next_amd.pressure`` / ``nekstab_next_amd.incompressible`` (csrc/pressure.hip), built on
``advdiff_reference.Reference`` and ``burgers_reference.Burgers``: the oracle of their tests.

The pressure lives on ``lx2 = lx1 - 2`` Gauss-Legendre points per direction and element, element-discontinuous.
With ``g[d][a]`` the cofactors of the Reference, ``D_a`` the GLL line derivative, ``I^`` the tensor product of
the Lagrange interpolation from the GLL to the Gauss points and ``w^`` that of the Gauss weights:

    D u    = w^ I^( sum_{d<ldim} sum_a g[d][a] D_a u_d )                (the weak divergence)
    D^T p  = ( sum_a D_a^T [ g[d][a] I^^T(w^ p) ] )_d                   (unassembled; the transpose of D)
    E phi  = D( minv dsavg( D^T phi ) ),    minv = mask / dsavg(bm1)
    P v    = v - minv dsavg( D^T E^+ D v )                              (velocity rows only)

When the domain is closed the constant is a (near) null vector of E and everything runs on the mean-free
pressures: ``E~ = Z E Z``, ``Z = I - 1 1^T / n``, ``b = Z D v``.  ``cg_project`` is the device's iteration:
unpreconditioned CG from 0, the mean of every ``E p`` removed, the residual tested every ``check_every``
iterations; ``project`` is the same projection through the dense pseudo-inverse of ``E~``.

``Incompressible`` is ``Burgers`` with ``P`` behind every assembled right-hand side and ``P Pi`` for ``Pi``;
its dense forms on the free points carry the projector (``P L P``, the propagator times ``P``): without it the
dense propagator has eigenvalue 1 on every non-solenoidal direction and the dense Newton is singular.

Records of tests/test_incompressible.py on the fixed 2-D case (``case2d``), which holds each to 8 times these:"""
import numpy as np

import advdiff_reference as ar
import burgers_reference as br
from nekstab_next_amd.fld import gauss_points, gll_points, interp_matrix
from nekstab_next_amd.layout import NekLayout

TRANSPOSE_D = 1.4e-17          # |<D u, p> - <u, D^T p>| / sum |terms|, random u, p (the three projector meshes)
SYMMETRY_E = 2.5e-16           # max |E - E^T| / max |E|
DT_RHO = 0.7966                # dt times the spectral radius of P L P about q_t
LEAD = (1.29775313, 1.13775864 + 0.26039568j, 1.03707006 + 0.4755569j)   # leading propagator eigenvalues
LEAD_MODULI = (1.29775313, 1.16717635, 1.14090695)
NEXT_MODULUS = 0.97623736
DENSE_TRANSPOSE = 3.4e-15      # max |M J - (M J^+)^T| over the largest entry of M J
FD_LINEARISATION = 2.1e-13     # |central difference of N - P L_B v| relative, eps = 1e-3
PROPAGATOR_ADJOINT = 1.2e-15   # |<A x, y> - <x, A^+ y>| / sum bm1 |A x| |y|
NEWTON_STEPS = 4               # dense Newton from q_t + 0.02 P Pi pert: ||F||^2 = 1.1e-4, 1.6e-9, 7.3e-17, 5.3e-30
CLOSED_RATIOS = {"closed2d": 4.2e-31, "open2d": 0.173, "closed3d": 7.9e-11}   # constant / probe Rayleigh quotients
EIG_3D = (1.3e-9, 0.0945, 41.1)   # closed3d: smallest eigenvalue of E, smallest non-zero of Z E Z, largest
# the projector at tol = 1e-13 on the three meshes of ``projector_case``, measured in f64 by ``projector_records``
# (seed 5): distance of the CG projection to the dense one, the divergence left, idempotence, self-adjointness
# in bm1 (all relative), CG iterations (tested every 8)
PROJECTOR = {
    "closed2d": dict(dist=8.3e-15, div=2.8e-15, twice=2.3e-15, selfadj=7.4e-16, iterations=104),
    "open2d": dict(dist=8.2e-15, div=3.3e-15, twice=5.4e-15, selfadj=1.7e-16, iterations=80),
    "closed3d": dict(dist=5.0e-15, div=4.1e-15, twice=2.0e-15, selfadj=3.7e-17, iterations=88),
}

PI = np.pi
CLOSED_RATIO = 1e-6


def probe_vector(n, dtype=np.float64):
    """The fixed mean-free vector of the closed-domain test: cos(1 + 2.399963 k), mean removed."""
    z = np.cos(1.0 + 2.399963 * np.arange(n)).astype(dtype)
    return z - z.mean()


class Pressure:
    def __init__(self, ref: ar.Reference, closed="auto"):
        self.ref, self.dtype, self.ldim = ref, ref.dtype, ref.ldim
        lx1 = ref.lx1
        self.m = m = lx1 - 2
        if m < 1:
            raise ValueError("lx1 >= 3")
        self.I = interp_matrix(gll_points(lx1), gauss_points(m)).astype(self.dtype)
        gw = np.polynomial.legendre.leggauss(m)[1].astype(self.dtype)
        wt = gw[None, None, :, None] * gw[None, None, None, :]
        if self.ldim == 3:
            wt = wt * gw[None, :, None, None]
        self.wt = wt
        self.nel = ref.n // (lx1 ** self.ldim)
        self.pshape = (self.nel, m if self.ldim == 3 else 1, m, m)
        self.npz = int(np.prod(self.pshape))
        self._dense, self.closed_ratio = None, None
        if isinstance(closed, str):
            one = np.ones(self.npz, dtype=self.dtype)
            z = probe_vector(self.npz, self.dtype)
            q1 = float(one @ self.E(one) / (one @ one))
            qz = float(z @ self.E(z) / (z @ z))
            self.closed_ratio = q1 / qz
            closed = self.closed_ratio < CLOSED_RATIO
        self.closed = bool(closed)

    # ---- interpolation by sum factorisation ----
    def _interp(self, A):
        I = self.I
        A = np.einsum("ai,...i->...a", I, A)
        A = np.einsum("bj,...ja->...ba", I, A)
        if self.ldim == 3:
            A = np.einsum("ck,...kba->...cba", I, A)
        return A

    def _interp_t(self, P):
        I = self.I
        if self.ldim == 3:
            P = np.einsum("ck,...cba->...kba", I, P)
        P = np.einsum("bj,...ba->...ja", I, P)
        return np.einsum("ai,...a->...i", I, P)

    # ---- the operators ----
    def div(self, u, mult=None):
        """u: (ldim, [batch,] n_v) -> ([batch,] npz)."""
        ref = self.ref
        u = np.asarray(u).astype(self.dtype)
        dv = 0
        for d in range(self.ldim):
            ud = u[d] if mult is None else mult * u[d]
            ut = ud.reshape(ud.shape[:-1] + ref.bm1_t.shape)
            dv = dv + sum(ref.g[d][a] * ref._d(a, ut) for a in range(self.ldim))
        out = self.wt * self._interp(dv)
        return out.reshape(u.shape[1:-1] + (self.npz,))

    def gradt(self, p):
        """p: ([batch,] npz) -> (ldim, [batch,] n_v), unassembled."""
        ref = self.ref
        p = np.asarray(p).astype(self.dtype)
        s = self._interp_t(self.wt * p.reshape(p.shape[:-1] + self.pshape))
        return np.stack([sum(ref._dT(a, ref.g[d][a] * s) for a in range(self.ldim)).reshape(p.shape[:-1] + (ref.n,))
                         for d in range(self.ldim)])

    def E(self, phi):
        ref = self.ref
        return self.div(ref.dsavg(self.gradt(phi)), mult=ref.minv)

    def Z(self, b):
        return b - b.mean(axis=-1, keepdims=True) if self.closed else b

    def dense_E(self):
        return self.E(np.eye(self.npz, dtype=self.dtype)).T

    def correction(self, phi):
        """minv dsavg(D^T phi): what the projection subtracts."""
        return self.ref.minv * self.ref.dsavg(self.gradt(phi))

    # ---- the projection through the dense pseudo-inverse ----
    def solver(self):
        """G with phi = G (D v): the pseudo-inverse of Z E Z (of E when open) times Z, in f64."""
        if self._dense is None:
            E = self.dense_E().astype(np.float64)
            E = 0.5 * (E + E.T)
            n = self.npz
            Zm = np.eye(n) - (1.0 / n if self.closed else 0.0)
            self._dense = np.linalg.pinv(Zm @ E @ Zm, rcond=1e-10, hermitian=True) @ Zm
        return self._dense

    def project(self, v):
        """P v on velocity rows (ldim, [batch,] n_v) through the dense pseudo-inverse."""
        v = np.asarray(v).astype(self.dtype)
        phi = self.div(v) @ self.solver().T.astype(self.dtype)
        return v - self.correction(phi)

    # ---- the projection by the device's CG ----
    def cg_project(self, v, tol=1e-12, maxiter=None, check_every=8):
        """(P v, iterations, phi): unpreconditioned CG from 0 on the (deflated) system, the residual tested
        every ``check_every`` iterations against tol ||b||; raises RuntimeError past ``maxiter``."""
        v = np.asarray(v).astype(self.dtype)
        maxiter = 2 * self.npz + 20 if maxiter is None else maxiter
        zero = self.dtype(0)
        mean = (lambda a: a.mean()) if self.closed else (lambda a: zero)
        b = self.div(v)
        r = b - mean(b)
        x = np.zeros_like(r)
        rr = r @ r
        bb = rr
        it = 0
        if bb == 0:
            return v.copy(), 0, x
        p = r.copy()
        while True:
            Ep = self.E(p)
            mu = mean(Ep)
            den = p @ Ep - mu * p.sum()
            alpha = rr / den if den != 0 else zero
            x = x + alpha * p
            r = r - alpha * (Ep - mu)
            rr_new = r @ r
            it += 1
            if it % check_every == 0 and np.sqrt(rr_new) <= tol * np.sqrt(bb):
                break
            if it >= maxiter:
                raise RuntimeError(f"CG: {it} iterations, |r|/|b| = {float(np.sqrt(rr_new / bb)):.3e}")
            p = r + (rr_new / rr if rr != 0 else zero) * p
            rr = rr_new
        return v - self.correction(x), it, x


class Incompressible(br.Burgers):
    """``Burgers`` with the projection behind every assembled right-hand side (module docstring)."""

    def __init__(self, ref, kappa, dt=None, nsteps=None, forcing=None, closed="auto"):
        self.pr = Pressure(ref, closed=closed)
        super().__init__(ref, kappa, dt, nsteps, forcing)
        self._Pd = None

    def P(self, q):
        q = np.array(q, dtype=self.dtype)
        q[: self.ldim] = self.pr.project(q[: self.ldim])
        return q

    def project(self, x):
        return self.P(self.ref.project(self._cast(x)))

    def assemble(self, r):
        return self.P(self.ref.minv * self.ref.dsavg(r))

    # ---- dense forms on the free unique points, with the projector ----
    def dense_P(self):
        if self._Pd is None:
            m = self.ref.free.size
            eye = np.eye(self.nf * m, dtype=self.dtype)
            cols = self.project(self.ref.expand(eye.reshape(self.nf * m, self.nf, m)).transpose(1, 0, 2))
            self._Pd = self.ref.restrict(cols).transpose(0, 2, 1).reshape(self.nf * m, self.nf * m)
        return self._Pd

    def dense(self, B, adjoint=False):
        return super().dense(B, adjoint) @ self.dense_P()

    def dense_propagator(self, B, adjoint=False):
        return super().dense_propagator(B, adjoint) @ self.dense_P()


# ---- the fixed 2-D case ------------------------------------------------------------------------------
CASE = dict(lx1=5, ne=(3, 3), amp=0.04, kappa=(0.02, 0.02), dt=0.05, nsteps=8, offset=0.02)


def case2d(dtype=np.float64, nsteps=None, masked=True):
    """(coords, mask, Incompressible with the steady forcing set, q_t, the Newton starting point, target, pert):
    3 x 3 elements of lx1 = 5 on [0, pi]^2 deformed by 0.04, walls of the undeformed box, layout (vx, vy)."""
    c = CASE
    co = ar.box_mesh_2d(c["lx1"], c["ne"], (PI, PI), amp=c["amp"])
    mask = ar.box_mask(ar.box_mesh_2d(c["lx1"], c["ne"], (PI, PI))) if masked else None
    x, y = co["x"], co["y"]
    ref = ar.Reference(c["lx1"], 2, co, [np.zeros_like(x), np.zeros_like(x)], mask=mask, dtype=dtype)
    ns = Incompressible(ref, c["kappa"], c["dt"], c["nsteps"] if nsteps is None else nsteps)
    target = 2.0 * np.stack([np.sin(x) ** 2 * np.sin(2 * y), -np.sin(2 * x) * np.sin(y) ** 2])
    pert = np.stack([np.sin(2 * x) * np.sin(y), np.sin(x) * np.sin(3 * y)])
    qt = ns.steady_forcing(target)
    q0 = qt + dtype(c["offset"]) * ns.project(pert)
    return co, mask, ns, qt, q0, target, pert


def projector_case(name, dtype=np.float64):
    """(lx1, ldim, coords, mask, Reference) of the three meshes the projector is tested on: the fixed 2-D mesh
    closed ("closed2d"), the same with no mask ("open2d"), and 2 x 2 x 2 elements of lx1 = 4 deformed by 0.04
    with the walls of the undeformed box ("closed3d": the constant is only nearly a null vector)."""
    if name in ("closed2d", "open2d"):
        c = CASE
        co = ar.box_mesh_2d(c["lx1"], c["ne"], (PI, PI), amp=c["amp"])
        mask = ar.box_mask(ar.box_mesh_2d(c["lx1"], c["ne"], (PI, PI))) if name == "closed2d" else None
        lx1, ldim = c["lx1"], 2
    elif name == "closed3d":
        from seed_helpers import box_mesh_coords
        from test_bf_sensitivity import deformed_box

        lx1, ldim = 4, 3
        lay = NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=8)
        co = deformed_box(lay, (2, 2, 2), amp=0.04)
        mask = ar.box_mask(box_mesh_coords(lay, (2, 2, 2)))
    else:
        raise KeyError(name)
    zero = [np.zeros(co["x"].size)] * ldim
    return lx1, ldim, co, mask, ar.Reference(lx1, ldim, co, zero, mask=mask, dtype=dtype)


def projector_records(name, tol=1e-13, seed=5):
    """The figures of PROJECTOR for one mesh, measured in f64: a random Pi-projected velocity v; the distance
    of the CG projection to the dense one, the divergence left, idempotence, self-adjointness, iterations."""
    lx1, ldim, co, mask, ref = projector_case(name)
    pr = Pressure(ref)
    rng = np.random.default_rng(seed)
    v, w = (ref.project(rng.standard_normal((ldim, ref.n))) for _ in range(2))
    Pv, it, _ = pr.cg_project(v, tol=tol)
    Pw = pr.cg_project(w, tol=tol)[0]
    dense = pr.project(v)
    scale = float(np.max(np.abs(v)))
    PPv = pr.cg_project(Pv, tol=tol)[0]
    bm = ref.bm1
    lhs, rhs = float(np.sum(bm * w * Pv)), float(np.sum(bm * Pw * v))
    return dict(dist=float(np.max(np.abs(Pv - dense))) / scale,
                div=float(np.max(np.abs(pr.Z(pr.div(Pv)))) / np.max(np.abs(pr.Z(pr.div(v))))),
                twice=float(np.max(np.abs(PPv - Pv))) / scale,
                selfadj=abs(lhs - rhs) / float(np.sum(bm * np.abs(w) * np.abs(Pv))),
                iterations=it, closed=pr.closed, ratio=pr.closed_ratio)
