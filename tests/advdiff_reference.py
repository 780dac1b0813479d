"""NumPy restatement of the advection-diffusion operator of ``nekstab_next_amd.advdiff`` (csrc/advdiff.hip):
the oracle of its tests, since Nek5000's scalar stepper is not part of the reference tree.

Per element, with the geometric factors of gradm1 (glmapm1 / xyzrst: cofactors ``g[d][a]``, ``jac``),
``d_d u = (1/jac) sum_a u_a g[d][a]``, ``bm1 = jac w_i w_j [w_k]`` and ``D_a^T`` the transposed line sum:

    forward:  r = -bm1 (U . grad u) + sum_a D_a^T [ sum_d (g[d][a]/jac) (-kappa bm1 d_d u) ]
    adjoint:  r =                     sum_a D_a^T [ sum_d (g[d][a]/jac) (-kappa bm1 d_d u - bm1 U_d u) ]
    L u = minv dsavg(r),  minv = mask / dsavg(bm1);      Pi x = minv dsavg(bm1 x)
    P x = p(dt L)^nsteps Pi x,  p in Horner form: w <- v + (dt/s) L w, s = 4, 3, 2, 1.

``dsavg`` sums each group of coincident points (``seeds.group_ids``) in ascending point order and scales by
1/count.  Everything runs in ``dtype`` from the same f64-rounded ``D``, weights and inputs, so the distance
between the ``np.float64`` and the ``np.longdouble`` run is the restatement's own rounding error.  Fields
may carry leading batch axes: (..., n_v)."""
import numpy as np

from nekstab_next_amd.fld import gll_points
from nekstab_next_amd.seeds import group_ids
from nekstab_next_amd.sensitivity import gll_derivative
from nekstab_next_amd.synthetic import gll_weights


def box_mesh_2d(lx1, ne=(3, 3), L=(np.pi, np.pi), amp=0.0):
    """GLL coordinates (Nek point order, elements x fastest) of a conforming ne[0] x ne[1] mesh of
    [0, L0] x [0, L1], moved by the smooth map of ``deformed_box`` restricted to x, y (z = 0):
    x + amp sin(2 y), y + amp sin(x).  Coincident points stay coincident."""
    g = 0.5 * (gll_points(lx1) + 1.0)
    xs, ys = [], []
    for e in range(ne[0] * ne[1]):
        ex, ey = e % ne[0], e // ne[0]
        jj, ii = np.meshgrid(g, g, indexing="ij")
        xs.append(((ex + ii) * L[0] / ne[0]).ravel())
        ys.append(((ey + jj) * L[1] / ne[1]).ravel())
    x, y = np.concatenate(xs), np.concatenate(ys)
    return {"x": x + amp * np.sin(2.0 * y), "y": y + amp * np.sin(x)}


def box_mask(coords, rel_tol=1e-9):
    """0 on the faces of the bounding box, 1 elsewhere."""
    xs = [np.asarray(coords[k], dtype=np.float64) for k in ("x", "y", "z") if k in coords]
    tol = rel_tol * max(float(np.ptp(x)) for x in xs)
    m = np.ones(xs[0].size)
    for x in xs:
        m[(np.abs(x - x.min()) <= tol) | (np.abs(x - x.max()) <= tol)] = 0.0
    return m


class Reference:
    def __init__(self, lx1, ldim, coords, U, mask=None, dtype=np.float64, rel_tol=1e-9):
        self.lx1, self.ldim, self.dtype = lx1, ldim, dtype
        self.D = gll_derivative(lx1).astype(dtype)
        w = gll_weights(lx1).astype(dtype)
        nz = lx1 if ldim == 3 else 1
        self.shp = (-1, nz, lx1, lx1)
        xs64 = [np.asarray(coords[k], dtype=np.float64).ravel() for k in ("x", "y", "z")[:ldim]]
        self.n = xs64[0].size
        X = [x.astype(dtype).reshape(self.shp) for x in xs64]
        # rows: coordinate c; columns: reference direction a -> dx_c / dr_a
        J = [[self._d(a, X[c]) for a in range(ldim)] for c in range(ldim)]
        if ldim == 2:
            (xr, xs), (yr, ys) = J
            jac = xr * ys - xs * yr
            g = [[ys, -yr], [-xs, xr]]                      # g[d][a]
        else:
            (xr, xs, xt), (yr, ys, yt), (zr, zs, zt) = J
            jac = xr * ys * zt + xt * yr * zs + xs * yt * zr - xr * yt * zs - xs * yr * zt - xt * ys * zr
            g = [[ys * zt - yt * zs, yt * zr - yr * zt, yr * zs - ys * zr],
                 [xt * zs - xs * zt, xr * zt - xt * zr, xs * zr - xr * zs],
                 [xs * yt - xt * ys, xt * yr - xr * yt, xr * ys - xs * yr]]
        self.jac, self.g = jac, g
        wt = w[None, None, :, None] * w[None, None, None, :]   # w_j w_i over (k, j, i)
        if ldim == 3:
            wt = wt * w[None, :, None, None]
        self.bm1_t = jac * wt
        self.bm1 = self.bm1_t.reshape(-1)
        self.U = [np.asarray(c, dtype=np.float64).astype(dtype).reshape(self.shp) for c in U]
        ext = max(float(np.ptp(x)) for x in xs64)
        gid = group_ids(xs64, rel_tol * (ext or 1.0))
        self.first, self.gid = np.unique(gid, return_index=True, return_inverse=True)[1:]   # first member, dense id
        self.gid = self.gid.reshape(-1)
        self.inv_count = dtype(1.0) / np.bincount(self.gid).astype(dtype)
        m = np.ones(self.n, dtype=dtype) if mask is None else np.asarray(mask, dtype=np.float64).astype(dtype)
        self.mask = (self.dsavg(m) > 0.95).astype(dtype)      # a point is masked when any copy is
        self.minv = self.mask / self.dsavg(self.bm1)
        self.free = np.flatnonzero(self.mask[self.first] == 1)   # unique unmasked points (group ids)

    # ---- element arithmetic ----
    def _d(self, a, A):
        """The line sum along reference direction a of fields shaped (..., k, j, i)."""
        D = self.D
        return np.einsum(("im,...m->...i", "jm,...mi->...ji", "km,...mji->...kji")[a], D, A)

    def _dT(self, a, F):
        D = self.D
        return np.einsum(("mi,...m->...i", "mj,...mi->...ji", "mk,...mji->...kji")[a], D, F)

    def grad(self, u):
        u = np.asarray(u).astype(self.dtype)
        ut = u.reshape(u.shape[:-1] + self.bm1_t.shape)
        ua = [self._d(a, ut) for a in range(self.ldim)]
        return [sum(ua[a] * self.g[d][a] for a in range(self.ldim)) / self.jac for d in range(self.ldim)]

    def local_rhs(self, u, kappa, adjoint=False):
        """The unassembled right-hand side of one field (leading batch axes allowed)."""
        u = np.asarray(u).astype(self.dtype)
        ut = u.reshape(u.shape[:-1] + self.bm1_t.shape)
        du = self.grad(u)
        kap = self.dtype(kappa)
        G = [-kap * self.bm1_t * du[d] for d in range(self.ldim)]
        if adjoint:
            G = [G[d] - self.bm1_t * self.U[d] * ut for d in range(self.ldim)]
        r = 0
        for a in range(self.ldim):
            F = sum(self.g[d][a] / self.jac * G[d] for d in range(self.ldim))
            r = r + self._dT(a, F)
        if not adjoint:
            r = r - self.bm1_t * sum(self.U[d] * du[d] for d in range(self.ldim))
        return r.reshape(u.shape)

    # ---- assembly ----
    def dsavg(self, q):
        q = np.asarray(q)
        flat = q.reshape(-1, self.n)
        out = np.empty_like(flat)
        for b in range(flat.shape[0]):
            s = np.zeros(self.inv_count.size, dtype=q.dtype)
            np.add.at(s, self.gid, flat[b])
            out[b] = (s * self.inv_count.astype(q.dtype))[self.gid]
        return out.reshape(q.shape)

    def L(self, u, kappa, adjoint=False):
        return self.minv * self.dsavg(self.local_rhs(u, kappa, adjoint))

    def project(self, x):
        return self.minv * self.dsavg(self.bm1 * np.asarray(x).astype(self.dtype))

    def propagate(self, x, kappa, dt, nsteps, adjoint=False):
        v = self.project(x)
        dt = self.dtype(dt)
        for _ in range(nsteps):
            w = v
            for s in (4, 3, 2, 1):
                w = v + dt / self.dtype(s) * self.L(w, kappa, adjoint)
            v = w
        return v

    # ---- dense forms over the free unique points ----
    def expand(self, c):
        """Continuous fields (..., n_v) from values on the free unique points (..., n_free)."""
        c = np.asarray(c)
        full = np.zeros(c.shape[:-1] + (self.inv_count.size,), dtype=c.dtype)
        full[..., self.free] = c
        return full[..., self.gid]

    def restrict(self, u):
        return np.asarray(u)[..., self.first[self.free]]

    def dense(self, kappa, adjoint=False):
        """The matrix of L on the free unique points: column j = L applied to the j-th nodal function."""
        eye = np.eye(self.free.size, dtype=self.dtype)
        return self.restrict(self.L(self.expand(eye), kappa, adjoint)).T

    def mass(self):
        """The assembled (diagonal) mass matrix on the free unique points."""
        s = np.zeros(self.inv_count.size, dtype=self.dtype)
        np.add.at(s, self.gid, self.bm1)
        return s[self.free]

    def dense_propagator(self, kappa, dt, nsteps, adjoint=False):
        A = self.dense(kappa, adjoint) * self.dtype(dt)
        I = np.eye(A.shape[0], dtype=self.dtype)
        step = I
        for s in (4, 3, 2, 1):
            step = I + A @ step / self.dtype(s)
        P = I
        for _ in range(nsteps):
            P = step @ P
        return P


def rk4_symbol(z):
    return 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24
