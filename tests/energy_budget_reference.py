"""NumPy restatement of ``stability_energy_budget`` (core/postproc.f90:649-872), written routine by
routine as the reference does it: ``compute_production`` with one gradm1 per base component and nine
separate products, ``compute_gradients`` as gradm1 followed by dsavg of each output,
``compute_laplacian`` as four of those with the three averaged second derivatives summed afterwards,
``compute_dissipation``'s dummy sums, and ten separate ``glsc2(bm1, .)``.  It is NOT the fused form of
csrc/postproc.hip (one production pass, gradient + divergence + averaged sum): the tests compare the two.

Built on ``oracle.gradm1`` and ``oracle.coincident_average``.  ``gradm1_generic`` / ``GroupAverage`` are a
dtype-generic copy of their arithmetic, so the same chain runs in ``np.longdouble`` from the same
f64-rounded ``D`` and inputs: the distance of the two results is the restatement's own rounding error,
the unit in which the device's (equally valid, differently ordered) rounding is gated.

Fields are this rank's n_v points in Nek order; components are lists.  In 2-D every term with a z
factor is absent (zero): the reference reads never-set arrays there.
"""
import math

import numpy as np

import oracle as orc


# ---- dtype-generic copies of the oracle's gradient and averaging arithmetic ---------------------
def _mxm_r(D, A):
    out = D[None, None, None, :, 0] * A[..., 0:1]
    for m in range(1, A.shape[-1]):
        out = out + D[None, None, None, :, m] * A[..., m:m + 1]
    return out


def _mxm_s(D, A):
    out = A[:, :, 0:1, :] * D[None, None, :, 0, None]
    for m in range(1, A.shape[2]):
        out = out + A[:, :, m:m + 1, :] * D[None, None, :, m, None]
    return out


def _mxm_t(D, A):
    out = A[:, 0:1] * D[None, :, 0, None, None]
    for m in range(1, A.shape[1]):
        out = out + A[:, m:m + 1] * D[None, :, m, None, None]
    return out


def gradm1_generic(lx1, ldim, coords, u, dtype=np.float64):
    """``oracle.gradm1`` operation for operation in ``dtype`` (D is the oracle's f64 matrix, cast)."""
    D = orc.gll_derivative(lx1).astype(dtype)
    nz = lx1 if ldim == 3 else 1
    shp = (-1, nz, lx1, lx1)
    X, Y, U = (np.asarray(a).astype(dtype).reshape(shp) for a in (coords["x"], coords["y"], u))
    zero = dtype(0.0)
    one = dtype(1.0)
    xr, yr, ur = _mxm_r(D, X), _mxm_r(D, Y), _mxm_r(D, U)
    xs, ys, us = _mxm_s(D, X), _mxm_s(D, Y), _mxm_s(D, U)
    if ldim == 2:
        jac = zero + xr * ys
        jac = jac - xs * yr
        rx, ry, sx, sy = ys, -xs, -yr, xr
        jacmi = one / jac
        return [(jacmi * (ur * rx + us * sx)).ravel(), (jacmi * (ur * ry + us * sy)).ravel()]
    Z = np.asarray(coords["z"]).astype(dtype).reshape(shp)
    zr, zs = _mxm_r(D, Z), _mxm_s(D, Z)
    xt, yt, zt, ut = _mxm_t(D, X), _mxm_t(D, Y), _mxm_t(D, Z), _mxm_t(D, U)
    jac = zero + xr * ys * zt
    jac = jac + xt * yr * zs
    jac = jac + xs * yt * zr
    jac = jac - xr * yt * zs
    jac = jac - xs * yr * zt
    jac = jac - xt * ys * zr
    rx, ry, rz = ys * zt - yt * zs, xt * zs - xs * zt, xs * yt - xt * ys
    sx, sy, sz = yt * zr - yr * zt, xr * zt - xt * zr, xt * yr - xr * yt
    tx, ty, tz = yr * zs - ys * zr, xs * zr - xr * zs, xr * ys - xs * yr
    jacmi = one / jac
    return [(jacmi * (ur * rx + us * sx + ut * tx)).ravel(), (jacmi * (ur * ry + us * sy + ut * ty)).ravel(),
            (jacmi * (ur * rz + us * sz + ut * tz)).ravel()]


class GroupAverage:
    """``oracle.coincident_average`` with its grouping computed once: the groups are read off ONE oracle
    call on a random field (every group's mean is a distinct value), then each call sums a group's
    members in ascending point order and scales by 1/count, in the dtype of its argument — the
    oracle's arithmetic (tests/test_energy_budget.py holds the two bit-equal in f64)."""

    def __init__(self, coords):
        n = np.asarray(coords["x"]).size
        q = np.random.default_rng(12345).standard_normal(n)
        out = orc.coincident_average(q, coords)
        moved = np.nonzero(out != q)[0]
        _, inv = np.unique(out[moved], return_inverse=True)
        order = np.argsort(inv, kind="stable")              # members ascending within a group
        self.members = moved[order]
        self.start = np.concatenate([[0], np.cumsum(np.bincount(inv))]).astype(np.int64)
        self.count = np.diff(self.start)
        assert np.all(self.count >= 2)

    def __call__(self, q):
        out = q.copy()
        dtype = q.dtype.type
        for k in np.unique(self.count):                     # all groups of k members at once
            g = np.nonzero(self.count == k)[0]
            idx = self.members[self.start[g][:, None] + np.arange(k)[None, :]]
            s = dtype(0.0) + q[idx[:, 0]]
            for j in range(1, k):
                s = s + q[idx[:, j]]
            v = s * (dtype(1.0) / dtype(k))
            out[idx] = v[:, None]
        return out


# ---- postproc.f90:801-872, routine by routine --------------------------------------------------
def compute_production(grad, base_c, re, im, c, ldim):
    """:801-836 for base component ``c``: (prod_x, prod_y[, prod_z])."""
    dc = grad(base_c)                                       # gradm1, no dsavg
    out = []
    for d in range(ldim):
        if d == c:
            out.append(-0.5 * (re[c] ** 2 + im[c] ** 2) * dc[d])
        else:
            out.append(-0.5 * (re[c] * re[d] + im[d] * im[c]) * dc[d])
    return out


def compute_gradients(grad, average, u):
    """:838-851: gradm1, then dsavg of each output."""
    return [average(g) for g in grad(u)]


def compute_laplacian(grad, average, a, ldim):
    """:853-872: the three averaged second derivatives, then their sum."""
    da = compute_gradients(grad, average, a)
    d2 = [compute_gradients(grad, average, da[d])[d] for d in range(ldim)]
    lap = d2[0] + d2[1]
    if ldim == 3:
        lap = lap + d2[2]
    return lap


def compute_dissipation(grad, average, re, im, nu, ldim):
    """:761-799 with nu = param(2)/param(1)."""
    lap_a = [compute_laplacian(grad, average, re[c], ldim) for c in range(ldim)]
    lap_b = [compute_laplacian(grad, average, im[c], ldim) for c in range(ldim)]
    diss = 0.0 * re[0]
    for c in range(ldim):
        dummy = re[c] * lap_a[c] + im[c] * lap_b[c]
        diss = diss + dummy
    return 0.5 * diss * nu, lap_a, lap_b


def energy_budget(lx1, ldim, coords, bm1, base, re, im, nu, average=None, dtype=np.float64):
    """:716-730: energy_budget(:, 1..10) as a (10, n) array and the ten ``glsc2(bm1, .)``.  ``base``,
    ``re``, ``im``: lists of ldim component fields.  ``average``: dsavg (default the one-rank
    coincident-point average).  f64 runs on ``oracle.gradm1``; any other dtype on the generic copy,
    with every input cast from its f64 value."""
    if average is None:
        average = GroupAverage(coords)
    if dtype is np.float64:
        grad = lambda u: orc.gradm1(lx1, ldim, coords, u)  # noqa: E731
    else:
        grad = lambda u: gradm1_generic(lx1, ldim, coords, u, dtype)  # noqa: E731
    cast = lambda xs: [np.asarray(x, dtype=np.float64).astype(dtype) for x in xs]  # noqa: E731
    base, re, im = cast(base), cast(re), cast(im)
    w = np.asarray(bm1, dtype=np.float64).astype(dtype)
    nu = dtype(nu)
    fields = np.zeros((10, w.size), dtype=dtype)
    for c in range(ldim):
        for d, p in enumerate(compute_production(grad, base[c], re, im, c, ldim)):
            fields[3 * c + d] = p
    fields[9], lap_a, lap_b = compute_dissipation(grad, average, re, im, nu, ldim)
    integrals = np.array([np.sum(w * fields[i]) for i in range(10)], dtype=dtype)
    return fields, integrals, (lap_a, lap_b)


def mode_scale(ws, re, im, normalize):
    """:701-708: alpha = sqrt(norm(dRe)^2 + norm(dIm)^2) with ``inner_product``'s weights ``ws`` (bm1s,
    eigensolvers.f90:46-47) and the factor applied to both parts: alpha itself for "reference"
    (nopcmult multiplies), 1/alpha for "unit", 1 for None."""
    ip = lambda q: sum(float(np.sum(c * ws * c)) for c in q)  # noqa: E731
    alpha = math.sqrt(math.sqrt(ip(re)) ** 2 + math.sqrt(ip(im)) ** 2)
    return alpha, {"reference": alpha, "unit": 1.0 / alpha, None: 1.0}[normalize]


def pke_lines(integrals):
    """:748-753: twelve (1E15.7) records — the ten integrals, sum(1:9), sum(1:9) - integrals(10)."""
    from nekstab_next_amd.newton import fortran_e

    vals = [float(v) for v in integrals]
    total = 0.0
    for v in vals[:9]:
        total = total + v
    return [fortran_e(v, 15, 7) for v in vals + [total, total - vals[9]]]
