"""NumPy restatement of the monitors layer (csrc/monitors.hip): the surface-force integrals of
``nekStab_torque`` (utils.f90:718-879, with Nek5000's comp_sij / drgtrq / mappr restated from their
definitions) and the update of ``nekStab_avg`` (postproc.f90:581-599).

Every function works in the dtype of its inputs, so the same code is the float64 restatement (the operand
order of the kernels, operation for operation: NumPy never contracts a product and a sum) and, fed long
double, the extended-precision reference.  Per-element arrays are (nel, pts) with r fastest."""
import numpy as np

FACES = {1: (1, -1), 2: (0, +1), 3: (1, +1), 4: (0, -1), 5: (2, -1), 6: (2, +1)}   # face -> (direction, side)


def face_index(lx1, ldim, face):
    """Element-point indices of the face's GLL points, fp = a + lx1 b over the in-face directions ascending."""
    d, side = FACES[face]
    n = lx1
    c0 = n - 1 if side > 0 else 0
    out = []
    for b in range(n if ldim == 3 else 1):
        for a in range(n):
            i, j, k = {0: (c0, a, b), 1: (a, c0, b), 2: (a, b, c0)}[d]
            out.append(i + n * j + n * n * k)
    return np.asarray(out)


def face_ab(lx1, ldim):
    nfp = lx1 ** (ldim - 1)
    fp = np.arange(nfp)
    return fp % lx1, fp // lx1


# ---- k_gradm1's arithmetic (mxm line sums with m ascending, addcol4 / subcol4, ascol5) -------------------

def _shape(A, lx1, ldim):
    return A.reshape(-1, lx1 if ldim == 3 else 1, lx1, lx1)


def d_r(D, A):
    out = D[None, None, None, :, 0] * A[..., 0:1]
    for m in range(1, A.shape[-1]):
        out = out + D[None, None, None, :, m] * A[..., m:m + 1]
    return out


def d_s(D, A):
    out = A[:, :, 0:1, :] * D[None, None, :, 0, None]
    for m in range(1, A.shape[2]):
        out = out + A[:, :, m:m + 1, :] * D[None, None, :, m, None]
    return out


def d_t(D, A):
    out = A[:, 0:1] * D[None, :, 0, None, None]
    for m in range(1, A.shape[1]):
        out = out + A[:, m:m + 1] * D[None, :, m, None, None]
    return out


def cofactors(D, coords, lx1, ldim):
    """g[d][dir] (the cofactor of direction d and reference coordinate dir) and 1/jac, each (nel, pts)."""
    X, Y = _shape(coords["x"], lx1, ldim), _shape(coords["y"], lx1, ldim)
    xr, yr, xs, ys = d_r(D, X), d_r(D, Y), d_s(D, X), d_s(D, Y)
    if ldim == 2:
        jac = 0.0 + xr * ys
        jac = jac - xs * yr
        g = [[ys, -yr], [-xs, xr]]
    else:
        Z = _shape(coords["z"], lx1, ldim)
        zr, zs = d_r(D, Z), d_s(D, Z)
        xt, yt, zt = d_t(D, X), d_t(D, Y), d_t(D, Z)
        jac = 0.0 + xr * ys * zt
        jac = jac + xt * yr * zs
        jac = jac + xs * yt * zr
        jac = jac - xr * yt * zs
        jac = jac - xs * yr * zt
        jac = jac - xt * ys * zr
        g = [[ys * zt - yt * zs, yt * zr - yr * zt, yr * zs - ys * zr],
             [xt * zs - xs * zt, xr * zt - xt * zr, xs * zr - xr * zs],
             [xs * yt - xt * ys, xt * yr - xr * yt, xr * ys - xs * yr]]
    nel = jac.shape[0]
    return [[a.reshape(nel, -1) for a in row] for row in g], (1.0 / jac).reshape(nel, -1)


def gradient(D, coords, lx1, ldim, comps):
    """G[c][d] = d u_c / d x_d as nkv_gradm1 stores it: jacmi (ur g[d][0] + us g[d][1] [+ ut g[d][2]])."""
    g, jacmi = cofactors(D, coords, lx1, ldim)
    nel = jacmi.shape[0]
    G = []
    for c in range(ldim):
        U = _shape(comps[c], lx1, ldim)
        ur, us = d_r(D, U).reshape(nel, -1), d_s(D, U).reshape(nel, -1)
        row = []
        for d in range(ldim):
            acc = ur * g[d][0] + us * g[d][1]
            if ldim == 3:
                acc = acc + d_t(D, U).reshape(nel, -1) * g[d][2]
            row.append(jacmi * acc)
        G.append(row)
    return G


# ---- the face integrand --------------------------------------------------------------------------------

def face_normals(g, wg, faces, lx1, ldim):
    """nA[face][d][fp] = +-(g[d][dir] w), w = wg[a] wg[b] (2-D wg[a])."""
    a, b = face_ab(lx1, ldim)
    w = wg[a] * wg[b] if ldim == 3 else wg[a]
    out = []
    for e, fc, _ in faces:
        d, side = FACES[fc]
        idx = face_index(lx1, ldim, fc)
        rows = [g[k][d][e, idx] * w for k in range(ldim)]
        out.append([r if side > 0 else -r for r in rows])
    return np.asarray(out).reshape(len(faces), ldim, -1)


def face_values(field, faces, lx1, ldim):
    """A mesh-1 field (nel, pts) at the face points: [face][fp]."""
    return np.asarray([field[e, face_index(lx1, ldim, fc)] for e, fc, _ in faces]).reshape(len(faces), -1)


def interp_pressure(Ip, p2, faces, lx1, lx2, ldim):
    """pm[face][fp] = sum_c Ip[k][c] (sum_b Ip[j][b] (sum_a Ip[i][a] p(a, b, c))), every sum ascending with a
    product as its first term; p2: (nel, lx2^ldim)."""
    out = []
    for e, fc, _ in faces:
        idx = face_index(lx1, ldim, fc)
        i, j, k = idx % lx1, (idx // lx1) % lx1, idx // (lx1 * lx1)
        P = p2[e].reshape(lx2 if ldim == 3 else 1, lx2, lx2)

        def line(b, c):
            s = Ip[i, 0] * P[c, b, 0]
            for m in range(1, lx2):
                s = s + Ip[i, m] * P[c, b, m]
            return s

        def plane(c):
            s = Ip[j, 0] * line(0, c)
            for m in range(1, lx2):
                s = s + Ip[j, m] * line(m, c)
            return s

        if ldim == 3:
            pm = Ip[k, 0] * plane(0)
            for m in range(1, lx2):
                pm = pm + Ip[k, m] * plane(m)
        else:
            pm = plane(0)
        out.append(pm)
    return np.asarray(out).reshape(len(faces), -1)


def add_mean_gradient(pm, xyz, dp_mean, ldim):
    for d in range(ldim):
        pm = pm + xyz[d] * dp_mean[d]
    return pm


def strain(G, faces, lx1, ldim):
    """sij[face][3 | 6][fp] = G_ij + G_ji in comp_sij's order (s11, s22, [s33,] s12[, s23, s31])."""
    pairs = [(0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (2, 0)] if ldim == 3 else [(0, 0), (1, 1), (0, 1)]
    return np.stack([face_values(G[i][j] + G[j][i], faces, lx1, ldim) for i, j in pairs], axis=1)


def _s(sij, c, d, ldim):
    if c == d:
        return sij[:, c]
    if ldim == 2:
        return sij[:, 2]
    return sij[:, {(0, 1): 3, (1, 2): 4, (0, 2): 5}[(min(c, d), max(c, d))]]


def face_terms(sij, na, pm, nu, xyz, x0, ldim):
    """T[face][3 l + k][fp]: dg(k, l) of drgtrq per face point."""
    nf, _, nfp = na.shape
    dg = np.zeros((nf, 4, 3, nfp), dtype=na.dtype)
    for c in range(ldim):
        dg[:, 0, c] = pm * na[:, c]
        acc = _s(sij, c, 0, ldim) * na[:, 0]
        acc = acc + _s(sij, c, 1, ldim) * na[:, 1]
        if ldim == 3:
            acc = acc + _s(sij, c, 2, ldim) * na[:, 2]
        dg[:, 1, c] = -nu * acc
    r1, r2 = xyz[0] - x0[0], xyz[1] - x0[1]
    r3 = (xyz[2] - x0[2]) if ldim == 3 else None
    for l in range(2):
        if ldim == 3:
            dg[:, 2 + l, 0] = r2 * dg[:, l, 2] - r3 * dg[:, l, 1]
            dg[:, 2 + l, 1] = r3 * dg[:, l, 0] - r1 * dg[:, l, 2]
        dg[:, 2 + l, 2] = r1 * dg[:, l, 1] - r2 * dg[:, l, 0]
    return dg.reshape(nf, 12, nfp)


def face_sums(T, scale):
    """dgtq[face][12]: the face's terms added one by one in ascending fp, then the scale (cmult, :811)."""
    acc = T[:, :, 0].copy()
    for p in range(1, T.shape[2]):
        acc = acc + T[:, :, p]
    return acc * scale


def object_sums(faces, dgtq, nobj):
    """[nobj + 1][12] in k_torque_objects' order: lane m mod 64 adds the object's faces in ascending table
    row m onto 0.0, the lanes meet in the butterfly xor 32, 16, 8, 4, 2, 1; row 0: the object rows in
    ascending order onto 0.0."""
    out = np.zeros((nobj + 1, 12), dtype=dgtq.dtype)
    lanes = np.arange(64)
    for o in range(1, nobj + 1):
        s = np.zeros((64, 12), dtype=dgtq.dtype)
        for m, (_, _, ob) in enumerate(faces):
            if ob == o:
                s[m % 64] = s[m % 64] + dgtq[m]
        for off in (32, 16, 8, 4, 2, 1):
            s = s + s[lanes ^ off]
        out[o] = s[0]
        out[0] = out[0] + s[0]
    return out


def torque(D, wg, coords, comps, faces, nobj, lx1, ldim, nu, pm_faces, x0=(0.0, 0.0, 0.0), scale=2.0,
           dp_mean=(0.0, 0.0, 0.0), plain_sums=False):
    """The whole chain on the faces table ``faces`` (rows (local element, face, object)); ``pm_faces``:
    the pressure at the face points before the mean-gradient term; ``nu``: a scalar or (nel, pts).
    ``plain_sums``: NumPy's own summation instead of the kernels' orders (the independent route).
    Returns (out [nobj + 1][12], dgtq, sij, na)."""
    nel = np.asarray(coords["x"]).size // lx1 ** ldim
    g, _ = cofactors(D, coords, lx1, ldim)
    G = gradient(D, coords, lx1, ldim, comps)
    return assemble(g, G, wg, coords, faces, nobj, lx1, ldim, nu, pm_faces, x0, scale, dp_mean, plain_sums, nel)


def assemble(g, G, wg, coords, faces, nobj, lx1, ldim, nu, pm_faces, x0, scale, dp_mean, plain_sums, nel):
    na = face_normals(g, wg, faces, lx1, ldim)
    sij = strain(G, faces, lx1, ldim)
    xyz = [face_values(np.asarray(coords[k]).reshape(nel, -1), faces, lx1, ldim) for k in ("x", "y", "z")[:ldim]]
    nuf = nu if np.isscalar(nu) else face_values(np.asarray(nu).reshape(nel, -1), faces, lx1, ldim)
    pm = add_mean_gradient(pm_faces, xyz, dp_mean, ldim)
    T = face_terms(sij, na, pm, nuf, xyz, x0, ldim)
    if plain_sums:
        dgtq = T.sum(axis=2) * scale
        out = np.zeros((nobj + 1, 12), dtype=dgtq.dtype)
        for o in range(1, nobj + 1):
            sel = [m for m, f in enumerate(faces) if f[2] == o]
            out[o] = dgtq[sel].sum(axis=0) if sel else 0.0
        out[0] = out[1:].sum(axis=0)
        return out, dgtq, sij, na
    dgtq = face_sums(T, scale)
    return object_sums(faces, dgtq, nobj), dgtq, sij, na


# ---- nekStab_avg -----------------------------------------------------------------------------------------

def avg_step(lay, v, avg, rms, cross, alpha, beta):
    """One update on padded host vectors (in place on avg, rms and the cross buffer [ncross][sv]); only
    live rows are touched."""
    for _, s, n in lay.field_slices():
        x = v[s:s + n]
        avg[s:s + n] = alpha * avg[s:s + n] + beta * x
        if rms is not None:
            rms[s:s + n] = alpha * rms[s:s + n] + (beta * x) * x
    if cross is not None:
        n, sv = lay.n_v, lay.sv
        vel = [v[k * sv:k * sv + n] for k in range(lay.ldim)]
        pairs = [(0, 1), (1, 2), (2, 0)] if lay.ldim == 3 else [(0, 1)]
        for m, (f, g) in enumerate(pairs):
            cross[m, :n] = alpha * cross[m, :n] + (beta * vel[f]) * vel[g]


# ---- the shared cases of tests/test_monitors.py and tests/test_gpu_monitors.py ----------------------------

X0 = (0.3, -0.2, 0.1)
DP_MEAN = (0.05, -0.02, 0.03)
NU = 0.01
CASE_NAMES = ("cyl", "box2d", "one2", "one3", "one4", "one8", "one10", "def5", "def6")


def box2d_coords(lay, ne=(3, 2), L=(2.0, 1.0), amp=0.03):
    """A conforming ne[0] x ne[1] 2-D box mesh moved by a smooth map (this rank's elements)."""
    from nekstab_next_amd.fld import gll_points

    g = 0.5 * (gll_points(lay.lx1) + 1.0)
    e0, e1 = lay.elem_range()
    xs, ys = [], []
    for e in range(e0, e1):
        ex, ey = e % ne[0], e // ne[0]
        jj, ii = np.meshgrid(g, g, indexing="ij")
        xs.append(((ex + ii) * L[0] / ne[0]).ravel())
        ys.append(((ey + jj) * L[1] / ne[1]).ravel())
    x = np.concatenate(xs) if xs else np.zeros(0)
    y = np.concatenate(ys) if ys else np.zeros(0)
    return {"x": x + amp * np.sin(2.0 * y), "y": y + amp * np.sin(1.5 * x)}


def box_boundary(ne):
    """(global element, face) of every boundary face of an ne[0] x ne[1] [x ne[2]] box mesh, elements
    ascending."""
    out = []
    three = len(ne) == 3
    for e in range(int(np.prod(ne))):
        ex, ey = e % ne[0], (e // ne[0]) % ne[1]
        if ey == 0:
            out.append((e, 1))
        if ex == ne[0] - 1:
            out.append((e, 2))
        if ey == ne[1] - 1:
            out.append((e, 3))
        if ex == 0:
            out.append((e, 4))
        if three:
            ez = e // (ne[0] * ne[1])
            if ez == 0:
                out.append((e, 5))
            if ez == ne[2] - 1:
                out.append((e, 6))
    return out


def case(name):
    """(layout, global coords, objects, ne): objects are lists of (global element, face)."""
    from nekstab_next_amd.layout import NekLayout
    from nekstab_next_amd.monitors import wall_faces
    from test_bf_sensitivity import _cyl, deformed_box

    if name == "cyl":
        lay = NekLayout(ldim=2, lx1=6, lx2=4, nelgv=1996)
        co = _cyl()
        return lay, co, [wall_faces(lay, co, lambda x, y: np.abs(np.hypot(x, y) - 0.5) < 1e-6)], None
    if name == "box2d":
        ne = (3, 2)
        lay = NekLayout(ldim=2, lx1=5, lx2=3, nelgv=6)
        b = box_boundary(ne)
        return lay, box2d_coords(lay, ne), [[m for m in b if m[1] in (1, 2)], [m for m in b if m[1] in (3, 4)]], ne
    if name.startswith("one"):
        lx1 = int(name[3:])
        lay = NekLayout(ldim=3, lx1=lx1, lx2=max(lx1 - 2, 1), nelgv=1)     # lx1 = 2: the smallest instance
        return lay, deformed_box(lay, (1, 1, 1)), [box_boundary((1, 1, 1))], (1, 1, 1)
    lx1 = int(name[3:])
    ne = (2, 3, 2)
    lay = NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=12)
    b = box_boundary(ne)
    rng = np.random.default_rng(5)
    order = rng.permutation(len(b))          # an unsorted member list
    shuffled = [b[i] for i in order]
    return lay, deformed_box(lay, ne), [shuffled[0::2], shuffled[1::2]], ne


def fields(lay, co, seed=3):
    """(velocity components, mesh-2 pressure (nel, lx2^ldim), viscosity field) on the global mesh."""
    rng = np.random.default_rng(seed)
    x, y = co["x"], co["y"]
    z = co.get("z", np.zeros_like(x))
    vel = [np.sin(1.3 * x + 0.2 * c) * np.cos(0.7 * y - 0.4 * c) + 0.2 * (c + 1) * z * x + 0.3 * z * z
           + 1e-3 * rng.standard_normal(x.size) for c in range(lay.ldim)]
    p2 = rng.standard_normal((lay.nelgv, lay.lx2 ** lay.ldim))
    nu = NU * (1.0 + 0.1 * np.cos(x + y))
    return vel, p2, nu


def faces_table(lay, objects):
    """The rows (local element, face, object) a rank of ``lay`` keeps, as monitors.Torque builds them."""
    e0, e1 = lay.elem_range()
    return [(eg - e0, fc, o) for o, mem in enumerate(objects, start=1) for eg, fc in mem if e0 <= eg < e1]


def routes(name):
    """The three host routes to the [nobj + 1][12] result of a case: the float64 restatement in the
    kernels' orders (the product's D), the independent float64 route (``oracle.gradm1``'s gradient and D,
    the host's ``map_pressure_to_mesh1``, NumPy's own summation) and the long-double reference (the
    oracle's D, every operation in extended precision)."""
    import oracle as orc
    from nekstab_next_amd import fld
    from nekstab_next_amd.sensitivity import gll_derivative
    from nekstab_next_amd.synthetic import gll_weights

    lay, co, objects, _ = case(name)
    vel, p2, nu = fields(lay, co)
    n, d, nel, nobj = lay.lx1, lay.ldim, lay.nelgv, len(objects)
    faces = faces_table(lay, objects)
    wg = gll_weights(n)
    Ip = fld.interp_matrix(fld.gauss_points(lay.lx2), fld.gll_points(n))
    restate = torque(gll_derivative(n), wg, co, vel, faces, nobj, n, d, nu,
                     interp_pressure(Ip, p2, faces, n, lay.lx2, d), X0, 2.0, DP_MEAN)[0]
    Do = orc.gll_derivative(n)
    G = [[a.reshape(nel, -1) for a in orc.gradm1(n, d, co, vel[c])] for c in range(d)]
    pm1 = fld.map_pressure_to_mesh1(p2, n, lay.lx2, d)
    ref64 = assemble(cofactors(Do, co, n, d)[0], G, wg, co, faces, nobj, n, d, nu, face_values(pm1, faces, n, d), X0,
                     2.0, DP_MEAN, True, nel)[0]
    ld = np.longdouble
    co_ld = {k: np.asarray(v).astype(ld) for k, v in co.items()}
    ref_ld = torque(Do.astype(ld), wg.astype(ld), co_ld, [v.astype(ld) for v in vel], faces, nobj, n, d, nu.astype(ld),
                    interp_pressure(Ip.astype(ld), p2.astype(ld), faces, n, lay.lx2, d), tuple(ld(a) for a in X0),
                    ld(2.0), tuple(ld(a) for a in DP_MEAN), True)[0]
    return restate, ref64, ref_ld
