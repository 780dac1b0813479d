"""NumPy restatement of the flow-diagnostics layer, routine by routine, written from the formulas:
``vortex_core``'s criteria (core/postproc.f90:2-522), Nek5000's ``filter_s0`` from its definition,
lambda2 by cyclic Jacobi sweeps, ``comp_vort3``'s curl and mass-weighted average, and the sums and records of
``nekStab_energy`` / ``nekStab_enstrophy`` (core/utils.f90:647-716).

The gradient tensor is G[i, j] = du_i/dx_j as an (ldim, ldim, n) array (0-based; the reference's
``mygi(l, i+1, j+1)``).  Every rational criterion uses only IEEE + - * / sqrt in the reference's operand
order, one NumPy operation per rounding, so it can be compared bit for bit (lambda2 included); the one
criterion with transcendental calls, the 3-D swirling strength (two cube roots), returns the scale its
comparison is gated on.
"""
import numpy as np

import oracle as orc

EPS_OMEGA = 1.0e-5


# ---- the gradient tensor and the curl ----------------------------------------------------------
def gradient_tensor(lx1, ldim, coords, vel):
    """G[i, j] = gradm1 of component i along direction j (``oracle.gradm1``, no dsavg)."""
    return np.stack([np.stack(orc.gradm1(lx1, ldim, coords, vel[c])) for c in range(ldim)])


def vorticity(G):
    """comp_vort3's curl: (g32 - g23, g13 - g31, g21 - g12) in 3-D, g21 - g12 in 2-D (one row)."""
    if G.shape[0] == 3:
        return np.stack([G[2, 1] - G[1, 2], G[0, 2] - G[2, 0], G[1, 0] - G[0, 1]])
    return np.stack([G[1, 0] - G[0, 1]])


# ---- the invariants (postproc.f90:346-435) -----------------------------------------------------
def first_inv(G):
    if G.shape[0] == 3:
        return (G[0, 0] + G[1, 1]) + G[2, 2]
    return G[0, 0] + G[1, 1]


def second_inv(G):
    if G.shape[0] == 3:
        a = G[1, 1] * G[2, 2] - G[1, 2] * G[2, 1]
        b = G[0, 0] * G[1, 1] - G[0, 1] * G[1, 0]
        c = G[2, 2] * G[0, 0] - G[0, 2] * G[2, 0]
        return (a + b) + c
    s = G[0, 0] + G[1, 1]                                   # :395-396 as written
    a = s * s
    a = a - (2.0 * G[0, 1]) * G[1, 0]
    a = a - G[0, 0] * G[0, 0]
    a = a - G[1, 1] * G[1, 1]
    return a


def third_inv(G):
    if G.shape[0] == 3:
        a = -(G[0, 0] * (G[1, 2] * G[2, 1] - G[1, 1] * G[2, 2]))
        a = a - G[0, 1] * (G[1, 0] * G[2, 2] - G[2, 0] * G[1, 2])
        a = a - G[0, 2] * (G[2, 0] * G[1, 1] - G[1, 0] * G[2, 1])
        return a
    return G[0, 0] * G[1, 1] - G[0, 1] * G[1, 0]


# ---- the criteria ---------------------------------------------------------------------------------
def compute_q(G):
    return second_inv(G)


def compute_delta(G):
    """:177-210."""
    P1, Q1, R1 = -first_inv(G), second_inv(G), -third_inv(G)
    Q = Q1 - (P1 * P1) / 3.0
    R = R1 + (((P1 * P1) * P1) * 2.0) / 27.0
    R = R - (P1 * Q1) / 3.0
    r2, q3 = R / 2.0, Q / 3.0
    return r2 * r2 + (q3 * q3) * q3


def cubic_lambda_ci(b, c, d):
    """cubicLambdaCi (:437-474), a = 1: (lci, |s| + |u|, h).  sign(abs(r)**(1/3), r) is the real cube
    root (``np.cbrt``)."""
    b, c, d = (np.asarray(a, dtype=np.float64) for a in (b, c, d))
    f = c - (1.0 / 3.0) * (b * b)
    g = 2.0 * ((b * b) * b)
    g = g - (9.0 * b) * c
    g = g + 27.0 * d
    g = g / 27.0
    g2, f3 = g / 2.0, f / 3.0
    h = g2 * g2 + (f3 * f3) * f3
    pos = h > 0.0
    sh = np.sqrt(np.where(pos, h, 0.0))
    s = np.cbrt(-g2 + sh)
    u = np.cbrt(-g2 - sh)
    lci = ((s - u) * np.sqrt(3.0)) / 2.0
    return np.where(pos, lci, 0.0), np.where(pos, np.abs(s) + np.abs(u), 0.0), h


def quad_lambda_ci(b, c):
    """quadLambdaCi (:476-500), a = 1."""
    d = b * b - 4.0 * c
    return np.where(d >= 0.0, 0.0, np.sqrt(np.abs(d)) / 2.0)


def swirling_raw(G):
    """lambda_ci before filter and square (:252-294): (lci, scale)."""
    if G.shape[0] == 3:
        lci, scale, _ = cubic_lambda_ci(-first_inv(G), second_inv(G), -third_inv(G))
        return lci, scale
    lci = quad_lambda_ci(-first_inv(G), -third_inv(G))
    return lci, np.abs(lci)


def compute_omega_jc(G):
    """:31-79 with the sums of squares taken directly (i fastest, then j)."""
    d = G.shape[0]
    sa = np.zeros_like(G[0, 0])
    sb = np.zeros_like(G[0, 0])
    for j in range(d):
        for i in range(d):
            ss = 0.5 * (G[i, j] + G[j, i])
            oo = 0.5 * (G[i, j] - G[j, i])
            sa = sa + ss * ss
            sb = sb + oo * oo
    a, b = sa * sa, sb * sb
    return b / ((a + b) + EPS_OMEGA)


def compute_antisymmetric(G):
    """:307-325, the reference's '+' kept."""
    a = G[0, 1] + G[1, 0]
    if G.shape[0] == 3:
        b, c = G[0, 2] + G[2, 0], G[1, 2] + G[2, 1]
        return ((a * a + b * b) + c * c) / 4.0
    return (a * a) / 4.0


def compute_symmetric(G):
    """:327-344."""
    B = compute_antisymmetric(G)
    if G.shape[0] == 3:
        return B + ((G[0, 0] * G[0, 0] + G[1, 1] * G[1, 1]) + G[2, 2] * G[2, 2]) / 2.0
    return B + (G[0, 0] * G[0, 0] + G[1, 1] * G[1, 1]) / 2.0


def s2_plus_o2(G):
    """The six entries (a00, a01, a02, a11, a12, a22) of A = S^2 + O^2, k ascending, S term then O term."""
    S = [[0.5 * (G[i, j] + G[j, i]) for j in range(3)] for i in range(3)]
    Om = [[0.5 * (G[i, j] - G[j, i]) for j in range(3)] for i in range(3)]

    def entry(i, j):
        acc = S[i][0] * S[0][j]
        acc = acc + Om[i][0] * Om[0][j]
        for k in (1, 2):
            acc = acc + S[i][k] * S[k][j]
            acc = acc + Om[i][k] * Om[k][j]
        return acc

    return entry(0, 0), entry(0, 1), entry(0, 2), entry(1, 1), entry(1, 2), entry(2, 2)


JACOBI_SWEEPS = 5


def _jacobi_rotate(app, aqq, apq, arp, arq):
    """One Jacobi rotation annihilating a_pq (Rutishauser's formulas); r is the third index."""
    nz = apq != 0.0
    den = np.where(nz, apq, 1.0)
    with np.errstate(over="ignore"):
        theta = (aqq - app) / (2.0 * den)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    t = np.where(nz, t, 0.0)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    return app - h, aqq + h, 0.0 * apq, c * arp - s * arq, s * arp + c * arq


def middle_eigenvalue(a00, a01, a02, a11, a12, a22, sweeps=JACOBI_SWEEPS):
    """Middle eigenvalue of a symmetric 3 x 3 matrix by ``sweeps`` cyclic Jacobi sweeps over (0,1), (0,2),
    (1,2) — only + - * / sqrt in a fixed order, so the device repeats it bit for bit — and its scale
    |tr/3| + 2 p, p = sqrt(tr (A - tr/3 I)^2 / 6) (the eigenvalues lie in tr/3 +- 2 p)."""
    q = ((a00 + a11) + a22) / 3.0
    p1 = (a01 * a01 + a02 * a02) + a12 * a12
    d0, d1, d2 = a00 - q, a11 - q, a22 - q
    scale = np.abs(q) + 2.0 * np.sqrt((((d0 * d0 + d1 * d1) + d2 * d2) + 2.0 * p1) / 6.0)
    for _ in range(sweeps):
        a00, a11, a01, a02, a12 = _jacobi_rotate(a00, a11, a01, a02, a12)
        a00, a22, a02, a01, a12 = _jacobi_rotate(a00, a22, a02, a01, a12)
        a11, a22, a12, a01, a02 = _jacobi_rotate(a11, a22, a12, a01, a02)
    lo, hi = np.minimum(a00, a11), np.maximum(a00, a11)
    return np.maximum(lo, np.minimum(hi, a22)), scale


def lambda2(G):
    """Nek5000's lambda2 (Jeong & Hussain): the middle eigenvalue of S^2 + O^2, 3-D: (value, scale)."""
    if G.shape[0] != 3:
        raise ValueError("lambda2 is 3-D only")
    return middle_eigenvalue(*s2_plus_o2(G))


RATIONAL = {"q": compute_q, "delta": compute_delta, "omega": compute_omega_jc, "symmetric": compute_symmetric,
            "assymetric": compute_antisymmetric}


# ---- filter_s0 ------------------------------------------------------------------------------------
def filter_matrix(lx1, wght=0.5, ncut=1):
    """An independent float64 build of F = Phi diag(sigma) Phi^-1 (numpy.polynomial + linalg.solve)."""
    from numpy.polynomial import legendre as L

    N = lx1 - 1
    dP = L.Legendre.basis(N).deriv()
    z = np.concatenate([[-1.0], np.sort(dP.roots().real), [1.0]])
    P = np.stack([L.Legendre.basis(k)(z) for k in range(lx1)], axis=1)
    phi = P.copy()
    for k in range(2, lx1):
        phi[:, k] = P[:, k] - P[:, k - 2]
    sigma = np.ones(lx1)
    k0 = lx1 - ncut
    for k in range(k0 + 1, lx1 + 1):
        sigma[k - 1] = 1.0 - wght * (k - k0) ** 2 / ncut ** 2
    return np.linalg.solve(phi.T, (phi * sigma[None, :]).T).T, z, phi


def filter_s0(v, F, lx1, ldim):
    """filterq's order, r then s then t, explicit loops with m ascending:
    v'(i,j,k) = sum_m F[i,m] v(m,j,k)."""
    nz = lx1 if ldim == 3 else 1
    A = np.asarray(v, dtype=np.float64).reshape(-1, nz, lx1, lx1)
    out = F[None, None, None, :, 0] * A[..., 0:1]
    for m in range(1, lx1):
        out = out + F[None, None, None, :, m] * A[..., m:m + 1]
    A = out
    out = F[None, None, :, 0, None] * A[:, :, 0:1, :]
    for m in range(1, lx1):
        out = out + F[None, None, :, m, None] * A[:, :, m:m + 1, :]
    if ldim == 3:
        A = out
        out = F[None, :, 0, None, None] * A[:, 0:1]
        for m in range(1, lx1):
            out = out + F[None, :, m, None, None] * A[:, m:m + 1]
    return out.ravel()


def vortex_core(G, name, F=None, lx1=None):
    """vortex_core (:2-29) on a gradient tensor; F = None leaves the criterion unfiltered."""
    ldim = G.shape[0]
    filt = (lambda a: filter_s0(a, F, lx1, ldim)) if F is not None else (lambda a: a)  # noqa: E731
    if name == "lambda2":
        return lambda2(G)[0]                                # never filtered (:8-9)
    if name == "swirling":
        a = filt(swirling_raw(G)[0])
        return a * a                                        # :298-302
    return filt(RATIONAL[name](G))


# ---- comp_vort3, energy, enstrophy ---------------------------------------------------------------
def comp_vort3(G, bm1, average):
    """The curl, then dssum(bm1 w)/dssum(bm1) = dsavg(bm1 w)/dsavg(bm1); ``average`` None: raw."""
    w = vorticity(G)
    if average is None:
        return w
    den = average(np.asarray(bm1, dtype=np.float64).copy())
    return np.stack([average(bm1 * row) / den for row in w])


def component_sums(w, comps):
    """glsc3(f, bm1s, f) per component, padded to three."""
    out = [float(np.sum((f * w) * f)) for f in comps]
    return out + [0.0] * (3 - len(out))


def energy_line(time, sums, pot, volume):
    """(6E15.7), utils.f90:675."""
    from nekstab_next_amd.newton import fortran_e

    eek = 0.5 / volume
    uek, vek, wek = sums
    return "".join(fortran_e(v, 15, 7) for v in (time, uek * eek, vek * eek, wek * eek, (uek + vek + wek) * eek, pot * eek))


def enstrophy_line(time, sums, volume):
    """(5E15.7), utils.f90:711."""
    from nekstab_next_amd.newton import fortran_e

    eek = 0.5 / volume
    uek, vek, wek = sums
    return "".join(fortran_e(v, 15, 7) for v in (time, uek * eek, vek * eek, wek * eek, (uek + vek + wek) * eek))
