"""Flow diagnostics, CPU side: the filter matrix, the NumPy restatement (tests/vortex_reference.py)
pinned by known tensors and by numpy.linalg, the record formats and the ABI wiring of the three device
entries."""
import os
import re

import numpy as np
import pytest

import vortex_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


# ---- legendre_filter ---------------------------------------------------------------------------
@pytest.mark.parametrize("lx1", range(3, 11))
def test_legendre_filter_properties(lx1):
    """Row sums 1 (constants pass), end-point rows are unit vectors (boundary values are kept: the
    bubble modes vanish there), polynomials of degree lx1 - 2 pass, the top mode is halved; each to
    16 lx1 eps.  And the long-double build agrees with an independent float64 one."""
    from nekstab_next_amd.vortex import legendre_filter

    F = legendre_filter(lx1)
    Fref, z, phi = vr.filter_matrix(lx1)
    tol = 16 * lx1 * EPS
    assert F.shape == (lx1, lx1) and F.dtype == np.float64 and F.flags.c_contiguous
    assert np.max(np.abs(F.sum(axis=1) - 1.0)) <= tol
    unit0, unit1 = np.eye(lx1)[0], np.eye(lx1)[-1]
    assert np.max(np.abs(F[0] - unit0)) <= tol and np.max(np.abs(F[-1] - unit1)) <= tol
    zp = z ** (lx1 - 2)
    assert np.max(np.abs(F @ zp - zp)) <= tol
    top = phi[:, -1]
    assert np.max(np.abs(F @ top - 0.5 * top)) <= tol
    assert np.max(np.abs(F - Fref)) <= 1e-12


def test_legendre_filter_arguments():
    from nekstab_next_amd.vortex import legendre_filter

    with pytest.raises(ValueError, match="lx1"):
        legendre_filter(2)
    with pytest.raises(ValueError, match="ncut"):
        legendre_filter(5, ncut=4)
    F2 = legendre_filter(6, wght=0.25, ncut=2)              # sigma = (1, 1, 1, 1, 1 - 1/16, 1 - 1/4)
    _, _, phi = vr.filter_matrix(6)
    np.testing.assert_allclose(F2 @ phi[:, 4], (1 - 0.0625) * phi[:, 4], rtol=0, atol=1e-13)
    np.testing.assert_allclose(F2 @ phi[:, 5], 0.75 * phi[:, 5], rtol=0, atol=1e-13)


# ---- the restatement on known tensors ------------------------------------------------------------
def _tensor(A, n=5):
    return np.repeat(np.asarray(A, dtype=np.float64)[:, :, None], n, axis=2)


@pytest.mark.parametrize("Om", [0.7, 3.0])
def test_solid_body_rotation(Om):
    """u = (-Om y, Om x, 0): q = Om^2, vorticity (0, 0, 2 Om), swirling Om^2, delta (Om^2/3)^3,
    lambda2 = -Om^2, omega = 4 Om^4/(4 Om^4 + 1e-5) with a = 0 and b = (2 Om^2)^2."""
    G = _tensor([[0, -Om, 0], [Om, 0, 0], [0, 0, 0]])
    tol = dict(rtol=1e-14, atol=1e-300)
    np.testing.assert_allclose(vr.compute_q(G), Om ** 2, **tol)
    w = vr.vorticity(G)
    assert not w[0].any() and not w[1].any()
    np.testing.assert_allclose(w[2], 2 * Om, **tol)
    np.testing.assert_allclose(vr.vortex_core(G, "swirling"), Om ** 2, rtol=1e-14)
    np.testing.assert_allclose(vr.compute_delta(G), (Om ** 2 / 3) ** 3, rtol=1e-14)
    np.testing.assert_allclose(vr.lambda2(G)[0], -Om ** 2, rtol=1e-14)
    np.testing.assert_allclose(vr.compute_omega_jc(G), 4 * Om ** 4 / (4 * Om ** 4 + 1e-5), rtol=1e-14)
    # 2-D: omega and the single vorticity component are the same; q is 2 det as the reference writes it
    # (:395-396), and the reference hands quadLambdaCi R1 = -det where the characteristic polynomial has
    # +det (:283-288), so its 2-D swirling vanishes in a rotation and equals a^2 in a strain (a, -a)
    G2 = _tensor([[0, -Om], [Om, 0]])
    np.testing.assert_allclose(vr.compute_q(G2), 2 * Om ** 2, **tol)
    np.testing.assert_allclose(vr.vorticity(G2)[0], 2 * Om, **tol)
    assert not vr.vortex_core(G2, "swirling").any()
    np.testing.assert_allclose(vr.vortex_core(_tensor([[Om, 0], [0, -Om]]), "swirling"), Om ** 2, rtol=1e-14)
    np.testing.assert_allclose(vr.compute_omega_jc(G2), 4 * Om ** 4 / (4 * Om ** 4 + 1e-5), rtol=1e-14)


def test_pure_strain():
    """u = (a x, -a y, 0): q = -a^2, swirling 0, lambda2 = a^2; symmetric = a^2, assymetric = 0."""
    a = 1.3
    G = _tensor([[a, 0, 0], [0, -a, 0], [0, 0, 0]])
    np.testing.assert_allclose(vr.compute_q(G), -a ** 2, rtol=1e-14)
    assert not vr.vortex_core(G, "swirling").any()
    np.testing.assert_allclose(vr.lambda2(G)[0], a ** 2, rtol=1e-14)
    np.testing.assert_allclose(vr.compute_symmetric(G), a ** 2, rtol=1e-14)
    assert not vr.compute_antisymmetric(G).any()
    assert not vr.vorticity(G).any()
    assert not vr.compute_omega_jc(G).any()


def test_assymetric_keeps_the_reference_plus():
    """compute_antisymmetric adds the off-diagonal pairs (postproc.f90:320): a pure rotation gives 0, a
    pure shear-strain its square."""
    assert not vr.compute_antisymmetric(_tensor([[0, -2.0, 0], [2.0, 0, 0], [0, 0, 0]])).any()
    np.testing.assert_allclose(vr.compute_antisymmetric(_tensor([[0, 1.5, 0], [1.5, 0, 0], [0, 0, 0]])), 2.25)


def _gaussian_tensors(n=20000, seed=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((3, 3, n)) * 10.0 ** rng.uniform(-3, 3, n)[None, None, :]


LAMBDA2_GATE = 4 * 7.03e-16  # 4 x the measured worst case: see test_lambda2_vs_eigvalsh


def test_lambda2_vs_eigvalsh():
    """The middle eigenvalue (five cyclic Jacobi sweeps) against numpy.linalg.eigvalsh on 20,000 Gaussian
    tensors scaled over 1e-3 .. 1e3, error relative to ||S^2 + O^2||_F.  The trigonometric closed form
    q + 2 p sin(acos(det B/2)/3 - pi/6) measured 3e-15 on these samples but 5.7e-9 on a solid-body
    rotation (a double eigenvalue: acos near 1), above the project's 1e-12 field gate, hence Jacobi.
    Measured worst case of the Jacobi form here: 7.03e-16 (seed 7); the gate is 4 x that."""
    G = _gaussian_tensors()
    a = vr.s2_plus_o2(G)
    val, scale = vr.lambda2(G)
    A = np.empty((G.shape[2], 3, 3))
    for (i, j), e in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), a):
        A[:, i, j] = A[:, j, i] = e
    ref = np.linalg.eigvalsh(A)[:, 1]
    fro = np.sqrt(np.sum(A * A, axis=(1, 2)))
    err = np.max(np.abs(val - ref) / fro)
    print(f"lambda2 (Jacobi) vs eigvalsh: worst {err:.2e} of ||A||_F")
    assert err <= LAMBDA2_GATE
    assert np.all(scale <= 3.0 * fro) and np.all(scale > 0)
    # four sweeps already reach the same values to rounding: the fifth is margin
    v4 = vr.middle_eigenvalue(*a, sweeps=4)[0]
    assert np.max(np.abs(v4 - val) / fro) <= LAMBDA2_GATE


def test_lambda2_degenerate_tensors():
    """A = q I, double eigenvalues and a rotated double eigenvalue: no NaN, the middle value to rounding."""
    z = np.zeros((3, 3, 2))
    assert np.array_equal(vr.lambda2(z)[0], np.zeros(2))
    G = _tensor(np.diag([2.0, 2.0, 2.0]))                   # S = 2 I: A = 4 I
    np.testing.assert_array_equal(vr.lambda2(G)[0], 4.0)
    G = _tensor(np.diag([1.0, 1.0, 3.0]))                   # A = diag(1, 1, 9): middle 1
    np.testing.assert_array_equal(vr.lambda2(G)[0], 1.0)
    # a solid-body rotation about a tilted axis: A = -W^2 (I - n n^T), eigenvalues (-W^2, -W^2, 0)
    n = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    W = 1.7
    cross = W * np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    np.testing.assert_allclose(vr.lambda2(_tensor(cross))[0], -W * W, rtol=1e-14)


def test_cubic_lambda_ci_vs_eigvals():
    """cubicLambdaCi against the imaginary part of numpy.linalg.eigvals on 20,000 Gaussian tensors: the
    classification zero / nonzero agrees on every sample whose discriminant h is not within rounding of
    zero (none of the 20,000 is).  The values are compared at sqrt(128 eps) ||G||_F = 1.7e-7 ||G||_F: the
    imaginary part of a nearly double root is the square root of a discriminant that both routes form
    with an absolute error of order 100 eps ||G||^2 (measured worst case 9.8e-8)."""
    G = _gaussian_tensors(seed=8)
    lci, scale, h = vr.cubic_lambda_ci(-vr.first_inv(G), vr.second_inv(G), -vr.third_inv(G))
    ev = np.linalg.eigvals(np.moveaxis(G, 2, 0))
    ref = np.max(ev.imag, axis=1)
    nrm = np.sqrt(np.sum(G * G, axis=(0, 1)))
    assert np.array_equal(lci > 0, ref > 0)
    assert np.all(lci >= 0)
    err = np.max(np.abs(lci - ref) / nrm)
    print(f"cubicLambdaCi vs eigvals: worst {err:.2e} of ||G||_F")
    assert err <= np.sqrt(128 * EPS)
    assert np.all(scale[lci > 0] > 0)


def test_quad_lambda_ci_vs_eigvals():
    """quadLambdaCi(b, c) on lambda^2 + b lambda + c with the polynomial's own coefficients (-tr, det)."""
    rng = np.random.default_rng(9)
    G = rng.standard_normal((2, 2, 5000))
    lci = vr.quad_lambda_ci(-vr.first_inv(G), vr.third_inv(G))
    ref = np.max(np.linalg.eigvals(np.moveaxis(G, 2, 0)).imag, axis=1)
    assert np.array_equal(lci > 0, ref > 0)
    np.testing.assert_allclose(lci, ref, rtol=0, atol=1e-12)


def test_filter_restatement_matches_matrix_form():
    """The explicit ascending-m loops equal the Kronecker form to rounding, keep polynomials of degree
    lx1 - 2 per direction and the element's boundary values."""
    from nekstab_next_amd.vortex import legendre_filter

    lx1 = 5
    F = legendre_filter(lx1)
    rng = np.random.default_rng(1)
    v = rng.standard_normal((3, lx1, lx1, lx1))
    got = vr.filter_s0(v, F, lx1, 3).reshape(v.shape)
    want = np.einsum("kc,jb,ia,ecba->ekji", F, F, F, v)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
    z = vr.filter_matrix(lx1)[1]
    X, Y, Z = np.meshgrid(z, z, z, indexing="ij")           # any axis order: the field is symmetric in use
    poly = (1 + X + X ** 3) * (2 - Y ** 2) * (Z ** 3 - Z)
    np.testing.assert_allclose(vr.filter_s0(poly, F, lx1, 3), poly.ravel(), rtol=0, atol=3 * lx1 * EPS * 8 * 8)
    got2 = vr.filter_s0(v[:, 0], F, lx1, 2).reshape(3, lx1, lx1)
    np.testing.assert_allclose(got2, np.einsum("jb,ia,eba->eji", F, F, v[:, 0]), rtol=0, atol=1e-14)
    np.testing.assert_allclose(got2[:, 0, 0], v[:, 0, 0, 0], rtol=0, atol=1e-14)   # corners are kept


# ---- records ------------------------------------------------------------------------------------
def test_monitor_records_through_fortran_e():
    from nekstab_next_amd.newton import fortran_e
    from nekstab_next_amd.vortex import energy_record, enstrophy_record

    sums = [2.0, 0.5, 0.25, -3.0]
    eek = 0.5 / 4.0
    line = energy_record(1.5, sums, eek)
    assert len(line) == 90
    assert line == ("  0.1500000E+01  0.2500000E+00  0.6250000E-01  0.3125000E-01  0.3437500E+00 -0.3750000E+00")
    assert line == vr.energy_line(1.5, sums[:3], sums[3], 4.0)
    line = enstrophy_record(0.0, sums, eek)
    assert len(line) == 75 and line.startswith("  0.0000000E+00  0.2500000E+00")
    assert line == vr.enstrophy_line(0.0, sums[:3], 4.0)
    assert line[60:] == fortran_e((2.0 + 0.5 + 0.25) * eek, 15, 7)


# ---- ABI wiring -----------------------------------------------------------------------------------
def test_entries_are_declared_typed_and_built():
    import __graft_entry__ as ge
    from nekstab_next_amd import _lib
    from nekstab_next_amd import vortex

    hdr = open(os.path.join(ROOT, "include", "nekkrylov.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("nkv_vortex_criteria", 17), ("nkv_filter_s0", 10), ("nkv_energy_components", 10)):
        assert name in _lib.EXPORTED
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib._SIGNATURES[name][1]), name
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define NKV_ABI_VERSION 3\b", hdr) and _lib.NKV_ABI_VERSION == 3
    # the enum, the Python constants and the name table agree
    enum = re.search(r"enum nkv_vortex_criterion \{(.*?)\};", code, flags=re.S).group(1)
    codes = {k: int(v) for k, v in re.findall(r"(NKV_VC_[A-Z0-9_]+)\s*=\s*(\d+)", enum)}
    assert len(codes) == 10 and codes["NKV_VC_COUNT"] == 9
    for k, v in codes.items():
        assert getattr(_lib, k) == v, k
    assert {f"NKV_VC_{n.upper()}": c for n, c in vortex.CRITERIA.items()} == {k: v for k, v in codes.items()
                                                                               if k != "NKV_VC_COUNT"}
    assert set(vortex.VORTEX_NAMES) == set(vortex.CRITERIA) - {"vorticity", "lambda_ci"}
    for cite in ("postproc.f90:2-522", "utils.f90:647-716", "utils.f90:420-444"):
        assert cite in hdr, cite
    src = os.path.join(ROOT, "nekstab_next_amd", "csrc", "vortex.hip")
    assert src in ge.HIP_SRCS
    body = open(src).read()
    assert "#pragma clang fp contract(off)" in body and "atomic" not in body
    # one copy of the tiling helpers, in the shared header
    internal = open(os.path.join(ROOT, "nekstab_next_amd", "csrc", "nkv_internal.h")).read()
    post = open(os.path.join(ROOT, "nekstab_next_amd", "csrc", "postproc.hip")).read()
    for helper in ("struct TilePoint", "void geometric_factors", "void line_sums", "double physical_derivative",
                   "constexpr int tile_pts", "constexpr int tile_threads", "inline int tile_epb"):
        assert helper in internal and helper not in body and helper not in post, helper


def test_package_exports_the_module():
    import nekstab_next_amd as pkg
    from nekstab_next_amd import vortex

    assert pkg.vortex is vortex
    for name in vortex.__all__:
        assert hasattr(vortex, name), name


def test_hooks_default_off():
    import inspect

    from nekstab_next_amd.fixedp import SFD, TDF
    from nekstab_next_amd.krylov_schur import outpost_ks

    assert inspect.signature(outpost_ks).parameters["vorticity"].default is None
    assert inspect.signature(SFD.__init__).parameters["monitors"].default == ()
    assert inspect.signature(TDF.__init__).parameters["monitors"].default == ()
