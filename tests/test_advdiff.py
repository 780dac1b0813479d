"""The advection-diffusion operator (nekstab_next_amd/advdiff.py, csrc/advdiff.hip), CPU side: the NumPy
restatement the device is tested against (tests/advdiff_reference.py) pinned by known answers, and the ABI
surface of the new entries.

(a) analytic eigenvalues of -U.grad + kappa Lap on [0, pi]^2 with Dirichlet walls;
(b) matvec / rmatvec are adjoints in the bm1 inner product for arbitrary (unprojected) vectors;
(c) the Horner stepping equals the dense polynomial of the assembled matrix;
(d) the projector is idempotent and its image continuous and masked;
(e) header, ctypes table and ABI version."""
import os
import re

import numpy as np
import pytest

import advdiff_reference as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = np.pi


def cellular_case(dtype=np.float64):
    """The deformed 3 x 3, lx1 = 6 mesh of [0, pi]^2 with the cellular base flow and Dirichlet walls (the
    walls are those of the box before the deformation), kappa = 0.02."""
    co = ar.box_mesh_2d(6, (3, 3), (PI, PI), amp=0.04)
    x, y = co["x"], co["y"]
    U = [2.0 * np.sin(x) * np.cos(y) + 0.5, -2.0 * np.cos(x) * np.sin(y)]
    mask = ar.box_mask(ar.box_mesh_2d(6, (3, 3), (PI, PI)))
    return co, U, mask, ar.Reference(6, 2, co, U, mask=mask, dtype=dtype)


@pytest.fixture(scope="module")
def cellular():
    co, U, mask, ref = cellular_case()
    rho = float(np.max(np.abs(np.linalg.eigvals(ref.dense(0.02)))))
    return ref, 2.0 / rho


def test_analytic_eigenvalues():
    """u_t = -c u_x + kappa Lap u on [0, pi]^2, u = 0 on the walls: lambda = -kappa (k^2 + l^2) - c^2 / (4 kappa)
    (u = exp(c x / (2 kappa)) sin(k x) sin(l y)); c = 0.3, kappa = 0.05: -0.55, -0.70, -0.70.  3 x 3
    elements of lx1 = 8.  Measured 1.06e-9, 3.32e-8, 1.06e-9."""
    co = ar.box_mesh_2d(8, (3, 3), (PI, PI))
    n = co["x"].size
    ref = ar.Reference(8, 2, co, [np.full(n, 0.3), np.zeros(n)], mask=ar.box_mask(co))
    assert ref.free.size == 20 * 20
    ev = np.linalg.eigvals(ref.dense(0.05))
    ev = ev[np.argsort(-ev.real)][:3]
    err = np.abs(ev - np.array([-0.55, -0.70, -0.70]))
    print("analytic eigenvalue errors", err)
    assert np.all(err < 1e-7), err


def test_adjoint_identity(cellular):
    """sum bm1 y (P x) = sum bm1 (P^T y) x for unprojected random x, y: 40 steps at dt = 2 / rho(L)."""
    ref, dt = cellular
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(ref.n), rng.standard_normal(ref.n)
    Px = ref.propagate(x, 0.02, dt, 40)
    Pty = ref.propagate(y, 0.02, dt, 40, adjoint=True)
    lhs, rhs = np.sum(ref.bm1 * y * Px), np.sum(ref.bm1 * Pty * x)
    scale = np.sum(ref.bm1 * np.abs(y) * np.abs(Px))
    print("adjoint identity", abs(lhs - rhs) / scale)
    assert scale > 0 and abs(lhs - rhs) <= 1e-13 * scale


def test_adjoint_generator_is_the_transpose(cellular):
    """B L = (B L^T-form)^T on the free points, B the assembled mass matrix: the adjoint right-hand side
    is the transpose of the forward one, not only its propagator."""
    ref, _ = cellular
    B = ref.mass()
    A, At = ref.dense(0.02), ref.dense(0.02, adjoint=True)
    S = B[:, None] * A
    assert np.max(np.abs(S - (B[:, None] * At).T)) <= 1e-13 * np.max(np.abs(S))
    assert np.max(np.abs(S - S.T)) > 1e-3 * np.max(np.abs(S))   # and L is not self-adjoint


@pytest.mark.parametrize("adjoint", [False, True])
def test_stepping_equals_dense_polynomial(cellular, adjoint):
    ref, dt = cellular
    x = np.random.default_rng(1).standard_normal(ref.n)
    got = ref.propagate(x, 0.02, dt, 40, adjoint)
    P = ref.dense_propagator(0.02, dt, 40, adjoint)
    want = ref.expand(P @ ref.restrict(ref.project(x)))
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print("stepping vs dense polynomial", err)
    assert err <= 1e-12


def test_operator_is_non_normal(cellular):
    """sigma_1 of B^(1/2) P B^(-1/2) exceeds the spectral radius (0.842 against 0.831)."""
    ref, dt = cellular
    P = ref.dense_propagator(0.02, dt, 40)
    sB = np.sqrt(ref.mass())
    s1 = np.linalg.svd(sB[:, None] * P / sB[None, :], compute_uv=False)[0]
    rho = np.max(np.abs(np.linalg.eigvals(P)))
    print("sigma_1", s1, "rho", rho)
    assert rho < 1.0 and s1 > rho * (1 + 1e-3)


def test_projector(cellular):
    ref, _ = cellular
    x = np.random.default_rng(2).standard_normal(ref.n)
    p = ref.project(x)
    scale = np.max(np.abs(p))
    assert np.max(np.abs(ref.project(p) - p)) <= 1e-14 * scale        # idempotent
    assert np.array_equal(ref.dsavg(p), p) or np.max(np.abs(ref.dsavg(p) - p)) <= 1e-15 * scale   # continuous
    assert np.all(p[ref.mask == 0] == 0) and np.any(ref.mask == 0)     # masked
    assert np.max(np.abs(p - x)) > 0.1                                  # and it did something
    # bm1-orthogonal: <x - Pi x, Pi z> = 0
    z = ref.project(np.random.default_rng(3).standard_normal(ref.n))
    assert abs(np.sum(ref.bm1 * (x - p) * z)) <= 1e-13 * np.sum(ref.bm1 * np.abs(x) * np.abs(z))


def test_longdouble_run_is_close():
    """The dtype switch: the f64 and long double restatements differ by rounding only."""
    _, _, _, r64 = cellular_case()
    _, _, _, rld = cellular_case(np.longdouble)
    u = np.sin(r64.bm1 * 50.0)
    a, b = r64.local_rhs(u, 0.02), rld.local_rhs(u, 0.02)
    assert b.dtype == np.longdouble
    assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(a))


def test_masks():
    from nekstab_next_amd.advdiff import box_boundary_mask, mask_from_faces
    from nekstab_next_amd.layout import NekLayout
    from nekstab_next_amd.monitors import wall_faces

    co = ar.box_mesh_2d(4, (3, 2), (2.0, 1.0))
    m = box_boundary_mask(co)
    assert np.array_equal(m, ar.box_mask(co)) and 0 < m.sum() < m.size
    lay = NekLayout(ldim=2, lx1=4, lx2=2, nelgv=6)
    faces = wall_faces(lay, co, lambda x, y: np.abs(y) < 1e-12)
    mf = mask_from_faces(lay, faces)
    assert np.array_equal(mf == 0, np.abs(co["y"]) < 1e-12)
    sh = lay.shard(1, 2)
    assert mask_from_faces(sh, faces).size == sh.n_v and np.all(mask_from_faces(sh, faces) == 1)


def test_header_and_bindings():
    from nekstab_next_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "nekkrylov.h")).read()
    lib = _lib.load()
    for name, nargs in (("nkv_advdiff_rhs", 18), ("nkv_advdiff_bm1", 10), ("nkv_advdiff_stage", 12)):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTED and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][1]) == nargs
        decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
        assert decl.count(",") + 1 == nargs, name
    assert lib.nkv_abi_version() == _lib.NKV_ABI_VERSION == 3
    assert "advdiff.hip" in open(os.path.join(ROOT, "nekstab_next_amd", "csrc", "nkv_internal.h")).read()
    import nekstab_next_amd

    assert nekstab_next_amd.AdvectionDiffusion is nekstab_next_amd.advdiff.AdvectionDiffusion
