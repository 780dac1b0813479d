"""The restatement of the fast-diagonalisation preconditioner (tests/pressure_precond_reference.py) on its own:
the algebra of M, the records of its header, and what the preconditioner buys in iterations."""
import numpy as np
import pytest

import advdiff_reference as ar
import pressure_precond_reference as pp

from nekstab_next_amd.pressure import fdm_eigenpairs, fdm_element_scales


def _undeformed(ldim):
    """A rectilinear mesh with elements of different sizes per direction, lx1 = 5 (2-D) or 4 (3-D)."""
    if ldim == 2:
        lx1 = 5
        co = ar.box_mesh_2d(lx1, (2, 3), (2.0, 4.5))
    else:
        from nekstab_next_amd.layout import NekLayout
        from seed_helpers import box_mesh_coords

        lx1 = 4
        co = box_mesh_coords(NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=4), (2, 2, 1))
        co = {"x": co["x"], "y": 1.7 * co["y"], "z": 0.6 * co["z"]}
    ref = ar.Reference(lx1, ldim, co, [np.zeros(co["x"].size)] * ldim)
    return lx1, co, pp.PressureFDM(ref, co, closed=False)


@pytest.mark.parametrize("ldim", [2, 3])
def test_M_is_the_inverse_of_the_kronecker_sum(ldim):
    """On an undeformed mesh M_e is the dense inverse of sum_d c[e,d] (A^ in slot d, B^ elsewhere), with c the
    half-extents' (prod h) / h_d^2; dense M is symmetric positive definite and block diagonal."""
    lx1, co, pr = _undeformed(ldim)
    S, lam, A, B = pp.fdm_matrices(lx1)
    c = pr.fdm_data()[2]
    m = lx1 - 2
    assert np.allclose(S.T @ B @ S, np.eye(m), atol=1e-13) and np.allclose(S.T @ A @ S, np.diag(lam), atol=1e-12)
    assert np.all(lam > 0)
    X = [co[k].reshape(pr.nel, -1) for k in ("x", "y", "z")[:ldim]]
    h = np.stack([0.5 * np.ptp(x, axis=1) for x in X], axis=1)
    assert np.allclose(c, np.prod(h, axis=1, keepdims=True) / h ** 2, rtol=1e-13)
    Md = pr.dense_M()
    pm = m ** ldim
    for e in range(pr.nel):
        if ldim == 2:       # the first direction is the fastest index: the last Kronecker factor
            K = c[e, 0] * np.kron(B, A) + c[e, 1] * np.kron(A, B)
        else:
            K = (c[e, 0] * np.kron(B, np.kron(B, A)) + c[e, 1] * np.kron(B, np.kron(A, B))
                 + c[e, 2] * np.kron(A, np.kron(B, B)))
        blk = Md[e * pm:(e + 1) * pm, e * pm:(e + 1) * pm]
        assert np.max(np.abs(blk @ K - np.eye(pm))) <= 1e-12 * np.linalg.cond(K)
        Md[e * pm:(e + 1) * pm, e * pm:(e + 1) * pm] = 0.0
    assert np.all(Md == 0.0)                                        # nothing outside the element blocks
    Md = pr.dense_M()
    assert np.max(np.abs(Md - Md.T)) <= 1e-14 * np.max(np.abs(Md))
    assert np.linalg.eigvalsh(0.5 * (Md + Md.T)).min() > 0


def test_package_builds_the_restatements_data():
    """pressure.fdm_eigenpairs and fdm_element_scales give the restatement's S, lambda and c on a deformed mesh."""
    lx1, ldim, co, mask, ref, pr = pp.projector_pressure("closed3d")
    S, lam, c = pr.fdm_data()
    S2, lam2 = fdm_eigenpairs(lx1)
    assert np.array_equal(lam, lam2) and np.array_equal(S, S2)
    assert np.allclose(c, fdm_element_scales([co[k] for k in ("x", "y", "z")], lx1, ldim), rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", ["closed2d", "open2d", "closed3d"])
def test_projector_records(name):
    """The records of the header, regenerated (the rule of test_incompressible.py: figures within 8 times, the
    count exact)."""
    got, rec = pp.projector_records(name), pp.PROJECTOR[name]
    print(name, got)
    for key in ("dist", "div", "twice", "selfadj"):
        assert got[key] <= 8 * rec[key], (key, got[key], rec[key])
    assert got["iterations"] == rec["iterations"]


def test_flow_record():
    got = pp.flow_difference()
    print("flow difference", got)
    assert 0 < got <= 8 * pp.FLOW_DIFFERENCE


def test_resolvent_record():
    got = pp.resolvent_difference()
    print("resolvent difference", got)
    assert 0 < got <= 8 * pp.RESOLVENT_DIFFERENCE


@pytest.mark.parametrize("name", ["big2d", "big3d", "closed2d", "open2d", "closed3d"])
def test_iterations(name):
    """Tested every 8 iterations at tol = 1e-12: PCG needs at most half of CG's iterations on the two larger meshes
    and fewer on the three projector meshes; the counts are the header's."""
    cg, pcg = pp.iteration_records(name)
    print(name, cg, pcg)
    assert (cg, pcg) == pp.ITERATIONS[name]
    if name.startswith("big"):
        assert pcg <= 0.5 * cg
    else:
        assert pcg < cg


def test_pcg_refuses_to_run_past_maxiter():
    lx1, ldim, co, mask, ref, pr = pp.projector_pressure("closed2d")
    v = ref.project(np.random.default_rng(5).standard_normal((ldim, ref.n)))
    with pytest.raises(RuntimeError):
        pr.pcg_project(v, tol=1e-13, maxiter=5)
    out, it, phi = pr.pcg_project(np.zeros_like(v))
    assert it == 0 and np.all(out == 0)
