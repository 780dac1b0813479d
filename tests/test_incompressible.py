"""The NumPy restatement of the divergence-free projection and the incompressible flow
(tests/incompressible_reference.py) against its own records: each figure it measured is held to 8 times the
record, as tests/test_burgers.py holds the Burgers restatement.  No GPU."""
import numpy as np
import pytest

import incompressible_reference as ir

_CASE = []


def _case():
    if not _CASE:
        _CASE.append(ir.case2d())
    return _CASE[0]


@pytest.mark.parametrize("name", ["closed2d", "open2d", "closed3d"])
def test_operators_transpose_symmetry_and_null_vector(name):
    """D and D^T are transposes, E is symmetric; closed: the constant is the one (near) null vector and the
    Rayleigh-quotient test finds it; open: E is positive definite."""
    lx1, ldim, co, mask, ref = ir.projector_case(name)
    pr = ir.Pressure(ref)
    rng = np.random.default_rng(1)
    u, p = rng.standard_normal((ldim, ref.n)), rng.standard_normal(pr.npz)
    g = pr.gradt(p)
    defect = abs(float(pr.div(u) @ p - np.sum(u * g))) / float(np.sum(np.abs(u * g)))
    E = pr.dense_E()
    sym = float(np.max(np.abs(E - E.T)) / np.max(np.abs(E)))
    ev = np.linalg.eigvalsh(0.5 * (E + E.T))
    print(f"{name}: transpose {defect:.2e}, symmetry {sym:.2e}, eigenvalues {ev[0]:.3e} {ev[1]:.3e} .. {ev[-1]:.3e}, "
          f"closed ratio {pr.closed_ratio:.3e}")
    assert defect <= 8 * ir.TRANSPOSE_D and sym <= 8 * ir.SYMMETRY_E
    assert pr.closed == (name != "open2d")
    rec = ir.CLOSED_RATIOS[name]
    assert pr.closed_ratio <= 8 * rec and (pr.closed or pr.closed_ratio >= rec / 8)
    if name == "open2d":
        assert ev[0] > 0.1
    else:
        assert abs(ev[0]) < 1e-6 * ev[1] and ev[1] > 0.05
        if name == "closed2d":   # the 2-D cofactor identity holds discretely: the constant is exactly null
            assert np.max(np.abs(E @ np.ones(pr.npz))) <= 1e-12 * ev[-1]
    if name == "closed3d":   # the near-null mode plain CG cannot resolve, and what the deflation leaves
        Zm = np.eye(pr.npz) - 1.0 / pr.npz
        evz = np.linalg.eigvalsh(Zm @ (0.5 * (E + E.T)) @ Zm)
        assert 0.1 * ir.EIG_3D[0] < ev[0] < 8 * ir.EIG_3D[0]
        assert abs(evz[1] - ir.EIG_3D[1]) < 1e-3 and abs(ev[-1] - ir.EIG_3D[2]) < 0.1


@pytest.mark.parametrize("name", ["closed2d", "open2d", "closed3d"])
def test_projector_records(name):
    """The CG projection against the dense pseudo-inverse projection, the divergence left, idempotence (the
    second solve has a right-hand side of rounding noise), self-adjointness and the iteration count."""
    got, rec = ir.projector_records(name), ir.PROJECTOR[name]
    print(name, got)
    for key in ("dist", "div", "twice", "selfadj"):
        assert got[key] <= 8 * rec[key], (key, got[key], rec[key])
    assert got["iterations"] == rec["iterations"]
    assert got["iterations"] <= 2 * ir.Pressure(ir.projector_case(name)[4]).npz + 20


def test_cg_refuses_to_run_past_maxiter():
    lx1, ldim, co, mask, ref = ir.projector_case("closed2d")
    pr = ir.Pressure(ref)
    v = ref.project(np.random.default_rng(5).standard_normal((ldim, ref.n)))
    with pytest.raises(RuntimeError):
        pr.cg_project(v, tol=1e-13, maxiter=3)
    out, it, phi = pr.cg_project(np.zeros_like(v))
    assert it == 0 and not out.any() and not phi.any()


def test_steady_state_and_dense_forms():
    """q_t is an exact steady state and divergence-free; dt rho; the dense forms are adjoints in the mass
    matrix; the leading eigenvalues of the dense propagator."""
    co, mask, ns, qt, q0, target, pert = _case()
    assert np.max(np.abs(ns.N(qt))) == 0.0
    assert np.max(np.abs(ns.pr.div(qt))) <= 1e-14
    J, Ja, M = ns.dense(qt), ns.dense(qt, True), ns.mass()
    rho = float(ns.dt * np.max(np.abs(np.linalg.eigvals(J))))
    assert abs(rho - ir.DT_RHO) < 1e-3
    MJ = M[:, None] * J
    tr = float(np.max(np.abs(MJ - (M[:, None] * Ja).T)) / np.max(np.abs(MJ)))
    print(f"dt rho {rho:.4f}, dense transpose {tr:.2e}")
    assert tr <= 8 * ir.DENSE_TRANSPOSE
    P, sB = ns.dense_propagator(qt), np.sqrt(M)
    ev = np.linalg.eigvals(sB[:, None] * P / sB[None, :])
    ev = ev[np.argsort(-np.abs(ev))]
    print("leading eigenvalues", ev[:7])
    for mu, want in zip((ev[0], ev[1], ev[3]), ir.LEAD):
        assert abs(mu.real - want.real) < 1e-7 and abs(abs(mu.imag) - abs(want.imag)) < 1e-7
    assert np.allclose(np.abs(ev[[0, 1, 3]]), ir.LEAD_MODULI, atol=1e-7) and abs(abs(ev[5]) - ir.NEXT_MODULUS) < 1e-6
    # the dense forms carry the projector: without it every non-solenoidal direction has eigenvalue 1
    c = np.random.default_rng(2).standard_normal(P.shape[0])
    assert np.max(np.abs(ns.restrict(ns.propagate_lin(ns.expand(c), qt)) - P @ c)) <= 1e-12 * np.max(np.abs(c))


def test_linearisation_and_adjoint():
    co, mask, ns, qt, q0, target, pert = _case()
    rng = np.random.default_rng(3)
    v = ns.project(rng.standard_normal(qt.shape))
    eps = 1e-3
    fd = (ns.N(qt + eps * v) - ns.N(qt - eps * v)) / (2 * eps)
    L = ns.L(v, qt)
    lin = float(np.max(np.abs(fd - L)) / np.max(np.abs(L)))
    a, b = rng.standard_normal(qt.shape), rng.standard_normal(qt.shape)
    Pa, Ptb, bm = ns.propagate_lin(a, qt), ns.propagate_lin(b, qt, adjoint=True), ns.ref.bm1
    adj = abs(float(np.sum(bm * b * Pa) - np.sum(bm * Ptb * a))) / float(np.sum(bm * np.abs(Pa) * np.abs(b)))
    print(f"finite-difference linearisation {lin:.2e}, propagator adjoint identity {adj:.2e}")
    assert lin <= 8 * ir.FD_LINEARISATION and adj <= 8 * ir.PROPAGATOR_ADJOINT


def test_dense_newton_is_quadratic():
    co, mask, ns, qt, q0, target, pert = _case()
    q, hist = ns.newton(q0)
    print("Newton ||F||^2:", hist)
    assert len(hist) == ir.NEWTON_STEPS and hist[-1] < 1e-24
    assert hist[1] < 1e-3 * hist[0] and hist[2] < 1e-5 * hist[1]
    assert np.max(np.abs(q - qt)) <= 1e-12
