"""The viscous Burgers flow (nekstab_next_amd/burgers.py, nkv_linconv_rhs and nkv_rk4_stage), CPU side: the
NumPy restatement the device is tested against (tests/burgers_reference.py) pinned by its own identities on the
end-to-end case, and what the package checks without a GPU.

(a) the coupled linearisation and its adjoint are transposes in the bm1 inner product: dense M J = (M J^+)^T;
(b) N is quadratic, so a central difference of N is L_B v to rounding at any step;
(c) q_t is an exact steady state, the dense frozen-base Newton reaches it quadratically, and the dense
    propagator about it is unstable only through the production term;
(d) constructor checks, the resolvent's refusal, header, ctypes table and lazy exports.

Gates of (a) and (b): the measured figure is printed; the records are in burgers_reference.py (and DESIGN §9)
and the test holds each to 8 times its record, the margin ``_gate`` of tests/test_gpu_advdiff.py gives a
rounding error."""
import os
import re
import types

import numpy as np
import pytest

import advdiff_reference as ar
import burgers_reference as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    return br.e2e_case()


def test_dense_linearisation_and_adjoint_are_transposes(case):
    _, _, bg, qt, *_ = case
    M = bg.mass()
    MJ, MJa = M[:, None] * bg.dense(qt), M[:, None] * bg.dense(qt, adjoint=True)
    assert MJ.shape == (2 * 196, 2 * 196)
    defect = float(np.max(np.abs(MJ - MJa.T)) / np.max(np.abs(MJ)))
    print(f"dense transpose defect {defect:.2e} (record {br.DENSE_TRANSPOSE:.1e})")
    assert defect <= 8 * br.DENSE_TRANSPOSE
    # the production term is there: without it the two velocity components do not couple
    assert np.max(np.abs(MJ[:196, 196:])) > 1e-3 * np.max(np.abs(MJ))


def test_central_difference_of_the_generator_is_the_linearisation(case):
    _, _, bg, qt, *_ = case
    rng = np.random.default_rng(0)
    v = bg.project(rng.standard_normal((2, bg.ref.n)))
    Lv = bg.L(v, qt)
    eps = 1e-3
    fd = (bg.N(qt + eps * v) - bg.N(qt - eps * v)) / (2 * eps)
    rel = float(np.max(np.abs(fd - Lv)) / np.max(np.abs(Lv)))
    print(f"central difference against L_B v: {rel:.2e} (record {br.FD_LINEARISATION:.1e})")
    assert rel <= 8 * br.FD_LINEARISATION
    # a larger step changes nothing but rounding: N is exactly quadratic
    fd2 = (bg.N(qt + 0.5 * v) - bg.N(qt - 0.5 * v)) / 1.0
    assert np.max(np.abs(fd2 - Lv)) <= 8 * br.FD_LINEARISATION * np.max(np.abs(Lv))


def test_steady_state_newton_and_spectrum(case):
    _, _, bg, qt, q0, *_ = case
    assert np.max(np.abs(bg.N(qt))) == 0.0                          # -a + a, point by point
    assert np.array_equal(bg.step(qt), qt)                          # every stage equals q_t
    dt_rho = bg.dt * np.max(np.abs(np.linalg.eigvals(bg.dense(qt))))
    assert abs(dt_rho - 1.66) < 0.01                                # inside RK4's 2.78
    q, hist = bg.newton(q0)
    print("dense Newton ||F||^2:", hist, "max|q - q_t|", np.max(np.abs(q - qt)))
    assert len(hist) == 5 and hist[-1] < 1e-20
    np.testing.assert_allclose(hist[:4], [3.3e-3, 2.2e-6, 3.6e-10, 1.0e-17], rtol=0.05)
    # quadratic: ||F_k+1|| <= C ||F_k||^2 with C ~ 9 here (ratios 0.45, 8.6, 8.7), held as C^2 = 200 on ||F||^2
    assert all(hist[i + 1] <= 200.0 * hist[i] ** 2 for i in range(3))
    assert np.max(np.abs(q - qt)) <= 1e-14
    mu = np.linalg.eigvals(bg.dense_propagator(qt))
    mu = mu[np.argsort(-np.abs(mu))]
    assert abs(mu[0] - 1.168724411411) < 1e-10
    assert abs(abs(mu[1]) - 1.145783) < 1e-6 and abs(abs(mu[3]) - 1.083103) < 1e-6
    # the parent operator about the same flow (no production term) is stable
    ref = ar.Reference(6, 2, case[0], [qt[0], qt[1]], mask=case[1])
    P0 = [np.max(np.abs(np.linalg.eigvals(ref.dense_propagator(k, float(bg.dt), bg.nsteps)))) for k in bg.kappa]
    assert abs(max(P0) - 0.866) < 1e-3
    # the adjoint propagator has the same spectrum
    mua = np.linalg.eigvals(bg.dense_propagator(qt, adjoint=True))
    mua = mua[np.argsort(-np.abs(mua))]
    assert np.max(np.abs(np.sort_complex(mu[:5]) - np.sort_complex(mua[:5]))) < 1e-12


def test_long_double_variant(case):
    _, _, bg, qt, q0, *_ = case
    _, _, bl, qtl, q0l, *_ = br.e2e_case(np.longdouble)
    a, b = bg.L(q0, qt), bl.L(q0, qt)
    assert b.dtype == np.longdouble
    assert 0 < np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(a))


# ---- the package, without a GPU -------------------------------------------------------------------------
def _stub_ctx():
    from nekstab_next_amd.layout import NekLayout

    return types.SimpleNamespace(layout=NekLayout(ldim=2, lx1=6, lx2=4, nelgv=9))


def test_constructor_checks(case):
    from nekstab_next_amd.burgers import LinearisedConvection, ViscousBurgers

    co = case[0]
    ctx = _stub_ctx()
    n = ctx.layout.n_v
    good = [np.zeros(n), np.zeros(n)]
    with pytest.raises(ValueError, match="n_wf=2"):
        LinearisedConvection(ctx, co, good[:1], 0.05, 0.05, 4)
    with pytest.raises(ValueError, match="n_wf=2"):
        LinearisedConvection(ctx, co, good + good[:1], 0.05, 0.05, 4)
    with pytest.raises(ValueError, match=r"base\[1\]"):
        LinearisedConvection(ctx, co, [np.zeros(n), np.zeros(n - 1)], 0.05, 0.05, 4)
    with pytest.raises(ValueError, match="dt"):
        LinearisedConvection(ctx, co, good, 0.05, 0.0, 4)
    with pytest.raises(ValueError, match="nsteps"):
        LinearisedConvection(ctx, co, good, 0.05, 0.05, 0)
    with pytest.raises(ValueError, match="dt"):
        ViscousBurgers(ctx, co, 0.05, -1.0, 4)
    with pytest.raises(ValueError, match="nsteps"):
        ViscousBurgers(ctx, co, 0.05, 0.05, 0)


def test_resolvent_refuses_the_coupled_operator():
    from nekstab_next_amd.burgers import LinearisedConvection
    from nekstab_next_amd.resolvent import ResolventOperator

    op = object.__new__(LinearisedConvection)
    with pytest.raises(ValueError, match="production term"):
        ResolventOperator(None, op, 1.0)


def test_header_and_bindings():
    from nekstab_next_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "nekkrylov.h")).read()
    lib = _lib.load()
    for name, nargs in (("nkv_linconv_rhs", 18), ("nkv_rk4_stage", 20)):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTED and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][1]) == nargs
        decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
        assert decl.count(",") + 1 == nargs, name
    assert _lib._SIGNATURES["nkv_linconv_rhs"] == _lib._SIGNATURES["nkv_advdiff_rhs"]   # U, U_stride -> B, B_stride
    assert lib.nkv_abi_version() == _lib.NKV_ABI_VERSION == 3
    import nekstab_next_amd

    assert nekstab_next_amd.LinearisedConvection is nekstab_next_amd.burgers.LinearisedConvection
    assert nekstab_next_amd.ViscousBurgers is nekstab_next_amd.burgers.ViscousBurgers
