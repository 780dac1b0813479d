"""The time-periodic Burgers flow (nekstab_next_amd/orbit.py, nkv_burgers_tangent_rhs and nkv_orbit_stage), CPU
side: the NumPy restatement the device is tested against (tests/orbit_reference.py) pinned by its own identities
on the end-to-end case, and what the package checks without a GPU.

(a) the tangent is the Jacobian of the discrete period map: a central difference of Phi_T against it;
(b) the dense monodromy and the dense adjoint are transposes in the bm1 inner product: M P = (M P^+)^T;
(c) the end-to-end case: the dense Newton's history from Pi target, the size of the orbit, the Floquet
    multipliers, the frozen-base multiplier and the intracycle gains reproduce the recorded figures;
(d) header, ctypes table, lazy exports and the constructor's refusals.

Gates of (a) and (b): the measured figure is printed; the records are in orbit_reference.py and the test holds
each to 8 times its record, as tests/test_burgers.py does."""
import os
import re

import numpy as np
import pytest

import orbit_reference as orf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    """The end-to-end case, its dense Newton and the orbit of the converged state (run once)."""
    co, mask, ob, qt, *_ = orf.e2e_case()
    q, hist = ob.newton(qt)
    phi, orbit = ob.propagate(q)
    return ob, qt, q, hist, phi, orbit


def test_central_difference_of_the_period_map_is_the_tangent(case):
    ob, qt, q, hist, phi, orbit = case
    rng = np.random.default_rng(0)
    v = ob.bg.project(rng.standard_normal((2, ob.bg.ref.n)))
    eps = 1e-4
    fd = (ob.propagate(q + eps * v)[0] - ob.propagate(q - eps * v)[0]) / (2 * eps)
    Pv = ob.tangent(v, orbit)
    rel = float(np.max(np.abs(fd - Pv)) / np.max(np.abs(Pv)))
    print(f"central difference of Phi_T against the tangent: {rel:.2e} (record {orf.FD_LINEARISATION:.1e})")
    assert rel <= 8 * orf.FD_LINEARISATION
    # the frozen-base propagator about q(0) is not the tangent
    frozen = ob.bg.propagate_lin(v, q)
    assert np.max(np.abs(frozen - Pv)) > 1e-3 * np.max(np.abs(Pv))
    # the dense monodromy is the same map on the free unique points
    P = ob.monodromy(orbit)
    dense = ob.bg.expand(P @ ob.bg.restrict(v))
    assert np.max(np.abs(dense - Pv)) <= 1e-12 * np.max(np.abs(Pv))


def test_dense_monodromy_and_adjoint_are_transposes(case):
    ob, qt, q, hist, phi, orbit = case
    M = ob.bg.mass()
    MP, MPa = M[:, None] * ob.monodromy(orbit), M[:, None] * ob.monodromy(orbit, adjoint=True)
    assert MP.shape == (98, 98)
    defect = float(np.max(np.abs(MP - MPa.T)) / np.max(np.abs(MP)))
    print(f"dense transpose defect {defect:.2e} (record {orf.DENSE_TRANSPOSE:.1e})")
    assert defect <= 8 * orf.DENSE_TRANSPOSE
    # and the stepped adjoint is the dense one
    rng = np.random.default_rng(1)
    w = ob.bg.project(rng.standard_normal((2, ob.bg.ref.n)))
    Aw = ob.adjoint(w, orbit)
    dense = ob.bg.expand(ob.monodromy(orbit, adjoint=True) @ ob.bg.restrict(w))
    assert np.max(np.abs(dense - Aw)) <= 1e-12 * np.max(np.abs(Aw))


def test_end_to_end_case_reproduces_the_recorded_figures(case):
    ob, qt, q, hist, phi, orbit = case
    bg = ob.bg
    assert bg.ref.free.size == 49 and abs(float(bg.dt) * ob.nsteps - 1.0) < 1e-14
    print("dense Newton ||F||^2:", hist)
    assert len(hist) == 5 and hist[-1] < 1e-20
    # the history is recorded to a few digits: each figure to half a unit of its last one; the fifth is rounding
    for got, want, half in zip(hist, orf.NEWTON_HISTORY[:4], (0.5e-7, 0.5e-7, 0.5e-11, 0.5e-18)):
        assert abs(got - want) <= half, (got, want)
    assert hist[4] < 1e-28
    C2 = orf.NEWTON_C ** 2
    assert all(hist[k + 1] <= C2 * hist[k] ** 2 for k in range(4) if hist[k] > 1e-12)
    moves = max(float(np.max(np.abs(st[0] - q))) for st in orbit)
    print("the orbit moves", moves, "from its start; max|q|", np.max(np.abs(q)))
    assert abs(moves - 0.12) < 0.005 and abs(np.max(np.abs(q)) - 1.0) < 0.02
    assert np.max(np.abs(phi - q)) <= 1e-14
    mu = np.linalg.eigvals(ob.monodromy(orbit))
    mu = mu[np.argsort(-np.abs(mu))]
    print("multipliers", mu[:7])
    m0, m1 = orf.MULTIPLIERS
    assert abs(mu[0] - m0) <= 1e-9 * abs(m0)
    pair = sorted(mu[1:3], key=lambda z: -z.imag)
    assert abs(pair[0] - m1) <= 1e-9 * abs(m1) and abs(pair[1] - np.conj(m1)) <= 1e-9 * abs(m1)
    assert abs(abs(mu[3]) - 1.0545) < 1e-4 and abs(abs(mu[4]) - 1.0545) < 1e-4 and abs(abs(mu[5]) - 0.784) < 1e-3
    frozen = np.linalg.eigvals(bg.dense_propagator(q))
    frozen = frozen[np.argsort(-np.abs(frozen))][0]
    assert abs(frozen - orf.FROZEN_BASE_MULTIPLIER) <= 1e-8 and abs(frozen - m0) > 1e-3
    sB = np.sqrt(bg.mass())
    sig = np.linalg.svd(sB[:, None] * ob.monodromy(orbit) / sB[None, :], compute_uv=False) ** 2
    print("intracycle gains", sig[:2])
    assert abs(sig[0] - orf.GAIN) <= 1e-9 * orf.GAIN and abs(sig[1] - 2.0852) < 1e-4


def test_unforced_orbit_is_the_parent_flow(case):
    """Without cos and sin parts the period map is Burgers.propagate with the constant forcing, bit for bit, and
    every stage of a steady state is that state."""
    ob, qt, *_ = case
    plain = orf.Orbit(ob.bg)
    plain.g0 = ob.g0
    ob.bg.g = ob.g0
    try:
        q0 = qt + 0.02 * ob.bg.project(np.stack([np.sin(qt[0]), np.cos(qt[1])]))
        assert np.array_equal(plain.propagate(q0)[0], ob.bg.propagate(q0))
        nxt, stages = plain.step(qt, 0)
        assert all(np.array_equal(s, qt) for s in stages) and np.array_equal(nxt, qt)
    finally:
        ob.bg.g = ob.bg.dtype(0.0)


def test_long_double_variant():
    _, _, ob, qt, *_ = orf.e2e_case(nsteps=3)
    _, _, ol, qtl, *_ = orf.e2e_case(np.longdouble, nsteps=3)
    a, b = ob.propagate(qt)[0], ol.propagate(qt)[0]
    assert b.dtype == np.longdouble
    assert 0 < np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(a))
    assert orf.phase(3, 0.5, 20) == (np.cos(2.0 * np.pi * 3.5 / 20), np.sin(2.0 * np.pi * 3.5 / 20))


# ---- the package, without a GPU -------------------------------------------------------------------------
def test_header_and_bindings():
    from nekstab_next_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "nekkrylov.h")).read()
    lib = _lib.load()
    for name, nargs in (("nkv_burgers_tangent_rhs", 19), ("nkv_orbit_stage", 34)):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTED and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][1]) == nargs
        decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
        assert decl.count(",") + 1 == nargs, name
    # nkv_linconv_rhs without the adjoint switch, with a second result
    lc, bt = _lib._SIGNATURES["nkv_linconv_rhs"][1], _lib._SIGNATURES["nkv_burgers_tangent_rhs"][1]
    assert bt[:16] == lc[:16] and bt[16:] == [lc[14], lc[15], lc[17]]
    assert lib.nkv_abi_version() == _lib.NKV_ABI_VERSION == 3
    import nekstab_next_amd

    assert nekstab_next_amd.OrbitFlow is nekstab_next_amd.orbit.OrbitFlow
    assert nekstab_next_amd.OrbitPropagator is nekstab_next_amd.orbit.OrbitPropagator


def test_docstrings_name_the_buffer_size_and_the_upo_mode():
    from nekstab_next_amd import newton, orbit

    assert "4·nsteps·n_wf·sv·8" in orbit.OrbitFlow.__doc__
    assert "orbit.OrbitFlow" in newton.__doc__ and "2.2" in newton.__doc__
    assert "the orbit storage for UPOs (:82-91)" not in " ".join(newton.__doc__.split())
