"""Eigenmode kinetic-energy budget (core/postproc.f90:649-872), CPU side: the NumPy restatement
(tests/energy_budget_reference.py) pinned by known answers, the ABI wiring of the three device
entries and the text records of ``PKE_dRe<session>0.f<mode>``.

* a base flow linear in the coordinates, U_c = A[c].x, on a deformed box: an isoparametric element
  holds it exactly, so P[c][d] = -0.5 (re_c re_d + im_d im_c) A[c][d] pointwise;
* modes quadratic in the coordinates on the affine box (lx1 = 5, 8): first derivatives are linear and
  continuous (dsavg changes nothing beyond rounding), Laplacians are the constants 2 tr(Q), so the
  dissipation is a known polynomial;
* the routine-by-routine form equals the tensor form;
* the restatement's cached averaging equals ``oracle.coincident_average`` bit for bit, and its
  dtype-generic gradient equals ``oracle.gradm1`` bit for bit in f64."""
import os
import re

import numpy as np
import pytest

import energy_budget_reference as ebr
import oracle as orc
from seed_helpers import box_mesh_coords
from test_bf_sensitivity import deformed_box

from nekstab_next_amd.layout import NekLayout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

A_BASE = np.array([[0.3, -0.2, 0.1], [0.05, 0.4, -0.3], [0.2, 0.1, 0.6]])


def _smooth_modes(co, ldim, seed=0):
    rng = np.random.default_rng(seed)
    x, y = co["x"], co["y"]
    z = co.get("z", np.zeros_like(x))
    re = [np.sin(0.9 * x + 0.4 * c) * np.cos(0.7 * y) + 0.1 * z + 1e-3 * rng.standard_normal(x.size) for c in range(ldim)]
    im = [np.cos(0.6 * x) * np.sin(1.1 * y + 0.3 * c) - 0.2 * z + 1e-3 * rng.standard_normal(x.size) for c in range(ldim)]
    return re, im


def test_production_linear_base_flow_known_answer():
    ne = (3, 2, 2)
    lay = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=12)
    co = deformed_box(lay, ne)
    base = [A_BASE[c, 0] * co["x"] + A_BASE[c, 1] * co["y"] + A_BASE[c, 2] * co["z"] + 0.5 for c in range(3)]
    re, im = _smooth_modes(co, 3)
    bm1 = np.random.default_rng(1).uniform(0.5, 1.5, lay.n_v)
    fields, integrals, _ = ebr.energy_budget(5, 3, co, bm1, base, re, im, 0.02, average=lambda q: q)
    for c in range(3):
        for d in range(3):
            want = -0.5 * (re[c] * re[d] + im[d] * im[c]) * A_BASE[c, d]
            np.testing.assert_allclose(fields[3 * c + d], want, rtol=0, atol=1e-9)
            assert abs(integrals[3 * c + d] - np.sum(bm1 * want)) <= 1e-9 * np.sum(bm1 * np.abs(want))


def quadratic_modes(co, seed=4):
    """(re, im, lap_re, lap_im): components x^T Q x + b.x with random symmetric Q; Lap = 2 tr Q."""
    rng = np.random.default_rng(seed)
    X = np.stack([co["x"], co["y"], co["z"]])
    out = []
    for _ in range(2):
        comps, laps = [], []
        for _c in range(3):
            Q = rng.uniform(-0.5, 0.5, (3, 3))
            Q = 0.5 * (Q + Q.T)
            b = rng.uniform(-1, 1, 3)
            comps.append(np.einsum("in,ij,jn->n", X, Q, X) + b @ X + 0.3)
            laps.append(2.0 * np.trace(Q))
        out += [comps, laps]
    return out[0], out[2], out[1], out[3]


@pytest.mark.parametrize("lx1", [5, 8])
def test_dissipation_quadratic_modes_known_answer(lx1):
    ne = (2, 2, 3)
    lay = NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=12)
    co = box_mesh_coords(lay, ne)
    re, im, lre, lim = quadratic_modes(co)
    base = [co["x"], co["y"], co["z"]]
    bm1 = np.random.default_rng(2).uniform(0.5, 1.5, lay.n_v)
    nu = 0.02
    fields, integrals, (lap_a, lap_b) = ebr.energy_budget(lx1, 3, co, bm1, base, re, im, nu)
    for c in range(3):
        np.testing.assert_allclose(lap_a[c], lre[c], rtol=0, atol=1e-8)
        np.testing.assert_allclose(lap_b[c], lim[c], rtol=0, atol=1e-8)
    want = 0.5 * nu * sum(re[c] * lre[c] + im[c] * lim[c] for c in range(3))
    np.testing.assert_allclose(fields[9], want, rtol=0, atol=1e-8)
    assert abs(integrals[9] - np.sum(bm1 * want)) <= 1e-8 * np.sum(bm1 * np.abs(want))


@pytest.mark.parametrize("ldim", [2, 3])
def test_routine_form_equals_tensor_form(ldim):
    """With gradients and Laplacians given, the routine-by-routine sums are the tensor expressions
    P_cd = -1/2 (re_c re_d + im_c im_d) G_cd and diss = nu/2 sum_c (re_c L^re_c + im_c L^im_c); the 2-D
    budget leaves entries 3, 6, 7, 8, 9 at zero."""
    rng = np.random.default_rng(9 + ldim)
    n = 257
    re, im = rng.standard_normal((ldim, n)), rng.standard_normal((ldim, n))
    G = rng.standard_normal((ldim, ldim, n))          # G[c, d] = d base_c / d x_d
    Lr, Li = rng.standard_normal((ldim, n)), rng.standard_normal((ldim, n))
    base = [np.full(n, float(c)) for c in range(ldim)]   # tags: grad() recognises the component
    grad = lambda u: list(G[int(u[0])])  # noqa: E731
    P = np.zeros((10, n))
    for c in range(ldim):
        for d, p in enumerate(ebr.compute_production(grad, base[c], list(re), list(im), c, ldim)):
            P[3 * c + d] = p
    want = -0.5 * (np.einsum("cn,dn->cdn", re, re) + np.einsum("cn,dn->cdn", im, im)) * G
    for c in range(ldim):
        for d in range(ldim):
            np.testing.assert_allclose(P[3 * c + d], want[c, d], rtol=0, atol=1e-13)
    if ldim == 2:
        assert not P[[2, 5, 6, 7, 8]].any()
    # the dissipation's dummy sums, from Laplacians handed in through a stub of compute_laplacian
    laps = iter(list(Lr) + list(Li))
    orig = ebr.compute_laplacian
    ebr.compute_laplacian = lambda *a: next(laps)
    try:
        diss, _, _ = ebr.compute_dissipation(None, None, list(re), list(im), 0.02, ldim)
    finally:
        ebr.compute_laplacian = orig
    np.testing.assert_allclose(diss, 0.01 * (np.sum(re * Lr, axis=0) + np.sum(im * Li, axis=0)), rtol=0, atol=1e-13)


def test_restatement_helpers_equal_the_oracle_bitwise():
    ne = (3, 2, 2)
    lay = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=12)
    co = deformed_box(lay, ne)
    avg = ebr.GroupAverage(co)
    rng = np.random.default_rng(3)
    for _ in range(2):
        q = rng.standard_normal(lay.n_v)
        assert np.array_equal(avg(q), orc.coincident_average(q, co))
        for a, b in zip(ebr.gradm1_generic(5, 3, co, q), orc.gradm1(5, 3, co, q)):
            assert np.array_equal(a, b)
    # a 2-D mesh: the z = 0 face of every element of the 3 x 2 x 1 box
    lay2 = NekLayout(ldim=2, lx1=4, lx2=2, nelgv=6)
    box = box_mesh_coords(NekLayout(ldim=3, lx1=4, lx2=2, nelgv=6), (3, 2, 1))
    co2 = {k: box[k].reshape(6, 4, 16)[:, 0].ravel() for k in ("x", "y")}
    q = rng.standard_normal(lay2.n_v)
    assert np.array_equal(ebr.GroupAverage(co2)(q), orc.coincident_average(q, co2))
    for a, b in zip(ebr.gradm1_generic(4, 2, co2, q), orc.gradm1(4, 2, co2, q)):
        assert np.array_equal(a, b)
    # and in long double the same chain runs, close to the f64 one
    q = rng.standard_normal(lay.n_v)
    ld = ebr.gradm1_generic(5, 3, co, q, np.longdouble)
    assert ld[0].dtype == np.longdouble
    assert np.max(np.abs(ld[0].astype(np.float64) - orc.gradm1(5, 3, co, q)[0])) < 1e-11


def test_restatement_rounding_error_is_measurable():
    """e_ref = max |f64 - long double| of the restatement: the unit the device gates use for the
    Laplacian-borne quantities; positive and small against the field's scale."""
    ne = (2, 2, 1)
    lay = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=4)
    co = deformed_box(lay, ne)
    re, im = _smooth_modes(co, 3, seed=2)
    base = [np.cos(co["x"]) * co["y"], np.sin(co["y"] + co["z"]), co["x"] * co["z"]]
    bm1 = np.random.default_rng(5).uniform(0.5, 1.5, lay.n_v)
    avg = ebr.GroupAverage(co)
    f64, i64, _ = ebr.energy_budget(5, 3, co, bm1, base, re, im, 0.02, average=avg)
    fld_, ild, _ = ebr.energy_budget(5, 3, co, bm1, base, re, im, 0.02, average=avg, dtype=np.longdouble)
    assert fld_.dtype == np.longdouble
    scale = np.max(np.abs(f64[9]))
    e_ref = float(np.max(np.abs(f64[9] - fld_[9])))
    assert 0 < e_ref < 1e-9 * scale
    assert abs(float(i64[9] - ild[9])) < 1e-9 * np.sum(bm1 * np.abs(f64[9]))


def test_mode_scale_follows_the_reference():
    rng = np.random.default_rng(6)
    ws = rng.uniform(0.5, 1.5, 100)
    re, im = list(rng.standard_normal((2, 100))), list(rng.standard_normal((2, 100)))
    alpha, s = ebr.mode_scale(ws, re, im, "reference")
    assert alpha == pytest.approx(np.sqrt(sum(np.sum(ws * c * c) for c in re + im)), rel=1e-14)
    assert s == alpha                                       # nopcmult multiplies (postproc.f90:707-708)
    assert ebr.mode_scale(ws, re, im, "unit")[1] == 1.0 / alpha
    assert ebr.mode_scale(ws, re, im, None)[1] == 1.0


# ---- ABI wiring -----------------------------------------------------------------------------------

def test_entries_are_declared_typed_and_built():
    import __graft_entry__ as ge
    from nekstab_next_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "nekkrylov.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("nkv_pke_production", "nkv_divm1", "nkv_pke_dissipation"):
        assert name in _lib.EXPORTED
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert hasattr(_lib.load(), name)
    assert len(_lib._SIGNATURES["nkv_pke_production"][1]) == 18
    assert len(_lib._SIGNATURES["nkv_divm1"][1]) == 13
    assert len(_lib._SIGNATURES["nkv_pke_dissipation"][1]) == 13
    # the reference lines each entry replaces are cited, as for every other entry
    for cite in ("postproc.f90:649-872", "postproc.f90:801-836", "postproc.f90:853-872", "postproc.f90:784-796"):
        assert cite in hdr, cite
    src = os.path.join(ROOT, "nekstab_next_amd", "csrc", "postproc.hip")
    assert src in ge.HIP_SRCS
    body = open(src).read()
    assert "postproc.f90:649-872" in body and "#pragma clang fp contract(off)" in body
    assert re.search(r"#define NKV_ABI_VERSION 3\b", hdr)


def test_package_exports_the_module():
    import nekstab_next_amd as pkg
    from nekstab_next_amd import postproc

    assert pkg.postproc is postproc
    assert callable(postproc.stability_energy_budget) and callable(postproc.energy_budget_fields)


# ---- the PKE_ text records ---------------------------------------------------------------------

def test_pke_records_known_values():
    from nekstab_next_amd.newton import fortran_e
    from nekstab_next_amd.postproc import pke_records

    vals = [1.0, -1.2345678e-5, 0.0, 0.25, -3.0e3, 7.5e-9, 2.0, -0.5, 1.0e-12, 4.0]
    lines, total, balance = pke_records(vals)
    assert len(lines) == 12 and all(len(ln) == 15 for ln in lines)
    assert lines[0] == "  0.1000000E+01" and lines[1] == " -0.1234568E-04" and lines[2] == "  0.0000000E+00"
    assert lines[4] == " -0.3000000E+04" and lines[9] == "  0.4000000E+01"
    want_total = 0.0
    for v in vals[:9]:
        want_total = want_total + v
    assert total == want_total and balance == want_total - vals[9]
    assert lines[10] == fortran_e(want_total, 15, 7) == " -0.2997250E+04"
    assert lines[11] == fortran_e(want_total - 4.0, 15, 7) == " -0.3001250E+04"
    assert lines == ebr.pke_lines(vals)
    with pytest.raises(ValueError):
        pke_records(vals[:9])
