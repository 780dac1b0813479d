"""The coupled time-stepper resolvent (nekstab_next_amd/resolvent.py: CoupledResolventOperator, nkv_linconv_crhs),
CPU side: the NumPy restatement the device is tested against (tests/coupled_resolvent_reference.py) pinned by the
dense inverse of the linearised convection, and the ABI surface of the new entry.

(a) the fixed point of the stepped solve is the dense (i omega - J)^-1 Pi f, J = Burgers.dense(B), direct and adjoint;
(b) the adjoint run is the adjoint of the direct one in the pair bm1 product, for unprojected vectors;
(c) the gains are those of the dense weighted SVD, and they are not the uncoupled operator's: the production term
    is in;
(d) the cases stay stable and inside RK4's region;
(e) k_dim of the analysis test and the restatement's own bidiagonalisation;
(f) header, ctypes table and export.

Gates of (a), (b) and (e): the figure the test itself measures in f64 is printed; its worst value is recorded in
coupled_resolvent_reference.py and the test holds every run to 8 times that record, the margin ``_gate`` of
tests/test_gpu_advdiff.py gives a rounding error."""
import os
import re

import numpy as np
import pytest

import advdiff_reference as ar
import burgers_reference as br
import coupled_resolvent_reference as cr
import resolvent_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = cr.cell_case(name)
    return _CASES[name]


def _random_complex(n, seed, nf=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))


@pytest.mark.parametrize("name", ["cell", "odd"])
def test_fixed_point_is_the_dense_inverse(name):
    """Direct and adjoint at omega in {0, 1}, inner solve at 1e-13, random unprojected forcings: the distance from
    the one dense solve on all fields, and the adjoint defect of the same pairs."""
    bg, B, dt, nsteps = _case(name)
    f, g = _random_complex(bg.ref.n, 4), _random_complex(bg.ref.n, 5)
    worst_d = worst_a = 0.0
    for omega in (0.0, 1.0):
        R = cr.CoupledResolvent(bg, B, dt, nsteps, omega)
        y, it = R.apply(f)
        ya, ita = R.apply(g, adjoint=True)
        want, wanta = R.dense_apply(f), R.dense_apply(g, adjoint=True)
        d = float(np.max(np.abs(y - want)) / np.max(np.abs(want)))
        da = float(np.max(np.abs(ya - wanta)) / np.max(np.abs(wanta)))
        lhs, rhs = R.dot(y, g), R.dot(f, ya)
        scale = float(np.sum(bg.ref.bm1 * (np.abs(y.real * g.real) + np.abs(y.imag * g.imag))))
        defect = abs(float(lhs - rhs)) / scale
        print(f"{name} omega {omega}: GMRES {it}/{ita}, distance {d:.2e} / {da:.2e}, adjoint defect {defect:.2e}")
        worst_d, worst_a = max(worst_d, d, da), max(worst_a, defect)
        assert np.max(np.abs(want)) > 0 and scale > 0
        assert np.all(y[:, bg.ref.mask == 0] == 0) and np.any(bg.ref.mask == 0)
    assert worst_d <= 8 * cr.DENSE_DISTANCE, worst_d
    assert worst_a <= 8 * cr.ADJOINT_DEFECT, worst_a


@pytest.mark.parametrize("name", ["cell", "odd"])
def test_gains_differ_from_the_uncoupled_operator(name):
    """The dense gains are the recorded ones, coupled and uncoupled: sigma_1^2 = 54.01 against 4.419 on "cell"
    at omega = 1.  The stepped operator maps the leading right singular vector onto sigma times a unit vector:
    the restatement has the production term, and with B = 0 it has the uncoupled gains."""
    bg, B, dt, nsteps = _case(name)
    c = rr.CASES[name]
    co, U, mask = rr.cell_mesh(c["lx1"])
    plain = ar.Reference(c["lx1"], 2, co, U, mask=mask)
    for omega in (1.0, 0.0):
        R = cr.CoupledResolvent(bg, B, dt, nsteps, omega)
        coupled, uncoupled = R.gains(), rr.Resolvent(plain, c["kappa"], dt, nsteps, omega).gains()
        want_c, want_u = cr.LEADING_GAINS[(name, omega)]
        print(f"{name} omega {omega}: coupled {coupled[:4]}, uncoupled {uncoupled[:2]}")
        assert abs(coupled[0] - want_c) <= 5e-4 * want_c and abs(uncoupled[0] - want_u) <= 5e-4 * want_u
        assert coupled[0] > 2 * uncoupled[0]
    R = cr.CoupledResolvent(bg, B, dt, nsteps, 1.0)
    sB = np.sqrt(bg.mass())
    _, s, Vh = np.linalg.svd(R.weighted())
    v = bg.expand(Vh[0].conj() / sB)                                 # unit in the bm1 product, continuous
    y, _ = R.apply(v)
    gain = float(R.dot(y, y)) / float(R.dot(v, v))
    assert abs(gain - s[0] ** 2) <= 1e-11 * s[0] ** 2, (gain, s[0] ** 2)
    # the advecting velocity alone (no production term): the uncoupled operator of the same mesh
    J0 = np.zeros_like(bg.dense(B))
    m = bg.ref.free.size
    for k in range(2):
        J0[k * m:(k + 1) * m, k * m:(k + 1) * m] = plain.dense(c["kappa"][k])
    assert np.max(np.abs(bg.dense(B) - J0)) > 1e-2 * np.max(np.abs(J0))
    pair = np.block([[R.weighted().real, -R.weighted().imag], [R.weighted().imag, R.weighted().real]])
    sp = np.linalg.svd(pair, compute_uv=False)
    assert np.max(np.abs(sp[0::2] - s)) <= 1e-12 * s[0] and np.max(np.abs(sp[1::2] - s)) <= 1e-12 * s[0]


def _box3d():
    import test_gpu_burgers as gb                                    # its _case builds the 3-D base state

    lay, co, B, mask, _ = gb._case(cr.BOX3D)
    p = cr.BOX3D_PARAMS
    zero = [np.zeros(lay.n_v)] * 3
    return br.Burgers(ar.Reference(lay.lx1, 3, co, zero, mask=mask), p["kappa"], p["dt"], p["nsteps"]), np.stack(B), p["dt"]


@pytest.mark.parametrize("name", ["cell", "odd", "box3d"])
def test_cases_are_stable_and_inside_rk4(name):
    """max Re lambda(J) < 0 and dt (rho(J) + 1) < 2.78 with the recorded values, so that a changed case cannot
    drift out of RK4's region unnoticed; M J = (M J†)^T to burgers_reference.DENSE_TRANSPOSE."""
    bg, B, dt = _box3d() if name == "box3d" else _case(name)[:3]
    J = bg.dense(B)
    ev = np.linalg.eigvals(J)
    growth, rho = float(ev.real.max()), float(np.abs(ev).max())
    print(f"{name}: max Re lambda {growth:.4f}, rho {rho:.3f}, dt rho {dt * rho:.3f}")
    want_growth, want_rho = cr.MARGINS[name]
    assert abs(growth - want_growth) <= 2e-3 * abs(want_growth) + 5e-4 and abs(rho - want_rho) <= 2e-3 * want_rho
    assert growth < 0 and dt * (rho + 1.0) < cr.RK4_EDGE
    MJ = bg.mass()[:, None] * J
    MJa = bg.mass()[:, None] * bg.dense(B, adjoint=True)
    defect = float(np.max(np.abs(MJ - MJa.T)) / np.max(np.abs(MJ)))
    print(f"{name}: transpose defect {defect:.2e}")
    assert defect <= 8 * br.DENSE_TRANSPOSE


def test_analysis_kdim_and_the_restatements_bidiagonalisation():
    """"odd" at omega = 1.  k_dim: a bidiagonalisation of the dense pair operator with 1e-13 relative noise in
    every product has the four leading values within 1e-12 of the dense SVD at ANALYSIS_KDIM for every one of 40
    seeds, and not at ANALYSIS_KDIM - 2 (one below is the edge: its worst seed lands on either side of 1e-12 with
    the noise drawn).  Then the restatement's own bidiagonalisation (inner tolerance 1e-13, the
    hashed seed of the device test) against the dense SVD: GAIN_DISTANCE, and the gate it implies."""
    from nekstab_next_amd import synthetic as syn
    from nekstab_next_amd.layout import NekLayout, pair_layout

    bg, B, dt, nsteps = _case("odd")
    R = cr.CoupledResolvent(bg, B, dt, nsteps, 1.0)
    S = R.weighted()
    pair = np.block([[S.real, -S.imag], [S.imag, S.real]])
    gains = R.gains()
    exact = np.repeat(gains[:2], 2)
    for got, want in zip(gains, (287.90, 40.33, 7.17)):
        assert abs(got - want) <= 1e-3 * want
    worst = {cr.ANALYSIS_KDIM - 2: 0.0, cr.ANALYSIS_KDIM: 0.0}
    for sd in range(40):
        rng = np.random.default_rng(100 + sd)

        def noisy(M):
            def product(v):
                y = M @ v
                return y + 1e-13 * np.linalg.norm(y) * rng.standard_normal(y.size) / np.sqrt(y.size)
            return product

        seed = np.random.default_rng(sd).standard_normal(pair.shape[0])
        for k in worst:
            g = cr.bidiagonal_gains(noisy(pair), noisy(pair.T), np.dot, seed, k)
            worst[k] = max(worst[k], float(np.max(np.abs(g[:4] - exact) / exact)))
    print(f"noisy dense bidiagonalisation, worst of 40 seeds: {worst}")
    assert worst[cr.ANALYSIS_KDIM] <= 1e-12 < worst[cr.ANALYSIS_KDIM - 2]
    lay = NekLayout(ldim=2, lx1=3, lx2=1, nelgv=9)
    p, n = pair_layout(lay), lay.n_v
    h = syn.hash_vector(p, 17)
    seed = np.stack([h[f * p.sv: f * p.sv + n] + 1j * h[f * p.sv + n: f * p.sv + 2 * n] for f in range(2)])
    g = cr.bidiagonal_gains(lambda v: R.apply(v)[0], lambda v: R.apply(v, adjoint=True)[0], R.dot, seed, cr.ANALYSIS_KDIM)
    d = float(np.max(np.abs(g[:4] - exact) / exact))
    print(f"restatement bidiagonalisation: {g[:4]} against {exact}: distance {d:.2e}")
    assert d <= 8 * cr.GAIN_DISTANCE
    assert cr.GAIN_GATE == (1e-10 if 8 * cr.GAIN_DISTANCE <= 1e-10 else 8 * cr.GAIN_DISTANCE)


def test_header_and_bindings():
    from nekstab_next_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "nekkrylov.h")).read()
    lib = _lib.load()
    name, nargs = "nkv_linconv_crhs", 20
    assert re.search(r"\bint %s\(" % name, hdr)
    assert name in _lib.EXPORTED and hasattr(lib, name)
    assert len(_lib._SIGNATURES[name][1]) == nargs
    decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    assert len(params) == nargs
    # the declaration matches the signature table, argument by argument
    kinds = {"const nkv_layout*": _lib._L, "int": _lib.c_int, "int64_t": _lib.c_int64, "const double*": _lib._P,
             "double*": _lib._P, "void*": _lib._P}
    assert [kinds[p.rsplit(" ", 1)[0]] for p in params] == _lib._SIGNATURES[name][1]
    assert [p.rsplit(" ", 1)[1] for p in params] == ["L", "lx1", "ldim", "D", "w", "xm", "ym", "zm", "B", "B_stride", "kappa",
                                                      "u_re", "u_im", "nfld", "u_stride", "r_re", "r_im", "r_stride",
                                                      "adjoint", "stream"]
    # nkv_linconv_rhs with u, r doubled: one stride per operand
    one = list(_lib._SIGNATURES["nkv_linconv_rhs"][1])
    assert _lib._SIGNATURES[name][1] == one[:12] + [_lib._P] + one[12:15] + [_lib._P] + one[15:]
    assert lib.nkv_abi_version() == _lib.NKV_ABI_VERSION == 3
    import nekstab_next_amd

    assert nekstab_next_amd.CoupledResolventOperator is nekstab_next_amd.resolvent.CoupledResolventOperator
    assert issubclass(nekstab_next_amd.CoupledResolventOperator, nekstab_next_amd.ResolventOperator)
