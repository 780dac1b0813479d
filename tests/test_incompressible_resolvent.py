"""The incompressible time-stepper resolvent (nekstab_next_amd/resolvent.py: IncompressibleResolventOperator; the
two-system pressure entries of csrc/pressure.hip), CPU side: the NumPy restatement the device is tested against
(tests/incompressible_resolvent_reference.py) pinned by the dense answer on range(P Pi), and the ABI surface of the
three new entries.

(a) the fixed point of the stepped solve, every projection by CG at 1e-13, is the dense
    Q (i omega - Q^T M J Q)^-1 Q^T M Pi f, direct and adjoint, and the adjoint run is the adjoint of the direct one in
    the pair bm1 product, for unprojected vectors; the answer lies in range(P Pi);
(b) the cases stay inside RK4's region;
(c) the gains are not those of the unprojected CoupledResolventOperator: a projection silently skipped shows;
(d) header, ctypes table and export.

Gates of (a): the figure the test itself measures in f64 is printed; its worst value is recorded in
incompressible_resolvent_reference.py and the test holds every run to 8 times that record, the margin ``_gate`` of
tests/test_gpu_advdiff.py gives a rounding error.  (a) is the long one: an inner solve is about a hundred GMRES
iterations of nsteps steps of four stages of two CG solves."""
import os
import re

import numpy as np
import pytest

import coupled_resolvent_reference as cr
import incompressible_resolvent_reference as irr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["case2d", "box3d"]

_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = irr.CASES[name]()
    return _CASES[name]


def _random_complex(nf, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))


@pytest.mark.parametrize("name", NAMES)
def test_fixed_point_is_the_dense_answer(name):
    """Direct and adjoint at both frequencies of the case, CG and inner solve at 1e-13, random unprojected forcings:
    the distance from the dense answer, the adjoint defect of the same pairs, and Z D y at the level of the CG
    tolerance: the answer lies in range(P Pi)."""
    co, mask, ns, B, dt, nsteps = _case(name)
    f, g = _random_complex(ns.nf, ns.ref.n, 4), _random_complex(ns.nf, ns.ref.n, 5)
    worst_d = worst_a = 0.0
    for omega in irr.OMEGAS[name]:
        R = irr.IncompressibleResolvent(ns, B, dt, nsteps, omega)
        y, it = R.solve(R.forced_run(R.project(f)), tol=1e-13, kdim=400)
        ya, ita = R.solve(R.forced_run(R.project(g), True), True, tol=1e-13, kdim=400)
        want, wanta = R.dense_apply(f), R.dense_apply(g, adjoint=True)
        d = float(np.max(np.abs(y - want)) / np.max(np.abs(want)))
        da = float(np.max(np.abs(ya - wanta)) / np.max(np.abs(wanta)))
        lhs, rhs = R.dot(y, g), R.dot(f, ya)
        scale = float(np.sum(ns.ref.bm1 * (np.abs(y.real * g.real) + np.abs(y.imag * g.imag))))
        defect = abs(float(lhs - rhs)) / scale
        pif = ns.ref.project(f.real) + 1j * ns.ref.project(f.imag)
        unprojected = float(np.max(np.abs(R.divergence(pif))) * np.max(np.abs(y)) / np.max(np.abs(pif)))
        div = float(np.max(np.abs(R.divergence(y)))) / unprojected   # against a field of y's size that is not projected
        print(f"{name} omega {omega}: GMRES {it}/{ita}, distance {d:.2e} / {da:.2e}, adjoint defect {defect:.2e}, "
              f"|Z D y| / |Z D of an unprojected field| {div:.2e}")
        worst_d, worst_a = max(worst_d, d, da), max(worst_a, defect)
        assert np.max(np.abs(want)) > 0 and scale > 0
        assert np.all(y[:, ns.ref.mask == 0] == 0) and np.any(ns.ref.mask == 0)
        # every stage ends in a projection solved to 1e-13 of its own right-hand side, and the error of the multiplier
        # is at most cond(E~) times that: below 1e3 on both cases (incompressible_reference.EIG_3D: 41.1 / 0.0945)
        assert div <= 1e3 * irr.CG_TOL
    print(f"{name}: worst distance {worst_d:.2e}, worst adjoint defect {worst_a:.2e}")
    assert worst_d <= 8 * irr.DENSE_DISTANCE, worst_d
    assert worst_a <= 8 * irr.ADJOINT_DEFECT, worst_a


@pytest.mark.parametrize("name", NAMES)
def test_cases_are_inside_rk4(name):
    """dt (lambda - i omega) lies inside RK4's region for every eigenvalue lambda of the dense P L_B on range(P Pi)
    and both frequencies: |dt (lambda - i omega)| below the edge, as tests/test_coupled_resolvent.py asks, and
    |p(z)| < 1 for every decaying mode.  The 2-D steady state is unstable (incompressible_reference.LEAD): its few
    growing modes grow in the stepper as they must, and what the solve needs of them is that I - Phi is regular."""
    co, mask, ns, B, dt, nsteps = _case(name)
    R = irr.IncompressibleResolvent(ns, B, dt, nsteps, 0.0)
    ev = R.spectrum()
    assert ev.size == R.reduced()[0].shape[1] < ns.nf * ns.ref.free.size
    for omega in irr.OMEGAS[name]:
        z = dt * (ev - 1j * omega)
        print(f"{name} omega {omega}: max Re lambda {ev.real.max():.4f}, max |dt (lambda - i omega)| {np.abs(z).max():.3f}")
        assert np.abs(z).max() < irr.RK4_EDGE
        p = 1 + z * (1 + z / 2 * (1 + z / 3 * (1 + z / 4)))
        assert np.all(np.abs(p[z.real < 0]) < 1.0)                  # every decaying mode decays in the stepper
        assert np.min(np.abs(p ** nsteps - 1.0)) > 1e-3              # I - Phi is regular


@pytest.mark.parametrize("name", NAMES)
def test_gains_differ_from_the_unprojected_operator(name):
    """The dense gains on range(P Pi) against those of CoupledResolventOperator's dense operator on the same case:
    they differ by far more than the gate, so a projection that is silently skipped fails the device tests.  The
    restatement (dense projection: the CG form is (a)'s), away from the eigenfrequency, maps the leading right singular
    vector onto sigma times a unit vector, to the project's 1e-10."""
    co, mask, ns, B, dt, nsteps = _case(name)
    for omega in irr.OMEGAS[name]:
        R = irr.IncompressibleResolvent(ns, B, dt, nsteps, omega, cg=False)
        own, plain = R.gains(), irr.unprojected_gains(ns, B, dt, nsteps, omega)
        print(f"{name} omega {omega}: projected {own[:3]}, unprojected {plain[:3]}")
        assert abs(own[0] - plain[0]) > 0.1 * own[0]
    omega = irr.OMEGAS[name][1]
    R = irr.IncompressibleResolvent(ns, B, dt, nsteps, omega, cg=False)
    Q, A = R.reduced()
    _, s, Vh = np.linalg.svd(np.linalg.inv(1j * omega * np.eye(A.shape[0]) - A))
    v = ns.expand(Q @ Vh[0].conj())
    y, _ = R.solve(R.forced_run(R.project(v)), tol=1e-13, kdim=400)
    gain = float(R.dot(y, y)) / float(R.dot(v, v))
    print(f"{name} omega {omega}: gain of the leading singular vector {gain:.10g}, sigma^2 {s[0] ** 2:.10g}")
    assert abs(gain - s[0] ** 2) <= 1e-10 * s[0] ** 2


def test_header_and_bindings():
    from nekstab_next_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "nekkrylov.h")).read()
    lib = _lib.load()
    kinds = {"const nkv_layout*": _lib._L, "int": _lib.c_int, "int64_t": _lib.c_int64, "const double*": _lib._P,
             "double*": _lib._P, "void*": _lib._P, "double": _lib.c_double}
    head = ["L", "lx1", "ldim", "D", "interp", "gw", "xm", "ym", "zm"]
    names = {
        "nkv_pressure_div2": head + ["u0", "u1", "u_stride", "mult", "out0", "out1", "pv0", "pv1", "partials", "active", "stream"],
        "nkv_pressure_gradt2": head + ["p0", "p1", "res0", "res1", "rr_new", "rr_old", "B", "first", "t0", "t1", "t_stride",
                                       "active", "stream"],
        "nkv_pressure_cg_update2": ["n", "x0", "x1", "r0", "r1", "p0", "p1", "Ep0", "Ep1", "red", "Br", "rr_old", "Bo", "inv_n",
                                    "closed", "init", "rr_out", "active", "stream"],
    }
    for name, args in names.items():
        assert re.search(r"\bint %s\(" % name, hdr)
        assert name in _lib.EXPORTED and hasattr(lib, name)
        decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert [p.rsplit(" ", 1)[1] for p in params] == args
        # the declaration matches the signature table, argument by argument
        assert [kinds[p.rsplit(" ", 1)[0]] for p in params] == _lib._SIGNATURES[name][1]
    # each is its single-system entry with the per-system operands doubled and ``active`` before the stream
    one, two = _lib._SIGNATURES["nkv_pressure_div"][1], _lib._SIGNATURES["nkv_pressure_div2"][1]
    assert len(two) == len(one) + 4 and two[-2] == _lib.c_int
    one, two = _lib._SIGNATURES["nkv_pressure_gradt"][1], _lib._SIGNATURES["nkv_pressure_gradt2"][1]
    assert len(two) == len(one) + 4 and two[-2] == _lib.c_int
    one, two = _lib._SIGNATURES["nkv_pressure_cg_update"][1], _lib._SIGNATURES["nkv_pressure_cg_update2"][1]
    assert len(two) == len(one) + 5 and two[-2] == _lib.c_int
    assert lib.nkv_abi_version() == _lib.NKV_ABI_VERSION == 3
    import nekstab_next_amd

    op = nekstab_next_amd.IncompressibleResolventOperator
    assert op is nekstab_next_amd.resolvent.IncompressibleResolventOperator
    assert issubclass(op, nekstab_next_amd.CoupledResolventOperator)
    assert op.projects_stages and not nekstab_next_amd.CoupledResolventOperator.projects_stages
    assert cr.RK4_EDGE == irr.RK4_EDGE
