"""The time-stepper resolvent (nekstab_next_amd/resolvent.py, nkv_advdiff_cstage), CPU side: the NumPy
restatement the device is tested against (tests/resolvent_reference.py) pinned by the dense inverse, and the
ABI surface of the new entry.

(a) the fixed point of the stepped solve is the dense (i omega - L)^-1 Pi f for any dt and nsteps: no time error;
(b) the adjoint run is the adjoint of the direct one in the pair bm1 product, for unprojected vectors;
(c) the operator's gains are those of the dense weighted SVD, each twice in the pair space;
(d) header, ctypes table and export.

Gates of (a) and (b): the figure the test itself measures in f64 is printed; its worst value over the runs
below is recorded in resolvent_reference.py (and DESIGN §9 item 13) and the test holds every run to 8 times
that record, the margin ``_gate`` of tests/test_gpu_advdiff.py gives a rounding error."""
import os
import re

import numpy as np
import pytest

import advdiff_reference as ar
import resolvent_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAPPA = rr.CASES["cell"]["kappa"]


@pytest.fixture(scope="module")
def ref():
    co, U, mask = rr.cell_mesh(6)
    return ar.Reference(6, 2, co, U, mask=mask)


def _random_complex(ref, seed, nf=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nf, ref.n)) + 1j * rng.standard_normal((nf, ref.n))


@pytest.mark.parametrize("omega", [0.0, 1.0])
def test_fixed_point_is_the_dense_inverse(ref, omega):
    """Direct and adjoint, dt in {0.06, 0.04} x nsteps in {16, 32}, inner solve at 1e-13: the distance from the
    dense solve does not depend on the stepping (dt^4 would be 1e-5).  The same pairs give the adjoint defect."""
    f, g = _random_complex(ref, 4), _random_complex(ref, 5)
    worst_d = worst_a = 0.0
    for dt in (0.06, 0.04):
        for nsteps in (16, 32):
            R = rr.Resolvent(ref, KAPPA, dt, nsteps, omega)
            y, it = R.apply(f)
            ya, ita = R.apply(g, adjoint=True)
            want, wanta = R.dense_apply(f), R.dense_apply(g, adjoint=True)
            d = float(np.max(np.abs(y - want)) / np.max(np.abs(want)))
            da = float(np.max(np.abs(ya - wanta)) / np.max(np.abs(wanta)))
            lhs, rhs = R.dot(y, g), R.dot(f, ya)
            scale = float(np.sum(ref.bm1 * (np.abs(y.real * g.real) + np.abs(y.imag * g.imag))))
            defect = abs(float(lhs - rhs)) / scale
            print(f"omega {omega} dt {dt} nsteps {nsteps}: GMRES {it}/{ita}, distance {d:.2e} / {da:.2e}, "
                  f"adjoint defect {defect:.2e}")
            worst_d, worst_a = max(worst_d, d, da), max(worst_a, defect)
            assert np.max(np.abs(want)) > 0 and scale > 0
    assert worst_d <= 8 * rr.DENSE_DISTANCE, worst_d
    assert worst_a <= 8 * rr.ADJOINT_DEFECT, worst_a


def test_forcing_is_projected_and_the_response_continuous(ref):
    """R f = R Pi f; the response is continuous, vanishes on the walls and solves (i omega - L) y = Pi f."""
    c = rr.CASES["cell"]
    R = rr.Resolvent(ref, KAPPA, c["dt"], c["nsteps"], 1.0)
    f = _random_complex(ref, 6)
    y, _ = R.apply(f)
    y2, _ = R.apply(R.project(f))
    scale = np.max(np.abs(y))
    assert np.max(np.abs(y - y2)) <= 1e-12 * scale
    assert np.all(y[:, ref.mask == 0] == 0) and np.any(ref.mask == 0)
    back = 1j * 1.0 * y - R.L(y)
    pf = R.project(f)
    # |L| <= 32.5 and |y| <= 12.5 |Pi f| (sqrt of the leading gain): an error of 1e-13 |y| in y is 4e-11 |Pi f| here
    assert np.max(np.abs(back - pf)) <= 1e-10 * np.max(np.abs(pf))


@pytest.mark.parametrize("omega,pinned", [(1.0, (3.197, 1.077)), (0.0, (62.19,))])
def test_gains_are_those_of_the_dense_weighted_svd(ref, omega, pinned):
    """kappa = 0.05 on both fields: the dense gains are the pinned ones; the stepped operator maps the leading
    right singular vectors onto sigma times unit vectors; and in the pair space (real dimension doubled) every
    gain appears twice."""
    c = rr.CASES["cell"]
    R = rr.Resolvent(ref, (0.05, 0.05), c["dt"], c["nsteps"], omega)
    gains = R.gains(0)
    print(f"omega {omega}: leading gains {gains[:3]}")
    for got, want in zip(gains, pinned):
        assert abs(got - want) <= 5e-4 * want, (got, want)
    sB = np.sqrt(ref.mass())
    S = sB[:, None] * R.dense_inverse(0) / sB[None, :]
    _, s, Vh = np.linalg.svd(S)
    for j in range(len(pinned)):
        v = ref.expand(Vh[j].conj() / sB)                       # unit in the bm1 product, continuous
        x = np.stack([v, 1j * v])                                # field 1 carries i v: the other copy
        y, _ = R.apply(x)
        for k in range(2):
            gain = float(R.dot(y[k:k + 1], y[k:k + 1])) / float(R.dot(x[k:k + 1], x[k:k + 1]))
            assert abs(gain - gains[j]) <= 1e-11 * gains[j], (j, k, gain, gains[j])
        assert abs(float(R.dot(y[0:1], y[1:2]))) <= 1e-11 * gains[j]   # R v and R (i v) are orthogonal
    pair = np.block([[S.real, -S.imag], [S.imag, S.real]])
    sp = np.linalg.svd(pair, compute_uv=False)
    assert np.max(np.abs(sp[0::2] - s)) <= 1e-12 * s[0] and np.max(np.abs(sp[1::2] - s)) <= 1e-12 * s[0]


def test_header_and_bindings():
    from nekstab_next_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "nekkrylov.h")).read()
    lib = _lib.load()
    name, nargs = "nkv_advdiff_cstage", 22
    assert re.search(r"\bint %s\(" % name, hdr) and "linear_operators.f90:348-431" in hdr
    assert name in _lib.EXPORTED and hasattr(lib, name)
    assert len(_lib._SIGNATURES[name][1]) == nargs
    decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
    assert decl.count(",") + 1 == nargs
    assert lib.nkv_abi_version() == _lib.NKV_ABI_VERSION == 3
    import nekstab_next_amd

    assert nekstab_next_amd.ResolventOperator is nekstab_next_amd.resolvent.ResolventOperator
    assert nekstab_next_amd.pair_context is nekstab_next_amd.resolvent.pair_context
