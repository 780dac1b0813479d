"""SFD / TDF (core/fixedp.f90:2-216) on the CPU: the coefficient formulas, the op-for-op restatement
(tests/fixedp_reference.py) stabilising an unstable oscillator, the host logic of
nekstab_next_amd.fixedp and the ABI wiring.  The device kernels are compared with the restatement
in tests/test_gpu_fixedp.py."""
import math
import os
import re

import numpy as np
import pytest

import fixedp_reference as fr
from nekstab_next_amd import fixedp
from nekstab_next_amd import synthetic as syn
from nekstab_next_amd.layout import NekLayout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST, SIG, DT, TOL = 1.0 / (2.0 * math.pi), 0.25, 0.1, 1e-10


# ---- coefficients -----------------------------------------------------------------------------

def test_sfd_coefficients_both_branches():
    frq, sig = 0.37 * 2 * math.pi, 0.21
    cut, gain = fixedp.sfd_coefficients(0.37, 0.21)            # Akervik
    assert cut == pytest.approx(0.5 * frq, rel=1e-15) and gain == pytest.approx(-2 * sig, rel=1e-15)
    cut, gain = fixedp.sfd_coefficients(-0.37, 0.21)           # Casacuberta
    root = math.sqrt(frq ** 2 + sig ** 2)
    assert cut == pytest.approx(0.5 * (root - sig), rel=1e-15)
    assert gain == pytest.approx(-0.5 * (root + sig), rel=1e-15)
    # uparam(4) = 0 is not > 0: the Casacuberta formulas with frq = 0
    assert fixedp.sfd_coefficients(0.0, 0.3) == (0.0, pytest.approx(-0.3))
    # abs() of both parameters (:134-135)
    assert fixedp.sfd_coefficients(0.37, -0.21) == fixedp.sfd_coefficients(0.37, 0.21)


def test_ab3_coefficients():
    assert fixedp.ab3_coefficients(1) == (1.0, 0.0, 0.0)
    assert fixedp.ab3_coefficients(2) == (1.5, -0.5, 0.0)
    for k in (3, 4, 1000):
        a, b, c = fixedp.ab3_coefficients(k)
        assert (a, b, c) == (23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0)
    for k in (1, 2, 3):
        assert sum(fixedp.ab3_coefficients(k)) == pytest.approx(1.0, abs=1e-15)   # consistency
    with pytest.raises(ValueError):
        fixedp.ab3_coefficients(0)


def test_tdf_parameters():
    norbit, dt, gain = fixedp.tdf_parameters(period=5.0, dt_target=0.3)
    assert norbit == 17 and dt == 5.0 / 17 and norbit * dt == pytest.approx(5.0, rel=1e-15)
    assert gain == pytest.approx(-0.04432 * 2 * math.pi / 5.0, rel=1e-15)
    assert fixedp.tdf_parameters(1.0, 0.25)[0] == 4              # an exact multiple is not rounded up
    with pytest.raises(ValueError):
        fixedp.tdf_parameters(0.0, 0.1)


# ---- the restatement stabilises an unstable oscillator -------------------------------------------

def _oscillator():
    lay = NekLayout(2, 4, 2, 6)
    w = syn.mass_weights(lay)
    b = syn.hash_vector(lay, 41)[:lay.rows].copy()
    v0 = syn.hash_vector(lay, 42)[:lay.rows].copy()
    b[2 * lay.sv:] = 0.0
    v0[2 * lay.sv:] = 0.0
    ustar = -(b[:lay.sv] + 1j * b[lay.sv:2 * lay.sv]) / fr.LAMBDA
    return lay, w, b, v0, ustar


def _err(lay, v, ustar):
    return float(np.max(np.abs(v[:lay.sv] + 1j * v[lay.sv:2 * lay.sv] - ustar)))


@pytest.mark.parametrize("uparam4", [ST, -ST], ids=["akervik", "casacuberta"])
def test_restatement_stabilises_the_oscillator(uparam4):
    """u' = (0.1 + i) u + b + f per point with f the SFD forcing: the coupled system is stable (real
    parts <= -0.26), so the residual falls below 1e-10 and the flow reaches u* = -b / lambda."""
    lay, w, b, v0, ustar = _oscillator()
    k, v, hist = fr.run_oscillator(lay, w, b, v0, uparam4, SIG, DT, TOL, 1500)
    assert k is not None and 100 < k < 1000, k
    assert hist[-1] < TOL
    # the decay rate of the residual over the last 100 steps: slower than no coupled eigenvalue allows
    assert math.log(hist[-1] / hist[-101]) / (100 * DT) < -0.25
    # 100 more steps of the converged iteration: within 1e-9 of the fixed point
    k2, v2, hist2 = fr.run_oscillator(lay, w, b, v0, uparam4, SIG, DT, 0.0, k + 100)
    assert k2 is None and hist2[-1] < TOL and _err(lay, v2, ustar) < 1e-9


def test_unforced_oscillator_diverges():
    lay, w, b, v0, ustar = _oscillator()
    _, v, _ = fr.run_oscillator(lay, w, b, v0, ST, SIG, DT, TOL, 1500, forced=False)
    assert _err(lay, v, ustar) > 1e5


def test_restatement_rotation_is_the_reference_copies():
    """qc <- qb <- qa by copies: after three steps the three histories are the three last d's."""
    lay, w, b, v0, _ = _oscillator()
    sfd = fr.SFDReference(lay, w, 0.5, -0.5, DT, float(np.sum(w)))
    sfd.start(v0)
    ds = []
    fc = np.zeros(lay.rows)
    for istep in (1, 2, 3):
        v = syn.hash_vector(lay, 50 + istep)[:lay.rows]
        ds.append(sfd.oldV - sfd.oldQ)
        sfd.step(v, fc, fixedp.ab3_coefficients(istep))
    np.testing.assert_array_equal(sfd.qa, ds[2])
    np.testing.assert_array_equal(sfd.qb, ds[1])
    np.testing.assert_array_equal(sfd.qc, ds[0])


def test_tdf_restatement_is_zero_on_a_periodic_flow():
    lay = NekLayout(2, 4, 2, 6)
    w = syn.mass_weights(lay)
    norbit = 5
    tdf = fr.TDFReference(lay, w, norbit, -0.3, float(np.sum(w)))
    fc = np.zeros(lay.rows)
    orbit = [syn.hash_vector(lay, 60 + i)[:lay.rows] for i in range(norbit)]
    for istep in range(1, 14):
        l2, rate = tdf.step(orbit[(istep - 1) % norbit], fc)
        assert l2 == 0.0 and rate == 0.0
    assert not fc.any()


# ---- host logic -----------------------------------------------------------------------------------

def test_convergence_rules():
    assert not fixedp.sfd_converged(100, 1e-12, 1e-10)           # istep > 100, not >=
    assert fixedp.sfd_converged(101, 1e-12, 1e-10)
    assert not fixedp.sfd_converged(101, 1e-10, 1e-10)           # res < tol, strictly
    assert fixedp.sfd_converged(6, 1e-12, 1e-10, min_steps=5)
    assert not fixedp.sfd_converged(5, 1e-12, 1e-10, min_steps=5)
    assert fixedp.tdf_converged(1e-12, 1e-10)
    assert not fixedp.tdf_converged(0.0, 1e-10)                  # l2 > 0 (:105)
    assert not fixedp.tdf_converged(1e-10, 1e-10)


def test_monitor_mode_switch():
    assert fixedp.sfd_is_monitor(0.0) and fixedp.sfd_is_monitor(-0.2)
    assert not fixedp.sfd_is_monitor(0.2)


def test_ring_slot_index():
    norbit = 5
    assert [fixedp.tdf_slot(i, norbit) for i in range(1, 13)] == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1]
    # the slot of step istep > norbit holds step istep - norbit: the reference's uor(:, 1)
    hist, ring = [None] * norbit, [None] * norbit
    for istep in range(1, 20):
        s = fixedp.tdf_slot(istep, norbit)
        if istep <= norbit:
            hist[istep - 1] = istep
        else:
            assert ring[s] == hist[0] == istep - norbit
            hist = hist[1:] + [istep]
        ring[s] = istep
    with pytest.raises(ValueError):
        fixedp.tdf_slot(0, norbit)


def test_residu_line_formats():
    """(4E15.7) for SFD (:191), (3E15.7) for TDF (:99): Fortran's 0.ddddddd normalisation."""
    assert fixedp.fortran_e(1.0) == "  0.1000000E+01"
    assert fixedp.fortran_e(-1.2345678e-5) == " -0.1234568E-04"
    assert fixedp.fortran_e(0.0) == "  0.0000000E+00"
    assert fixedp.fortran_e(9.99999999) == "  0.1000000E+02"      # rounding carries into the exponent
    assert fixedp.fortran_e(1e-100) == "  0.1000000E-99"
    assert fixedp.fortran_e(1e-101) == "  0.1000000-100"          # three-digit exponent: no letter
    line = fixedp.residu_line(0.5, 1.25e-3, -2.5e-2, 1e-10)
    assert line == "  0.5000000E+00  0.1250000E-02 -0.2500000E-01  0.1000000E-09" and len(line) == 60
    line = fixedp.residu_line(12.0, 3e-7, 0.0)
    assert line == "  0.1200000E+02  0.3000000E-06  0.0000000E+00" and len(line) == 45
    for x in (3.14159e17, -2.5e-33, 7e-9):
        assert float(fixedp.fortran_e(x)) == pytest.approx(x, rel=1e-6)


# ---- ABI wiring -----------------------------------------------------------------------------------

def test_entries_are_declared_and_typed():
    from nekstab_next_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "nekkrylov.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("nkv_sfd_step", "nkv_tdf_step"):
        assert name in _lib.EXPORTED
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert hasattr(_lib.load(), name)
    defs = {k: int(v, 0) for k, v in re.findall(r"#define (NKV_[A-Z0-9_]+)\s+(0x[0-9a-f]+)u", hdr)}
    assert defs["NKV_SFD_MONITOR"] == _lib.NKV_SFD_MONITOR and defs["NKV_TDF_STORE"] == _lib.NKV_TDF_STORE
    flags = [v for k, v in defs.items() if k not in ("NKV_ACCUMULATE",)]
    assert len(set(flags)) == len(flags)                          # no flag bit is shared
    # the reference lines each entry replaces are cited, as for every other entry
    assert "fixedp.f90:157-189" in hdr and "fixedp.f90:71-96" in hdr
    assert "fixedp.f90:124-216" in open(os.path.join(ROOT, "nekstab_next_amd", "csrc", "fixedp.hip")).read()


def test_package_exports_the_classes():
    import nekstab_next_amd as pkg

    assert pkg.SFD is fixedp.SFD and pkg.TDF is fixedp.TDF and pkg.fixedp is fixedp
