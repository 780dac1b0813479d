"""The sponge and the body-force assembly (core/forcing.f90:2-251) on the CPU: the section constants, the
step function, the line-for-line restatement (tests/forcing_reference.py) on the reference's back-facing-step
mesh, the reference quirks, the host logic of nekstab_next_amd.forcing and the ABI wiring.  The device kernels
are compared with the restatement in tests/test_gpu_forcing.py."""
import functools
import math
import os
import re
import warnings

import numpy as np
import pytest

import forcing_reference as fref
from helpers import reference_file
from nekstab_next_amd import fld, forcing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS = "examples/back_fstep/transient_growth/BF_bfs0.f00001"
BFS_CFG = dict(xLspg=5.0, xRspg=10.0, spng_st=2.0)        # userparam08..10 = 5, 10, 2 of the bfs cases


@functools.lru_cache(maxsize=None)
def bfs_mesh():
    f = fld.read_fld(reference_file(BFS))
    assert (f.nx, f.emap.size, f.ldim) == (6, 1670, 2)
    return {k: np.ascontiguousarray(f.fields[k]).reshape(-1).copy() for k in ("x", "y")}


def _extents(co):
    keys = [k for k in ("x", "y", "z") if k in co]
    return [float(co[k].min()) for k in keys], [float(co[k].max()) for k in keys]


# ---- section constants ------------------------------------------------------------------------------

def test_section_constants_for_the_bfs_parameters():
    cfg = forcing.SpongeConfig(**BFS_CFG)
    assert cfg.acc_spg == 0.333
    sx, sy = forcing.sponge_sections(cfg, [-10.0, -1.0], [50.0, 1.0], 2)
    for got, want in zip(sx.constants()[:4], (-8.33, -6.665, 43.33, 46.66)):
        assert got == pytest.approx(want, rel=0, abs=1e-13)
    assert sx.active and not sy.active
    # the reference's arithmetic order (:126-140, :192-195), bit for bit
    wl, wr, dl, dr = (1.0 - 0.333) * 5.0, (1.0 - 0.333) * 10.0, 0.333 * 5.0, 0.333 * 10.0
    assert (sx.wl, sx.wr, sx.dl, sx.dr) == (wl, wr, dl, dr)
    assert sx.constants() == ((-10.0 + wl) - dl, -10.0 + wl, 50.0 - wr, (50.0 - wr) + dr, wl, wr)
    # and the restatement's widths are the same numbers
    rwl, rwr, rdl, rdr = fref.spng_init(0.333, [(5.0, 10.0), (0.0, 0.0)], 2)
    assert (rwl[0], rwr[0], rdl[0], rdr[0]) == (wl, wr, dl, dr)


def test_config_defaults_and_abs():
    cfg = forcing.SpongeConfig()
    assert (cfg.xLspg, cfg.xRspg, cfg.yLspg, cfg.yRspg, cfg.zLspg, cfg.zRspg) == (0.0,) * 6     # main.f90:40-45
    assert cfg.acc_spg == 0.333 and cfg.spng_st == 0.0                                         # main.f90:46-47
    cfg = forcing.SpongeConfig(acc_spg=-0.25, spng_st=-2.0)                                    # :95-97, :124
    assert cfg.acc_spg == 0.25 and cfg.spng_st == 2.0
    assert not any(s.active for s in forcing.sponge_sections(forcing.SpongeConfig(), [0.0] * 3, [1.0] * 3, 3))


def test_too_wide_is_refused():
    cfg = forcing.SpongeConfig(xLspg=40.0, xRspg=60.0)
    with pytest.raises(ValueError, match="Sponge too wide"):
        forcing.sponge_sections(cfg, [-10.0, -1.0], [50.0, 1.0], 2)
    # the reference skips the dimension instead (:198-199): the restatement records it and returns zeros
    stats = {}
    x = np.linspace(-10.0, 50.0, 13)
    fn = fref.sponge_function([x, 0 * x], [-10.0, 0.0], [50.0, 0.0], [(40.0, 60.0), (0.0, 0.0)], stats=stats)
    assert stats["too_wide"] == [0] and not fn.any()


def test_wrong_parameters_warn_and_continue():
    cfg = forcing.SpongeConfig(xLspg=5.0, acc_spg=0.75)          # section 1.25 below the drop 3.75
    with pytest.warns(UserWarning, match="Wrong sponge parameters"):
        sx, _ = forcing.sponge_sections(cfg, [-10.0, -1.0], [50.0, 1.0], 2)
    assert sx.active and sx.wl == 1.25 and sx.dl == 3.75
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        forcing.sponge_sections(forcing.SpongeConfig(**BFS_CFG), [-10.0, -1.0], [50.0, 1.0], 2)


# ---- mth_stepf ------------------------------------------------------------------------------------------

def test_step_function():
    assert fref.mth_stepf(0.5) == 0.5                            # exp(1/(-0.5) + 1/0.5) = exp(0) = 1, exactly
    assert fref.mth_stepf(0.001) == 0.0 and fref.mth_stepf(-3.0) == 0.0 and fref.mth_stepf(0.0) == 0.0
    lo = fref.mth_stepf(np.nextafter(0.001, 1.0))
    assert lo == 0.0                                             # just above the threshold exp(~999) = Inf: still 0
    assert 0.0 < fref.mth_stepf(0.0015) < 1e-280                 # exp(665.7) is finite
    assert fref.mth_stepf(0.999) == 1.0 / (1.0 + math.exp(1.0 / (0.999 - 1.0) + 1.0 / 0.999))
    assert fref.mth_stepf(0.999) == 1.0                          # continuous to rounding at the upper threshold
    assert fref.mth_stepf(np.nextafter(0.999, 1.0)) == 1.0 and fref.mth_stepf(7.0) == 1.0
    xs = np.linspace(0.002, 0.998, 499)
    ys = np.array([fref.mth_stepf(x) for x in xs])
    assert np.all(np.diff(ys) >= 0) and np.all((ys >= 0) & (ys <= 1))
    np.testing.assert_allclose(ys + ys[::-1], 1.0, rtol=0, atol=1e-13)     # f(x) + f(1 - x) = 1


# ---- the restatement on the reference's mesh ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bfs_fn():
    co = bfs_mesh()
    bmin, bmax = _extents(co)
    stats = {}
    fn = fref.sponge_function([co["x"], co["y"]], bmin, bmax, [(5.0, 10.0), (0.0, 0.0)], stats=stats)
    return fn, stats, bmin, bmax


def test_restatement_on_the_bfs_mesh():
    co = bfs_mesh()
    fn, stats, bmin, bmax = bfs_fn()
    assert co["x"].size == 60120 and (bmin[0], bmax[0]) == (-10.0, 50.0)
    assert np.count_nonzero(fn) == 3120
    assert np.count_nonzero(fn == 1.0) == 1560
    ramp = fn[(fn > 0) & (fn < 1)]
    assert ramp.max() == pytest.approx(0.4204, abs=5e-5)
    assert ramp.min() == pytest.approx(1.07e-16, rel=5e-3)
    assert stats["max_exp_arg"] == pytest.approx(36.8, abs=0.05)
    assert "too_wide" not in stats
    # the weights: zero exactly on the sponge points
    bm1 = 1.0 + np.arange(fn.size) % 7
    bm1s = fref.activate_sponge(bm1, fn)
    assert np.count_nonzero(bm1s == 0) == 3120 and np.array_equal(bm1s[fn == 0], bm1[fn == 0])


def test_quirk_the_ramp_divides_by_the_section_width():
    """arg = (xxmin - x)/wl reaches only dl/wl = acc/(1 - acc) = 0.499 at the constant section, so fn stays
    below mth_stepf(0.499) < 0.5 on the ramp and jumps to 1 there (on the bfs mesh from 0.4204, the last GLL
    point before the constant section); dividing by the drop width would reach 1 continuously."""
    fn, _, _, _ = bfs_fn()
    top = fref.mth_stepf(0.333 / (1.0 - 0.333))
    assert top == pytest.approx(0.4985, abs=5e-5)
    ramp = fn[(fn > 0) & (fn < 1)]
    assert ramp.max() == pytest.approx(0.4204, abs=5e-5) and ramp.max() <= top
    assert not np.any((fn > top) & (fn < 1.0))


def test_quirk_right_only_sponge_masks_the_left_boundary():
    """wl = 0: xxmin_c = xxmin = bmin, and 'x <= xxmin_c' gives fn = 1 at exactly x == bmin."""
    sx, _ = forcing.sponge_sections(forcing.SpongeConfig(xRspg=10.0, spng_st=1.0), [-10.0, -1.0], [50.0, 1.0], 2)
    assert sx.active and sx.wl == 0.0 and sx.xxmin_c == sx.xxmin == -10.0
    co = bfs_mesh()
    bmin, bmax = _extents(co)
    fn = fref.sponge_function([co["x"], co["y"]], bmin, bmax, [(0.0, 10.0), (0.0, 0.0)])
    at_inflow = co["x"] == bmin[0]
    assert at_inflow.any() and np.all(fn[at_inflow] == 1.0)
    assert not fn[(co["x"] > bmin[0]) & (co["x"] <= sx.xxmax)].any()
    assert np.count_nonzero(fref.activate_sponge(np.ones_like(fn), fn)[at_inflow]) == 0


# ---- harmonic forcing -------------------------------------------------------------------------------------

def test_harmonic_phase():
    om, c, s = forcing.harmonic_phase(0.75, 3.0)
    assert om == (8.0 * math.atan(1.0) / 3.0) * 0.75 and (c, s) == (math.cos(om), math.sin(om))
    assert om == pytest.approx(math.pi / 2, rel=1e-15) and s == 1.0
    assert forcing.harmonic_phase(0.0, 3.0) == (0.0, 1.0, 0.0)       # the first step: unforced (:19)
    assert forcing.harmonic_phase(-0.75, 3.0)[0] == -om              # a negative phase picks the imaginary branch


def test_quirks_of_the_force_in_the_restatement():
    """omega_t = 0 leaves the harmonic term out, and the perturbation sponge ignores spng_st."""
    from nekstab_next_amd.layout import NekLayout
    from nekstab_next_amd import synthetic as syn

    lay = NekLayout(2, 3, 1, 2, n_scalars=1)
    vec = lambda seed: syn.hash_vector(lay, seed)[:lay.rows].copy()   # noqa: E731
    v, fre, fim = vec(1), vec(2), vec(3)
    fn = np.abs(syn.hash_vector(lay, 4)[:lay.n_v])
    ff = fref.nekstab_forcing(lay, np.zeros(lay.rows), v, omega_t=0.0, fR_Re=fre, fR_Im=fim)
    assert not ff.any()
    a = fref.nekstab_forcing(lay, np.zeros(lay.rows), v, spng_st=1.0, spng_fn=fn, jp=1)
    b = fref.nekstab_forcing(lay, np.zeros(lay.rows), v, spng_st=7.5, spng_fn=fn, jp=1)
    assert np.array_equal(a, b) and a.any()
    for c in range(lay.n_wf):
        s = slice(c * lay.sv, c * lay.sv + lay.n_v)
        assert np.array_equal(a[s], 0.0 - fn * v[s])
    assert not a[lay.n_wf * lay.sv:].any()                           # the pressure is not forced


# ---- ABI wiring -------------------------------------------------------------------------------------------

def test_entries_are_declared_and_typed():
    from nekstab_next_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "nekkrylov.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("nkv_sponge_fn", 10), ("nkv_body_force", 15)):
        assert name in _lib.EXPORTED
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib._SIGNATURES[name][1]), name
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define NKV_ABI_VERSION 3\b", hdr) and _lib.NKV_ABI_VERSION == 3
    assert _lib.load().nkv_abi_version() == 3
    defs = {k: int(v, 0) for k, v in re.findall(r"#define (NKV_[A-Z0-9_]+)\s+(0x[0-9a-f]+)u", hdr)}
    assert defs["NKV_BF_IMAG"] == _lib.NKV_BF_IMAG and defs["NKV_BF_PERTURBATION"] == _lib.NKV_BF_PERTURBATION
    flags = [v for k, v in defs.items() if k not in ("NKV_ACCUMULATE",)]
    assert len(set(flags)) == len(flags)                          # no flag bit is shared
    # the reference lines each entry replaces are cited, as for every other entry
    assert "forcing.f90:157-251" in hdr and "forcing.f90:2-79" in hdr and ":101-104" in hdr
    src = open(os.path.join(ROOT, "nekstab_next_amd", "csrc", "forcing.hip")).read()
    assert "forcing.f90:157-251" in src and "5 ldim + 1" in src and "fp contract(off)" in src
    internal = open(os.path.join(ROOT, "nekstab_next_amd", "csrc", "nkv_internal.h")).read()
    assert "forcing.hip" in internal


def test_package_exports_the_classes():
    import nekstab_next_amd as pkg

    assert pkg.forcing is forcing
    assert pkg.Sponge is forcing.Sponge and pkg.BodyForce is forcing.BodyForce
    assert pkg.SpongeConfig is forcing.SpongeConfig
