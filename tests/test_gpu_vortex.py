"""GPU parity of the flow-diagnostics layer (vortex criteria, filter_s0, vorticity, energy / enstrophy)
against the NumPy restatement (tests/vortex_reference.py).

Gates (every one covers every point):

1. ``grad`` of ``nkv_vortex_criteria`` is bit-identical to ``nkv_gradm1``.
2. The rational criteria (vorticity, q, delta, symmetric, assymetric, omega, 2-D swirling / lambda_ci) and
   lambda2 on the device's own gradient are bit-identical to the restatement: only IEEE + - * / sqrt in
   a fixed order without contraction.  lambda2 has no transcendental call (cyclic Jacobi), so the
   issue-style bound (U_dev + U_host + 2) eps (|tr/3| + 2 p) with U = 0 holds a fortiori.
3. 3-D lambda_ci (swirling before the square): everything up to the two cube roots is bit-identical, so
   the branch h <= 0 is the same at every point (asserted).  lci = (s - u) sqrt(3)/2 with s, u = cbrt(.):
   the device's cbrt is within U_dev = 2 ulp (no ULP table ships with the HIP headers here; the OpenCL
   f64 bound for cbrt is 2), glibc's within U_host = 1, so s and u each differ by at most 3 ulp, i.e.
   3 eps |s| and 3 eps |u|; the subtraction, the product with sqrt(3) (< 1 after the division by 2) add
   two roundings of at most eps (|s| + |u|): |lci_dev - lci_host| <= (2 + 1 + 2) eps (|s| + |u|).
   The squared ``swirling`` output then differs by at most 2 lci g + g^2 + eps lci^2 (g the bound above).
4. ``nkv_filter_s0`` is bit-identical to the restatement's explicit ascending-m loops; a field of
   per-direction degree <= lx1 - 2 on the affine box is unchanged to 3 lx1 eps ||F||_inf^3 max|v|; in place
   equals out of place; nfld = 1 and 5.
5. A fused filtered output is bit-identical to the raw output followed by ``nkv_filter_s0`` (swirling: the
   square after the standalone filter of lambda_ci; lambda2 and vorticity stay raw).
6. The chain against the independent gradient (``oracle.gradm1``): averaged vorticity to 1e-12 max|w|,
   energy and enstrophy sums to 1e-12 sum w f^2, the records as the PKE test compares its E15.7 lines.
7. Known answers on the device (rotation, strain; affine and deformed box; filtered and unfiltered).
8. Hygiene: NaN padding, element sub-ranges, the NaN flag, argument checks, empty shard.
9. The opt-in hooks of ``outpost_ks`` and ``SFD``.
"""
import functools

import numpy as np
import pytest
import torch

import energy_budget_reference as ebr
import nekio
import vortex_reference as vr
from seed_helpers import box_mesh_coords
from test_bf_sensitivity import _cyl, deformed_box

from nekstab_next_amd import _lib, fixedp, fld
from nekstab_next_amd import synthetic as syn
from nekstab_next_amd import vortex as vx
from nekstab_next_amd.layout import NekLayout
from nekstab_next_amd.newton import fortran_e
from nekstab_next_amd.seeds import FaceAverage
from nekstab_next_amd.sensitivity import Gradm1, velocity_layout
from nekstab_next_amd.vector import NekContext

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _cases():
    yield "cyl", NekLayout(ldim=2, lx1=6, lx2=4, nelgv=1996), None
    for lx1, ne in ((5, (3, 2, 2)), (8, (2, 3, 2)), (8, (1, 1, 1)), (6, (5, 3, 3)), (4, (7, 1, 1)), (10, (2, 1, 1)),
                    (3, (5, 1, 1))):
        yield f"box{lx1}_{np.prod(ne)}", NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=int(np.prod(ne))), ne


CASES = list(_cases())
IDS = [c[0] for c in CASES]
ALL3 = ["vorticity", "lambda2", "q", "delta", "swirling", "omega", "symmetric", "assymetric", "lambda_ci"]
FILTERABLE = ["q", "delta", "swirling", "omega", "symmetric", "assymetric", "lambda_ci"]


def _names(ldim):
    return [n for n in ALL3 if ldim == 3 or n != "lambda2"]


def _ctx(lay):
    vlay = velocity_layout(lay)
    return NekContext(vlay, weights=syn.mass_weights(vlay), max_cols=4)


def _coords(lay, ne):
    return _cyl() if ne is None else deformed_box(lay, ne)


def _velocity(co, ldim, seed):
    rng = np.random.default_rng(seed)
    x, y = co["x"], co["y"]
    z = co.get("z", np.zeros_like(x))
    return [np.sin(1.3 * x + 0.2 * c) * np.cos(0.7 * y - 0.4 * c) + 0.2 * (c + 1) * z * x + 0.3 * z * z
            + 1e-3 * rng.standard_normal(x.size) for c in range(ldim)]


def _dev(ctx, comps, stride):
    t = torch.zeros(len(comps) * stride, dtype=torch.float64, device=ctx.device)
    for c, a in enumerate(comps):
        t[c * stride: c * stride + a.size] = torch.as_tensor(np.asarray(a, dtype=np.float64)).to(ctx.device)
    return t


class _Run:
    """One velocity on the device and ``nkv_vortex_criteria`` on element sub-ranges of it."""

    def __init__(self, ctx, co, vel, pad=6):
        self.ctx, self.lay = ctx, ctx.layout
        self.core = vx.VortexCore(ctx, co)
        self.n = self.lay.n_v
        self.stride = self.n + pad
        self.u = _dev(ctx, vel, self.stride)
        self.pts = self.lay.lx1 ** self.lay.ldim

    def __call__(self, names, filtered=(), e0=0, e1=None, grad=False, F=True):
        lay, d = self.lay, self.lay.ldim
        e1 = self.n // self.pts if e1 is None else e1
        L = lay.c_struct()
        L.n_v = (e1 - e0) * self.pts
        off = 8 * e0 * self.pts
        sl = self.core.slots(names)
        ns = max(1, sum(k for _, k in sl.values()))
        out = torch.full((ns, self.stride), np.nan, dtype=torch.float64, device=self.ctx.device)
        g = torch.full((d * d, self.stride), np.nan, dtype=torch.float64, device=self.ctx.device)
        xyz = [t.data_ptr() + off for t in self.core.xyz] + ([None] if d == 2 else [])
        mask = sum(1 << vx.CRITERIA[nm] for nm in names)
        fmask = sum(1 << vx.CRITERIA[nm] for nm in filtered)
        rc = self.ctx.lib.nkv_vortex_criteria(
            L, lay.lx1, d, self.core.D.data_ptr(), self.core.F.data_ptr() if F else None, *xyz,
            self.u.data_ptr() + off, self.stride, mask, fmask, out.data_ptr() + off, self.stride,
            (g.data_ptr() + off) if grad else None, self.stride, self.ctx.stream)
        _lib.check(rc, "nkv_vortex_criteria")
        torch.cuda.synchronize()
        res = {nm: out[s:s + k].cpu().numpy() for nm, (s, k) in sl.items()}
        return (res, g.cpu().numpy().reshape(d, d, -1)) if grad else res


@functools.lru_cache(maxsize=None)
def _case(name):
    _, lay, ne = CASES[IDS.index(name)]
    return lay, _coords(lay, ne)


def _run(name, seed=11):
    lay, co = _case(name)
    ctx = _ctx(lay)
    return _Run(ctx, co, _velocity(co, lay.ldim, seed)), lay, co


# ---- 1. gradient ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_gradient_is_gradm1_bitwise(gpu, name):
    run, lay, co = _run(name)
    d, n = lay.ldim, run.n
    _, g = run(_names(d), filtered=FILTERABLE, grad=True)
    _, g0 = run([], grad=True)                               # mask = 0: the gradient alone
    want = torch.full((d * d, n), np.nan, dtype=torch.float64, device=run.ctx.device)
    Gradm1(run.ctx, co)(run.u.data_ptr(), want.data_ptr(), nfld=d, u_stride=run.stride)
    want = want.cpu().numpy().reshape(d, d, n)
    assert np.array_equal(g[:, :, :n], want) and np.array_equal(g0[:, :, :n], want)
    assert np.all(np.isnan(g[:, :, n:])) and np.all(np.isnan(g0[:, :, n:]))


# ---- 2. + 3. criteria on the device's own gradient ---------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_criteria_on_device_gradient(gpu, name):
    run, lay, co = _run(name)
    d, n = lay.ldim, run.n
    names = _names(d)
    res, g = run(names, grad=True)                           # one launch, everything raw
    G = g[:, :, :n]
    assert np.all(np.isfinite(G))
    for nm, a in res.items():
        assert np.all(np.isnan(a[:, n:])), nm                # padding beyond n_v untouched
        assert np.all(np.isfinite(a[:, :n])), nm
    assert np.array_equal(res["vorticity"][:, :n], vr.vorticity(G))
    for nm, fn in vr.RATIONAL.items():
        assert np.array_equal(res[nm][0, :n], fn(G)), nm
    lci, scale = vr.swirling_raw(G)
    got = res["lambda_ci"][0, :n]
    if d == 2:
        assert np.array_equal(got, lci)
        assert np.array_equal(res["swirling"][0, :n], lci * lci)
    else:
        l2, l2scale = vr.lambda2(G)
        err2 = np.max(np.abs(res["lambda2"][0, :n] - l2) / l2scale)
        print(f"{name}: lambda2 device vs restatement worst {err2 / EPS:.2f} eps of |tr/3| + 2p")
        assert np.array_equal(res["lambda2"][0, :n], l2)
        assert np.array_equal(got > 0, lci > 0)              # the same branch at every point
        gate = (2 + 1 + 2) * EPS * scale
        err = np.abs(got - lci)
        live = scale > 0
        print(f"{name}: lambda_ci worst {np.max(err[live] / (EPS * scale[live])) if live.any() else 0:.2f} "
              f"eps (|s|+|u|), {int(live.sum())} of {n} points swirl")
        assert np.all(err <= gate)
        sq = res["swirling"][0, :n]
        assert np.all(np.abs(sq - lci * lci) <= 2 * lci * gate + gate * gate + EPS * lci * lci)
        assert np.array_equal(sq, got * got)                 # the square of the device's own lambda_ci


# ---- 4. filter ------------------------------------------------------------------------------------
def _filter(ctx, core, v, nfld, v_stride, o_stride=None, in_place=False):
    lay = ctx.layout
    out = v if in_place else torch.full((nfld * o_stride,), np.nan, dtype=torch.float64, device=ctx.device)
    ctx.call("nkv_filter_s0", lay.lx1, lay.ldim, core.F.data_ptr(), v.data_ptr(), v_stride, nfld, out.data_ptr(),
             v_stride if in_place else o_stride, ctx.stream)
    return out


@pytest.mark.parametrize("nfld", [1, 5])
@pytest.mark.parametrize("name", IDS)
def test_filter_bitwise_vs_restatement(gpu, name, nfld):
    lay, co = _case(name)
    ctx = _ctx(lay)
    core = vx.VortexCore(ctx, co)
    n = ctx.layout.n_v
    rng = np.random.default_rng(31)
    fields = [np.sin((1 + 0.2 * f) * co["x"]) * np.cos(0.6 * co["y"] + f) + 0.1 * rng.standard_normal(n)
              for f in range(nfld)]
    vs, os_ = n + 10, n + 4
    v = _dev(ctx, fields, vs)
    out = _filter(ctx, core, v, nfld, vs, os_).cpu().numpy().reshape(nfld, os_)
    F = core.F.cpu().numpy()
    for f in range(nfld):
        assert np.array_equal(out[f, :n], vr.filter_s0(fields[f], F, lay.lx1, lay.ldim)), f
    assert np.all(np.isnan(out[:, n:]))
    ip = _filter(ctx, core, v.clone(), nfld, vs, in_place=True).cpu().numpy().reshape(nfld, vs)
    assert np.array_equal(ip[:, :n], out[:, :n]) and not ip[:, n:].any()


@pytest.mark.parametrize("lx1", [3, 5, 8])
def test_filter_keeps_low_degree_fields(gpu, lx1):
    lay = NekLayout(ldim=3, lx1=lx1, lx2=max(lx1 - 2, 1), nelgv=4)
    co = box_mesh_coords(lay, (2, 2, 1))
    ctx = _ctx(lay)
    core = vx.VortexCore(ctx, co)
    n = ctx.layout.n_v
    k = lx1 - 2
    v = (1 + co["x"] ** k) * (2 - co["y"] ** k) + (co["z"] - 0.3) ** k * co["x"]
    out = _filter(ctx, core, _dev(ctx, [v], n), 1, n, n).cpu().numpy()
    F = core.F.cpu().numpy()
    bound = 3 * lx1 * EPS * np.max(np.sum(np.abs(F), axis=1)) ** 3 * np.max(np.abs(v))
    print(f"lx1={lx1}: filter moves a degree-{k} field by {np.max(np.abs(out - v)):.2e}, bound {bound:.2e}")
    assert np.max(np.abs(out - v)) <= bound


# ---- 5. fusion ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_fused_filter_equals_raw_then_standalone(gpu, name):
    run, lay, co = _run(name, seed=12)
    ctx, core, d, n = run.ctx, run.core, lay.ldim, run.n
    names = _names(d)
    raw = run(names)
    fused = run(names, filtered=names)                       # one launch, several criteria, all "filtered"

    def standalone(a):
        return _filter(ctx, core, _dev(ctx, [a], n), 1, n, n).cpu().numpy()

    for nm in names:
        if nm in ("vorticity", "lambda2"):                   # never filtered
            assert np.array_equal(fused[nm][:, :n], raw[nm][:, :n]), nm
        elif nm == "swirling":
            f = standalone(raw["lambda_ci"][0, :n])
            assert np.array_equal(fused[nm][0, :n], f * f)
        else:
            assert np.array_equal(fused[nm][0, :n], standalone(raw[nm][0, :n])), nm
        assert np.all(np.isnan(fused[nm][:, n:]))
    # each criterion on its own launch gives the same bits, filtered or not, and F = NULL means raw
    for nm in FILTERABLE:
        assert np.array_equal(run([nm], filtered=[nm])[nm], fused[nm], equal_nan=True), nm
    nof = run(names, filtered=names, F=False)
    for nm in names:
        assert np.array_equal(nof[nm], raw[nm], equal_nan=True), nm
    part = run(names, filtered=["q"])
    assert np.array_equal(part["q"], fused["q"], equal_nan=True)
    assert np.array_equal(part["omega"], raw["omega"], equal_nan=True)


# ---- 6. the chain against the independent gradient ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain_case(case):
    if case == "cyl":
        lay, co = NekLayout(ldim=2, lx1=6, lx2=4, nelgv=1996), _cyl()
    else:
        lay = NekLayout(ldim=3, lx1=6, lx2=4, nelgv=18)
        co = deformed_box(lay, (3, 3, 2))
    vel = _velocity(co, lay.ldim, 21)
    G = vr.gradient_tensor(lay.lx1, lay.ldim, co, vel)
    return lay, co, ebr.GroupAverage(co), vel, G


def _vector(ctx, comps):
    vl = ctx.layout
    host = np.zeros(vl.ld)
    for c, a in enumerate(comps):
        host[c * vl.sv: c * vl.sv + vl.n_v] = a
    return ctx.vector().from_packed(host)


def _ulp7(x):
    return 0.0 if x == 0 else 10.0 ** (np.floor(np.log10(abs(x))) + 1 - 7)


def _check_record(line, values, gates):
    """As the PKE test: the same text wherever the seven digits do not depend on where inside the gate the
    value lies, else the parsed values agree to the gate plus one unit of the seventh digit."""
    assert len(line) == 15 * len(values)
    for k, (v, gt) in enumerate(zip(values, gates)):
        got = line[15 * k: 15 * k + 15]
        if fortran_e(v - gt, 15, 7) == fortran_e(v + gt, 15, 7):
            assert got == fortran_e(v, 15, 7), (k, got)
        else:
            assert abs(float(got) - float(fortran_e(v, 15, 7))) <= gt + _ulp7(v), (k, got)


@pytest.mark.parametrize("case", ["cyl", "box"])
def test_vorticity_energy_enstrophy_chain(gpu, tmp_path, case):
    lay, co, avg, vel, G = _chain_case(case)
    ctx = _ctx(lay)
    vl, d, n = ctx.layout, lay.ldim, lay.n_v
    w = syn.mass_weights(vl)
    core = vx.VortexCore(ctx, co)
    vec = _vector(ctx, vel)
    fa = FaceAverage(ctx, co).apply
    got = core.comp_vort3(vec, fa)[:, :n].cpu().numpy()
    ref = vr.comp_vort3(G, w, avg)
    scale = np.max(np.abs(ref))
    print(f"{case}: averaged vorticity err {np.max(np.abs(got - ref)) / scale:.2e} of max|w|")
    assert scale > 0 and got.shape == ref.shape and np.max(np.abs(got - ref)) <= 1e-12 * scale
    raw = core.comp_vort3(vec, None)[:, :n].cpu().numpy()
    assert np.max(np.abs(raw - vr.vorticity(G))) <= 1e-12 * scale
    assert np.array_equal(core.comp_vort3(vec, fa)[:, :n].cpu().numpy(), got)   # cached denominator: same bits

    vol = float(np.sum(w)) + 0.5
    em = vx.EnergyMonitor(ctx, tmp_path / "total_energy.dat", skip=1, volume=vol)
    zm = vx.EnstrophyMonitor(ctx, core, tmp_path / "total_enstrophy.dat", skip=1, volume=vol, average=fa)
    es, zs = em(vec, 4, 0.25), zm(vec, 4, 0.25)
    em.close(), zm.close()
    ctx.check_nan()
    eref, zref = vr.component_sums(w, vel), vr.component_sums(w, list(ref))
    for gotv, refv in ((es, eref), (zs, zref)):
        tot = sum(refv)
        for c in range(3):
            assert abs(gotv[c] - refv[c]) <= 1e-12 * tot, c
        assert gotv[3] == 0.0
    eek = 0.5 / vol
    for path, refv, npot in ((tmp_path / "total_energy.dat", eref, 1), (tmp_path / "total_enstrophy.dat", zref, 0)):
        lines = open(path).read().split("\n")
        assert lines[-1] == "" and len(lines) == 2
        tot = sum(refv)
        vals = [0.25] + [s * eek for s in refv] + [((refv[0] + refv[1]) + refv[2]) * eek] + [0.0] * npot
        gates = [0.0] + [1e-12 * tot * eek] * 3 + [3e-12 * tot * eek] + [0.0] * npot
        _check_record(lines[0], vals, gates)


def test_outpost_files(gpu, tmp_path):
    lay, co, avg, vel, G = _chain_case("box")
    ctx = _ctx(lay)
    n = lay.n_v
    core = vx.VortexCore(ctx, co)
    vec = _vector(ctx, vel)
    fa = FaceAverage(ctx, co).apply
    paths = vx.nekstab_outpost(ctx, vec, 3, core, outdir=str(tmp_path), session="vt", average=fa, time=1.5, istep=7)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["vorvt0.f00003", "voxvt0.f00003"]
    w = core.comp_vort3(vec, fa)[:, :n].cpu().numpy()
    tok, ids, fields = nekio.read_std(paths[0])
    assert tok[11] == "U" and float(tok[7]) == 1.5 and np.array_equal(ids, np.arange(1, lay.nelgv + 1))
    for k, nm in enumerate(("vx", "vy", "vz")):
        assert np.array_equal(fields[nm].ravel(), w[k])
    c = core.criteria(vec, ["lambda2", "q", "omega"])
    tok, _, fields = nekio.read_std(paths[1])
    assert tok[11] == "U"
    for nm, key in (("vx", "lambda2"), ("vy", "q"), ("vz", "omega")):
        assert np.array_equal(fields[nm].ravel(), c[key][:n].cpu().numpy())
    assert torch.equal(c["q"], core.vortex_core(vec, "q")) and torch.equal(c["lambda2"], core.vortex_core(vec, "lambda2"))
    with pytest.raises(ValueError, match="vortex determinant"):
        core.vortex_core(vec, "vorticity")
    # 2-D: omega in the temperature slot of vox, the single vorticity component as vx
    lay2, co2, _, vel2, _ = _chain_case("cyl")
    ctx2 = _ctx(lay2)
    core2 = vx.VortexCore(ctx2, co2)
    vec2 = _vector(ctx2, vel2)
    p2 = vx.nekstab_outpost(ctx2, vec2, 1, core2, outdir=str(tmp_path), session="v2", average=None)
    f = fld.read_fld(p2[1])
    assert f.rdcode == "T"
    assert np.array_equal(f.fields["t"].ravel(), core2.vortex_core(vec2, "omega")[: lay2.n_v].cpu().numpy())
    f = fld.read_fld(p2[0])
    assert f.rdcode == "U" and not f.fields["vy"].any()
    assert np.array_equal(f.fields["vx"].ravel(), core2.comp_vort3(vec2, None)[0, : lay2.n_v].cpu().numpy())


# ---- 7. known answers -----------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["affine", "deformed"])
def test_known_answers_on_device(gpu, mesh):
    ne = (3, 2, 2)
    lay = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=12)
    co = box_mesh_coords(lay, ne) if mesh == "affine" else deformed_box(lay, ne)
    ctx = _ctx(lay)
    n = lay.n_v
    core = vx.VortexCore(ctx, co)
    Om, a = 0.7, 1.3
    tol = dict(rtol=0, atol=1e-9)
    rot = _vector(ctx, [-Om * co["y"] + 0.5, Om * co["x"] - 1.0, 0.0 * co["x"] + 2.0])
    strain = _vector(ctx, [a * co["x"], -a * co["y"], 0.0 * co["x"]])
    names = ["vorticity", "lambda2", "q", "delta", "swirling", "omega", "symmetric", "assymetric"]
    for filtered in (True, False):                           # linear fields: the filter changes nothing
        r = {k: v[..., :n].cpu().numpy() for k, v in core.criteria(rot, names, filtered=filtered).items()}
        np.testing.assert_allclose(r["q"], Om ** 2, **tol)
        np.testing.assert_allclose(r["vorticity"][0], 0.0, **tol)
        np.testing.assert_allclose(r["vorticity"][1], 0.0, **tol)
        np.testing.assert_allclose(r["vorticity"][2], 2 * Om, **tol)
        np.testing.assert_allclose(r["swirling"], Om ** 2, **tol)
        np.testing.assert_allclose(r["delta"], (Om ** 2 / 3) ** 3, **tol)
        np.testing.assert_allclose(r["lambda2"], -Om ** 2, **tol)
        np.testing.assert_allclose(r["omega"], 4 * Om ** 4 / (4 * Om ** 4 + 1e-5), **tol)
        np.testing.assert_allclose(r["symmetric"], 0.0, **tol)
        np.testing.assert_allclose(r["assymetric"], 0.0, **tol)
        s = {k: v[..., :n].cpu().numpy() for k, v in core.criteria(strain, names, filtered=filtered).items()}
        np.testing.assert_allclose(s["q"], -a ** 2, **tol)
        np.testing.assert_allclose(s["swirling"], 0.0, **tol)
        np.testing.assert_allclose(s["lambda2"], a ** 2, **tol)
        np.testing.assert_allclose(s["vorticity"], 0.0, **tol)
        np.testing.assert_allclose(s["symmetric"], a ** 2, **tol)
        np.testing.assert_allclose(s["omega"], 0.0, **tol)


# ---- 8. hygiene -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("box5_12", 5), ("box4_7", 3), ("cyl", 1001)])
def test_criteria_are_element_local(gpu, name, k):
    run, lay, co = _run(name, seed=13)
    names = _names(lay.ldim)
    n, pts, E = run.n, run.pts, lay.nelgv
    whole, gw = run(names, filtered=names, grad=True)
    lo, gl = run(names, filtered=names, e1=k, grad=True)
    hi, gh = run(names, filtered=names, e0=k, e1=E, grad=True)
    for nm in names:
        assert np.array_equal(lo[nm][:, : k * pts], whole[nm][:, : k * pts]), nm
        assert np.array_equal(hi[nm][:, k * pts: n], whole[nm][:, k * pts: n]), nm
        assert np.all(np.isnan(lo[nm][:, k * pts:])) and np.all(np.isnan(hi[nm][:, : k * pts])), nm
    assert np.array_equal(gl[:, :, : k * pts], gw[:, :, : k * pts]) and np.array_equal(gh[:, :, k * pts: n], gw[:, :, k * pts: n])


# (ncomp, n, pad, with pot): even strides take the 16-byte path (odd last point at n = 375), odd the 8-byte one
@pytest.mark.parametrize("ncomp,n,pad,pot", [(3, 375, 5, True), (3, 375, 6, False), (2, 7992, 8, True), (1, 4096, 0, False),
                                             (3, 300001, 1, True)])
def test_energy_components(gpu, ncomp, n, pad, pot):
    lay = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=n // 125 + 1)   # sv >= n; the entry sees n_v = n
    ctx = _ctx(lay)
    L = ctx.layout.c_struct()
    L.n_v = n
    rng = np.random.default_rng(n + pad)
    f = list(rng.standard_normal((ncomp, n)))
    w, t, y = rng.uniform(0.5, 1.5, n), rng.standard_normal(n), rng.standard_normal(n)
    stride = n + pad
    fd, wd, td, yd = _dev(ctx, f, stride), _dev(ctx, [w], n), _dev(ctx, [t], n), _dev(ctx, [y], n)
    sums = torch.full((4,), np.nan, dtype=torch.float64, device=ctx.device)
    ws = ctx.ws
    for rep in range(2):
        rc = ctx.lib.nkv_energy_components(L, wd.data_ptr(), fd.data_ptr(), stride, ncomp, td.data_ptr() if pot else None,
                                           yd.data_ptr() if pot else None, sums.data_ptr(), ws.data_ptr(), ctx.stream)
        _lib.check(rc, "nkv_energy_components")
        got = sums.cpu().numpy()
        if rep:
            assert np.array_equal(got, first)                # run-to-run deterministic
        first = got.copy()
    tot = sum(float(np.sum(w * c * c)) for c in f)
    for c in range(3):
        ref = float(np.sum((f[c] * w) * f[c])) if c < ncomp else 0.0
        assert abs(got[c] - ref) <= 1e-12 * tot, c
    if pot:
        assert abs(got[3] - float(np.sum((t * w) * y))) <= 1e-12 * float(np.sum(np.abs(t * w * y)))
    else:
        assert got[3] == 0.0


def test_energy_components_nan_raises_the_workspace_flag(gpu):
    lay = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=12)
    ctx = _ctx(lay)
    n = ctx.layout.n_v
    rng = np.random.default_rng(2)
    f = list(rng.standard_normal((3, n)))
    f[1][77] = np.nan
    fd = _dev(ctx, f, n)
    sums = torch.zeros(4, dtype=torch.float64, device=ctx.device)
    ctx.call("nkv_energy_components", ctx.w.data_ptr(), fd.data_ptr(), n, 3, None, None, sums.data_ptr(),
             ctx.ws.data_ptr(), ctx.stream)
    got = sums.cpu().numpy()
    assert np.isnan(got[1]) and np.isfinite(got[[0, 2, 3]]).all()
    with pytest.raises(_lib.NkvNaNError):
        ctx.check_nan()
    ctx.check_nan()                                          # the flag is cleared by the read


def test_argument_checks(gpu):
    lay = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=2)
    ctx = _ctx(lay)
    co = box_mesh_coords(lay, (2, 1, 1))
    core = vx.VortexCore(ctx, co)
    n = ctx.layout.n_v
    z = lambda k: torch.zeros(k * n, dtype=torch.float64, device=ctx.device)  # noqa: E731
    u, out, g, sums = z(3), z(11), z(9), z(1)
    lib, ws = ctx.lib, ctx.ws.data_ptr()
    every = (1 << _lib.NKV_VC_COUNT) - 1

    def bad(fn, args, word, **kw):
        rc = fn(*{**args, **kw}.values())
        assert rc == _lib.NKV_EINVAL, (kw, rc)
        assert word in _lib.last_error(), (kw, _lib.last_error())

    V = dict(L=ctx._Lp, lx1=5, ldim=3, D=core.D.data_ptr(), F=core.F.data_ptr(), xm=core.xyz[0].data_ptr(),
             ym=core.xyz[1].data_ptr(), zm=core.xyz[2].data_ptr(), u=u.data_ptr(), u_stride=n, mask=every,
             filter_mask=every, out=out.data_ptr(), o_stride=n, grad=g.data_ptr(), g_stride=n, stream=ctx.stream)
    fn = lib.nkv_vortex_criteria
    assert fn(*V.values()) == _lib.NKV_OK
    assert fn(*{**V, "grad": None, "g_stride": 0}.values()) == _lib.NKV_OK
    assert fn(*{**V, "F": None}.values()) == _lib.NKV_OK
    assert fn(*{**V, "mask": 0, "out": None}.values()) == _lib.NKV_OK
    bad(fn, V, "ldim", ldim=4)
    bad(fn, V, "lx1", lx1=11)
    bad(fn, V, "n_v", lx1=6)
    bad(fn, V, "zm", zm=None)
    bad(fn, V, "mask", mask=1 << _lib.NKV_VC_COUNT)
    bad(fn, V, "filter_mask", filter_mask=1 << 12)
    bad(fn, V, "mask", mask=0, grad=None)
    for s in ("u_stride", "o_stride", "g_stride"):
        bad(fn, V, s, **{s: n - 1})
    for p in ("D", "xm", "ym", "u", "out"):
        bad(fn, V, p, **{p: None})
    # 2-D: lambda2 is refused (25 points divide n_v, no zm)
    bad(fn, V, "lambda2", ldim=2, zm=None, mask=1 << _lib.NKV_VC_LAMBDA2)
    assert fn(*{**V, "ldim": 2, "zm": None, "mask": every & ~(1 << _lib.NKV_VC_LAMBDA2)}.values()) == _lib.NKV_OK
    # lx1 = 2 with a filter is refused, without one it runs
    L2 = ctx.layout.c_struct()
    L2.n_v = 8 * (n // 8)
    bad(fn, V, "lx1", L=L2, lx1=2)
    assert fn(*{**V, "L": L2, "lx1": 2, "F": None}.values()) == _lib.NKV_OK

    S = dict(L=ctx._Lp, lx1=5, ldim=3, F=core.F.data_ptr(), v=u.data_ptr(), v_stride=n, nfld=3, out=out.data_ptr(),
             o_stride=n, stream=ctx.stream)
    fn = lib.nkv_filter_s0
    assert fn(*S.values()) == _lib.NKV_OK
    bad(fn, S, "ldim", ldim=1)
    bad(fn, S, "lx1", lx1=2)
    bad(fn, S, "lx1", lx1=11)
    bad(fn, S, "n_v", lx1=4)
    bad(fn, S, "nfld", nfld=0)
    for s in ("v_stride", "o_stride"):
        bad(fn, S, s, **{s: n - 1})
    for p in ("F", "v", "out"):
        bad(fn, S, p, **{p: None})

    Eg = dict(L=ctx._Lp, w=ctx.w.data_ptr(), f=u.data_ptr(), f_stride=n, ncomp=3, t=None, y=None,
              sums_dev=out.data_ptr(), ws=ws, stream=ctx.stream)
    fn = lib.nkv_energy_components
    assert fn(*Eg.values()) == _lib.NKV_OK
    bad(fn, Eg, "ncomp", ncomp=0)
    bad(fn, Eg, "ncomp", ncomp=4)
    bad(fn, Eg, "f_stride", f_stride=n - 1)
    bad(fn, Eg, "t and y", t=u.data_ptr())
    for p in ("w", "f", "sums_dev", "ws"):
        bad(fn, Eg, p, **{p: None})

    # an empty shard: NKV_OK, no pointer read; the sums are four zeros
    E0 = ctx.layout.c_struct()
    E0.n_v = 0
    none = {k: None for k in ("D", "F", "xm", "ym", "zm", "u", "out", "grad")}
    assert lib.nkv_vortex_criteria(*{**V, **none, "L": E0}.values()) == _lib.NKV_OK
    assert lib.nkv_filter_s0(*{**S, "L": E0, "F": None, "v": None, "out": None}.values()) == _lib.NKV_OK
    four = torch.full((4,), np.nan, dtype=torch.float64, device=ctx.device)
    assert fn(*{**Eg, "L": E0, "w": None, "f": None, "sums_dev": four.data_ptr()}.values()) == _lib.NKV_OK
    assert torch.equal(four, torch.zeros_like(four))
    ctx.check_nan()
    with pytest.raises(ValueError, match="auto"):
        core.comp_vort3(ctx.vector(), "dssum")
    del sums


# ---- 9. hooks -------------------------------------------------------------------------------------
def test_outpost_ks_vorticity_hook(gpu, tmp_path):
    from nekstab_next_amd.config import KrylovSchurConfig
    from nekstab_next_amd.krylov_schur import krylov_schur, outpost_ks
    from nekstab_next_amd.operators import DiagOperator

    lay = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=12)
    co = deformed_box(lay, (3, 2, 2))
    ctx = NekContext(lay, weights=syn.mass_weights(lay), max_cols=32)
    d, _ = syn.diag_spectrum(lay)
    seed = ctx.vector()
    seed.fill_hash(11)
    res = krylov_schur(ctx, DiagOperator(ctx, d), seed, KrylovSchurConfig(k_dim=16, schur_tgt=3))
    core = vx.VortexCore(ctx, co)
    kw = dict(evop="d", maxmodes=2, session="hk", orthonormality=False)
    a, b, c = (tmp_path / s for s in "abc")
    outpost_ks(ctx, res, str(a), **kw)
    outpost_ks(ctx, res, str(b), vorticity=None, **kw)
    out = outpost_ks(ctx, res, str(c), vorticity=core, **kw)
    assert len(out["modes"]) == 2
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir()) and not any("Rv" in nm for nm in names)
    for nm in names:                                         # hook off: byte-identical outputs
        assert (a / nm).read_bytes() == (b / nm).read_bytes() == (c / nm).read_bytes(), nm
    assert sorted(p.name for p in c.iterdir()) == sorted(names + ["dRvhk0.f00001", "dRvhk0.f00002"])
    for num in (1, 2):
        mode = fld.read_fld(str(c / fld.fld_name("dRe", "hk", 0, num)))
        vec = ctx.vector().from_packed(fld.vector_from_fld(lay, mode))
        want = core.comp_vort3(vec, "auto")[:, : lay.n_v].cpu().numpy()
        f = fld.read_fld(str(c / fld.fld_name("dRv", "hk", 0, num)))
        assert f.rdcode == "U" and f.time == float(num) and f.istep == num
        for k, nm in enumerate(("vx", "vy", "vz")):
            assert np.array_equal(f.fields[nm].ravel(), want[k]), (num, nm)


def test_sfd_energy_monitor_hook(gpu, tmp_path):
    lay = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=12)
    w = syn.mass_weights(lay)

    def run(monitored):
        ctx = NekContext(lay, weights=w, max_cols=4)
        mons = (vx.EnergyMonitor(ctx, tmp_path / "total_energy.dat", skip=2, volume=3.0),) if monitored else ()
        sfd = fixedp.SFD(ctx, 0.3, 0.25, 0.1, 1e-10, volume=2.0, residu=tmp_path / f"residu{int(monitored)}.dat",
                         **({"monitors": mons} if monitored else {}))
        v, fc = ctx.vector(), ctx.vector()
        v.fill_hash(100)
        sfd.start(v)
        hist = []
        for istep in range(1, 6):
            v.scal(0.97)
            fc.fill_hash(50 + istep)
            hist.append(sfd.step(v, fc))
        sfd.close()
        for m in mons:
            m.close()
        state = [t.to_packed().copy() for t in (v, fc, sfd.v_old, sfd.qbar, *sfd._q)]
        return hist, state, v.to_packed().copy(), ctx

    h0, s0, _, _ = run(False)
    h1, s1, vlast, ctx = run(True)
    assert h0 == h1
    for a, b in zip(s0, s1):
        assert np.array_equal(a, b)                          # the monitor leaves the state bit-identical
    assert (tmp_path / "residu0.dat").read_bytes() == (tmp_path / "residu1.dat").read_bytes()
    lines = open(tmp_path / "total_energy.dat").read().split("\n")
    assert lines[-1] == "" and len(lines) == 3               # steps 2 and 4 of 5 with skip = 2
    assert all(len(ln) == 90 for ln in lines[:2])
    assert lines[0][:15] == fortran_e(0.2, 15, 7) and lines[1][:15] == fortran_e(0.4, 15, 7)
    # the last record (step 4) from the state at step 5 scaled back: v_4 = v_5 / 0.97 up to one rounding
    sv, n = lay.sv, lay.n_v
    comps = [vlast[c * sv: c * sv + n] / 0.97 for c in range(3)]
    ref = vr.component_sums(w, comps)
    vals = [0.4] + [s * 0.5 / 3.0 for s in ref] + [sum(ref) * 0.5 / 3.0, 0.0]
    tot = sum(ref) * 0.5 / 3.0
    _check_record(lines[1], vals, [0.0] + [1e-12 * tot] * 3 + [3e-12 * tot, 0.0])
