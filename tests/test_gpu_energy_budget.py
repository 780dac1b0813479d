"""GPU parity of the eigenmode kinetic-energy budget (core/postproc.f90:649-872) against the NumPy
restatement (tests/energy_budget_reference.py).

* ``nkv_pke_production`` vs ``compute_production`` on ``oracle.gradm1``: fields to 1e-12 of each
  field's max (the project's gradm1 gate), integrals to 1e-12 sum(bm1 |P_ref|); ``prod = NULL`` and a
  second call give the same integral bits; padding is untouched; element sub-ranges reproduce the
  fields bit for bit;
* ``nkv_divm1`` bit-identical to (gx_x + gy_y) + gz_z from ``nkv_gradm1``'s outputs;
* ``nkv_pke_dissipation`` bit-identical to NumPy in the reference's order (both load paths);
* the whole chain (files, scaling, budget, K and PKE_ files) vs the restatement.  The quantities that
  pass through the Laplacians (two stacked differentiations: the dissipation field, integrals[9])
  take no number fixed in advance: the restatement is run in f64 and in long double on the same
  inputs, e_ref = max |f64 - long double| is its own rounding error, and the device — an equally
  valid f64 evaluation in another order — is gated at max(8 e_ref, 1e-12 scale);
* known answers on the device: linear base flow and quadratic modes on an affine box.
"""
import functools

import numpy as np
import pytest
import torch

import energy_budget_reference as ebr
import nekio
import oracle as orc
from seed_helpers import box_mesh_coords
from test_bf_sensitivity import _cyl, deformed_box
from test_energy_budget import A_BASE, quadratic_modes

from nekstab_next_amd import _lib
from nekstab_next_amd import fld
from nekstab_next_amd import synthetic as syn
from nekstab_next_amd.layout import NekLayout
from nekstab_next_amd.postproc import energy_budget_fields, stability_energy_budget
from nekstab_next_amd.seeds import FaceAverage
from nekstab_next_amd.sensitivity import Gradm1, velocity_layout
from nekstab_next_amd.vector import NekContext

pytestmark = pytest.mark.gpu


def _ctx(lay):
    vlay = velocity_layout(lay)
    return NekContext(vlay, weights=syn.mass_weights(vlay), max_cols=4)


def _cases():
    yield "cyl", NekLayout(ldim=2, lx1=6, lx2=4, nelgv=1996), None
    for lx1, ne in ((5, (3, 2, 2)), (8, (2, 3, 2)), (8, (1, 1, 1)), (6, (5, 3, 3)), (4, (7, 1, 1))):
        yield f"box{lx1}_{np.prod(ne)}", NekLayout(ldim=3, lx1=lx1, lx2=lx1 - 2, nelgv=int(np.prod(ne))), ne


CASES = list(_cases())
IDS = [c[0] for c in CASES]


def _coords(lay, ne):
    return _cyl() if ne is None else deformed_box(lay, ne)


def _fields(co, ldim, seed):
    """(base, re, im): smooth functions of the coordinates plus small noise, ldim components each."""
    rng = np.random.default_rng(seed)
    x, y = co["x"], co["y"]
    z = co.get("z", np.zeros_like(x))
    noise = lambda: 1e-3 * rng.standard_normal(x.size)  # noqa: E731
    base = [np.sin(1.3 * x + 0.2 * c) * np.cos(0.7 * y) + 0.2 * z * x + noise() for c in range(ldim)]
    re = [np.sin(0.9 * x + 0.4 * c) * np.cos(0.7 * y) + 0.1 * z + noise() for c in range(ldim)]
    im = [np.cos(0.6 * x) * np.sin(1.1 * y + 0.3 * c) - 0.2 * z + noise() for c in range(ldim)]
    return base, re, im


def _dev(ctx, comps, stride):
    t = torch.zeros(len(comps) * stride, dtype=torch.float64, device=ctx.device)
    for c, a in enumerate(comps):
        t[c * stride: c * stride + a.size] = torch.as_tensor(np.asarray(a, dtype=np.float64)).to(ctx.device)
    return t


class _Prod:
    """One set of device inputs for nkv_pke_production, callable on element sub-ranges."""

    def __init__(self, ctx, co, base, re, im, bm1, pad=6):
        self.ctx, self.lay = ctx, ctx.layout
        self.op = Gradm1(ctx, co)
        n = self.lay.n_v
        self.stride = n + pad
        self.base, self.re, self.im = (_dev(ctx, a, self.stride) for a in (base, re, im))
        self.bm1 = _dev(ctx, [bm1], n)
        self.pts = self.lay.lx1 ** self.lay.ldim

    def __call__(self, e0=0, e1=None, with_prod=True):
        lay, d, n = self.lay, self.lay.ldim, self.lay.n_v
        e1 = n // self.pts if e1 is None else e1
        L = lay.c_struct()
        L.n_v = (e1 - e0) * self.pts
        off = 8 * e0 * self.pts
        prod = torch.full((d * d, self.stride), np.nan, dtype=torch.float64, device=self.ctx.device)
        integ = torch.full((d * d,), np.nan, dtype=torch.float64, device=self.ctx.device)
        xyz = [t.data_ptr() + off for t in self.op.xyz] + ([None] if d == 2 else [])
        rc = self.ctx.lib.nkv_pke_production(
            L, lay.lx1, d, self.op.D.data_ptr(), *xyz, self.base.data_ptr() + off, self.stride,
            self.re.data_ptr() + off, self.im.data_ptr() + off, self.stride, self.bm1.data_ptr() + off,
            (prod.data_ptr() + off) if with_prod else None, self.stride, integ.data_ptr(), self.ctx.ws.data_ptr(),
            self.ctx.stream)
        _lib.check(rc, "nkv_pke_production")
        torch.cuda.synchronize()
        return prod.cpu().numpy(), integ.cpu().numpy()


def _production_reference(lay, co, base, re, im, bm1):
    d = lay.ldim
    grad = lambda u: orc.gradm1(lay.lx1, d, co, u)  # noqa: E731
    P = [ebr.compute_production(grad, base[c], re, im, c, d) for c in range(d)]
    return P, [[float(np.sum(bm1 * P[c][k])) for k in range(d)] for c in range(d)]


@pytest.mark.parametrize("name,lay,ne", CASES, ids=IDS)
def test_production_vs_restatement(gpu, name, lay, ne):
    ctx = _ctx(lay)
    co = _coords(lay, ne)
    d, n = lay.ldim, ctx.layout.n_v
    base, re, im = _fields(co, d, 11)
    bm1 = syn.mass_weights(ctx.layout)
    run = _Prod(ctx, co, base, re, im, bm1)
    prod, integ = run()
    P, I = _production_reference(lay, co, base, re, im, bm1)
    for c in range(d):
        for k in range(d):
            got, ref = prod[c * d + k, :n], P[c][k]
            err, scale = np.max(np.abs(got - ref)), np.max(np.abs(ref))
            ierr, iscale = abs(integ[c * d + k] - I[c][k]), float(np.sum(bm1 * np.abs(ref)))
            print(f"{name} P[{c}][{k}]: field err {err / scale:.2e} of max, integral err {ierr / iscale:.2e} of sum|.|")
            assert np.all(np.isfinite(got)) and scale > 0
            assert err <= 1e-12 * scale
            assert ierr <= 1e-12 * iscale
    assert np.all(np.isnan(prod[:, n:]))                    # padding untouched
    _, integ_null = run(with_prod=False)
    _, integ_again = run()
    assert np.array_equal(integ_null, integ) and np.array_equal(integ_again, integ)


@pytest.mark.parametrize("name,k", [("box5_12", 5), ("box4_7", 3), ("cyl", 1001)])
def test_production_is_element_local(gpu, name, k):
    _, lay, ne = CASES[IDS.index(name)]
    ctx = _ctx(lay)
    co = _coords(lay, ne)
    d, n = lay.ldim, ctx.layout.n_v
    base, re, im = _fields(co, d, 12)
    bm1 = syn.mass_weights(ctx.layout)
    run = _Prod(ctx, co, base, re, im, bm1)
    whole, iw = run()
    E, pts = lay.nelgv, run.pts
    lo, il = run(0, k)
    hi, ih = run(k, E)
    assert np.array_equal(lo[:, : k * pts], whole[:, : k * pts])
    assert np.array_equal(hi[:, k * pts: n], whole[:, k * pts: n])
    assert np.all(np.isnan(lo[:, k * pts:])) and np.all(np.isnan(hi[:, : k * pts]))
    P, _ = _production_reference(lay, co, base, re, im, bm1)
    for c in range(d):
        for j in range(d):
            assert abs((il + ih)[c * d + j] - iw[c * d + j]) <= 1e-12 * float(np.sum(bm1 * np.abs(P[c][j])))


def test_production_nan_raises_the_workspace_flag(gpu):
    _, lay, ne = CASES[IDS.index("box5_12")]
    ctx = _ctx(lay)
    co = _coords(lay, ne)
    base, re, im = _fields(co, 3, 13)
    base[1][77] = np.nan
    _, integ = _Prod(ctx, co, base, re, im, syn.mass_weights(ctx.layout))()
    assert np.isnan(integ[3:6]).all() and np.isfinite(integ[:3]).all()
    with pytest.raises(_lib.NkvNaNError):
        ctx.check_nan()
    ctx.check_nan()                                          # the flag is cleared by the read


def _divm1(ctx, op, g, nvec, g_stride, d_stride):
    lay = ctx.layout
    d = lay.ldim
    out = torch.full((nvec, d_stride), np.nan, dtype=torch.float64, device=ctx.device)
    xyz = [t.data_ptr() for t in op.xyz] + ([None] if d == 2 else [])
    ctx.call("nkv_divm1", lay.lx1, d, op.D.data_ptr(), *xyz, g.data_ptr(), nvec, g_stride, out.data_ptr(), d_stride,
             ctx.stream)
    return out


@pytest.mark.parametrize("nvec", [1, 6])
@pytest.mark.parametrize("name,lay,ne", CASES, ids=IDS)
def test_divm1_equals_gradm1_sum_bitwise(gpu, name, lay, ne, nvec):
    ctx = _ctx(lay)
    co = _coords(lay, ne)
    d, n = lay.ldim, ctx.layout.n_v
    op = Gradm1(ctx, co)
    rng = np.random.default_rng(21)
    x, y = co["x"], co["y"]
    stride = n + 10
    comps = [np.sin((1.0 + 0.1 * f) * x) * np.cos(0.8 * y + 0.2 * f) + 1e-3 * rng.standard_normal(n)
             for f in range(nvec * d)]
    g = _dev(ctx, comps, stride)
    div = _divm1(ctx, op, g, nvec, stride, n + 4)
    grads = torch.empty((nvec * d * d, n), dtype=torch.float64, device=ctx.device)
    op(g.data_ptr(), grads.data_ptr(), nfld=nvec * d, u_stride=stride)
    G = grads.view(nvec, d, d, n)
    for v in range(nvec):
        want = G[v, 0, 0] + G[v, 1, 1]
        if d == 3:
            want = want + G[v, 2, 2]
        assert torch.equal(div[v, :n], want), (name, v)
    assert torch.all(torch.isnan(div[:, n:]))


@pytest.mark.parametrize("name", ["cyl", "box5_12"])
def test_divm1_linear_vector_field(gpu, name):
    _, lay, ne = CASES[IDS.index(name)]
    ctx = _ctx(lay)
    co = _coords(lay, ne)
    d, n = lay.ldim, ctx.layout.n_v
    A = A_BASE[:d, :d]
    comps = [sum(A[c, k] * co["xyz"[k]] for k in range(d)) - 1.0 for c in range(d)]
    div = _divm1(ctx, Gradm1(ctx, co), _dev(ctx, comps, n), 1, n, n)
    np.testing.assert_allclose(div[0].cpu().numpy(), np.trace(A), rtol=0, atol=1e-9)


def _dissipation_numpy(re, im, lr, li, nu):
    s = 0.0 * re[0]
    for c in range(len(re)):
        dummy = re[c] * lr[c] + im[c] * li[c]
        s = s + dummy
    return 0.5 * s * nu


# (ldim, lx1, E, pad): even strides take the 16-byte path (with an odd last point at lx1 = 5, E = 3),
# odd strides the 8-byte one
@pytest.mark.parametrize("ldim,lx1,E,pad", [(2, 6, 37, 6), (3, 6, 37, 6), (3, 6, 37, 7), (3, 5, 3, 5), (3, 5, 3, 6)])
def test_dissipation_kernel_bit_exact(gpu, ldim, lx1, E, pad):
    lay = NekLayout(ldim=ldim, lx1=lx1, lx2=lx1 - 2, nelgv=E)
    ctx = _ctx(lay)
    n = ctx.layout.n_v
    rng = np.random.default_rng(3 * ldim + pad)
    re, im, lr, li = (list(rng.standard_normal((ldim, n))) for _ in range(4))
    bm1 = rng.uniform(0.5, 1.5, n)
    nu = 0.02
    stride = n + pad
    dre, dim_, lap, w = _dev(ctx, re, stride), _dev(ctx, im, stride), _dev(ctx, lr + li, stride), _dev(ctx, [bm1], n)
    ref = _dissipation_numpy(re, im, lr, li, nu)
    iref, iscale = float(np.sum(bm1 * ref)), float(np.sum(bm1 * np.abs(ref)))
    integ = torch.full((2,), np.nan, dtype=torch.float64, device=ctx.device)
    for with_field in (True, False):
        diss = torch.full((n + 4,), np.nan, dtype=torch.float64, device=ctx.device)
        ctx.call("nkv_pke_dissipation", dre.data_ptr(), dim_.data_ptr(), stride, lap.data_ptr(), stride, ldim, nu,
                 w.data_ptr(), diss.data_ptr() if with_field else None, integ.data_ptr(), ctx.ws.data_ptr(), ctx.stream)
        got = diss.cpu().numpy()
        if with_field:
            assert np.array_equal(got[:n], ref)
            assert np.all(np.isnan(got[n:]))
        val = float(integ[0].item())
        print(f"dissipation integral err {abs(val - iref) / iscale:.2e} of sum|.|")
        assert abs(val - iref) <= 1e-12 * iscale
    ctx.check_nan()


# ---- the chain ---------------------------------------------------------------------------------

def _write_inputs(tmp, lay, co, session, nmodes=1):
    """BF_ (file 1) and dRe/dIm (files 1..nmodes): smooth fields of the coordinates plus 1e-4 noise,
    written by the oracle's own #std writer (pressure present; the budget ignores it)."""
    g = nekio.Geom(lay.ldim, lay.lx1, lay.lx2, lay.nelgv)
    x, y = co["x"], co["y"]
    z = co.get("z", np.zeros_like(x))
    rng = np.random.default_rng(5)
    nv = lay.n_v
    names = [("BF_", 1)] + [(p, m) for m in range(1, nmodes + 1) for p in ("dRe", "dIm")]
    for k, (prefix, num) in enumerate(names):
        ref = np.zeros(lay.ldim * nv + lay.n_p + 1)
        for c in range(lay.ldim):
            f = np.sin((1.0 + 0.3 * k) * x + 0.5 * c) * np.cos((0.6 + 0.1 * c) * y - 0.2 * k) + 0.1 * (c + 1) * z
            ref[c * nv:(c + 1) * nv] = f + 1e-4 * rng.standard_normal(nv)
        ref[lay.ldim * nv: lay.ldim * nv + lay.n_p] = rng.standard_normal(lay.n_p)
        nekio.write_std(str(tmp / fld.fld_name(prefix, session, 0, num)), g, ref, time=float(num), istep=num)


@functools.lru_cache(maxsize=None)
def _chain_case(case):
    if case == "cyl":
        lay, co = NekLayout(ldim=2, lx1=6, lx2=4, nelgv=1996), _cyl()
    else:
        lay = NekLayout(ldim=3, lx1=6, lx2=4, nelgv=18)
        co = deformed_box(lay, (3, 3, 2))
    return lay, co, ebr.GroupAverage(co)   # the grouping is computed once per mesh


def _ulp7(x):
    """One unit of the seventh digit of an E15.7 record of x."""
    return 0.0 if x == 0 else 10.0 ** (np.floor(np.log10(abs(x))) + 1 - 7)


@pytest.mark.parametrize("normalize", ["reference", "unit", None])
@pytest.mark.parametrize("case", ["cyl", "box"])
def test_energy_budget_chain_vs_restatement(gpu, tmp_path, case, normalize):
    lay, co, avg = _chain_case(case)
    d, nu, ses = lay.ldim, 0.02, "pke"
    _write_inputs(tmp_path, lay, co, ses)
    ctx = _ctx(lay)
    res = stability_energy_budget(ctx, str(tmp_path), co, session=ses, nu=nu, normalize=normalize, write_coords=True)
    assert len(res) == 1                                    # mode 2 has no files: the loop stops
    r = res[0]

    g = nekio.Geom(lay.ldim, lay.lx1, lay.lx2, lay.nelgv)
    nv = lay.n_v

    def load(prefix):
        v = nekio.read_std_vector([str(tmp_path / fld.fld_name(prefix, ses, 0, 1))], g)
        return [v[c * nv:(c + 1) * nv] for c in range(d)]

    w = syn.mass_weights(ctx.layout)                       # bm1s = bm1 here (no sponge)
    base, re, im = load("BF_"), load("dRe"), load("dIm")
    alpha, s = ebr.mode_scale(w, re, im, normalize)
    assert r["alpha"] == pytest.approx(alpha, rel=1e-13)
    re, im = [c * s for c in re], [c * s for c in im]
    F, I, _ = ebr.energy_budget(lay.lx1, d, co, w, base, re, im, nu, average=avg)
    Fl, Il, _ = ebr.energy_budget(lay.lx1, d, co, w, base, re, im, nu, average=avg, dtype=np.longdouble)

    gates = np.zeros(10)
    for c in range(d):
        for k in range(d):
            i = 3 * c + k
            got, ref = r["production"][c][k], F[i]
            scale = np.max(np.abs(ref))
            gates[i] = 1e-12 * float(np.sum(w * np.abs(ref)))
            assert scale > 0 and np.max(np.abs(got - ref)) <= 1e-12 * scale, (c, k)
            assert abs(r["integrals"][i] - I[i]) <= gates[i], (c, k)
    absent = [i for i in range(9) if i // 3 >= d or i % 3 >= d]
    assert not r["integrals"][absent].any()
    # the Laplacian-borne quantities, in units of the restatement's own rounding error
    scale = float(np.max(np.abs(F[9])))
    e_ref = float(np.max(np.abs(F[9] - Fl[9])))
    err = float(np.max(np.abs(r["dissipation"] - F[9])))
    err_ld = float(np.max(np.abs(r["dissipation"] - Fl[9])))
    iscale = float(np.sum(w * np.abs(F[9])))
    ie_ref = float(abs(I[9] - Il[9]))
    ierr = abs(r["integrals"][9] - float(I[9]))
    print(f"{case} normalize={normalize}: dissipation e_ref/scale {e_ref / scale:.2e}, device-f64 {err / scale:.2e}, "
          f"device-longdouble {err_ld / scale:.2e}; integral e_ref/scale {ie_ref / iscale:.2e}, device {ierr / iscale:.2e}")
    assert scale > 0 and e_ref > 0
    assert err <= max(8 * e_ref, 1e-12 * scale)
    gates[9] = max(8 * ie_ref, 1e-12 * iscale)
    assert ierr <= gates[9]

    # K files: velocity (P[c][x], P[c][y][, P[c][z]]) of file c+1, read back by the oracle's reader bit for bit
    kfiles, pke = r["paths"][:d], r["paths"][d]
    assert [p.rsplit("/", 1)[1] for p in kfiles] == [fld.fld_name("K01", ses, 0, c + 1) for c in range(d)]
    for c, path in enumerate(kfiles):
        tok, ids, fields = nekio.read_std(path)
        assert tok[11] == "XU" and float(tok[7]) == 1.0
        assert np.array_equal(ids, np.arange(1, lay.nelgv + 1))
        for k, nm in enumerate(("vx", "vy", "vz")[:d]):
            assert np.array_equal(fields[nm].ravel(), r["production"][c][k])
        assert np.array_equal(fields["x"].ravel(), co["x"])
    # PKE_ text: twelve E15.7 records; equal to the formatted reference integrals wherever the seven
    # digits do not depend on where inside the gate the value lies, else the parsed values agree to the
    # gate plus one unit of the seventh digit (all a 7-digit record can show)
    assert pke.rsplit("/", 1)[1] == f"PKE_dRe{ses}0.f00001"
    lines = open(pke).read().split("\n")
    assert lines[-1] == "" and len(lines) == 13 and all(len(ln) == 15 for ln in lines[:12])
    from nekstab_next_amd.newton import fortran_e

    ref_vals = [float(v) for v in I]
    total = 0.0
    for v in ref_vals[:9]:
        total = total + v
    ref_vals += [total, total - ref_vals[9]]
    rec_gates = list(gates) + [float(np.sum(gates[:9])), float(np.sum(gates))]
    for ln, v, gt in zip(lines, ref_vals, rec_gates):
        if fortran_e(v - gt, 15, 7) == fortran_e(v + gt, 15, 7):
            assert ln == fortran_e(v, 15, 7)
        else:
            assert abs(float(ln) - float(fortran_e(v, 15, 7))) <= gt + _ulp7(v)
    assert r["total"] == pytest.approx(total, abs=rec_gates[10]) and r["balance"] == pytest.approx(ref_vals[11], abs=rec_gates[11])


def test_energy_budget_mode_loop_and_options(gpu, tmp_path):
    """Two modes on disk, maxmodes caps the loop; face_average=None skips dsavg; a scalar-carrying
    context is refused."""
    lay, co, _ = _chain_case("box")
    _write_inputs(tmp_path, lay, co, "m", nmodes=2)
    ctx = _ctx(lay)
    out = tmp_path / "out"
    res = stability_energy_budget(ctx, str(tmp_path), co, session="m", nu=0.02, outdir=str(out))
    assert [len(r["paths"]) for r in res] == [4, 4]
    assert (out / "K02m0.f00003").exists() and (out / "PKE_dRem0.f00002").exists()
    assert len(stability_energy_budget(ctx, str(tmp_path), co, session="m", nu=0.02, maxmodes=1, outdir=str(out))) == 1
    noavg = stability_energy_budget(ctx, str(tmp_path), co, session="m", nu=0.02, maxmodes=1, outdir=str(out),
                                    face_average=None)[0]
    assert np.array_equal(noavg["integrals"][:9], res[0]["integrals"][:9])       # production has no dsavg
    assert noavg["integrals"][9] != res[0]["integrals"][9]
    with pytest.raises(ValueError):
        stability_energy_budget(NekContext(lay, max_cols=4), str(tmp_path), co, session="m")
    with pytest.raises(ValueError):
        stability_energy_budget(ctx, str(tmp_path), co, session="m", normalize="yes")


def test_energy_budget_known_answer_on_device(gpu):
    """Affine box, lx1=5, E=12: a base flow linear in the coordinates and modes quadratic in them make
    every term a known polynomial (production -0.5 (..) A[c][d], Laplacians 2 tr Q)."""
    ne = (2, 2, 3)
    lay = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=12)
    co = box_mesh_coords(lay, ne)
    ctx = _ctx(lay)
    vl = ctx.layout
    re, im, lre, lim = quadratic_modes(co)
    base = [A_BASE[c, 0] * co["x"] + A_BASE[c, 1] * co["y"] + A_BASE[c, 2] * co["z"] + 0.5 for c in range(3)]

    def vec(comps):
        host = np.zeros(vl.ld)
        for c in range(3):
            host[c * vl.sv: c * vl.sv + vl.n_v] = comps[c]
        return ctx.vector().from_packed(host)

    nu = 0.02
    bm1 = syn.mass_weights(vl)
    prod, diss, integ = energy_budget_fields(ctx, vec(base), vec(re), vec(im), Gradm1(ctx, co),
                                             FaceAverage(ctx, co).apply, nu)
    ctx.check_nan()
    P = prod.view(3, 3, vl.sv)[:, :, : vl.n_v].cpu().numpy()
    integ = integ.cpu().numpy()
    for c in range(3):
        for d in range(3):
            want = -0.5 * (re[c] * re[d] + im[d] * im[c]) * A_BASE[c, d]
            np.testing.assert_allclose(P[c, d], want, rtol=0, atol=1e-8)
            assert abs(integ[3 * c + d] - np.sum(bm1 * want)) <= 1e-8 * np.sum(bm1 * np.abs(want))
    want = 0.5 * nu * sum(re[c] * lre[c] + im[c] * lim[c] for c in range(3))
    np.testing.assert_allclose(diss[: vl.n_v].cpu().numpy(), want, rtol=0, atol=1e-8)
    assert abs(integ[9] - np.sum(bm1 * want)) <= 1e-8 * np.sum(bm1 * np.abs(want))
    assert not diss[vl.n_v:].any()


# ---- argument checks ---------------------------------------------------------------------------

def test_energy_budget_argument_checks(gpu):
    lay = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=2)
    ctx = _ctx(lay)
    co = box_mesh_coords(lay, (2, 1, 1))
    op = Gradm1(ctx, co)
    n = ctx.layout.n_v
    z = lambda k: torch.zeros(k * n, dtype=torch.float64, device=ctx.device)  # noqa: E731
    u, re, im, bm1, prod, lap, g, out = z(3), z(3), z(3), z(1), z(9), z(6), z(18), z(6)
    integ = torch.full((10,), np.nan, dtype=torch.float64, device=ctx.device)
    lib, ws = ctx.lib, ctx.ws.data_ptr()
    P = dict(L=ctx._Lp, lx1=5, ldim=3, D=op.D.data_ptr(), xm=op.xyz[0].data_ptr(), ym=op.xyz[1].data_ptr(),
             zm=op.xyz[2].data_ptr(), ubase=u.data_ptr(), b_stride=n, dRe=re.data_ptr(), dIm=im.data_ptr(), m_stride=n,
             bm1=bm1.data_ptr(), prod=prod.data_ptr(), p_stride=n, integrals_dev=integ.data_ptr(), ws=ws,
             stream=ctx.stream)

    def bad(fn, args, word, **kw):
        rc = fn(*{**args, **kw}.values())
        assert rc == _lib.NKV_EINVAL, (kw, rc)
        assert word in _lib.last_error(), (kw, _lib.last_error())

    fn = lib.nkv_pke_production
    assert fn(*P.values()) == _lib.NKV_OK
    assert fn(*{**P, "prod": None}.values()) == _lib.NKV_OK
    bad(fn, P, "ldim", ldim=4)
    bad(fn, P, "lx1", lx1=11)
    bad(fn, P, "lx1", lx1=1)
    bad(fn, P, "n_v", lx1=6)                                 # 216 points per element do not divide n_v
    bad(fn, P, "zm", zm=None)
    bad(fn, P, "zm", ldim=2)                                 # 25 points divide n_v, but zm is given
    for s in ("b_stride", "m_stride", "p_stride"):
        bad(fn, P, s, **{s: n - 1})
    for p in ("D", "xm", "ym", "ubase", "dRe", "dIm", "bm1", "integrals_dev", "ws"):
        bad(fn, P, p, **{p: None})

    V = dict(L=ctx._Lp, lx1=5, ldim=3, D=P["D"], xm=P["xm"], ym=P["ym"], zm=P["zm"], g=g.data_ptr(), nvec=6,
             g_stride=n, div=out.data_ptr(), d_stride=n, stream=ctx.stream)
    fn = lib.nkv_divm1
    assert fn(*V.values()) == _lib.NKV_OK
    bad(fn, V, "ldim", ldim=1)
    bad(fn, V, "lx1", lx1=12)
    bad(fn, V, "n_v", lx1=4)
    bad(fn, V, "zm", zm=None)
    bad(fn, V, "nvec", nvec=0)
    for s in ("g_stride", "d_stride"):
        bad(fn, V, s, **{s: n - 1})
    for p in ("D", "xm", "ym", "g", "div"):
        bad(fn, V, p, **{p: None})

    S = dict(L=ctx._Lp, dRe=re.data_ptr(), dIm=im.data_ptr(), m_stride=n, lap=lap.data_ptr(), l_stride=n, ncomp=3,
             nu=0.02, bm1=bm1.data_ptr(), diss=out.data_ptr(), integral_dev=integ.data_ptr(), ws=ws, stream=ctx.stream)
    fn = lib.nkv_pke_dissipation
    assert fn(*S.values()) == _lib.NKV_OK
    assert fn(*{**S, "diss": None}.values()) == _lib.NKV_OK
    bad(fn, S, "ncomp", ncomp=4)
    bad(fn, S, "ncomp", ncomp=1)
    for s in ("m_stride", "l_stride"):
        bad(fn, S, s, **{s: n - 1})
    for p in ("dRe", "dIm", "lap", "bm1", "integral_dev", "ws"):
        bad(fn, S, p, **{p: None})

    # an empty shard: NKV_OK, zeros into the integrals, no other pointer read
    E = ctx.layout.c_struct()
    E.n_v = 0
    integ.fill_(float("nan"))
    none = {k: None for k in ("D", "xm", "ym", "zm", "ubase", "dRe", "dIm", "bm1", "prod")}
    assert lib.nkv_pke_production(*{**P, **none, "L": E}.values()) == _lib.NKV_OK
    assert lib.nkv_pke_dissipation(*{**S, "L": E, "dRe": None, "dIm": None, "lap": None, "bm1": None, "diss": None,
                                     "integral_dev": integ.data_ptr() + 8 * 9}.values()) == _lib.NKV_OK
    assert lib.nkv_divm1(*{**V, "L": E, "g": None, "div": None}.values()) == _lib.NKV_OK
    assert torch.equal(integ, torch.zeros_like(integ))
    ctx.check_nan()
