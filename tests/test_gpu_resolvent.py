"""The time-stepper resolvent on the device (nkv_advdiff_cstage in csrc/advdiff.hip, nekstab_next_amd/resolvent.py)
against its NumPy restatement (tests/resolvent_reference.py) and the dense (i omega - L)^-1.

The fused stage is compared bit for bit with the NumPy expression of its header comment.  Runs of the stepper
are held to the project's gate for everything differentiated twice (tests/test_gpu_advdiff.py: ``_gate``,
max(8 e_ref, 1e-12 scale) with e_ref the distance of the f64 from the long double restatement).  The operator is
held to the dense solve: 4 times the distance of the f64 restatement of the same algorithm from that solve
(resolvent_reference.DENSE_DISTANCE, measured by tests/test_resolvent.py), with 1e-11 relative as the floor."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import advdiff_reference as ar
import resolvent_reference as rr
from test_gpu_advdiff import _free_port, _gate, _mesh

from nekstab_next_amd import _lib
from nekstab_next_amd.layout import NekLayout, pair_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

BOX3D = (5, (2, 2, 2))
SHAPES = ["cell", "odd", BOX3D]


# ---- cases -------------------------------------------------------------------------------------------
def _case(name):
    """(global layout, coordinates, base flow, wall mask, kappas, dt, nsteps) of a named case."""
    if name in rr.CASES:
        c = rr.CASES[name]
        lay = NekLayout(ldim=2, lx1=c["lx1"], lx2=max(c["lx1"] - 2, 1), nelgv=9)
        return (lay,) + rr.cell_mesh(c["lx1"]) + (c["kappa"], c["dt"], c["nsteps"])
    # 3-D with a scalar (n_wf = 4): rho(L) = 43.6 at kappa = 0.05, so dt (rho + omega) = 1.8 at dt = 0.04
    return _mesh(name) + ((0.05, 0.04, 0.03, 0.02), 0.04, 4)


_REFS, _ADVS = {}, {}


def _refs(name):
    if name not in _REFS:
        lay, co, U, mask = _case(name)[:4]
        _REFS[name] = tuple(ar.Reference(lay.lx1, lay.ldim, co, U, mask=mask, dtype=t) for t in (np.float64, np.longdouble))
    return _REFS[name]


def _adv(name, batched=False):
    """(AdvectionDiffusion, pair context) of a case on one rank, built once.  ``batched``: the averages go
    through a one-rank GatherScatter (one launch for the 2 n_wf segments of a pass) instead of "auto"."""
    if (name, batched) not in _ADVS:
        from nekstab_next_amd.advdiff import AdvectionDiffusion
        from nekstab_next_amd.gs import GatherScatter
        from nekstab_next_amd.resolvent import pair_context
        from nekstab_next_amd.vector import NekContext

        lay, co, U, mask, kap, dt, nsteps = _case(name)
        ctx = NekContext(lay, max_cols=4)
        adv = AdvectionDiffusion(ctx, co, U, kap, dt, nsteps, mask=mask,
                                 face_average=GatherScatter(ctx, co) if batched else "auto")
        _ADVS[(name, batched)] = (adv, pair_context(adv))
    return _ADVS[(name, batched)]


def _upload(pctx, z, pressure=0.0, time=0.0, fill=0.0):
    """A pair vector from complex fields (n_wf, n_v of the base shard); the rest of the storage is ``fill``."""
    p, n = pctx.layout, pctx.layout.n_v // 2
    host = np.full(p.ld, fill)
    for f in range(p.n_wf):
        host[f * p.sv: f * p.sv + n] = z[f].real
        host[f * p.sv + n: f * p.sv + 2 * n] = z[f].imag
    host[p.n_wf * p.sv: p.n_wf * p.sv + p.n_p] = pressure
    host[p.time_offset] = time
    return pctx.vector().from_packed(host)


def _download(pctx, v):
    p, n = pctx.layout, pctx.layout.n_v // 2
    host = v.to_packed()
    return np.stack([host[f * p.sv: f * p.sv + n] + 1j * host[f * p.sv + n: f * p.sv + 2 * n] for f in range(p.n_wf)])


def _check_rest(p, packed, value=7.0):
    """Pressure rows and time are zero; every padding row still holds the sentinel."""
    for f in range(p.n_wf):
        assert np.all(packed[f * p.sv + p.n_v:(f + 1) * p.sv] == value)
    p0 = p.n_wf * p.sv
    assert np.all(packed[p0:p0 + p.n_p] == 0.0) and p.n_p > 0
    assert np.all(packed[p0 + p.n_p:p.time_offset] == value)
    assert packed[p.time_offset] == 0.0 and np.all(packed[p.time_offset + 1:] == value)


def _check_zeroed(p, packed):
    p0 = p.n_wf * p.sv
    assert p.n_p > 0 and np.all(packed[p0:p0 + p.n_p] == 0.0) and packed[p.time_offset] == 0.0


def _random_complex(nf, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))


def _gate_complex(got, a, b, what):
    for f in range(got.shape[0]):
        _gate(got[f].real, a[f].real, np.asarray(b[f].real), f"{what} field {f} re")
        _gate(got[f].imag, a[f].imag, np.asarray(b[f].imag), f"{what} field {f} im")


# ---- nkv_advdiff_cstage ------------------------------------------------------------------------------
SV, NF, NP = 4096, 2, 10


def _stage_layout(n):
    return _lib.nkv_layout(n_v=2 * n, n_p=NP, sv=SV, sp=SV, ld=4 * SV, n_wf=NF, rank0=1)


def _expected(m, r, s, f, v, om, c):
    """The header's expression on (NF, n) complex arrays, one rounding per operation."""
    g_re = m * r.real + om * s.imag
    g_im = m * r.imag - om * s.real
    if f is not None:
        g_re, g_im = g_re + f.real, g_im + f.imag
    t_re, t_im = c * g_re, c * g_im
    return (t_re, t_im) if v is None else (v.real + t_re, v.imag + t_im)


class _Operand:
    """NF complex fields on the device in one of three arrangements: "pair" (im = re + n, stride SV: a pair
    vector's), "split" (both halves 16-byte aligned, even stride: the 16-byte path for any n >= 2) and "shifted"
    (split, every pointer moved by one double, odd stride: the scalar path)."""

    def __init__(self, z, n, how, fill=7.0):
        self.n, self.how = n, how
        self.stride = {"pair": SV, "split": 2 * ((n + 3) // 2) + 2, "shifted": 2 * ((n + 3) // 2) + 3}[how]
        self.off_re = 1 if how == "shifted" else 0
        self.off_im = self.off_re + (n if how == "pair" else NF * self.stride + 2)
        size = 4 * SV if how == "pair" else self.off_im + NF * self.stride + 2
        host = np.full(size, fill)
        if z is not None:
            for f in range(NF):
                host[self.off_re + f * self.stride: self.off_re + f * self.stride + n] = z[f].real
                host[self.off_im + f * self.stride: self.off_im + f * self.stride + n] = z[f].imag
        self.t = torch.as_tensor(host).to("cuda")

    @property
    def re(self):
        return self.t.data_ptr() + 8 * self.off_re

    @property
    def im(self):
        return self.t.data_ptr() + 8 * self.off_im

    def get(self):
        host = self.t.cpu().numpy()
        re = np.stack([host[self.off_re + f * self.stride: self.off_re + f * self.stride + self.n] for f in range(NF)])
        im = np.stack([host[self.off_im + f * self.stride: self.off_im + f * self.stride + self.n] for f in range(NF)])
        return re, im

    def untouched_outside(self, fill=7.0, zeroed=False):
        """Everything but the NF x 2 live segments still holds ``fill`` (``zeroed``: but the pressure rows and time)."""
        host = self.t.cpu().numpy().copy()
        for f in range(NF):
            host[self.off_re + f * self.stride: self.off_re + f * self.stride + self.n] = fill
            host[self.off_im + f * self.stride: self.off_im + f * self.stride + self.n] = fill
        if zeroed:
            assert np.all(host[NF * SV: NF * SV + NP] == 0.0) and host[NF * SV + SV] == 0.0
            host[NF * SV: NF * SV + NP] = fill
            host[NF * SV + SV] = fill
        return bool(np.all(host == fill))


def _cstage(L, v, m, r, s, f, om, c, w, zero_rest=0):
    lib = _lib.load()
    none = (None, None, 0)
    return lib.nkv_advdiff_cstage(ctypes.byref(L), *((v.re, v.im, v.stride) if v else none), m.data_ptr(), r.re, r.im,
                                  r.stride, s.re, s.im, s.stride, *((f.re, f.im, f.stride) if f else none), om, c, w.re, w.im,
                                  w.stride, NF, zero_rest, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("n", [1, 81, 324])
def test_cstage_bits(gpu, n):
    """Every combination of v / f present or NULL, omega of both signs and zero, w aliasing v, in the three
    arrangements (so the 16-byte and the scalar path at every n >= 2): the bits of the NumPy expression; in the
    pair arrangement with zero_rest the pressure rows and the time slot are zeroed; nothing else is written."""
    L = _stage_layout(n)
    rng = np.random.default_rng(n)
    m_h = rng.uniform(0.5, 2.0, n)
    m_h[::5] = 0.0                                                   # masked points
    z = {k: _random_complex(NF, n, 10 * n + i) for i, k in enumerate("rsfv")}
    c = 0.06 / 3.0
    for how in ("pair", "split", "shifted"):
        mt = torch.as_tensor(np.concatenate([[7.0], m_h, [7.0]])).to("cuda")
        m = mt[1:] if how == "shifted" else mt[1:].clone()
        assert (m.data_ptr() % 16 != 0) == (how == "shifted")
        r, s, f = (_Operand(z[k], n, how) for k in "rsf")
        zr = int(how == "pair")
        for om in (-0.7, 0.0, 1.3):
            for has_v in (False, True):
                for has_f in (False, True):
                    for alias in ((False, True) if has_v else (False,)):
                        v = _Operand(z["v"], n, how) if has_v else None
                        w = v if alias else _Operand(None, n, how)
                        rc = _cstage(L, v, m, r, s, f if has_f else None, om, c, w, zero_rest=zr)
                        assert rc == _lib.NKV_OK, _lib.last_error()
                        want = _expected(m_h, z["r"], z["s"], z["f"] if has_f else None, z["v"] if has_v else None, om, c)
                        got = w.get()
                        what = (how, om, has_v, has_f, alias)
                        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
                        assert w.untouched_outside(zeroed=bool(zr)), what
                        if has_v and not alias:
                            assert np.array_equal(v.get()[0], z["v"].real) and v.untouched_outside(), what
        for o, k in ((r, "r"), (s, "s"), (f, "f")):                 # the inputs are read only
            assert np.array_equal(o.get()[0], z[k].real) and np.array_equal(o.get()[1], z[k].imag) and o.untouched_outside()


def test_cstage_entry_checks(gpu):
    """An empty shard returns NKV_OK and touches nothing; bad arguments return NKV_EINVAL with a message and
    launch nothing."""
    n = 81
    L = _stage_layout(n)
    z = _random_complex(NF, n, 3)
    m = torch.ones(n + 2, dtype=torch.float64, device="cuda")
    r, s, f, v, w = (_Operand(z, n, "pair") for _ in range(5))
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    V = dict(L=ctypes.byref(L), v_re=v.re, v_im=v.im, v_stride=SV, minv=m.data_ptr(), r_re=r.re, r_im=r.im, r_stride=SV,
             s_re=s.re, s_im=s.im, s_stride=SV, f_re=f.re, f_im=f.im, f_stride=SV, omega=1.0, c=0.5, w_re=w.re, w_im=w.im,
             w_stride=SV, nfld=NF, zero_rest=1, stream=st)
    Lodd = _lib.nkv_layout(n_v=2 * n + 1, n_p=NP, sv=SV, sp=SV, ld=4 * SV, n_wf=NF, rank0=1)
    bad = [("L", ctypes.byref(Lodd), "odd"), ("v_im", None, "v_re and v_im"), ("f_re", None, "f_re and f_im"),
           ("v_stride", n - 1, "stride"), ("r_stride", n - 1, "stride"), ("s_stride", 0, "stride"),
           ("f_stride", n - 1, "stride"), ("w_stride", n - 1, "stride"), ("minv", None, "minv is NULL"),
           ("r_re", None, "r_re is NULL"), ("r_im", None, "r_im is NULL"), ("s_re", None, "s_re is NULL"),
           ("s_im", None, "s_im is NULL"), ("w_re", None, "w_re is NULL"), ("w_im", None, "w_im is NULL"),
           ("nfld", 0, "nfld"), ("c", float("nan"), "c="), ("omega", float("inf"), "omega="),
           ("w_re", s.re, "overlaps"), ("w_im", r.im, "overlaps"), ("w_re", f.re, "overlaps"),
           ("w_im", w.re + 8 * (n - 1), "halves of w overlap"), ("nfld", 1, "zero_rest"),
           ("w_im", w.im + 16, "zero_rest")]
    for key, val, msg in bad:
        assert lib.nkv_advdiff_cstage(*{**V, key: val}.values()) == _lib.NKV_EINVAL, key
        assert msg in _lib.last_error(), (key, _lib.last_error())
    assert lib.nkv_advdiff_cstage(*{**V, "w_stride": SV - 2, "zero_rest": 1}.values()) == _lib.NKV_EINVAL
    E = _stage_layout(0)
    args = {**V, "L": ctypes.byref(E), "minv": None, "r_re": None, "s_im": None, "w_re": None, "w_im": None}
    assert lib.nkv_advdiff_cstage(*args.values()) == _lib.NKV_OK
    torch.cuda.synchronize()
    for o in (r, s, f, v, w):
        assert np.array_equal(o.get()[0], z.real) and np.array_equal(o.get()[1], z.imag) and o.untouched_outside()


# ---- the stepper against the restatement -------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES, ids=str)
def test_runs_against_restatement(gpu, name):
    """project, forced_run and propagate, direct and adjoint, at omega = 1 (0 on the 3-D case) against the
    restatement in f64 and long double; pressure rows and time zeroed, padding untouched; deterministic."""
    from nekstab_next_amd.resolvent import ResolventOperator

    adv, pctx = _adv(name)
    lay, _, _, _, kap, dt, nsteps = _case(name)
    omega = 0.0 if name == BOX3D else 1.0
    op = ResolventOperator(pctx, adv, omega)
    r64, rld = (rr.Resolvent(r, kap, dt, nsteps, omega) for r in _refs(name))
    assert abs(op.tau - nsteps * dt) <= 1e-15 * op.tau
    x = _upload(pctx, _random_complex(lay.n_wf, lay.n_v, 7), pressure=1.0, time=3.0)
    xz = _download(pctx, x)
    f = _upload(pctx, 0 * xz, pressure=7.0, time=7.0, fill=7.0)
    op.project(x, f)
    _check_rest(pctx.layout, f.to_packed())
    fz = _download(pctx, f)
    _gate_complex(fz, r64.project(xz), rld.project(xz), f"{name} project")
    inplace = pctx.vector()
    inplace.copy_from(x)
    op.project(inplace)
    assert np.array_equal(_download(pctx, inplace), fz)
    for adjoint in (False, True):
        b = _upload(pctx, 0 * xz, pressure=7.0, time=7.0)
        op.forced_run(f, b, adjoint)
        _check_zeroed(pctx.layout, b.to_packed())
        _gate_complex(_download(pctx, b), r64.forced_run(fz, adjoint), rld.forced_run(fz, adjoint),
                      f"{name} forced_run adjoint={adjoint}")
        y = _upload(pctx, 0 * xz, pressure=7.0, time=7.0)
        op.propagate(x, y, adjoint)                                  # pressure 1, time 3 in x
        _check_zeroed(pctx.layout, y.to_packed())
        op.propagate(f, y, adjoint)
        got = _download(pctx, y)
        _gate_complex(got, r64.propagate(fz, adjoint), rld.propagate(fz, adjoint), f"{name} propagate adjoint={adjoint}")
        y2 = pctx.vector()
        y2.copy_from(f)
        op.propagate(y2, y2, adjoint)                                # in place
        assert np.array_equal(_download(pctx, y2), got)
        assert np.array_equal(_download(pctx, f), fz)               # the forcing is read only
    with pytest.raises(ValueError):
        op.forced_run(f, f)


# ---- the operator against the dense inverse ------------------------------------------------------------
@pytest.mark.parametrize("name,omega", [("cell", 0.0), ("cell", 1.0), ("odd", 0.0), ("odd", 1.0)], ids=str)
def test_operator_against_dense_inverse(gpu, name, omega):
    """matvec / rmatvec at inner tol = 1e-13 against the dense (±i omega - L)^-1 Pi f of random unprojected f, g
    (gate: module docstring), and <R f, g> = <f, R† g> in the pair bm1 product of the context, held to 4 times the
    restatement's defect (resolvent_reference.ADJOINT_DEFECT)."""
    from nekstab_next_amd.resolvent import ResolventOperator

    adv, pctx = _adv(name)
    lay, _, _, _, kap, dt, nsteps = _case(name)
    op = ResolventOperator(pctx, adv, omega, tol=1e-13)
    dense = rr.Resolvent(_refs(name)[0], kap, dt, nsteps, omega)
    gate = max(4 * rr.DENSE_DISTANCE, 1e-11)
    fz, gz = _random_complex(lay.n_wf, lay.n_v, 4), _random_complex(lay.n_wf, lay.n_v, 5)
    f, g = _upload(pctx, fz, pressure=1.0, time=2.0), _upload(pctx, gz)
    y, ya = _upload(pctx, 0 * fz, pressure=7.0, time=7.0), pctx.vector()
    op.matvec(f, y)
    info = op.last_gmres
    assert info["info"] == 0 and info["adjoint"] is False and info["residuals"][-1] <= 1e-13 * info["residuals"][0]
    _check_zeroed(pctx.layout, y.to_packed())
    op.rmatvec(g, ya)
    assert op.last_gmres["info"] == 0 and op.last_gmres["adjoint"] is True
    for got, want, what in ((_download(pctx, y), dense.dense_apply(fz), "matvec"),
                            (_download(pctx, ya), dense.dense_apply(gz, adjoint=True), "rmatvec")):
        d = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f"{name} omega {omega} {what}: distance from the dense solve {d:.2e} (gate {gate:.1e}), "
              f"{len(op.last_gmres['residuals'])} residuals")
        assert np.max(np.abs(want)) > 0 and d <= gate, (what, d)
    lhs, rhs = pctx.dot(y, g, time=False), pctx.dot(f, ya, time=False)
    yz = _download(pctx, y)
    scale = float(np.sum(adv.bm1.cpu().numpy() * (np.abs(yz.real * gz.real) + np.abs(yz.imag * gz.imag))))
    print(f"{name} omega {omega} adjoint identity: {abs(lhs - rhs) / scale:.2e} (gate {4 * rr.ADJOINT_DEFECT:.1e})")
    assert scale > 0 and abs(lhs - rhs) <= 4 * rr.ADJOINT_DEFECT * scale


def test_resolvent_analysis_on_the_stepper(gpu, tmp_path):
    """drivers.resolvent_analysis, unchanged, on "cell" at omega = 1 with inner tol = 1e-13: the two leading
    distinct gains within 1e-10 relative of the dense weighted SVD (the project's parity gate), each twice, and
    Spectrum_Sr.dat written.  k_dim = 32: a bidiagonalisation of the dense operator with 1e-13 noise in every
    product has all four values converged by k = 28.  The 64 inner solves are some 1.3 million launches, so the
    averages are batched here (a one-rank GatherScatter); the other tests run "auto"."""
    from nekstab_next_amd.drivers import resolvent_analysis
    from nekstab_next_amd.resolvent import ResolventOperator

    adv, pctx = _adv("cell", batched=True)
    lay, _, _, _, kap, dt, nsteps = _case("cell")
    op = ResolventOperator(pctx, adv, 1.0, tol=1e-13)
    gains = rr.Resolvent(_refs("cell")[0], kap, dt, nsteps, 1.0).gains()
    seed = pctx.vector()
    seed.fill_hash(17)
    out = resolvent_analysis(pctx, op, seed, k_dim=32, nev=4, tolerance=1e-9, outdir=str(tmp_path))
    exact = np.repeat(gains[:2], 2)
    print("gains", out["sigma2"][:4], "dense", exact, "residuals", out["residuals"][:4])
    assert gains[1] < gains[0] * (1 - 1e-3)                          # two distinct values
    assert out["info"] == 0
    np.testing.assert_allclose(out["sigma2"][:4], exact, rtol=1e-10)
    data = np.loadtxt(tmp_path / "Spectrum_Sr.dat")
    assert data.shape == (32, 2)
    np.testing.assert_allclose(data[:4, 0], exact, rtol=1e-6)


def test_refusals(gpu):
    """A non-converged inner solve raises; contexts with other weights or another layout, and bad solver
    parameters, are refused."""
    from nekstab_next_amd.advdiff import AdvectionDiffusion
    from nekstab_next_amd.resolvent import ResolventOperator, pair_context
    from nekstab_next_amd.vector import NekContext

    adv, pctx = _adv("odd")
    lay = adv.ctx.layout
    op = ResolventOperator(pctx, adv, 1.0, tol=1e-13, kdim=2, maxiter=1)
    f, y = _upload(pctx, _random_complex(lay.n_wf, lay.n_v, 1)), pctx.vector()
    with pytest.raises(RuntimeError, match="did not converge"):
        op.matvec(f, y)
    assert op.last_gmres["info"] == 1 and len(op.last_gmres["residuals"]) >= 2
    with pytest.raises(ValueError, match="weights"):
        ResolventOperator(NekContext(pair_layout(lay), max_cols=64), adv, 1.0)
    with pytest.raises(ValueError, match="pair_layout"):
        ResolventOperator(NekContext(lay, weights=adv.bm1, max_cols=64), adv, 1.0)
    other = pair_layout(NekLayout(ldim=2, lx1=3, lx2=1, nelgv=10))
    with pytest.raises(ValueError, match="pair_layout"):
        ResolventOperator(NekContext(other, max_cols=64), adv, 1.0)
    with pytest.raises(ValueError, match="kdim"):
        ResolventOperator(pair_context(adv, max_cols=8), adv, 1.0, kdim=9)
    for kw in (dict(tol=0.0), dict(maxiter=0), dict(omega=float("nan"))):
        with pytest.raises(ValueError):
            ResolventOperator(pctx, adv, **{"omega": 1.0, **kw})
    for dt, nsteps in ((0.0, 4), (-0.1, 4), (0.1, 0)):
        with pytest.raises(ValueError, match="dt"):
            AdvectionDiffusion(adv.ctx, *_case("odd")[1:3], 0.05, dt, nsteps)
        broken = copy.copy(adv)                                      # the operator looks again: adv is mutable
        broken.dt, broken.nsteps = dt, nsteps
        with pytest.raises(ValueError, match="dt"):
            ResolventOperator(pctx, broken, 1.0)


# ---- shards ------------------------------------------------------------------------------------------
def _jobs(rank, world):
    """forced_run of the projected forcing and matvec (inner tol 1e-10) on "cell", this rank's slice."""
    from nekstab_next_amd.advdiff import AdvectionDiffusion
    from nekstab_next_amd.comm import Comm
    from nekstab_next_amd.resolvent import ResolventOperator, pair_context
    from nekstab_next_amd.vector import NekContext

    comm = Comm()
    assert comm.world == world and comm.rank == rank
    lay_g, co_g, U_g, mask_g, kap, dt, nsteps = _case("cell")
    ctx = NekContext(lay_g, comm=comm, max_cols=4)
    lay = ctx.layout
    e0, e1 = lay.elem_range()
    sl = slice(e0 * lay.pts_v, e1 * lay.pts_v)
    adv = AdvectionDiffusion(ctx, {k: v[sl] for k, v in co_g.items()}, [u[sl] for u in U_g], kap, dt, nsteps,
                             mask=mask_g[sl])
    pctx = pair_context(adv)
    op = ResolventOperator(pctx, adv, 1.0, tol=1e-10)
    x = _upload(pctx, _random_complex(lay_g.n_wf, lay_g.n_v, 9)[:, sl])
    f, b, y = pctx.vector(), pctx.vector(), pctx.vector()
    op.project(x, f)
    op.forced_run(f, b)
    op.matvec(x, y)
    return {"b": _download(pctx, b), "y": _download(pctx, y), "residuals": op.last_gmres["residuals"]}


def _rank_main(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        out[rank] = _jobs(rank, world)
    finally:
        dist.destroy_process_group()


def test_shards_equal_one_rank(gpu):
    """Two gloo ranks sharing the GPU: forced_run equals the one-rank result bit for bit on every rank's slice;
    matvec to 100 times the inner tolerance (the dots of the inner GMRES reduce in another grouping)."""
    one = _jobs(0, 1)
    out = mp.Manager().dict()
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join()
    assert [p.exitcode for p in procs] == [0, 0]
    got = dict(out)
    lay_g = _case("cell")[0]
    scale = float(np.max(np.abs(one["y"])))
    assert scale > 0 and np.all(np.isfinite(one["y"])) and np.any(one["b"] != 0)
    for r in range(2):
        sh = lay_g.shard(r, 2)
        e0, e1 = sh.elem_range()
        sl = slice(e0 * sh.pts_v, e1 * sh.pts_v)
        np.testing.assert_array_equal(got[r]["b"], one["b"][:, sl], err_msg=f"forced_run rank {r}")
        d = float(np.max(np.abs(got[r]["y"] - one["y"][:, sl]))) / scale
        print(f"rank {r}: matvec differs from one rank by {d:.2e}")
        assert d <= 100 * 1e-10
