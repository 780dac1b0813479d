"""GPU parity of the monitors layer (``nkv_torque``, ``nkv_avg_step``; nekstab_next_amd/monitors.py) against
the NumPy restatement (tests/monitors_reference.py).

Torque gates (cases of ``monitors_reference.CASE_NAMES``: the cylinder, a 2-D box with faces 1-4, one 3-D
element with its six faces at lx1 = 2, 3, 4, 8, 10, the deformed (2, 3, 2) box at lx1 = 5, 6 with its boundary
split into two objects from a shuffled member list, a corner element carrying three member faces):

1. ``sij_out`` is bit-identical to G_ij + G_ji of ``nkv_gradm1``'s own output at the face points.
2. ``na_out`` is bit-identical to the restatement (cofactors of k_gradm1 times the GLL face weight).
3. The per-face partials are bit-identical to the restatement's sums of the same integrands: the kernel adds
   a face's terms one by one in ascending face point, which the restatement reproduces (gate 0).
4. The object rows are bit-identical to the restatement of the second stage's order (lane m mod 64, then
   the butterfly) on the device's per-face partials.
5. Row 0 is the object rows added in ascending order.
6. The independent route: max|dev - ref_ld| <= TORQUE_GATE max|ref64 - ref_ld| per case, ref_ld the long-double
   reference, ref64 the float64 route over ``oracle.gradm1``; TORQUE_GATE = 4 x 1.64, the ratio the float64
   restatement itself shows on these cases (measured on the host: 1.631, tests/test_monitors.py).
7. Known answers on the device: the cylinder (p = 1, p = x, u = A x) and sum nA = 0 on closed 3-D surfaces.
8. Shards (w = 2, 3, a shard owning no member, an empty shard): per-face partials bit-identical to the
   one-rank run, the shard's result the fixed-order sum of its partials.
9. The ``pm1`` path: equal to the mesh-2 path on an lx1 == lx2 layout; with lx2 = lx1 - 2 equal to the host's
   ``map_pressure_to_mesh1`` to lx2 ldim eps sum|I||p| per face point.
10. Hygiene: NaN-filled padding untouched, every argument check is NKV_EINVAL, nu as scalar and as field agree.
11. ``TorqueMonitor`` inside ``SFD(monitors=...)`` writes the expected lines.

Statistics gates: avg, rms and the cross moments bit-identical to the restatement over 8 irregular steps with a
dump in the middle, NaN padding preserved, shards bit-identical to the unsharded run, the aliasing check,
and the four files read back through ``fld``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import monitors_reference as mr
from test_monitors import TORQUE_GATE

from nekstab_next_amd import _lib, fixedp, fld
from nekstab_next_amd import monitors as mon
from nekstab_next_amd.layout import NekLayout
from nekstab_next_amd.sensitivity import gll_derivative
from nekstab_next_amd.synthetic import gll_weights
from nekstab_next_amd.vector import NekContext

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
SCALE = 2.0


class _ShardComm:
    """Stand-in for comm.Comm of rank r of `world`, run one rank after the other: the all-reduce leaves the
    local partial in place."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world

    def allreduce_(self, t):
        return t

    def raise_if_any(self, err):
        if err is not None:
            raise err

    def barrier(self):
        pass


class _Setup:
    """One case on the device (rank `rank` of `world`): context, state vector, Torque."""

    def __init__(self, name, rank=0, world=1, lay=None):
        glob, co, objects, _ = mr.case(name)
        glob = glob if lay is None else lay
        vel, p2, nu = mr.fields(glob, co)
        self.glob, self.objects = glob, objects
        lay = glob.shard(rank, world)
        e0, e1 = lay.elem_range()
        sl = slice(e0 * lay.pts_v, e1 * lay.pts_v)
        self.ctx = NekContext(lay, comm=_ShardComm(rank, world) if world > 1 else None, max_cols=4)
        self.lay = lay = self.ctx.layout
        self.co = {k: np.asarray(a)[sl] for k, a in co.items()}
        self.vel, self.p2, self.nu = [v[sl] for v in vel], p2[e0:e1], nu[sl]
        f = {nm: self.vel[c] for c, nm in enumerate(("vx", "vy", "vz")[: lay.ldim])}
        f["pr"] = self.p2.reshape(-1)[: lay.n_p]
        self.vec = self.ctx.vector().from_fields(f)
        self.tq = mon.Torque(self.ctx, self.co, objects)
        self.table = [tuple(int(a) for a in r) for r in self.tq.faces]
        self.keys = [(e + e0, fc, o) for e, fc, o in self.table]

    def compute(self, **kw):
        kw.setdefault("x0", mr.X0)
        kw.setdefault("dp_mean", mr.DP_MEAN)
        kw.setdefault("scale", SCALE)
        vals = self.tq.compute(self.vec, kw.pop("visc", self.nu), distributions=True, **kw)   # nu: a field
        torch.cuda.synchronize()
        nf = self.tq.nfaces
        return dict(vals=vals.reshape(-1, 12), dgtq=self.tq.dgtq.cpu().numpy()[:nf].copy(),
                    out=self.tq.out.cpu().numpy().copy(), sij=self.tq.sij.cpu().numpy()[:nf].copy(),
                    na=self.tq.na.cpu().numpy()[:nf].copy())

    def gradient(self):
        lay, n = self.lay, self.lay.n_v
        g = torch.zeros((lay.ldim * lay.ldim, max(n, 1)), dtype=torch.float64, device=self.ctx.device)
        self.tq.grad_op(self.vec.ptr, g.data_ptr(), nfld=lay.ldim, u_stride=lay.sv, g_stride=max(n, 1))
        a = g.cpu().numpy()[:, :n].reshape(lay.ldim, lay.ldim, lay.nelv, -1)
        return [[a[c, d] for d in range(lay.ldim)] for c in range(lay.ldim)]

    def restate_terms(self, sij, na, nu=None):
        """The restatement's per-face partials from the device's own sij and nA."""
        lay = self.lay
        nu = self.nu if nu is None else nu
        n, d, nel = lay.lx1, lay.ldim, lay.nelv
        Ip = fld.interp_matrix(fld.gauss_points(lay.lx2), fld.gll_points(n))
        pm = mr.interp_pressure(Ip, self.p2, self.table, n, lay.lx2, d)
        xyz = [mr.face_values(self.co[k].reshape(nel, -1), self.table, n, d) for k in ("x", "y", "z")[:d]]
        pm = mr.add_mean_gradient(pm, xyz, mr.DP_MEAN, d)
        nuf = nu if np.isscalar(nu) else mr.face_values(np.asarray(nu).reshape(nel, -1), self.table, n, d)
        return mr.face_terms(sij, na, pm, nuf, xyz, mr.X0, d)


@functools.lru_cache(maxsize=None)
def _one_rank(name):
    s = _Setup(name)
    return s, s.compute()


@pytest.mark.parametrize("name", mr.CASE_NAMES)
def test_integrands_and_sums(gpu, name):
    """Gates 1-5."""
    s, r = _one_rank(name)
    lay = s.lay
    n, d = lay.lx1, lay.ldim
    assert len(s.table) == sum(len(o) for o in s.objects)
    if name.startswith("def"):
        per_elem = {}
        for e, _, _ in s.table:
            per_elem[e] = per_elem.get(e, 0) + 1
        assert max(per_elem.values()) == 3                                   # a corner element
        assert [e for e, _, o in s.table if o == 1] != sorted(e for e, _, o in s.table if o == 1)
    if name == "box2d":
        assert {fc for _, fc, _ in s.table} == {1, 2, 3, 4}
    G = s.gradient()
    assert np.array_equal(r["sij"], mr.strain(G, s.table, n, d))                                    # 1
    g, _ = mr.cofactors(gll_derivative(n), s.co, n, d)
    assert np.array_equal(r["na"], mr.face_normals(g, gll_weights(n), s.table, n, d))               # 2
    T = s.restate_terms(r["sij"], r["na"])
    assert np.array_equal(r["dgtq"], mr.face_sums(T, SCALE))                                        # 3
    assert np.array_equal(r["out"], mr.object_sums(s.table, r["dgtq"], len(s.objects)))            # 4
    assert np.array_equal(r["out"][0], mon.sum_objects(r["out"][1:]))                              # 5
    assert np.array_equal(r["vals"], r["out"])
    assert np.all(np.isfinite(r["out"])) and np.max(np.abs(r["out"])) > 0


@pytest.mark.parametrize("name", mr.CASE_NAMES)
def test_independent_route(gpu, name):
    """Gate 6.  Measured on the host (tests/test_monitors.py::test_independent_route_ratio): the float64
    restatement's own ratio is at most 1.631 on these cases; the device is held to 4 x 1.64."""
    _, r = _one_rank(name)
    _, ref64, ref_ld = mr.routes(name)
    e_dev = float(np.max(np.abs(r["out"] - ref_ld)))
    e_ind = float(np.max(np.abs(ref64 - ref_ld)))
    print(f"{name}: device {e_dev:.3e}  independent {e_ind:.3e}  ratio {e_dev / e_ind:.3f}")
    assert e_dev <= TORQUE_GATE * e_ind


def test_cylinder_known_answers(gpu):
    """Gate 7 on the cylinder: p = 1 gives no force, p = x gives scale (-0.785398242, 0), u = A x no viscous
    force (a constant strain on a closed surface)."""
    s, _ = _one_rank("cyl")
    lay, ctx = s.lay, s.ctx
    g, _ = mr.cofactors(gll_derivative(6), s.co, 6, 2)
    na = mr.face_normals(g, gll_weights(6), s.table, 6, 2)
    perimeter = np.sum(np.hypot(na[:, 0], na[:, 1]))
    zero = ctx.vector()
    kw = dict(x0=(0.0, 0.0, 0.0), dp_mean=(0.0, 0.0, 0.0))
    f = s.tq.compute(zero, 0.01, scale=2.0, pm1=np.ones(lay.n_v), **kw)
    assert np.all(np.abs(f[1, 0]) <= 2.0 * 64 * EPS * perimeter) and np.all(f[1, 1] == 0)
    f = s.tq.compute(zero, 0.01, scale=3.0, pm1=s.co["x"], **kw)
    assert abs(f[1, 0, 0] / 3.0 - (-0.785398242)) < 1e-9 and abs(f[1, 0, 1]) < 1e-9
    assert abs(f[1, 0, 0] / 3.0 / (-np.pi / 4) - 1) < 2e-7
    # the same through the mean pressure gradient term: p = 0 + x dpdx_mean
    f2 = s.tq.compute(zero, 0.01, scale=3.0, pm1=np.zeros(lay.n_v), x0=(0.0, 0.0, 0.0), dp_mean=(1.0, 0.0, 0.0))
    assert np.array_equal(f2[1, 0], f[1, 0])
    A = np.array([[0.3, -1.1], [0.7, 0.2]])
    lin = ctx.vector().from_fields({"vx": A[0, 0] * s.co["x"] + A[0, 1] * s.co["y"],
                                    "vy": A[1, 0] * s.co["x"] + A[1, 1] * s.co["y"], "pr": np.zeros(lay.n_p)})
    f = s.tq.compute(lin, 0.5, scale=2.0, pm1=np.zeros(lay.n_v), **kw)
    # the gradient of a linear field on this mesh is exact to 1e-9 (test_gradm1_linear_field_on_cylinder_mesh)
    assert np.all(np.abs(f[1, 1]) <= 2.0 * 0.5 * 4e-9 * perimeter + 64 * EPS * perimeter)
    assert np.any(f[1, 1] != 0)


@pytest.mark.parametrize("name", ["one4", "one10", "def5"])
def test_closed_surface_unit_pressure(gpu, name):
    """Gate 7 in 3-D: with p = 1 the pressure force is scale sum nA over a closed surface, which GLL
    quadrature integrates exactly (degree 2N - 1 in the differentiated direction), so only rounding is left:
    a line sum of lx1 products errs by at most d = lx1 eps B with B = ||D||_inf max|x| >= every |x_a|; a
    cofactor of two such derivatives by 4 d B, times w and summed over the faces (sum w = 4 per face), plus
    the summation's 4 eps sum|nA|."""
    s, _ = _one_rank(name)
    lay = s.lay
    f = s.tq.compute(s.vec, 0.0, x0=(0.0, 0.0, 0.0), scale=2.0, dp_mean=(0.0, 0.0, 0.0), pm1=np.ones(lay.n_v),
                     distributions=True)
    na = s.tq.na.cpu().numpy()[: s.tq.nfaces]
    B = np.abs(gll_derivative(lay.lx1)).sum(axis=1).max() * max(np.abs(a).max() for a in s.co.values())
    tol = 2.0 * (4 * lay.lx1 * EPS * B * B * 4 * s.tq.nfaces + 4 * EPS * np.abs(na).sum())
    print(name, "sum nA", f[0, 0], "tol", tol)
    assert np.all(np.abs(f[0, 0]) <= tol)
    assert np.abs(na).sum() > 1.0


@pytest.mark.parametrize("name,world", [("cyl", 2), ("def5", 3), ("def6", 2), ("one8", 2)])
def test_shards(gpu, name, world):
    """Gate 8.  cyl, w = 2: rank 0 owns no member; one8, w = 2: rank 0 is an empty shard."""
    s1, r1 = _one_rank(name)
    ref = {k: r1["dgtq"][m] for m, k in enumerate(s1.keys)}
    seen, nomember, empty = 0, False, False
    total = np.zeros_like(r1["out"])
    for rank in range(world):
        s = _Setup(name, rank, world)
        r = s.compute()
        nomember |= s.tq.nfaces == 0 and s.lay.n_v > 0
        empty |= s.lay.n_v == 0
        for m, k in enumerate(s.keys):
            assert np.array_equal(r["dgtq"][m], ref[k]), (rank, k)
        seen += len(s.keys)
        assert np.array_equal(r["out"], mr.object_sums(s.table, r["dgtq"], len(s.objects)))
        assert np.array_equal(r["vals"][0], mon.sum_objects(r["out"][1:]))
        if s.tq.nfaces == 0:
            assert np.all(r["out"] == 0)
        total = total + r["out"]
    assert seen == len(s1.keys)
    assert nomember == (name == "cyl") and empty == (name == "one8")
    scale = np.max(np.abs(r1["out"]))
    assert np.max(np.abs(total - r1["out"])) <= 64 * world * EPS * scale


def test_pm1_equals_mesh2_when_lx1_is_lx2(gpu):
    """Gate 9, first half: on a PN-PN layout the pressure already lives on mesh 1."""
    for name, lay in (("box2d", NekLayout(ldim=2, lx1=5, lx2=5, nelgv=6)),
                      ("def5", NekLayout(ldim=3, lx1=5, lx2=5, nelgv=12))):
        s = _Setup(name, lay=lay)
        a = s.compute()
        b = s.compute(pm1=s.p2.reshape(-1))
        assert np.array_equal(a["dgtq"], b["dgtq"]) and np.array_equal(a["out"], b["out"])
        assert np.max(np.abs(a["out"][:, :3])) > 0


@pytest.mark.parametrize("name", ["cyl", "def6", "one3"])
def test_pm1_equals_host_pressure_map(gpu, name):
    """Gate 9, second half: pm1 = map_pressure_to_mesh1(p2) against the in-kernel interpolation.  Per face
    point the two interpolations differ by at most dp = lx2 ldim eps sum|I||p| (the tensor product of |I| on
    |p|); the pressure force of a face then by scale sum dp |nA| plus the rounding of the sum itself,
    (nfp + 2) eps scale sum|pm nA|."""
    s, r = _one_rank(name)
    lay = s.lay
    n, d = lay.lx1, lay.ldim
    pm1 = fld.map_pressure_to_mesh1(s.p2, n, lay.lx2, d)
    b = s.compute(pm1=pm1.reshape(-1))
    Ip = np.abs(fld.interp_matrix(fld.gauss_points(lay.lx2), fld.gll_points(n)))
    dp = lay.lx2 * d * EPS * mr.interp_pressure(Ip, np.abs(s.p2), s.table, n, lay.lx2, d)
    pm = np.abs(mr.interp_pressure(Ip, np.abs(s.p2), s.table, n, lay.lx2, d)) + 1.0   # + |x dp_mean| <= 1
    nfp = dp.shape[1]
    for k in range(d):
        na = np.abs(r["na"][:, k])
        bound = SCALE * (np.sum(dp * na, axis=1) + (nfp + 2) * EPS * np.sum(pm * na, axis=1))
        diff = np.abs(b["dgtq"][:, k] - r["dgtq"][:, k])
        assert np.all(diff <= bound), (k, float(np.max(diff / bound)))
    assert np.array_equal(b["dgtq"][:, 3:6], r["dgtq"][:, 3:6])            # the viscous force ignores p


# ---- 10. hygiene -----------------------------------------------------------------------------------------------

def _raw(s, nan_tail=8, **over):
    """nkv_torque on raw addresses with NaN-tailed output buffers; returns (rc, buffers)."""
    lay, ctx, tq = s.lay, s.ctx, s.tq
    three = lay.ldim == 3
    nf, nfp, ns = tq.nfaces, tq.nfp, 6 if three else 3
    f64 = dict(dtype=torch.float64, device=ctx.device)
    buf = {"dgtq": torch.full((nf * 12 + nan_tail,), np.nan, **f64),
           "out": torch.full(((tq.nobj + 1) * 12 + nan_tail,), np.nan, **f64),
           "sij": torch.full((nf * ns * nfp + nan_tail,), np.nan, **f64),
           "na": torch.full((nf * lay.ldim * nfp + nan_tail,), np.nan, **f64)}
    c3 = ctypes.c_double * 3
    faces = over.pop("faces", tq.faces)
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    fdev = torch.as_tensor(faces).to(ctx.device)
    a = dict(L=ctx.L, lx1=lay.lx1, lx2=lay.lx2, ldim=lay.ldim, D=tq.D.data_ptr(), wg=tq.wg.data_ptr(),
             Ipm=tq.Ipm.data_ptr(), xm=tq.xyz[0].data_ptr(), ym=tq.xyz[1].data_ptr(),
             zm=tq.xyz[2].data_ptr() if three else None, u=s.vec.ptr, u_stride=lay.sv,
             pr=s.vec.ptr + 8 * lay.n_wf * lay.sv, pm1=None, visc_field=None, visc=mr.NU, faces_host=faces.ctypes.data,
             faces_dev=fdev.data_ptr(), nfaces=faces.shape[0], nobj=tq.nobj, x0=c3(*mr.X0), dp=c3(*mr.DP_MEAN),
             scale=SCALE, dgtq=buf["dgtq"].data_ptr(), out=buf["out"].data_ptr(), sij=buf["sij"].data_ptr(),
             na=buf["na"].data_ptr(), stream=ctx.stream)
    a.update(over)
    rc = ctx.lib.nkv_torque(ctypes.byref(a.pop("L")), *a.values())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in buf.items()}


@pytest.mark.parametrize("name", ["box2d", "def5"])
def test_padding_and_viscosity_field(gpu, name):
    s, field = _one_rank(name)
    r = s.compute(visc=mr.NU)
    rc, b = _raw(s)
    assert rc == _lib.NKV_OK
    for k in ("dgtq", "out", "sij", "na"):
        assert np.all(np.isnan(b[k][-8:])) and np.all(np.isfinite(b[k][:-8])), k
        assert np.array_equal(b[k][:-8], r[k].reshape(-1)), k
    # nu as a field: a constant field equals the scalar, a varying one equals the restatement
    nu_c = torch.full((s.lay.n_v,), mr.NU, dtype=torch.float64, device=s.ctx.device)
    rc, c = _raw(s, visc_field=nu_c.data_ptr(), visc=123.0)
    assert rc == _lib.NKV_OK and np.array_equal(c["dgtq"], b["dgtq"], equal_nan=True)
    T = s.restate_terms(r["sij"], r["na"], nu=mr.NU)
    assert np.array_equal(r["dgtq"], mr.face_sums(T, SCALE))
    assert not np.array_equal(field["dgtq"][:, 3:6], r["dgtq"][:, 3:6])      # the varying field of the other tests


def test_argument_checks(gpu):
    s, _ = _one_rank("def5")
    s2, _ = _one_rank("box2d")
    nel = s.lay.nelv
    t = s.tq.faces.copy()

    def bad(col, val, setup=s):
        f = setup.tq.faces.copy()
        f[1, col] = val
        return dict(faces=f)

    z = s.tq.xyz[2].data_ptr()
    pm1 = torch.zeros(s.lay.n_v, dtype=torch.float64, device=s.ctx.device).data_ptr()
    cases = [(s, bad(1, 0)), (s, bad(1, 7)), (s2, bad(1, 5, s2)), (s, bad(0, nel)), (s, bad(0, -1)),
             (s, bad(2, 0)), (s, bad(2, 3)), (s, dict(zm=None)), (s2, dict(zm=z)), (s, dict(u_stride=s.lay.n_v - 1)),
             (s, dict(pm1=pm1)), (s, dict(pr=None)), (s, dict(lx1=11)), (s, dict(lx1=4)), (s, dict(ldim=4)),
             (s, dict(lx2=6)), (s, dict(lx2=2)), (s, dict(nobj=0)), (s, dict(nfaces=-1)), (s, dict(D=None)),
             (s, dict(wg=None)), (s, dict(Ipm=None)), (s, dict(faces_host=None)), (s, dict(faces_dev=None)),
             (s, dict(dgtq=None)), (s, dict(out=None)), (s, dict(x0=None)), (s, dict(dp=None)), (s, dict(u=None))]
    for setup, over in cases:
        rc, b = _raw(setup, **dict(over))
        assert rc == _lib.NKV_EINVAL, over
        assert _lib.last_error(), over
        for k, v in b.items():
            assert np.all(np.isnan(v)), (over, k)             # refused before any launch
    assert np.array_equal(t, s.tq.faces)
    rc, b = _raw(s, nfaces=0)                                  # no member: zeros, nothing else written
    assert rc == _lib.NKV_OK and np.all(b["out"][:-8] == 0) and np.all(np.isnan(b["out"][-8:]))
    assert np.all(np.isnan(b["dgtq"]))


def test_torque_monitor_in_sfd(gpu, tmp_path):
    """Gate 11."""
    s, _ = _one_rank("box2d")
    ctx, lay = s.ctx, s.lay
    path = tmp_path / "lift_drag.dat"
    tm = mon.TorqueMonitor(ctx, s.tq, path=str(path), skip=2, visc=mr.NU, x0=mr.X0, scale=SCALE, dp_mean=mr.DP_MEAN)
    sfd = fixedp.SFD(ctx, 0.1, 0.05, dt=0.01, tol=1e-9, monitors=[tm])
    v, fc = ctx.vector(), ctx.vector()
    v.copy_from(s.vec)
    sfd.start(v)
    expect = []
    for istep in range(1, 5):
        v.scal(1.0 + 0.01 * istep)
        sfd.step(v, fc, time=0.5 * istep)
        if istep % 2 == 0:
            vals = s.tq.compute(v, mr.NU, x0=mr.X0, scale=SCALE, dp_mean=mr.DP_MEAN)
            expect += [mon.torque_record(istep, 0.5 * istep, vals[o], lay.ldim) for o in (1, 2)]
    tm.close()
    sfd.close()
    lines = path.read_text().splitlines()
    assert lines == expect and len(lines) == 4 and tm.records == 2
    assert all(len(ln) == 8 + 10 * 15 for ln in lines)


# ---- statistics -------------------------------------------------------------------------------------------------

STAT_CASES = {
    "2d": NekLayout(ldim=2, lx1=4, lx2=2, nelgv=3),
    "3d_s0": NekLayout(ldim=3, lx1=5, lx2=3, nelgv=5),
    "3d_s1": NekLayout(ldim=3, lx1=5, lx2=3, nelgv=5, n_scalars=1),
    "3d_s2": NekLayout(ldim=3, lx1=5, lx2=3, nelgv=5, n_scalars=2),
    "3d_nopr": NekLayout(ldim=3, lx1=5, lx2=3, nelgv=5, n_scalars=1, ifpo=False),
    "3d_two_chunks": NekLayout(ldim=3, lx1=5, lx2=3, nelgv=19, n_scalars=1),   # n_v = 2375: odd, two chunks
}
TIMES = [0.0, 0.1, 0.25, 0.25, 0.4, 0.45, 0.7, 0.75]          # istep 1..8; a repeated time; dumps at 4 and 8


def _global_vector(glob, step):
    rng = np.random.default_rng(100 + step)
    return {nm: rng.standard_normal(glob.pts_v * glob.nelgv if nm != "pr" else glob.pts_p * glob.nelgv)
            for nm, _, _ in glob.field_slices()}


def _local_packed(lay, gv, fill):
    """The padded host vector of this shard with `fill` in the padding rows and the time slot."""
    out = np.full(lay.ld, fill)
    e0, e1 = lay.elem_range()
    for nm, s, n in lay.field_slices():
        per = lay.pts_p if nm == "pr" else lay.pts_v
        out[s:s + n] = gv[nm][e0 * per: e1 * per]
    return out


def _nan_padding(lay, a):
    live = np.zeros(lay.ld, dtype=bool)
    for _, s, n in lay.field_slices():
        live[s:s + n] = True
    a[~live] = np.nan
    return a


def _run_statistics(glob, rank, world, outdir, cross=True, ifstatis=True, base=True):
    lay = glob.shard(rank, world)
    ctx = NekContext(lay, comm=_ShardComm(rank, world) if world > 1 else None, max_cols=4)
    lay = ctx.layout
    bvec = None
    hb = _local_packed(lay, _global_vector(glob, 99), 0.0)
    if base:
        bvec = ctx.vector().from_packed(hb)
    st = mon.Statistics(ctx, base=bvec, ifstatis=ifstatis, cross=cross, iastep=4, outdir=str(outdir), session="s")
    # NaN in every padding row of the accumulators: the kernel must leave them alone
    for vec in [st.avg] + ([st.rms] if ifstatis else []):
        vec.from_packed(_nan_padding(lay, np.zeros(lay.ld)))
    nc = st.ncross
    if cross:
        c0 = np.zeros((nc, lay.sv))
        c0[:, lay.n_v:] = np.nan
        st.cross[: nc * lay.sv] = torch.as_tensor(c0.reshape(-1)).to(ctx.device)
    clock = mon.StatisticsSchedule(4)
    avg = _nan_padding(lay, np.zeros(lay.ld))
    rms = _nan_padding(lay, np.zeros(lay.ld)) if ifstatis else None
    cr = np.zeros((nc, lay.sv)) if cross else None
    if cross:
        cr[:, lay.n_v:] = np.nan
    v = ctx.vector()
    dumps = []
    for istep, t in enumerate(TIMES, start=1):
        hv = _local_packed(lay, _global_vector(glob, istep), np.nan)     # NaN padding in the input too
        v.from_packed(hv)
        paths = st(v, istep, t)
        ab = clock.advance(t)
        if ab:
            mr.avg_step(lay, hv, avg, rms, cr, *ab)
        if clock.due(istep):
            ft = clock.dump(istep)
            dumps.append((paths, ft, avg.copy(), None if rms is None else rms.copy(), None if cr is None else cr.copy()))
        else:
            assert paths is None
    torch.cuda.synchronize()
    dev = dict(avg=st.avg.to_packed(), rms=st.rms.to_packed() if ifstatis else None,
               cross=st.cross.cpu().numpy()[: nc * lay.sv].reshape(nc, lay.sv) if cross else None)
    return lay, st, dev, dict(avg=avg, rms=rms, cross=cr), dumps, hb


@pytest.mark.parametrize("name", list(STAT_CASES))
def test_statistics_bit_identical(gpu, name, tmp_path):
    glob = STAT_CASES[name]
    lay, st, dev, host, dumps, hb = _run_statistics(glob, 0, 1, tmp_path)
    assert st.updates == 6 and st.dumps == 2 and len(dumps) == 2
    for k in ("avg", "rms", "cross"):
        assert np.array_equal(dev[k], host[k], equal_nan=True), k
        assert np.any(np.isnan(dev[k])) and np.all(np.isfinite(host[k][..., : lay.n_v]))
    assert lay.n_v % 2048 != 0
    # the four files of the first dump (in the middle of the run)
    paths, ft, avg, rms, cr = dumps[0]
    assert [p.split("/")[-1][:3] for p in paths] == ["avt", "avg", "rms", "rm2"]
    vel = lambda a: [a[k * lay.sv: k * lay.sv + lay.n_v].reshape(lay.nelv, -1) for k in range(lay.ldim)]  # noqa: E731
    want = {"avt": vel(avg - np.where(np.isnan(avg), 0.0, hb)), "avg": vel(avg), "rms": vel(rms),
            "rm2": [cr[m, : lay.n_v].reshape(lay.nelv, -1) for m in range(st.ncross)]}
    for p in paths:
        f = fld.read_fld(p)
        kind = p.split("/")[-1][:3]
        assert f.wdsize == 8 and abs(f.time - ft) <= 1e-12 * ft and f.istep == 4
        for k, nm in enumerate(("vx", "vy", "vz")[: lay.ldim]):
            w = want[kind][k] if k < len(want[kind]) else np.zeros((lay.nelv, lay.pts_v))
            assert np.array_equal(f.fields[nm], w), (kind, nm)
        src = {"avt": avg - np.where(np.isnan(avg), 0.0, hb), "avg": avg}.get(kind, rms)
        assert ("pr" in f.fields) == bool(lay.n_p)
        if lay.n_p:
            s = lay.n_wf * lay.sv
            pm = fld.map_pressure_to_mesh1(src[s: s + lay.n_p].reshape(lay.nelv, -1), lay.lx1, lay.lx2, lay.ldim)
            assert np.array_equal(f.fields["pr"], pm), kind
        for sc in range(lay.n_scalars):
            k = lay.ldim + sc
            assert np.array_equal(f.fields["t" if sc == 0 else f"s{sc:02d}"],
                                  src[k * lay.sv: k * lay.sv + lay.n_v].reshape(lay.nelv, -1)), (kind, sc)
    assert abs(dumps[0][1] - 0.25) < 1e-15 and abs(dumps[1][1] - 0.5) < 1e-15


def test_statistics_options(gpu, tmp_path):
    """ifstatis = False (avg only), cross = False (rm2 holds zeros, as the reference writes), no base (no avt)."""
    glob = STAT_CASES["3d_s1"]
    lay, st, dev, host, dumps, _ = _run_statistics(glob, 0, 1, tmp_path / "a", cross=False, base=False)
    assert np.array_equal(dev["avg"], host["avg"], equal_nan=True)
    assert np.array_equal(dev["rms"], host["rms"], equal_nan=True)
    paths = dumps[0][0]
    assert [p.split("/")[-1][:3] for p in paths] == ["avg", "rms", "rm2"]
    f = fld.read_fld(paths[2])
    assert all(np.all(f.fields[nm] == 0) for nm in ("vx", "vy", "vz"))
    lay, st, dev, host, _, _ = _run_statistics(glob, 0, 1, tmp_path / "b", cross=False, ifstatis=False)
    assert np.array_equal(dev["avg"], host["avg"], equal_nan=True) and st.rms is None
    with pytest.raises(ValueError):
        mon.Statistics(st.ctx, cross=True, ifstatis=False)
    with pytest.raises(ValueError):
        st.dump(1)


@pytest.mark.parametrize("name,world", [("3d_two_chunks", 2), ("3d_s0", 3), ("2d", 4)])
def test_statistics_shards(gpu, name, world, tmp_path):
    """Each shard's accumulators are the unsharded run's rows of its elements, bit for bit (2d, w = 4: rank 0
    is an empty shard)."""
    glob = STAT_CASES[name]
    _, _, one, _, _, _ = _run_statistics(glob, 0, 1, tmp_path / "one")
    empty = False
    for rank in range(world):
        lay, _, dev, host, _, _ = _run_statistics(glob, rank, world, tmp_path / f"r{rank}")
        empty |= lay.n_v == 0
        e0, _ = lay.elem_range()
        for k in ("avg", "rms"):
            assert np.array_equal(dev[k], host[k], equal_nan=True)
            for (nm, s, n), (_, s1, _) in zip(lay.field_slices(), glob.field_slices()):
                o = e0 * (glob.pts_p if nm == "pr" else glob.pts_v)
                assert np.array_equal(dev[k][s:s + n], one[k][s1 + o: s1 + o + n]), (k, nm)
        for m in range(dev["cross"].shape[0]):
            o = e0 * glob.pts_v
            assert np.array_equal(dev["cross"][m, : lay.n_v], one["cross"][m, o: o + lay.n_v])
    assert empty == (name == "2d")


def test_avg_step_argument_checks(gpu):
    lay = STAT_CASES["3d_s1"]
    ctx = NekContext(lay, max_cols=4)
    v, a, r = ctx.vector(), ctx.vector(), ctx.vector()
    c = torch.zeros(3 * lay.sv, dtype=torch.float64, device=ctx.device)
    call = lambda *args: ctx.lib.nkv_avg_step(ctypes.byref(ctx.L), *args, 0.5, 0.5, ctx.stream)  # noqa: E731
    assert call(v.ptr, a.ptr, r.ptr, c.data_ptr(), 3) == _lib.NKV_OK
    for args in ((v.ptr, v.ptr, r.ptr, None, 0), (v.ptr, a.ptr, a.ptr, None, 0), (v.ptr, a.ptr, v.ptr, None, 0),
                 (v.ptr, a.ptr, r.ptr, a.ptr, 3), (v.ptr, a.ptr, r.ptr, v.ptr + 8 * lay.sv, 1),
                 (v.ptr, a.ptr + 16, a.ptr, None, 0), (v.ptr, a.ptr, r.ptr, c.data_ptr(), 2),
                 (v.ptr, a.ptr, None, c.data_ptr(), 3), (None, a.ptr, r.ptr, None, 0), (v.ptr, None, r.ptr, None, 0)):
        assert call(*args) == _lib.NKV_EINVAL, args
    lay2 = STAT_CASES["2d"]
    ctx2 = NekContext(lay2, max_cols=4)
    v2, a2, r2 = ctx2.vector(), ctx2.vector(), ctx2.vector()
    assert ctx2.lib.nkv_avg_step(ctypes.byref(ctx2.L), v2.ptr, a2.ptr, r2.ptr, c.data_ptr(), 3, 0.5, 0.5,
                                 ctx2.stream) == _lib.NKV_EINVAL     # three cross moments need three velocities
    torch.cuda.synchronize()
