"""Flow diagnostics on the device: vorticity, the vortex criteria and the energy / enstrophy files.

* ``vortex_core`` and its criteria (core/postproc.f90:2-522): :class:`VortexCore` evaluates any set of
  them in ONE tiled launch (``nkv_vortex_criteria``) that differentiates the velocity in LDS, keeps the
  gradient tensor in registers and runs Nek5000's ``filter_s0`` in LDS before the single store;
* ``comp_vort3`` (Nek5000's; the calls at utils.f90:432, 509, 707): the curl from the same launch, then
  the mass-weighted average ``dssum(bm1 w) / dssum(bm1)``, written ``dsavg(bm1 w) / dsavg(bm1)`` (the
  multiplicities cancel) so it takes the same ``average(ptr)`` callable as the energy budget;
* ``outpost_vort`` (utils.f90:420-444) and ``nekStab_outpost``'s ``vor`` / ``vox`` files (:489-536);
* ``nekStab_energy`` / ``nekStab_enstrophy`` (utils.f90:647-716): :class:`EnergyMonitor` and
  :class:`EnstrophyMonitor`, one streaming launch (``nkv_energy_components``) and one all-reduce per record.

``filter_s0(v, wght, ncut)`` is Nek5000's and not part of the reference tree: :func:`legendre_filter`
restates its matrix from the definition.  ``compute_omega`` (postproc.f90:81-104) is not
built: it reads an undefined ``glmax_qc`` and has no caller.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from .newton import fortran_e
from .sensitivity import Gradm1
from .vector import NekContext, NekVector

# criterion name -> code (include/nekkrylov.h, enum nkv_vortex_criterion); slots ascend with the code
CRITERIA = {"vorticity": _lib.NKV_VC_VORTICITY, "lambda2": _lib.NKV_VC_LAMBDA2, "q": _lib.NKV_VC_Q,
            "delta": _lib.NKV_VC_DELTA, "swirling": _lib.NKV_VC_SWIRLING, "omega": _lib.NKV_VC_OMEGA,
            "symmetric": _lib.NKV_VC_SYMMETRIC, "assymetric": _lib.NKV_VC_ASSYMETRIC,
            "lambda_ci": _lib.NKV_VC_LAMBDA_CI}   # swirling before its square (not a vortex_core name)
# the names vortex_core accepts (postproc.f90:8-21)
VORTEX_NAMES = ("lambda2", "q", "delta", "swirling", "omega", "symmetric", "assymetric")
# never filtered: the curl (averaged afterwards) and lambda2 (vortex_core calls it without filter_s0, :8-9)
UNFILTERED = ("vorticity", "lambda2")


def _gll_points_ld(n: int) -> np.ndarray:
    """The n Gauss–Lobatto–Legendre points in long double (Newton on P_N', as ``gll_derivative``)."""
    from .fld import gll_points

    ld = np.longdouble
    N = n - 1
    z = gll_points(n).astype(ld)
    if n <= 2:
        return z
    x = z[1:-1].copy()
    for _ in range(8):
        p0, p1 = np.ones_like(x), x.copy()
        for k in range(2, N + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        dp = N * (x * p1 - p0) / (x * x - 1)
        ddp = (2 * x * dp - N * (N + 1) * p1) / (1 - x * x)
        x = x - dp / ddp
    z[1:-1] = x
    return z


def _inverse_ld(A: np.ndarray) -> np.ndarray:
    """Gauss–Jordan with partial pivoting in the dtype of ``A`` (numpy.linalg has no long double)."""
    n = A.shape[0]
    M = np.concatenate([A.copy(), np.eye(n, dtype=A.dtype)], axis=1)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        M[c] = M[c] / M[c, c]
        for r in range(n):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return M[:, n:]


def legendre_filter(lx1: int, wght: float = 0.5, ncut: int = 1) -> np.ndarray:
    """The matrix of Nek5000's ``filter_s0(v, wght, ncut)`` (lx1 x lx1, row-major): F = Phi diag(sigma)
    Phi^-1 with Phi[j, k] = phi_k(z_j) on the GLL points, phi_1 = L_0, phi_2 = L_1, phi_k = L_{k-1} -
    L_{k-3} (k >= 3; the boundary-preserving bubble basis), sigma_k = 1 for k <= k0 = lx1 - ncut and
    1 - wght (k - k0)^2 / ncut^2 above.  The reference always filters with (0.5, 1): the top mode is
    halved.  Built in long double and rounded, as ``gll_derivative``."""
    if lx1 < 3:
        raise ValueError(f"legendre_filter: lx1={lx1} < 3 has no bubble mode to filter")
    if not 1 <= ncut <= lx1 - 2:
        raise ValueError(f"legendre_filter: ncut={ncut} outside 1..{lx1 - 2}")
    ld = np.longdouble
    z = _gll_points_ld(lx1)
    L = [np.ones_like(z), z.copy()]
    for k in range(2, lx1):
        L.append(((2 * k - 1) * z * L[k - 1] - (k - 1) * L[k - 2]) / k)
    phi = np.stack([L[k] if k < 2 else L[k] - L[k - 2] for k in range(lx1)], axis=1)
    sigma = np.ones(lx1, dtype=ld)
    k0 = lx1 - ncut
    for k in range(k0 + 1, lx1 + 1):                          # 1-based mode numbers
        sigma[k - 1] = 1 - ld(wght) * ld((k - k0) ** 2) / ld(ncut ** 2)
    F = (phi * sigma[None, :]) @ _inverse_ld(phi)
    return np.ascontiguousarray(F.astype(np.float64))


class VortexCore:
    """``vortex_core`` on this rank's elements.  Owns the GLL derivative matrix, the filter matrix and the
    coordinates on the device; ``grad_op`` reuses an existing :class:`~.sensitivity.Gradm1` (its D and
    coordinates) instead of uploading them again.  The velocity is the first ldim field segments of a
    :class:`NekVector` of ``ctx`` (any layout)."""

    def __init__(self, ctx: NekContext, coords: dict, grad_op: Gradm1 | None = None, wght: float = 0.5,
                 ncut: int = 1):
        lay = ctx.layout
        self.ctx, self.coords = ctx, coords
        self.grad_op = grad_op if grad_op is not None else Gradm1(ctx, coords)
        self.D, self.xyz = self.grad_op.D, self.grad_op.xyz
        self.F = (torch.as_tensor(legendre_filter(lay.lx1, wght, ncut)).to(ctx.device) if lay.lx1 >= 3 else None)
        self.n_vort = 3 if lay.ldim == 3 else 1
        self._denominators = {}
        self._auto = None

    # ---- the launches ----
    def slots(self, names) -> dict:
        """name -> (first slot, number of slots) of one launch selecting ``names``."""
        out, s = {}, 0
        for nm in sorted(set(names), key=CRITERIA.__getitem__):
            k = self.n_vort if nm == "vorticity" else 1
            out[nm] = (s, k)
            s += k
        return out

    def launch(self, u_ptr: int, u_stride: int, names, filtered, out_ptr: int, o_stride: int, grad_ptr=None,
               g_stride: int = 0) -> None:
        """One ``nkv_vortex_criteria`` launch on raw device addresses.  ``filtered``: True (every criterion
        the reference filters), False, or the names to filter."""
        lay = self.ctx.layout
        for nm in names:
            if nm not in CRITERIA:
                raise ValueError(f"unknown vortex determinant {nm!r}; use one of {sorted(CRITERIA)}")
        mask = sum(1 << CRITERIA[nm] for nm in set(names))
        fnames = set(names) if filtered is True else (set() if not filtered else set(filtered))
        fmask = sum(1 << CRITERIA[nm] for nm in fnames)
        use_f = self.F is not None and fmask
        if fmask and self.F is None and (fnames - set(UNFILTERED)):
            raise ValueError(f"lx1={lay.lx1} < 3 has no filter; pass filtered=False")
        self.ctx.call("nkv_vortex_criteria", lay.lx1, lay.ldim, self.D.data_ptr(),
                      self.F.data_ptr() if use_f else None, self.xyz[0].data_ptr(), self.xyz[1].data_ptr(),
                      self.xyz[2].data_ptr() if lay.ldim == 3 else None, u_ptr, int(u_stride), mask, fmask,
                      out_ptr, int(o_stride), grad_ptr, int(g_stride), self.ctx.stream)

    def criteria(self, vec: NekVector, names, filtered=True) -> dict:
        """Several criteria from one launch: name -> tensor of sv doubles (n_v live; ``vorticity``: a
        (1 or 3, sv) tensor)."""
        lay = self.ctx.layout
        names = list(names)
        sl = self.slots(names)
        n = sum(k for _, k in sl.values())
        out = torch.zeros((n, lay.sv), dtype=torch.float64, device=self.ctx.device)
        self.launch(vec.ptr, lay.sv, names, filtered, out.data_ptr(), lay.sv)
        return {nm: (out[s:s + k] if nm == "vorticity" else out[s]) for nm, (s, k) in sl.items()}

    def vortex_core(self, vec: NekVector, name: str, filtered: bool = True) -> torch.Tensor:
        """``vortex_core(l2, name)`` (postproc.f90:2-29) of the velocity of ``vec``: sv doubles."""
        if name not in VORTEX_NAMES:
            raise ValueError(f"unknown vortex determinant {name!r}. Please use one of: {', '.join(VORTEX_NAMES)}")
        return self.criteria(vec, [name], filtered)[name]

    def filter(self, ptr: int, nfld: int = 1, stride: int | None = None, out_ptr: int | None = None,
               o_stride: int | None = None) -> None:
        """``filter_s0`` of ``nfld`` field segments at ``ptr`` (in place unless ``out_ptr``)."""
        lay = self.ctx.layout
        if self.F is None:
            raise ValueError(f"lx1={lay.lx1} < 3 has no filter")
        stride = lay.sv if stride is None else stride
        self.ctx.call("nkv_filter_s0", lay.lx1, lay.ldim, self.F.data_ptr(), ptr, int(stride), int(nfld),
                      ptr if out_ptr is None else out_ptr, int(stride if o_stride is None else o_stride),
                      self.ctx.stream)

    # ---- comp_vort3 ----
    def _average(self, average):
        if isinstance(average, str):
            if average != "auto":
                raise ValueError("average: 'auto', a callable f(ptr) or None")
            if self._auto is None:
                from .gs import auto_average

                self._auto = auto_average(self.ctx, self.coords)   # FaceAverage at world 1, else GatherScatter
            return self._auto, "auto"
        return average, average

    def comp_vort3(self, vec: NekVector, average="auto", bm1=None) -> torch.Tensor:
        """Nek5000's ``comp_vort3``: the curl of the velocity of ``vec``, then dssum(bm1 w) / dssum(bm1)
        as two applications of ``average(ptr)`` (``dsavg`` of one segment in place, e.g.
        ``seeds.FaceAverage.apply``; "auto": ``FaceAverage`` on one rank, ``gs.GatherScatter`` over the
        shards on several; a ``GatherScatter`` averages the components in one batch; None: the raw
        element-local curl).  The averaged ``bm1`` is computed once per ``average``.  ``bm1``: the mass
        matrix (default the context's weights).  Returns a (1 or 3, sv) tensor."""
        from .postproc import _bm1_tensor

        ctx, lay = self.ctx, self.ctx.layout
        w = self.criteria(vec, ["vorticity"], filtered=False)["vorticity"]
        if average is None:
            return w
        from .gs import as_gather_scatter

        fn, key = self._average(average)
        gs = as_gather_scatter(fn)   # collective at world > 1: an empty shard takes part too
        n = lay.n_v
        b = _bm1_tensor(ctx, bm1)[:n]
        if key not in self._denominators or self._denominators[key][0] is not bm1:
            den = b.clone()
            if gs is not None:
                gs.apply(den.data_ptr())
            elif n:
                fn(den.data_ptr())
            self._denominators[key] = (bm1, den)
        den = self._denominators[key][1]
        if gs is not None:   # the components in one batch: one exchange
            w[:, :n] *= b
            gs.apply_many([w[c].data_ptr() for c in range(self.n_vort)])
            w[:, :n] /= den[:n]
            return w
        for c in range(self.n_vort):
            row = w[c]
            row[:n] *= b
            if n:
                fn(row.data_ptr())
            row[:n] /= den
        return w


def comp_vort3(core: VortexCore, vec: NekVector, average="auto", bm1=None) -> torch.Tensor:
    """:meth:`VortexCore.comp_vort3`."""
    return core.comp_vort3(vec, average, bm1)


# ---- field files ---------------------------------------------------------------------------------

def _empty_file(lay, time: float, istep: int):
    from . import fld

    e0, e1 = lay.elem_range()
    return fld.FldFile(lay.lx1, lay.lx1, lay.lx1 if lay.ldim == 3 else 1, lay.nelgv, float(time), int(istep),
                       lay.rank, lay.world, "", np.arange(e0 + 1, e1 + 1, dtype=np.int32), {})


def _put_velocity(lay, f, rows) -> None:
    """rows: up to ldim tensors of >= n_v doubles; missing components are written as zeros."""
    for k, nm in enumerate(("vx", "vy", "vz")[: lay.ldim]):
        a = rows[k][: lay.n_v].cpu().numpy() if k < len(rows) else np.zeros(lay.n_v)
        f.fields[nm] = a.reshape(lay.nelv, lay.pts_v)
    f.rdcode += "U"


def outpost_vort(ctx: NekContext, vec: NekVector, prefix: str, num: int, core: VortexCore | None = None,
                 coords: dict | None = None, outdir: str = ".", session: str = "nek", average="auto",
                 time: float = 0.0, istep: int = 0, bm1=None, write=None) -> str:
    """``outpost_vort`` (utils.f90:420-444): ``<prefix><session><rank>.f<num>`` with ``comp_vort3`` of the
    velocity of ``vec`` as the velocity field and neither pressure nor temperature (ifpo = ifto =
    .false.).  In 2-D the one component is vx and vy is zero.  ``core``: a :class:`VortexCore` (built from
    ``coords`` when absent).  ``write``: a ``fld.WriteGuard`` when called inside a collective block."""
    from . import fld

    lay = ctx.layout
    core = core if core is not None else VortexCore(ctx, coords)
    w = core.comp_vort3(vec, average, bm1)
    f = _empty_file(lay, time, istep)
    _put_velocity(lay, f, [w[c] for c in range(core.n_vort)])
    path = os.path.join(outdir, fld.fld_name(prefix, session, lay.rank, num))
    (write or (lambda fn, *a: fn(*a)))(fld.write_fld, path, f)
    return path


def nekstab_outpost(ctx: NekContext, vec: NekVector, num: int, core: VortexCore, outdir: str = ".",
                    session: str = "nek", ifvor: bool = True, ifvox: bool = True, average="auto",
                    time: float = 0.0, istep: int = 0, bm1=None) -> list:
    """``nekStab_outpost``'s two files (utils.f90:506-526): ``vor`` (the averaged vorticity as the velocity)
    and ``vox``.  In 3-D the ``vox`` velocity is (lambda2, q, omega) as ``vortex_core`` returns them (q
    and omega filtered), from one launch.  In 2-D ("no lambda2, no q", :520) the reference writes omega to
    the temperature slot of a second ``vox`` file after a first one whose velocity is meaningless; here
    the one 2-D ``vox`` file holds omega as the temperature and nothing else.  Returns the paths."""
    from . import fld

    lay = ctx.layout
    paths = []
    with fld.collective_output(ctx.comm) as write:
        write(os.makedirs, outdir, exist_ok=True)
        if ifvor:
            paths.append(outpost_vort(ctx, vec, "vor", num, core=core, outdir=outdir, session=session,
                                      average=average, time=time, istep=istep, bm1=bm1, write=write))
        if ifvox:
            f = _empty_file(lay, time, istep)
            if lay.ldim == 3:
                c = core.criteria(vec, ["lambda2", "q", "omega"], filtered=True)
                _put_velocity(lay, f, [c["lambda2"], c["q"], c["omega"]])
            else:
                om = core.vortex_core(vec, "omega")
                f.fields["t"] = om[: lay.n_v].cpu().numpy().reshape(lay.nelv, lay.pts_v)
                f.rdcode += "T"
            path = os.path.join(outdir, fld.fld_name("vox", session, lay.rank, num))
            write(fld.write_fld, path, f)
            paths.append(path)
    return paths


# ---- total_energy.dat / total_enstrophy.dat ----------------------------------------------------------

def energy_record(time: float, sums, eek: float) -> str:
    """``(6E15.7)`` of utils.f90:675: time, uek eek, vek eek, wek eek, (uek + vek + wek) eek, pot eek."""
    uek, vek, wek, pot = (float(s) for s in sums)
    return "".join(fortran_e(v, 15, 7) for v in (time, uek * eek, vek * eek, wek * eek, (uek + vek + wek) * eek, pot * eek))


def enstrophy_record(time: float, sums, eek: float) -> str:
    """``(5E15.7)`` of utils.f90:711: time, uek eek, vek eek, wek eek, (uek + vek + wek) eek."""
    uek, vek, wek = (float(s) for s in sums[:3])
    return "".join(fortran_e(v, 15, 7) for v in (time, uek * eek, vek * eek, wek * eek, (uek + vek + wek) * eek))


class _Monitor:
    """The file, ``skip`` and ``eek = 0.5 / volume`` the two monitors share.  ``volume`` defaults to the
    all-reduced sum of the context's weights; the reference divides by ``volvm1``, the sum of ``bm1``,
    which differs from the dot weights (``bm1s``) inside a sponge: pass the full volume there."""

    def __init__(self, ctx: NekContext, path, skip: int = 1, volume: float | None = None):
        from .fixedp import _volume

        if skip < 1:
            raise ValueError(f"skip={skip} < 1")
        self.ctx, self.skip = ctx, int(skip)
        self.volume = _volume(ctx) if volume is None else float(volume)
        self.eek = 0.5 / self.volume
        self.sums = torch.zeros(4, dtype=torch.float64, device=ctx.device)
        self.fh = open(path, "w") if (path is not None and ctx.comm.rank == 0) else None
        self.records = 0

    def _reduce(self, f_ptr: int, f_stride: int, ncomp: int, t_ptr=None, y_ptr=None):
        ctx = self.ctx
        ctx.call("nkv_energy_components", ctx.w.data_ptr(), f_ptr, int(f_stride), int(ncomp), t_ptr, y_ptr,
                 self.sums.data_ptr(), ctx.ws.data_ptr(), ctx.stream)
        ctx.comm.allreduce_(self.sums)                      # one all-reduce carries all the sums
        vals = self.sums.cpu().numpy().copy()
        if np.isnan(vals).any():
            ctx.check_nan()
        return vals

    def _write(self, line: str) -> None:
        self.records += 1
        if self.fh is not None:
            self.fh.write(line + "\n")
            self.fh.flush()

    def close(self) -> None:
        if self.fh is not None:
            self.fh.close()
            self.fh = None


class EnergyMonitor(_Monitor):
    """``nekStab_energy`` (utils.f90:647-679): every ``skip`` steps one ``(6E15.7)`` record of
    ``total_energy.dat``.  ``y``: the y coordinates (n_v values) for the potential-energy term
    ``pot = glsc3(t, bm1s, ym1)`` (:674, ifheat); without them, or on a layout without scalars, pot = 0."""

    def __init__(self, ctx: NekContext, path="total_energy.dat", skip: int = 1, volume: float | None = None, y=None):
        super().__init__(ctx, path, skip, volume)
        self.y = None
        if y is not None and ctx.layout.n_scalars:
            a = np.asarray(y, dtype=np.float64)
            if a.size != ctx.layout.n_v:
                raise ValueError(f"y: {a.size} points, the layout has n_v={ctx.layout.n_v}")
            self.y = torch.as_tensor(a if a.size else np.zeros(2)).to(ctx.device)

    def __call__(self, v: NekVector, istep: int, time: float):
        if istep % self.skip:
            return None
        lay = self.ctx.layout
        heat = self.y is not None
        vals = self._reduce(v.ptr, lay.sv, lay.ldim, v.ptr + 8 * lay.ldim * lay.sv if heat else None,
                            self.y.data_ptr() if heat else None)
        self._write(energy_record(time, vals, self.eek))
        return vals


class EnstrophyMonitor(_Monitor):
    """``nekStab_enstrophy`` (utils.f90:681-716): every ``skip`` steps ``comp_vort3`` and one ``(5E15.7)``
    record of ``total_enstrophy.dat``.  In 2-D the one vorticity component is the first sum and the
    others are zero (the reference reads never-set columns of ``vort`` there)."""

    def __init__(self, ctx: NekContext, core: VortexCore, path="total_enstrophy.dat", skip: int = 1,
                 volume: float | None = None, average="auto", bm1=None):
        super().__init__(ctx, path, skip, volume)
        self.core, self.average, self.bm1 = core, average, bm1

    def __call__(self, v: NekVector, istep: int, time: float):
        if istep % self.skip:
            return None
        w = self.core.comp_vort3(v, self.average, self.bm1)
        vals = self._reduce(w.data_ptr(), self.ctx.layout.sv, self.core.n_vort)
        self._write(enstrophy_record(time, vals, self.eek))
        return vals


__all__ = ["CRITERIA", "VORTEX_NAMES", "legendre_filter", "VortexCore", "comp_vort3", "outpost_vort",
           "nekstab_outpost", "EnergyMonitor", "EnstrophyMonitor", "energy_record", "enstrophy_record"]
