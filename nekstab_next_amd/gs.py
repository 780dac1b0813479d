"""Gather-scatter over element shards: Nek5000's ``dssum`` + ``vmult`` (and ``dsavg``, the same again)
for the consumers that average shared GLL points — the noise seed (utils.f90:258-359), the base-flow
sensitivity (sensitivity.f90:170-259), the energy budget (postproc.f90:853-872) and ``comp_vort3``.

:class:`GatherScatter` is :class:`~.seeds.FaceAverage` for any world size: every group of coincident
points gets the sum of its members in ascending GLOBAL point number (``e_first * pts_v + local
index``) times ``1.0 / count`` — ``nkv_group_average``'s arithmetic.  Ranks exchange member VALUES,
never partial sums, so the result is bit-identical to the one-rank average for any sharding, and
identical on every rank that holds a copy of a point.  ``apply_many`` averages up to
``NKV_GS_MAX_FIELDS`` field segments with one pack (``nkv_gs_pack``), one exchange
(``Comm.allgather_``) and one average launch (``nkv_gs_average``); longer lists go in rounds of that
many.

The plan is built by host NumPy functions that take arrays only (no process group), so a test can
drive them for every rank of a simulated world in one process:

* :func:`local_setup` — per rank: the local groups (``seeds.group_ids``: cells of ``tol``, joined
  across a rounding half-step; singletons included) and the *candidate* points, those that could
  have a copy on another rank, with their coordinates and global point numbers.  Candidates follow
  the exposed-face rule (:func:`candidate_points`): an element face is keyed by the sorted local-group
  ids of its 2^(ldim-1) corner points; a key that occurs once on the rank is an exposed face (no
  local neighbour); a point is a candidate when its local group has a member on an exposed face.  An
  element that touches another shard only along an edge or at a vertex still has an exposed face
  through that edge or vertex, since the elements around it on this rank do not close up.
* the all-gather of every rank's candidates (the caller's: a list in the test, ``Comm.allgather_``
  in :class:`GatherScatter`);
* :func:`build_plan` — per rank: the candidates of all ranks grouped by the same rule with the same
  ``tol`` (the cells are absolute, so this is the one-rank grouping restricted to the candidates);
  a candidate group with members on two or more ranks is *shared*.  Every rank derives every rank's
  send list from the gathered data alone (a rank's shared candidates, ascending), so a remote member
  is named by (rank, position in that rank's send list) without a second exchange.  The plan holds
  the CSR ``start``, one source per entry — ``local`` (a point index, or -1) or (``rank``, ``pos``) —
  in ascending global point number, and this rank's ``send`` list; groups ascend with their first
  local member.  Purely local groups of two or more are part of it; an empty shard has an empty plan.

The extent behind ``tol = rel_tol * extent`` is taken over all ranks, so every rank uses the one-rank
grid.  Out of scope, as for ``FaceAverage``: periodic boundaries (the coordinates do not coincide)
and non-conforming meshes.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .seeds import group_ids
from .vector import NekContext, NekVector

_NAMES = ("x", "y", "z")


@dataclass
class GsPlan:
    """One rank's gather-scatter plan (host arrays, int64)."""
    start: np.ndarray    # CSR offsets, n_groups + 1
    local: np.ndarray    # per entry: local point index, or -1 for a remote member
    rank: np.ndarray     # per entry: the owning rank of a remote member, or -1
    pos: np.ndarray      # per entry: position in that rank's send list, or -1
    send: np.ndarray     # this rank's send list: local point indices, ascending
    n_send: np.ndarray   # every rank's send count (the exchange is padded to the largest)

    @property
    def n_groups(self) -> int:
        return self.start.size - 1


def _dense(gid: np.ndarray) -> np.ndarray:
    if gid.size == 0:
        return gid.astype(np.int64)
    return np.unique(gid, return_inverse=True)[1].reshape(-1).astype(np.int64)


def face_templates(lx1: int, ldim: int):
    """(corners, faces): for each of the 2 ldim faces of an element, the in-element indices of its
    2^(ldim-1) corner points and of all its lx1^(ldim-1) points (Nek order, il fastest)."""
    idx = np.arange(lx1 ** ldim).reshape((lx1,) * ldim)
    corners, faces = [], []
    for ax in range(ldim):
        for side in (0, lx1 - 1):
            f = np.take(idx, side, axis=ax)
            faces.append(f.ravel())
            c = f
            for a in range(ldim - 1):
                c = np.take(c, [0, lx1 - 1], axis=a)
            corners.append(c.ravel())
    return np.array(corners), np.array(faces)


def candidate_points(gid: np.ndarray, lx1: int, ldim: int) -> np.ndarray:
    """The exposed-face rule (module docstring): ascending local indices of the points whose local
    group (``gid``: dense ids, one per point) has a member on an element face without a local
    neighbour."""
    pts = lx1 ** ldim
    if gid.size == 0:
        return np.zeros(0, np.int64)
    if gid.size % pts:
        raise ValueError(f"{gid.size} points are no multiple of lx1^ldim = {pts}")
    g = gid.reshape(-1, pts)
    corners, faces = face_templates(lx1, ldim)
    keys = np.sort(g[:, corners], axis=2)                          # (nel, nfaces, ncorners)
    _, inv, counts = np.unique(keys.reshape(-1, keys.shape[2]), axis=0, return_inverse=True, return_counts=True)
    exposed = (counts[inv.reshape(-1)] == 1).reshape(g.shape[0], -1)
    flag = np.zeros(int(gid.max()) + 1, dtype=bool)
    for f in range(faces.shape[0]):
        flag[g[exposed[:, f]][:, faces[f]]] = True
    return np.flatnonzero(flag[gid]).astype(np.int64)


def local_setup(coords: dict, lx1: int, ldim: int, tol: float, first_gnum: int) -> dict:
    """Steps 1 and 2 on one rank: ``gid`` (dense local group ids), ``cand`` (candidate points,
    ascending), their coordinates ``xyz`` (ldim x k) and global point numbers ``gnum`` (k)."""
    xs = [np.ascontiguousarray(coords[k], dtype=np.float64).ravel() for k in _NAMES[:ldim]]
    if any(x.size != xs[0].size for x in xs):
        raise ValueError("coords: the coordinate arrays differ in length")
    gid = _dense(group_ids(xs, tol))
    cand = candidate_points(gid, lx1, ldim)
    xyz = np.stack([x[cand] for x in xs]) if xs[0].size else np.zeros((ldim, 0))
    return dict(gid=gid, cand=cand, xyz=xyz, gnum=cand + int(first_gnum), tol=float(tol),
                first_gnum=int(first_gnum))


def build_plan(rank: int, local: dict, gathered) -> GsPlan:
    """Step 4 on rank ``rank``: ``local`` is its :func:`local_setup`, ``gathered`` every rank's
    (``xyz``, ``gnum``) in rank order (its own included)."""
    gid, first = local["gid"], local["first_gnum"]
    n = gid.size
    world = len(gathered)
    ks = np.array([np.asarray(g[1]).size for g in gathered], dtype=np.int64)
    a_gnum = np.concatenate([np.asarray(g[1], dtype=np.int64) for g in gathered])
    a_rank = np.repeat(np.arange(world, dtype=np.int64), ks)
    ldim = np.asarray(gathered[rank][0]).shape[0]
    a_xyz = np.concatenate([np.asarray(g[0], dtype=np.float64).reshape(ldim, -1) for g in gathered], axis=1)
    if a_gnum.size and np.any(np.diff(a_gnum) <= 0):
        raise ValueError("gather-scatter: the gathered global point numbers do not ascend (overlapping shards?)")
    cg = _dense(group_ids([a_xyz[c] for c in range(ldim)], local["tol"]))
    ncg = int(cg.max()) + 1 if cg.size else 0
    lo, hi = np.full(ncg, world, np.int64), np.full(ncg, -1, np.int64)
    np.minimum.at(lo, cg, a_rank)
    np.maximum.at(hi, cg, a_rank)
    shared = (lo != hi)[cg] if cg.size else np.zeros(0, bool)       # per candidate: its group spans ranks
    # every rank's send list: its shared candidates, ascending; a candidate's position in it
    offs = np.r_[0, np.cumsum(ks)]
    csum = np.cumsum(shared)
    before = np.r_[0, csum][offs[:-1]]                              # shared candidates of lower ranks
    a_pos = csum - 1 - before[a_rank]
    n_send = np.array([int(np.count_nonzero(shared[offs[r]:offs[r + 1]])) for r in range(world)], dtype=np.int64)
    own = slice(offs[rank], offs[rank + 1])
    send = (a_gnum[own][shared[own]] - first).astype(np.int64)
    # (a) shared groups with a member here: every candidate of the group, from every rank
    here = np.zeros(ncg, dtype=bool)
    here[cg[own][shared[own]]] = True
    ent = np.flatnonzero(here[cg]) if cg.size else np.zeros(0, np.int64)
    e_own = a_rank[ent] == rank
    e_local = np.where(e_own, a_gnum[ent] - first, -1)
    key_of = np.full(ncg, np.iinfo(np.int64).max, np.int64)        # a group's first local member
    np.minimum.at(key_of, cg[ent][e_own], e_local[e_own])
    e_key, e_gnum = key_of[cg[ent]], a_gnum[ent]
    e_rank = np.where(e_own, -1, a_rank[ent])
    e_pos = np.where(e_own, -1, a_pos[ent])
    # (b) groups of two or more whose members are all here
    in_shared = np.zeros(n, dtype=bool)
    in_shared[send] = True
    if n:
        counts = np.bincount(gid)
        idx = np.flatnonzero((counts[gid] > 1) & ~in_shared)
        first_of = np.full(counts.size, n, np.int64)
        np.minimum.at(first_of, gid[idx], idx)
        e_key = np.r_[e_key, first_of[gid[idx]]]
        e_gnum = np.r_[e_gnum, idx + first]
        e_local = np.r_[e_local, idx]
        e_rank = np.r_[e_rank, np.full(idx.size, -1, np.int64)]
        e_pos = np.r_[e_pos, np.full(idx.size, -1, np.int64)]
    order = np.lexsort((e_gnum, e_key))
    e_key, e_local, e_rank, e_pos = e_key[order], e_local[order], e_rank[order], e_pos[order]
    starts = np.flatnonzero(np.r_[True, e_key[1:] != e_key[:-1]]) if e_key.size else np.zeros(0, np.int64)
    if e_local.size and (e_local.max() >= n or np.any((e_rank >= 0) & (e_pos >= n_send[np.maximum(e_rank, 0)]))):
        raise ValueError("gather-scatter: a plan entry points outside its shard or send list")
    return GsPlan(np.r_[starts, e_key.size].astype(np.int64), e_local.astype(np.int64), e_rank.astype(np.int64),
                  e_pos.astype(np.int64), send, n_send)


def as_gather_scatter(f):
    """``f`` if it is a :class:`GatherScatter`, its owner if ``f`` is a bound method of one (``gs.apply``),
    else None: the consumers batch their averaging through ``apply_many`` for these."""
    if isinstance(f, GatherScatter):
        return f
    owner = getattr(f, "__self__", None)
    return owner if isinstance(owner, GatherScatter) else None


def auto_average(ctx: NekContext, coords: dict):
    """The consumers' ``"auto"``: ``seeds.FaceAverage(...).apply`` on one rank (unchanged, bit for bit),
    a :class:`GatherScatter` over the shards on several (collective)."""
    if ctx.comm.world > 1:
        return GatherScatter(ctx, coords)
    from .seeds import FaceAverage

    return FaceAverage(ctx, coords).apply


def average_segments(face_average, ptrs) -> None:
    """``dsavg`` of the field segments at ``ptrs``: one batched ``apply_many`` for a gather-scatter
    (collective: an empty shard takes part), else ``face_average(ptr)`` per segment."""
    gs = as_gather_scatter(face_average)
    if gs is not None:
        gs.apply_many(ptrs)
        return
    for p in ptrs:
        face_average(p)


class GatherScatter:
    """``dssum`` + ``vmult`` / ``dsavg`` over this rank's shard and its neighbours': a drop-in for
    ``seeds.FaceAverage`` at any world size.  Construction is collective at world > 1 (the extent's
    min/max, one all-gather of the candidates); a rank that fails reports through
    ``comm.raise_if_any`` so no peer waits in a collective.  ``coords``: this rank's GLL coordinates
    {"x", "y"[, "z"]} (n_v each)."""

    MAX_FIELDS = _lib.NKV_GS_MAX_FIELDS

    def __init__(self, ctx: NekContext, coords: dict, rel_tol: float = 1e-9):
        comm, lay = ctx.comm, ctx.layout
        self.ctx = ctx
        self.world, self.n_v = comm.world, lay.n_v
        ldim = lay.ldim
        err, mins, maxs = None, [np.inf] * ldim, [-np.inf] * ldim
        try:
            xs = [np.asarray(coords[k], dtype=np.float64).ravel() for k in _NAMES[:ldim]]
            for k, x in zip(_NAMES, xs):
                if x.size != lay.n_v:
                    raise ValueError(f"coords[{k!r}]: {x.size} points, the layout has n_v={lay.n_v}")
            if lay.n_v > np.iinfo(np.int32).max:
                raise ValueError(f"n_v={lay.n_v} does not fit the gather-scatter's 32-bit indices")
            if lay.n_v:
                mins, maxs = [float(x.min()) for x in xs], [float(x.max()) for x in xs]
        except Exception as e:   # noqa: BLE001  (agreed on below: no peer is left in a collective)
            err = e
        comm.raise_if_any(err)
        ext = 0.0
        for c in range(ldim):
            lo = comm.min_scalar(mins[c], device=ctx.device)
            hi = comm.max_scalar(maxs[c], device=ctx.device)
            if hi >= lo:
                ext = max(ext, hi - lo)
        tol = rel_tol * (ext or 1.0)
        local = None
        try:
            local = local_setup(coords, lay.lx1, ldim, tol, lay.elem_range()[0] * lay.pts_v)
        except Exception as e:   # noqa: BLE001
            err = e
        comm.raise_if_any(err)
        gathered = [(local["xyz"], local["gnum"])]
        if self.world > 1:
            gathered = self._gather_candidates(local, ldim)
        plan = None
        try:
            plan = build_plan(comm.rank, local, gathered)
            self.stride = int(plan.n_send.max()) if plan.n_send.size else 0
            if self.stride * self.world > np.iinfo(np.int32).max:
                raise ValueError(f"{self.world} ranks x {self.stride} shared points do not fit the 32-bit indices")
        except Exception as e:   # noqa: BLE001
            err = e
        comm.raise_if_any(err)
        self.plan = plan
        self.n_groups, self.n_send = plan.n_groups, int(plan.send.size)
        self.n_candidates = int(local["cand"].size)
        src = np.where(plan.local >= 0, plan.local, -(1 + plan.rank * self.stride + plan.pos))

        def dev(a):
            a = np.asarray(a, dtype=np.int32)
            return torch.as_tensor(a if a.size else np.zeros(1, np.int32)).to(ctx.device)

        self.start, self.src, self.send_idx = dev(plan.start), dev(src), dev(plan.send)
        self._send = self._recv = None

    def _gather_candidates(self, local: dict, ldim: int):
        ctx, comm = self.ctx, self.ctx.comm
        k = int(local["cand"].size)
        kmax = int(comm.max_scalar(float(k), device=ctx.device))
        if kmax == 0:
            return [(np.zeros((ldim, 0)), np.zeros(0, np.int64)) for _ in range(self.world)]
        xyz = np.zeros((ldim, kmax))
        xyz[:, :k] = local["xyz"]
        gnum = np.full(kmax, -1, np.int64)
        gnum[:k] = local["gnum"]
        xs, gs = torch.as_tensor(xyz).to(ctx.device), torch.as_tensor(gnum).to(ctx.device)
        xo = torch.empty(self.world * ldim * kmax, dtype=torch.float64, device=ctx.device)
        go = torch.empty(self.world * kmax, dtype=torch.int64, device=ctx.device)
        comm.allgather_(xs, xo)
        comm.allgather_(gs, go)
        xo, go = xo.cpu().numpy().reshape(self.world, ldim, kmax), go.cpu().numpy().reshape(self.world, kmax)
        out = []
        for r in range(self.world):
            kr = int(np.count_nonzero(go[r] >= 0))
            out.append((xo[r, :, :kr].copy(), go[r, :kr].copy()))
        return out

    def _buffers(self, nf: int):
        need = nf * self.stride
        if self._send is None or self._send.numel() < need:
            f64 = dict(dtype=torch.float64, device=self.ctx.device)
            self._send = torch.zeros(max(need, 1), **f64)
            self._recv = torch.zeros(max(self.world * need, 1), **f64)
        return self._send[:need], self._recv[: self.world * need]

    def apply(self, ptr: int) -> None:
        """Average one field segment (n_v points at device address ``ptr``) in place."""
        self.apply_many([ptr])

    def apply_many(self, ptrs) -> None:
        """Average the field segments at the device addresses ``ptrs`` in place: per round of up to
        ``MAX_FIELDS`` segments one pack, one exchange and one average launch.  Collective at world > 1
        (every rank passes as many segments; an empty shard's addresses are not read)."""
        ptrs = [int(p) for p in ptrs]
        ctx = self.ctx
        if self.world > 1 and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GatherScatter: the exchange at world > 1 cannot be captured into a HIP graph")
        for i in range(0, len(ptrs), self.MAX_FIELDS):
            chunk = ptrs[i:i + self.MAX_FIELDS]
            nf = len(chunk)
            arr = (ctypes.c_void_p * nf)(*chunk)
            recv_ptr = None
            if self.world > 1 and self.stride:
                send, recv = self._buffers(nf)
                ctx.call_nl("nkv_gs_pack", nf, arr, self.n_v, self.n_send, self.send_idx.data_ptr(), self.stride,
                            send.data_ptr(), ctx.stream)
                ctx.comm.allgather_(send, recv)
                recv_ptr = recv.data_ptr()
            ctx.call_nl("nkv_gs_average", nf, arr, self.n_v, self.n_groups, self.start.data_ptr(),
                        self.src.data_ptr(), recv_ptr, self.stride if recv_ptr else 0, self.world, ctx.stream)

    def __call__(self, vec: NekVector, fields) -> None:
        sv = self.ctx.layout.sv
        self.apply_many([vec.ptr + 8 * f * sv for f in fields])


__all__ = ["GatherScatter", "GsPlan", "local_setup", "build_plan", "candidate_points", "face_templates",
           "as_gather_scatter", "average_segments", "auto_average"]
