"""The checkpointed adjoint of the periodic-orbit tangent (nekstab_next_amd/orbit.py, nkv_burgers_backward_rhs), CPU
side: the backward walk ``checkpoint_schedule`` as a pure list of operations, replayed here on a model of the two
windows, and what the package checks without a GPU (header, ctypes table, the "auto" segment length).

The model: a window holds at most one segment; "recompute" fills a window from the segment's own checkpoint, a
"pair" runs the adjoint of one segment out of its window while it fills the other window with the segment before,
the steps past the paired ones following unfused.  Replaying a schedule must run the adjoint of every step exactly
once in the order N-1 ... 0, each about a window that holds its segment."""
import os
import re

import pytest

from nekstab_next_amd.orbit import auto_checkpoint, checkpoint_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NS = (1, 2, 7, 8, 50)


def _cs(N):
    return sorted({1, 2, 3, 4, 7, 9, N, N + 1})


def _span(N, c, j):
    return j * c, min((j + 1) * c, N)


def _replay(N, c, ops):
    """Run the operations on the model; returns the adjoint steps in the order they ran."""
    J = -(-N // c)
    cap = min(c, N)
    window = [None, None]          # the segment each window holds
    ran = []

    def fill(j, w, steps):
        assert 0 <= j < J and w in (0, 1)
        assert steps == _span(N, c, j)[1] - _span(N, c, j)[0]      # from its own checkpoint, the whole segment
        assert steps <= cap                                        # a window never holds more than min(c, N) steps
        window[w] = j

    def adjoint(j, w):
        assert window[w] == j, f"the adjoint of segment {j} runs about window {w}, which holds {window[w]}"
        start, end = _span(N, c, j)
        ran.extend(range(end - 1, start - 1, -1))

    for op in ops:
        assert op[0] in ("recompute", "adjoint", "pair"), op
        if op[0] == "recompute":
            _, j, w = op
            fill(j, w, _span(N, c, j)[1] - _span(N, c, j)[0])
        elif op[0] == "adjoint":
            _, j, w = op
            adjoint(j, w)
        else:
            _, ja, jr, k = op
            assert jr == ja - 1 >= 0
            la = _span(N, c, ja)[1] - _span(N, c, ja)[0]
            lr = _span(N, c, jr)[1] - _span(N, c, jr)[0]
            assert 1 <= k <= min(la, lr)                           # never more steps than either segment has
            assert k == la                                         # the adjoint of ja ends inside the pair
            assert (ja & 1) != (jr & 1)                            # two windows, two segments
            assert window[ja & 1] == ja
            adjoint(ja, ja & 1)
            fill(jr, jr & 1, lr)                                   # k paired steps, lr - k unfused
        assert sum(w is not None for w in window) <= 2
    return ran


@pytest.mark.parametrize("fused", [False, True], ids=["sequential", "pipelined"])
@pytest.mark.parametrize("N", NS)
def test_schedule_runs_every_adjoint_step_once_backwards(N, fused):
    for c in _cs(N):
        ops = checkpoint_schedule(N, c, fused=fused)
        J = -(-N // c)
        assert _replay(N, c, ops) == list(range(N - 1, -1, -1)), (N, c)
        kinds = [op[0] for op in ops]
        if fused:
            assert kinds == ["recompute"] + ["pair"] * (J - 1) + ["adjoint"], (N, c, ops)
            assert ops[0] == ("recompute", J - 1, (J - 1) & 1) and ops[-1] == ("adjoint", 0, 0)
            # only the last segment is shorter than c: every pair but the first pairs c steps
            assert [op[3] for op in ops[1:-1]] == ([N - (J - 1) * c] + [c] * (J - 2) if J > 1 else [])
        else:
            assert kinds == ["recompute", "adjoint"] * J, (N, c, ops)
            assert [op[1] for op in ops[::2]] == list(range(J - 1, -1, -1))
        # every segment is filled exactly once per walk
        filled = [op[1] for op in ops if op[0] == "recompute"] + [op[2] for op in ops if op[0] == "pair"]
        assert sorted(filled) == list(range(J))
        assert checkpoint_schedule(N, c) == checkpoint_schedule(N, c, fused=True)  # pipelined is the function's default


@pytest.mark.parametrize("N", NS + (3, 9, 100, 1000, 20000))
def test_auto_segment_length(N):
    c = max(1, round((N / 8) ** 0.5))
    assert auto_checkpoint(N) == c
    assert checkpoint_schedule(N, "auto") == checkpoint_schedule(N, c)
    assert checkpoint_schedule(N, "auto", fused=False) == checkpoint_schedule(N, c, fused=False)
    # the slots of checkpoints, windows and the side-by-side matvec stay below the stored orbit's once N > 8
    J = -(-N // c)
    slots = J + 8 * min(c, N) + 4
    if N >= 20:
        assert slots < 4 * N
    if N >= 100:
        assert slots <= 5.7 * N ** 0.5 + 8


def test_schedule_refuses_bad_arguments():
    for bad in (0, -1, 1.5, True, "auto3", None):
        with pytest.raises(ValueError, match="checkpoint"):
            checkpoint_schedule(7, bad)
    for bad in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="nsteps"):
            checkpoint_schedule(bad, 2)


def test_header_and_bindings():
    """nkv_burgers_backward_rhs: declared, exported and typed with the argument count of the header's prototype;
    nkv_burgers_tangent_rhs with one more state (S, S_stride) after the first."""
    from nekstab_next_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "nekkrylov.h")).read()
    name = "nkv_burgers_backward_rhs"
    assert re.search(r"\bint %s\(" % name, hdr), name
    assert name in _lib.EXPORTED
    decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
    assert decl.count(",") + 1 == len(_lib._SIGNATURES[name][1]) == 21
    bt, bb = _lib._SIGNATURES["nkv_burgers_tangent_rhs"][1], _lib._SIGNATURES[name][1]
    assert bb[:10] == bt[:10] and bb[10:12] == bt[8:10] and bb[12:] == bt[10:]
    assert _lib.NKV_ABI_VERSION == 3
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, name) and lib.nkv_abi_version() == 3
    import nekstab_next_amd

    assert nekstab_next_amd.checkpoint_schedule is checkpoint_schedule


def test_docstrings_name_the_way_out():
    from nekstab_next_amd import orbit

    assert "checkpoint=" in orbit.OrbitFlow.__doc__ and "4·nsteps·n_wf·sv·8" in orbit.OrbitFlow.__doc__
    assert "rmatvec`` needs the whole orbit stored" not in orbit.__doc__
    assert "nkv_burgers_backward_rhs" in orbit.__doc__
