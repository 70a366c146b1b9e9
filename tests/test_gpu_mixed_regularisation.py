"""GPU test of the regularisation block in p_solve's backward factor step: the wavefront skips the block when none of its NLPs is
regularised (one test on the whole wavefront), and inside it every lane still decides for itself.  What that can break: a mate's
delta_w = 0 must not switch a lane's regularisation off, and a mate's delta_w != 0 must not add +0.0 to a lane whose entry is -0.0.

One Newton step (A.kkt_step on the persistent path: one round of p_solve) for a wavefront's worth of problems whose mates carry
different delta_w, against the same problem run ALONE with its own delta_w: step and inertia flag bit for bit (compared as 64-bit
patterns, so that -0.0 and +0.0 differ).  A refused step is reported as zeros with inertia 1, so it compares like any other.

Cases: delta_w patterns [0, 1e-2, 0, 1e-4] (mixed), all zero, all 1e-2; grids nt = 18 (17 nodes: a full chunk and one node) and
nt = 34 (33 nodes: three chunks, the last one partial), and nt = 17 (16 nodes: exactly one chunk); batches 4 and 5 (a second
wavefront with three dead groups, which shadow the last NLP); with and without the move penalty; four NLPs and one NLP per wavefront
(ASCENT_PERSIST_WIDE, as test_gpu_lockstep.py::test_both_forms forces them).  The iterates are those of the other step tests
(test_terminal_step_reference.blob_of: a few oracle iterations from the cold start, multipliers perturbed)."""
import functools

import numpy as np
import pytest

import lunar_module_ascent_trajectory_optimiser_amd as A
from test_terminal_step_reference import MU, blob_of, problems

pytestmark = pytest.mark.gpu

PATTERNS = {"mixed": (0.0, 1e-2, 0.0, 1e-4), "none": (0.0, 0.0, 0.0, 0.0), "all": (1e-2, 1e-2, 1e-2, 1e-2)}
GRIDS = (17, 18, 34)
BATCHES = (4, 5)


def _step(wide, S, blobs, mu, dw, nt, mp):
    """(step, inertia) of one round of p_solve in the given wavefront form, as 64-bit patterns / int32"""
    with pytest.MonkeyPatch.context() as m:
        m.setenv("ASCENT_PERSIST_WIDE", str(wide))
        step, inertia = A.kkt_step(S, blobs, mu, dw, nt, path="persist", move_penalty=mp)
    return np.ascontiguousarray(step).view(np.uint64), inertia


@functools.lru_cache(maxsize=None)
def _alone(wide, nt, b, dw, mp):
    """problem b in a batch of one with its own delta_w (computed once, shared by the cases)"""
    blob = np.array(blob_of(nt, 0, b))
    bits, inertia = _step(wide, problems()[b:b + 1], blob[:, None], MU[b:b + 1].copy(), np.array([dw]), nt, mp)
    bits.setflags(write=False)
    return bits[:, 0], int(inertia[0])


@pytest.mark.parametrize("wide", [0, 1], ids=["four_per_wavefront", "one_per_wavefront"])
@pytest.mark.parametrize("mp", [False, True], ids=["plain", "penalty"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("nt", GRIDS)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_step_equals_the_problem_alone(pattern, nt, B, mp, wide):
    S = problems()[:B]
    blobs = np.stack([blob_of(nt, 0, b) for b in range(B)], axis=1)
    dw = np.resize(np.array(PATTERNS[pattern]), B)
    bits, inertia = _step(wide, S, blobs, MU[:B].copy(), dw, nt, mp)
    for b in range(B):
        ref_bits, ref_inertia = _alone(wide, nt, b, float(dw[b]), mp)
        assert inertia[b] == ref_inertia, (b, inertia[b], ref_inertia)
        diff = np.flatnonzero(bits[:, b] != ref_bits)
        assert diff.size == 0, (b, float(dw[b]), diff[:8], diff.size)


@pytest.mark.parametrize("wide", [0, 1], ids=["four_per_wavefront", "one_per_wavefront"])
@pytest.mark.parametrize("mp", [False, True], ids=["plain", "penalty"])
def test_the_regularisation_enters_the_step(mp, wide):
    """The comparison above says something only if delta_w changes the step: on every grid a regularised problem of the mixed
    pattern whose step is accepted gets another step (or is refused) without its delta_w."""
    for nt in GRIDS:
        changed = 0
        for b in (1, 3):
            with_dw, in_dw = _alone(wide, nt, b, PATTERNS["mixed"][b], mp)
            without, in_0 = _alone(wide, nt, b, 0.0, mp)
            changed += in_dw == 0 and (in_0 != 0 or bool(np.any(with_dw != without)))
        assert changed >= 1, nt
