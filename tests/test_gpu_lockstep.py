"""The four NLPs of a wavefront of the persistent kernel p_solve and their line searches.

A wavefront of the four-per-wavefront form carries four NLPs through trial point / factorisation / solves in rounds; an NLP
whose step the Armijo test rejects is tried again at half the step inside the trial phase of the same round while its mates
wait.  That changes when an NLP's operations run, never which: every NLP must come out with the bits it has when solved alone,
and with the iteration counts of the C restatement (oracle/ascent_oracle.c), which runs the same algorithm one NLP at a time.

The inputs are rows of the bench's workload -- the 64 x 64 Isp x dry-mass sweep with DCOST = 1e-5, move penalty on, tol 1e-9,
cold start (nested iteration 17 -> 60 -> 200) -- picked by the rejections the oracle's line search counts on each level:

    rows 2700-2703   iterations (11,4,10) (11,4,10) (11,4,11) (11,4,10); row 2702 rejects three times in fine iteration 9,
                     its mates never: one NLP retries three times while three wait
    rows 3508-3511   iterations (11,4,12) (11,4,10) (11,4,11) (11,4,11); fine-level rejections 2 (iterations 5, 6) / 0 / 1 / 1
                     (iteration 9): retries at different rounds
    rows 2800-2803   iterations (11,4,12) (9,4,12) (9,4,12) (9,4,12); rejections on the 17-node level 2 / 1 / 1 / 1, on the fine
                     level 1 / 0 / 0 / 2: mates out of step on the coarse level too
    rows 2700-2706   rows 2704-2706: (11,4,10), fine-level rejections (2,0,0): a second wavefront with a dead group
    rows 0-3 at nt = 17 on a single grid: every NLP rejects once in iterations 1 and 5 (everyone retries together)

No case comes near a line-search failure (40 rejections in one iteration)."""
import numpy as np
import pytest

import lunar_module_ascent_trajectory_optimiser_amd as A
from oracle import c_oracle

GROUPS = {"one_retries_three_wait": (2700, 2704), "retries_at_different_rounds": (3508, 3512), "coarse_level_out_of_step": (2800, 2804),
          "second_wavefront_dead_group": (2700, 2707)}
ORACLE_ITERS = {"one_retries_three_wait": [25, 25, 26, 25], "retries_at_different_rounds": [27, 25, 26, 26],
                "coarse_level_out_of_step": [27, 25, 25, 25]}
KW = dict(tol=1e-9, move_penalty=True)


def _sweep():
    S = A.sweep_isp_drymass(64, 64).copy()
    S[:, 15] = 1e-5
    return S


@pytest.fixture(scope="module")
def solved():
    """Every group as one batch and every row of a group alone, four NLPs per wavefront (a batch of 1: three dead groups), solved
    once for the module; the oracle's solutions of the same rows."""
    S = _sweep()
    mp = pytest.MonkeyPatch()
    mp.setenv("ASCENT_PERSIST_WIDE", "0")
    try:
        assert A.default_path(4, 200, move_penalty=True) == "persist" and A.default_path(1, 200, move_penalty=True) == "persist"
        group = {name: A.solve_batch(S[a:b], 200, **KW) for name, (a, b) in GROUPS.items()}
        rows = sorted({i for a, b in GROUPS.values() for i in range(a, b)})
        alone = {i: A.solve_batch(S[i:i + 1], 200, **KW) for i in rows}
        coarse = (A.solve_batch(S[0:4], 17, coarse_nodes=-1, **KW), [A.solve_batch(S[i:i + 1], 17, coarse_nodes=-1, **KW) for i in range(4)])
    finally:
        mp.undo()
    ref = {name: c_oracle.solve_batch(S[a:b], 200, 300, 1e-9, move_penalty=True) for name, (a, b) in GROUPS.items()}
    ref17 = c_oracle.solve_batch(S[0:4], 17, 300, 1e-9, move_penalty=True, coarse_nodes=-1)
    return dict(S=S, group=group, alone=alone, coarse=coarse, ref=ref, ref17=ref17)


def _same_bits(batch, singles):
    for j, one in enumerate(singles):
        assert one.status[0] == 0 and batch.status[j] == 0, (j, one.status, batch.status)
        assert batch.iters[j] == one.iters[0], (j, batch.iters, one.iters)
        assert np.array_equal(batch.tf[j:j + 1], one.tf), (j, batch.tf[j], one.tf[0], batch.tf[j] - one.tf[0])
        assert np.array_equal(batch.traj[:, :, j], one.traj[:, :, 0]), (j, np.abs(batch.traj[:, :, j] - one.traj[:, :, 0]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GROUPS))
def test_a_mate_changes_nothing(solved, name):
    """Each group solved as one batch gives, NLP by NLP, the bits of that row solved alone in the same form: status, iteration
    count, t_f and the whole trajectory.  No arithmetic crosses a 16-lane group, and a retry inside the trial phase only moves an
    NLP's operations in time."""
    a, b = GROUPS[name]
    _same_bits(solved["group"][name], [solved["alone"][i] for i in range(a, b)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GROUPS))
def test_same_iterates_as_the_oracle(solved, name):
    """Iteration counts of every group equal the C restatement's (which solves one NLP at a time, retrying a rejected step at
    once), and t_f agrees to the 3e-10 relative that bench.py's live parity check reports."""
    r, ref = solved["group"][name], solved["ref"][name]
    assert np.all(ref["status"] == 0) and np.all(r.status == 0), (ref["status"], r.status)
    print(name, "iters", r.iters, "oracle", ref["iters"], "rel tf", np.abs(r.tf - ref["tf"]) / ref["tf"])
    assert np.array_equal(r.iters, ref["iters"]), (r.iters, ref["iters"])
    if name in ORACLE_ITERS:
        assert list(r.iters) == ORACLE_ITERS[name], r.iters
    assert (np.abs(r.tf - ref["tf"]) / ref["tf"]).max() <= 3e-10


@pytest.mark.gpu
def test_single_coarse_grid_everyone_rejects_together(solved):
    """Rows 0-3 on 17 nodes, single grid: every NLP rejects once in iterations 1 and 5, so all four retry in the same pass."""
    batch, singles = solved["coarse"]
    ref = solved["ref17"]
    assert np.all(batch.status == 0) and np.all(ref["status"] == 0), (batch.status, ref["status"])
    assert np.array_equal(batch.iters, ref["iters"]), (batch.iters, ref["iters"])
    _same_bits(batch, singles)


@pytest.mark.gpu
def test_both_forms(solved, monkeypatch):
    """The first group with one NLP per wavefront (where a retry follows its rejection at once in either build): the same
    iteration counts and t_f to 1e-12, the tolerance of test_one_nlp_per_wavefront_equals_four_per_wavefront."""
    a, b = GROUPS["one_retries_three_wait"]
    monkeypatch.setenv("ASCENT_PERSIST_WIDE", "1")
    wide = A.solve_batch(solved["S"][a:b], 200, **KW)
    four = solved["group"]["one_retries_three_wait"]
    assert np.all(wide.status == 0)
    assert np.array_equal(wide.iters, four.iters), (wide.iters, four.iters)
    assert np.abs(wide.tf - four.tf).max() <= 1e-12
