"""The independent reference of the terminal block of the Newton step (tests/terminal_step_reference.py) checked on the CPU
before any kernel is held to it: at terminal 0 it is conftest.generic_lu_newton_step bit for bit and agrees with the C oracle;
at every case of the table below -- the table tests/test_gpu_terminal_step.py runs the kernels on -- the KKT matrix has the
inertia the case says, the reference's own float64 error is a hundredth of the 1e-8 the kernels are held to, and a step
computed without the terminal constraints' Hessian is at least a hundred times that bound away from it."""
import collections
import functools

import numpy as np
import pytest

import lunar_module_ascent_trajectory_optimiser_amd as A
from conftest import generic_lu_newton_step, params_of_row
from terminal_step_reference import lu_newton_step, sections, stagewise_inertia_ok

# ---- the problems: five of a 2 x 3 Isp x dry-mass sweep (the GPU file runs the first three and all five), each with its own
# barrier parameter, regularisation (0 and 1.0 among the first three) and move-penalty weight
N_PROBLEMS = 5
MU = np.array([0.1, 0.02, 1e-3, 0.05, 1e-6])
DW = np.array([0.0, 1.0, 1e-2, 1e-3, 1e-4])
DCOST = np.array([1e-5, 1e-5, 1e-3, 1e-4, 1e-2])
# On the grids of 64 and 65 intervals the generic LU's own float64 error with delta_w = 1.0 is 0.4 .. 7e-10 of the section's
# scale, for every one of the five problems and at every iterate tried (1 .. 8 oracle iterations, eleven seeds, the twelve
# systems of a grid): at the 1e-10 gate of test_every_case_is_fit_to_judge_a_kernel or past it, never a factor of three
# inside.  So the second problem carries 0.1 there (3e-11 and less); p_solve's one-NLP-per-wavefront form still meets 1.0
# on its three-node grid, the four-per-wavefront form and h_solve's two forms on all of theirs.
DW_LONG = np.array([0.0, 0.1, 1e-2, 1e-3, 1e-4])


def dw_of(nt, b):
    return (DW_LONG if nt - 1 >= 64 else DW)[b]


# terminal multipliers nu3, nu1, nu2 of problem b: NU * (1 + b/10) -- distinct, O(0.1 - 1), nu1 and nu2 with the sign they have at
# a solution of every terminal mode (both conditions are active inequalities g - s = 0, s >= 0: nu = -z_s < 0)
NU = np.array([0.3, -0.7, -0.45])


def problems():
    S = A.sweep_isp_drymass(2, 3)[:N_PROBLEMS].copy()
    S[:, 15] = DCOST
    return S


# ---- the iterates: (oracle iterations from the cold start, seed of the perturbation) of problem b on an nt-node grid of a
# scheme; one iterate serves every terminal mode, with and without the penalty.  The rule is _interior_blobs' (3 + b % 4
# iterations, seed 300 + b); ITERATE lists the iterates exchanged for another, never skipped: those at which one of the
# systems has the wrong inertia (problem 0 carries no regularisation; problem 3 on the three-node grids), those at which the
# reference's own error comes within a factor of three of the 1e-10 gate below or misses it (the three-node Hermite-Simpson
# iterate of problem 2 after five iterations: a step of 1e6, an error of 9e-10 of it), and those at which the inertia is right
# but a stage-wise factorisation cannot certify it (problem 4 on the 64- and 65-interval grids after three
# iterations; four serve: SUFFICIENT_ONLY below keeps one of them).
def _default_iterate(b):
    return 3 + b % 4, 300 + b


ITERATE = {(3, 0, 3): (3, 303), (3, 1, 3): (3, 303), (3, 2, 3): (3, 303), (3, 2, 2): (3, 302),
           (49, 2, 0): (4, 300), (50, 2, 0): (4, 300), (65, 0, 0): (4, 300), (65, 1, 0): (4, 300), (66, 0, 0): (4, 300), (66, 1, 0): (4, 300),
           (65, 0, 4): (4, 304), (66, 0, 4): (4, 304), (66, 1, 1): (5, 301)}
# (nt, scheme, problem, iterate): the KKT matrix has the right inertia, its block without t_f and nu3 has not
SUFFICIENT_ONLY = (65, 0, 4, (3, 304))


def iterate_of(nt, scheme, b):
    return ITERATE.get((nt, scheme, b), _default_iterate(b))


@functools.lru_cache(maxsize=None)
def _blob(nt, scheme, b, flipped, iterate):
    from oracle import c_oracle
    c_oracle.build()
    iters, seed = iterate
    K = nt - 1
    rng = np.random.default_rng(seed)
    r = c_oracle.solve_batch(problems()[b][None], nt, iters, 1e-9, want_blob=True, coarse_nodes=-1, scheme=min(scheme, 1))
    c_oracle.set_scheme(0)
    blob = r["blob"][0].copy()
    blob[8 * K:15 * K] += 0.05 * rng.standard_normal(7 * K)              # lambda
    blob[15 * K:21 * K] *= rng.uniform(0.7, 1.3, 6 * K)                  # bound multipliers: off the central path
    blob[21 * K + 3:21 * K + 7] *= rng.uniform(0.7, 1.3, 4)              # s1 s2 z_s1 z_s2: strictly positive, off the central path
    blob[21 * K + 7:] = NU * (1.0 + 0.1 * b)
    if flipped:                                                          # strongly negative curvature: the wrong inertia
        blob[8 * K:15 * K] *= -50.0
    blob.setflags(write=False)
    return blob


def blob_of(nt, scheme, b, flipped=False, iterate=None):
    """The strictly interior primal-dual iterate of problem b (read-only, made once): a few iterations of the C oracle (terminal 0,
    the scheme itself or, for Hermite-Simpson, the trapezoid) from the cold start, multipliers perturbed as the other step
    tests perturb them -- and the terminal block's own unknowns too, so that the terminal Hessian and the slack rows enter."""
    return _blob(nt, scheme, b, flipped, iterate or iterate_of(nt, scheme, b))


# ---- the case table.  A case is one Newton system per problem: (grid, scheme, ascent_opts.terminal, move penalty); `flipped`
# marks the wrong-inertia cases (defect multipliers x -50, mu = 1e-6, no regularisation, problem 0 only).
Case = collections.namedtuple("Case", "nt scheme terminal mp flipped")
# the grids of each kernel form: three nodes, the last node of a chunk, one node past it (K = nt - 1 nodes carry unknowns)
GRIDS = {("p_solve", 0): (3, 17, 18), ("p_solve", 1): (3, 65, 66), ("h_solve", 0): (3, 13, 14), ("h_solve", 1): (3, 49, 50),
         "dense": (3, 14)}
_P_GRIDS = sorted(set(GRIDS["p_solve", 0] + GRIDS["p_solve", 1] + GRIDS["dense"]))
_H_GRIDS = sorted(set(GRIDS["h_solve", 0] + GRIDS["h_solve", 1] + GRIDS["dense"]))
CASES = ([Case(nt, scheme, term, mp, False) for scheme in (0, 1) for nt in _P_GRIDS for term in (0, 1, 2) for mp in (False, True)]
         + [Case(nt, 2, term, mp, False) for nt in _H_GRIDS for term in (0, 1, 2) for mp in (False, True) if not mp or nt in GRIDS["dense"]])
WRONG_INERTIA_NT = 18
WRONG_INERTIA_CASES = [Case(WRONG_INERTIA_NT, scheme, term, False, True) for scheme in (0, 2) for term in (0, 1, 2)]


def case_id(c):
    return f"nt{c.nt}-scheme{c.scheme}-terminal{c.terminal}-{'penalty' if c.mp else 'plain'}" + ("-flipped" if c.flipped else "")


@functools.lru_cache(maxsize=None)
def reference(case, b):
    """(step, inertia_ok, ref_err) of problem b of a case, computed once for every test that needs it (arrays read-only)."""
    if case.flipped:
        mu, dw = 1e-6, 0.0
    else:
        mu, dw = MU[b], dw_of(case.nt, b)
    step, ok, err = lu_newton_step(params_of_row(problems()[b]), case.nt, blob_of(case.nt, case.scheme, b, case.flipped), mu, dw,
                                   case.scheme, case.terminal, case.mp)
    step.setflags(write=False); err.setflags(write=False)
    return step, ok, err


def _section_scales(step, K):
    return np.array([max(1.0, np.abs(step[lo:hi]).max()) for lo, hi in sections(K)])


# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,mp", [(0, False), (1, False), (2, False), (0, True), (1, True), (2, True)])
def test_terminal0_is_the_generic_lu_of_conftest_bit_for_bit(scheme, mp):
    nt = 14
    for b in range(3):
        P = params_of_row(problems()[b])
        blob = np.array(blob_of(nt, scheme, b))
        ref = generic_lu_newton_step(P, nt, blob, MU[b], DW[b], scheme, move_penalty=mp)[0]
        step, _, _ = lu_newton_step(P, nt, blob, MU[b], DW[b], scheme, 0, mp)
        assert np.array_equal(step, ref)


@pytest.mark.parametrize("scheme", [0, 1])
def test_terminal0_agrees_with_the_c_oracle(coracle, scheme):
    """The stage-wise step of the C oracle (formulation 0) to 1e-9 relative, test_kkt_step_matches_oracle's bound; the oracle's
    inertia flag (0: right) is the eigenvalue count's -- also at the flipped iterate."""
    for nt, flipped in ((14, False), (18, False), (WRONG_INERTIA_NT, True)):
        case = Case(nt, scheme, 0, False, flipped)
        for b in range(1 if flipped else N_PROBLEMS):
            step, ok, _ = reference(case, b)
            mu, dw = (1e-6, 0.0) if flipped else (MU[b], dw_of(nt, b))
            rc, ref = coracle.newton_step(problems()[b], nt, np.array(blob_of(nt, scheme, b, flipped)), mu, dw, scheme=scheme)
            coracle.set_scheme(0)
            assert (rc == 0) == ok
            if ok:
                assert np.abs(step - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    assert not reference(Case(WRONG_INERTIA_NT, scheme, 0, False, True), 0)[1]


@pytest.mark.parametrize("case", CASES + WRONG_INERTIA_CASES, ids=case_id)
def test_every_case_is_fit_to_judge_a_kernel(case):
    """Inertia as the case says; the terminal unknowns of the iterate as the issue wants them; the reference's own error at most
    1e-10 x max(1, |section|max) in every section -- a hundredth of the bound the kernels are held to, so that the comparison on
    the device measures the kernel --; and, where there is a step to compare, a step without the terminal constraints' Hessian is
    more than 1e-6 x max(1, |section|max) away in some section: a hundred times that bound."""
    K = case.nt - 1
    for b in range(1 if case.flipped else N_PROBLEMS):
        blob = blob_of(case.nt, case.scheme, b, case.flipped)
        sc = blob[21 * K:]
        assert np.all(sc[3:7] > 0.0) and len(set(np.abs(sc[7:10]))) == 3 and np.all((np.abs(sc[7:10]) >= 0.1) & (np.abs(sc[7:10]) <= 1.0))
        step, ok, err = reference(case, b)
        assert ok == (not case.flipped), (b, iterate_of(case.nt, case.scheme, b))
        if case.flipped:
            continue
        # (... and a stage-wise factorisation can certify it: the kernels' flags are held to `ok` on the device)
        assert stagewise_inertia_ok(params_of_row(problems()[b]), case.nt, blob, MU[b], dw_of(case.nt, b), case.scheme, case.terminal, case.mp)
        scale = _section_scales(step, K)
        assert np.all(err <= 1e-10 * scale), (b, err / scale)
        if case.terminal == 2:
            assert step[21 * K + 7] == 0.0
        mu, dw = MU[b], dw_of(case.nt, b)
        wrong = lu_newton_step(params_of_row(problems()[b]), case.nt, blob, mu, dw, case.scheme, case.terminal, case.mp,
                               without_terminal_hessian=True)[0]
        diff = np.array([np.abs(wrong[lo:hi] - step[lo:hi]).max() for lo, hi in sections(K)])
        assert np.any(diff > 1e-6 * scale), (b, diff / scale)


def test_the_stagewise_inertia_test_is_sufficient_not_necessary(coracle):
    """A finding of this table, kept: at SUFFICIENT_ONLY the KKT matrix has n positive and m negative eigenvalues (the smallest
    |eigenvalue| 9e-7 against a largest of 6e4: resolved), but its block without the t_f column and the nu3 row has n - 2 and m
    -- one direction of negative curvature inside, made good by a positive definite 2 x 2 Schur complement of the border.  The
    recursion over the nodes meets a non-positive pivot and the C oracle refuses the step, as the kernels do (the GPU file): their
    flag means "cannot certify", which costs a regularisation, never a wrong step.  Terminal 0 and 1 alike (the same block)."""
    nt, scheme, b, iterate = SUFFICIENT_ONLY
    blob = np.array(blob_of(nt, scheme, b, iterate=iterate))
    P = params_of_row(problems()[b])
    for term in (0, 1):
        assert lu_newton_step(P, nt, blob, MU[b], dw_of(nt, b), scheme, term)[1]
        assert not stagewise_inertia_ok(P, nt, blob, MU[b], dw_of(nt, b), scheme, term)
    rc, _ = coracle.newton_step(problems()[b], nt, blob, MU[b], dw_of(nt, b), scheme=scheme)
    assert rc == 1


@pytest.mark.parametrize("scheme,mp", [(0, False), (1, True), (2, False)])
def test_the_step_differs_between_the_terminal_modes(scheme, mp):
    """Terminal 0, 1 and 2 are three Newton systems: 0 and 1 share the block and differ in its right-hand side (the target
    radius and speed), 2 has another block.  Pairwise more than 1e-6 x max(1, |section|max) apart in some section, on the reference."""
    nt = 14
    K = nt - 1
    for b in range(N_PROBLEMS):
        steps = [reference(Case(nt, scheme, term, mp, False), b)[0] for term in (0, 1, 2)]
        for i, j in ((0, 1), (0, 2), (1, 2)):
            scale = np.maximum(_section_scales(steps[i], K), _section_scales(steps[j], K))
            diff = np.array([np.abs(steps[i][lo:hi] - steps[j][lo:hi]).max() for lo, hi in sections(K)])
            assert np.any(diff > 1e-6 * scale), (b, i, j)
