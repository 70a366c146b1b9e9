"""GPU parity tests of the terminal block of the Newton step: A.kkt_step with ascent_opts.terminal 0, 1 and 2 through every kernel
that carries a terminal block -- p_solve (schemes 0 / 1, with and without the move penalty) and h_solve (scheme 2) in their
four-NLPs- and one-NLP-per-wavefront forms, the dense-block path with its Riccati and its cyclic-reduction Newton solver -- against
tests/terminal_step_reference.py: a generic sparse LU of the full KKT matrix with the terminal Jacobian and Hessian of
oracle/ascent_general.py (checked against central differences in tests/test_general_oracle.py), which shares no derivation with the
two HIP paths.  tests/test_terminal_step_reference.py holds the case table and shows on the CPU that every case is fit to judge a
kernel (inertia, the reference's own error <= 1e-10, a step without the terminal Hessian >= 1e-6 away).

Bounds, the project's existing ones: the step to 1e-8 x max(1, |LU section|max) per blob section; the inertia flag equal to the
eigenvalue count's on the exact-inertia forms (persist, dense/riccati); the cyclic-reduction variant may refuse a step the others
take, a step it returns meets the bound; row 21K+7 (d nu3) of a terminal-2 step is exactly 0.0.

Grids: three nodes, the last node of a chunk and one node past it, for each form (the terminal block sits in the last node, in
the last and usually partial chunk); batches of 3 and 5 (a ragged last wavefront with four NLPs per wavefront).  The largest
error / bound ratio of every variant is collected in PARITY; with ASCENT_TERMINAL_STEP_PARITY_OUT=<file> it is written there as JSON
when the module is done (profiles/terminal_step_parity.json is such a file)."""
import os

import numpy as np
import pytest

import lunar_module_ascent_trajectory_optimiser_amd as A
from gpu_cases import parity_writer
from terminal_step_reference import sections
from test_terminal_step_reference import (CASES, GRIDS, MU, SUFFICIENT_ONLY, WRONG_INERTIA_CASES, WRONG_INERTIA_NT, Case, blob_of, dw_of,
                                          problems, reference)

pytestmark = pytest.mark.gpu
PARITY = {}
_write_parity = parity_writer("ASCENT_TERMINAL_STEP_PARITY_OUT",
                              {"bound": "1e-8 x max(1, |LU section|max) per blob section", "largest_error_over_bound": PARITY}, sort_keys=True)


# ---- the variants, spelled out: (kernel, form, scheme, terminal, move penalty, nt, batch)
#   kernel "p_solve" / "h_solve": path "persist" with ASCENT_PERSIST_WIDE = form (0: four NLPs per wavefront, 1: one);
#   kernel "dense": path "dense" with ASCENT_DENSE_NEWTON = form ("riccati" | "pcr")
BATCHES = (3, 5)
P_SOLVE = [("p_solve", wide, scheme, term, mp, nt, B) for wide in (0, 1) for scheme in (0, 1) for term in (0, 1, 2) for mp in (False, True)
           for nt in GRIDS["p_solve", wide] for B in BATCHES]
H_SOLVE = [("h_solve", wide, 2, term, False, nt, B) for wide in (0, 1) for term in (0, 1, 2) for nt in GRIDS["h_solve", wide] for B in BATCHES]
DENSE = [("dense", newton, scheme, term, mp, nt, B) for newton in ("riccati", "pcr") for scheme in (0, 1, 2) for term in (0, 1, 2)
         for mp in (False, True) for nt in GRIDS["dense"] for B in BATCHES]
assert len(P_SOLVE) == 144 and len(H_SOLVE) == 36 and len(DENSE) == 144
assert {Case(nt, scheme, term, mp, False) for _, _, scheme, term, mp, nt, _ in P_SOLVE + H_SOLVE + DENSE} == set(CASES)


def _id(v):
    kernel, form, scheme, term, mp, nt, B = v
    form = f"wide{form}" if kernel != "dense" else form
    return f"{kernel}-{form}-scheme{scheme}-terminal{term}-{'penalty' if mp else 'plain'}-nt{nt}-B{B}"


def _kkt_step(kernel, form, S, blobs, mu, dw, nt, scheme, term, mp):
    name, value = ("ASCENT_DENSE_NEWTON", form) if kernel == "dense" else ("ASCENT_PERSIST_WIDE", str(form))
    assert name not in os.environ
    os.environ[name] = value
    try:
        return A.kkt_step(S, blobs, mu, dw, nt, path="dense" if kernel == "dense" else "persist", scheme=scheme, terminal=term, move_penalty=mp)
    finally:
        del os.environ[name]


@pytest.mark.parametrize("variant", P_SOLVE + H_SOLVE + DENSE, ids=_id)
def test_kkt_step_matches_the_terminal_lu(variant):
    kernel, form, scheme, term, mp, nt, B = variant
    K = nt - 1
    case = Case(nt, scheme, term, mp, False)
    S = problems()[:B]
    blobs = np.stack([blob_of(nt, scheme, b) for b in range(B)], axis=1)
    mu = MU[:B].copy(); dw = np.array([dw_of(nt, b) for b in range(B)])
    step, inertia = _kkt_step(kernel, form, S, blobs, mu, dw, nt, scheme, term, mp)
    exact = not (kernel == "dense" and form == "pcr")
    worst, n_compared = 0.0, 0
    failures = []
    for b in range(B):
        lu, ok, _ = reference(case, b)
        assert ok                                    # (every case of the table has the right inertia: test_terminal_step_reference.py)
        if exact:
            assert inertia[b] == 0, (b, "the kernel reports a wrong inertia where the eigenvalue count says it is right")
        elif inertia[b]:
            continue                                 # (its curvature test may refuse a step the exact-inertia forms take)
        n_compared += 1
        for i, (lo, hi) in enumerate(sections(K)):
            ratio = np.abs(step[lo:hi, b] - lu[lo:hi]).max() / (1e-8 * max(1.0, np.abs(lu[lo:hi]).max()))
            worst = max(worst, float(ratio))
            if not ratio <= 1.0:
                failures.append((b, i, float(ratio)))
        if term == 2:
            assert step[21 * K + 7, b] == 0.0, (b, step[21 * K + 7, b])
    key = _id(variant).rsplit("-nt", 1)[0]
    PARITY[key] = max(PARITY.get(key, 0.0), worst)
    print(f"{_id(variant)}: largest error / bound {worst:.3g} over {n_compared} of {B} problems")
    assert not failures, failures
    assert n_compared >= (B if exact else 1)


# ---- wrong inertia: defect multipliers x -50 (test_kkt_step_detects_wrong_inertia's iterate, here for every terminal mode): the
# eigenvalue count says the inertia is wrong (test_terminal_step_reference.py), the exact-inertia forms must report it
WRONG = [(kernel, form, c.scheme, c.terminal) for c in WRONG_INERTIA_CASES
         for kernel, form in ((("p_solve", 0), ("p_solve", 1)) if c.scheme == 0 else (("h_solve", 0), ("h_solve", 1))) + (("dense", "riccati"),)]


@pytest.mark.parametrize("kernel,form,scheme,term", WRONG,
                         ids=[f"{k}-{'wide' + str(f) if k != 'dense' else f}-scheme{s}-terminal{t}" for k, f, s, t in WRONG])
def test_kkt_step_reports_the_wrong_inertia_in_every_terminal_mode(kernel, form, scheme, term):
    nt = WRONG_INERTIA_NT
    case = Case(nt, scheme, term, False, True)
    assert case in WRONG_INERTIA_CASES and not reference(case, 0)[1]
    blob = np.array(blob_of(nt, scheme, 0, True))
    _, inertia = _kkt_step(kernel, form, problems()[:1], blob[:, None], np.array([1e-6]), np.array([0.0]), nt, scheme, term, False)
    assert inertia[0] == 1


@pytest.mark.parametrize("kernel,form", [("p_solve", 0), ("p_solve", 1), ("dense", "riccati")], ids=["p_solve-wide0", "p_solve-wide1", "dense-riccati"])
@pytest.mark.parametrize("term", [0, 1])
def test_kkt_step_refuses_what_a_stagewise_factorisation_cannot_certify(kernel, form, term):
    """test_the_stagewise_inertia_test_is_sufficient_not_necessary's iterate: the right inertia by eigenvalue count, one negative
    direction inside the block without t_f and nu3.  The kernels' test is the C oracle's: they report it."""
    nt, scheme, b, iterate = SUFFICIENT_ONLY
    blob = np.array(blob_of(nt, scheme, b, iterate=iterate))
    _, inertia = _kkt_step(kernel, form, problems()[b:b + 1], blob[:, None], MU[b:b + 1].copy(), np.array([dw_of(nt, b)]), nt, scheme, term, False)
    assert inertia[0] == 1
