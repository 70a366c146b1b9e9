"""The step rows p_solve no longer stores: the bound-multiplier steps and, with the move penalty, the
steps of the slack pair and its multipliers are closed forms of the node's iterate, of dz_angle, dz_mass, du of the node, du of
node k-1 and of the NLP's mu and delta_w.  The forward phase computes them for the fraction to the boundary; the adjoint phase's
trial point, a line-search retry and p_probe_out compute them again (step_locals) from rows they load anyway.  What can go
wrong is a recomputation that sees another operand than the forward phase did -- du of node k-1 across a chunk boundary, the
control before node 0, mu or delta_w of another round -- so the cases are the smallest grids on which those differ:

    nt = 17, single grid   rows 0-3 of the DCOST sweep: every NLP rejects once in iterations 1 and 5 (test_gpu_lockstep.py), so the
                           retry's recomputation runs on one full chunk
    nt = 18                K = 17: the second chunk holds one node; du of node k-1 and d lambda_u of node k+1 cross a chunk boundary;
                           also the v1 formulation (the control before node 0 is -1) and the trapezoid
    nt = 34                three chunks, the last one partial
    nt = 66, one NLP per wavefront (ASCENT_PERSIST_WIDE=1): the 64-node chunk boundary

each with and without the penalty, five NLPs (a second wavefront with three dead groups; nt = 17: the four rows named above),
against the C restatement (oracle/c_oracle.py), which stores nothing of the kind: equal status and iteration counts, t_f to the
3e-10 relative of test_gpu_lockstep.py and bench.py.  The oracle converges on every case, and the kernel that stored the rows
matched its iteration counts on every one of them (profiles/step_rows_parity.json).

The probe (ascent_kkt_step_path on the persistent path) returns the bound-multiplier steps, which p_probe_out now forms:
test_probe_bound_multiplier_steps compares them with (mu - z_b dx) / dist - z_b in numpy from the probe's own iterate and
primal step."""
import functools

import numpy as np
import pytest

import lunar_module_ascent_trajectory_optimiser_amd as A
from oracle import c_oracle
from test_terminal_step_reference import MU, blob_of, dw_of, problems

pytestmark = pytest.mark.gpu

# (nt, one NLP per wavefront, scheme, formulation)
SHAPES = {"nt17": (17, 0, 0, 0), "nt18": (18, 0, 0, 0), "nt18_v1": (18, 0, 0, 1), "nt18_trapezoid": (18, 0, 1, 0), "nt34": (34, 0, 0, 0),
          "nt66_wide": (66, 1, 0, 0)}


def _rows(name):
    S = A.sweep_isp_drymass(64, 64)[:4 if name == "nt17" else 5].copy()
    S[:, 15] = 1e-5
    return S


@functools.lru_cache(maxsize=None)
def _oracle(name, mp):
    nt, _, scheme, form = SHAPES[name]
    r = c_oracle.solve_batch(_rows(name), nt, 300, 1e-9, scheme=scheme, formulation=form, coarse_nodes=-1, move_penalty=mp)
    c_oracle.set_scheme(0); c_oracle.set_formulation(0)
    return r


@pytest.mark.parametrize("mp", [False, True], ids=["plain", "penalty"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_same_iterations_as_the_oracle(name, mp, monkeypatch):
    nt, wide, scheme, form = SHAPES[name]
    S = _rows(name)
    monkeypatch.setenv("ASCENT_PERSIST_WIDE", str(wide))
    assert A.default_path(len(S), nt, scheme=scheme, formulation=form, move_penalty=mp) == "persist"
    r = A.solve_batch(S, nt, tol=1e-9, scheme=scheme, formulation=form, coarse_nodes=-1, move_penalty=mp)
    ref = _oracle(name, mp)
    print(name, "penalty" if mp else "plain", "iters", r.iters, "oracle", ref["iters"], "status", r.status, ref["status"],
          "rel tf", np.abs(r.tf - ref["tf"]) / ref["tf"])
    assert np.all(ref["status"] == 0), ref["status"]
    assert np.array_equal(r.status, ref["status"]), (r.status, ref["status"])
    assert np.array_equal(r.iters, ref["iters"]), (r.iters, ref["iters"])
    assert (np.abs(r.tf - ref["tf"]) / ref["tf"]).max() <= 3e-10


# The bound of test_probe_bound_multiplier_steps, in ulps of |mu/dist| + |z_b dx/dist| + |z_b|.  The kernel's value is
# id (mu - z_b dx) - z_b with id = rcp(dist) to about one ulp, one fused multiply-add inside the bracket and one outside; numpy
# rounds every operation of (mu - z_b dx)/dist - z_b: each side is a handful of roundings of terms no larger than that sum.
# Measured on the kernel that stored the rows (the parent of this change), over the cases below in both wavefront forms: worst
# ratio 2.0; the bound is four times that (both figures: profiles/step_rows_parity.json).
ULP_BOUND = 8.0


@pytest.mark.parametrize("mp", [False, True], ids=["plain", "penalty"])
@pytest.mark.parametrize("nt", [18, 34])
def test_probe_bound_multiplier_steps(nt, mp):
    K = nt - 1
    S = problems()
    B = len(S)
    blobs = np.stack([blob_of(nt, 0, b) for b in range(B)], axis=1)
    dw = np.array([dw_of(nt, b) for b in range(B)])
    with pytest.MonkeyPatch.context() as m:
        m.setenv("ASCENT_PERSIST_WIDE", "0")
        step, inertia = A.kkt_step(S, blobs, MU.copy(), dw, nt, path="persist", move_penalty=mp)
    assert np.all(inertia == 0), inertia
    worst = 0.0
    for b in range(B):
        it, st = blobs[:, b], step[:, b]
        z, dz = it[:7 * K].reshape(K, 7), st[:7 * K].reshape(K, 7)
        u, du = it[7 * K:8 * K], st[7 * K:8 * K]
        zb, dzb = it[15 * K:21 * K].reshape(K, 6), st[15 * K:21 * K].reshape(K, 6)
        aub = S[b, 12]
        dist = np.stack([z[:, 4], aub - z[:, 4], z[:, 6], 1.0 - z[:, 6], u + 1.0, 1.0 - u], axis=1)
        dx = np.stack([dz[:, 4], -dz[:, 4], dz[:, 6], -dz[:, 6], du, -du], axis=1)
        ref = (MU[b] - zb * dx) / dist - zb
        scale = np.abs(MU[b] / dist) + np.abs(zb * dx / dist) + np.abs(zb)
        assert np.any(dzb != 0.0)
        worst = max(worst, float((np.abs(dzb - ref) / (np.spacing(scale))).max()))
    print("nt", nt, "penalty" if mp else "plain", "worst error in ulps of the scale", worst)
    assert worst <= ULP_BOUND
