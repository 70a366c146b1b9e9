"""GPU parity tests: the HIP path, called through the C ABI (include/ascent.h), against the oracle
and the golden fixtures.  Tolerances: BASELINE.md section 4 -- t_f within 1e-4 relative of the IPOPT
golden value; HIP vs oracle 1e-9 relative on t_f (they run the same algorithm in different code and
different summation orders; observed agreement is ~1e-15)."""
import numpy as np
import pytest

import lunar_module_ascent_trajectory_optimiser_amd as A
from conftest import random_interior_blob

pytestmark = pytest.mark.gpu

NT = 200
K = NT - 1


@pytest.fixture(scope="module")
def nominal_gpu():
    r = A.solve_batch(A.AscentParams(), NT, tol=1e-9, want_blob=True)
    assert r.status[0] == 0
    return r


def test_device_present():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    assert _lib.load().ascent_device_count() >= 1


def test_nominal_matches_golden(nominal_gpu, golden):
    """Numerical_results.png (Launch_Optimiser.py:188-194)."""
    o, g, tol = nominal_gpu.outputs(0), golden["current"], golden["tolerances"]
    downrange, speed = abs(g["final_x"]), np.hypot(g["final_xdot"], g["final_ydot"])
    assert abs(o["final_time"] - g["final_time"]) <= tol["final_time_rel"] * g["final_time"]
    for k in ("final_x", "final_y"):
        assert abs(o[k] - g[k]) <= tol["position_rel_of_downrange"] * downrange
    for k in ("final_xdot", "final_ydot"):
        assert abs(o[k] - g[k]) <= tol["velocity_rel_of_speed"] * speed
    for k in ("final_xdoubledot", "final_ydoubledot"):
        assert abs(o[k] - g[k]) <= tol["acceleration_rel"] * abs(g[k])
    assert abs(o["theta_deg"][-1] - golden["qualitative"]["angle_final_deg"]) < 0.2
    assert abs(o["x_pos"][-1] - 290.1e3) < 100 and abs(o["r"][-1] - (1738100 + 17703)) < 1.0


def test_nominal_matches_oracle(nominal_gpu, nominal_oracle_solution, coracle):
    p16, ref = nominal_oracle_solution
    r = nominal_gpu
    assert abs(r.tf[0] - ref["tf"][0]) <= 1e-9 * ref["tf"][0]
    assert np.abs(r.traj[:, :, 0] - ref["traj"][0]).max() < 1e-8
    # the oracle's own optimality measure at the GPU's primal-dual solution
    assert coracle.kkt_error(p16, NT, np.ascontiguousarray(r.blob[:, 0])) <= 2e-9


V1 = dict(r_peri=53108.4, r_apo=53108.4, mass_scalar=2576.0)     # the v1 script's constants (PDF p26-28)
STEP_CASES = [("fused", 0, 0), ("split_lane", 0, 0), ("split_wide", 0, 0), ("split_lane", 1, 0), ("split_wide", 1, 0),
              ("split_lane", 0, 1), ("split_wide", 0, 1)]


def _interior_blobs(coracle, S, nt, scheme, form):
    """Strictly interior primal-dual iterates: a few oracle iterations from the cold start, multipliers perturbed."""
    blobs = []
    for b, row in enumerate(S):
        rng = np.random.default_rng(100 + b)
        r = coracle.solve_batch(row[None], nt, 3 + b % 4, 1e-9, want_blob=True, coarse_nodes=-1, scheme=scheme, formulation=form)
        blob = r["blob"][0].copy()
        Kk = nt - 1
        blob[8 * Kk:15 * Kk] += 0.05 * rng.standard_normal(7 * Kk)
        blob[15 * Kk:21 * Kk] *= rng.uniform(0.7, 1.3, 6 * Kk)
        blobs.append(blob)
    coracle.set_scheme(0); coracle.set_formulation(0)
    return np.stack(blobs, axis=1)


@pytest.mark.parametrize("path,scheme,form", STEP_CASES + [("persist", 0, 0), ("persist", 1, 0), ("persist", 0, 1)])
def test_eval_nodes_matches_oracle(coracle, path, scheme, form):
    """Defects and Jacobian/Hessian blocks of every step (Launch_Optimiser.py:114-136), 1e-12 relative, through the
    kernels each solver path really runs: "fused" = k_eval_nodes, "split_*" = q_trial_eval, whose materialised rows
    Q_C / Q_G / Q_H come back through q_probe_out, "persist" = p_solve (the kernel the bench headline times): the rows its
    node-parallel phase stages in LDS for the factorisation sweep (S_G / S_H / S_C), copied out of LDS by the kernel itself
    before the sweep would read them (probe kind 2) -- a wrong Jacobian row there is localised, not just a step mismatch."""
    base = A.AscentParams(**V1) if form else A.AscentParams()
    S = A.sweep_isp_drymass(2, 2, base=base)
    blobs = _interior_blobs(coracle, S, NT, scheme, form)
    d, j, h = A.eval_nodes(S, blobs, NT, path=path, scheme=scheme, formulation=form)
    for b in range(4):
        blob = np.ascontiguousarray(blobs[:, b])
        if form == 0:       # (the oracle's constraint export is for the current formulation)
            cref = coracle.constraints(S[b], NT, blob, scheme=scheme)
            coracle.set_scheme(0)
            assert np.allclose(d[:, b], cref[:7 * K], rtol=1e-12, atol=1e-14)
        z = blob[:7 * K].reshape(K, 7); lam = blob[8 * K:15 * K].reshape(K, 7)
        dt = (1.0 / K) * S[b, 11] * blob[21 * K]
        lw = lam if scheme == 0 else 0.5 * (lam + np.vstack([lam[1:], np.zeros((1, 7))]))   # trapezoid: node k sits in steps k and k+1
        ax, ay, gax, gay, H = coracle.accel(S[b], z[:, 0], z[:, 1], z[:, 4], z[:, 6], -dt * lw[:, 2], -dt * lw[:, 3])
        assert np.allclose(j[:, b].reshape(K, 8), np.hstack([gax, gay]), rtol=1e-12, atol=1e-15)
        hb = h[:, b].reshape(K, 10)
        assert np.allclose(np.delete(hb, (7, 9), 1), np.delete(H, (7, 9), 1), rtol=1e-11, atol=1e-14)
        # the split kernels fold the bound-barrier curvature Sigma = z_L/d_L + z_U/d_U into the aa / mm entries and
        # q_probe_out takes it out again: those two entries carry the rounding of that round trip, ~eps * Sigma
        zbk = blob[15 * K:21 * K].reshape(K, 6)
        sig = np.stack([zbk[:, 0] / z[:, 4] + zbk[:, 1] / (S[b, 12] - z[:, 4]), zbk[:, 2] / z[:, 6] + zbk[:, 3] / (1 - z[:, 6])], 1)
        slack = 1e-14 + (0 if path == "fused" else 1) * 4e-16 * sig
        assert np.all(np.abs(hb[:, (7, 9)] - H[:, (7, 9)]) <= 1e-11 * np.abs(H[:, (7, 9)]) + slack)


@pytest.mark.parametrize("path,scheme,form", STEP_CASES + [("persist", 0, 0), ("persist", 1, 0), ("persist", 0, 1)])
def test_kkt_step_matches_oracle(coracle, path, scheme, form):
    """One Newton step of the barrier problem at random interior iterates, with and without primal regularisation,
    through one round of exactly the kernels each path runs in a solve ("persist" = one round of p_solve, the kernel the
    bench headline times: trial evaluation, node blocks through LDS into the 16-lane factorisation, forward and adjoint
    sweeps).  Checked against the C oracle's stage-wise step AND against a generic sparse-LU solve of the full KKT matrix
    (numpy oracle; no stage structure)."""
    from conftest import generic_lu_newton_step, params_of_row
    nt = 60
    Kk = nt - 1
    base = A.AscentParams(**V1) if form else A.AscentParams()
    S = A.sweep_isp_drymass(2, 3, base=base)
    B = len(S)
    blobs = _interior_blobs(coracle, S, nt, scheme, form)
    mu = np.array([0.1, 0.02, 1e-3, 0.05, 0.01, 0.2]); dw = np.array([0.0, 0.0, 1e-2, 1.0, 0.0, 1e-4])
    step, inertia = A.kkt_step(S, blobs, mu, dw, nt, path=path, scheme=scheme, formulation=form)
    n_ok = 0
    for b in range(B):
        blob = np.ascontiguousarray(blobs[:, b])
        rc, ref = coracle.newton_step(S[b], nt, blob, mu[b], dw[b], scheme=scheme, formulation=form)
        coracle.set_scheme(0); coracle.set_formulation(0)
        assert rc == inertia[b]
        if rc:
            continue
        n_ok += 1
        assert np.abs(step[:, b] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        if form == 0:
            lu, _, _, _ = generic_lu_newton_step(params_of_row(S[b]), nt, blob, mu[b], dw[b], scheme)
            for lo, hi in ((0, 8 * Kk), (8 * Kk, 15 * Kk), (15 * Kk, 21 * Kk), (21 * Kk, 21 * Kk + 10)):
                assert np.abs(step[lo:hi, b] - lu[lo:hi]).max() <= 1e-8 * max(1.0, np.abs(lu[lo:hi]).max())
    assert n_ok >= 3


@pytest.mark.parametrize("path,scheme", [("persist", 0), ("persist", 1), ("dense", 0), ("dense", 1)])
def test_kkt_step_with_move_penalty_matches_oracle_and_generic_lu(coracle, monkeypatch, path, scheme):
    """a12 (Launch_Optimiser.py:99) at step level: one Newton step of the barrier problem WITH the l1 move penalty through one
    round of p_solve<.,0,1> (the control as the eighth state of the 16-lane sweeps, the slack pair reduced to one pivot) and
    through the dense-block path, against the C restatement (1e-9) and against a generic sparse LU of the full KKT matrix in
    which the slack pairs and the movement equations are explicit unknowns and rows (nothing reduced, 1e-8)."""
    from conftest import generic_lu_newton_step, params_of_row
    monkeypatch.setenv("ASCENT_DENSE_NEWTON", "riccati")      # (the dense path's PCR variant exposes no inertia; its Riccati form does)
    nt = 60
    Kk = nt - 1
    S = A.sweep_isp_drymass(2, 3)
    S[:, 15] = [1e-5, 1e-5, 1e-3, 1e-4, 1e-5, 1e-2]
    blobs = _interior_blobs(coracle, S, nt, scheme, 0)
    mu = np.array([0.1, 0.02, 1e-3, 0.05, 1e-6, 0.2]); dw = np.array([0.0, 0.0, 1e-2, 1.0, 0.0, 1e-4])
    step, inertia = A.kkt_step(S, blobs, mu, dw, nt, path=path, scheme=scheme, move_penalty=True)
    n_ok = 0
    for b in range(len(S)):
        blob = np.ascontiguousarray(blobs[:, b])
        rc, ref = coracle.newton_step(S[b], nt, blob, mu[b], dw[b], scheme=scheme, move_penalty=True)
        coracle.set_scheme(0)
        assert rc == inertia[b]
        if rc:
            continue
        n_ok += 1
        assert np.abs(step[:, b] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        lu, _, _, _ = generic_lu_newton_step(params_of_row(S[b]), nt, blob, mu[b], dw[b], scheme, move_penalty=True)
        for lo, hi in ((0, 8 * Kk), (8 * Kk, 15 * Kk), (15 * Kk, 21 * Kk), (21 * Kk, 21 * Kk + 10)):
            assert np.abs(step[lo:hi, b] - lu[lo:hi]).max() <= 1e-8 * max(1.0, np.abs(lu[lo:hi]).max())
    assert n_ok >= 4
    # the penalty changes the step: the same call without it differs
    b = int(np.flatnonzero(inertia == 0)[0])
    step0, in0 = A.kkt_step(S[b:b + 1], blobs[:, b:b + 1], mu[b:b + 1], dw[b:b + 1], nt, path=path, scheme=scheme)
    assert in0[0] == 0 and np.abs(step0[:, 0] - step[:, b]).max() > 1e-6


def test_move_penalty_in_the_persistent_kernel_matches_the_oracle_on_a_sweep(coracle):
    """a12 at solve level, through the default dispatch (the persistent kernel): a 7 x 6 sweep with the reference's DCOST, both
    schemes -- every NLP converges, identical iteration counts and t_f to 1e-12 against the C restatement (same algorithm:
    slack pairs re-centred on every grid level), t_f to 2e-8 against the dense-block path (an independent HIP implementation) at
    tol 1e-9 and to 2e-9 at tol 1e-10."""
    S = A.sweep_isp_drymass(7, 6)
    S[:, 15] = 1e-5
    assert A.default_path(len(S), NT, move_penalty=True) == "persist"
    for scheme in (0, 1):
        r = A.solve_batch(S, NT, tol=1e-9, scheme=scheme, move_penalty=True)
        ref = coracle.solve_batch(S, NT, 300, 1e-9, scheme=scheme, move_penalty=True)
        coracle.set_scheme(0)
        assert np.all(r.status == 0) and np.all(ref["status"] == 0)
        assert np.array_equal(r.iters, ref["iters"])
        assert np.abs(r.tf - ref["tf"]).max() <= 1e-12
        assert np.abs(np.moveaxis(r.traj, 2, 0)[:, :8] - ref["traj"][:, :8]).max() < 1e-6
        dn = A.solve_batch(S[::5], NT, tol=1e-9, scheme=scheme, move_penalty=True, path="dense")
        assert np.all(dn.status == 0) and np.abs(dn.tf - r.tf[::5]).max() <= 2e-8     # (<= 32 NLPs: its PCR variant, another regularisation rule; two KKT points at tol 1e-9)
        # ... and at tol = 1e-10, where two KKT points lie closer: 2e-9 (measured 5.1e-9 at 1e-9, 2.2e-10 at 1e-10, 3.7e-10 at 1e-11: it
        # falls with the tolerance -- KKT slack, not the slack-pair reduction)
        r10 = A.solve_batch(S, NT, tol=1e-10, scheme=scheme, move_penalty=True, max_iter=500)
        dn10 = A.solve_batch(S[::5], NT, tol=1e-10, scheme=scheme, move_penalty=True, path="dense", max_iter=500)
        assert np.all(r10.status == 0) and np.all(dn10.status == 0) and np.abs(dn10.tf - r10.tf[::5]).max() <= 2e-9
    # ragged batch, dead wavefront groups, an odd grid, an iteration cap, warm start from the penalised solution
    r5 = A.solve_batch(S[:5], 37, tol=1e-9, move_penalty=True)
    o5 = coracle.solve_batch(S[:5], 37, 300, 1e-9, move_penalty=True)
    assert np.all(r5.status == 0) and np.abs(r5.tf - o5["tf"]).max() <= 1e-10 and np.abs(r5.iters.astype(int) - o5["iters"]).max() <= 1
    rc = A.solve_batch(S[:3], NT, tol=1e-9, move_penalty=True, max_iter=3)
    assert np.all(rc.status == 1)
    full = A.solve_batch(S[:6], NT, tol=1e-9, move_penalty=True, want_blob=True)
    warm = A.solve_batch(S[:6], NT, tol=1e-9, move_penalty=True, guess=full.blob, warm_start=2, mu_init=1e-8)
    assert np.all(warm.status == 0) and warm.iters.max() <= 12 and np.abs(warm.tf - full.tf).max() <= 1e-8


def test_move_penalty_with_the_v1_formulation(coracle):
    """The v1 script's own `angle.DCOST = 1e-5` (PDF p26): ascent_opts.move_penalty with formulation 1 in the persistent kernel
    (p_solve<0,1,1>: the control enters the algebraic angle row, weight dcost * angle_ub/2 on u, u before node 0 = -1).
    Step level against the C restatement (1e-9); solve level against tests/golden/dcost_fixtures.json["v1_cases"] -- the v1
    formulation's own numpy NLP with explicit slack pairs, generic LU (t_f to 2e-8) -- and against the C restatement on a sweep
    (identical iteration counts, t_f to 1e-9, the median to 1e-14)."""
    import json, os
    base = A.AscentParams(**V1)
    S = A.sweep_isp_drymass(2, 3, base=base)
    S[:, 15] = [1e-5, 1e-5, 1e-3, 1e-4, 1e-5, 1e-2]
    nt = 60
    blobs = _interior_blobs(coracle, S, nt, 0, 1)
    mu = np.array([0.1, 0.02, 1e-3, 0.05, 1e-6, 0.2]); dw = np.array([0.0, 0.0, 1e-2, 1.0, 0.0, 1e-4])
    step, inertia = A.kkt_step(S, blobs, mu, dw, nt, path="persist", formulation=1, move_penalty=True)
    n_ok = 0
    for b in range(len(S)):
        rc, ref = coracle.newton_step(S[b], nt, np.ascontiguousarray(blobs[:, b]), mu[b], dw[b], formulation=1, move_penalty=True)
        assert rc == inertia[b]
        if rc == 0:
            n_ok += 1
            assert np.abs(step[:, b] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    coracle.set_formulation(0)
    assert n_ok >= 4
    fx = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "dcost_fixtures.json")))
    for c in fx["v1_cases"]:
        P = A.AscentParams(**c["params"])
        for on in (False, True):
            r = A.solve_batch(P, c["nt"], tol=1e-9, formulation=1, move_penalty=on, max_iter=500)
            ref = c["on" if on else "off"]
            assert r.status[0] == 0 and abs(r.tf[0] - ref["tf"]) <= 2e-8, (c["nt"], c["dcost"], on, r.tf[0], ref["tf"])
            ang = r.traj[6, :, 0]
            assert abs(np.abs(np.diff(ang)).sum() - ref["total_variation"]) <= 2e-3 * ref["total_variation"]
    S2 = A.sweep_isp_drymass(5, 4, base=base)
    S2[:, 15] = 1e-5
    r = A.solve_batch(S2, NT, tol=1e-9, formulation=1, move_penalty=True)
    ref = coracle.solve_batch(S2, NT, 300, 1e-9, formulation=1, move_penalty=True)
    coracle.set_formulation(0)
    assert np.all(r.status == 0) and np.array_equal(r.iters, ref["iters"]) and np.abs(r.tf - ref["tf"]).max() <= 1e-9
    assert np.median(np.abs(r.tf - ref["tf"])) <= 1e-14


@pytest.mark.parametrize("scheme,mp", [(0, False), (1, False), (0, True)])
def test_kkt_step_with_terminal2_persistent_kernel_equals_dense_path(coracle, monkeypatch, scheme, mp):
    """ascent_opts.terminal = 2 (burnout anywhere on the ellipse) at step level: one Newton step through one round of
    p_solve<.,0,.,2> against the dense-block path's Riccati form -- two independent HIP implementations of the generalised terminal
    block (gradients of both conditions in position AND velocity, the antisymmetric position-velocity Hessian of the angular
    momentum, the unit pivot that closes the absent r.v = 0 row) -- with and without regularisation and the move penalty.
    Both follow one derivation: the independent anchor of this block (and of terminal 1's) is tests/test_gpu_terminal_step.py,
    where every kernel's step is held to a generic LU with the terminal derivatives of oracle/ascent_general.py."""
    monkeypatch.setenv("ASCENT_DENSE_NEWTON", "riccati")
    nt = 60
    S = A.sweep_isp_drymass(2, 3)
    S[:, 15] = 1e-5
    blobs = _interior_blobs(coracle, S, nt, scheme, 0)
    mu = np.array([0.1, 0.02, 1e-3, 0.05, 1e-6, 0.2]); dw = np.array([0.0, 1e-3, 1e-2, 1.0, 0.0, 1e-4])
    sp, ip = A.kkt_step(S, blobs, mu, dw, nt, path="persist", scheme=scheme, terminal=2, move_penalty=mp)
    sd, idn = A.kkt_step(S, blobs, mu, dw, nt, path="dense", scheme=scheme, terminal=2, move_penalty=mp)
    s0, _ = A.kkt_step(S, blobs, mu, dw, nt, path="persist", scheme=scheme, terminal=1, move_penalty=mp)
    assert np.array_equal(ip, idn) and (ip == 0).sum() >= 3
    monkeypatch.setenv("ASCENT_DENSE_NEWTON", "pcr")             # ... and the dense path's cyclic-reduction variant (no inertia information)
    sc_, ic_ = A.kkt_step(S, blobs, mu, dw, nt, path="dense", scheme=scheme, terminal=2, move_penalty=mp)
    assert ((ip == 0) & (ic_ == 0)).sum() >= 2
    for b in np.flatnonzero(ip == 0):
        assert np.abs(sp[:, b] - sd[:, b]).max() <= 1e-9 * max(1.0, np.abs(sd[:, b]).max())
        if ic_[b] == 0:      # (its curvature test may refuse a step the exact-inertia forms take)
            assert np.abs(sc_[:, b] - sd[:, b]).max() <= 1e-8 * max(1.0, np.abs(sd[:, b]).max())
        assert np.abs(sp[:, b] - s0[:, b]).max() > 1e-6          # (another terminal block: another step)


@pytest.mark.parametrize("path", ["fused", "split_lane", "split_wide", "persist"])
def test_kkt_step_detects_wrong_inertia(coracle, path):
    """A strongly negative curvature (flipped multipliers) must be reported, not solved through."""
    S = A.sweep_isp_drymass(1, 1)
    blob = random_interior_blob(NT, 2, S[0], coracle)
    blob[8 * K:15 * K] *= -50.0
    step, inertia = A.kkt_step(S, blob[:, None], 1e-6, 0.0, NT, path=path)
    rc, _ = coracle.newton_step(S[0], NT, blob, 1e-6, 0.0)
    assert inertia[0] == rc == 1


def test_batch_sweep_matches_oracle(coracle):
    """8x8 Isp x dry-mass sweep: every problem against the oracle."""
    S = A.sweep_isp_drymass(8, 8)
    r = A.solve_batch(S, NT, tol=1e-9)
    ref = coracle.solve_batch(S, NT, 300, 1e-9)
    assert np.all(r.status == 0) and np.all(ref["status"] == 0)
    assert np.abs(r.tf - ref["tf"]).max() <= 1e-9 * ref["tf"].max()
    assert np.abs(np.moveaxis(r.traj, 2, 0) - ref["traj"]).max() < 1e-7
    assert np.array_equal(r.iters, ref["iters"])


def test_split_and_fused_paths_agree(coracle, monkeypatch):
    """The two solver paths (split pipeline for small batches, fused one-lane-per-NLP kernel for large
    ones; ASCENT_PIPELINE overrides the batch-size rule) run the same algorithm: same answers, same
    iteration counts, both equal to the oracle."""
    S = A.sweep_isp_drymass(10, 7)
    ref = coracle.solve_batch(S, NT, 300, 1e-9)
    out = {}
    for mode in ("split", "fused"):
        monkeypatch.setenv("ASCENT_PIPELINE", mode)
        out[mode] = A.solve_batch(S, NT, tol=1e-9, want_blob=True)
        assert np.all(out[mode].status == 0)
        assert np.abs(out[mode].tf - ref["tf"]).max() <= 1e-9 * ref["tf"].max()
        assert np.abs(np.moveaxis(out[mode].traj, 2, 0) - ref["traj"]).max() < 1e-7
        assert np.array_equal(out[mode].iters, ref["iters"])
    assert np.abs(out["split"].tf - out["fused"].tf).max() <= 1e-12
    assert np.abs(out["split"].blob - out["fused"].blob).max() <= 1e-6 * np.abs(out["fused"].blob).max()
    # warm start and max_iter through both paths
    for mode in ("split", "fused"):
        monkeypatch.setenv("ASCENT_PIPELINE", mode)
        w = A.solve_batch(S, NT, tol=1e-9, guess=out["fused"].blob, warm_start=2, mu_init=1e-9)
        assert np.all(w.status == 0) and w.iters.max() <= 8 and np.abs(w.tf - ref["tf"]).max() <= 1e-9
        m = A.solve_batch(S[:5], NT, tol=1e-9, max_iter=4, coarse_nodes=-1)
        assert np.all(m.status == 1) and np.all(m.iters == 4)
        # nested iteration: the cap holds per grid level; a coarse solve that hits it makes the fine one start cold
        m = A.solve_batch(S[:5], NT, tol=1e-9, max_iter=4)            # three grids: 17 -> 60 -> 200 nodes
        assert np.all(m.status == 1) and np.all(m.iters == 12)


def test_persistent_kernel_matches_split_pipeline_and_oracle(coracle, monkeypatch):
    """The persistent kernel (csrc/ascent_persist.hip: one wavefront owns four NLPs for the whole solve, node blocks handed
    to the 16-lane sweeps through LDS; the default for 2 .. 28 671 NLPs of scheme 0 at N=200) against the split pipeline and the
    oracle: same algorithm, same arithmetic per lane -- identical iteration counts on every problem, t_f to rounding.
    Ragged batches exercise partially filled wavefronts (dead groups) and chunks (199 = 12 x 16 + 7 nodes)."""
    for B, nt in ((5, 200), (67, 200), (130, 37), (1000, 200), (9, 1000)):
        S = A.sweep_isp_drymass()[:: max(1, 4096 // B)][:B]
        out = {}
        for mode in ("persist", "split"):
            monkeypatch.setenv("ASCENT_PIPELINE", mode)
            out[mode] = A.solve_batch(S, nt, tol=1e-9, want_blob=True, max_iter=500)
            assert np.all(out[mode].status == 0)
        if nt >= 200:
            assert np.array_equal(out["persist"].iters, out["split"].iters)
        else:     # (37 nodes: no nested iteration, 17-22 iterations from the cold start; the convergence test is a rounding knife edge)
            assert np.abs(out["persist"].iters.astype(int) - out["split"].iters).max() <= 1
        assert np.abs(out["persist"].tf - out["split"].tf).max() <= 1e-9
        for f in (0, 1, 2, 3, 6, 9):
            assert np.abs(out["persist"].traj[f] - out["split"].traj[f]).max() <= 1e-6 * max(1.0, np.abs(out["split"].traj[f]).max())
        idx = np.linspace(0, B - 1, min(B, 24)).astype(int)
        ref = coracle.solve_batch(S[idx], nt, 500, 1e-9)
        assert np.abs(out["persist"].iters[idx].astype(int) - ref["iters"]).max() <= (0 if nt >= 200 else 1)
        assert np.abs(out["persist"].tf[idx] - ref["tf"]).max() <= 1e-9
    monkeypatch.setenv("ASCENT_PIPELINE", "persist")
    # warm start, iteration cap, a problem that cannot converge, the default dispatch
    S = A.sweep_isp_drymass(6, 5)
    w = A.solve_batch(S, NT, tol=1e-9, guess=out["persist"].blob[:, :1].repeat(30, 1) if False else A.solve_batch(S, NT, tol=1e-9, want_blob=True).blob,
                      warm_start=2, mu_init=1e-9)
    assert np.all(w.status == 0) and w.iters.max() <= 8
    m = A.solve_batch(S[:5], NT, tol=1e-9, max_iter=4, coarse_nodes=-1)
    assert np.all(m.status == 1) and np.all(m.iters == 4)
    bad = A.solve_batch(A.AscentParams(Ft=3000.0).as_row()[None].repeat(9, 0), NT, tol=1e-9, max_iter=60)
    assert np.all(bad.status != 0)
    monkeypatch.delenv("ASCENT_PIPELINE")
    S = A.sweep_isp_drymass()
    d = A.solve_batch(S, NT, tol=1e-9, want_traj=False)                     # default dispatch at 4096 = the persistent kernel
    monkeypatch.setenv("ASCENT_PIPELINE", "split")
    s = A.solve_batch(S, NT, tol=1e-9, want_traj=False)
    assert np.all(d.status == 0) and np.array_equal(d.iters, s.iters) and np.abs(d.tf - s.tf).max() <= 1e-12


def test_wide_and_one_lane_sweeps_agree(coracle, monkeypatch):
    """The split pipeline has two implementations of its three serial sweeps: one lane per NLP, and 16 lanes per
    NLP (DPP row broadcasts + LDS transpose; used for batches <= 4096; ASCENT_FACTOR=lane|wide overrides).  Same
    algorithm, different summation order: identical iteration counts, answers equal to rounding, both equal to
    the oracle; ragged batch sizes exercise partially filled wavefronts and workgroups of the 16-lane kernels."""
    for scheme, form, P in ((0, "current", A.sweep_isp_drymass(10, 7)),
                            (1, "current", A.sweep_isp_drymass(7, 5)),
                            (0, "v1", np.repeat(A.AscentParams(r_peri=53108.4, r_apo=53108.4, mass_scalar=2576.0).as_row()[None], 3, 0))):
        out = {}
        for mode in ("lane", "wide"):
            monkeypatch.setenv("ASCENT_PIPELINE", "split")
            monkeypatch.setenv("ASCENT_FACTOR", mode)
            out[mode] = A.solve_batch(P, NT, tol=1e-9, want_blob=True, formulation=form, scheme=scheme, max_iter=500)
            assert np.all(out[mode].status == 0)
        assert np.array_equal(out["lane"].iters, out["wide"].iters)
        assert np.abs(out["lane"].tf - out["wide"].tf).max() <= 1e-12
        assert np.abs(out["lane"].blob - out["wide"].blob).max() <= 1e-6 * np.abs(out["lane"].blob).max()
        ref = coracle.solve_batch(P, NT, 500, 1e-9, formulation=1 if form == "v1" else 0, scheme=scheme)
        assert np.array_equal(out["wide"].iters, ref["iters"])
        assert np.abs(out["wide"].tf - ref["tf"]).max() <= 1e-9 * ref["tf"].max()
    # the inertia-correction path of the 16-lane factorisation (needs a regularised step somewhere in the sweep)
    S = A.sweep_isp_drymass()[::37]
    monkeypatch.setenv("ASCENT_FACTOR", "wide")
    w = A.solve_batch(S, NT, tol=1e-9)
    monkeypatch.setenv("ASCENT_FACTOR", "lane")
    l = A.solve_batch(S, NT, tol=1e-9)
    assert np.all(w.status == 0) and np.array_equal(w.iters, l.iters) and np.abs(w.tf - l.tf).max() <= 1e-12


def test_ragged_batch_and_small_grids(coracle):
    """Batch sizes that are not multiples of the wave size, and other grid sizes."""
    for B, nt in ((1, 3), (3, 12), (65, 50), (130, 25)):
        S = A.sweep_isp_drymass(B, 1)
        r = A.solve_batch(S, nt, tol=1e-8)
        idx = sorted({0, B // 2, B - 1})
        ref = coracle.solve_batch(S[idx], nt, 300, 1e-8)
        assert np.array_equal(r.status[idx], ref["status"])
        ok = ref["status"] == 0
        assert np.abs(r.tf[idx][ok] - ref["tf"][ok]).max(initial=0) <= 1e-8


def test_warm_start_from_nominal(nominal_gpu):
    """Continuation: primal-dual warm start from the nominal solution converges to the same
    optimum as the cold start in fewer iterations (policy stated with every throughput number)."""
    S = A.sweep_isp_drymass(4, 4, isp=(305.0, 315.0), dry=(2400.0, 2490.0))
    cold = A.solve_batch(S, NT, tol=1e-9)
    guess = np.repeat(nominal_gpu.blob, len(S), axis=1)
    warm = A.solve_batch(S, NT, tol=1e-9, guess=guess, warm_start=2, mu_init=1e-3)
    assert np.all(cold.status == 0) and np.all(warm.status == 0)
    assert np.abs(warm.tf - cold.tf).max() <= 1e-8
    assert warm.iters.mean() < cold.iters.mean()


def test_config3_full_size_properties():
    """BASELINE.json config 3 at full size (4096 NLPs): size-independent properties."""
    S = A.sweep_isp_drymass()
    r = A.solve_batch(S, NT, tol=1e-9)
    assert np.all(r.status == 0)
    f = A.PARAM_FIELDS
    rho0 = S[:, f.index("R0")] / S[:, f.index("r_peri")]
    x, y, vx, vy = (r.field(n)[-1] for n in ("x", "y", "xdot", "ydot"))
    # terminal constraints (Launch_Optimiser.py:158-173) hold for every problem
    assert np.abs(np.hypot(x, y + rho0) - (rho0 + 1)).max() < 1e-7
    vp2 = (6.674e-11 * 7.346e22 / (1738100 + 0.5 * (17703 + 88615))) / 17703 ** 2
    assert np.abs(vx * vx + vy * vy - vp2).max() < 1e-8
    assert np.abs((y + rho0) * vy + x * vx).max() < 1e-8
    # bounds
    assert np.all(np.abs(r.field("angledoubledot")) <= 1 + 1e-9)
    assert r.field("angle").min() >= -1e-12 and r.field("angle").max() <= np.pi / 3 + 1e-12
    assert r.field("mass").max() <= 1 + 1e-12
    # mass is linear in time for every problem (Launch_Optimiser.py:123)
    k = np.arange(NT)[:, None]
    mrate = S[:, f.index("mdot")] / S[:, f.index("fuel_mass")]
    assert np.abs(r.field("mass") - mrate * (k / K) * r.tf * 470.0).max() < 1e-9
    # physics: ascent time falls as Isp falls at fixed dry mass?  No -- lower Isp burns more mass per
    # second, so the vehicle gets lighter faster: t_f must be monotone along each sweep axis.
    tf = r.tf.reshape(64, 64)
    assert np.all(np.diff(tf, axis=1) > 0)        # heavier dry mass -> longer ascent
    assert np.all(np.diff(tf, axis=0) > 0)        # higher Isp (lower mdot) -> longer ascent
    # idempotence: solving a permuted batch gives bit-identical per-problem answers
    perm = np.random.default_rng(0).permutation(len(S))
    r2 = A.solve_batch(S[perm], NT, tol=1e-9, want_traj=False)
    assert np.array_equal(r2.tf, r.tf[perm]) and np.array_equal(r2.iters, r.iters[perm])


def test_mesh_refinement_matches_oracle_and_richardson(coracle, monkeypatch):
    """Other grid sizes through the same path: N = 400 against the oracle, and first-order convergence of the
    backward-Euler scheme: 2*t_f(400) - t_f(200) = 435.217 s, the mesh-converged value
    the trapezoid probe gave (435.227 s)."""
    P = A.AscentParams()
    r2, r4 = A.solve_batch(P, 200, tol=1e-9), A.solve_batch(P, 400, tol=1e-9)
    ref = coracle.solve_batch(P.as_row()[None], 400, 300, 1e-9)
    assert r4.status[0] == 0 and ref["status"][0] == 0
    # (a single NLP on 400 nodes runs on the dense-block path with the PCR Newton solve, whose curvature rule may pick other
    #  regularisations on the coarse levels than the exact inertia does: a few iterations more or less, same optimum; the
    #  hand-tuned kernels follow the oracle's rule -- their count is the oracle's up to the rounding knife edge of a
    #  coarse level's convergence test)
    assert abs(r4.tf[0] - ref["tf"][0]) <= 1e-9 * ref["tf"][0] and abs(int(r4.iters[0]) - int(ref["iters"][0])) <= 4
    monkeypatch.setenv("ASCENT_SMALL_BATCH", "off")
    h4 = A.solve_batch(P, 400, tol=1e-9)
    monkeypatch.delenv("ASCENT_SMALL_BATCH")
    assert abs(h4.tf[0] - ref["tf"][0]) <= 1e-9 * ref["tf"][0] and abs(int(h4.iters[0]) - int(ref["iters"][0])) <= 1
    assert abs(r4.final_time()[0] - 434.6222) < 2e-3              # survey probe: 434.62229 s
    assert abs(2 * r4.final_time()[0] - r2.final_time()[0] - 435.217) < 0.02


def test_non_converged_problems_are_flagged():
    """max_iter too small -> status max_iter, never silently 'converged'."""
    r = A.solve_batch(A.sweep_isp_drymass(2, 2), NT, tol=1e-9, max_iter=5, coarse_nodes=-1)
    assert np.all(r.status == 1) and np.all(r.iters == 5)
    r = A.solve_batch(A.sweep_isp_drymass(2, 2), NT, tol=1e-9, max_iter=5)          # per level: 5 + 5 + 5 (17 -> 60 -> 200 nodes)
    assert np.all(r.status == 1) and np.all(r.iters == 15)
    # an infeasible problem (far too little thrust) must not report convergence
    bad = A.AscentParams(Ft=3000.0)
    rb = A.solve_batch(bad, NT, tol=1e-9, max_iter=60)
    assert rb.status[0] != 0


def test_trapezoid_scheme_matches_oracle(coracle):
    """scheme=1 (trapezoid, control held over the step; BASELINE.json configs name 'N=200 trapezoidal'):
    not a reference scheme -- the reference's NODES=2 is backward Euler -- so it is checked against the oracle
    in the same scheme and against SURVEY.md Appendix C's independent probe value 435.227 s."""
    P = A.AscentParams()
    r = A.solve_batch(P, NT, tol=1e-9, scheme="trapezoid")
    ref = coracle.solve_batch(P.as_row()[None], NT, 300, 1e-9, scheme=1)
    assert r.status[0] == 0 and ref["status"][0] == 0
    assert abs(r.final_time()[0] - 435.22715) < 5e-3
    assert abs(r.tf[0] - ref["tf"][0]) <= 1e-9 * ref["tf"][0]
    assert np.abs(r.traj[:, :, 0] - ref["traj"][0]).max() < 1e-7
    S = A.sweep_isp_drymass(6, 5)
    rb = A.solve_batch(S, NT, tol=1e-9, scheme=1)
    refb = coracle.solve_batch(S, NT, 300, 1e-9, scheme=1)
    coracle.set_scheme(0)
    assert np.all(rb.status == 0) and np.all(refb["status"] == 0)
    assert np.abs(rb.tf - refb["tf"]).max() <= 1e-9 * refb["tf"].max()
    # second order vs first order: the trapezoid answer is the mesh-converged one (Richardson of backward Euler)
    assert abs(rb.final_time()[0] - A.solve_batch(S[:1], 400, tol=1e-9, scheme=1).final_time()[0]) < 0.01


def test_v1_formulation_matches_second_golden_vector(coracle, golden):
    """formulation=1: the v1 script of the PDF appendix (p26-28; the angle itself is the MV, circular target,
    mass_scalar 2576 with mflow 5.053/2376).  Second golden vector: the numbers printed on PDF p30."""
    P = A.AscentParams(r_peri=53108.4, r_apo=53108.4, mass_scalar=2576.0)
    r = A.solve_batch(P, NT, tol=1e-9, formulation="v1", max_iter=500)
    assert r.status[0] == 0
    g, S = golden["v1"], 53108.4
    assert abs(r.final_time()[0] - g["final_time"]) <= 1e-4 * g["final_time"]
    assert abs(r.tf[0] - g["tf"]) <= 1e-4 * g["tf"]
    tr = r.traj[:, :, 0]
    assert abs(-tr[0, -1] * S - g["final_x_flipped"]) <= 1e-4 * g["final_x_flipped"]        # the v1 prints flip x
    assert abs(tr[1, -1] * S - g["final_y"]) <= 1e-4 * g["final_x_flipped"]
    assert abs(-tr[2, -1] * S - g["final_xdot_flipped"]) <= 1e-4 * g["final_xdot_flipped"]
    assert abs(tr[3, -1] * S - g["final_ydot"]) <= 1e-4 * g["final_xdot_flipped"]
    assert abs(-tr[4, -1] * S - g["final_xdoubledot_flipped"]) <= 2e-3 * g["final_xdoubledot_flipped"]
    ang = 3 * tr[6] * 180 / np.pi
    assert 33 < ang[1] < 37 and 109 < ang[-1] < 113 and np.abs(tr[7]).max() == 0.0    # PDF p21,31 plot facts
    # against the oracle in the same embedding, and a small sweep
    ref = coracle.solve_batch(P.as_row()[None], NT, 500, 1e-9, formulation=1)
    assert abs(r.tf[0] - ref["tf"][0]) <= 1e-9 * ref["tf"][0] and r.iters[0] == ref["iters"][0]
    S8 = A.sweep_isp_drymass(3, 3, base=P)
    rb = A.solve_batch(S8, NT, tol=1e-9, formulation=1, max_iter=500)
    refb = coracle.solve_batch(S8, NT, 500, 1e-9, formulation=1)
    coracle.set_formulation(0)
    assert np.all(rb.status == 0) and np.abs(rb.tf - refb["tf"]).max() <= 1e-9 * refb["tf"].max()


def test_orbit_of_the_insertion_state(nominal_gpu):
    """Kepler-exact orbit of the final state.  The reference targets the circular speed of the mean radius
    (1654.40 m/s, Launch_Optimiser.py:72-78) at 17.7 km altitude with r.v = 0; the local circular speed there is
    1671.0 m/s, so the modelled insertion point is the APOAPSIS of the resulting two-body orbit (the 87 x 17 km
    ellipse would need 1687.5 m/s).  The restatement reproduces that property of the reference faithfully."""
    o = nominal_gpu.orbit()
    assert abs(o["apoapsis_alt"][0] - 17703.0) < 1.0            # insertion altitude, r.v = 0
    assert abs(o["flight_path_angle"][0]) < 1e-9
    mu, r = 6.674e-11 * 7.346e22, 1738100.0 + 17703.0
    a = 1.0 / (2.0 / r - 1654.3956154295 ** 2 / mu)
    assert abs(o["semi_major_axis"][0] - a) < 1.0
    assert o["periapsis_alt"][0] < 0                             # below the surface: v < local circular speed


def test_nested_iteration_matches_single_grid_and_oracle(coracle, monkeypatch):
    """Cold starts solve a coarse grid first and warm-start the requested grid from its prolonged primal-dual
    solution (ascent_opts.coarse_nodes; include/ascent.h).  Same NLP, same tolerance: the answers agree with the
    single-grid solve to the solver tolerance; the oracle runs the same nested iteration (same iteration counts);
    all three solver paths do it."""
    S = A.sweep_isp_drymass(9, 8)
    single = A.solve_batch(S, NT, tol=1e-9, coarse_nodes=-1)
    ref = coracle.solve_batch(S, NT, 300, 1e-9)
    for mode, fac in (("split", "wide"), ("split", "lane"), ("fused", "lane")):
        monkeypatch.setenv("ASCENT_PIPELINE", mode)
        monkeypatch.setenv("ASCENT_FACTOR", fac)
        nested = A.solve_batch(S, NT, tol=1e-9)
        assert np.all(nested.status == 0) and np.all(single.status == 0)
        assert np.abs(nested.tf - single.tf).max() <= 2e-9
        # states to 1e-4 of their scale; the control on the singular arc is only weakly determined by a KKT point of
        # tolerance 1e-9 (the single-grid solution itself moves by 0.3 in u between tol 1e-9 and 1e-12), so it is
        # compared through the angle it integrates to
        for f in (0, 1, 2, 3, 6, 9):
            assert np.abs(nested.traj[f] - single.traj[f]).max() <= 1e-4 * np.abs(single.traj[f]).max()
        assert np.array_equal(nested.iters, ref["iters"])             # both levels counted, exactly as the oracle does
        assert np.abs(nested.tf - ref["tf"]).max() <= 1e-9
    monkeypatch.delenv("ASCENT_PIPELINE"); monkeypatch.delenv("ASCENT_FACTOR")
    # explicit coarse grid; three levels on a fine grid; the other scheme and formulation
    e = A.solve_batch(S[:8], NT, tol=1e-9, coarse_nodes=26)
    oe = coracle.solve_batch(S[:8], NT, 300, 1e-9, coarse_nodes=26)
    assert np.all(e.status == 0) and np.array_equal(e.iters, oe["iters"]) and np.abs(e.tf - single.tf[:8]).max() <= 2e-9
    h = A.solve_batch(S[:4], 1000, tol=1e-9, max_iter=500)
    h1 = A.solve_batch(S[:4], 1000, tol=1e-9, max_iter=500, coarse_nodes=-1)
    assert np.all(h.status == 0) and np.all(h1.status == 0) and np.abs(h.tf - h1.tf).max() <= 2e-9
    t = A.solve_batch(S[:6], NT, tol=1e-9, scheme=1)
    t1 = A.solve_batch(S[:6], NT, tol=1e-9, scheme=1, coarse_nodes=-1)
    assert np.all(t.status == 0) and np.abs(t.tf - t1.tf).max() <= 2e-9
    P1 = A.AscentParams(r_peri=53108.4, r_apo=53108.4, mass_scalar=2576.0)
    v = A.solve_batch(P1, NT, tol=1e-9, formulation="v1", max_iter=500)
    v1 = A.solve_batch(P1, NT, tol=1e-9, formulation="v1", max_iter=500, coarse_nodes=-1)
    ov = coracle.solve_batch(P1.as_row()[None], NT, 500, 1e-9, formulation=1)
    assert v.status[0] == 0 and abs(v.tf[0] - v1.tf[0]) <= 2e-9 and v.iters[0] == ov["iters"][0]


def test_independent_sweep_corners():
    """tests/golden/sweep_corners.json: the numpy generic-LU oracle's solutions of the four config-3 corners and the
    sixteen config-4 corners (made by scripts/make_sweep_corners.py) -- independent anchors away from nominal."""
    import json, os
    fx = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "sweep_corners.json")))
    for grp in ("config3", "config4"):
        P = np.array([[e["params"][f] for f in A.PARAM_FIELDS] for e in fx[grp]])
        r = A.solve_batch(P, fx["nt"], tol=1e-10)
        assert np.all(r.status == 0)
        assert np.abs(r.tf - np.array([e["tf"] for e in fx[grp]])).max() <= 1e-9
        for name, key in (("x", "final_x"), ("y", "final_y"), ("xdot", "final_xdot"), ("ydot", "final_ydot"),
                          ("angle", "final_angle"), ("mass", "final_mass")):
            # states to 1e-6: the end of the singular arc is only weakly determined by a KKT point
            assert np.abs(r.field(name)[-1] - np.array([e[key] for e in fx[grp]])).max() <= 1e-6


def _check_against_oracle_samples(coracle, S, r, idx, tol=1e-9):
    ref = coracle.solve_batch(S[idx], NT, 300, tol)
    assert np.all(ref["status"] == 0)
    assert np.abs(r.tf[idx] - ref["tf"]).max() <= 1e-9 * ref["tf"].max()
    assert np.array_equal(r.iters[idx], ref["iters"])
    for f in (0, 1, 2, 3, 6, 9):
        assert np.abs(np.moveaxis(r.traj[f][:, idx], 1, 0) - ref["traj"][:, f]).max() <= 1e-6 * max(1.0, np.abs(ref["traj"][:, f]).max())


def test_config4_shard_default_dispatch(coracle, monkeypatch):
    """BASELINE.json configs[3]: one contiguous 32 768-NLP shard of the 262 144-problem config-4 box (what each of
    the 8 GPUs solves), through the DEFAULT dispatch -- the persistent kernel at every size since round 2 (round 1: the fused k_solve).  Every problem
    converges; 64 spread samples equal the oracle (same iteration counts, t_f to 1e-9)."""
    monkeypatch.delenv("ASCENT_PIPELINE", raising=False)
    monkeypatch.delenv("ASCENT_FACTOR", raising=False)
    full = A.sweep_config4()
    assert full.shape == (262144, 16)
    S = np.ascontiguousarray(full[:32768])
    r = A.solve_batch(S, NT, tol=1e-9)
    assert np.all(r.status == 0)
    idx = np.linspace(0, len(S) - 1, 64).astype(int)
    _check_against_oracle_samples(coracle, S, r, idx)
    # the two extra sweep axes (Launch_Optimiser.py:66,71) really vary inside the shard
    f = A.PARAM_FIELDS
    assert len(np.unique(S[:, f.index("r_apo")])) == 8 and len(np.unique(S[:, f.index("ang_acc_max")])) == 8
    # size-independent properties on all 32 768
    rho0 = S[:, f.index("R0")] / S[:, f.index("r_peri")]
    x, y, vx, vy = (r.field(n)[-1] for n in ("x", "y", "xdot", "ydot"))
    assert np.abs(np.hypot(x, y + rho0) - (rho0 + 1)).max() < 1e-7
    assert np.abs((y + rho0) * vy + x * vx).max() < 1e-8
    assert np.all(np.abs(r.field("angledoubledot")) <= 1 + 1e-9)


def test_config4_every_eighth_problem(coracle, monkeypatch):
    """The other cut through the config-4 box: every 8th problem (all 64 x 64 x 8 (Isp, dry mass, apoapsis)
    combinations at one angular-acceleration cap per stride), 32 768 NLPs, default dispatch."""
    monkeypatch.delenv("ASCENT_PIPELINE", raising=False)
    monkeypatch.delenv("ASCENT_FACTOR", raising=False)
    S = np.ascontiguousarray(A.sweep_config4()[3::8])
    r = A.solve_batch(S, NT, tol=1e-9, want_traj=True)
    assert np.all(r.status == 0)
    _check_against_oracle_samples(coracle, S, r, np.linspace(0, len(S) - 1, 48).astype(int))


def test_high_resolution_grid_matches_oracle(coracle):
    """N = 2000 nodes (BASELINE.json configs[4]'s grid size) with the two schemes of the hand-tuned path: the nominal
    problem and a 16-NLP sweep against the oracle; backward Euler lands on its Richardson prediction 435.10 s
    (SURVEY.md Appendix C), the trapezoid rule on the mesh-converged 435.23 s."""
    S = np.vstack([A.AscentParams().as_row()[None], A.sweep_isp_drymass(4, 4)])
    for scheme, t_expect in ((0, 435.104), (1, 435.225)):
        r = A.solve_batch(S, 2000, tol=1e-9, max_iter=500, scheme=scheme)
        ref = coracle.solve_batch(S, 2000, 500, 1e-9, scheme=scheme)
        coracle.set_scheme(0)
        assert np.all(r.status == 0) and np.all(ref["status"] == 0)
        assert np.abs(r.tf - ref["tf"]).max() <= 1e-9 * ref["tf"].max()
        assert np.abs(r.iters.astype(int) - ref["iters"]).max() <= 1      # (coarse-level convergence test is a rounding knife edge)
        assert abs(r.final_time()[0] - t_expect) < 0.01
        for f in (0, 1, 2, 3, 6, 9):
            assert np.abs(np.moveaxis(r.traj[f], 1, 0) - ref["traj"][:, f]).max() <= 1e-6 * max(1.0, np.abs(ref["traj"][:, f]).max())


_TWO_STREAMS = r"""
import sys, numpy as np, torch
torch.cuda.set_device(0)                      # torch's HIP runtime first, as in bench.py (the library then binds to the same one)
sys.path.insert(0, %r)
import lunar_module_ascent_trajectory_optimiser_amd as A
dev = torch.device("cuda", 0)
Pa = torch.from_numpy(A.sweep_isp_drymass(16, 16)).to(dev)
Pb = torch.from_numpy(np.ascontiguousarray(A.sweep_config4()[::1031][:200])).to(dev)
ref_a = {k: v.clone() for k, v in A.solve_batch_torch(Pa, 200, tol=1e-9, sync=True).items()}
ref_b = {k: v.clone() for k, v in A.solve_batch_torch(Pb, 120, tol=1e-9, sync=True).items()}
sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
oa, ob = {}, {}
for _ in range(4):
    with torch.cuda.stream(sa):
        A.solve_batch_torch(Pa, 200, tol=1e-9, out=oa)
    with torch.cuda.stream(sb):
        A.solve_batch_torch(Pb, 120, tol=1e-9, out=ob)
torch.cuda.synchronize(dev)
for o, r in ((oa, ref_a), (ob, ref_b)):
    assert bool((o["status"] == 0).all()) and torch.equal(o["iters"], r["iters"])
    assert torch.equal(o["tf"], r["tf"]) and torch.equal(o["traj"], r["traj"])
# the move penalty through the device-resident entry (parameters in HBM: the positive-weight check is the caller's)
Pc = Pa[:8].clone(); Pc[:, 15] = 1e-5
mp = A.solve_batch_torch(Pc, 100, tol=1e-9, sync=True, move_penalty=True, max_iter=500)
host = A.solve_batch(Pc.cpu().numpy(), 100, tol=1e-9, move_penalty=True, max_iter=500)
assert bool((mp["status"] == 0).all()) and np.array_equal(mp["tf"].cpu().numpy(), host.tf) and np.all(host.tf > ref_a["tf"][:8].cpu().numpy() - 1.0)
print("two-streams-ok")
"""


def test_solves_on_two_streams_overlap_safely():
    """One workspace per caller stream (include/ascent.h, Concurrency): solves enqueued alternately on two streams, different
    batches and grids in flight at once, give bit-identical results to the same solves run one after another.  (In a process of
    its own: torch has to bring up its HIP runtime before the library binds to one.)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _TWO_STREAMS % root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "two-streams-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_unusual_grid_sizes_match_oracle(coracle):
    """Tiny grids, grids around the 16-interval chunk boundaries of the persistent kernel, grids with several nested levels:
    same status, same iteration counts and t_f to rounding as the C oracle on every problem."""
    S = A.sweep_isp_drymass(3, 3)
    for nt in (3, 4, 5, 8, 14, 16, 17, 18, 32, 33, 34, 49, 65, 199, 201, 257, 640):
        r = A.solve_batch(S, nt, tol=1e-9, max_iter=500)
        o = coracle.solve_batch(S, nt, 500, 1e-9)
        assert np.array_equal(r.status, o["status"]) and np.all(r.status == 0), nt
        assert np.array_equal(r.iters, o["iters"]), nt
        assert np.abs(r.tf - o["tf"]).max() <= 1e-12, nt


def test_config4_whole_box_on_one_gpu(coracle):
    """BASELINE.json configs[3] in full -- 262 144 NLPs (64 x 64 x 8 x 8: Isp, dry mass, apoapsis, angular-acceleration cap) -- as
    ONE batch on one GPU: every problem converges; a shard solved on its own gives bit-identical results (what each of
    eight GPUs would compute); spread samples agree with the oracle with equal iteration counts."""
    full = A.sweep_config4()
    r = A.solve_batch(full, NT, tol=1e-9, want_traj=False)
    assert len(full) == 262144 and np.all(r.status == 0) and r.iters.max() <= 30
    sh = A.solve_batch(full[5 * 32768:6 * 32768], NT, tol=1e-9, want_traj=False)
    assert np.array_equal(sh.tf, r.tf[5 * 32768:6 * 32768]) and np.array_equal(sh.iters, r.iters[5 * 32768:6 * 32768])
    idx = np.linspace(0, len(full) - 1, 48).astype(int)
    ref = coracle.solve_batch(full[idx], NT, 300, 1e-9)
    assert np.array_equal(r.iters[idx], ref["iters"]) and np.abs(r.tf[idx] - ref["tf"]).max() <= 1e-12
    # the same box of the model the reference declares -- with its MV DCOST as the l1 move penalty (Launch_Optimiser.py:99)
    full[:, 15] = 1e-5
    rd = A.solve_batch(full, NT, tol=1e-9, want_traj=False, move_penalty=True)
    assert np.all(rd.status == 0) and rd.iters.max() <= 32 and np.all(rd.tf > r.tf) and np.all(rd.tf - r.tf < 1e-4)
    refd = coracle.solve_batch(full[idx], NT, 300, 1e-9, move_penalty=True)
    assert np.abs(rd.iters[idx].astype(int) - refd["iters"]).max() <= 1 and np.abs(rd.tf[idx] - refd["tf"]).max() <= 1e-9


def test_persistent_kernel_trapezoid_matches_split_pipeline_and_oracle(coracle, monkeypatch):
    """scheme 1 (trapezoid, control held over the step) through the persistent kernel -- second evaluation point of every
    step, pull-back of the value function through Abar = I + (dt/2) F_z in the factorisation, Abar folded into the affine
    forward / adjoint recursions -- against the split pipeline (which carried the trapezoid in round 1) and the oracle:
    identical iteration counts on nested grids, t_f to rounding; ragged batches and chunks."""
    for B, nt in ((5, 200), (67, 200), (1000, 200), (9, 1000)):
        S = A.sweep_isp_drymass()[:: max(1, 4096 // B)][:B]
        out = {}
        for mode in ("persist", "split"):
            monkeypatch.setenv("ASCENT_PIPELINE", mode)
            out[mode] = A.solve_batch(S, nt, tol=1e-9, scheme=1, max_iter=500)
            assert np.all(out[mode].status == 0)
        assert np.array_equal(out["persist"].iters, out["split"].iters)
        assert np.abs(out["persist"].tf - out["split"].tf).max() <= 1e-12
        for f in (0, 1, 2, 3, 6, 9):
            assert np.abs(out["persist"].traj[f] - out["split"].traj[f]).max() <= 1e-6 * max(1.0, np.abs(out["split"].traj[f]).max())
        idx = np.linspace(0, B - 1, min(B, 16)).astype(int)
        ref = coracle.solve_batch(S[idx], nt, 500, 1e-9, scheme=1)
        coracle.set_scheme(0)
        assert np.array_equal(out["persist"].iters[idx], ref["iters"]) and np.abs(out["persist"].tf[idx] - ref["tf"]).max() <= 1e-12
    monkeypatch.delenv("ASCENT_PIPELINE")
    assert A.default_path(4096, NT, scheme=1) == "persist"
    r = A.solve_batch(A.AscentParams(), NT, tol=1e-9, scheme=1)
    assert r.status[0] == 0 and abs(r.final_time()[0] - 435.22714) < 1e-4          # SURVEY Appendix C's independent trapezoid probe: 435.22715 s


def test_persistent_kernel_tight_tolerances_on_the_config4_box(coracle):
    """The persistent kernel evaluates the Jacobian blocks of a node again in every phase; the phases must see the same bits
    (floating-point contraction is pinned to the statement level in ascent_persist.hip).  A 1e-16 difference between the
    implicit block of the factor phase and that of the sweeps is multiplied by sigma = z/s ~ 1e12 of the eliminated terminal
    slacks: before the pin the trapezoid needed up to 58 iterations where the oracle needs 28 at tol 1e-9 and ran into
    max_iter at 1e-10.  64 NLPs across BASELINE config 4's box, both schemes: iteration counts of the oracle (equal at
    1e-9, within 2 at 1e-10), every NLP converged."""
    S = A.sweep_config4()[::4099][:64]
    for scheme in (0, 1):
        for tol, slack in ((1e-9, 0), (1e-10, 2)):
            r = A.solve_batch(S, 200, tol=tol, scheme=scheme, max_iter=500)
            ref = coracle.solve_batch(S, 200, 500, tol, scheme=scheme)
            coracle.set_scheme(0)
            assert np.all(r.status == 0) and np.all(ref["status"] == 0)
            assert np.abs(r.iters.astype(int) - ref["iters"]).max() <= slack, (scheme, tol, r.iters, ref["iters"])
            assert np.abs(r.tf - ref["tf"]).max() <= 1e-10


def test_newton_step_residual_with_inconsistent_slack_multipliers(coracle):
    """The Newton step of every hand-tuned path at an iterate whose terminal slack multipliers do not match their constraint
    multipliers (what a truncated dual step leaves behind: nu_i + z_i != 0), against the generic sparse LU: the multiplier
    steps of the terminal inequalities (sigma ~ 1e12 there) and of the defects.  This is the iterate at which the persistent
    kernel's trapezoid lost four digits before its phases were made to evaluate bit-identical blocks."""
    from conftest import generic_lu_newton_step, params_of_row
    S = A.sweep_config4()[::4099][:64]
    nt, K = 200, 199
    for scheme in (0, 1):
        sol = coracle.solve_batch(S[42:43], nt, 500, 1e-8, want_blob=True, scheme=scheme)
        coracle.set_scheme(0)
        blob = sol["blob"][0].copy()
        blob[21 * K + 5] *= 0.9
        blob[21 * K + 6] *= 0.9
        lu = generic_lu_newton_step(params_of_row(S[42]), nt, blob, 1e-9, 0.0, scheme)[0]
        for path in ("persist", "split_wide", "split_lane"):
            step = A.kkt_step(S[42:43], blob[:, None], 1e-9, 0.0, nt, path=path, scheme=scheme)[0][:, 0]
            for j in (5, 6, 8, 9):        # d zs1, d zs2, d nu1, d nu2: 1e-10 of the multipliers themselves (z_s2 ~ 30; before the pin: 1.6e-8)
                assert abs(step[21 * K + j] - lu[21 * K + j]) <= 1e-10 * max(1.0, abs(blob[21 * K + 6])), (scheme, path, j)
            dl = np.abs(step[8 * K:15 * K] - lu[8 * K:15 * K]).max()
            assert dl <= 1e-9, (scheme, path, dl)                  # (before the pin: 2.1e-8)


def test_persistent_kernel_v1_formulation_matches_split_pipeline_and_oracle(coracle, monkeypatch):
    """formulation 1 (the v1 script of the PDF appendix: the angle itself is the MV, an algebraic row without coupling to the
    previous step) through the persistent kernel: identical iteration counts and t_f to rounding against the split pipeline and
    the oracle, single grids and nested ones; the second golden vector through the default dispatch."""
    base = A.AscentParams(**V1)
    for shape, nt in (((1, 1), 200), ((3, 2), 200), ((13, 10), 37), ((32, 32), 200), ((3, 3), 1000)):
        S = A.sweep_isp_drymass(*shape, base=base)
        out = {}
        for mode in ("persist", "split"):
            monkeypatch.setenv("ASCENT_PIPELINE", mode)
            out[mode] = A.solve_batch(S, nt, tol=1e-9, formulation="v1", max_iter=500)
            assert np.all(out[mode].status == 0)
        assert np.array_equal(out["persist"].iters, out["split"].iters)
        assert np.abs(out["persist"].tf - out["split"].tf).max() <= 1e-12
        assert np.abs(out["persist"].traj - out["split"].traj).max() <= 1e-9
        idx = np.linspace(0, len(S) - 1, min(len(S), 16)).astype(int)
        ref = coracle.solve_batch(S[idx], nt, 500, 1e-9, formulation=1)
        coracle.set_formulation(0)
        assert np.array_equal(out["persist"].iters[idx], ref["iters"]) and np.abs(out["persist"].tf[idx] - ref["tf"]).max() <= 1e-12
    monkeypatch.delenv("ASCENT_PIPELINE")
    assert A.default_path(1, NT, formulation=1) == "persist"
    v = A.solve_batch(base, NT, tol=1e-9, formulation="v1", max_iter=500)
    assert v.status[0] == 0 and abs(v.final_time()[0] - 435.29773) < 2e-3        # PDF p30: 435.29773 s (here 435.29896)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,mp,terminal,formulation", [(0, False, 0, 0), (1, False, 0, 0), (0, True, 0, 0), (1, True, 0, 0), (0, False, 0, 1),
                                                            (0, True, 0, 1), (0, False, 2, 0), (1, False, 2, 0), (0, True, 2, 0), (1, True, 2, 0)])
def test_one_nlp_per_wavefront_equals_four_per_wavefront(monkeypatch, scheme, mp, terminal, formulation):
    """Every variant of the persistent kernel (scheme x move penalty x terminal condition x formulation) exists in both forms --
    four NLPs per wavefront with 16-node chunks, and one NLP per wavefront with 64-node chunks (the default for batches <= 1024:
    ASCENT_PERSIST_WIDE overrides).  Same arithmetic per node and per sweep step (sums over the nodes run 16 or 64 at a time), so: identical iteration
    counts and t_f to 1e-12 -- with terminal 2 (two nearly dependent conditions, iteration counts that depend on the last bit) convergence and t_f to 5e-9 -- on a ragged batch and on grids that end inside a chunk of either form."""
    S = A.sweep_isp_drymass(3, 3)[:7]
    S[:, 15] = 1e-5
    for nt in (60, 131):
        out = {}
        for wide in ("0", "1"):
            monkeypatch.setenv("ASCENT_PERSIST_WIDE", wide)
            assert A.default_path(len(S), nt, scheme=scheme, move_penalty=mp, terminal=terminal, formulation=formulation) == "persist"
            out[wide] = A.solve_batch(S, nt, tol=1e-9, scheme=scheme, move_penalty=mp, terminal=terminal, formulation=formulation, max_iter=500)
        monkeypatch.delenv("ASCENT_PERSIST_WIDE")
        assert np.all(out["0"].status == 0) and np.all(out["1"].status == 0), (nt, out["0"].status, out["1"].status)
        if terminal == 2:      # (its two nearly dependent conditions: 50-60 iterations, the convergence test now and then a knife edge)
            assert np.abs(out["0"].tf - out["1"].tf).max() <= 5e-9      # (iteration counts: 29-94, and tens apart between the forms on single problems)
            continue          # (where on the ellipse the burn ends is a nearly flat direction of t_f: the states of two KKT points at tol 1e-9 differ by 1e-4)
        else:
            assert np.array_equal(out["0"].iters, out["1"].iters), (nt, out["0"].iters, out["1"].iters)
            assert np.abs(out["0"].tf - out["1"].tf).max() <= 1e-12
        assert np.abs(out["0"].traj[:8] - out["1"].traj[:8]).max() <= 1e-6      # (sums over the nodes run 16 / 64 at a time: the control at the junction of its arcs is only weakly determined)
