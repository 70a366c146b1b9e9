"""Flight verification (ascent_fly_batch) on the GPU: the kernels against the CPU reference integrators flown from the same
blob, against the committed fixtures (another solver's solution of the same NLP), on an exact synthetic blob, against each
other, over a whole sweep, and the surfaces built on them.

The differences seen are collected in PARITY; with ASCENT_FLIGHT_PARITY_OUT=<file> they are written there as JSON when the
module is done (profiles/flight_parity.json is such a file)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import flight_reference as fr
from gpu_cases import parity_writer, points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DCOST = 1e-4
_points = functools.partial(points, dcost=DCOST)
PARITY = {"reference_rk4": {}, "reference_dop853": {}, "fixtures": {}}
SI_ROWS = [0, 1, 2, 3, 4, 5, 6, 7]
_write_parity = parity_writer("ASCENT_FLIGHT_PARITY_OUT", PARITY)


def _lib():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    return _lib


def _combos():
    """every option combination ascent_solve_batch accepts"""
    out = []
    for scheme in (0, 1, 2):
        for form in ((0, 1) if scheme == 0 else (0,)):
            for term in ((0, 1) if form == 1 else (0, 1, 2)):
                for mp in (0, 1):
                    out.append((scheme, form, term, mp))
    return out


@pytest.mark.parametrize("scheme,form,term,mp", _combos())
def test_kernels_match_rk4_reference(scheme, form, term, mp):
    """Kernel against the numpy RK4 with the same m, flown from the same GPU blob, N = 200 (m = 5: 1000 RK4 steps): trajectory,
    local errors and summary to 1e-10 scaled (SI rows: times r_peri).  About 1000-2000 RK4 steps of states of size <= 17, a few
    ulp each from rcp, sincos_bounded and FMA contraction, give about 1e-12; the factor 100 covers the growth of a perturbation
    over one ascent."""
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch, fly_batch
    nt, P = 200, _points(2)
    kw = dict(scheme=scheme, formulation=form, terminal=term, move_penalty=bool(mp))
    r = solve_batch(P, nt, want_blob=True, **kw)
    assert (r.status == 0).all(), r.status
    f = fly_batch(P, r.blob, nt, **kw)
    assert f.traj.shape == (2, 10, nt) and f.local_error.shape == (2, nt - 1, 7) and f.summary.shape == (2, 10)
    worst = dict(traj=0.0, local=0.0, summary_si_over_r_peri=0.0)
    for j in range(P.shape[0]):
        ref = fr.fly(P[j], r.blob[:, j], nt, formulation=form)
        assert f.summary[j, 9] == ref["m"] == 5 and f.summary[j, 8] == ref["summary"][8]
        worst["traj"] = max(worst["traj"], np.abs(f.traj[j] - ref["traj"]).max())
        worst["local"] = max(worst["local"], np.abs(f.local_error[j] - ref["local"]).max())
        worst["summary_si_over_r_peri"] = max(worst["summary_si_over_r_peri"],
                                              np.abs(f.summary[j, SI_ROWS] - ref["summary"][SI_ROWS]).max() / P[j, 9])
        # the control row is the solve's own
        assert np.array_equal(f.traj[j, 8], r.traj[8, :, j])
    PARITY["reference_rk4"][f"scheme{scheme}_form{form}_term{term}_mp{mp}"] = worst
    print(scheme, form, term, mp, worst)
    assert max(worst.values()) <= 1e-10, worst


@pytest.mark.parametrize("scheme,nt", [(0, 200), (1, 200), (2, 50)])
def test_kernel_matches_dop853_reference(scheme, nt):
    """Kernel (automatic substeps) against DOP853 at rtol 1e-13 flown from the same GPU blob, nominal: end state within 1e-4 m
    and 1e-6 m/s, the RK4 truncation bound of tests/test_flight_reference.py."""
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch, fly_batch
    P = _points(1)
    r = solve_batch(P, nt, want_blob=True, scheme=scheme, tol=1e-10 if scheme == 2 else 1e-9, max_iter=500)
    assert r.status[0] == 0
    f = fly_batch(P, r.blob, nt, scheme=scheme)
    ref = fr.fly(P[0], r.blob[:, 0], nt, integrator="dop853")
    S = P[0, 9]
    dpos = S * np.hypot(*(f.traj[0, :2, -1] - ref["traj"][:2, -1]))
    dvel = S * np.hypot(*(f.traj[0, 2:4, -1] - ref["traj"][2:4, -1]))
    PARITY["reference_dop853"][f"scheme{scheme}_nt{nt}"] = dict(end_position_m=dpos, end_velocity_ms=dvel, miss_position_m=f.summary[0, 0],
                                                                  miss_position_dop853_m=ref["summary"][0])
    print(scheme, nt, dpos, dvel, f.summary[0], ref["summary"])
    assert dpos <= 1e-4 and dvel <= 1e-6
    assert abs(f.summary[0, 0] - ref["summary"][0]) <= 1e-4 and abs(f.summary[0, 1] - ref["summary"][1]) <= 1e-6


def _fixture_cases():
    with open(os.path.join(ROOT, "tests", "golden", "flight_fixtures.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _fixture_cases(), ids=lambda c: c["name"])
def test_kernel_matches_fixtures(case):
    """The GPU solve of the same NLP, flown on the GPU, against the CPU oracle's solution flown with DOP853: t_f equal to 1e-7 s,
    misses within 1e-4 m (m/s) + 1e-5 of the fixture's value, flown apsides within 0.1 m.  The relative part is there because
    two solvers stop at different points of the tolerance ball and the control on the singular arc is only weakly determined."""
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch
    P = np.array([case["params"]])
    hs = case["scheme"] == 2
    r = solve_batch(P, case["nt"], tol=1e-10 if hs else 1e-9, max_iter=500 if hs else 300, scheme=case["scheme"],
                    formulation=case["formulation"], terminal=case["terminal"], flight=True)
    assert r.status[0] == 0
    dtf = abs(r.tf[0] - case["tf"]) * P[0, 11]
    s, fx = r.flight.summary[0], case["summary"]
    d = dict(tf_s=dtf, miss_pos_m=s[0] - fx["miss_pos_m"], miss_vel_ms=s[1] - fx["miss_vel_ms"],
             flown_periapsis_m=s[2] - fx["flown_periapsis_alt_m"], flown_apoapsis_m=s[3] - fx["flown_apoapsis_alt_m"],
             max_local_pos_m=s[6] - fx["max_local_pos_m"], miss_pos_fixture_m=fx["miss_pos_m"])
    PARITY["fixtures"][case["name"]] = d
    print(case["name"], d)
    assert dtf <= 1e-7
    assert abs(d["miss_pos_m"]) <= 1e-4 + 1e-5 * fx["miss_pos_m"]
    assert abs(d["miss_vel_ms"]) <= 1e-4 + 1e-5 * fx["miss_vel_ms"]
    assert abs(d["flown_periapsis_m"]) <= 0.1 and abs(d["flown_apoapsis_m"]) <= 0.1


def test_exact_blob_has_no_error():
    """The integrator alone: a blob whose states are a DOP853 flight of an arbitrary control, substeps = 16 (0.13 s at N = 200):
    local error and miss <= 1e-9 scaled (see tests/test_flight_reference.py for the expected 4e-12)."""
    from lunar_module_ascent_trajectory_optimiser_amd import fly_batch
    nt, P = 200, _points(1)
    blob = fr.synthetic_exact_blob(P[0], nt, tf=0.9, seed=3)
    f = fly_batch(P, blob[:, None], nt, substeps=16)
    zs = fr.blob_parts(blob, nt)[0]
    miss = np.abs(f.traj[0, [0, 1, 2, 3, 6, 7, 9], -1] - zs[-1]).max()
    print("exact blob:", np.abs(f.local_error).max(), miss, f.summary[0])
    assert f.summary[0, 9] == 16
    assert np.abs(f.local_error).max() <= 1e-9 and miss <= 1e-9
    assert f.summary[0, 0] <= 1e-9 * P[0, 9] and f.summary[0, 6] <= 1e-9 * P[0, 9]


@pytest.mark.parametrize("scheme,form", [(0, 0), (1, 0), (2, 0), (0, 1)])
def test_the_two_kernels_agree(scheme, form):
    """Both kernels start step 1 from the zero state: eta_1 = flown node 1 - z_1.  Rows 4 / 5 are the apsides ascent_coast_batch
    gives for the same last node."""
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch
    P, nt = _points(5), 100
    r = solve_batch(P, nt, want_blob=True, scheme=scheme, formulation=form, flight=True)
    assert (r.status == 0).all()
    z1 = r.blob[:7].T
    flown1 = r.flight.traj[:, [0, 1, 2, 3, 6, 7, 9], 1]
    assert np.abs(r.flight.local_error[:, 0, :] - (flown1 - z1)).max() <= 1e-15
    c = r.coast(coast_nodes=4)
    assert np.abs(r.flight.nlp_periapsis_alt - c["periapsis_alt"]).max() <= 1e-6
    assert np.abs(r.flight.nlp_apoapsis_alt - c["apoapsis_alt"]).max() <= 1e-6
    cf = r.coast(coast_nodes=4, flown=True)
    assert np.abs(r.flight.flown_periapsis_alt - cf["periapsis_alt"]).max() <= 1e-6
    assert np.abs(r.flight.flown_apoapsis_alt - cf["apoapsis_alt"]).max() <= 1e-6


def test_sweep_of_4096():
    """The 4096-NLP Isp x dry-mass sweep at N = 200: all converged, every summary value finite, every backward-Euler miss in
    [5000, 6500] m and every trapezoid miss in [5, 8] m (a 10 x 10 subgrid solved by the C oracle and flown by the CPU reference
    spans 5429.7 .. 5802.3 m and 6.012 .. 6.403 m, extremes at the corners), the trapezoid's below a hundredth of backward Euler's."""
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch, sweep_isp_drymass
    S = sweep_isp_drymass()
    miss = {}
    for scheme in (0, 1):
        r = solve_batch(S, 200, scheme=scheme, want_traj=False, flight=True)
        assert (r.status == 0).all()
        assert np.isfinite(r.flight.summary).all() and np.isfinite(r.flight.traj).all() and np.isfinite(r.flight.local_error).all()
        miss[scheme] = r.flight.miss_position
        print("scheme", scheme, "miss", miss[scheme].min(), miss[scheme].max(), "m; substeps", np.unique(r.flight.substeps))
    assert miss[0].shape == (4096,) and miss[0].min() >= 5000.0 and miss[0].max() <= 6500.0
    assert miss[1].min() >= 5.0 and miss[1].max() <= 8.0
    assert (miss[1] < miss[0] / 100.0).all()


def test_pointer_kinds_and_substeps():
    """Host and device pointers give the same bits; solve_batch_torch(flight=True) on torch's stream equals the host-pointer call
    on its blob; explicit substeps = 5 equals the automatic choice at N = 200."""
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch_torch, fly_batch, solve_batch
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    nt, P = 200, _points(5)
    B, K = P.shape[0], nt - 1
    r = solve_batch(P, nt, want_blob=True)
    host = fly_batch(P, r.blob, nt)
    L, lib = _lib().load(), _lib()
    pt = torch.from_numpy(P).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(r.blob)).cuda()
    tt = torch.empty((10, nt, B), dtype=torch.float64, device="cuda")
    lt = torch.empty((K, 7, B), dtype=torch.float64, device="cuda")
    st = torch.empty((10, B), dtype=torch.float64, device="cuda")
    o = _opts(nt, 0, 1.0, 0, 0.0)
    stream = torch.cuda.current_stream().cuda_stream
    lib.check(L.ascent_fly_batch(pt.data_ptr(), B, C.byref(o), bt.data_ptr(), 0, tt.data_ptr(), lt.data_ptr(), st.data_ptr(), 0,
                                 C.c_void_p(stream), 1))
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy().T, host.summary)
    assert np.array_equal(tt.cpu().numpy().transpose(2, 0, 1), host.traj)
    assert np.array_equal(lt.cpu().numpy().transpose(2, 0, 1), host.local_error)
    # outputs that are not asked for change nothing in the others
    only = fly_batch(P, r.blob, nt, want_traj=False, want_local=False)
    assert only.traj is None and only.local_error is None and np.array_equal(only.summary, host.summary)
    out = solve_batch_torch(pt, nt, flight=True, sync=True, want_blob=True)
    again = fly_batch(P, out["blob"].cpu().numpy(), nt)
    assert (out["status"] == 0).all()
    assert np.array_equal(out["flight_summary"].cpu().numpy(), again.summary)
    assert np.array_equal(out["flight_traj"].cpu().numpy(), again.traj)
    assert np.array_equal(out["flight_local"].cpu().numpy(), again.local_error)
    five = fly_batch(P[:1], r.blob[:, :1], nt, substeps=5)
    auto = fly_batch(P[:1], r.blob[:, :1], nt)
    assert five.summary[0, 9] == 5 and np.array_equal(five.summary, auto.summary) and np.array_equal(five.traj, auto.traj)
    assert np.array_equal(five.local_error, auto.local_error)
    # a batch of one and the same problem inside a batch of five: the maxima do not depend on how the steps are split
    assert np.array_equal(auto.summary[0], host.summary[0]) and np.array_equal(auto.traj[0], host.traj[0])


def test_unconverged_rows_are_nan_and_the_call_returns():
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch
    r = solve_batch(_points(3), 50, max_iter=2, coarse_nodes=-1, flight=True)
    assert (r.status != 0).all()
    assert np.isnan(r.flight.summary).all() and np.isnan(r.flight.traj).all() and np.isnan(r.flight.local_error).all()
    with pytest.raises(ValueError):
        solve_batch(_points(1), 50).coast(flown=True)


def test_argument_errors_return_e_arg():
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    L = _lib().load()
    P = _points(2)
    nt, K = 50, 49
    blob = np.zeros((21 * K + 10, 2))
    blob[21 * K] = 0.9
    t, l, s = np.zeros((10 * nt, 2)), np.zeros((7 * K, 2)), np.zeros((10, 2))
    pp, bp, tp, lp, sp = (a.ctypes.data_as(C.c_void_p) for a in (P, blob, t, l, s))
    ok = _opts(nt, 0, 1.0, 0, 0.0)
    assert L.ascent_fly_batch(pp, 2, C.byref(ok), bp, 0, tp, lp, sp, 0, None, 0) == 0
    assert L.ascent_fly_batch(pp, 2, C.byref(ok), bp, 4096, None, None, sp, 0, None, 0) == 0
    assert s[9, 0] == 4096
    assert L.ascent_fly_batch(pp, 2, C.byref(ok), bp, -1, tp, lp, sp, 0, None, 0) == -1
    assert L.ascent_fly_batch(pp, 2, C.byref(ok), bp, 4097, tp, lp, sp, 0, None, 0) == -1
    assert L.ascent_fly_batch(pp, 2, C.byref(ok), bp, 0, tp, lp, None, 0, None, 0) == -1
    assert L.ascent_fly_batch(pp, 2, C.byref(ok), None, 0, tp, lp, sp, 0, None, 0) == -1
    assert L.ascent_fly_batch(None, 2, C.byref(ok), bp, 0, tp, lp, sp, 0, None, 0) == -1
    assert L.ascent_fly_batch(pp, 2, None, bp, 0, tp, lp, sp, 0, None, 0) == -1
    assert L.ascent_fly_batch(pp, 0, C.byref(ok), bp, 0, tp, lp, sp, 0, None, 0) == -1
    for bad in (_opts(2, 0, 1.0, 0, 0.0), _opts(nt, 0, 1.0, 0, 0.0, scheme=2, formulation=1),
                _opts(nt, 0, 1.0, 0, 0.0, scheme=1, formulation=1), _opts(nt, 0, 1.0, 0, 0.0, terminal=2, formulation=1),
                _opts(nt, 0, 1.0, 0, 0.0, scheme=3)):
        assert L.ascent_fly_batch(pp, 2, C.byref(bad), bp, 0, tp, lp, sp, 0, None, 0) == -1
        assert L.ascent_strerror(-1)
    # a blob that holds nothing sensible: non-finite and huge t_f -- the call terminates, rows are defined
    for tf in (np.nan, np.inf, 1e300, -1.0):
        blob[21 * K] = tf
        assert L.ascent_fly_batch(pp, 2, C.byref(ok), bp, 0, tp, lp, sp, 0, None, 0) == 0
        assert s[9, 0] == (4096 if tf == 1e300 else 1)


@pytest.mark.parametrize("batch,pb", [(20000, 32), (32768, 64)])
def test_large_batches_reduce_like_small_ones(batch, pb):
    """f_local's reduction over the steps has three shapes: several shuffle rounds (fewer than 32 NLPs per workgroup: every batch
    above), one round (32: batches from about 16 400), none, the waves in LDS only (64: from about 32 700, config 4's shard
    size).  Five different solutions repeated through a large batch give, for every copy, the bits that each gives alone."""
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch, fly_batch
    nt, P = 30, _points(5)
    r = solve_batch(P, nt, want_blob=True)
    assert (r.status == 0).all()
    alone = np.vstack([fly_batch(P[j:j + 1], r.blob[:, j:j + 1], nt).summary for j in range(5)])
    idx = np.arange(batch) % 5
    big = fly_batch(P[idx], np.ascontiguousarray(r.blob[:, idx]), nt, want_traj=False)
    assert np.array_equal(big.summary, alone[idx])
    loc = fly_batch(P, r.blob, nt).local_error
    assert np.array_equal(big.local_error[:10], loc[idx[:10]]) and np.array_equal(big.local_error[-5:], loc[idx[-5:]])


def test_flight_blob_and_the_example():
    """BatchResult.flight_blob() carries what the flight reads; examples/apollo11.py --fly goes through it."""
    import importlib.util
    import io
    from contextlib import redirect_stdout
    from lunar_module_ascent_trajectory_optimiser_amd import solve_batch, fly_batch
    P = _points(3)
    for form in (0, 1):
        r = solve_batch(P, 100, want_blob=True, formulation=form)
        assert (r.status == 0).all()
        a, b = fly_batch(P, r.blob, 100, formulation=form), fly_batch(P, r.flight_blob(), 100, formulation=form)
        assert np.array_equal(a.summary, b.summary) and np.array_equal(a.traj, b.traj) and np.array_equal(a.local_error, b.local_error)
    spec = importlib.util.spec_from_file_location("apollo11_example", os.path.join(ROOT, "examples", "apollo11.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    m, _, _ = ex.build()
    out = io.StringIO()
    with redirect_stdout(out):
        m.solve(disp=False)
        f = ex.fly(m, 0)
    direct = solve_batch(m.result.params, m.result.nt, move_penalty=True, flight=True)      # the script's DCOST is applied by default
    assert abs(direct.tf[0] - m.result.tf[0]) <= 1e-12
    assert np.allclose(f.summary, direct.flight.summary, rtol=1e-9, atol=1e-6)
    assert "flown with RK4, 5 substeps per step: the control ends %.4g m" % f.miss_position[0] in out.getvalue()
