"""The two-body kernels on the GPU -- k_coast (ascent_coast_batch), apsides_of (flight summary rows 2..5) and apsides_grad
(rows 7 / 8 of ascent_flight_jacobian) -- against the 50-digit reference tests/coast_reference.py, which
tests/test_coast_reference.py proves first.

Bounds: a device value may differ from the reference by 64 x floor, where floor is what the reference itself moves by when
every float64 input moves by 1 ulp (coast_reference.floor: it grows like 1 / e where the question is ill-posed); a float64
transcription of the reference algorithm stays within 16 x floor on the same cases (test_coast_reference.py).  Position and
velocity errors are Euclidean norms against the norm of the two component floors.  The largest error / floor seen per check is
collected in PARITY["ratios"]; with ASCENT_COAST_PARITY_OUT=<file> it is written there as JSON when the module is done
(profiles/coast_parity.json is such a file).  Every call is tiny: batches of at most 130, at most 64 coast nodes except the one
test of the documented maximum."""
import ctypes as C
import functools

import numpy as np
import pytest

import coast_reference as cr
import flight_reference as fr
from gpu_cases import parity_writer

pytestmark = pytest.mark.gpu

MARGIN = 64.0
NODES = 4                       # nodes 1 .. 4 of every arc: a quarter, a half, three quarters and the apoapsis
CASES = cr.case_matrix()
PARITY = {"ratios": {}, "info": {}}
E_ARG = -1
_write_parity = parity_writer("ASCENT_COAST_PARITY_OUT", PARITY, sort_keys=True)


def _record(check, ratio):
    PARITY["ratios"][check] = max(PARITY["ratios"].get(check, 0.0), float(ratio))


def _lib():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    return _lib


def _batch():
    """(P (130, 16), states (4, 130)): the case matrix, then the first 59 of its orbits turned to another phase: all distinct"""
    P = [c[2] for c in CASES]
    S = [c[3] for c in CASES]
    k = 0
    for e in cr.ECCENTRICITIES:
        for nu in cr.ANOMALIES:
            if len(S) < 130:
                P.append(cr.NOMINAL)
                S.append(cr.orbit_state(cr.NOMINAL, e, nu, phase=1.1 + 0.01 * k))
                k += 1
    return np.array(P), np.ascontiguousarray(np.array(S).T)


@functools.lru_cache(maxsize=None)
def _device():
    """one coast of all 130 states with NODES nodes and one flight of 130 two-step blobs whose last node is that state"""
    from lunar_module_ascent_trajectory_optimiser_amd import coast_batch, fly_batch
    P, S = _batch()
    c = coast_batch(P, S, coast_nodes=NODES)
    blobs = []
    for j in range(S.shape[1]):
        z = np.zeros((2, 7))
        z[0, :4], z[1, :4] = 0.5 * S[:, j], S[:, j]
        blobs.append(fr.make_blob(z, np.array([0.3, -0.2]), 0.05))
    f = fly_batch(P, np.ascontiguousarray(np.array(blobs).T), 3, want_traj=False, want_local=False)
    for a in (P, S, c["traj"], c["tf"], c["periapsis_alt"], c["apoapsis_alt"], f.summary):
        a.setflags(write=False)
    return P, S, c, f.summary


def _propagation_ratio(p, s, arc, tf):
    """largest error / floor over nodes 1 .. of one arc (4, nodes + 1) against propagate at the device's own node times"""
    nodes = arc.shape[1] - 1
    worst = 0.0
    for j in range(1, nodes + 1):
        t = j * tf * p[cr.IT] / nodes
        ref, fl = cr.to_float(cr.propagate(p, s, t)), cr.floor(cr.propagate, p, s, t)
        worst = max(worst, np.hypot(*(arc[:2, j] - ref[:2])) / np.hypot(*fl[:2]), np.hypot(*(arc[2:, j] - ref[2:])) / np.hypot(*fl[2:]))
    return worst


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_case_matrix(i):
    """One state of the matrix: node 0 is the input to 4 ulp; every other node against propagate(); the apsides against
    apsides() and bitwise against rows 4 / 5 of the flight summary; e >= 1e-6: the duration against time_to_apoapsis() and the
    radius of the last node against a (1 + e); below: 0 <= duration <= one period and everything finite."""
    name, e, p, s = CASES[i]
    P, S, c, summary = _device()
    assert np.array_equal(P[i], p) and np.array_equal(S[:, i], s)
    arc, tf = c["traj"][:, :, i], c["tf"][i]
    assert np.isfinite(arc).all() and np.isfinite(tf)
    failed = []                                              # every check is made and reported before the test fails
    ulps = (np.abs(arc[:, 0] - s) / np.spacing(np.abs(s))).max()
    print(name, "node 0 off by (ulp)", ulps, "(m)", np.hypot(*(arc[:2, 0] - s[:2])) * p[cr.IS])
    PARITY["info"]["node0_largest_ulp"] = max(PARITY["info"].get("node0_largest_ulp", 0.0), float(ulps))
    if not ulps <= 4.0:
        failed.append(f"node 0 is {ulps} ulp from the input")
    ratio = _propagation_ratio(p, s, arc, tf)
    print(name, "propagation error / floor", ratio)
    _record("propagation", ratio)
    if not ratio <= MARGIN:
        failed.append(f"propagation {ratio} floors")
    aps = np.array([c["periapsis_alt"][i], c["apoapsis_alt"][i]])
    ref_aps, fl_aps = cr.to_float(cr.apsides(p, s)), cr.floor(cr.apsides, p, s)
    ra = (np.abs(aps - ref_aps) / fl_aps).max()
    print(name, "apsides error / floor", ra, "floor (m)", fl_aps)
    _record("apsides", ra)
    if not ra <= MARGIN:
        failed.append(f"apsides {ra} floors")
    if not np.array_equal(aps, summary[i, 4:6]):
        failed.append(f"apsides differ from the flight summary by {aps - summary[i, 4:6]} m")
    T = tf * p[cr.IT]
    if e in cr.WELL_POSED:
        ref_T, fl_T = float(cr.time_to_apoapsis(p, s)), cr.floor(cr.time_to_apoapsis, p, s)[0]
        rt = abs(T - ref_T) / fl_T
        el = cr.elements(p, s)
        rad = np.hypot(arc[0, -1] * p[cr.IS], arc[1, -1] * p[cr.IS] + p[cr.IR0])
        rr = abs(rad - float(el["a"] * (1 + el["e"]))) / fl_aps[1]
        print(name, "duration error / floor", rt, "floor (s)", fl_T, "end radius error / floor", rr)
        _record("duration", rt)
        _record("end_radius", rr)
        if not (rt <= MARGIN and rr <= MARGIN):
            failed.append(f"duration {rt} floors, end radius {rr} floors")
    elif not 0.0 <= T <= float(cr.period(p, s)):
        failed.append(f"duration {T} s outside [0, one period]")
    assert not failed, failed


def test_energy_not_negative_in_the_middle_of_a_batch():
    """a state above the escape speed between bound ones: ASCENT_OK, its trajectory and duration NaN, its periapsis the
    apsides_of value and its apoapsis +inf (also in the flight summary); the neighbours bitwise what they are alone"""
    from lunar_module_ascent_trajectory_optimiser_amd import coast_batch, fly_batch
    P, S, c, _ = _device()
    idx = [19, 31, 0, 44, 7]
    Pb, Sb = P[idx].copy(), np.ascontiguousarray(S[:, idx])
    Pb[2] = cr.NOMINAL
    Sb[:, 2] = cr.orbit_state(cr.NOMINAL, 0.03, 0.7) * np.array([1.0, 1.0, 1.5, 1.5])
    assert cr.elements(Pb[2], Sb[:, 2])["energy"] > 0
    got = coast_batch(Pb, Sb, coast_nodes=NODES)            # (raises unless the call returned ASCENT_OK)
    assert np.isnan(got["traj"][:, :, 2]).all() and np.isnan(got["tf"][2])
    peri, apo = cr.apsides(Pb[2], Sb[:, 2])
    fl = cr.floor(cr.apsides, Pb[2], Sb[:, 2])[0]
    ratio = abs(got["periapsis_alt"][2] - float(peri)) / fl
    print("hyperbolic periapsis", got["periapsis_alt"][2], "error / floor", ratio)
    _record("apsides", ratio)
    assert ratio <= MARGIN and apo == cr.MP.inf and got["apoapsis_alt"][2] == np.inf
    z = np.zeros((2, 7))
    z[1, :4] = Sb[:, 2]
    f = fly_batch(Pb[2:3], fr.make_blob(z, np.zeros(2), 0.05)[:, None], 3, want_traj=False, want_local=False)
    assert f.summary[0, 4] == got["periapsis_alt"][2] and f.summary[0, 5] == np.inf
    for k in (0, 1, 3, 4):
        alone = coast_batch(Pb[k:k + 1], Sb[:, k:k + 1], coast_nodes=NODES)
        for key in ("traj", "tf", "periapsis_alt", "apoapsis_alt"):
            assert np.array_equal(alone[key][..., 0], got[key][..., k]), (k, key)
            assert np.array_equal(alone[key][..., 0], c[key][..., idx[k]]), (k, key)


@pytest.mark.parametrize("batch", [1, 63, 65])
def test_batch_sizes(batch):
    """The first `batch` of the 130 distinct states as a batch of their own -- one problem, a partly filled wavefront, one
    wavefront and a lane -- give the bits they have in the batch of 130 (two wavefronts and two lanes), whose first 71 problems
    test_case_matrix checks against the reference: the batch stride and the tail of the last wavefront."""
    from lunar_module_ascent_trajectory_optimiser_amd import coast_batch
    P, S, c, _ = _device()
    got = coast_batch(P[:batch], np.ascontiguousarray(S[:, :batch]), coast_nodes=NODES)
    for key in ("traj", "tf", "periapsis_alt", "apoapsis_alt"):
        assert np.array_equal(got[key], c[key][..., :batch]), key
    assert np.isfinite(c["traj"]).all() and c["traj"].shape == (4, NODES + 1, 130)


@pytest.mark.parametrize("nodes", [1, 64, 65535])
def test_coast_nodes(nodes):
    """one node, 64, and the documented maximum (65536 lanes in the node dimension, 2 MB of output) at batch 1: node 0 is the
    input, the last node is the reference's state at the device's duration, the duration does not depend on the node count, and
    node j of the short arcs is the matching node of the longest to 64 floors"""
    from lunar_module_ascent_trajectory_optimiser_amd import coast_batch
    P, S, c, _ = _device()
    i = 13                                                   # e = 0.3 at true anomaly 0.7
    p, s = P[i], S[:, i]
    got = coast_batch(P[i:i + 1], np.ascontiguousarray(S[:, i:i + 1]), coast_nodes=nodes)
    arc, tf = got["traj"][:, :, 0], got["tf"][0]
    assert arc.shape == (4, nodes + 1) and np.isfinite(arc).all()
    assert tf == c["tf"][i] and np.array_equal(arc[:, 0], s)
    ratio = _propagation_ratio(p, s, arc[:, [0, nodes]], tf)
    print("coast_nodes", nodes, "last node error / floor", ratio)
    _record("propagation", ratio)
    assert ratio <= MARGIN
    if nodes % NODES == 0:                                   # the same instants: nodes / 4, / 2, 3/4
        step = nodes // NODES
        fl = [cr.floor(cr.propagate, p, s, j * tf * p[cr.IT] / NODES) for j in range(NODES + 1)]
        for j in range(1, NODES + 1):
            assert np.hypot(*(arc[:2, j * step] - c["traj"][:2, j, i])) <= MARGIN * np.hypot(*fl[j][:2])
    if nodes > 1:                                            # a uniform sampling in time moves on along the orbit at every node
        X, Y = arc[0] * p[cr.IS], arc[1] * p[cr.IS] + p[cr.IR0]
        ang = np.unwrap(np.arctan2(-X, Y))
        assert (np.diff(ang) > 0).all()


def test_refused_arguments():
    """coast_nodes 0 and 65536, a null pointer and batch 0 return ASCENT_E_ARG"""
    L = _lib().load()
    P, S, _, _ = _device()
    p, s = np.array(P[:1]), np.ascontiguousarray(S[:, :1])
    traj, tf, aps = np.empty((4, 5, 1)), np.empty(1), np.empty((2, 1))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [ptr(p), 1, ptr(s), 4, ptr(traj), ptr(tf), ptr(aps), 0, None, 0]
    assert L.ascent_coast_batch(*good) == 0
    for pos, bad in ((3, 0), (3, 65536), (3, -1), (1, 0), (0, None), (2, None), (4, None), (5, None), (6, None)):
        args = list(good)
        args[pos] = bad
        assert L.ascent_coast_batch(*args) == E_ARG, (pos, bad)


def test_device_pointers_and_streams():
    """the same call with device pointers from torch tensors, on a stream of its own and on the NULL stream: bit-identical
    to the host-pointer result"""
    import torch
    L = _lib().load()
    P, S, c, _ = _device()
    B = P.shape[0]
    pt, st = torch.from_numpy(np.array(P)).cuda(), torch.from_numpy(np.array(S)).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stream in (side.cuda_stream, None):
        traj = torch.full((4, NODES + 1, B), -1.0, dtype=torch.float64, device="cuda")
        tf = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
        aps = torch.full((2, B), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = L.ascent_coast_batch(pt.data_ptr(), B, st.data_ptr(), NODES, traj.data_ptr(), tf.data_ptr(), aps.data_ptr(), 0,
                                  None if stream is None else C.c_void_p(stream), 1)
        assert rc == 0
        if stream is not None:
            side.synchronize()
        assert np.array_equal(traj.cpu().numpy(), c["traj"]) and np.array_equal(tf.cpu().numpy(), c["tf"])
        assert np.array_equal(aps.cpu().numpy()[0], c["periapsis_alt"]) and np.array_equal(aps.cpu().numpy()[1], c["apoapsis_alt"])


V1 = dict(r_peri=53108.4, r_apo=53108.4, mass_scalar=2576.0)        # the v1 script's constants: a circular target


@pytest.mark.parametrize("name", ["v1_formulation0", "v1_formulation1", "nominal_circular"])
def test_the_projects_circular_solutions(name):
    """The project's own near-circular burnout states, N = 50 at tol 1e-10: the coast from the NLP's last node (at an apsis:
    r.v = 0 is a constraint), from the last node the untrimmed control reaches when flown (away from it) and from the flown last
    node after the trim: node 0 is the input, every node against propagate().  Prints the eccentricity of each start."""
    from lunar_module_ascent_trajectory_optimiser_amd import AscentParams, solve_batch, coast_batch
    par, form = {"v1_formulation0": (AscentParams(**V1), 0), "v1_formulation1": (AscentParams(**V1), 1),
                 "nominal_circular": (AscentParams(r_apo=17703.0), 0)}[name]
    nt = 50
    r = solve_batch(par, nt, tol=1e-10, max_iter=500, formulation=form, want_blob=True, flight=True, trim=True)
    assert r.status[0] == 0 and r.trim.status[0] == 0
    p = r.params[0]
    trimmed = np.ascontiguousarray(r.trim.blob[7 * (nt - 2):7 * (nt - 2) + 4])           # the trimmed blob's last node, (4, 1)
    arcs = {"nlp": r.coast(coast_nodes=NODES), "flown": r.coast(coast_nodes=NODES, flown=True),
            "trimmed": coast_batch(r.params, trimmed, coast_nodes=NODES)}
    starts = {"nlp": r.traj[:4, -1, 0], "flown": r.flight.traj[0, :4, -1], "trimmed": trimmed[:, 0]}
    for kind, c in arcs.items():
        s = np.array(starts[kind])
        e = float(cr.elements(p, s)["e"])
        arc = c["traj"][:, :, 0]
        assert np.isfinite(arc).all() and 0.0 <= c["tf"][0] * p[cr.IT] <= float(cr.period(p, s))
        ulps = (np.abs(arc[:, 0] - s) / np.spacing(np.abs(s))).max()
        ratio = _propagation_ratio(p, s, arc, c["tf"][0])
        ref_aps, fl_aps = cr.to_float(cr.apsides(p, s)), cr.floor(cr.apsides, p, s)
        ra = (np.abs(np.array([c["periapsis_alt"][0], c["apoapsis_alt"][0]]) - ref_aps) / fl_aps).max()
        print(name, kind, "burnout e", e, "node 0 off by (ulp)", ulps, "propagation error / floor", ratio, "apsides error / floor", ra)
        PARITY["info"][f"burnout_e_{name}_{kind}"] = e
        _record("propagation", ratio)
        _record("apsides", ra)
        assert ulps <= 4.0 and ratio <= MARGIN and ra <= MARGIN


def _jac_rows(J, j=0):
    """rows 0..8 of problem j over all columns: z_0 (7), the 16 fields, t_f, u_1..u_K"""
    return np.concatenate([J.dz0[j], J.dparams[j], J.dtf[j][:, None], J.dcontrols[j]], axis=1)


@functools.lru_cache(maxsize=None)
def _trimmed(delta):
    """(P, trimmed blob, flown end state, its e): nt = 34, the (r_peri, r_peri + delta) ellipse, solved to 1e-10 and trimmed"""
    from lunar_module_ascent_trajectory_optimiser_amd import AscentParams, solve_batch, trim_batch, fly_batch
    nt = 34
    P = AscentParams(r_apo=17703.0 + delta).as_row()[None]
    r = solve_batch(P, nt, tol=1e-10, max_iter=500, terminal=1, want_blob=True)
    assert r.status[0] == 0
    t = trim_batch(P, r.blob, nt, terminal=1, tol=1e-12)
    assert t.status[0] == 0, t.summary
    f = fly_batch(P, t.blob, nt, terminal=1, want_local=False)
    end = np.array(f.traj[0, :4, -1])
    return P, t.blob, end, float(cr.elements(P[0], end)["e"]), f.summary[0]


@pytest.mark.parametrize("delta", [70912.0, 1000.0, 1.0])
def test_flight_jacobian_apsides_rows(delta):
    """Rows 7 / 8 of ascent_flight_jacobian at a trimmed blob whose flown orbit is the (r_peri, r_peri + delta) ellipse -- every
    column: z_0, the 16 fields with their four direct terms, t_f, every u_k -- against apsides_gradient() at the device's own
    flown end state contracted with the device's rows 0..3: an error here is apsides_grad's, the RK4 tangent is left to
    test_gpu_trim.py.  Errors relative to the row's largest entry (parameters as elasticities, as test_gpu_trim.py scales);
    bound 64 x the floor of the gradient, contracted the same way, plus 1e-12."""
    from lunar_module_ascent_trajectory_optimiser_amd import flight_jacobian
    nt = 34
    P, blob, end, e, summary = _trimmed(delta)
    p = P[0]
    a = p[cr.IR0] + p[cr.IS] + 0.5 * delta
    print("delta", delta, "flown e", e, "delta / 2a", delta / (2 * a), "flown apsides", summary[2:4])
    assert 0.5 * delta / (2 * a) <= e <= 2.0 * delta / (2 * a)
    J = flight_jacobian(P, blob, nt, terminal=1)
    rows = _jac_rows(J)
    assert np.isfinite(rows).all()
    g = cr.to_float(cr.apsides_gradient(p, end)).reshape(2, 8)
    gf = cr.floor(cr.apsides_gradient, p, end).reshape(2, 8)
    w = np.concatenate([np.ones(7), p, [blob[21 * (nt - 1), 0]], np.ones(nt - 1)])          # elasticities
    worst = 0.0
    for q in range(2):
        want = g[q, :4] @ rows[:4]
        fl = gf[q, :4] @ np.abs(rows[:4])
        for k, field in enumerate(cr.P_READ):                # the direct terms: G, M, R0, r_peri with the scaled state held
            want[7 + field] += g[q, 4 + k]
            fl[7 + field] += gf[q, 4 + k]
        scale = np.abs(want * w).max()
        err, bound = np.abs(rows[7 + q] - want) * w / scale, MARGIN * fl * w / scale + 1e-12
        ratio = (err / (bound / MARGIN)).max()
        print("delta", delta, "row", 7 + q, "largest error / row scale", err.max(), "at a floor of", (fl * w / scale)[np.argmax(err)],
              "error / (floor + 1e-12 / 64)", ratio)
        worst = max(worst, ratio)
        _record("jacobian_apsides_rows", ratio)
        assert (err <= bound).all(), (q, np.argmax(err - bound))
    PARITY["info"][f"jacobian_flown_e_delta{delta:g}"] = e


def test_flight_jacobian_apsides_rows_on_the_circle():
    """the delta = 0 solution (flown e of 1e-9 or so): rows 7 + 8 are the gradient of 2 a - 2 R0, which is smooth at e = 0, to
    1e-10 of the row's largest entry, and every entry of rows 7 and 8 is finite"""
    from lunar_module_ascent_trajectory_optimiser_amd import flight_jacobian
    nt = 34
    P, blob, end, e, summary = _trimmed(0.0)
    p = P[0]
    print("delta 0: flown e", e, "flown apsides", summary[2:4])
    PARITY["info"]["jacobian_flown_e_delta0"] = e
    J = flight_jacobian(P, blob, nt, terminal=1)
    rows = _jac_rows(J)
    assert np.isfinite(rows).all()
    g = cr.to_float(cr.axis_gradient(p, end))
    want = g[:4] @ rows[:4]
    for k, field in enumerate(cr.P_READ):
        want[7 + field] += g[4 + k]
    w = np.concatenate([np.ones(7), p, [blob[21 * (nt - 1), 0]], np.ones(nt - 1)])
    err = np.abs(rows[7] + rows[8] - want) * w / np.abs(want * w).max()
    print("delta 0: rows 7 + 8 against the gradient of 2 a - 2 R0, relative", err.max())
    PARITY["info"]["jacobian_axis_sum_relative_error_delta0"] = float(err.max())
    assert err.max() <= 1e-10
