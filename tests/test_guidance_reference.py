"""The CPU reference of the closed-loop guidance (tests/guidance_reference.py) checked against the references it is built on
(flight_jacobian_reference, dispersion_reference), against the optimality of its own gains, against its own closed-loop
Jacobian to second order and for what the feedback is worth on the nominal problem; and the argument refusals of the two
entry points (include/ascent.h: ascent_guidance_gains, ascent_disperse_guided_batch).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import dispersion_reference as dr
import flight_jacobian_reference as jr
import flight_reference as fr
import guidance_reference as gr
from reference_cases import blob as _blob, p16 as _p16, prototype_case as _prototype_case


@pytest.mark.parametrize("form", [0, 1])
def test_zero_gains_are_the_open_loop_references(form):
    """All-zero gains: the guided flight is dispersion_reference.disperse's, sample for sample and bit for bit, and the closed-loop
    Jacobian is flight_jacobian_reference.jacobian's.  The latter two differ in how they are computed -- a product of K step
    Jacobians against one complex step through the whole flight -- so they agree to rounding: 1e-11 of the row's largest entry
    (K = 17 products of 7 x 7 matrices whose entries reach 1e3 of the row's result)."""
    nt, K, m = 18, 17, 2
    p16, blob = _p16(), _blob()
    xi = np.random.default_rng(1).standard_normal((24 + K, 5))
    sigma, su = dr.relative_sigma(p16, 1e-3), np.full(K, 1e-3)
    su[5] = 0.0
    ref = dr.disperse(p16, blob, nt, xi, sigma, su, form, m)
    g = gr.disperse_guided(p16, blob, nt, xi, sigma, su, np.zeros((K, 7)), np.zeros(7), 0.5, form, m)
    assert np.array_equal(g["samples"], ref["samples"]) and np.array_equal(g["nominal"], ref["nominal"])
    assert np.array_equal(g["stats"], ref["stats"], equal_nan=True) and np.all(g["effort"][:, :3] == 0.0)
    rec = gr.records(p16, blob, nt, form, m)
    cl = gr.closed_loop_jacobian(rec, np.zeros((K, 7)), np.zeros(7), p16, form)
    J = jr.jacobian(p16, blob, nt, form, m)
    for a, b in ((cl["jac"], J["jac"]), (cl["jac_u"], J["jac_u"])):
        scale = np.abs(b).max(axis=1)
        err = np.abs(a - b).max(axis=1) / np.where(scale > 0, scale, 1.0)          # the mass row does not depend on u
        print("form", form, "closed-loop Jacobian with zero gains against the flight Jacobian, per row", err)
        assert np.all(err <= 1e-11)


@pytest.mark.parametrize("smax", [0.0, 0.5])
def test_gains_minimise_the_cost_of_the_linear_closed_loop(smax):
    """dz_0' P_0 dz_0 is twice the cost of the simulated linear closed loop (to 1e-9: the recursion's own rounding at q = 1e4),
    the rows of saturated controls are exactly zero, and perturbing any gain row by 1 % of its size raises that cost."""
    nt, K = 18, 17
    p16, blob = _p16(), _blob()
    w = np.array([1e4, 2e4, 5e3, 1.0, 2.0, smax])
    rec = gr.records(p16, blob, nt, 0, 2)
    G = gr.gains(rec, p16, w)
    assert G["summary"][0] == 0 and G["summary"][1] == K - 2 and G["summary"][4] == 2
    assert np.all(G["gain_u"][[3, K - 2]] == 0.0) and (np.all(G["gain_t"] == 0.0) if smax == 0 else np.any(G["gain_t"] != 0.0))
    rng = np.random.default_rng(5)
    for _ in range(3):
        dz0 = rng.standard_normal(7) * 1e-3
        cost = gr.linear_cost(rec, p16, w, G["gain_u"], G["gain_t"], dz0)
        assert abs(dz0 @ G["P"][0] @ dz0 - 2.0 * cost) <= 1e-9 * 2.0 * cost
        free = [k for k in range(K) if k not in (3, K - 2)]
        for k in free + ([K] if smax > 0 else []):
            gu, gt = G["gain_u"].copy(), G["gain_t"].copy()
            row = gt if k == K else gu[k]
            row += 0.01 * np.abs(row).max() * rng.standard_normal(7)
            assert gr.linear_cost(rec, p16, w, gu, gt, dz0) > cost, k


def test_a_bad_weight_or_a_lost_pivot_freezes():
    nt = 18
    p16, blob = _p16(), _blob()
    rec = gr.records(p16, blob, nt, 0, 2)
    for w in ([1e6, 1e6, 1e6, 0.0, 1.0, 0.5], [1e6, -1.0, 1e6, 1.0, 1.0, 0.5], [1e6, 1e6, 1e6, 1.0, np.nan, 0.5], [1e6, 1e6, 1e6, 1.0, 1.0, -0.1]):
        G = gr.gains(rec, p16, np.array(w))
        assert G["summary"][0] == 2 and np.isnan(G["gain_u"]).all() and np.isnan(G["gain_t"]).all() and G["summary"][1] == 15


@pytest.mark.parametrize("form", [0, 1])
def test_one_guided_sample_agrees_with_the_closed_loop_jacobian_to_second_order(form):
    """remainder(sigma) = guided sample - nominal - J_cl (sigma o xi): halving sigma with the same xi divides it by 4, within
    [3, 5], on every row whose remainder is above 1e-9 of the row's scale at both sigmas -- as
    test_dispersion_reference.test_one_sample_agrees_with_the_jacobian_to_second_order does it, at its sigmas 1e-4 and 5e-5, where
    no command and no stretch is clipped (asserted)."""
    nt, K, m = 18, 17, 2
    p16 = _p16()
    blob = fr.synthetic_exact_blob(p16, nt, tf=0.9, seed=4)
    xi = np.random.default_rng(2).standard_normal((24 + K, 1))
    rec = gr.records(p16, blob, nt, form, m)
    G = gr.gains(rec, p16, np.array([1e4, 1e4, 1e4, 1.0, 1.0, 0.5]))
    J = gr.closed_loop_jacobian(rec, G["gain_u"], G["gain_t"], p16, form)
    rem = []
    for rel in (1e-4, 5e-5):
        sigma, su = dr.relative_sigma(p16, rel), np.full(K, rel)
        d = gr.disperse_guided(p16, blob, nt, xi, sigma, su, G["gain_u"], G["gain_t"], 0.5, form, m)
        assert d["stats"][0] == 1 and d["effort"][0, 0] == 0 and 0 < abs(d["effort"][0, 2]) < 0.5 and d["effort"][0, 1] > 0
        lin = J["jac"] @ (sigma * xi[:24, 0]) + J["jac_u"] @ (su * xi[24:, 0])
        rem.append(d["samples"][0] - d["nominal"] - lin)
    scale = np.maximum(np.abs(d["nominal"]), 1.0)
    big = (np.abs(rem[0]) > 1e-9 * scale) & (np.abs(rem[1]) > 1e-9 * scale)
    print("form", form, "remainders", rem[0], rem[1], "rows checked", np.flatnonzero(big))
    assert big[[0, 1, 2, 3, 7, 8]].all()
    ratio = rem[0][big] / rem[1][big]
    print("ratios", ratio)
    assert np.all((ratio >= 3.0) & (ratio <= 5.0))


def test_double_precision_loses_digits_as_the_weights_grow():
    """The gains in float64 against the same computation in longdouble, relative to each row's largest entry, printed for
    q = 1e6, 1e9, 1e12 (a prototype of the recursion alone saw 1e-12, 5e-8, 3e-5).  Only the order is asserted: the loss grows
    with q, and at 1e6 it is below 1e-9."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy's longdouble is float64 on this platform")
    p16, _, _, rec, recl = _prototype_case()
    assert rec["m"] == 18
    gaps = []
    for q in (1e6, 1e9, 1e12):
        w = np.array([q, q, q, 1.0, 1.0, 0.5])
        a, b = gr.gains(rec, p16, w), gr.gains(recl, p16, w, np.longdouble)
        gaps.append(max(gr.rel_gap(a["gain_u"], b["gain_u"]), gr.rel_gap(a["gain_t"], b["gain_t"])))
        print("q", q, "float64 against longdouble gains, relative to the row's largest entry:", gaps[-1])
    assert gaps[0] < gaps[1] < gaps[2] and gaps[0] <= 1e-9


def test_what_the_feedback_is_worth_on_the_nominal_problem():
    """128 samples of default_rng(0), 50 N of thrust sigma, 1e-3 per control step, q = 1e12, r_u = r_t = 1, stretch_max = 0.5:
    the guided apoapsis sigma is at least 100 times below the open-loop one and the periapsis sigma at least 4 times (a prototype
    saw 2000-fold and 9-fold); steering alone (stretch_max = 0) at q = 1e10 is worse than open loop -- it diverges against the
    actuator clip -- which is why the cutoff channel exists."""
    p16, blob, nt, rec, _ = _prototype_case()
    K = nt - 1
    xi = np.random.default_rng(0).standard_normal((24 + K, 128))
    sigma, su = np.zeros(24), np.full(K, 1e-3)
    sigma[7 + 3] = 50.0
    op = dr.disperse(p16, blob, nt, xi, sigma, su)
    G = gr.gains(rec, p16, np.array([1e12, 1e12, 1e12, 1.0, 1.0, 0.5]))
    cl = gr.disperse_guided(p16, blob, nt, xi, sigma, su, G["gain_u"], G["gain_t"], 0.5)
    G0 = gr.gains(rec, p16, np.array([1e10, 1e10, 1e10, 1.0, 1.0, 0.0]))
    st = gr.disperse_guided(p16, blob, nt, xi, sigma, su, G0["gain_u"], G0["gain_t"], 0.0)
    assert op["stats"][0] == 128 and cl["stats"][0] == 128 and G["summary"][0] == 0 and G0["summary"][0] == 0
    sd = lambda d: np.sqrt(d["stats"][19:64][[np.flatnonzero((dr.IU[0] == i) & (dr.IU[1] == i))[0] for i in (7, 8)]])
    so, sc, ss = sd(op), sd(cl), sd(st)
    print("1-sigma of the flown periapsis / apoapsis altitude (m): open loop", so, "closed loop", sc, "steering only, q = 1e10", ss,
          "valid", st["stats"][0])
    print("closed loop effort: clipped steps (mean)", cl["effort"][:, 0].mean(), "max |K.dz|", cl["effort"][:, 1].max(),
          "largest |stretch|", np.abs(cl["effort"][:, 2]).max())
    assert sc[1] * 100.0 <= so[1] and sc[0] * 4.0 <= so[0]
    assert st["stats"][0] < 128 or ss[0] > so[0]


@pytest.fixture(scope="module")
def lib():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib, build
    build.build()
    return _lib.load()


def _guided_calls():
    def gains(L, a, o):
        return L.ascent_guidance_gains(a["p"], a["batch"], o, a["blob"], a["substeps"], a["weights"], a["out"], a["out2"], a["out3"],
                                       a["jac"], a["jac_u"], 0, None, 0)

    def guided(L, a, o):
        return L.ascent_disperse_guided_batch(a["p"], a["batch"], o, a["blob"], a["substeps"], a["samples"], a["xi"], a["sigma"], a["opt"],
                                              a["gain_u"], a["opt"], a["opt"], a["out"], a["opt"], 0, None, 0)
    return dict(ascent_guidance_gains=gains, ascent_disperse_guided_batch=guided)


@pytest.mark.parametrize("name", sorted(_guided_calls()))
def test_guidance_entry_points_refuse_bad_arguments_before_the_device(lib, name):
    """Every argument error of the two entry points is ASCENT_E_ARG with its own message, on a machine with or without a GPU:
    refusals come before the device is looked at.  A refused call touches none of its arrays."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    assert name in _lib.SYMBOLS
    call = _guided_calls()[name]
    P = np.vstack([A.AscentParams().as_row()] * 2)
    P0 = P.copy()
    P0[1, 15] = 0.0
    arrays = {k: np.full(8, 7.25) for k in ("blob", "out", "out2", "out3", "opt", "weights", "jac", "jac_u", "xi", "sigma", "gain_u")}
    good = dict({k: v.ctypes.data_as(C.c_void_p) for k, v in arrays.items()}, p=P.ctypes.data_as(C.c_void_p), batch=2, substeps=0,
                samples=4)
    gains = name == "ascent_guidance_gains"

    def opts(**kw):
        return C.byref(_lib.AscentOptsC(**dict(dict(n_nodes=50, scheme=0, max_iter=0, warm_start=0, tol=1.0, mu_init=0.0), **kw)))

    def refused(what, o=None, **changes):
        rc = call(lib, dict(good, **changes), opts() if o is None else o)
        msg = lib.ascent_strerror(rc)
        assert rc == -1 and what in msg, (name, changes, rc, msg)

    refused(b"null", p=None)
    refused(b"batch <= 0", batch=0)
    refused(b"null", blob=None)
    refused(b"null", out=None)
    refused(b"null", o=C.POINTER(_lib.AscentOptsC)())
    refused(b"scheme", o=opts(scheme=7))
    refused(b"dcost", o=opts(move_penalty=1), p=P0.ctypes.data_as(C.c_void_p))
    refused(b"substeps", substeps=-1)
    refused(b"substeps", substeps=4097)
    if gains:
        refused(b"null", weights=None)
        refused(b"null", out2=None)
        refused(b"null", out3=None)
        refused(b"jac_u_cl_out needs jac_cl_out", jac=None)
        refused(b"terminal 2", o=opts(terminal=2))
    else:
        refused(b"null", xi=None)
        refused(b"null", sigma=None)
        refused(b"null", gain_u=None)
        refused(b"samples", samples=0)
        refused(b"samples", samples=65537)
    for k, v in arrays.items():
        assert (v == 7.25).all(), k


def test_python_front_end_checks_shapes():
    import lunar_module_ascent_trajectory_optimiser_amd as A
    nt, K = 18, 17
    P = np.vstack([A.AscentParams().as_row()] * 2)
    assert "guidance_gains" in A.__all__ and "GuidanceResult" in A.__all__ and A.GUIDE_ROWS[0] == "status"
    with pytest.raises(ValueError):
        A.guidance_gains(P, np.zeros((21 * K + 9, 2)), nt)
    with pytest.raises(ValueError):
        A.guidance_gains(P, np.zeros((21 * K + 10, 2)), nt, cond_weights=(1.0, 1.0))
    bad = A.GuidanceResult(np.zeros((2, K - 1, 7)), np.zeros((2, 7)), np.zeros((2, 5)), np.zeros(2), None)
    with pytest.raises(ValueError):
        A.disperse_batch(P, np.zeros((21 * K + 10, 2)), nt, guidance=bad)
