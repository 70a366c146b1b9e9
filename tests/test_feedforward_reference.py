"""The CPU reference of the guidance feed-forward and the navigation errors (tests/feedforward_reference.py) checked against
guidance_reference, against the optimality of its own augmented value function, against its own closed-loop Jacobian to second
order and for what the feed-forward is worth on the nominal problem; and the argument refusals of the two entry points
(include/ascent.h: ascent_guidance_feedforward, ascent_disperse_navigated_batch) and of the Python front end.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import dispersion_reference as dr
import feedforward_reference as ffr
import flight_reference as fr
import guidance_reference as gr
from reference_cases import blob as _blob, p16 as _p16, prototype_case as _prototype_case

E_FT = np.eye(16)[3]           # the direction of the tests: theta is newtons of thrust


@pytest.mark.parametrize("smax", [0.0, 0.5])
def test_feedback_gains_are_those_of_the_plain_recursion(smax):
    """certainty equivalence: K_k, k_t and summary rows 0..4 do not see the direction, for e_Ft and for a dense random one"""
    p16, blob = _p16(), _blob()
    w = np.array([1e4, 2e4, 5e3, 1.0, 2.0, smax])
    rec = gr.records(p16, blob, 18, 0, 2)
    G0 = gr.gains(rec, p16, w)
    for d in (E_FT, np.random.default_rng(3).standard_normal(16) * np.abs(p16) * 1e-3, np.zeros(16)):
        G = ffr.gains(rec, p16, w, d)
        assert np.array_equal(G["gain_u"], G0["gain_u"]) and np.array_equal(G["gain_t"], G0["gain_t"])
        assert np.array_equal(G["summary"][:5], G0["summary"]) and all(np.array_equal(a, b) for a, b in zip(G["P"], G0["P"]))
        if not d.any():
            assert np.all(G["ff_u"] == 0.0) and G["ff_t"] == 0.0
    bad = E_FT.copy()
    bad[7] = np.nan
    G = ffr.gains(rec, p16, w, bad)
    assert G["summary"][0] == 2 and np.isnan(G["ff_u"]).all() and np.isnan(G["gain_u"]).all()


@pytest.mark.parametrize("smax", [0.0, 0.5])
def test_feedforward_minimises_the_cost_of_the_linear_closed_loop(smax):
    """[dz_0; theta]' [[P_0, p_0], [p_0', pi0_0]] [dz_0; theta] is twice the cost of the simulated linear closed loop with theta
    known (to 1e-9, as the plain recursion's test), f of a saturated step is exactly zero, and perturbing any f_k, or f_t, by 1 %
    of the largest |f_k| (of |f_t|) raises that cost."""
    nt, K = 18, 17
    p16, blob = _p16(), _blob()
    w = np.array([1e4, 2e4, 5e3, 1.0, 2.0, smax])
    rec = gr.records(p16, blob, nt, 0, 2)
    G = ffr.gains(rec, p16, w, E_FT)
    assert G["summary"][0] == 0 and G["summary"][1] == K - 2 and G["summary"][5] == np.abs(G["ff_u"]).max() > 0
    assert np.all(G["ff_u"][[3, K - 2]] == 0.0) and (G["ff_t"] == 0.0 if smax == 0 else G["ff_t"] != 0.0)
    free = [k for k in range(K) if k not in (3, K - 2)]
    assert np.all(G["ff_u"][free] != 0.0)
    rng = np.random.default_rng(6)
    for _ in range(3):
        dz0, theta = rng.standard_normal(7) * 1e-3, rng.standard_normal() * 50.0
        cost = ffr.linear_cost(rec, p16, w, G, E_FT, dz0, theta)
        x = np.concatenate([dz0, [theta]])
        V = np.block([[G["P"][0], G["p"][0][:, None]], [G["p"][0][None, :], np.array([[G["pi0"][0]]])]])
        print("smax", smax, "x' V x", x @ V @ x, "2 cost", 2.0 * cost)
        assert abs(x @ V @ x - 2.0 * cost) <= 1e-9 * 2.0 * cost
        for k in free + ([K] if smax > 0 else []):
            fu, ft = G["ff_u"].copy(), G["ff_t"]
            sign = 1.0 if rng.random() < 0.5 else -1.0
            if k == K:
                ft = ft + sign * 0.01 * abs(ft)
            else:
                fu[k] += sign * 0.01 * np.abs(fu).max()
            assert ffr.linear_cost(rec, p16, w, G, E_FT, dz0, theta, ff_u=fu, ff_t=ft) > cost, k


@pytest.mark.parametrize("form", [0, 1])
def test_one_navigated_sample_agrees_with_the_closed_loop_jacobian_to_second_order(form):
    """remainder(sigma) = navigated sample - nominal - [J_cl | J_u | J_nav] (sigma o xi) with thrust, navigation-bias and knowledge
    errors all non-zero: halving every sigma with the same draws divides it by 4, within [3, 5], on rows 0..3, 7 and 8 -- the rows
    and the sigmas (1e-4, 5e-5 relative) of guidance_reference's own second-order test; no command and no stretch is clipped
    (asserted)."""
    nt, K, m = 18, 17, 2
    p16 = _p16()
    blob = fr.synthetic_exact_blob(p16, nt, tf=0.9, seed=4)
    xi = np.random.default_rng(2).standard_normal((24 + K, 1))
    xn = np.random.default_rng(12).standard_normal((8, 1))
    rec = gr.records(p16, blob, nt, form, m)
    G = ffr.gains(rec, p16, np.array([1e4, 1e4, 1e4, 1.0, 1.0, 0.5]), E_FT)
    J = ffr.closed_loop_jacobian(rec, G, E_FT, p16, form)
    assert G["summary"][0] == 0 and G["ff_t"] != 0.0
    rem = []
    for rel in (1e-4, 5e-5):
        sigma, su = dr.relative_sigma(p16, rel), np.full(K, rel)
        sn = np.concatenate([np.full(7, rel), [rel * p16[3]]])
        assert sigma[7 + 3] != 0.0
        d = ffr.disperse_navigated(p16, blob, nt, xi, sigma, su, G["gain_u"], G["gain_t"], 0.5, G["ff_u"], G["ff_t"], E_FT, xn, sn, form, m)
        assert d["stats"][0] == 1 and d["effort"][0, 0] == 0 and 0 < abs(d["effort"][0, 2]) < 0.5 and d["effort"][0, 1] > 0
        lin = J["jac"] @ (sigma * xi[:24, 0]) + J["jac_u"] @ (su * xi[24:, 0]) + J["jac_nav"] @ (sn * xn[:, 0])
        rem.append(d["samples"][0] - d["nominal"] - lin)
    scale = np.maximum(np.abs(d["nominal"]), 1.0)
    big = (np.abs(rem[0]) > 1e-9 * scale) & (np.abs(rem[1]) > 1e-9 * scale)
    print("form", form, "remainders", rem[0], rem[1], "rows checked", np.flatnonzero(big))
    assert big[[0, 1, 2, 3, 7, 8]].all()
    ratio = rem[0][big] / rem[1][big]
    print("ratios", ratio)
    assert np.all((ratio >= 3.0) & (ratio <= 5.0))


def test_jacobian_without_feedforward_is_the_plain_closed_loop_jacobian():
    """d = 0: the forward product of the closed-loop maps and guidance_reference's backward one agree to rounding (1e-11 of each
    row's largest entry, the bound of the zero-gain comparison there), and the theta-hat column is zero"""
    p16, blob = _p16(), _blob()
    rec = gr.records(p16, blob, 18, 0, 2)
    G = ffr.gains(rec, p16, np.array([1e4, 2e4, 5e3, 1.0, 2.0, 0.5]), np.zeros(16))
    J = ffr.closed_loop_jacobian(rec, G, E_FT, p16)
    J0 = gr.closed_loop_jacobian(rec, G["gain_u"], G["gain_t"], p16)
    keep = [c for c in range(24) if c not in (7 + 10, 7 + 13, 7 + 14, 7 + 15, 7 + 12)]          # columns the kernels define as zero
    assert gr.rel_gap(J["jac"][:, keep], J0["jac"][:, keep]) <= 1e-11 and gr.rel_gap(J["jac_u"], J0["jac_u"]) <= 1e-11
    assert np.all(J["jac_nav"][:, 7] == 0.0) and np.any(J["jac_nav"][:, :7] != 0.0)


def test_what_the_feedforward_is_worth_on_the_nominal_problem():
    """The case of test_what_the_feedback_is_worth_on_the_nominal_problem (128 samples of default_rng(0), 50 N of thrust sigma,
    1e-3 per control step, q = 1e12, r_u = r_t = 1, stretch_max = 0.5): the periapsis 1-sigma with the thrust known is at least 10
    times below feedback only (a prototype saw 2588 m -> 100.6 m, 25.7-fold), with the thrust known to 10 N (1-sigma; draws of
    default_rng(1)) it lies strictly between the two (prototype: 444.5 m), and no command is clipped in either."""
    p16, blob, nt, rec, _ = _prototype_case()
    K = nt - 1
    xi = np.random.default_rng(0).standard_normal((24 + K, 128))
    xn = np.random.default_rng(1).standard_normal((8, 128))
    sigma, su = np.zeros(24), np.full(K, 1e-3)
    sigma[7 + 3] = 50.0
    G = ffr.gains(rec, p16, np.array([1e12, 1e12, 1e12, 1.0, 1.0, 0.5]), E_FT)
    assert G["summary"][0] == 0
    fb = gr.disperse_guided(p16, blob, nt, xi, sigma, su, G["gain_u"], G["gain_t"], 0.5)
    args = (p16, blob, nt, xi, sigma, su, G["gain_u"], G["gain_t"], 0.5, G["ff_u"], G["ff_t"], E_FT)
    known = ffr.disperse_navigated(*args)
    sn = np.zeros(8)
    sn[7] = 10.0
    approx = ffr.disperse_navigated(*args, xn, sn)
    sd = lambda d: np.sqrt(d["stats"][19:64][[np.flatnonzero((dr.IU[0] == i) & (dr.IU[1] == i))[0] for i in (7, 8)]])
    sf, sk, sa = sd(fb), sd(known), sd(approx)
    print("1-sigma of the flown periapsis / apoapsis altitude (m): feedback only", sf, "feed-forward, thrust known", sk,
          "feed-forward, thrust known to 10 N", sa)
    print("clipped steps (mean): feedback only", fb["effort"][:, 0].mean(), "known", known["effort"][:, 0].mean(), "10 N",
          approx["effort"][:, 0].mean(), "max |f_k|", G["summary"][5], "|f_t|", G["summary"][6])
    assert fb["stats"][0] == 128 and known["stats"][0] == 128 and approx["stats"][0] == 128
    assert sk[0] * 10.0 <= sf[0]
    assert sk[0] < sa[0] < sf[0]
    assert np.all(known["effort"][:, 0] == 0) and np.all(approx["effort"][:, 0] == 0)


@pytest.fixture(scope="module")
def lib():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib, build
    build.build()
    return _lib.load()


def _feedforward_calls():
    def gains(L, a, o):
        return L.ascent_guidance_feedforward(a["p"], a["batch"], o, a["blob"], a["substeps"], a["weights"], a["ff_dir"], a["ff_know"],
                                             a["out"], a["out2"], a["ff_u"], a["ff_t"], a["out3"], a["jac"], a["jac_u"], a["jac_nav"],
                                             0, None, 0)

    def navigated(L, a, o):
        return L.ascent_disperse_navigated_batch(a["p"], a["batch"], o, a["blob"], a["substeps"], a["samples"], a["xi"], a["sigma"],
                                                 a["opt"], a["gain_u"], a["opt"], a["opt"], a["ff_u"], a["ff_t"], a["ff_know"],
                                                 a["xi_nav"], a["sigma_nav"], a["out"], a["opt"], 0, None, 0)
    return dict(ascent_guidance_feedforward=gains, ascent_disperse_navigated_batch=navigated)


@pytest.mark.parametrize("name", sorted(_feedforward_calls()))
def test_feedforward_entry_points_refuse_bad_arguments_before_the_device(lib, name):
    """Every argument error of the two entry points is ASCENT_E_ARG with its own message, on a machine with or without a GPU:
    refusals come before the device is looked at.  A refused call touches none of its arrays."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    assert name in _lib.SYMBOLS
    call = _feedforward_calls()[name]
    P = np.vstack([A.AscentParams().as_row()] * 2)
    P0 = P.copy()
    P0[1, 15] = 0.0
    arrays = {k: np.full(8, 7.25) for k in ("blob", "out", "out2", "out3", "opt", "weights", "jac", "jac_u", "jac_nav", "xi", "sigma",
                                            "gain_u", "ff_dir", "ff_know", "ff_u", "ff_t", "xi_nav", "sigma_nav")}
    good = dict({k: v.ctypes.data_as(C.c_void_p) for k, v in arrays.items()}, p=P.ctypes.data_as(C.c_void_p), batch=2, substeps=0,
                samples=4)
    gains = name == "ascent_guidance_feedforward"

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
        refused(b"null ff_dir", ff_dir=None)
        refused(b"null ff_dir", ff_u=None)
        refused(b"null ff_dir", ff_t=None)
        refused(b"jac_u_cl_out needs jac_cl_out", jac=None, jac_nav=None)
        refused(b"jac_nav_out needs jac_cl_out", jac=None, jac_u=None)
        refused(b"jac_cl_out needs ff_know", ff_know=None)
        refused(b"terminal 2", o=opts(terminal=2))
    else:
        refused(b"null", xi=None)
        refused(b"null", sigma=None)
        refused(b"null", gain_u=None)
        refused(b"samples", samples=0)
        refused(b"samples", samples=65537)
        refused(b"xi_nav and sigma_nav", xi_nav=None)
        refused(b"xi_nav and sigma_nav", sigma_nav=None)
        refused(b"ff_know needs ff_u", ff_u=None)
    for k, v in arrays.items():
        assert (v == 7.25).all(), k


def test_python_front_end_checks_shapes():
    import lunar_module_ascent_trajectory_optimiser_amd as A
    nt, K = 18, 17
    P = np.vstack([A.AscentParams().as_row()] * 2)
    blob = np.zeros((21 * K + 10, 2))
    assert A.GUIDE_FF_ROWS[:5] == A.GUIDE_ROWS and len(A.GUIDE_FF_ROWS) == 7
    g5 = A.GuidanceResult(np.zeros((2, K, 7)), np.zeros((2, 7)), np.zeros((2, 5)), np.zeros(2), None)
    assert g5.ff_u is None and g5.ff_t is None and g5.ff_dir is None and g5.ff_know is None and g5.jacobian_nav is None
    with pytest.raises(ValueError):
        A.guidance_gains(P, blob, nt, feedforward="thrust")
    with pytest.raises(ValueError):
        A.guidance_gains(P, blob, nt, feedforward=np.zeros(15))
    with pytest.raises(ValueError):
        A.guidance_gains(P, blob, nt, feedforward="Ft", knowledge=np.zeros((3, 16)))
    with pytest.raises(ValueError):
        A.guidance_gains(P, blob, nt, knowledge=np.zeros(16))
    with pytest.raises(ValueError):
        A.disperse_batch(P, blob, nt, nav_sigma=np.zeros(7))
    with pytest.raises(ValueError):
        A.disperse_batch(P, blob, nt, guidance=g5, nav_sigma=np.zeros(6))
    with pytest.raises(ValueError):
        A.disperse_batch(P, blob, nt, guidance=g5, knowledge_sigma=np.zeros(3))
    with pytest.raises(ValueError):
        A.disperse_batch(P, blob, nt, guidance=g5, nav_sigma=np.zeros(7), xi_nav=np.zeros((7, 256)))
    for bad in (dict(ff_u=np.zeros((2, K - 1))), dict(ff_u=np.zeros((2, K)), ff_t=np.zeros(3)),
                dict(ff_u=np.zeros((2, K)), ff_t=np.zeros(2), ff_know=np.zeros((2, 15)))):
        with pytest.raises(ValueError):
            A.disperse_batch(P, blob, nt, guidance=A.GuidanceResult(g5.gain_u, g5.gain_t, np.zeros((2, 7)), g5.stretch_max, None, **bad))
    d = A.DispersionResult(*([None] * 12))
    assert d.xi_nav is None and d.nav_sigma is None
