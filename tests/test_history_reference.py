"""The CPU reference of the per-node Monte Carlo history (tests/history_reference.py) checked against the three references it
stands beside -- at the last node its state rows are their end rows, bit for bit in float64 --, its altitude against
flight_reference.apsides, its nominal case; and the argument refusals of the entry point (include/ascent.h:
ascent_disperse_history_batch) and of the front end.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import dispersion_reference as dr
import feedforward_reference as ffr
import flight_reference as fr
import guidance_reference as gr
import history_reference as hr
from reference_cases import blob as _blob, p16 as _p16

NT, K, M = 18, 17, 2


def _blobs():
    return (("bounded control with saturated steps", _blob()), ("synthetic exact blob", fr.synthetic_exact_blob(_p16(), NT, tf=0.9, seed=2)))


def _draws(S=5):
    p16 = _p16()
    xi = np.random.default_rng(1).standard_normal((24 + K, S))
    sigma, su = dr.relative_sigma(p16, 1e-3), np.full(K, 1e-3)
    su[5] = 0.0
    return p16, xi, sigma, su


@pytest.mark.parametrize("form", [0, 1])
def test_last_node_is_the_end_of_the_three_dispersion_references(form):
    """Rows 0..6 of node K are the end rows 0..6 of dispersion_reference.disperse, guidance_reference.disperse_guided and
    feedforward_reference.disperse_navigated on the same inputs, bit for bit; the open-loop correction is exactly 0, and the
    clipped flags add up to the effort row of the guided references."""
    p16, xi, sigma, su = _draws()
    xn, sn = np.random.default_rng(2).standard_normal((8, xi.shape[1])), np.array([1e-6] * 7 + [1e-3 * p16[3]])
    e_ft = np.zeros(16)
    e_ft[3] = 1.0
    for name, blob in _blobs():
        op = dr.disperse(p16, blob, NT, xi, sigma, su, form, M)
        h = hr.history(p16, blob, NT, xi, sigma, su, formulation=form, substeps=M)
        assert h["samples"].shape == (xi.shape[1], K, 10) and h["m"] == op["m"], name
        assert np.array_equal(h["samples"][:, -1, :7], op["samples"][:, :7]) and np.array_equal(h["nominal"][-1, :7], op["nominal"][:7]), name
        assert np.all(h["samples"][:, :, 9] == 0.0) and not h["clipped"].any() and np.isinf(h["margin"]).all()
        rec = gr.records(p16, blob, NT, form, M)
        G = ffr.gains(rec, p16, np.array([1e6, 1e6, 1e6, 1.0, 1.0, 0.5]), e_ft)
        assert G["summary"][0] == 0
        gd = gr.disperse_guided(p16, blob, NT, xi, sigma, su, G["gain_u"], G["gain_t"], 0.5, form, M)
        h = hr.history(p16, blob, NT, xi, sigma, su, G["gain_u"], G["gain_t"], 0.5, formulation=form, substeps=M)
        assert np.array_equal(h["samples"][:, -1, :7], gd["samples"][:, :7]) and np.array_equal(h["nominal"][-1, :7], gd["nominal"][:7]), name
        assert np.array_equal(h["clipped"].sum(axis=1), gd["effort"][:, 0]) and np.array_equal(np.abs(h["samples"][:, :, 9]).max(axis=1), gd["effort"][:, 1])
        nv = ffr.disperse_navigated(p16, blob, NT, xi, sigma, su, G["gain_u"], G["gain_t"], 0.5, G["ff_u"], G["ff_t"], e_ft, xn, sn, form, M)
        h = hr.history(p16, blob, NT, xi, sigma, su, G["gain_u"], G["gain_t"], 0.5, G["ff_u"], G["ff_t"], e_ft, xn, sn, form, M)
        assert np.array_equal(h["samples"][:, -1, :7], nv["samples"][:, :7]) and np.array_equal(h["nominal"][-1, :7], nv["nominal"][:7]), name
        assert np.array_equal(h["clipped"].sum(axis=1), nv["effort"][:, 0]) and np.array_equal(np.abs(h["samples"][:, :, 9]).max(axis=1), nv["effort"][:, 1])
        assert np.array_equal(np.where(np.isinf(h["margin"]), np.inf, h["margin"]).min(axis=1), nv["effort"][:, 3])
        # the history's own rows: the nominal control is the blob's, node k of the nominal flight is nominal_nodes' node k
        assert np.array_equal(h["nominal"][:, 8], fr.blob_parts(blob, NT)[1]) and np.all(h["nominal"][:, 9] == 0.0)
        assert np.array_equal(h["nominal"][:, :7], np.asarray(h["nodes"][1:], dtype=np.float64))
        assert np.array_equal(h["stats"][:, 0], np.full(K, xi.shape[1])) and np.array_equal(h["stats"][:, 1:11], h["nominal"])


def test_altitude_is_the_radius_relation_of_apsides():
    """A hand-built state with a purely tangential velocity sits at an apsis of its orbit: below the circular speed the apoapsis of
    flight_reference.apsides is the altitude, above it the periapsis.  1e-6 m: a (1 +- e) - R0 carries a few ulps of a = 1.8e6 m."""
    p16 = _p16()
    x, y = 0.3, 0.02
    X, Y = x * p16[9], y * p16[9] + p16[2]
    r = np.hypot(X, Y)
    vc = np.sqrt(p16[0] * p16[1] / r) / p16[9]
    alt = hr.altitude(p16, x, y)
    assert abs(alt - (r - p16[2])) <= 1e-9
    for f, which in ((0.9, 1), (1.1, 0)):
        got = fr.apsides(p16, x, y, f * vc * Y / r, -f * vc * X / r)[which]
        assert abs(got - alt) <= 1e-6, (f, got, alt)
    # and at node K of a flight the recorded altitude is that of the recorded state
    blob = _blob()
    _, us, tf = fr.blob_parts(blob, NT)
    nodes = gr.nominal_nodes(p16, us, tf, M)
    h, _, _ = hr.fly_history(p16, np.zeros(7), us, np.zeros(K), tf, M, nodes)
    assert h[-1, 7] == hr.altitude(p16, h[-1, 0], h[-1, 1]) and h[0, 7] > 0.0


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_zero_sigmas_give_the_nominal_rows(dtype):
    """All sigmas 0: every sample's history is the nominal row, whatever xi holds, open loop and under a feedback (whose
    correction is then K . 0 = 0); min = max = nominal, the mean within an ulp of it and the variance 0 within that ulp squared."""
    p16, xi, _, _ = _draws(3)
    blob = _blob()
    gu = np.random.default_rng(3).standard_normal((K, 7))
    for g in (None, gu):
        h = hr.history(p16, blob, NT, xi, np.zeros(24), np.zeros(K), g, substeps=M, dtype=dtype)
        s = h["samples"].astype(np.float64)
        assert np.array_equal(s, np.broadcast_to(h["nominal"], s.shape)) and not h["clipped"].any()
        st = h["stats"]
        # numpy's mean of n equal values x is x within an ulp, so its variance is 0 within (eps |x|)^2
        assert np.all(st[:, 21:31] <= (2.3e-16 * np.abs(h["nominal"])) ** 2)
        assert np.array_equal(st[:, 31:41], h["nominal"]) and np.array_equal(st[:, 41:51], h["nominal"])
        assert np.allclose(st[:, 11:21], h["nominal"], rtol=1e-15, atol=0.0) and np.all(st[:, 51] == 0.0)


@pytest.fixture(scope="module")
def lib():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib, build
    build.build()
    return _lib.load()


SIG = ("p", "batch", "o", "sol_blob", "substeps", "samples", "xi", "sigma", "sigma_u", "gain_u", "gain_t", "stretch_max", "ff_u", "ff_t",
       "ff_know", "xi_nav", "sigma_nav", "node_stride", "stats_out", "samples_out", "hist_out", "hist_samples_out", "device_id", "stream",
       "ptr_is_device")
SCALARS = dict(batch=2, substeps=0, samples=4, node_stride=1, device_id=0, stream=None, ptr_is_device=0)
NAV = ("gain_t", "stretch_max", "ff_u", "ff_t", "ff_know", "xi_nav", "sigma_nav")
# (defect, null arguments, scalars, options, the text names)
REFUSALS = [
    ("null hist_out", ("hist_out",), {}, {}, "hist_out"),
    ("stride 0", (), dict(node_stride=0), {}, "node_stride"),
    ("stride K + 1", (), dict(node_stride=K + 1), {}, "node_stride"),
    ("gain_t without gain_u", ("gain_u",) + NAV[1:], {}, {}, "gain_u"),
    ("sigma_nav without xi_nav", ("xi_nav",), {}, {}, "xi_nav and sigma_nav"),
    ("samples 0", (), dict(samples=0), {}, "samples out of range"),
    ("terminal 2 with formulation 1", (), {}, dict(terminal=2, formulation=1), "terminal 2"),
    ("null stats_out", ("stats_out",), {}, {}, "stats_out"),
    ("substeps -1", (), dict(substeps=-1), {}, "substeps out of range"),
]


@pytest.mark.parametrize("defect,null,scalars,opts,names", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_point_refuses_before_the_device_is_looked_at(lib, defect, null, scalars, opts, names):
    """One defect per call, as tests/test_analysis_host.py does it for the nine: ASCENT_E_ARG (-1), the text names the defect, and
    none of the arrays -- filled with 7.25 -- is touched.  The same with or without a GPU."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    assert len(SIG) == len(lib.ascent_disperse_history_batch.argtypes)
    P = np.vstack([A.AscentParams().as_row()] * 2)
    o = _lib.AscentOptsC(**dict(dict(n_nodes=NT, scheme=0, max_iter=0, warm_start=0, tol=1.0, mu_init=0.0), **opts))
    buffers, args = [], []
    for name in SIG:
        if name in null:
            args.append(None)
        elif name == "p":
            args.append(P.ctypes.data_as(C.c_void_p))
        elif name == "o":
            args.append(C.byref(o))
        elif name in SCALARS:
            args.append(scalars.get(name, SCALARS[name]))
        else:
            buffers.append(np.full(4096, 7.25))
            args.append(buffers[-1].ctypes.data_as(C.c_void_p))
    rc = lib.ascent_disperse_history_batch(*args)
    msg = lib.ascent_strerror(rc).decode()
    assert rc == -1 and names in msg, (defect, rc, msg)
    assert all((b == 7.25).all() for b in buffers), defect


def test_front_end_refuses_a_bad_stride_and_samples_without_history(lib):
    import lunar_module_ascent_trajectory_optimiser_amd as A
    P = A.AscentParams().as_row()[None].copy()
    blob = _blob()[:, None]
    for bad in (0, K + 1, -3):
        with pytest.raises(ValueError, match="stride"):
            A.disperse_batch(P, blob, NT, samples=4, history=bad)
    with pytest.raises(ValueError, match="keep_history_samples"):
        A.disperse_batch(P, blob, NT, samples=4, keep_history_samples=True)
    assert A.HISTORY_ROWS == ("x", "y", "xdot", "ydot", "angle", "angledot", "mass", "altitude", "control", "correction")
    assert [f.name for f in A.solver.dataclasses.fields(A.DispersionResult)][-1] == "history"
    assert np.array_equal(A.solver.history_nodes(17, 5), [5, 10, 15, 17]) and np.array_equal(A.solver.history_nodes(17, 17), [17])
