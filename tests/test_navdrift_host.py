"""The argument refusals of the two entry points of the time-varying navigation error (include/ascent.h:
ascent_disperse_drifting_batch, ascent_covariance_drifting_batch), the translation of time constants into phi and q, and the
front end's own refusals.  Every refusal comes before the device is looked at: no GPU."""
import ctypes as C

import numpy as np
import pytest

from reference_cases import blob as _blob

NT, K = 18, 17


@pytest.fixture(scope="module")
def lib():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib, build
    build.build()
    return _lib.load()


MC_SIG = ("p", "batch", "o", "sol_blob", "substeps", "samples", "xi", "sigma", "sigma_u", "gain_u", "gain_t", "stretch_max", "ff_u", "ff_t",
          "ff_know", "xi_nav", "sigma_nav", "nav_phi", "nav_q", "xi_drift", "node_stride", "stats_out", "samples_out", "hist_out",
          "hist_samples_out", "device_id", "stream", "ptr_is_device")
LC_SIG = ("p", "batch", "o", "sol_blob", "substeps", "sigma", "sigma_u", "gain_u", "gain_t", "stretch_max", "ff_u", "ff_t", "ff_know", "sigma_nav",
          "nav_phi", "nav_q", "node_stride", "nominal_out", "cov_out", "jac_hist_out", "device_id", "stream", "ptr_is_device")
SCALARS = dict(batch=2, substeps=0, samples=4, node_stride=1, device_id=0, stream=None, ptr_is_device=0)
# (defect, null arguments, scalars, values of phi and q, the text names, which calls: "mc", "lc" or both)
REFUSALS = [
    # the parent calls' own
    ("null options", ("o",), {}, None, "", "mc lc"),
    ("null blob", ("sol_blob",), {}, None, "solution blob", "mc lc"),
    ("null sigma", ("sigma",), {}, None, "sigma", "mc lc"),
    ("null xi", ("xi",), {}, None, "xi", "mc"),
    ("null stats_out", ("stats_out",), {}, None, "stats_out", "mc"),
    ("null hist_out", ("hist_out",), {}, None, "hist_out", "mc"),
    ("null nominal_out", ("nominal_out",), {}, None, "nominal_out", "lc"),
    ("null cov_out", ("cov_out",), {}, None, "cov_out", "lc"),
    ("samples 0", (), dict(samples=0), None, "samples out of range", "mc"),
    ("xi_nav without sigma_nav", ("sigma_nav",), {}, None, "come together", "mc"),
    ("stride 0", (), dict(node_stride=0), None, "node_stride", "mc lc"),
    ("stride K + 1", (), dict(node_stride=K + 1), None, "node_stride", "mc lc"),
    ("ff_know without ff_u", ("ff_u",), {}, None, "ff_know needs ff_u", "mc lc"),
    ("substeps -1", (), dict(substeps=-1), None, "substeps out of range", "mc lc"),
    ("gain_t without gain_u", ("gain_u", "stretch_max", "ff_u", "ff_t", "ff_know", "xi_nav", "sigma_nav", "nav_phi", "nav_q", "xi_drift"), {}, None,
     "need gain_u", "mc lc"),
    # the new ones
    ("nav_phi without nav_q", ("nav_q",), {}, None, "nav_phi and nav_q come together", "mc lc"),
    ("nav_q without nav_phi", ("nav_phi",), {}, None, "nav_phi and nav_q come together", "mc lc"),
    ("nav_phi and nav_q without gain_u", ("gain_u", "gain_t", "stretch_max", "ff_u", "ff_t", "ff_know", "xi_nav", "sigma_nav"), {}, None,
     "nav_phi and nav_q need gain_u", "mc lc"),
    ("nav_q without xi_drift", ("xi_drift",), {}, None, "nav_q needs xi_drift", "mc"),
    ("phi above 1", (), {}, ((3, 1, 1.0000001), None), "nav_phi outside [0, 1]", "mc lc"),
    ("phi below 0", (), {}, ((0, 0, -1e-9), None), "nav_phi outside [0, 1]", "mc lc"),
    ("phi NaN", (), {}, ((7, 1, np.nan), None), "nav_phi outside [0, 1]", "mc lc"),
    ("phi inf", (), {}, ((7, 0, np.inf), None), "nav_phi outside [0, 1]", "mc lc"),
    ("q negative", (), {}, (None, (2, 0, -1.0)), "nav_q negative or not finite", "mc lc"),
    ("q NaN", (), {}, (None, (5, 1, np.nan)), "nav_q negative or not finite", "mc lc"),
    ("q inf", (), {}, (None, (7, 1, np.inf)), "nav_q negative or not finite", "mc lc"),
]
CASES = [(r, which) for r in REFUSALS for which in r[5].split()]


@pytest.mark.parametrize("refusal,which", CASES, ids=[f"{w}-{r[0]}" for r, w in CASES])
def test_entry_points_refuse_before_the_device_is_looked_at(lib, refusal, which):
    """One defect per call: ASCENT_E_ARG (-1), the text names the defect, and none of the arrays -- filled with 7.25, phi and q
    with 0.5 but for the defect -- is touched.  The same with or without a GPU."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    defect, null, scalars, values, names, _ = refusal
    sig, fn = (MC_SIG, lib.ascent_disperse_drifting_batch) if which == "mc" else (LC_SIG, lib.ascent_covariance_drifting_batch)
    assert len(sig) == len(fn.argtypes)
    P = np.vstack([A.AscentParams().as_row()] * 2)
    o = _lib.AscentOptsC(n_nodes=NT, scheme=0, max_iter=0, warm_start=0, tol=1.0, mu_init=0.0)
    buffers, args = [], []
    for name in sig:
        if name in null:
            args.append(None)
        elif name == "p":
            args.append(P.ctypes.data_as(C.c_void_p))
        elif name == "o":
            args.append(C.byref(o))
        elif name in SCALARS:
            args.append(scalars.get(name, SCALARS[name]))
        else:
            fill = 0.5 if name in ("nav_phi", "nav_q") else 7.25
            b = np.full(16384, fill)
            v = values[("nav_phi", "nav_q").index(name)] if values and name in ("nav_phi", "nav_q") else None
            if v:
                b[v[0] * 2 + v[1]] = v[2]          # [8][batch = 2]
            buffers.append((b, b.copy()))
            args.append(b.ctypes.data_as(C.c_void_p))
    rc = fn(*args)
    msg = lib.ascent_strerror(rc).decode()
    assert rc == -1 and names in msg, (defect, rc, msg)
    assert all(np.array_equal(b, c, equal_nan=True) for b, c in buffers), defect


def test_time_constants_translate_to_phi_and_q():
    from lunar_module_ascent_trajectory_optimiser_amd import solver
    B = 2
    dt = np.array([2.0, 3.0])
    nav_s = np.tile(np.array([1.0, 2.0, 0.0, 1.0, 1.0, 1.0, 1.0, 5.0]), (B, 1))
    assert solver._nav_drift(None, None, None, None, nav_s, dt, B) == (None, None)
    phi, q = solver._nav_drift(np.inf, None, None, None, nav_s, dt, B)
    assert np.all(phi == 1.0) and np.all(q == 0.0)          # inf and None: exactly frozen
    phi, q = solver._nav_drift([60.0, np.inf, 10.0, 60.0, 60.0, 60.0, 60.0], 5.0, None, 0.0, nav_s, dt, B)
    assert phi.shape == q.shape == (B, 8)
    assert np.array_equal(phi[:, 0], np.exp(-dt / 60.0)) and np.array_equal(phi[:, 7], np.exp(-dt / 5.0))
    assert np.all(phi[:, 1] == 1.0) and np.all(q[:, 1] == 0.0)
    assert np.array_equal(q[:, 0], 1.0 * np.sqrt(1.0 - phi[:, 0] ** 2))          # steady None: the initial sigma, stationary
    assert np.all(q[:, 2] == 0.0) and np.all(q[:, 7] == 0.0)                   # initial sigma 0; steady = 0: pure decay
    phi, q = solver._nav_drift(np.full((B, 7), 30.0), np.array([5.0, 6.0]), 3.0, np.array([1.0, 2.0]), None, dt, B)
    assert np.array_equal(phi[:, 7], np.exp(-dt / np.array([5.0, 6.0])))
    assert np.array_equal(q[:, 3], 3.0 * np.sqrt(1.0 - phi[:, 3] ** 2)) and np.array_equal(q[:, 7], np.array([1.0, 2.0]) * np.sqrt(1.0 - phi[:, 7] ** 2))
    assert np.all((phi >= 0) & (phi <= 1) & (q >= 0))
    # a problem whose blob has no final time: frozen, so that the call is not refused for the whole batch
    phi, q = solver._nav_drift(60.0, 5.0, None, None, nav_s, np.array([np.nan, 2.0]), B)
    assert np.all(phi[0] == 1.0) and np.all(q[0] == 0.0) and np.all(phi[1] < 1.0)
    phi, q = solver._nav_drift(60.0, 5.0, None, None, nav_s, np.array([-1.0, np.inf]), B)
    assert np.all(phi == 1.0) and np.all(q == 0.0)


def test_front_end_refuses(lib):
    import lunar_module_ascent_trajectory_optimiser_amd as A
    P = A.AscentParams().as_row()[None].copy()
    blob = _blob()[:, None]
    for fn in (A.linear_corridor, A.disperse_batch):
        for kw in (dict(nav_tau=60.0), dict(knowledge_tau=5.0), dict(nav_steady_sigma=1e-5), dict(knowledge_steady_sigma=1.0)):
            with pytest.raises(ValueError, match="need guidance"):
                fn(P, blob, NT, **kw)
    with pytest.raises(ValueError, match="need guidance"):
        A.disperse_batch(P, blob, NT, xi_drift=np.zeros((8, K, 256)))
    g = A.GuidanceResult(np.zeros((1, K, 7)), np.zeros((1, 7)), np.zeros((1, 5)), np.full(1, 0.5), None)
    for fn in (A.linear_corridor, A.disperse_batch):
        for kw, what in ((dict(nav_tau=np.ones(6)), "nav_tau"), (dict(knowledge_tau=np.ones(3)), "knowledge_tau"),
                         (dict(nav_tau=1.0, nav_steady_sigma=np.ones((2, 7))), "nav_steady_sigma"),
                         (dict(nav_tau=1.0, knowledge_steady_sigma=np.ones(4)), "knowledge_steady_sigma"),
                         (dict(nav_tau=0.0), "positive"), (dict(knowledge_tau=-1.0), "positive"),
                         (dict(nav_tau=1.0, nav_steady_sigma=-1.0), "negative"), (dict(nav_steady_sigma=1.0), "need nav_tau")):
            with pytest.raises(ValueError, match=what):
                fn(P, blob, NT, guidance=g, **kw)
    with pytest.raises(ValueError, match="xi_drift"):
        A.disperse_batch(P, blob, NT, guidance=g, nav_tau=60.0, samples=4, xi_drift=np.zeros((8, K, 5)))
    with pytest.raises(ValueError, match="xi_drift needs"):
        A.disperse_batch(P, blob, NT, guidance=g, samples=4, xi_drift=np.zeros((8, K, 4)))
    names = [f.name for f in A.solver.dataclasses.fields(A.DispersionResult)]
    assert names[-4:] == ["xi_drift", "nav_phi", "nav_q", "history"]
