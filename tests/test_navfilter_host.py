"""The argument refusals of the navigation filter's entry points (include/ascent.h: ascent_navigation_filter,
ascent_covariance_filtered_batch) and of their front ends (navigation_filter, linear_corridor(filter=...)).  Every refusal comes
before the device is looked at: no GPU."""
import ctypes as C

import numpy as np
import pytest

from reference_cases import blob as _blob

NT, K, B = 18, 17, 2


@pytest.fixture(scope="module")
def lib():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib, build
    build.build()
    return _lib.load()


SIGS = {
    "ascent_navigation_filter": ("p", "batch", "o", "sol_blob", "substeps", "sigma_nav", "sigma_u", "filter_q", "meas_h", "meas_sigma", "n_meas",
                                 "meas_stride", "gain_l_out", "pfilt_out", "summary_out", "device_id", "stream", "ptr_is_device"),
    "ascent_covariance_filtered_batch": ("p", "batch", "o", "sol_blob", "substeps", "sigma", "sigma_u", "gain_u", "gain_t", "stretch_max",
                                         "sigma_nav", "gain_l", "meas_h", "meas_sigma", "n_meas", "meas_stride", "node_stride", "nominal_out",
                                         "cov_out", "nav_cov_out", "jac_hist_out", "nav_jac_out", "device_id", "stream", "ptr_is_device"),
}
SCALARS = dict(batch=B, substeps=0, n_meas=2, meas_stride=1, node_stride=1, device_id=0, stream=None, ptr_is_device=0)
# (defect, null arguments, scalars, options, values written into an array, the text names)
SHARED = [
    ("null options", ("o",), {}, {}, {}, ""),
    ("null blob", ("sol_blob",), {}, {}, {}, "solution blob"),
    ("batch 0", (), dict(batch=0), {}, {}, ""),
    ("substeps -1", (), dict(substeps=-1), {}, {}, "substeps out of range"),
    ("terminal 2 with formulation 1", (), {}, dict(terminal=2, formulation=1), {}, "terminal 2"),
    ("n_meas 0", (), dict(n_meas=0), {}, {}, "n_meas"),
    ("n_meas 5", (), dict(n_meas=5), {}, {}, "n_meas"),
    ("meas_stride 0", (), dict(meas_stride=0), {}, {}, "meas_stride"),
    ("null sigma_nav", ("sigma_nav",), {}, {}, {}, "sigma_nav"),
    ("null meas_h", ("meas_h",), {}, {}, {}, "meas_h"),
    ("null meas_sigma", ("meas_sigma",), {}, {}, {}, "meas_sigma"),
    ("meas_sigma 0", (), {}, {}, dict(meas_sigma=(3, 0.0)), "meas_sigma"),
    ("meas_sigma negative", (), {}, {}, dict(meas_sigma=(0, -1.0)), "meas_sigma"),
    ("meas_sigma NaN", (), {}, {}, dict(meas_sigma=(1, np.nan)), "meas_sigma"),
    ("meas_h inf", (), {}, {}, dict(meas_h=(2 * 7 * B - 1, np.inf)), "meas_h"),
    ("sigma_nav NaN", (), {}, {}, dict(sigma_nav=(7 * B - 1, np.nan)), "sigma_nav"),
]
REFUSALS = {
    "ascent_navigation_filter": SHARED + [
        ("null gain_l_out", ("gain_l_out",), {}, {}, {}, "gain_l_out"),
        ("null summary_out", ("summary_out",), {}, {}, {}, "summary_out"),
        ("filter_q inf", (), {}, {}, dict(filter_q=(0, np.inf)), "filter_q"),
    ],
    "ascent_covariance_filtered_batch": SHARED + [
        ("null sigma", ("sigma",), {}, {}, {}, "sigma"),
        ("null nominal_out", ("nominal_out",), {}, {}, {}, "nominal_out"),
        ("null cov_out", ("cov_out",), {}, {}, {}, "cov_out"),
        ("null nav_cov_out", ("nav_cov_out",), {}, {}, {}, "nav_cov_out"),
        ("null gain_l", ("gain_l",), {}, {}, {}, "gain_l"),
        ("stride 0", (), dict(node_stride=0), {}, {}, "node_stride"),
        ("stride K + 1", (), dict(node_stride=K + 1), {}, {}, "node_stride"),
        ("gain_t without gain_u", ("gain_u", "stretch_max"), {}, {}, {}, "need gain_u"),
        ("stretch_max without gain_u", ("gain_u", "gain_t"), {}, {}, {}, "need gain_u"),
    ],
}
CASES = [(fn, *r) for fn, rs in REFUSALS.items() for r in rs]


@pytest.mark.parametrize("fn,defect,null,scalars,opts,values,names", CASES, ids=[f"{c[0].split('_')[1]}-{c[1]}" for c in CASES])
def test_entry_point_refuses_before_the_device_is_looked_at(lib, fn, defect, null, scalars, opts, values, names):
    """One defect per call: ASCENT_E_ARG (-1), the text names the defect, and none of the arrays, filled with 7.25 (a legal value
    of every input), is touched apart from the one value the case itself writes.  The same with or without a GPU."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    sig = SIGS[fn]
    assert len(sig) == len(getattr(lib, fn).argtypes)
    P = np.vstack([A.AscentParams().as_row()] * B)
    o = _lib.AscentOptsC(**dict(dict(n_nodes=NT, scheme=0, max_iter=0, warm_start=0, tol=1.0, mu_init=0.0), **opts))
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
            buf = np.full(16384, 7.25)
            if name in values:
                buf[values[name][0]] = values[name][1]
            buffers.append((name, buf))
            args.append(buf.ctypes.data_as(C.c_void_p))
    rc = getattr(lib, fn)(*args)
    msg = lib.ascent_strerror(rc).decode()
    assert rc == -1 and names in msg, (defect, rc, msg)
    for name, buf in buffers:
        keep = np.ones(buf.size, dtype=bool)
        if name in values:
            keep[values[name][0]] = False
        assert (buf[keep] == 7.25).all(), (defect, name)


def test_a_stride_above_K_passes_the_argument_checks(lib):
    """meas_stride = K + 1 is legal: with every argument in order the call gets as far as the device (ASCENT_OK with one, the HIP or
    device error without) -- never ASCENT_E_ARG."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    nf = None
    try:
        nf = A.navigation_filter(A.AscentParams().as_row()[None].copy(), _blob()[:, None], NT, nav_sigma=1e-3, meas_rows=np.eye(7)[:2],
                                 meas_sigma=1e-4, meas_stride=K + 1)
    except A._lib.AscentLibraryError as e:
        assert "libascent error -1" not in str(e), e
    if nf is not None:
        assert np.all(nf.gain_l == 0) and nf.gain_l.shape == (1, K, 2, 7) and nf.cov.shape == (1, K, 7, 7) and (nf.meas_nodes == 0).all()


class _Filter:
    """what linear_corridor(filter=...) reads of a NavigationFilter"""
    def __init__(self, **kw):
        self.gain_l, self.meas_rows, self.meas_sigma = np.zeros((1, K, 2, 7)), np.eye(7)[:2], np.full(2, 1e-4)
        self.meas_stride, self.nav_sigma = 1, np.full(7, 1e-3)
        self.__dict__.update(kw)


def test_front_ends_refuse_bad_shapes_and_combinations(lib):
    import lunar_module_ascent_trajectory_optimiser_amd as A
    P = A.AscentParams().as_row()[None].copy()
    blob = _blob()[:, None]
    ok = dict(nav_sigma=1e-3, meas_rows=np.eye(7)[:2], meas_sigma=1e-4)
    for kw, what in ((dict(meas_stride=0), "meas_stride"), (dict(meas_rows=np.eye(7)[:5]), "meas_rows"), (dict(meas_rows=np.ones((2, 6))), "meas_rows"),
                     (dict(meas_rows=np.ones((3, 2, 7))), "meas_rows"), (dict(meas_sigma=np.ones(3)), "meas_sigma"), (dict(meas_sigma=0.0), "meas_sigma"),
                     (dict(meas_sigma=None), "meas_sigma"), (dict(meas_rows=np.full((1, 7), np.nan)), "meas_rows"), (dict(nav_sigma=np.ones(6)), "nav_sigma"),
                     (dict(nav_sigma=None), "nav_sigma"), (dict(nav_sigma=np.inf), "nav_sigma"), (dict(control_sigma=np.ones(K + 1)), "control_sigma"),
                     (dict(process_sigma=np.ones(8)), "process_sigma")):
        with pytest.raises(ValueError, match=what):
            A.navigation_filter(P, blob, NT, **dict(ok, **kw))
    g = A.GuidanceResult(np.zeros((1, K, 7)), np.zeros((1, 7)), np.zeros((1, 5)), np.full(1, 0.5), None)
    ff = A.GuidanceResult(np.zeros((1, K, 7)), np.zeros((1, 7)), np.zeros((1, 7)), np.full(1, 0.5), None, ff_u=np.zeros((1, K)), ff_t=np.zeros(1))
    for kw, what in ((dict(knowledge_sigma=1.0), "knowledge_sigma"), (dict(guidance=ff), "feed-forward"), (dict(nav_tau=10.0), "nav_tau"),
                     (dict(knowledge_tau=10.0), "nav_tau"), (dict(nav_steady_sigma=1e-3), "nav_tau"), (dict(knowledge_steady_sigma=1.0), "nav_tau"),
                     (dict(history=0), "stride"), (dict(history=K + 1), "stride"), (dict(nav_sigma=np.ones(6)), "nav_sigma")):
        with pytest.raises(ValueError, match=what):
            A.linear_corridor(P, blob, NT, **dict(dict(guidance=g, filter=_Filter()), **kw))
    for bad, what in ((_Filter(gain_l=np.zeros((1, K + 1, 2, 7))), "gain_l"), (_Filter(gain_l=np.zeros((1, K, 5, 7))), "gain_l"),
                      (_Filter(gain_l=np.zeros((1, K, 1, 7))), "disagree"), (_Filter(meas_stride=0), "meas_stride"),
                      (_Filter(meas_sigma=np.zeros(2)), "meas_sigma")):
        with pytest.raises(ValueError, match=what):
            A.linear_corridor(P, blob, NT, guidance=g, filter=bad)
    assert A.NAVFILTER_ROWS == ("status", "first_bad", "meas_nodes", "substeps")
    lc = A.LinearCorridor(np.arange(1), np.zeros((1, 1, 10)), np.zeros((1, 1, 10, 10)), None)
    assert lc.nav_cov is None and lc.nav_std is None and lc.nav_jacobian is None
