"""The argument refusals of the linear covariance corridor's entry point (include/ascent.h: ascent_covariance_history_batch) and
of its front end (linear_corridor).  Every refusal comes before the device is looked at: no GPU."""
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


SIG = ("p", "batch", "o", "sol_blob", "substeps", "sigma", "sigma_u", "gain_u", "gain_t", "stretch_max", "ff_u", "ff_t", "ff_know", "sigma_nav",
       "node_stride", "nominal_out", "cov_out", "jac_hist_out", "device_id", "stream", "ptr_is_device")
SCALARS = dict(batch=2, substeps=0, node_stride=1, device_id=0, stream=None, ptr_is_device=0)
LAW = ("gain_t", "stretch_max", "ff_u", "ff_t", "ff_know", "sigma_nav")
# (defect, null arguments, scalars, options, the text names)
REFUSALS = [
    ("null options", ("o",), {}, {}, ""),
    ("null blob", ("sol_blob",), {}, {}, "solution blob"),
    ("null sigma", ("sigma",), {}, {}, "sigma"),
    ("null nominal_out", ("nominal_out",), {}, {}, "nominal_out"),
    ("null cov_out", ("cov_out",), {}, {}, "cov_out"),
    ("stride 0", (), dict(node_stride=0), {}, "node_stride"),
    ("stride K + 1", (), dict(node_stride=K + 1), {}, "node_stride"),
    ("ff_know without ff_u", ("ff_u",), {}, {}, "ff_know needs ff_u"),
    ("substeps -1", (), dict(substeps=-1), {}, "substeps out of range"),
    ("batch 0", (), dict(batch=0), {}, ""),
    ("terminal 2 with formulation 1", (), {}, dict(terminal=2, formulation=1), "terminal 2"),
] + [(f"{name} without gain_u", tuple(n for n in ("gain_u",) + LAW if n != name) + (("ff_u",) if name == "ff_know" else ()), {}, {},
      "ff_know needs ff_u" if name == "ff_know" else "need gain_u") for name in LAW]


@pytest.mark.parametrize("defect,null,scalars,opts,names", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_point_refuses_before_the_device_is_looked_at(lib, defect, null, scalars, opts, names):
    """One defect per call, as tests/test_history_reference.py does it for the history call: ASCENT_E_ARG (-1), the text names the
    defect -- the shared refusals with the text of ascent_disperse_history_batch --, and none of the arrays, filled with 7.25, is
    touched.  The same with or without a GPU."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    assert len(SIG) == len(lib.ascent_covariance_history_batch.argtypes)
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
            buffers.append(np.full(16384, 7.25))
            args.append(buffers[-1].ctypes.data_as(C.c_void_p))
    rc = lib.ascent_covariance_history_batch(*args)
    msg = lib.ascent_strerror(rc).decode()
    assert rc == -1 and names in msg, (defect, rc, msg)
    assert all((b == 7.25).all() for b in buffers), defect


def test_the_shared_refusals_have_the_history_calls_text(lib):
    """node_stride, ff_know and what needs gain_u are refused by the functions the history call uses: the same text from both."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    P = np.vstack([A.AscentParams().as_row()] * 2)
    o = _lib.AscentOptsC(n_nodes=NT, scheme=0, max_iter=0, warm_start=0, tol=1.0, mu_init=0.0)
    buf = lambda: np.full(16384, 7.25).ctypes.data_as(C.c_void_p)
    keep = []

    def both(stride, gain_u, gain_t, ff_u, ff_know):
        ptr = lambda on: (keep.append(np.full(16384, 7.25)) or keep[-1].ctypes.data_as(C.c_void_p)) if on else None
        head = [P.ctypes.data_as(C.c_void_p), 2, C.byref(o), buf(), 0]
        law = [ptr(gain_u), ptr(gain_t), None, ptr(ff_u), None, ptr(ff_know)]
        rc = lib.ascent_covariance_history_batch(*head, buf(), None, *law, None, stride, buf(), buf(), None, 0, None, 0)
        a = lib.ascent_strerror(rc).decode()
        rc2 = lib.ascent_disperse_history_batch(*head, 4, buf(), buf(), None, *law, None, None, stride, buf(), None, buf(), None, 0, None, 0)
        return rc, a, rc2, lib.ascent_strerror(rc2).decode()

    for case in ((0, True, False, False, False), (1, False, True, False, False), (1, True, False, False, True)):
        rc, a, rc2, b = both(*case)
        assert rc == rc2 == -1 and a == b, (case, a, b)


def test_front_end_refuses_bad_shapes(lib):
    import lunar_module_ascent_trajectory_optimiser_amd as A
    P = A.AscentParams().as_row()[None].copy()
    blob = _blob()[:, None]
    for bad in (0, K + 1, -3, False, None):
        with pytest.raises(ValueError, match="stride"):
            A.linear_corridor(P, blob, NT, history=bad)
    for kw, what in ((dict(param_sigma=np.ones(15)), "param_sigma"), (dict(z0_sigma=np.ones((2, 7))), "z0_sigma"),
                     (dict(control_sigma=np.ones(K + 1)), "control_sigma"), (dict(tf_sigma=np.ones(3)), "tf_sigma")):
        with pytest.raises(ValueError, match=what):
            A.linear_corridor(P, blob, NT, **kw)
    with pytest.raises(ValueError, match="need guidance"):
        A.linear_corridor(P, blob, NT, nav_sigma=np.ones(7))
    with pytest.raises(ValueError, match="need guidance"):
        A.linear_corridor(P, blob, NT, knowledge_sigma=1.0)
    g = A.GuidanceResult(np.zeros((1, K + 1, 7)), np.zeros((1, 7)), np.zeros((1, 5)), np.full(1, 0.5), None)
    with pytest.raises(ValueError, match="gain_u"):
        A.linear_corridor(P, blob, NT, guidance=g)
    g = A.GuidanceResult(np.zeros((1, K, 7)), np.zeros((1, 6)), np.zeros((1, 5)), np.full(1, 0.5), None)
    with pytest.raises(ValueError, match="gain_t"):
        A.linear_corridor(P, blob, NT, guidance=g)
    g = A.GuidanceResult(np.zeros((1, K, 7)), np.zeros((1, 7)), np.zeros((1, 5)), np.full(1, 0.5), None, ff_u=np.zeros((1, K - 1)))
    with pytest.raises(ValueError, match="ff_u"):
        A.linear_corridor(P, blob, NT, guidance=g)
    assert len(A.LINCOV_COLS) == 32 and A.LINCOV_COLS[7:23] == A.PARAM_FIELDS and A.LINCOV_COLS[23] == "tf"
    assert [f.name for f in A.solver.dataclasses.fields(A.LinearCorridor)] == ["nodes", "nominal", "cov", "jacobian"]
