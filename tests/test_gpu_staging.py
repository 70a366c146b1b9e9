"""The staging of host-pointer calls (csrc/ascent_solver.hip: Staging) on the paths no other test takes: host pointers on a
caller's stream, and optional outputs left out.  The five entry points that work on a solve's results, through ctypes, at
batch 5 and 40 nodes: two grid levels in the solve, a batch that is a multiple of neither 4 nor 64."""
import ctypes as C

import numpy as np
import pytest

from gpu_cases import ptr as _ptr, same as _same

pytestmark = pytest.mark.gpu

NT, K, B, COAST_NODES = 40, 39, 5, 7


@pytest.fixture(scope="module")
def solved():
    from lunar_module_ascent_trajectory_optimiser_amd import AscentParams, solve_batch, sweep_isp_drymass, _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    sw = sweep_isp_drymass()
    P = np.vstack([AscentParams().as_row(), sw[0], sw[4095], sw[63], sw[4032]])
    L = _lib.load()
    o = _opts(NT, 0, 1.0, 0, 0.0)
    assert L.ascent_workspace_layout(B, C.byref(o), (C.c_int64 * 4)()) == 2      # two grid levels
    r = solve_batch(P, NT, want_blob=True)
    assert (r.status == 0).all()
    return L, P, r.blob, np.ascontiguousarray(r.traj[:4, -1, :]), o


def _calls(L, P, blob, state, o, stream, optional=True):
    """every entry point once with host pointers on `stream`; returns {name: {output: array or None}}"""
    out = {}

    def run(name, fn, *args, **arrays):
        for a in arrays.values():
            if a is not None:
                a.fill(-7.0)
        assert fn(*args) == 0, (name, L.ascent_strerror(-2))
        out[name] = arrays

    opt = (lambda *shape: np.empty(shape)) if optional else (lambda *shape: None)
    traj, local, summ = opt(10, NT, B), opt(K, 7, B), np.empty((10, B))
    run("fly", L.ascent_fly_batch, _ptr(P), B, C.byref(o), _ptr(blob), 0, _ptr(traj), _ptr(local), _ptr(summ), 0, stream, 0,
        traj=traj, local=local, summary=summ)
    g = np.empty((16, B))
    run("sensitivity", L.ascent_param_sensitivity, _ptr(P), B, C.byref(o), _ptr(blob), _ptr(g), 0, stream, 0, grad=g)
    jac, ju = np.empty((9, 24, B)), opt(9, K, B)
    run("jacobian", L.ascent_flight_jacobian, _ptr(P), B, C.byref(o), _ptr(blob), 0, _ptr(jac), _ptr(ju), 0, stream, 0, jac=jac, jac_u=ju)
    tb, ts = np.empty_like(blob), np.empty((10, B))
    run("trim", L.ascent_trim_batch, _ptr(P), B, C.byref(o), _ptr(blob), 0, 0, 0.0, _ptr(tb), _ptr(ts), 0, stream, 0, blob=tb, summary=ts)
    ct, ctf, aps = np.empty((4, COAST_NODES + 1, B)), np.empty(B), np.empty((2, B))
    run("coast", L.ascent_coast_batch, _ptr(P), B, _ptr(state), COAST_NODES, _ptr(ct), _ptr(ctf), _ptr(aps), 0, stream, 0,
        traj=ct, tf=ctf, apsides=aps)
    return out


def test_host_pointers_on_a_caller_stream_and_without_optional_outputs(solved):
    import torch
    L, P, blob, state, o = solved
    blob0 = blob.copy()
    ref = _calls(L, P, blob, state, o, None)
    for name, arrays in ref.items():
        for k, a in arrays.items():
            assert not (a == -7.0).all(), (name, k)      # (written)
    side = torch.cuda.Stream()
    on_stream = _calls(L, P, blob, state, o, C.c_void_p(side.cuda_stream))
    without = _calls(L, P, blob, state, o, None, optional=False)
    without_on_stream = _calls(L, P, blob, state, o, C.c_void_p(side.cuda_stream), optional=False)
    for name, arrays in ref.items():
        for k, a in arrays.items():
            assert _same(on_stream[name][k], a), (name, k)
            for got in (without, without_on_stream):
                assert got[name][k] is None or _same(got[name][k], a), (name, k)
    assert without["fly"]["traj"] is None and without["fly"]["local"] is None and without["jacobian"]["jac_u"] is None
    assert np.array_equal(blob, blob0)
