"""The library surface of the Monte Carlo dispersion (include/ascent.h: ascent_disperse_batch): export and binding, argument
checks before the device, and DispersionResult's host-side algebra.  No GPU."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbol_is_exported_and_bound(lib):
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    assert "ascent_disperse_batch" in _lib.SYMBOLS and hasattr(lib, "ascent_disperse_batch")
    assert lib.ascent_disperse_batch.restype is C.c_int and len(lib.ascent_disperse_batch.argtypes) == 14
    assert callable(A.disperse_batch) and A.DispersionResult and callable(A.BatchResult.disperse)
    assert "disperse_batch" in A.__all__ and "DispersionResult" in A.__all__


def test_argument_errors_are_refused_before_the_device(lib):
    """ASCENT_E_ARG with or without a GPU, each with its own message; a refused call touches none of its arrays."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    nt, K, B, S = 18, 17, 2, 4
    P = np.vstack([A.AscentParams().as_row()] * B)
    arrays = dict(blob=np.full((21 * K + 10, B), 7.25), xi=np.full((24 + K, S), 7.25), sigma=np.full((24, B), 7.25),
                  sigma_u=np.full((K, B), 7.25), stats=np.full((82, B), 7.25), samples_out=np.full((9, S, B), 7.25))
    good = dict({k: v.ctypes.data_as(C.c_void_p) for k, v in arrays.items()}, p=P.ctypes.data_as(C.c_void_p), batch=B, substeps=0,
                samples=S)

    def opts(**kw):
        return _lib.AscentOptsC(**dict(dict(n_nodes=nt, scheme=0, max_iter=0, warm_start=0, tol=1.0, mu_init=0.0), **kw))

    def refused(what, o=None, null_opts=False, **changes):
        a = dict(good, **changes)
        rc = lib.ascent_disperse_batch(a["p"], a["batch"], None if null_opts else C.byref(o if o is not None else opts()), a["blob"],
                                       a["substeps"], a["samples"], a["xi"], a["sigma"], a["sigma_u"], a["stats"], a["samples_out"],
                                       0, None, 0)
        msg = lib.ascent_strerror(rc)
        assert rc == -1 and what in msg, (changes, rc, msg)

    refused(b"null", xi=None)
    refused(b"null", sigma=None)
    refused(b"null", stats=None)
    refused(b"null", blob=None)
    refused(b"null", p=None)
    refused(b"null", null_opts=True)
    refused(b"batch <= 0", batch=0)
    refused(b"samples", samples=0)
    refused(b"samples", samples=65537)
    refused(b"samples", samples=-1)
    refused(b"substeps", substeps=-1)
    refused(b"substeps", substeps=4097)
    # what ascent_fly_batch refuses
    refused(b"scheme", o=opts(scheme=7))
    P0 = P.copy()
    P0[1, 15] = 0.0
    refused(b"dcost", o=opts(move_penalty=1), p=P0.ctypes.data_as(C.c_void_p))
    refused(b"n_nodes", o=opts(n_nodes=2))
    refused(b"formulation 1", o=opts(formulation=1, scheme=1))
    refused(b"terminal 2 has formulation 0 only", o=opts(terminal=2, formulation=1))
    for k, v in arrays.items():
        assert (v == 7.25).all(), k


def test_terminal_2_passes_the_argument_checks(lib):
    """terminal = 2 is not an argument error here (the flight Jacobian and the trim refuse it): the call gets as far as the
    device -- ASCENT_OK with one, ASCENT_E_NODEVICE without."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    nt, K = 3, 2
    P = np.asarray(A.AscentParams().as_row()).reshape(1, 16).copy()
    blob, xi, sigma, stats = np.zeros((21 * K + 10, 1)), np.zeros((24, 1)), np.zeros((24, 1)), np.zeros((82, 1))
    o = _lib.AscentOptsC(n_nodes=nt, scheme=0, max_iter=0, warm_start=0, tol=1.0, mu_init=0.0, terminal=2)
    p = [a.ctypes.data_as(C.c_void_p) for a in (P, blob, xi, sigma, stats)]
    rc = lib.ascent_disperse_batch(p[0], 1, C.byref(o), p[1], 1, 1, p[2], p[3], None, p[4], None, 0, None, 0)
    assert rc in (0, -3), (rc, lib.ascent_strerror(rc))


def test_python_front_end_checks_shapes():
    import lunar_module_ascent_trajectory_optimiser_amd as A
    nt, K = 18, 17
    P = np.vstack([A.AscentParams().as_row()] * 2)
    with pytest.raises(ValueError):
        A.disperse_batch(P, np.zeros((21 * K + 9, 2)), nt)
    with pytest.raises(ValueError):
        A.disperse_batch(P, np.zeros((21 * K + 10, 2)), nt, xi=np.zeros((24, 8)))
    with pytest.raises(ValueError):
        A.disperse_batch(P, np.zeros((21 * K + 10, 2)), nt, param_sigma=np.zeros(15))


def test_linear_covariance_on_a_hand_made_jacobian():
    """Two non-zero columns: thrust (param 3) and the second control of K = 2.  J D C_xi D J' written out by hand with the
    sample covariance of the two rows of xi that these columns read."""
    from lunar_module_ascent_trajectory_optimiser_amd import DispersionResult, FlightJacobian
    B, K, S = 2, 2, 5
    rng = np.random.default_rng(7)
    xi = rng.standard_normal((24 + K, S))
    a, b = rng.standard_normal((B, 9)), rng.standard_normal((B, 9))        # d / d Ft, d / d u_2
    dparams, dcontrols = np.zeros((B, 9, 16)), np.zeros((B, 9, K))
    dparams[:, :, 3], dcontrols[:, :, 1] = a, b
    J = FlightJacobian(np.zeros((B, 9, 7)), dparams, np.zeros((B, 9)), dcontrols)
    ps, cs = np.zeros((B, 16)), np.zeros((B, K))
    ps[:, 3], cs[:, 1] = [50.0, 20.0], [1e-3, 2e-3]
    z9, z99 = np.zeros((B, 9)), np.zeros((B, 9, 9))
    r = DispersionResult(np.full(B, S), z9, z9, z99, z9, z9, None, xi, np.zeros((B, 7)), ps, np.zeros(B), cs)
    x1, x2 = xi[7 + 3], xi[24 + 1]
    c11 = ((x1 - x1.mean()) ** 2).sum() / (S - 1)
    c22 = ((x2 - x2.mean()) ** 2).sum() / (S - 1)
    c12 = ((x1 - x1.mean()) * (x2 - x2.mean())).sum() / (S - 1)
    got = r.linear_covariance(J)
    assert got.shape == (B, 9, 9)
    for j in range(B):
        A1, A2 = a[j] * ps[j, 3], b[j] * cs[j, 1]
        want = c11 * np.outer(A1, A1) + c22 * np.outer(A2, A2) + c12 * (np.outer(A1, A2) + np.outer(A2, A1))
        assert np.allclose(got[j], want, rtol=1e-12, atol=0)
        assert np.allclose(got[j], got[j].T, rtol=1e-14, atol=0)
    # without control sigmas a Jacobian without control columns will do
    r0 = DispersionResult(np.full(B, S), z9, z9, z99, z9, z9, None, xi, np.zeros((B, 7)), ps, np.zeros(B), np.zeros((B, K)))
    got0 = r0.linear_covariance(FlightJacobian(J.dz0, J.dparams, J.dtf, None))
    assert np.allclose(got0[0], c11 * np.outer(a[0] * 50.0, a[0] * 50.0), rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        r.linear_covariance(FlightJacobian(J.dz0, J.dparams, J.dtf, None))
    assert np.array_equal(DispersionResult(np.full(B, S), z9, z9, np.tile(4.0 * np.eye(9), (B, 1, 1)), z9, z9, None, xi, np.zeros((B, 7)), ps,
                                           np.zeros(B), cs).std, np.full((B, 9), 2.0))
