"""The CPU reference of the flight Jacobian and the trim (tests/flight_jacobian_reference.py) checked against central
differences of tests/flight_reference.py, against the identities the model's scalings imply, and on C-oracle solutions; and
the library surface of the two entry points (exports, argument checks).  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import flight_jacobian_reference as jr
import flight_reference as fr
from oracle.ascent_numpy import Params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = fr.FIELDS


def _p16():
    return np.array([getattr(Params(), f) for f in F], dtype=np.float64)


def _blob18(seed):
    p16 = _p16()
    return p16, fr.synthetic_exact_blob(p16, 18, tf=0.9, seed=seed)


def _end(p16, blob, nt, form, m):
    r = fr.fly(p16, blob, nt, formulation=form, substeps=m, want_local=False)
    return np.concatenate([r["traj"][[0, 1, 2, 3, 6, 7, 9], -1], r["summary"][2:4]])


def _row_scale(J, p16, tf):
    """largest entry of every row, the parameter columns as elasticities p d/dp, t_f likewise"""
    el = np.concatenate([J["jac"][:, :7], J["jac"][:, 7:23] * p16, J["jac"][:, 23:] * tf, J["jac_u"]], axis=1)
    scale = np.abs(el).max(axis=1)
    return np.where(scale > 0, scale, 1.0)       # (formulation 1: the angledot row is identically zero)


@pytest.mark.parametrize("form", [0, 1])
def test_reference_against_central_differences(form):
    """Complex-step Jacobian against central differences of flight_reference.fly with relative step 1e-6 (absolute for the
    controls), nt = 18, m = 4 held fixed: every parameter column, t_f and every control, error per row <= 1e-7 of the row's
    largest entry (elasticities).  Seen: 6.4e-10 (the finite differences' own noise).  (flight_reference.fly starts from the
    zero state, so the z_0 columns are not covered here; the identities below and the device test cover them.)"""
    nt, m, K = 18, 4, 17
    p16, blob = _blob18(5 + form)
    tf = blob[21 * K]
    J = jr.jacobian(p16, blob, nt, form, m)
    scale = _row_scale(J, p16, tf)
    assert J["m"] == m and np.all(np.isfinite(J["jac"]))
    worst = 0.0
    for i in range(16):
        if p16[i] == 0.0:        # (dcost: an elasticity of zero whatever the derivative; the exact-zero test covers the column)
            continue
        h = 1e-6 * p16[i]
        a, b = p16.copy(), p16.copy()
        a[i] += h; b[i] -= h
        fd = (_end(a, blob, nt, form, m) - _end(b, blob, nt, form, m)) / (2 * h)
        worst = max(worst, (np.abs(fd - J["jac"][:, 7 + i]) * p16[i] / scale).max())
    h = 1e-6 * tf
    a, b = blob.copy(), blob.copy()
    a[21 * K] += h; b[21 * K] -= h
    fd = (_end(p16, a, nt, form, m) - _end(p16, b, nt, form, m)) / (2 * h)
    worst = max(worst, (np.abs(fd - J["jac"][:, 23]) * tf / scale).max())
    for k in range(K):
        a, b = blob.copy(), blob.copy()
        a[7 * K + k] += 1e-6; b[7 * K + k] -= 1e-6
        fd = (_end(p16, a, nt, form, m) - _end(p16, b, nt, form, m)) / 2e-6
        worst = max(worst, (np.abs(fd - J["jac_u"][:, k]) / scale).max())
    print(f"formulation {form}: complex step against central differences, worst error / row scale {worst:.3g}")
    assert worst <= 1e-7


@pytest.mark.parametrize("form", [0, 1])
def test_identities_and_zero_columns(form):
    """What the model's scalings imply, to 1e-10 of the row scale (seen: about 1e-14): G and M enter as G M; mdot and fuel_mass
    as mdot / fuel_mass; Ft, M0, mass_scalar as Ft / (M0 - mass_scalar m), homogeneous of degree 0; T_scale and t_f as t_f T.
    The end state equals flight_reference.fly's.  The fields the flight does not read give exact zeros."""
    nt, K = 18, 17
    p16, blob = _blob18(9 + form)
    tf = blob[21 * K]
    J = jr.jacobian(p16, blob, nt, form, 0)
    j, scale = J["jac"], _row_scale(J, p16, tf)
    g = {f: j[:, 7 + i] for i, f in enumerate(F)}
    P = dict(zip(F, p16))
    res = [P["G"] * g["G"] - P["M"] * g["M"], P["mdot"] * g["mdot"] + P["fuel_mass"] * g["fuel_mass"],
           P["Ft"] * g["Ft"] + P["M0"] * g["M0"] + P["mass_scalar"] * g["mass_scalar"], P["T_scale"] * g["T_scale"] - tf * j[:, 23]]
    worst = max((np.abs(r) / scale).max() for r in res)
    print(f"formulation {form}: identities, worst residual / row scale {worst:.3g}")
    assert worst <= 1e-10
    assert np.allclose(J["end"], _end(p16, blob, nt, form, 0), rtol=1e-13, atol=1e-15)
    for f in ("r_apo", "tf_lb", "tf_ub", "dcost", "ang_acc_max" if form == 1 else "angle_ub"):
        assert np.all(g[f] == 0.0), f
    for f in ("G", "R0", "Ft", "mdot", "r_peri", "T_scale", "angle_ub" if form == 1 else "ang_acc_max"):
        assert np.any(g[f] != 0.0), f
    if form == 1:      # the reset: the flown state does not depend on the initial angle and angledot
        assert np.all(j[:, 4:6] == 0.0)


@pytest.fixture(scope="module")
def hs100_tf():
    with open(os.path.join(ROOT, "tests", "golden", "flight_fixtures.json")) as f:
        c = {c["name"]: c for c in json.load(f)["cases"]}["hs100"]
    return c["tf"] * c["params"][11]


@pytest.mark.parametrize("scheme,nt", [(0, 60), (1, 60), (0, 200)])
def test_reference_trim_on_oracle_solutions(coracle, hs100_tf, scheme, nt):
    """The trim on nominal C-oracle solutions, to tol = 1e-12 (a condition of 1e-10 in the scaled speed^2 is still 0.03 m of
    periapsis): converged within 6 rounds, the flown apsides are the NLP's own to 1e-3 m, |u| <= 1, saturated controls untouched;
    backward Euler at nt = 200 lands within 0.02 s of the Hermite-Simpson t_f (untrimmed 1.2 s away; seen 0.004 s).
    The oracle solves to 1e-10: the NLP's own last node sits off its target orbit by the slack the interior-point method
    leaves on the two terminal inequalities, 1.5e-3 m of periapsis at tol 1e-9 and 1.5e-4 m at 1e-10; the trim aims at the
    target itself (conditions = 0), so that slack is the floor of this comparison."""
    p16 = coracle.pack_params(Params())
    r = coracle.solve_batch(p16[None], nt, 300, 1e-10, want_blob=True, scheme=scheme)
    assert r["status"][0] == 0
    blob = r["blob"][0]
    K = nt - 1
    zs, u0, tf0 = fr.blob_parts(blob, nt)
    t = jr.trim(p16, blob, nt, 0, 0, 0, rounds=6, tol=1e-12)
    s = t["summary"]
    print(f"scheme {scheme} nt {nt}: |c| per round {['%.2g' % c for c in t['history']]}, t_f {tf0 * p16[11]:.4f} -> {t['tf'] * p16[11]:.4f} s, "
          f"free {int(s[6])} of {K}, flown apsides {s[7]:.3f} / {s[8]:.3f} m")
    assert s[0] == 0 and s[1] <= 6 and s[2] <= 1e-12
    pn, an = fr.apsides(p16, *zs[-1, :4])
    assert abs(s[7] - pn) <= 1e-3 and abs(s[8] - an) <= 1e-3
    assert np.abs(t["u"]).max() <= 1.0
    sat = np.abs(u0) >= 0.999
    assert np.array_equal(t["u"][sat], u0[sat])
    f = fr.fly(p16, t["blob"], nt, want_local=True)
    assert np.abs(f["local"]).max() <= 1e-12 and abs(f["summary"][2] - s[7]) <= 1e-6
    if nt == 200:
        print(f"  t_f trimmed {t['tf'] * p16[11]:.4f} s, Hermite-Simpson N = 100 {hs100_tf:.4f} s, untrimmed {tf0 * p16[11]:.4f} s")
        assert abs(t["tf"] * p16[11] - hs100_tf) < 0.02


def test_exports_and_argument_checks():
    """The built library exports both entry points, the package both functions, and every argument error returns -1 before any
    device work (this runs without a GPU)."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib, build
    build.build()
    L = _lib.load()
    assert hasattr(L, "ascent_flight_jacobian") and hasattr(L, "ascent_trim_batch")
    assert callable(A.flight_jacobian) and callable(A.trim_batch) and A.FlightJacobian and A.TrimResult
    nt, K, B = 18, 17, 2
    P = np.tile(np.asarray(A.AscentParams().as_row()).reshape(1, 16), (B, 1))
    blob, jac, ju = np.zeros((21 * K + 10, B)), np.zeros((9, 24, B)), np.zeros((9, K, B))
    out, summ = np.zeros_like(blob), np.zeros((10, B))
    pp, bp, jp, up, op, sp = (a.ctypes.data_as(C.c_void_p) for a in (P, blob, jac, ju, out, summ))

    def opts(**kw):
        d = dict(n_nodes=nt, scheme=0, max_iter=0, warm_start=0, tol=1.0, mu_init=0.0)
        d.update(kw)
        return _lib.AscentOptsC(**d)

    def jacobian(p=pp, batch=B, o=None, b=bp, m=0, j=jp, u=up):
        return L.ascent_flight_jacobian(p, batch, C.byref(o) if o is not None else C.byref(opts()), b, m, j, u, 0, None, 0)

    def trim(p=pp, batch=B, o=None, b=bp, m=0, rounds=0, tol=0.0, out_=op, s=sp):
        return L.ascent_trim_batch(p, batch, C.byref(o) if o is not None else C.byref(opts()), b, m, rounds, tol, out_, s, 0, None, 0)

    assert jacobian(p=None) == -1 and jacobian(b=None) == -1 and jacobian(j=None) == -1 and jacobian(batch=0) == -1
    assert L.ascent_flight_jacobian(pp, B, None, bp, 0, jp, up, 0, None, 0) == -1
    assert jacobian(m=-1) == -1 and jacobian(m=4097) == -1
    assert trim(p=None) == -1 and trim(b=None) == -1 and trim(out_=None) == -1 and trim(s=None) == -1 and trim(batch=0) == -1
    assert L.ascent_trim_batch(pp, B, None, bp, 0, 0, 0.0, op, sp, 0, None, 0) == -1
    assert trim(m=-1) == -1 and trim(m=4097) == -1 and trim(rounds=33) == -1 and trim(rounds=-1) == -1
    assert b"rounds" in L.ascent_strerror(-1)
    for call in (jacobian, trim):
        assert call(o=opts(terminal=2)) == -1
        assert b"terminal 2" in L.ascent_strerror(-1)
        # what ascent_fly_batch refuses
        for bad in (opts(n_nodes=2), opts(scheme=3), opts(formulation=2), opts(formulation=1, scheme=1), opts(terminal=3),
                    opts(coarse_nodes=1), opts(solver_path=3), opts(move_penalty=2), opts(formulation=1, solver_path=4),
                    opts(formulation=1, scheme=2)):
            assert call(o=bad) == -1
    P0 = P.copy()
    P0[:, 15] = 0.0            # move_penalty = 1 needs dcost > 0 on host-resident parameter sets
    p0 = P0.ctypes.data_as(C.c_void_p)
    assert jacobian(p=p0, o=opts(move_penalty=1)) == -1 and trim(p=p0, o=opts(move_penalty=1)) == -1
    with pytest.raises(ValueError):
        A.flight_jacobian(P, np.zeros((21 * K + 9, B)), nt)
    with pytest.raises(ValueError):
        A.trim_batch(P, np.zeros((21 * K + 10, B + 1)), nt)


def test_predict_and_sigma():
    """FlightJacobian.predict is the first-order change, sigma the root-sum-square of independent errors"""
    from lunar_module_ascent_trajectory_optimiser_amd import FlightJacobian
    rng = np.random.default_rng(0)
    J = FlightJacobian(rng.standard_normal((2, 9, 7)), rng.standard_normal((2, 9, 16)), rng.standard_normal((2, 9)),
                       rng.standard_normal((2, 9, 5)))
    dp, du = rng.standard_normal(16), rng.standard_normal((2, 5))
    want = J.dparams @ dp + J.dtf * 0.5 + np.einsum("bqk,bk->bq", J.dcontrols, du)
    assert np.allclose(J.predict(dparams=dp, dtf=0.5, dcontrols=du), want, rtol=1e-14)
    sp = np.abs(dp)
    want = np.sqrt(((J.dparams * sp) ** 2).sum(axis=2) + ((J.dcontrols * 0.01) ** 2).sum(axis=2))
    assert np.allclose(J.sigma(param_sigma=sp, control_sigma=0.01), want, rtol=1e-14)
    with pytest.raises(ValueError):
        FlightJacobian(J.dz0, J.dparams, J.dtf, None).predict(dcontrols=du[0])
