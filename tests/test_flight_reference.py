"""The CPU reference of the flight verification (tests/flight_reference.py) checked against itself and against the committed
fixtures (tests/golden/flight_fixtures.json, scripts/make_flight_fixtures.py): its RK4 against its DOP853, the order of the
miss of every scheme, and an exact synthetic blob.  No GPU."""
import json
import os

import numpy as np
import pytest

import flight_reference as fr
from oracle.ascent_numpy import Params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixtures():
    with open(os.path.join(ROOT, "tests", "golden", "flight_fixtures.json")) as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def _oracle_blob(coracle, nt, scheme):
    p16 = coracle.pack_params(Params())
    if scheme == 2:       # the generalised numpy oracle, as scripts/make_flight_fixtures.py
        from oracle.ascent_general import GeneralNLP
        from oracle.ascent_numpy import solve_ip
        K = nt - 1
        nlp = GeneralNLP(Params(), ((K, "burn"),), 2, terminal="reference")
        v, lam, info = solve_ip(nlp, tol=1e-10, max_iter=500)
        assert info["status"] == "converged", info
        W = v[:8 * K].reshape(K, 8)
        return p16, fr.make_blob(W[:, :7], W[:, 7], v[nlp.itf])
    r = coracle.solve_batch(p16[None], nt, 300, 1e-9, want_blob=True, scheme=scheme)
    assert r["status"][0] == 0
    return p16, r["blob"][0]


@pytest.mark.parametrize("nt", [50, 200, 2000])
def test_rk4_against_dop853(coracle, nt):
    """RK4 with the automatic substeps (<= 0.5 s) against DOP853 at rtol 1e-13 on nominal trapezoid solutions: end state within
    1e-4 m and 1e-6 m/s.  Seen with this rule: 1.75e-5 m at 0.493 s (N = 50), 7.9e-6 m at 0.437 s (N = 200), 4.9e-7 m at 0.218 s
    (N = 2000), growing as substep^4; the bound is that law at 0.5 s with a factor 5."""
    p16, blob = _oracle_blob(coracle, nt, 1)
    a = fr.fly(p16, blob, nt, integrator="rk4", want_local=False)
    b = fr.fly(p16, blob, nt, integrator="dop853", want_local=False)
    S = p16[9]
    dt = blob[21 * (nt - 1)] * p16[11] / (nt - 1)
    assert a["m"] == max(1, int(np.ceil(dt / 0.5))) and dt / a["m"] <= 0.5
    dpos = S * np.hypot(*(a["traj"][:2, -1] - b["traj"][:2, -1]))
    dvel = S * np.hypot(*(a["traj"][2:4, -1] - b["traj"][2:4, -1]))
    print(f"nt={nt}: m={a['m']} substep {dt / a['m']:.3f} s, RK4 - DOP853 at the last node {dpos:.3g} m, {dvel:.3g} m/s")
    assert dpos <= 1e-4 and dvel <= 1e-6


@pytest.mark.parametrize("names,lo,hi", [(("be200", "be400"), 1.9, 2.1), (("trap200", "trap400"), 3.6, 4.4),
                                         (("hs50", "hs100"), 13.0, 19.0)])
def test_order_of_the_miss(fixtures, coracle, names, lo, hi):
    """Halving the step divides the position miss by 2^p, p the order of the scheme: backward Euler 1, trapezoid 2,
    Hermite-Simpson 4 (intervals: 2^p with room for the next term of the expansion).  Every case is solved again by the oracle
    that made its fixture and flown with RK4; the result must be the fixture's (DOP853) to the RK4 truncation bound."""
    coarse, fine = fixtures[names[0]], fixtures[names[1]]
    miss = []
    for c in (coarse, fine):
        p16, blob = _oracle_blob(coracle, c["nt"], c["scheme"])
        assert np.array_equal(p16, c["params"]) and abs(blob[21 * (c["nt"] - 1)] - c["tf"]) * p16[11] <= 1e-7
        s = fr.fly(p16, blob, c["nt"], integrator="rk4", want_local=False)["summary"]
        assert abs(s[0] - c["summary"]["miss_pos_m"]) <= 1e-4 and abs(s[1] - c["summary"]["miss_vel_ms"]) <= 1e-6
        miss.append(s[0])
    ratio = miss[0] / miss[1]
    print(f"{names}: miss {miss[0]:.6g} m -> {miss[1]:.6g} m, ratio {ratio:.4f}")
    assert lo <= ratio <= hi


def test_exact_blob_has_no_error():
    """A blob whose states are a DOP853 flight of an arbitrary bounded control: under RK4 with m = 16 the local errors and the miss
    are the integrator's own error.  N = 200, t_f = 0.9 T: substeps of 0.13 s, by the substep^4 law 1.9e-5 m (0.137 / 0.547)^4 =
    7e-8 m = 4e-12 scaled, far below the 1e-9 asked."""
    nt = 200
    p16 = np.array([getattr(Params(), f) for f in fr.FIELDS])
    blob = fr.synthetic_exact_blob(p16, nt, tf=0.9, seed=3)
    r = fr.fly(p16, blob, nt, substeps=16)
    zs, us, tf = fr.blob_parts(blob, nt)
    assert r["m"] == 16 and np.abs(us).max() <= 1.0 and np.abs(zs[-1, :2]).max() > 1.0       # it does go somewhere
    miss = np.abs(r["traj"][[0, 1, 2, 3, 6, 7, 9], -1] - zs[-1]).max()
    print(f"exact blob: max |local error| {np.abs(r['local']).max():.3g}, miss {miss:.3g} (scaled)")
    assert np.abs(r["local"]).max() <= 1e-9 and miss <= 1e-9
    assert r["summary"][0] <= 1e-9 * p16[9] and r["summary"][6] <= 1e-9 * p16[9]
