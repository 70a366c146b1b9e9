#!/usr/bin/env python3
"""Generates tests/golden/flight_fixtures.json: what the CPU oracles' solutions reach when their control is flown with an
accurate integrator (tests/flight_reference.py, DOP853 at rtol 1e-13 restarted at every node, control held over each step).

Cases (Apollo 11 parameters, terminal 0): backward Euler and trapezoid at N = 200 and 400 from the C oracle (tol 1e-9),
Hermite-Simpson at N = 50 and 100 from the generalised numpy oracle (tol 1e-10, as scripts/make_hs_fixtures.py), and
formulation 1 with the v1 script's parameters at N = 200 from the C oracle.  Each case holds the parameters, the options,
t_f and the summary rows of include/ascent.h: ascent_fly_batch; the solutions themselves are not stored (a test solves the
same NLP again and flies its own solution).   Run on the CPU box:  python scripts/make_flight_fixtures.py
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import flight_reference as fr  # noqa: E402
from oracle import c_oracle  # noqa: E402
from oracle.ascent_general import GeneralNLP  # noqa: E402
from oracle.ascent_numpy import Params, solve_ip, v1_params  # noqa: E402


def c_case(P, nt, scheme, formulation):
    p16 = c_oracle.pack_params(P)
    r = c_oracle.solve_batch(p16[None], nt, 300, 1e-9, want_blob=True, scheme=scheme, formulation=formulation)
    assert r["status"][0] == 0, r["status"]
    return p16, r["blob"][0], "C oracle, tol 1e-9"


def general_case(P, nt, scheme):
    K = nt - 1
    nlp = GeneralNLP(P, ((K, "burn"),), scheme, terminal="reference")
    v, lam, info = solve_ip(nlp, tol=1e-10, max_iter=500)
    assert info["status"] == "converged", info
    W = v[:8 * K].reshape(K, 8)
    return c_oracle.pack_params(P), fr.make_blob(W[:, :7], W[:, 7], v[nlp.itf]), "generalised numpy oracle, tol 1e-10"


def main():
    c_oracle.build()
    cases = []
    todo = [("be200", Params(), 200, 0, 0), ("be400", Params(), 400, 0, 0), ("trap200", Params(), 200, 1, 0),
            ("trap400", Params(), 400, 1, 0), ("hs50", Params(), 50, 2, 0), ("hs100", Params(), 100, 2, 0),
            ("v1_be200", v1_params(), 200, 0, 1)]
    for name, P, nt, scheme, form in todo:
        t = time.time()
        p16, blob, src = general_case(P, nt, scheme) if scheme == 2 else c_case(P, nt, scheme, form)
        f = fr.fly(p16, blob, nt, formulation=form, integrator="dop853")
        s = f["summary"]
        cases.append(dict(name=name, params=[float(x) for x in p16], nt=nt, scheme=scheme, formulation=form, terminal=0,
                          source=src, tf=float(blob[21 * (nt - 1)]), final_time=float(blob[21 * (nt - 1)] * p16[11]),
                          summary={k: float(x) for k, x in zip(fr.SUMMARY, s)}))
        print(f"{name}: t_f = {cases[-1]['final_time']:.5f} s, miss {s[0]:.6g} m {s[1]:.6g} m/s, flown orbit {s[2]:.1f} / {s[3]:.1f} m, "
              f"NLP's {s[4]:.1f} / {s[5]:.1f} m, max local {s[6]:.4g} m at step {int(s[8])}  ({time.time() - t:.1f} s)", flush=True)
    out = {"_comment": "made by scripts/make_flight_fixtures.py: CPU oracles' solutions flown by tests/flight_reference.py (DOP853, "
                       "rtol 1e-13, atol 1e-15, restarted at every node); summary rows as include/ascent.h: ascent_fly_batch "
                       "(substeps = the rule's m, not used by DOP853)", "cases": cases}
    path = os.path.join(ROOT, "tests", "golden", "flight_fixtures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
