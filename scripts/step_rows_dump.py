"""Developer tool: what solve_batch and the persistent path's Newton-step probe return, as SHA-256 of the raw bytes of every output
array, for comparing two builds of the library bit for bit (p_solve recomputes the node-local step rows
instead of storing them; no result may change).

    python scripts/step_rows_dump.py --out FILE.json              (on the GPU, once in each tree)
    python scripts/step_rows_dump.py --compare PARENT.json CHANGE.json --json profiles/step_rows_parity.json    (anywhere)

Arrays per solve: tf, status, iters, the trajectory and the solution blob.  Cases: the bench's sweep (4096 NLPs, nt = 200) with and
without DCOST; the four row groups of tests/test_gpu_lockstep.py; rows 0-3 at nt = 17 on a single grid; five NLPs at nt = 18, 34
and 66, single grid, four NLPs and one NLP per wavefront (ASCENT_PERSIST_WIDE 0 / 1); the trapezoid, the v1 formulation and
terminal 2 (and the trapezoid with terminal 2) at nt = 34 and 200 in both forms -- every case with and without the move penalty.
The probe: ascent_kkt_step_path on the persistent path at nt = 18 and 34, both forms, move penalty on and off (step and inertia), and
the worst error of its bound-multiplier section against (mu - z_b dx) / dist - z_b in numpy, in ulps of
|mu/dist| + |z_b dx/dist| + |z_b| (the figure behind the bound of tests/test_gpu_step_rows.py)."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOCKSTEP_GROUPS = {"one_retries_three_wait": (2700, 2704), "retries_at_different_rounds": (3508, 3512), "coarse_level_out_of_step": (2800, 2804),
                   "second_wavefront_dead_group": (2700, 2707)}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def probe_ulps(S, blobs, step, mu, nt):
    """worst |dz_b - ((mu - z_b dx) / dist - z_b)| over the bound-multiplier section, in ulps of |mu/dist| + |z_b dx/dist| + |z_b|"""
    K, worst = nt - 1, 0.0
    for b in range(blobs.shape[1]):
        it, st = blobs[:, b], step[:, b]
        z, dz = it[:7 * K].reshape(K, 7), st[:7 * K].reshape(K, 7)
        u, du = it[7 * K:8 * K], st[7 * K:8 * K]
        zb, dzb = it[15 * K:21 * K].reshape(K, 6), st[15 * K:21 * K].reshape(K, 6)
        aub = S[b, 12]
        dist = np.stack([z[:, 4], aub - z[:, 4], z[:, 6], 1.0 - z[:, 6], u + 1.0, 1.0 - u], axis=1)
        dx = np.stack([dz[:, 4], -dz[:, 4], dz[:, 6], -dz[:, 6], du, -du], axis=1)
        ref = (mu[b] - zb * dx) / dist - zb
        scale = np.abs(mu[b] / dist) + np.abs(zb * dx / dist) + np.abs(zb)
        worst = max(worst, float((np.abs(dzb - ref) / np.spacing(scale)).max()))
    return worst


def dump(path):
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from test_terminal_step_reference import MU, blob_of, dw_of, problems
    res, info = {}, {}

    def solve(tag, S, nt, wide=None, **kw):
        if wide is None:
            os.environ.pop("ASCENT_PERSIST_WIDE", None)
        else:
            os.environ["ASCENT_PERSIST_WIDE"] = str(wide)
        r = A.solve_batch(S, nt, tol=1e-9, want_blob=True, **kw)
        for k in ("tf", "status", "iters", "traj", "blob"):
            res[f"{tag}/{k}"] = sha(getattr(r, k))
        pk = {k: v for k, v in kw.items() if k in ("scheme", "formulation", "move_penalty", "terminal")}
        info[tag] = {"path": A.default_path(len(S), nt, **pk), "converged": int((r.status == 0).sum()),
                     "iters_min_max": [int(r.iters.min()), int(r.iters.max())]}
        print(tag, info[tag], flush=True)

    S = A.sweep_isp_drymass(64, 64).copy()
    S[:, 15] = 1e-5
    for mp in (True, False):
        m = "penalty" if mp else "plain"
        solve(f"headline_{m}", S, 200, move_penalty=mp)
        for nt in (18, 34, 66):
            for wide in (0, 1):
                solve(f"nt{nt}_wide{wide}_{m}", S[:5], nt, wide, coarse_nodes=-1, move_penalty=mp)
        solve(f"nt17_single_grid_{m}", S[:4], 17, 0, coarse_nodes=-1, move_penalty=mp)
        for name, kw in (("trapezoid", dict(scheme=1)), ("v1", dict(formulation=1)), ("terminal2", dict(terminal=2)),
                         ("trapezoid_terminal2", dict(scheme=1, terminal=2))):
            for nt in (34, 200):
                for wide in (0, 1):
                    solve(f"{name}_nt{nt}_wide{wide}_{m}", S[:5], nt, wide, move_penalty=mp, **kw)
    for name, (a, b) in LOCKSTEP_GROUPS.items():
        solve(f"lockstep_{name}", S[a:b], 200, 0, move_penalty=True)
    P = problems()
    worst = 0.0
    for nt in (18, 34):
        blobs = np.stack([blob_of(nt, 0, b) for b in range(len(P))], axis=1)
        dw = np.array([dw_of(nt, b) for b in range(len(P))])
        for mp in (True, False):
            for wide in (0, 1):
                os.environ["ASCENT_PERSIST_WIDE"] = str(wide)
                step, inertia = A.kkt_step(P, blobs, MU.copy(), dw, nt, path="persist", move_penalty=mp)
                tag = f"probe_nt{nt}_wide{wide}_{'penalty' if mp else 'plain'}"
                res[f"{tag}/step"], res[f"{tag}/inertia"] = sha(step), sha(inertia)
                u = probe_ulps(P, blobs, step, MU, nt)
                info[tag] = {"inertia": inertia.tolist(), "bound_multiplier_ulps": u}
                worst = max(worst, u)
                print(tag, info[tag], flush=True)
    with open(path, "w") as f:
        json.dump({"arrays": res, "info": info, "probe_worst_ulps": worst}, f, indent=1)
    print(f"{len(res)} arrays -> {path}")


def compare(a, b, json_path):
    x, y = json.load(open(a)), json.load(open(b))
    names = sorted(set(x["arrays"]) | set(y["arrays"]))
    bad = [n for n in names if x["arrays"].get(n) != y["arrays"].get(n)]
    groups = {}
    for n in names:
        g = groups.setdefault(n.split("/")[0], [0, 0])
        g[0] += 1
        g[1] += n in bad
    doc = {"_comment": "scripts/step_rows_dump.py --compare: SHA-256 of the bytes of tf, status, iters, trajectory and solution blob of every "
                       "solve, and of step and inertia of every probe, the parent commit's library against this tree's, both run on the same "
                       "MI355X; per case [arrays, differing]; info: the parent's run.  probe_worst_ulps: worst error of the probe's "
                       "bound-multiplier steps against numpy in ulps of |mu/dist| + |z_b dx/dist| + |z_b|, parent and change; "
                       "probe_ulp_bound = 4 x the parent's, the bound of tests/test_gpu_step_rows.py",
           "arrays": len(names), "differ": len(bad), "differing": bad,
           "probe_worst_ulps": {"parent": x["probe_worst_ulps"], "change": y["probe_worst_ulps"]}, "probe_ulp_bound": 4.0 * x["probe_worst_ulps"],
           "cases": groups, "info": x["info"]}
    if json_path:
        with open(json_path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(f"{len(names)} arrays, {len(bad)} differ; probe ulps parent {x['probe_worst_ulps']} change {y['probe_worst_ulps']}")
    for n in bad:
        print("  differ:", n)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.json))
    dump(a.out)
