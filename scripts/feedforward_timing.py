"""Device time of the guidance feed-forward on the bench sweep, 4096 x N = 200, backward Euler, automatic substeps:
ascent_guidance_feedforward beside ascent_guidance_gains (gains only, and with the closed-loop Jacobian -- the feed-forward call
then also with the navigation block), and ascent_disperse_navigated_batch (feed-forward, navigation biases and a knowledge error
all on) beside ascent_disperse_guided_batch at samples = 16, 256 and 1024 with the gains just computed.  HIP events on torch's
stream, device pointers: every call only enqueues.  Warm (three untimed calls), median of --reps calls with min .. max, all
from one process.  Also the physics table: the trimmed nominal solution under 50 N of thrust and 1e-3 per control step, 1024
samples, feedback only / feed-forward with the thrust known / known to 10 N with a navigation bias (weights 1e12, 1, 1;
stretch_max 0.5 and 2).
Prints one JSON object; --out FILE writes it too.  Per-kernel times of one call:
`rocprofv3 --kernel-trace --stats -- python scripts/feedforward_timing.py --only gains --reps 1`."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAV_BIAS = (1e-3, 1e-3, 1e-6, 1e-6, 0.0, 0.0, 0.0)      # scaled units (r_peri, r_peri per second): 17.7 m and 1.8 cm/s per axis on the nominal problem


def main():
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import (AscentParams, sweep_isp_drymass, solve_batch, solve_batch_torch, trim_batch,
                                                              disperse_batch, guidance_gains, _lib)
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--samples", type=int, nargs="*", default=[16, 256, 1024])
    ap.add_argument("--weight", type=float, default=1e6, help="q of the three conditions in the timed calls")
    ap.add_argument("--only", choices=("gains", "disperse", "table"), help="only this part (for a profiler run)")
    a = ap.parse_args()
    L = _lib.load()
    nt, K = 200, 199
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, nt=nt, weight=a.weight)
    dev = dict(dtype=torch.float64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = _opts(nt, 0, 1.0, 0, 0.0)

    def timed(call):
        ts = []
        for _ in range(a.reps + 3):
            e0.record()
            _lib.check(call())
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts = np.array(ts[3:])
        return dict(median=round(float(np.median(ts)), 1), min=round(float(ts.min()), 1), max=round(float(ts.max()), 1))

    if a.only != "table":
        sw = sweep_isp_drymass()
        B = sw.shape[0]
        pt = torch.from_numpy(np.ascontiguousarray(sw)).cuda()
        out = solve_batch_torch(pt, nt, sync=True, want_traj=False, want_blob=True)
        blob = out["blob"]
        res.update(batch=B, converged=int((out["status"] == 0).sum().item()))
        w = torch.tensor([[a.weight] * 3 + [1.0, 1.0, 0.5]] * B, **dev).T.contiguous()
        d = torch.zeros((16, B), **dev)
        d[3] = 1.0                               # e_Ft, known exactly: the knowledge row is the direction
        gu, gt, gs = torch.empty((7, K, B), **dev), torch.empty((7, B), **dev), torch.empty((7, B), **dev)
        fu, ft = torch.empty((K, B), **dev), torch.empty((B,), **dev)
        jac, jac_u, jac_n = torch.empty((9, 24, B), **dev), torch.empty((9, K, B), **dev), torch.empty((9, 8, B), **dev)
        us = {}
        gains = lambda j, ju: L.ascent_guidance_gains(pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, w.data_ptr(), gu.data_ptr(), gt.data_ptr(),
                                                      gs.data_ptr(), j, ju, 0, stream, 1)
        ffwd = lambda j, ju, jn: L.ascent_guidance_feedforward(pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, w.data_ptr(), d.data_ptr(),
                                                               d.data_ptr(), gu.data_ptr(), gt.data_ptr(), fu.data_ptr(), ft.data_ptr(),
                                                               gs.data_ptr(), j, ju, jn, 0, stream, 1)
        if a.only != "disperse":
            us["guidance_gains"] = timed(lambda: gains(None, None))
            us["guidance_feedforward"] = timed(lambda: ffwd(None, None, None))
            us["guidance_gains_with_jacobian"] = timed(lambda: gains(jac.data_ptr(), jac_u.data_ptr()))
            us["guidance_feedforward_with_jacobian"] = timed(lambda: ffwd(jac.data_ptr(), jac_u.data_ptr(), jac_n.data_ptr()))
            res["feedforward_vs_gains"] = round(us["guidance_feedforward"]["median"] / us["guidance_gains"]["median"], 4)
            res["feedforward_vs_gains_with_jacobian"] = round(us["guidance_feedforward_with_jacobian"]["median"] / us["guidance_gains_with_jacobian"]["median"], 4)
            s = gs.cpu().numpy()
            res["gains_status_ok"] = int((s[0] == 0).sum())
        else:
            _lib.check(ffwd(None, None, None))
        if a.only != "gains":
            sig = torch.zeros((24, B), **dev)
            sig[7 + 3] = 50.0
            sig_u = torch.full((K, B), 1e-3, **dev)
            sn = torch.tensor([list(NAV_BIAS) + [10.0]] * B, **dev).T.contiguous()
            stats = torch.empty((82, B), **dev)
            for S in a.samples:
                xi = torch.from_numpy(np.random.default_rng(0).standard_normal((24 + K, S))).cuda()
                xn = torch.from_numpy(np.random.default_rng(1).standard_normal((8, S))).cuda()
                us[f"disperse_guided_{S}"] = timed(lambda: L.ascent_disperse_guided_batch(
                    pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, S, xi.data_ptr(), sig.data_ptr(), sig_u.data_ptr(), gu.data_ptr(), gt.data_ptr(),
                    w[5].data_ptr(), stats.data_ptr(), None, 0, stream, 1))
                us[f"disperse_navigated_{S}"] = timed(lambda: L.ascent_disperse_navigated_batch(
                    pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, S, xi.data_ptr(), sig.data_ptr(), sig_u.data_ptr(), gu.data_ptr(), gt.data_ptr(),
                    w[5].data_ptr(), fu.data_ptr(), ft.data_ptr(), d.data_ptr(), xn.data_ptr(), sn.data_ptr(), stats.data_ptr(), None, 0, stream, 1))
                s = stats.cpu().numpy()
                us[f"disperse_navigated_{S}"]["valid_samples"] = [int(s[0].min()), int(s[0].max())]
                res[f"navigated_vs_guided_{S}"] = round(us[f"disperse_navigated_{S}"]["median"] / us[f"disperse_guided_{S}"]["median"], 4)
        res.update(us=us)
    if a.only in (None, "table"):
        P = AscentParams(tf_ub=1.2).as_row()[None].copy()
        table = {}
        for n in (50, nt):
            r = solve_batch(P, n, want_blob=True)
            t = trim_batch(P, r.blob, n, rounds=8, tol=1e-12)
            thrust = np.zeros(16)
            thrust[3] = 50.0
            kw = dict(param_sigma=thrust, control_sigma=1e-3, samples=1024, keep_samples=True)
            tab = dict(trim_status=int(t.status[0]), nav_bias_sigma_scaled=list(NAV_BIAS), knowledge_sigma_N=10.0)
            for smax in (0.5, 2.0):
                wk = dict(cond_weights=(1e12,) * 3, control_weight=1.0, cutoff_weight=1.0, stretch_max=smax)
                g = guidance_gains(P, t.blob, n, feedforward="Ft", **wk)
                g0 = guidance_gains(P, t.blob, n, want_jacobian=False, **wk)
                runs = dict(feedback_only=disperse_batch(P, t.blob, n, guidance=g0, **kw),
                            feedforward_known=disperse_batch(P, t.blob, n, guidance=g, **kw),
                            feedforward_10N=disperse_batch(P, t.blob, n, guidance=g, knowledge_sigma=10.0, **kw),
                            feedforward_10N_nav_bias=disperse_batch(P, t.blob, n, guidance=g, knowledge_sigma=10.0, nav_sigma=NAV_BIAS, **kw))
                row = {}
                for name, c in runs.items():
                    e = c.effort[0]
                    row[name] = dict(periapsis_sigma_m=float(c.std[0, 7]), apoapsis_sigma_m=float(c.std[0, 8]), valid_samples=int(c.n_valid[0]),
                                     clipped_steps_per_flight=float(e[:, 0].mean()), largest_correction=float(e[:, 1].max()),
                                     largest_stretch=float(np.abs(e[:, 2]).max()))
                c = runs["feedforward_10N_nav_bias"]
                lin = np.sqrt(np.diagonal(c.linear_covariance(g.jacobian, g.jacobian_nav)[0]))
                row["feedforward_10N_nav_bias"].update(linear_periapsis_sigma_m=float(lin[7]), linear_apoapsis_sigma_m=float(lin[8]))
                row.update(gains_status=int(g.status[0]), max_feedforward=float(g.max_feedforward[0]), max_cutoff_feedforward=float(g.max_cutoff_feedforward[0]))
                tab[f"stretch_max_{smax:g}"] = row
            table[f"nt{n}"] = tab
        res["trimmed_nominal_50N_1e-3_1024"] = table
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
