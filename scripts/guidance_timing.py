"""Device time of the closed-loop guidance on the bench sweep, 4096 x N = 200, backward Euler, automatic substeps:
ascent_guidance_gains (with the closed-loop Jacobian) beside ascent_flight_jacobian -- the same record evaluation under a larger
sweep --, and ascent_disperse_guided_batch beside ascent_disperse_batch at samples = 16, 256 and 1024 with the gains just
computed.  HIP events on torch's stream, device pointers: every call only enqueues.  Warm (three untimed calls), median of
--reps calls with min .. max.  Also the physics table: the trimmed nominal solution under 50 N of thrust and 1e-3 per control
step, 1024 samples, open loop against closed loop (weights 1e12, 1, 1; stretch_max 0.5 and 2).
Prints one JSON object; --out FILE writes it too.  Per-kernel times of one call:
`rocprofv3 --kernel-trace --stats -- python scripts/guidance_timing.py --only gains --reps 1`."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
        gu, gt, gs = torch.empty((7, K, B), **dev), torch.empty((7, B), **dev), torch.empty((5, B), **dev)
        jac, jac_u = torch.empty((9, 24, B), **dev), torch.empty((9, K, B), **dev)
        us = {}
        gains = lambda j, ju: L.ascent_guidance_gains(pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, w.data_ptr(), gu.data_ptr(), gt.data_ptr(),
                                                      gs.data_ptr(), j, ju, 0, stream, 1)
        if a.only != "disperse":
            us["flight_jacobian"] = timed(lambda: L.ascent_flight_jacobian(pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, jac.data_ptr(),
                                                                           jac_u.data_ptr(), 0, stream, 1))
            us["guidance_gains"] = timed(lambda: gains(None, None))
            us["guidance_gains_with_jacobian"] = timed(lambda: gains(jac.data_ptr(), jac_u.data_ptr()))
            res["gains_with_jacobian_vs_flight_jacobian"] = round(us["guidance_gains_with_jacobian"]["median"] / us["flight_jacobian"]["median"], 4)
            s = gs.cpu().numpy()
            res["gains_status_ok"] = int((s[0] == 0).sum())
        else:
            _lib.check(gains(None, None))
        if a.only != "gains":
            sig = torch.zeros((24, B), **dev)
            sig[7 + 3] = 50.0
            sig_u = torch.full((K, B), 1e-3, **dev)
            stats = torch.empty((82, B), **dev)
            for S in a.samples:
                xi = torch.from_numpy(np.random.default_rng(0).standard_normal((24 + K, S))).cuda()
                us[f"disperse_{S}"] = timed(lambda: L.ascent_disperse_batch(pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, S, xi.data_ptr(),
                                                                            sig.data_ptr(), sig_u.data_ptr(), stats.data_ptr(), None, 0, stream, 1))
                us[f"disperse_guided_{S}"] = timed(lambda: L.ascent_disperse_guided_batch(
                    pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, S, xi.data_ptr(), sig.data_ptr(), sig_u.data_ptr(), gu.data_ptr(), gt.data_ptr(),
                    w[5].data_ptr(), stats.data_ptr(), None, 0, stream, 1))
                s = stats.cpu().numpy()
                us[f"disperse_guided_{S}"]["valid_samples"] = [int(s[0].min()), int(s[0].max())]
                res[f"guided_vs_open_loop_{S}"] = round(us[f"disperse_guided_{S}"]["median"] / us[f"disperse_{S}"]["median"], 4)
        res.update(us=us)
    if a.only in (None, "table"):
        P = AscentParams(tf_ub=1.2).as_row()[None].copy()
        r = solve_batch(P, nt, want_blob=True)
        t = trim_batch(P, r.blob, nt, rounds=8, tol=1e-12)
        thrust = np.zeros(16)
        thrust[3] = 50.0
        kw = dict(param_sigma=thrust, control_sigma=1e-3, samples=1024)
        op = disperse_batch(P, t.blob, nt, **kw)
        table = dict(valid_open_loop=int(op.n_valid[0]), trim_status=int(t.status[0]), last_step_seconds=float(t.tf[0] * P[0, 11] / K))
        # the cutoff stretches the last step only (2.2 s at N = 200): at stretch_max = 0.5 it sits on its bound, 2 covers the burn-time dispersion
        for smax in (0.5, 2.0):
            g = guidance_gains(P, t.blob, nt, cond_weights=(1e12,) * 3, control_weight=1.0, cutoff_weight=1.0, stretch_max=smax)
            cl = disperse_batch(P, t.blob, nt, guidance=g, keep_samples=True, **kw)
            lin = g.jacobian.sigma(param_sigma=thrust, control_sigma=1e-3)
            e = cl.effort[0]
            row = {name: dict(nominal_m=float(cl.nominal[0, q]), open_loop_sigma_m=float(op.std[0, q]), closed_loop_sigma_m=float(cl.std[0, q]),
                              closed_loop_linear_sigma_m=float(lin[0, q]), closed_loop_min_m=float(cl.min[0, q]), closed_loop_max_m=float(cl.max[0, q]))
                   for name, q in (("periapsis_alt", 7), ("apoapsis_alt", 8))}
            row.update(valid_samples=int(cl.n_valid[0]), gains_status=int(g.status[0]), max_gain=float(g.max_gain[0]),
                       max_cutoff_gain=float(g.max_cutoff_gain[0]), clipped_steps_per_flight=float(e[:, 0].mean()), largest_feedback=float(e[:, 1].max()),
                       stretch_sigma=float(e[:, 2].std()), largest_stretch=float(np.abs(e[:, 2]).max()))
            table[f"stretch_max_{smax:g}"] = row
        res["trimmed_nominal_50N_1e-3_1024"] = table
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
