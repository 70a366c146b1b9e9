"""Device time of the Monte Carlo dispersion (ascent_disperse_batch) on the bench sweep, 4096 x N = 200, backward Euler,
automatic substeps, at samples = 16, 256 and 1024, beside the only alternative without it: the blob tiled `--tile` (16) times
and flown as 4096 x 16 problems by ascent_fly_batch (summary only), in the same run.  HIP events on torch's stream, device
pointers: every call only enqueues.  Warm (three untimed calls), median of --reps calls with min .. max.  Also the bytes each
route allocates, and the physics table: the trimmed nominal solution under 50 N of thrust and 1e-3 per control step, 1024
samples, Monte Carlo against linear 1-sigma of the flown apsides.
Prints one JSON object; --out FILE writes it too.  Per-kernel times of one call:
`rocprofv3 --kernel-trace --stats -- python scripts/dispersion_timing.py --only disperse --samples 16 --reps 1`."""
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
                                                              disperse_batch, flight_jacobian, _lib)
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--samples", type=int, nargs="*", default=[16, 256, 1024])
    ap.add_argument("--tile", type=int, default=16)
    ap.add_argument("--only", choices=("disperse", "tiled", "table"), help="only this part (for a profiler run)")
    a = ap.parse_args()
    L = _lib.load()
    nt, K = 200, 199
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, nt=nt)
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
        sig = torch.zeros((24, B), **dev)
        sig[7 + 3] = 50.0
        sig_u = torch.full((K, B), 1e-3, **dev)
        stats = torch.empty((82, B), **dev)
        us, ws = {}, {}
        if a.only != "tiled":
            for S in a.samples:
                xi = torch.from_numpy(np.random.default_rng(0).standard_normal((24 + K, S))).cuda()
                us[f"disperse_{S}"] = timed(lambda: L.ascent_disperse_batch(pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, S, xi.data_ptr(),
                                                                            sig.data_ptr(), sig_u.data_ptr(), stats.data_ptr(), None, 0, stream, 1))
                us[f"disperse_{S}"]["us_per_flight"] = round(us[f"disperse_{S}"]["median"] / (B * S), 5)
                # inputs the caller stages (xi, sigma, sigma_u) + the library's workspace (trajectory, f_fly's rows, partial records)
                ws[f"disperse_{S}"] = 8 * ((24 + K) * S + (24 + K) * B + (10 * nt + 10 + 73 * ((S + 255) // 256)) * B)
                s = stats.cpu().numpy()
                us[f"disperse_{S}"]["valid_samples"] = [int(s[0].min()), int(s[0].max())]
        if a.only != "disperse":
            T = a.tile
            pt_t, blob_t = pt.repeat(T, 1).contiguous(), blob.repeat(1, T).contiguous()
            fsum = torch.empty((10, B * T), **dev)
            us[f"tiled_fly_{T}"] = timed(lambda: L.ascent_fly_batch(pt_t.data_ptr(), B * T, C.byref(o), blob_t.data_ptr(), 0, None, None,
                                                                    fsum.data_ptr(), 0, stream, 1))
            us[f"tiled_fly_{T}"]["us_per_flight"] = round(us[f"tiled_fly_{T}"]["median"] / (B * T), 5)
            ws[f"tiled_fly_{T}"] = 8 * ((21 * K + 10) + 16 + 10) * B * T          # the tiled blob, parameters and summary
            if f"disperse_{T}" in us:
                res["disperse_vs_tiled_at_equal_work"] = round(us[f"disperse_{T}"]["median"] / us[f"tiled_fly_{T}"]["median"], 4)
        res.update(us=us, bytes=ws)
    if a.only in (None, "table"):
        P = AscentParams(tf_ub=1.2).as_row()[None].copy()
        r = solve_batch(P, nt, want_blob=True)
        t = trim_batch(P, r.blob, nt)
        thrust = np.zeros(16)
        thrust[3] = 50.0
        d = disperse_batch(P, t.blob, nt, param_sigma=thrust, control_sigma=1e-3, samples=1024)
        lin = np.sqrt(np.diagonal(d.linear_covariance(flight_jacobian(P, t.blob, nt)), axis1=1, axis2=2))
        res["trimmed_nominal_50N_1e-3_1024"] = {
            name: dict(nominal_m=float(d.nominal[0, q]), monte_carlo_sigma_m=float(d.std[0, q]), linear_sigma_m=float(lin[0, q]),
                       mean_shift_m=float(d.mean[0, q] - d.nominal[0, q]), min_m=float(d.min[0, q]), max_m=float(d.max[0, q]))
            for name, q in (("periapsis_alt", 7), ("apoapsis_alt", 8))}
        res["trimmed_nominal_50N_1e-3_1024"]["valid_samples"] = int(d.n_valid[0])
        res["trimmed_nominal_50N_1e-3_1024"]["trim_status"] = int(t.status[0])
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
