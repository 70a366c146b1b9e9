"""Device time of the flight Jacobian (ascent_flight_jacobian) and the trim (ascent_trim_batch) beside the solve whose blob
they read and the ascent_fly_batch of the same build.  HIP events on torch's stream, device pointers: every call only enqueues.
The condition to report: the Jacobian call must cost less than the 2 (K + 17) calls of ascent_fly_batch that central
differences over the 16 parameters, t_f and the K controls would take -- `jacobian_vs_differences` is that ratio, from the
medians of the same run.
Cases: the bench sweep 4096 x N = 200 (backward Euler) and one NLP at N = 2000 (Hermite-Simpson).
Warm (three untimed calls), median of --reps calls.  Prints one JSON object; --out FILE writes it too.  Per-kernel times of
one trim call: `rocprofv3 --kernel-trace --stats -- python scripts/trim_timing.py --case NAME --only trim --reps 1`."""
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
    from lunar_module_ascent_trajectory_optimiser_amd import AscentParams, sweep_isp_drymass, solve_batch_torch, _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--case", help="only this case")
    ap.add_argument("--only", choices=("fly", "jacobian", "trim"), help="only this entry point (for a profiler run)")
    a = ap.parse_args()
    L = _lib.load()
    sw = sweep_isp_drymass()
    nom = AscentParams(tf_ub=1.2).as_row()
    cases = [("sweep_4096_n200_backward_euler", sw, 200, 0), ("single_n2000_hermite_simpson", nom[None].copy(), 2000, 2)]
    if a.case:
        cases = [c for c in cases if c[0] == a.case]
        assert cases, a.case
    res = {}
    for name, P, nt, scheme in cases:
        pt = torch.from_numpy(np.ascontiguousarray(P)).cuda()
        B, K = P.shape[0], nt - 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kw = dict(want_traj=False, want_blob=True, scheme=scheme, tol=1e-10 if scheme == 2 else 1e-9, max_iter=500)
        out = solve_batch_torch(pt, nt, sync=True, **kw)
        ts = []
        for _ in range(5):
            e0.record()
            solve_batch_torch(pt, nt, out=out, **kw)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        solve_ms = float(np.median(ts[1:]))
        blob = out["blob"]
        dev = dict(dtype=torch.float64, device="cuda")
        traj, loc, fsum = torch.empty((10, nt, B), **dev), torch.empty((K, 7, B), **dev), torch.empty((10, B), **dev)
        jac, jac_u = torch.empty((9, 24, B), **dev), torch.empty((9, K, B), **dev)
        tblob, tsum = torch.empty_like(blob), torch.empty((10, B), **dev)
        o = _opts(nt, 0, 1.0, 0, 0.0, scheme)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        calls = dict(
            fly=lambda: L.ascent_fly_batch(pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, traj.data_ptr(), loc.data_ptr(), fsum.data_ptr(),
                                           0, stream, 1),
            jacobian=lambda: L.ascent_flight_jacobian(pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, jac.data_ptr(), jac_u.data_ptr(), 0,
                                                      stream, 1),
            trim=lambda: L.ascent_trim_batch(pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, 0, 0.0, tblob.data_ptr(), tsum.data_ptr(), 0,
                                             stream, 1))
        us = {}
        for what, call in calls.items():
            if a.only and what != a.only:
                continue
            ts = []
            for _ in range(a.reps + 3):
                e0.record()
                _lib.check(call())
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            ts = np.array(ts[3:])
            us[what] = dict(median=round(float(np.median(ts)), 1), min=round(float(ts.min()), 1), max=round(float(ts.max()), 1))
        r = dict(batch=B, nt=nt, scheme=scheme, converged=int((out["status"] == 0).sum().item()), solve_ms=round(solve_ms, 3), us=us)
        if "fly" in us and "jacobian" in us:
            r["differences_us"] = round(2 * (K + 17) * us["fly"]["median"], 1)
            r["jacobian_vs_differences"] = round(us["jacobian"]["median"] / r["differences_us"], 5)
            r["jacobian_share_of_solve"] = round(us["jacobian"]["median"] / (solve_ms * 1e3), 4)
        if "trim" in us:
            s = tsum.cpu().numpy()
            r["trim_share_of_solve"] = round(us["trim"]["median"] / (solve_ms * 1e3), 4)
            r["trim_status_counts"] = [int((s[0] == v).sum()) for v in (0, 1, 2)]
            r["trim_rounds"] = [int(s[1].min()), int(s[1].max())]
            r["trim_residual_max"] = float(np.nanmax(s[2]))
            r["trim_delta_tf_seconds"] = [float(np.nanmin(s[4])), float(np.nanmax(s[4]))]
        res[name] = r
        print(name, r, flush=True)
    s = json.dumps(dict(device=torch.cuda.get_device_name(0), reps=a.reps, cases=res), indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
