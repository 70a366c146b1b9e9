"""Device time of the flight verification (ascent_fly_batch: the serial fly-out f_fly and the per-step local error f_local)
beside the solve whose blob it reads.  HIP events on torch's stream, device pointers: the call only enqueues.  The entry point
always launches both kernels (each owns rows of the summary), so the events bracket the pair; the time of each kernel comes
from `rocprofv3 --kernel-trace --stats -- python scripts/flight_timing.py --case NAME` (kernel names f_fly / f_local), a run
of its own per case (profiles/flight_kernels.csv).
Cases: the bench sweep 4096 x N = 200 with backward Euler and with the trapezoid, and one NLP at N = 2000 (Hermite-Simpson).
Warm (three untimed calls), median of --reps calls.  Prints one JSON object; --out FILE writes it too."""
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
    ap.add_argument("--case", help="only this case (for a profiler run whose per-kernel statistics then belong to one case)")
    a = ap.parse_args()
    L = _lib.load()
    sw = sweep_isp_drymass()
    nom = AscentParams(tf_ub=1.2).as_row()
    cases = [("sweep_4096_n200_backward_euler", sw, 200, 0), ("sweep_4096_n200_trapezoid", sw, 200, 1),
             ("single_n2000_hermite_simpson", nom[None].copy(), 2000, 2)]
    res = {}
    if a.case:
        cases = [c for c in cases if c[0] == a.case]
        assert cases, a.case
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
        traj = torch.empty((10, nt, B), dtype=torch.float64, device="cuda")
        loc = torch.empty((K, 7, B), dtype=torch.float64, device="cuda")
        summ = torch.empty((10, B), dtype=torch.float64, device="cuda")
        o = _opts(nt, 0, 1.0, 0, 0.0, scheme)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ts = []
        for _ in range(a.reps + 3):
            e0.record()
            _lib.check(L.ascent_fly_batch(pt.data_ptr(), B, C.byref(o), out["blob"].data_ptr(), 0, traj.data_ptr(), loc.data_ptr(),
                                          summ.data_ptr(), 0, stream, 1))
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts = np.array(ts[3:])
        s = summ.cpu().numpy()
        res[name] = dict(batch=B, nt=nt, scheme=scheme, converged=int((out["status"] == 0).sum().item()),
                         substeps=sorted(set(int(v) for v in s[9])), solve_ms=round(solve_ms, 3),
                         fly_us_median=round(float(np.median(ts)), 1), fly_us_min=round(float(ts.min()), 1),
                         fly_us_max=round(float(ts.max()), 1), fly_share_of_solve=round(float(np.median(ts)) / (solve_ms * 1e3), 4),
                         miss_position_m=[float(s[0].min()), float(s[0].max())])
        print(name, res[name], flush=True)
    s = json.dumps(dict(device=torch.cuda.get_device_name(0), reps=a.reps, cases=res), indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
