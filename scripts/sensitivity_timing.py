"""Device time of the post-optimal sensitivity kernel (ascent_param_sensitivity) beside the solve it reads (HIP events on
torch's stream, device pointers: the call only enqueues).  Cases: the bench sweep 4096 x N = 200 with and without the move
penalty, 256 x N = 2000 Hermite-Simpson, one NLP at N = 2000.  Prints one JSON object; --out FILE writes it too."""
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
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts, blob_rows
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.load()
    sw = sweep_isp_drymass()
    sw[:, 15] = 1e-4
    nom = AscentParams(tf_ub=1.2, dcost=1e-4).as_row()
    cases = [("sweep_4096_n200", sw, 200, 0, False), ("sweep_4096_n200_penalty", sw, 200, 0, True),
             ("hs_256_n2000", np.tile(nom, (256, 1)), 2000, 2, False), ("single_n2000", nom[None].copy(), 2000, 0, False)]
    res = {}
    for name, P, nt, scheme, mp in cases:
        pt = torch.from_numpy(np.ascontiguousarray(P)).cuda()
        B = P.shape[0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = solve_batch_torch(pt, nt, want_traj=False, want_blob=True, scheme=scheme, move_penalty=mp, sync=True)
        e0.record()
        solve_batch_torch(pt, nt, want_traj=False, want_blob=True, scheme=scheme, move_penalty=mp, out=out)
        e1.record()
        torch.cuda.synchronize()
        solve_ms = e0.elapsed_time(e1)
        g = torch.empty((16, B), dtype=torch.float64, device="cuda")
        o = _opts(nt, 0, 1.0, 0, 0.0, scheme, move_penalty=mp)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ts = []
        for _ in range(a.reps + 3):
            e0.record()
            _lib.check(L.ascent_param_sensitivity(pt.data_ptr(), B, C.byref(o), out["blob"].data_ptr(), g.data_ptr(), 0, stream, 1))
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts = np.array(ts[3:])
        blob_mb = blob_rows(nt) * B * 8 / 1e6
        res[name] = dict(batch=B, nt=nt, scheme=scheme, move_penalty=mp, converged=int((out["status"] == 0).sum().item()),
                         solve_ms=round(solve_ms, 3), sens_us_median=round(float(np.median(ts)), 2),
                         sens_us_min=round(float(ts.min()), 2), blob_MB=round(blob_mb, 2),
                         sens_share_of_solve=round(float(np.median(ts)) / (solve_ms * 1e3), 5))
        print(name, res[name], flush=True)
    s = json.dumps(dict(device=torch.cuda.get_device_name(0), reps=a.reps, cases=res), indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
