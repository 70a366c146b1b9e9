"""Device time of the per-node Monte Carlo history on the bench sweep, 4096 x N = 200, backward Euler, automatic substeps:
ascent_disperse_history_batch beside the plain call of the same kind -- ascent_disperse_batch (open loop),
ascent_disperse_guided_batch and ascent_disperse_navigated_batch (feed-forward, navigation biases and a knowledge error all on)
with the gains just computed -- at samples = 16, 256 and 1024 and node strides 1, 10 and K.  HIP events on torch's stream, device
pointers: every call only enqueues.  Warm (three untimed calls), median of --reps calls with min .. max, all from one process.
Prints one JSON object; --out FILE writes it too.  Per-kernel times of one call:
`rocprofv3 --kernel-trace --stats -- python scripts/history_timing.py --kinds navigated --samples 1024 --strides 1 --reps 1`."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAV_BIAS = (1e-3, 1e-3, 1e-6, 1e-6, 0.0, 0.0, 0.0)      # as scripts/feedforward_timing.py


def main():
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import sweep_isp_drymass, solve_batch_torch, _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--samples", type=int, nargs="*", default=[16, 256, 1024])
    ap.add_argument("--strides", type=int, nargs="*", default=[1, 10, 199])
    ap.add_argument("--kinds", nargs="*", default=["open", "guided", "navigated"], choices=("open", "guided", "navigated"))
    ap.add_argument("--weight", type=float, default=1e6, help="q of the three conditions of the gains")
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

    sw = sweep_isp_drymass()
    B = sw.shape[0]
    pt = torch.from_numpy(np.ascontiguousarray(sw)).cuda()
    out = solve_batch_torch(pt, nt, sync=True, want_traj=False, want_blob=True)
    blob = out["blob"]
    res.update(batch=B, converged=int((out["status"] == 0).sum().item()))
    w = torch.tensor([[a.weight] * 3 + [1.0, 1.0, 0.5]] * B, **dev).T.contiguous()
    d = torch.zeros((16, B), **dev)
    d[3] = 1.0
    gu, gt, gs = torch.empty((7, K, B), **dev), torch.empty((7, B), **dev), torch.empty((7, B), **dev)
    fu, ft = torch.empty((K, B), **dev), torch.empty((B,), **dev)
    _lib.check(L.ascent_guidance_feedforward(pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, w.data_ptr(), d.data_ptr(), d.data_ptr(),
                                             gu.data_ptr(), gt.data_ptr(), fu.data_ptr(), ft.data_ptr(), gs.data_ptr(), None, None, None, 0, stream, 1))
    sig = torch.zeros((24, B), **dev)
    sig[7 + 3] = 50.0
    sig_u = torch.full((K, B), 1e-3, **dev)
    sn = torch.tensor([list(NAV_BIAS) + [10.0]] * B, **dev).T.contiguous()
    stats = torch.empty((82, B), **dev)
    p = lambda t: None if t is None else t.data_ptr()
    us = {}
    for S in a.samples:
        xi = torch.from_numpy(np.random.default_rng(0).standard_normal((24 + K, S))).cuda()
        xn = torch.from_numpy(np.random.default_rng(1).standard_normal((8, S))).cuda()
        head = (pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, S, xi.data_ptr(), sig.data_ptr(), sig_u.data_ptr())
        tail = (stats.data_ptr(), None, 0, stream, 1)
        law = dict(open=[None] * 8, guided=[gu, gt, w[5]] + [None] * 5, navigated=[gu, gt, w[5], fu, ft, d, xn, sn])
        plain = dict(open=lambda: L.ascent_disperse_batch(*head, *tail),
                     guided=lambda: L.ascent_disperse_guided_batch(*head, gu.data_ptr(), gt.data_ptr(), w[5].data_ptr(), *tail),
                     navigated=lambda: L.ascent_disperse_navigated_batch(*head, *[p(t) for t in law["navigated"]], *tail))
        for kind in a.kinds:
            us[f"{kind}_{S}"] = timed(plain[kind])
            for stride in a.strides:
                nj = K // stride + (K % stride != 0)
                hist = torch.empty((52, nj, B), **dev)
                key = f"{kind}_{S}_history_stride{stride}"
                us[key] = timed(lambda: L.ascent_disperse_history_batch(*head, *[p(t) for t in law[kind]], stride, stats.data_ptr(), None,
                                                                        hist.data_ptr(), None, 0, stream, 1))
                h = hist.cpu().numpy()
                us[key]["valid_samples_last_node"] = [int(h[0, -1].min()), int(h[0, -1].max())]
                res[f"history_vs_plain_{kind}_{S}_stride{stride}"] = round(us[key]["median"] / us[f"{kind}_{S}"]["median"], 4)
                del hist
    res.update(us=us)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
