"""Device time of the linear covariance corridor on the bench sweep, 4096 x N = 200, backward Euler, automatic substeps:
ascent_covariance_history_batch open loop and navigated (feed-forward, navigation biases and a knowledge error all on, the gains
just computed), at node strides 1 and 10, with and without jac_hist_out -- beside ascent_guidance_feedforward (the backward sweep
of the same length over the same step records), ascent_flight_jacobian, and ascent_disperse_history_batch at 1024 samples, the
sampled answer to the same question.  HIP events on torch's stream, device pointers: every call only enqueues.  Warm (three untimed
calls), median of --reps calls with min .. max, all from one process.  Prints one JSON object; --out FILE writes it too."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAV_BIAS = (1e-3, 1e-3, 1e-6, 1e-6, 0.0, 0.0, 0.0)      # as scripts/history_timing.py


def main():
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import sweep_isp_drymass, solve_batch_torch, _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--samples", type=int, default=1024, help="of the history call timed beside")
    ap.add_argument("--strides", type=int, nargs="*", default=[1, 10])
    ap.add_argument("--weight", type=float, default=1e6, help="q of the three conditions of the gains")
    a = ap.parse_args()
    L = _lib.load()
    nt, K = 200, 199
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, nt=nt, weight=a.weight, samples=a.samples)
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
    jac, jac_u = torch.empty((9, 24, B), **dev), torch.empty((9, K, B), **dev)
    head = (pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0)
    gains = lambda j, ju: L.ascent_guidance_feedforward(*head, w.data_ptr(), d.data_ptr(), d.data_ptr(), gu.data_ptr(), gt.data_ptr(), fu.data_ptr(),
                                                        ft.data_ptr(), gs.data_ptr(), j, ju, None, 0, stream, 1)
    us = dict(guidance_feedforward=timed(lambda: gains(None, None)), guidance_feedforward_jacobian=timed(lambda: gains(jac.data_ptr(), jac_u.data_ptr())),
              flight_jacobian=timed(lambda: L.ascent_flight_jacobian(*head, jac.data_ptr(), jac_u.data_ptr(), 0, stream, 1)))
    sig = torch.zeros((24, B), **dev)
    sig[7 + 3] = 50.0
    sig_u = torch.full((K, B), 1e-3, **dev)
    sn = torch.tensor([list(NAV_BIAS) + [10.0]] * B, **dev).T.contiguous()
    p = lambda t: None if t is None else t.data_ptr()
    law = dict(open=[None] * 7, navigated=[gu, gt, w[5], fu, ft, d, sn])
    S = a.samples
    xi = torch.from_numpy(np.random.default_rng(0).standard_normal((24 + K, S))).cuda()
    xn = torch.from_numpy(np.random.default_rng(1).standard_normal((8, S))).cuda()
    stats = torch.empty((82, B), **dev)
    for kind in ("open", "navigated"):
        for stride in a.strides:
            nj = K // stride + (K % stride != 0)
            nom, cov, jh, hist = torch.empty((10, nj, B), **dev), torch.empty((55, nj, B), **dev), torch.empty((10, 32, nj, B), **dev), torch.empty((52, nj, B), **dev)
            lin = lambda j: L.ascent_covariance_history_batch(*head, sig.data_ptr(), sig_u.data_ptr(), *[p(t) for t in law[kind]], stride,
                                                              nom.data_ptr(), cov.data_ptr(), j, 0, stream, 1)
            key = f"{kind}_stride{stride}"
            us[f"covariance_{key}"] = timed(lambda: lin(None))
            us[f"covariance_{key}_jacobian"] = timed(lambda: lin(jh.data_ptr()))
            mc = law[kind][:6] + ([xn, sn] if kind == "navigated" else [None, None])
            us[f"history_{S}_{key}"] = timed(lambda: L.ascent_disperse_history_batch(*head, S, xi.data_ptr(), sig.data_ptr(), sig_u.data_ptr(),
                                                                                    *[p(t) for t in mc], stride, stats.data_ptr(), None,
                                                                                    hist.data_ptr(), None, 0, stream, 1))
            c, h = cov.cpu().numpy(), hist.cpu().numpy()
            # the altitude's 1-sigma at the last node from both, over the sweep: what the two calls say about the same flight
            us[f"covariance_{key}"]["altitude_sigma_last_node_m"] = [round(float(np.sqrt(c[49, -1]).min()), 2), round(float(np.sqrt(c[49, -1]).max()), 2)]
            us[f"history_{S}_{key}"]["altitude_sigma_last_node_m"] = [round(float(np.sqrt(h[28, -1]).min()), 2), round(float(np.sqrt(h[28, -1]).max()), 2)]
            res[f"covariance_vs_history_{key}"] = round(us[f"covariance_{key}"]["median"] / us[f"history_{S}_{key}"]["median"], 4)
            res[f"covariance_vs_feedforward_{key}"] = round(us[f"covariance_{key}"]["median"] / us["guidance_feedforward"]["median"], 4)
            del nom, cov, jh, hist
    res.update(us=us)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
