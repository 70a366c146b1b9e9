"""Device time of the navigation filter on the bench sweep, 4096 x N = 200, backward Euler, automatic substeps, the guided flight
(gains at q = 1e6, no feed-forward), M = 4 measurements (the unit rows of x, y, xdot, ydot): ascent_navigation_filter (f_fly, n_filter)
at measurement strides 1 and 10, and ascent_covariance_filtered_batch (f_fly, l_lincov_filtered) at the same measurement strides
and node strides 1 and 10, beside the guided ascent_covariance_history_batch (f_fly, l_lincov) with a frozen navigation bias at the
same node strides.  The calls alternate: --rounds rounds (at least three), in each every call one after the other, each the median
of --reps calls after three untimed ones; reported per call: the median of the rounds' medians and their min .. max -- the
run-to-run spread.  HIP events on torch's stream, device pointers: every call only enqueues.  Prints one JSON object; --out FILE
writes it too."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAV_BIAS = (1e-3, 1e-3, 1e-6, 1e-6, 0.0, 0.0, 0.0)      # as scripts/history_timing.py
FIX_SIGMA = (3e-4, 3e-4, 3e-6, 3e-6)                    # as examples/apollo11.py


def main():
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import sweep_isp_drymass, solve_batch_torch, _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--strides", type=int, nargs="*", default=[1, 10], help="node strides")
    ap.add_argument("--meas-strides", type=int, nargs="*", default=[1, 10])
    ap.add_argument("--weight", type=float, default=1e6, help="q of the three conditions of the gains")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds: at least three")
    L = _lib.load()
    nt, K, M = 200, 199, 4
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, nt=nt, weight=a.weight, n_meas=M)
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
        return float(np.median(ts[3:]))

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
    head = (pt.data_ptr(), B, C.byref(o), blob.data_ptr(), 0)
    _lib.check(L.ascent_guidance_feedforward(*head, w.data_ptr(), d.data_ptr(), d.data_ptr(), gu.data_ptr(), gt.data_ptr(), fu.data_ptr(),
                                             ft.data_ptr(), gs.data_ptr(), None, None, None, 0, stream, 1))      # (the feedback gains are those of ascent_guidance_gains)
    sig = torch.zeros((24, B), **dev)
    sig[7 + 3] = 50.0
    sig_u = torch.full((K, B), 1e-3, **dev)
    sn8 = torch.tensor([list(NAV_BIAS) + [0.0]] * B, **dev).T.contiguous()
    sn7 = sn8[:7].contiguous()
    h = torch.zeros((M, 7, B), **dev)
    for i in range(M):
        h[i, i] = 1.0
    sm = torch.tensor([list(FIX_SIGMA)] * B, **dev).T.contiguous()
    smax = w[5].contiguous()
    law = [t.data_ptr() for t in (gu, gt, smax)]
    gl = {ms: torch.empty((M, 7, K, B), **dev) for ms in a.meas_strides}
    pf, summ = torch.empty((28, K, B), **dev), torch.empty((4, B), **dev)
    calls = {}
    for ms in a.meas_strides:
        calls[f"filter_meas{ms}"] = lambda ms=ms: L.ascent_navigation_filter(*head, sn7.data_ptr(), sig_u.data_ptr(), None, h.data_ptr(), sm.data_ptr(), M,
                                                                             ms, gl[ms].data_ptr(), pf.data_ptr(), summ.data_ptr(), 0, stream, 1)
        _lib.check(calls[f"filter_meas{ms}"]())
        torch.cuda.synchronize()
        res[f"filter_meas{ms}_status_ok"] = int((summ[0] == 0).sum().item())
    bufs = {}
    for stride in a.strides:
        nj = K // stride + (K % stride != 0)
        nom, cov, ncov = torch.empty((10, nj, B), **dev), torch.empty((55, nj, B), **dev), torch.empty((28, nj, B), **dev)
        bufs[stride] = (nom, cov, ncov)
        calls[f"covariance_parent_stride{stride}"] = lambda stride=stride, nom=nom, cov=cov: L.ascent_covariance_history_batch(
            *head, sig.data_ptr(), sig_u.data_ptr(), *law, None, None, None, sn8.data_ptr(), stride, nom.data_ptr(), cov.data_ptr(), None, 0, stream, 1)
        for ms in a.meas_strides:
            calls[f"covariance_filtered_meas{ms}_stride{stride}"] = lambda stride=stride, ms=ms, nom=nom, cov=cov, ncov=ncov: L.ascent_covariance_filtered_batch(
                *head, sig.data_ptr(), sig_u.data_ptr(), *law, sn7.data_ptr(), gl[ms].data_ptr(), h.data_ptr(), sm.data_ptr(), M, ms, stride,
                nom.data_ptr(), cov.data_ptr(), ncov.data_ptr(), None, None, 0, stream, 1)
    rounds = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k in calls:
            rounds[k].append(timed(calls[k]))
    us = {k: dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1)) for k, v in rounds.items()}
    for stride in a.strides:
        for ms in a.meas_strides:
            res[f"filtered_meas{ms}_vs_parent_stride{stride}"] = round(us[f"covariance_filtered_meas{ms}_stride{stride}"]["median"]
                                                                      / us[f"covariance_parent_stride{stride}"]["median"], 4)
    res.update(us=us)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
