"""Device time of the time-varying navigation error on the bench sweep, 4096 x N = 200, backward Euler, automatic substeps,
the navigated flight of scripts/lincov_timing.py (gains at q = 1e6, feed-forward, navigation biases and a 10 N knowledge error):
ascent_disperse_drifting_batch (f_history_drifting) beside ascent_disperse_history_batch (f_history_guided) at 1024 samples, and
ascent_covariance_drifting_batch (l_lincov_drifting) beside ascent_covariance_history_batch (l_lincov), at node strides 1 and 10,
the new calls once with all eight channels frozen (phi = 1, q = 0: the new kernels on the parent's arithmetic) and once with all
eight drifting (tau = 60 s, stationary).  The existing call and the new ones alternate: --rounds rounds (at least three), in each
the parent call, the frozen call and the drifting call one after the other, each the median of --reps calls after three untimed
ones; reported per call: the median of the rounds' medians and their min .. max -- the run-to-run spread.  HIP events on torch's
stream, device pointers: every call only enqueues.  Prints one JSON object; --out FILE writes it too."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--strides", type=int, nargs="*", default=[1, 10])
    ap.add_argument("--weight", type=float, default=1e6, help="q of the three conditions of the gains")
    ap.add_argument("--tau", type=float, default=60.0, help="correlation time (s) of the eight drifting channels")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds: at least three")
    L = _lib.load()
    nt, K, S = 200, 199, a.samples
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, nt=nt, weight=a.weight, samples=S, tau=a.tau)
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
                                             ft.data_ptr(), gs.data_ptr(), None, None, None, 0, stream, 1))
    sig = torch.zeros((24, B), **dev)
    sig[7 + 3] = 50.0
    sig_u = torch.full((K, B), 1e-3, **dev)
    sn = torch.tensor([list(NAV_BIAS) + [10.0]] * B, **dev).T.contiguous()
    law = [t.data_ptr() for t in (gu, gt, w[5].contiguous(), fu, ft, d)]
    xi = torch.from_numpy(np.random.default_rng(0).standard_normal((24 + K, S))).cuda()
    xn = torch.from_numpy(np.random.default_rng(1).standard_normal((8, S))).cuda()
    om = torch.from_numpy(np.random.default_rng(2).standard_normal((8, K, S))).cuda()
    dt = (blob[21 * K] * pt[:, 11] / K)
    phi_d = torch.exp(-dt / a.tau)[None, :].repeat(8, 1).contiguous()
    q_d = (sn * torch.sqrt(1.0 - phi_d * phi_d)).contiguous()
    q_d[q_d == 0] = 1e-9          # the channels without an initial sigma drift as well: all eight rows of the draws are read
    drift = dict(frozen=(torch.ones((8, B), **dev), torch.zeros((8, B), **dev)), drifting=(phi_d, q_d))
    stats = torch.empty((82, B), **dev)
    us = {}
    for stride in a.strides:
        nj = K // stride + (K % stride != 0)
        nom, cov, hist = torch.empty((10, nj, B), **dev), torch.empty((55, nj, B), **dev), torch.empty((52, nj, B), **dev)
        calls = {
            "history_parent": lambda: L.ascent_disperse_history_batch(*head, S, xi.data_ptr(), sig.data_ptr(), sig_u.data_ptr(), *law, xn.data_ptr(),
                                                                      sn.data_ptr(), stride, stats.data_ptr(), None, hist.data_ptr(), None, 0, stream, 1),
            "covariance_parent": lambda: L.ascent_covariance_history_batch(*head, sig.data_ptr(), sig_u.data_ptr(), *law, sn.data_ptr(), stride,
                                                                           nom.data_ptr(), cov.data_ptr(), None, 0, stream, 1)}
        for name, (ph, qq) in drift.items():
            calls[f"history_{name}"] = lambda ph=ph, qq=qq: L.ascent_disperse_drifting_batch(
                *head, S, xi.data_ptr(), sig.data_ptr(), sig_u.data_ptr(), *law, xn.data_ptr(), sn.data_ptr(), ph.data_ptr(), qq.data_ptr(),
                om.data_ptr(), stride, stats.data_ptr(), None, hist.data_ptr(), None, 0, stream, 1)
            calls[f"covariance_{name}"] = lambda ph=ph, qq=qq: L.ascent_covariance_drifting_batch(
                *head, sig.data_ptr(), sig_u.data_ptr(), *law, sn.data_ptr(), ph.data_ptr(), qq.data_ptr(), stride, nom.data_ptr(), cov.data_ptr(),
                None, 0, stream, 1)
        rounds = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k in ("history_parent", "history_frozen", "history_drifting", "covariance_parent", "covariance_frozen", "covariance_drifting"):
                rounds[k].append(timed(calls[k]))
        for k, v in rounds.items():
            us[f"{k}_stride{stride}"] = dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
        for kind in ("history", "covariance"):
            for name in drift:
                res[f"{kind}_{name}_vs_parent_stride{stride}"] = round(us[f"{kind}_{name}_stride{stride}"]["median"] / us[f"{kind}_parent_stride{stride}"]["median"], 4)
        del nom, cov, hist
    res.update(us=us)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
