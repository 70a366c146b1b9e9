"""Device time of the quantile call, ascent_disperse_quantiles_batch, beside its parent on the same inputs -- the navigated flight
through ascent_disperse_navigated_batch (no history) or ascent_disperse_history_batch (node stride 10) -- and the wall time of
what gives quantiles without it: the parent with its sample rows kept, copied to the host, and np.quantile there.  Regimes: the
bench sweep 4096 x 1024 samples without history and at stride 10, its first 64 problems x 4096 samples and its first problem x
65536 samples at stride 10; each with 1 and with 7 probabilities.  N = 200, backward Euler, automatic substeps.  HIP events on
torch's stream, device pointers: every call only enqueues.  The call and its parent alternate, rep by rep, in one process; warm
(three untimed pairs), median of --reps with min .. max.  The host path runs once per regime, on at most --host-problems
problems; where that is fewer than the regime's, its time is scaled by the ratio and marked so.
Prints one JSON object; --out FILE writes it too."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAV_BIAS = (1e-3, 1e-3, 1e-6, 1e-6, 0.0, 0.0, 0.0)      # as scripts/history_timing.py
PROBS = {1: [0.00135], 7: [0.0, 0.00135, 0.25, 0.5, 0.75, 0.99865, 1.0]}
REGIMES = (("sweep_1024_end", 4096, 1024, 0), ("sweep_1024_stride10", 4096, 1024, 10), ("64_4096_stride10", 64, 4096, 10),
           ("1_65536_stride10", 1, 65536, 10))


def main():
    import torch
    from lunar_module_ascent_trajectory_optimiser_amd import sweep_isp_drymass, solve_batch_torch, _lib
    from lunar_module_ascent_trajectory_optimiser_amd.solver import _opts
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--regimes", nargs="*", default=[r[0] for r in REGIMES])
    ap.add_argument("--host-problems", type=int, default=256)
    a = ap.parse_args()
    L = _lib.load()
    nt, K = 200, 199
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, nt=nt, regimes={})
    dev = dict(dtype=torch.float64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = _opts(nt, 0, 1.0, 0, 0.0)

    def once(call):
        e0.record()
        _lib.check(call())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def summary(ts):
        ts = np.array(ts[3:])
        return dict(median=round(float(np.median(ts)), 1), min=round(float(ts.min()), 1), max=round(float(ts.max()), 1))

    sw = sweep_isp_drymass()
    pt_all = torch.from_numpy(np.ascontiguousarray(sw)).cuda()
    out = solve_batch_torch(pt_all, nt, sync=True, want_traj=False, want_blob=True)
    res.update(converged=int((out["status"] == 0).sum().item()))
    p = lambda t: None if t is None else t.data_ptr()
    for name, B, S, stride in REGIMES:
        if name not in a.regimes:
            continue
        pt, blob = pt_all[:B].contiguous(), out["blob"][:, :B].contiguous()
        w = torch.tensor([[1e6] * 3 + [1.0, 1.0, 0.5]] * B, **dev).T.contiguous()
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
        xi = torch.from_numpy(np.random.default_rng(0).standard_normal((24 + K, S))).cuda()
        xn = torch.from_numpy(np.random.default_rng(1).standard_normal((8, S))).cuda()
        nj = K // stride + (K % stride != 0) if stride else 0
        per_problem = [pt.T, blob, sig, sig_u, gu, gt, w[5], fu, ft, d, sn]      # the problem index last in each

        def parent(b):      # -> the parent call on the first b problems, and its arrays
            cp, cblob, csig, csig_u, *claw, csn = [t if b == B else t[..., :b].contiguous() for t in per_problem]
            cp = cp.T.contiguous()
            stats, hist = torch.empty((82, b), **dev), torch.empty((52, nj, b), **dev) if stride else None
            head = (cp.data_ptr(), b, C.byref(o), cblob.data_ptr(), 0, S, xi.data_ptr(), csig.data_ptr(), csig_u.data_ptr(),
                    *[t.contiguous().data_ptr() for t in claw], xn.data_ptr(), csn.data_ptr())
            keep = (cp, cblob, csig, csig_u, claw, csn, stats, hist)

            def flight(smp=None, hsmp=None):
                if stride:
                    return L.ascent_disperse_history_batch(*head, stride, stats.data_ptr(), p(smp), hist.data_ptr(), p(hsmp), 0, stream, 1)
                return L.ascent_disperse_navigated_batch(*head, stats.data_ptr(), p(smp), 0, stream, 1)
            return flight, head, stats, hist, keep
        flight, head, stats, hist, keep = parent(B)
        rows_bytes = (12 + 10 * nj) * S * B * 8
        r = dict(batch=B, samples=S, node_stride=stride, history_nodes=nj, sample_row_bytes=rows_bytes,
                 workspace_bytes=int(L.ascent_disperse_quantiles_bytes(B, nt, S, stride)))
        for n_probs, probs in PROBS.items():
            pr = np.array(probs)
            quant, hquant = torch.empty((n_probs, 12, B), **dev), torch.empty((n_probs, 10, nj, B), **dev) if stride else None
            new = lambda: L.ascent_disperse_quantiles_batch(
                *head, None, None, None, stride, stats.data_ptr(), p(hist), pr.ctypes.data_as(C.c_void_p), n_probs, None, None, 0,
                quant.data_ptr(), None, p(hquant), None, 0, stream, 1)
            tp, tq = [], []
            for _ in range(a.reps + 3):
                tp.append(once(flight))
                tq.append(once(new))
            sp, sq = summary(tp), summary(tq)
            added = sq["median"] - sp["median"]
            # the host path: the sample rows of hb problems kept, copied, np.quantile over the samples (every sample valid here)
            hb = min(B, a.host_problems)
            smp = torch.empty((12, S, hb), **dev)
            hsmp = torch.empty((10, nj, S, hb), **dev) if stride else None
            torch.cuda.synchronize()
            host_flight, *host_keep = parent(hb)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(host_flight(smp, hsmp))
            torch.cuda.synchronize()
            hq = np.quantile(smp.cpu().numpy(), pr, axis=1)
            if stride:
                hq = np.quantile(hsmp.cpu().numpy(), pr, axis=2)
            host_s = (time.perf_counter() - t0) * B / hb
            del smp, hsmp, hq, host_flight, host_keep
            r[f"probs{n_probs}"] = dict(parent_us=sp, quantiles_us=sq, added_us=round(added, 1), added_over_parent=round(added / sp["median"], 4),
                                        sample_rows_gb_per_s_over_added=round(rows_bytes / max(added, 1e-3) / 1e3, 1),
                                        host_path_wall_s=round(host_s, 3), host_path_problems=hb, host_path_scaled=hb != B,
                                        host_path_over_quantiles=round(host_s * 1e6 / sq["median"], 1))
        res["regimes"][name] = r
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
