"""Every output array of the thirteen calls on a solution blob, as raw bytes, for comparing two builds of the library bit for bit.

    python scripts/analysis_dump.py --out FILE.npz              (on the GPU, once in each tree)
    python scripts/analysis_dump.py --compare A.npz B.npz --json profiles/analysis_refactor_parity.json    (anywhere)

Solves a batch of 5 at nt = 18 and 34 (K = 17: two chunks of the Jacobian sweep, the last holding one step; three chunks) in both
formulations, then makes problem 3's blob hold a NaN t_f and gives problem 4 invalid guidance weights (a frozen problem).  Every
call runs with substeps 0 and 2, through host pointers and through device pointers, with its optional outputs on and null:
sensitivity, flight, flight Jacobian, trim, gains and feed-forward gains (thrust direction, with and without ff_know, stretch_max
0 and 0.5), and the three dispersions at 70 samples (two wavefronts, the second partly filled) and 300 (two workgroups per
problem), with and without control sigmas, feed-forward, knowledge row and navigation sigmas.  Output buffers start as 7.25, so
an element a build does not write compares equal only if the other build does not write it either.

The four corridor calls (corridors): the two covariance calls at strides 1, 4 and K, open loop | feedback only | feedback with
feed-forward, ff_know and sigma_nav, stretch_max 0 and 0.5 (the stretched last step), sigma_u given and null, jac_hist_out given
and null; the drifting one with nav_phi / nav_q null, all frozen and the channel mix of tests/test_gpu_navdrift.py, and through
device pointers one problem with phi = 2.  The two Monte Carlo history calls run at 70 samples only, as the control.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 5
FILL = 7.25
# the channel mix of tests/test_gpu_navdrift.py: stationary | decaying | frozen | zero-start random walk | phi = 0 | zero-start | frozen | stationary
PHI = np.array([0.9, 0.5, 1.0, 1.0, 0.0, 0.97, 1.0, 0.7])
DRIVE = np.array([np.sqrt(1 - 0.81), 0.0, 0.0, 0.3, 1.0, 0.2, 0.0, np.sqrt(1 - 0.49)])


class Caller:
    """One entry point called with numpy arrays: inputs copied to the device and outputs back where dev is set."""

    def __init__(self, L, dev):
        self.L, self.dev = L, dev
        if dev:
            import torch
            self.torch = torch

    def __call__(self, entry, *args):
        keep, outs, real = [], [], []
        for a in args:
            if isinstance(a, np.ndarray):
                if self.dev:
                    t = self.torch.from_numpy(a.view(np.float64) if a.dtype != np.float64 else a).cuda()
                    keep.append(t)
                    outs.append((a, t))
                    real.append(C.c_void_p(t.data_ptr()))
                else:
                    real.append(a.ctypes.data_as(C.c_void_p))
            else:
                real.append(a)
        rc = getattr(self.L, entry)(*real, 0, None, 1 if self.dev else 0)
        if rc:
            raise RuntimeError(f"{entry}: {rc} {self.L.ascent_strerror(rc).decode()}")
        if self.dev:
            self.torch.cuda.synchronize()
            for a, t in outs:
                a[...] = t.cpu().numpy().reshape(a.shape)
        return rc


def out(*shape):
    return np.full(shape, FILL)


def corridors(call, keep, po, sub, K, dev, gains, xi, xn, om, sigma, sigma_u, sigma_nav, ff_know):
    """ascent_covariance_history_batch, ascent_covariance_drifting_batch and, at 70 samples, the two Monte Carlo history calls"""
    S = xi.shape[1]
    mix_phi, mix_q = np.ascontiguousarray(np.tile(PHI, (B, 1)).T), np.ascontiguousarray(sigma_nav * DRIVE[:, None])
    drifts = {"null": (None, None), "frozen": (np.ones((8, B)), np.zeros((8, B))), "mix": (mix_phi, mix_q)}
    if dev:                                                   # with host pointers a phi outside [0, 1] is refused
        bad = mix_phi.copy()
        bad[0, 1] = 2.0
        drifts["phi2"] = (bad, mix_q)
    laws = {"open": [None] * 7}
    for smax in (0.0, 0.5):
        gu, gt, fu, ft, sx = gains[smax]
        laws[f"fb_s{smax}"] = [gu, gt, sx, None, None, None, None]
        laws[f"ff_s{smax}"] = [gu, gt, sx, fu, ft, ff_know, sigma_nav]
    for stride in (1, 4, K):
        NJ = (K + stride - 1) // stride
        for law, a in laws.items():
            for su in (1, 0):
                u = sigma_u if su else None
                for jac_on in (1, 0):
                    name = f"n{stride}_{law}_u{su}_j{jac_on}"
                    nom, cov, jac = out(10, NJ, B), out(55, NJ, B), out(10, 32, NJ, B) if jac_on else None
                    call("ascent_covariance_history_batch", *po, sub, sigma, u, *a, stride, nom, cov, jac)
                    keep(f"lincov_{name}", nominal=nom, cov=cov, **({"jac": jac} if jac_on else {}))
                    for dn, (ph, qq) in drifts.items() if law != "open" else ():
                        nom, cov, jac = out(10, NJ, B), out(55, NJ, B), out(10, 32, NJ, B) if jac_on else None
                        call("ascent_covariance_drifting_batch", *po, sub, sigma, u, *a, ph, qq, stride, nom, cov, jac)
                        keep(f"lincov_drift_{dn}_{name}", nominal=nom, cov=cov, **({"jac": jac} if jac_on else {}))
    for stride in (4, K):
        NJ = (K + stride - 1) // stride
        for law, a in laws.items():
            mc = a[:6] + [xn if a[6] is not None else None, a[6]]
            st, sp, hi, hs = out(82, B), out(12, S, B), out(52, NJ, B), out(10, NJ, S, B)
            call("ascent_disperse_history_batch", *po, sub, S, xi, sigma, sigma_u, *mc, stride, st, sp, hi, hs)
            keep(f"history_n{stride}_{law}", stats=st, samples=sp, hist=hi, hist_samples=hs)
            for dn, (ph, qq) in drifts.items() if law != "open" else ():
                st, sp, hi, hs = out(82, B), out(12, S, B), out(52, NJ, B), out(10, NJ, S, B)
                call("ascent_disperse_drifting_batch", *po, sub, S, xi, sigma, sigma_u, *mc, ph, qq, om if ph is not None else None, stride,
                     st, sp, hi, hs)
                keep(f"history_drift_{dn}_n{stride}_{law}", stats=st, samples=sp, hist=hi, hist_samples=hs)


def dump(path):
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    L = _lib.load()
    res = {}
    rng = np.random.default_rng(11)
    for nt in (18, 34):
        K = nt - 1
        for form in (0, 1):
            P = np.ascontiguousarray(A.sweep_isp_drymass(3, 2)[:B])
            r = A.solve_batch(P, nt=nt, tol=1e-9, formulation=form, want_blob=True)
            print(f"nt {nt} formulation {form}: status {r.status.tolist()}", flush=True)
            blob = np.ascontiguousarray(r.blob, dtype=np.float64).copy()
            blob[21 * K + 0, 3] = np.nan                      # t_f of problem 3
            o = _lib.AscentOptsC(n_nodes=nt, scheme=0, max_iter=0, warm_start=0, tol=1.0, mu_init=0.0, formulation=form)
            sigma = np.zeros((24, B))
            sigma[:7] = 1e-5
            sigma[7:23] = 1e-3 * np.abs(P.T)
            sigma[7 + 10] = 0.0                               # r_apo: a zero sigma, its draw does not count
            sigma[23] = 1e-3
            sigma_u = np.full((K, B), 1e-2)
            sigma_u[1] = 0.0
            sigma_nav = np.full((8, B), 1e-5)
            sigma_nav[7] = 0.5
            ff_dir = np.zeros((16, B))
            ff_dir[3] = 1.0                                   # Ft
            ff_know = ff_dir.copy()
            xis = {S: rng.standard_normal((24 + K, S)) for S in (70, 300)}
            xin = {S: rng.standard_normal((8, S)) for S in (70, 300)}
            om = rng.standard_normal((8, K, 70))
            for sub in (0, 2):
                for dev in (0, 1):
                    call = Caller(L, dev)
                    tag = f"nt{nt}_f{form}_m{sub}_{'dev' if dev else 'host'}"
                    po = (P, B, C.byref(o), blob)

                    def keep(name, **arrays):
                        for k, v in arrays.items():
                            res[f"{tag}/{name}/{k}"] = v.copy().view(np.uint64)

                    g = out(16, B)
                    call("ascent_param_sensitivity", *po, g)
                    keep("sens", grad=g)
                    tr, le, sm = out(10, nt, B), out(7, K, B), out(10, B)
                    call("ascent_fly_batch", *po, sub, tr, le, sm)
                    keep("fly", traj=tr, local=le, summary=sm)
                    sm = out(10, B)
                    call("ascent_fly_batch", *po, sub, None, None, sm)
                    keep("fly_summary_only", summary=sm)
                    j, ju = out(9, 24, B), out(9, K, B)
                    call("ascent_flight_jacobian", *po, sub, j, ju)
                    keep("jac", jac=j, jac_u=ju)
                    j = out(9, 24, B)
                    call("ascent_flight_jacobian", *po, sub, j, None)
                    keep("jac_no_u", jac=j)
                    tb, ts = out(21 * K + 10, B), out(10, B)
                    call("ascent_trim_batch", *po, sub, 0, 0.0, tb, ts)
                    keep("trim", blob=tb, summary=ts)
                    gains = {}
                    for smax in (0.0, 0.5):
                        w = np.ascontiguousarray(np.array([[1e6] * B, [1e6] * B, [1e6] * B, [1.0] * B, [1.0] * B, [smax] * B]))
                        w[3, 4] = -1.0                        # problem 4: an invalid weight, a frozen problem
                        for jac_on in (1, 0):
                            gu, gt, gs = out(7, K, B), out(7, B), out(5, B)
                            j, ju = (out(9, 24, B), out(9, K, B)) if jac_on else (None, None)
                            call("ascent_guidance_gains", *po, sub, w, gu, gt, gs, j, ju)
                            keep(f"gains_s{smax}_j{jac_on}", gain_u=gu, gain_t=gt, summary=gs, **({"jac": j, "jac_u": ju} if jac_on else {}))
                        for know in (1, 0):
                            for jac_on in ((1, 0) if know else (0,)):
                                gu, gt, fu, ft, gs = out(7, K, B), out(7, B), out(K, B), out(B), out(7, B)
                                j, ju, jn = (out(9, 24, B), out(9, K, B), out(9, 8, B)) if jac_on else (None, None, None)
                                call("ascent_guidance_feedforward", *po, sub, w, ff_dir, ff_know if know else None, gu, gt, fu, ft, gs, j, ju, jn)
                                keep(f"ff_s{smax}_k{know}_j{jac_on}", gain_u=gu, gain_t=gt, ff_u=fu, ff_t=ft, summary=gs,
                                     **({"jac": j, "jac_u": ju, "jac_nav": jn} if jac_on else {}))
                        gains[smax] = (gu, gt, fu, ft, w[5].copy())
                    for S in (70, 300):
                        xi, xn = xis[S], xin[S]
                        for su in (1, 0):
                            x = xi if su else np.ascontiguousarray(xi[:24])
                            u = sigma_u if su else None
                            st, sp = out(82, B), out(9, S, B) if S == 70 else None
                            call("ascent_disperse_batch", *po, sub, S, x, sigma, u, st, sp)
                            keep(f"disperse_S{S}_u{su}", stats=st, **({"samples": sp} if sp is not None else {}))
                            for smax in (0.0, 0.5):
                                gu, gt, fu, ft, sx = gains[smax]
                                st, sp = out(82, B), out(12, S, B) if S == 70 else None
                                call("ascent_disperse_guided_batch", *po, sub, S, x, sigma, u, gu, gt, sx, st, sp)
                                keep(f"guided_S{S}_u{su}_s{smax}", stats=st, **({"samples": sp} if sp is not None else {}))
                                for know in (1, 0):
                                    for nav in (1, 0):
                                        st, sp = out(82, B), out(12, S, B) if S == 70 else None
                                        call("ascent_disperse_navigated_batch", *po, sub, S, x, sigma, u, gu, gt, sx, fu, ft,
                                             ff_know if know else None, xn if nav else None, sigma_nav if nav else None, st, sp)
                                        keep(f"navigated_S{S}_u{su}_s{smax}_k{know}_n{nav}", stats=st, **({"samples": sp} if sp is not None else {}))
                                st = out(82, B)       # zero gains and nothing new: the guided and navigated kernels on the open-loop flight
                                call("ascent_disperse_guided_batch", *po, sub, S, x, sigma, u, np.zeros((7, K, B)), None, None, st, None)
                                keep(f"guided_zero_S{S}_u{su}_s{smax}", stats=st)
                    corridors(call, keep, po, sub, K, dev, gains, xis[70], xin[70], om, sigma, sigma_u, sigma_nav, ff_know)
    np.savez_compressed(path, **res)
    print(f"{len(res)} arrays -> {path}")


def compare(a, b, json_path):
    x, y = np.load(a), np.load(b)
    names = sorted(set(x.files) | set(y.files))
    rows = {n: ("equal" if n in x.files and n in y.files and x[n].shape == y[n].shape and np.array_equal(x[n], y[n], equal_nan=True) else "differ")
            for n in names}
    bad = [n for n, v in rows.items() if v != "equal"]
    groups = {}                                               # per grid, formulation, substeps and pointer kind: arrays, of them differing
    for n, v in rows.items():
        g = groups.setdefault(n.split("/")[0], [0, 0])
        g[0] += 1
        g[1] += v != "equal"
    doc = {"_comment": "scripts/analysis_dump.py --compare: the uint64 views of every output array of the thirteen calls on a solution blob, "
                       "the parent commit's library against this tree's, both run on the same MI355X; per group [arrays, differing], "
                       "and the names of the arrays that differ",
           "arrays": len(names), "differ": len(bad), "groups": groups, "differing": bad}
    if json_path:
        with open(json_path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(f"{len(names)} arrays, {len(bad)} differ")
    for n in bad:
        print("  differ:", n)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.json))
    dump(a.out)
