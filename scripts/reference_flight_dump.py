"""Every array the closed-loop CPU references (tests/guidance_reference.py, feedforward_reference.py, history_reference.py,
navdrift_reference.py, lincov_reference.py) return, as digests of their raw bytes, for comparing two trees bit for bit.  The GPU
tests take their bounds from these functions' float64-against-longdouble gaps, so a change to them has to leave every bit alone.

    python scripts/reference_flight_dump.py --out FILE.json [--tests DIR]          (once per tree; DIR: that tree's tests/)
    python scripts/reference_flight_dump.py --compare A.json B.json --json profiles/reference_flight_parity.json

No GPU.  The dumps depend on the machine (math.* and the 80-bit longdouble) and are not kept; the comparison's counts are.

At nt = 18 (substeps 2) and nt = 3, both formulations, float64 and longdouble: the nominal nodes; the four sample drivers open
loop, under the reference's own gains at q = 1e6 and 1e10, with feed-forward and navigation errors, and with the drifting
channels null, all frozen and in the mix of tests/test_navdrift_reference.py; sigmas of 1e-3 and of 5e-2 (commands clip),
stretch_max 0.5, 1e-5 (the cutoff stretch saturates) and 0; seven samples, of which one has a perturbed t_f that is not finite,
three leave the finite range mid-flight, and one ends in an exception of math.* after two steps with effort accumulated; blobs
whose t_f is NaN and inf (an exception counts as an outcome and is compared by its type); every flight once more by itself; and
the two covariance corridors open loop, guided, navigated, with a feed-forward but no stretch, and with a feed-forward but no
gains.  A longdouble array is digested on its 10 significant bytes per element, not on the padding.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LD = np.longdouble
OUT = {}
E_FT = np.eye(16)[3]
SIGMA_NAV = np.array([1e-5, 2e-5, 0.0, 1e-5, 1e-4, 0.0, 1e-5, 5.0])
PHI = np.array([0.9, 0.5, 0.8, 1.0, 0.0, 0.97, 1.0, 0.7])
Q = np.array([1e-5 * np.sqrt(1 - 0.81), 0.0, 3e-6, 0.0, 1e-4, 2e-6, 0.0, 5.0 * np.sqrt(1 - 0.49)])


def put(name, v):
    if isinstance(v, dict):
        for k, x in v.items():
            if k != "rec":
                put(name + "/" + k, x)
        return
    if isinstance(v, (tuple, list)) and not all(np.isscalar(x) for x in v):
        for i, x in enumerate(v):
            put(f"{name}/{i}", x)
        return
    if v is None:
        OUT[name] = ["None", [], ""]
        return
    a = np.asarray(v)
    assert a.dtype != object, name
    assert name not in OUT, name
    a = np.ascontiguousarray(a)
    raw = a.tobytes()
    if a.dtype == np.longdouble and a.itemsize == 16:          # 80 bits in 16 bytes: the padding is not part of the value
        raw = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 16)[:, :10].tobytes()
    OUT[name] = [str(a.dtype), list(a.shape), hashlib.sha256(raw).hexdigest()]


def call(name, f, *a, **k):
    try:
        r = f(*a, **k)
    except Exception as e:          # an exception is an outcome too: its type is compared
        OUT[name] = ["raises", [], type(e).__name__]
        return None
    put(name, r)
    return r


# ---- one flight, in a tree that has fly_guided, fly_navigated and fly_drifting and in one that has guidance_reference.fly
def fly_guided(*a, **k):
    if hasattr(gr, "fly_guided"):
        return gr.fly_guided(*a, **k)
    f = gr.fly(*a[:10], None, None, 0.0, None, None, *a[10:], **k)
    return gr.end_rows(f), gr.effort(f)


def fly_navigated(*a, **k):
    if hasattr(ffr, "fly_navigated"):
        return ffr.fly_navigated(*a, **k)
    f = gr.fly(*a, **k)
    return gr.end_rows(f), gr.effort(f)


def fly_drifting(*a, **k):
    if hasattr(nd, "fly_drifting"):
        return nd.fly_drifting(*a, **k)
    return hr.fly_history(*a, **k)


def p16_():
    return np.array([getattr(Params(), f) for f in fr.FIELDS], dtype=np.float64)


def blob_(nt):
    p16 = p16_()
    if nt == 3:
        return fr.make_blob(np.zeros((2, 7)), np.array([0.4, -0.7]), 0.05)
    b = fr.synthetic_exact_blob(p16, nt, tf=0.9, seed=4)
    K = nt - 1
    b[7 * K + 3], b[7 * K + K - 2] = 1.0, -1.0
    return b


def law_(p16, blob, nt, form, q):
    K = nt - 1
    rec = gr.records(p16, blob, nt, form, 2, LD)
    G = ffr.gains(rec, p16, np.array([q, q, q, 1.0, 1.0, 0.5]), E_FT, LD)
    if G["summary"][0] != 0:
        r = np.random.default_rng(8)
        return r.standard_normal((K, 7)), r.standard_normal(7), r.standard_normal(K) * 1e-4, 1e-4
    return G["gain_u"].astype(np.float64), G["gain_t"].astype(np.float64), G["ff_u"].astype(np.float64), float(G["ff_t"])


def main():
    p16 = p16_()
    for nt in (18, 3):
        K = nt - 1
        blob = blob_(nt)
        _, us, tf = fr.blob_parts(blob, nt)
        S = 7
        r = np.random.default_rng(1)
        xi, xn, om = r.standard_normal((24 + K, S)), r.standard_normal((8, S)), r.standard_normal((8, K, S))
        xi[23, 2] = np.inf                  # a non-finite perturbed t_f
        xi[0, 3] = 1e305                    # states that leave the finite range mid-flight, three ways
        xi[7 + 6, 4] = -1e6
        xi[2, 5] = 1e200
        xi[5, 6] = 2e307                    # with the 5e-2 sigmas: math.cos(inf) raises after two steps, effort accumulated
        sigma, su = dr.relative_sigma(p16, 1e-3), np.full(K, 1e-3)
        su[min(5, K - 1)] = 0.0
        big = dr.relative_sigma(p16, 5e-2)
        sn = np.array([1e-6] * 7 + [1e-3 * p16[3]])
        nanblob = blob.copy()
        nanblob[21 * K] = np.nan
        infblob = blob.copy()
        infblob[21 * K] = np.inf
        for form in (0, 1):
            laws = {q: law_(p16, blob, nt, form, q) for q in (1e6, 1e10)}
            for dtype in (np.float64, LD):
                tag = f"nt{nt}/form{form}/{dtype.__name__}"
                kw = dict(formulation=form, substeps=2, dtype=dtype)
                m = fr.substeps_of((tf * p16[11]) / K, 2)
                nodes = call(tag + "/nominal_nodes", gr.nominal_nodes, p16, us, tf, m, form, dtype)
                call(tag + "/nominal_nodes_m0", gr.nominal_nodes, p16, us, tf, fr.substeps_of((tf * p16[11]) / K, 0), form, dtype)
                call(tag + "/nominal_nodes_inf", gr.nominal_nodes, p16, us, np.inf, m, form, dtype)
                zero = np.zeros((K, 7))
                # open loop
                call(tag + "/open/guided", gr.disperse_guided, p16, blob, nt, xi, sigma, su, zero, np.zeros(7), 0.5, **kw)
                call(tag + "/open/guided_nosu", gr.disperse_guided, p16, blob, nt, xi, sigma, None, zero, None, 0.0, **kw)
                call(tag + "/open/history", hr.history, p16, blob, nt, xi, sigma, su, **kw)
                call(tag + "/open/history_nav_ignored", hr.history, p16, blob, nt, xi, sigma, None, know=E_FT, xi_nav=xn, sigma_nav=sn, **kw)
                call(tag + "/open/drifting", nd.history_drifting, p16, blob, nt, xi, sigma, su, None, **kw)
                for q, (gu, gt, fu, ft) in laws.items():
                    for sname, sg in (("s1e-3", sigma), ("s5e-2", big)):
                        for smax in (0.5, 1e-5, 0.0):
                            t = f"{tag}/q{q:g}/{sname}/smax{smax:g}"
                            call(t + "/guided", gr.disperse_guided, p16, blob, nt, xi, sg, su, gu, gt, smax, **kw)
                            call(t + "/history_guided", hr.history, p16, blob, nt, xi, sg, su, gu, gt, smax, **kw)
                            call(t + "/navigated", ffr.disperse_navigated, p16, blob, nt, xi, sg, su, gu, gt, smax, fu, ft, E_FT, xn, sn, **kw)
                            call(t + "/history_navigated", hr.history, p16, blob, nt, xi, sg, su, gu, gt, smax, fu, ft, E_FT, xn, sn, **kw)
                            for dn, (phi, qq, o) in dict(none=(None, None, None), frozen=(np.ones(8), np.zeros(8), np.full((8, K, S), np.nan)),
                                                         mixed=(PHI, Q, om)).items():
                                call(f"{t}/drifting_{dn}", nd.history_drifting, p16, blob, nt, xi, sg, su, gu, gt, smax, fu, ft, E_FT, xn,
                                     SIGMA_NAV, phi, qq, o, **kw)
                    # partial argument lists
                    t = f"{tag}/q{q:g}"
                    call(t + "/navigated_no_nav", ffr.disperse_navigated, p16, blob, nt, xi, sigma, None, gu, gt, 0.5, fu, ft, E_FT, **kw)
                    call(t + "/navigated_no_ff", ffr.disperse_navigated, p16, blob, nt, xi, sigma, su, gu, None, 0.5, None, None, None, xn, sn, **kw)
                    call(t + "/drifting_no_nav", nd.history_drifting, p16, blob, nt, xi, sigma, None, gu, gt, 0.5, fu, ft, E_FT, None, None, PHI, Q, om, **kw)
                    # a blob whose t_f is not finite
                    for bn, b in (("nan", nanblob), ("inf", infblob)):
                        call(f"{t}/{bn}blob/guided", gr.disperse_guided, p16, b, nt, xi, sigma, su, gu, gt, 0.5, **kw)
                        call(f"{t}/{bn}blob/history", hr.history, p16, b, nt, xi, sigma, su, gu, gt, 0.5, **kw)
                        call(f"{t}/{bn}blob/navigated", ffr.disperse_navigated, p16, b, nt, xi, sigma, su, gu, gt, 0.5, fu, ft, E_FT, xn, sn, **kw)
                        call(f"{t}/{bn}blob/drifting", nd.history_drifting, p16, b, nt, xi, sigma, su, gu, gt, 0.5, fu, ft, E_FT, xn, SIGMA_NAV, PHI, Q,
                             om, **kw)
                    # the flights themselves, sample by sample
                    noise = su[:, None] * xi[24:24 + K]
                    if nodes is None:
                        continue
                    for s in range(S):
                        p, z0, _, ts = dr.perturbed(p16, us, tf, xi, big, None, s)
                        if not np.isfinite(ts):
                            ts = tf
                        a = (p, z0, us, noise[:, s], ts, m, nodes, gu, gt, 0.5)
                        call(f"{t}/s{s}/fly_guided", fly_guided, *a, form, dtype)
                        call(f"{t}/s{s}/fly_guided_nostretch", fly_guided, *a[:8], None, 0.5, form, dtype)
                        call(f"{t}/s{s}/fly_navigated", fly_navigated, *a, fu, ft, 0.3 * p16[3] * 1e-3, xn[:7, s] * 1e-6, np.arange(7) != 2, form, dtype)
                        call(f"{t}/s{s}/fly_navigated_noff", fly_navigated, *a, None, None, 0.0, np.zeros(7), np.zeros(7, dtype=bool), form, dtype)
                        call(f"{t}/s{s}/fly_history", hr.fly_history, *a, fu, ft, 0.3 * p16[3] * 1e-3, xn[:7, s] * 1e-6, np.arange(7) != 2, form, dtype)
                        call(f"{t}/s{s}/fly_history_open", hr.fly_history, *a[:7], formulation=form, dtype=dtype)
                        thk = (r.standard_normal(K) * 1e-3 * p16[3]).astype(dtype)
                        nuk = (np.random.default_rng(s).standard_normal((K, 7)) * 1e-6).astype(dtype)
                        call(f"{t}/s{s}/fly_drifting", fly_drifting, *a, fu, ft, thk, nuk, np.arange(7) != 2, form, dtype)
                        call(f"{t}/s{s}/fly_drifting_none", fly_drifting, *a, fu, ft, None, None, None, form, dtype)
                # the covariance corridors
                rec = gr.records(p16, blob, nt, form, 2, dtype)
                sg = np.full(24, 1e-6)
                for kind in ("open", "guided", "navigated", "ff_without_stretch", "ff_without_gains"):
                    gu, gt, fu, ft = laws[1e6]
                    law = dict(open={}, guided=dict(gain_u=gu, gain_t=gt, smax=0.5),
                               navigated=dict(gain_u=gu, gain_t=gt, smax=0.5, ff_u=fu, ff_t=ft, know=E_FT),
                               ff_without_stretch=dict(gain_u=gu, gain_t=gt, smax=0.0, ff_u=fu, ff_t=ft, know=E_FT),
                               ff_without_gains=dict(ff_u=fu, ff_t=ft, know=E_FT, gain_t=gt, smax=0.5))[kind]
                    t = f"{tag}/corridor/{kind}"
                    call(t + "/plain", lr.corridor, p16, blob, nt, sg, su, sigma_nav=SIGMA_NAV, rec=rec, **kw, **law)
                    call(t + "/bare", lr.corridor, p16, blob, nt, np.zeros(24), rec=rec, **kw, **law)
                    call(t + "/own_rec", lr.corridor, p16, blob, nt, sg, su, **kw, **law)
                    for dn, (phi, qq) in dict(none=(None, None), frozen=(np.ones(8), np.zeros(8)), mixed=(PHI, Q)).items():
                        call(f"{t}/drifting_{dn}", nd.corridor_drifting, p16, blob, nt, sg, su, sigma_nav=SIGMA_NAV, phi=phi, q=qq, rec=rec, **kw, **law)
                    call(t + "/drifting_bare", nd.corridor_drifting, p16, blob, nt, np.zeros(24), None, phi=PHI, q=Q, **kw, **law)
    return OUT


def compare(a, b, out):
    A, B = (json.load(open(f)) for f in (a, b))
    differ = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
    kinds = {"arrays": 0, "exceptions": 0, "none": 0}
    for v in A.values():
        kinds[{"raises": "exceptions", "None": "none"}.get(v[0], "arrays")] += 1
    groups = {}
    for k in A:
        g = "/".join(k.split("/")[:3])
        groups[g] = groups.get(g, 0) + 1
    res = dict(_comment="scripts/reference_flight_dump.py --compare: sha256 of the bytes of every array the closed-loop CPU references return "
               "(dtype and shape included), the parent commit's tests/ against this tree's, both on one machine", entries=len(A), **kinds,
               differ=len(differ), differing=differ[:50], entries_per_group=groups)
    print(json.dumps({k: v for k, v in res.items() if k != "entries_per_group"}, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    return 1 if differ or len(A) != len(B) else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--tests", default=os.path.join(ROOT, "tests"))
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.json))
    sys.path[:0] = [ROOT, args.tests]
    import dispersion_reference as dr
    import feedforward_reference as ffr
    import flight_reference as fr
    import guidance_reference as gr
    import history_reference as hr
    import lincov_reference as lr
    import navdrift_reference as nd
    from oracle.ascent_numpy import Params
    with np.errstate(all="ignore"):
        main()
    with open(args.out, "w") as f:
        json.dump(OUT, f)
    print(len(OUT), "entries written")
