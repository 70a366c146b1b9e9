"""tests/golden/analysis_arg_errors.json: what the nine calls on a solution blob (ascent_param_sensitivity ... ascent_disperse_navigated_batch)
answer to a call with exactly one defect -- return code and ascent_strerror text -- as the library built from the current tree
gives them.  Written by the library before the nine entry points were moved onto one host path; tests/test_analysis_host.py replays
the table against whatever is built now.

Only defects that are refused before the device is looked at are in the table (the answer to a bad device_id depends on how
many devices there are), so it reads the same with or without a GPU.  The file describes every call completely (argument order,
which pointers are null, which scalars and options differ from the good call), so the test needs nothing from this script.

    python scripts/make_analysis_arg_errors.py [--out tests/golden/analysis_arg_errors.json]
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

NT, BATCH, SAMPLES = 18, 2, 4
HEAD = ["p", "batch", "o", "sol_blob"]
TAIL = ["device_id", "stream", "ptr_is_device"]
DISP = ["substeps", "samples", "xi", "sigma", "sigma_u"]
SIGNATURES = {
    "ascent_param_sensitivity": HEAD + ["grad_out"] + TAIL,
    "ascent_fly_batch": HEAD + ["substeps", "flown_traj", "local_err", "summary"] + TAIL,
    "ascent_flight_jacobian": HEAD + ["substeps", "jac_out", "jac_u_out"] + TAIL,
    "ascent_trim_batch": HEAD + ["substeps", "rounds", "tol", "trim_blob_out", "summary_out"] + TAIL,
    "ascent_disperse_batch": HEAD + DISP + ["stats_out", "samples_out"] + TAIL,
    "ascent_guidance_gains": HEAD + ["substeps", "weights", "gain_u_out", "gain_t_out", "summary_out", "jac_cl_out", "jac_u_cl_out"] + TAIL,
    "ascent_disperse_guided_batch": HEAD + DISP + ["gain_u", "gain_t", "stretch_max", "stats_out", "samples_out"] + TAIL,
    "ascent_guidance_feedforward": HEAD + ["substeps", "weights", "ff_dir", "ff_know", "gain_u_out", "gain_t_out", "ff_u_out", "ff_t_out",
                                           "summary_out", "jac_cl_out", "jac_u_cl_out", "jac_nav_out"] + TAIL,
    "ascent_disperse_navigated_batch": HEAD + DISP + ["gain_u", "gain_t", "stretch_max", "ff_u", "ff_t", "ff_know", "xi_nav", "sigma_nav",
                                                      "stats_out", "samples_out"] + TAIL,
}
# the good call's scalars; every other argument is a pointer to a buffer of its own
SCALARS = {"batch": BATCH, "substeps": 0, "samples": SAMPLES, "rounds": 0, "tol": 0.0, "device_id": 0, "stream": None, "ptr_is_device": 0}
OPTS = dict(n_nodes=NT, scheme=0, max_iter=0, warm_start=0, tol=1.0, mu_init=0.0)
REQUIRED = {
    "ascent_param_sensitivity": ["grad_out"],
    "ascent_fly_batch": ["summary"],
    "ascent_flight_jacobian": ["jac_out"],
    "ascent_trim_batch": ["trim_blob_out", "summary_out"],
    "ascent_disperse_batch": ["xi", "sigma", "stats_out"],
    "ascent_guidance_gains": ["weights", "gain_u_out", "gain_t_out", "summary_out"],
    "ascent_disperse_guided_batch": ["xi", "sigma", "gain_u", "stats_out"],
    "ascent_guidance_feedforward": ["weights", "gain_u_out", "gain_t_out", "summary_out", "ff_dir", "ff_u_out", "ff_t_out"],
    "ascent_disperse_navigated_batch": ["xi", "sigma", "gain_u", "stats_out"],
}
REFUSES_TERMINAL_2 = ("ascent_flight_jacobian", "ascent_trim_batch", "ascent_guidance_gains", "ascent_guidance_feedforward")
BUF_DOUBLES = 4096      # more than the largest array of a call at NT, BATCH, SAMPLES (the blob: 367 x 2)


def defects(entry):
    """(label, null pointers, changed scalars, changed options, dcost of the last problem or None) of every one-defect call"""
    sig = SIGNATURES[entry]
    for name in ["p", "o", "sol_blob"] + REQUIRED[entry]:
        yield f"null {name}", [name], {}, {}, None
    yield "batch 0", [], {"batch": 0}, {}, None
    yield "scheme 7", [], {}, {"scheme": 7}, None
    yield "move_penalty with dcost 0", [], {}, {"move_penalty": 1}, 0.0
    if "samples" in sig:
        yield "samples 0", [], {"samples": 0}, {}, None
        yield "samples too large", [], {"samples": 65537}, {}, None
    if "substeps" in sig:
        yield "substeps -1", [], {"substeps": -1}, {}, None
        yield "substeps too large", [], {"substeps": 4097}, {}, None
    if "rounds" in sig:
        yield "rounds 33", [], {"rounds": 33}, {}, None
    if entry in REFUSES_TERMINAL_2:
        yield "terminal 2", [], {}, {"terminal": 2}, None
    if "jac_u_cl_out" in sig:
        yield "jac_u_cl_out without jac_cl_out", ["jac_cl_out"] + (["jac_nav_out"] if "jac_nav_out" in sig else []), {}, {}, None
    if "jac_nav_out" in sig:
        yield "jac_nav_out without jac_cl_out", ["jac_cl_out", "jac_u_cl_out"], {}, {}, None
        yield "jac_cl_out without ff_know", ["ff_know"], {}, {}, None
    if "xi_nav" in sig:
        yield "xi_nav without sigma_nav", ["sigma_nav"], {}, {}, None
        yield "sigma_nav without xi_nav", ["xi_nav"], {}, {}, None
        yield "ff_know without ff_u", ["ff_u"], {}, {}, None


def call(lib, entry, sig, null, scalars, opts, dcost):
    """One call as the table describes it; returns (return code, error text)."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    P = np.vstack([A.AscentParams().as_row()] * BATCH)
    if dcost is not None:
        P[-1, 15] = dcost
    o = _lib.AscentOptsC(**dict(OPTS, **opts))
    keep, args = [P], []
    for name in sig:
        if name in null:
            args.append(None)
        elif name == "p":
            args.append(P.ctypes.data_as(C.c_void_p))
        elif name == "o":
            args.append(C.byref(o))
        elif name in SCALARS:
            args.append(scalars.get(name, SCALARS[name]))
        else:
            keep.append(np.full(BUF_DOUBLES, 7.25))
            args.append(keep[-1].ctypes.data_as(C.c_void_p))
    rc = getattr(lib, entry)(*args)
    return int(rc), lib.ascent_strerror(rc).decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "analysis_arg_errors.json"))
    a = ap.parse_args()
    from lunar_module_ascent_trajectory_optimiser_amd import _lib, build
    build.build()
    lib = _lib.load()
    cases = []
    for entry, sig in SIGNATURES.items():
        for label, null, scalars, opts, dcost in defects(entry):
            rc, msg = call(lib, entry, sig, null, scalars, opts, dcost)
            assert rc == -1, (entry, label, rc, msg)       # ASCENT_E_ARG: anything else got as far as the device
            cases.append({"entry": entry, "defect": label, "null": null, "scalars": scalars, "opts": opts, "dcost": dcost, "rc": rc,
                          "message": msg})
    doc = {"_comment": "made by scripts/make_analysis_arg_errors.py from the library as it was before the nine entry points shared one "
                       "host path: one defect per call, the return code and the ascent_strerror text; every call is refused before the "
                       "device is looked at",
           "nt": NT, "batch": BATCH, "samples": SAMPLES, "buffer_doubles": BUF_DOUBLES, "good_scalars": SCALARS, "good_opts": OPTS,
           "signatures": SIGNATURES, "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{len(cases)} cases -> {a.out}")


if __name__ == "__main__":
    main()
