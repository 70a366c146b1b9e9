"""Writes tests/golden/route_table.json: the path code ascent_default_path returns over a grid of batch sizes, grids, options and
routing overrides (the environment variables the C ABI reads when it picks a kernel family).  tests/test_host.py compares the
library against it, so that a refactor of the dispatcher cannot move a route unnoticed.

    python scripts/make_route_table.py [path/to/libascent.so]      (default: the in-tree library)

No device work: ascent_default_path only decides."""
from __future__ import annotations

import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lunar_module_ascent_trajectory_optimiser_amd import _lib  # noqa: E402

AXES = {
    "batch": [1, 6, 7, 1024, 1025, 4096, 4097, 24576, 24577],
    "n_nodes": [201, 401, 2000],
    "scheme": [0, 1, 2],
    "formulation": [0, 1],
    "move_penalty": [0, 1],
    "terminal": [0, 1, 2],
    "solver_path": [_lib.PATHS["auto"], _lib.PATHS["dense"]],
}
ENV = [{}, {"ASCENT_PIPELINE": "persist"}, {"ASCENT_PIPELINE": "split"}, {"ASCENT_PIPELINE": "fused"},
       {"ASCENT_PIPELINE": "dense"}, {"ASCENT_FACTOR": "wide"}, {"ASCENT_FACTOR": "lane"},
       {"ASCENT_PIPELINE": "split", "ASCENT_FACTOR": "lane"}, {"ASCENT_SMALL_BATCH": "off"},
       {"ASCENT_DENSE_NEWTON": "pcr"}, {"ASCENT_DENSE_NEWTON": "riccati"}]
ROUTING_VARS = sorted({k for e in ENV for k in e})


def route_codes(lib, axes=AXES, envs=ENV):
    """Path codes in the order env, then the axes in their listed order (the last one fastest)."""
    f = lib.ascent_default_path
    f.restype, f.argtypes = C.c_int, [C.c_int64, C.POINTER(_lib.AscentOptsC)]
    saved = {k: os.environ.get(k) for k in ROUTING_VARS}
    out = []
    try:
        for env in envs:
            for k in ROUTING_VARS:
                os.environ.pop(k, None)
            os.environ.update(env)
            for b, nn, sc, fo, mp, te, sp in itertools.product(*axes.values()):
                o = _lib.AscentOptsC(n_nodes=nn, scheme=sc, max_iter=300, warm_start=0, tol=1e-9, mu_init=0.0, formulation=fo,
                                     coarse_nodes=0, terminal=te, solver_path=sp, move_penalty=mp, reserved=0)
                out.append(f(b, C.byref(o)))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


if __name__ == "__main__":
    lib = C.CDLL(sys.argv[1] if len(sys.argv) > 1 else _lib.LIB_PATH)
    codes = route_codes(lib)
    dst = os.path.join(ROOT, "tests", "golden", "route_table.json")
    with open(dst, "w") as fh:
        json.dump({"axes": AXES, "env": ENV, "paths": codes}, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{dst}: {len(codes)} entries")
