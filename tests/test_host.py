"""CPU tests of the host logic and of the C-ABI library surface (no compute without a GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lunar_module_ascent_trajectory_optimiser_amd as A
from lunar_module_ascent_trajectory_optimiser_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()          # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_library_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "ascent.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(ascent_[a-z_]+)\s*\(", hdr))
    assert {"ascent_solve_batch", "ascent_eval_nodes", "ascent_kkt_step", "ascent_version",
            "ascent_device_count", "ascent_strerror", "ascent_last_kernel_ms"} <= names
    for n in names:
        assert hasattr(lib, n), n
    assert set(_lib.SYMBOLS) == names
    assert lib.ascent_version() >= 100


def test_struct_layouts_match_header():
    assert C.sizeof(_lib.AscentParamsC) == 16 * 8
    assert C.sizeof(_lib.AscentOptsC) == 56 and [f[0] for f in _lib.AscentOptsC._fields_][-2:] == ["move_penalty", "reserved"]
    assert tuple(n for n, _ in _lib.AscentParamsC._fields_) == A.PARAM_FIELDS


def test_params_defaults_are_the_reference_constants():
    p = A.AscentParams()      # /root/reference/Launch_Optimiser.py:38-75
    assert (p.G, p.M, p.R0, p.Ft, p.M0, p.mdot, p.fuel_mass) == (6.674e-11, 7.346e22, 1738100.0, 15346.0, 4821.0, 5.053, 2376.0)
    assert (p.ang_acc_max, p.r_peri, p.r_apo, p.T_scale) == (5e-4, 17703.0, 88615.0, 470.0)
    assert abs(p.periapsis_v - 1654.3956154295) < 1e-6
    assert A.blob_rows(200) == 21 * 199 + 10


def test_sweeps_shapes_and_ranges():
    S = A.sweep_isp_drymass()
    assert S.shape == (4096, 16)
    f = A.PARAM_FIELDS
    isp = S[:, f.index("Ft")] / (S[:, f.index("mdot")] * 9.80665)
    assert abs(isp.min() - 300) < 1e-9 and abs(isp.max() - 320) < 1e-9
    dry = S[:, f.index("M0")] - S[:, f.index("fuel_mass")]
    assert dry.min() == 2345 and dry.max() == 2545
    S4 = A.sweep_config4(4, 4, 8, 8)
    assert S4.shape == (4 * 4 * 64, 16)
    assert abs(S4[:, f.index("r_apo")].min() - 70e3) < 1e-6 and abs(S4[:, f.index("r_apo")].max() - 105e3) < 1e-6
    assert abs(S4[:, f.index("ang_acc_max")].min() - 3e-4) < 1e-12
    # the full config-4 grid is 262 144 problems
    assert 64 * 64 * 8 * 8 == 262144


def test_product_fails_loudly_without_gpu(lib):
    """No CPU fallback: without a device the solve raises instead of silently computing elsewhere."""
    if lib.ascent_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.AscentLibraryError):
        A.solve_batch(A.AscentParams())


def test_argument_validation(lib):
    o = _lib.AscentOptsC(n_nodes=200, scheme=0, max_iter=10, warm_start=0, tol=1e-8, mu_init=0.0)
    assert lib.ascent_solve_batch(None, 1, C.byref(o), None, None, None, None, None, None, 0, None, 0) == -1
    assert b"null" in lib.ascent_strerror(-1)
    P = A.AscentParams().as_row()
    o2 = _lib.AscentOptsC(n_nodes=200, scheme=7, max_iter=10, warm_start=0, tol=1e-8, mu_init=0.0)
    rc = lib.ascent_solve_batch(P.ctypes.data_as(C.c_void_p), 1, C.byref(o2), None, None, None, None, None, None, 0, None, 0)
    assert rc == -1 and b"scheme" in lib.ascent_strerror(rc)
    for bad in (1, 2, 200, 500, -2):          # coarse grid of the nested iteration: -1, 0 or 3 .. n_nodes-1
        o3 = _lib.AscentOptsC(n_nodes=200, scheme=0, max_iter=10, warm_start=0, tol=1e-8, mu_init=0.0, coarse_nodes=bad)
        rc = lib.ascent_solve_batch(P.ctypes.data_as(C.c_void_p), 1, C.byref(o3), None, None, None, None, None, None, 0, None, 0)
        assert rc == -1 and b"coarse_nodes" in lib.ascent_strerror(rc)
    o4 = _lib.AscentOptsC(n_nodes=200, scheme=0, max_iter=10, warm_start=0, tol=1e-8, mu_init=0.0, move_penalty=2)
    rc = lib.ascent_solve_batch(P.ctypes.data_as(C.c_void_p), 1, C.byref(o4), None, None, None, None, None, None, 0, None, 0)
    assert rc == -1 and b"move_penalty" in lib.ascent_strerror(rc)
    # (the move penalty with the v1 formulation lives in the persistent kernel only; terminal 2 has the current formulation only)
    o5 = _lib.AscentOptsC(n_nodes=200, scheme=0, max_iter=10, warm_start=0, tol=1e-8, mu_init=0.0, move_penalty=1, formulation=1, solver_path=4)
    rc = lib.ascent_solve_batch(P.ctypes.data_as(C.c_void_p), 1, C.byref(o5), None, None, None, None, None, None, 0, None, 0)
    assert rc == -1 and b"formulation 0" in lib.ascent_strerror(rc)
    o6 = _lib.AscentOptsC(n_nodes=200, scheme=0, max_iter=10, warm_start=0, tol=1e-8, mu_init=0.0, terminal=2, formulation=1)
    rc = lib.ascent_solve_batch(P.ctypes.data_as(C.c_void_p), 1, C.byref(o6), None, None, None, None, None, None, 0, None, 0)
    assert rc == -1 and b"terminal 2" in lib.ascent_strerror(rc)
    o7 = _lib.AscentOptsC(n_nodes=200, scheme=0, max_iter=10, warm_start=0, tol=1e-8, mu_init=0.0, terminal=3)
    rc = lib.ascent_solve_batch(P.ctypes.data_as(C.c_void_p), 1, C.byref(o7), None, None, None, None, None, None, 0, None, 0)
    assert rc == -1 and b"terminal" in lib.ascent_strerror(rc)


def test_product_does_not_import_oracle():
    """The product package must never route through oracle/ (test infrastructure only)."""
    pkg = os.path.join(ROOT, "lunar_module_ascent_trajectory_optimiser_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                src = open(os.path.join(dirpath, fn)).read()
                assert "oracle" not in src.replace("# oracle-free", ""), fn


def test_default_path_dispatch_rule(monkeypatch):
    """ascent_default_path (include/ascent.h): which kernels a solve of that size runs -- no device work, so checked here.
    Schemes 0 and 1 and the v1 formulation: the persistent kernel, except (formulation 0) a handful of NLPs on a long grid
    (>= 400 intervals, batch <= min(6, intervals/300)), which take the dense blocks + PCR; scheme 2 (Hermite-Simpson): its own
    persistent kernel by the same rule, dense blocks with the move penalty.  The move penalty (ascent_opts.move_penalty, the
    reference's DCOST) rides in the persistent kernel for schemes 0 and 1."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    for k in ("ASCENT_PIPELINE", "ASCENT_FACTOR", "ASCENT_SMALL_BATCH", "ASCENT_DENSE_NEWTON"):
        monkeypatch.delenv(k, raising=False)
    assert [A.default_path(b, 201) for b in (1, 9, 4096, 32768, 262144)] == ["persist"] * 5
    assert [A.default_path(b, 2000) for b in (1, 6, 7)] == ["dense", "dense", "persist"]
    assert [A.default_path(b, 401) for b in (1, 2)] == ["dense", "persist"] and [A.default_path(b, 1000) for b in (3, 4)] == ["dense", "persist"]
    assert [A.default_path(b, 201, scheme=1) for b in (1, 8, 4096, 65536)] == ["persist"] * 4
    assert [A.default_path(b, 2000, scheme=1) for b in (6, 7)] == ["dense", "persist"]
    assert [A.default_path(b, 201, formulation=1) for b in (1, 4096, 8192)] == ["persist"] * 3 and A.default_path(4, 2000, formulation=1) == "persist"
    assert [A.default_path(b, 201, scheme=2) for b in (1, 256, 4096, 65536)] == ["persist"] * 4
    assert [A.default_path(b, 2000, scheme=2) for b in (1, 6, 7, 256)] == ["dense", "dense", "persist", "persist"]
    assert [A.default_path(b, 201, scheme=sc, move_penalty=True) for b in (1, 4096) for sc in (0, 1, 2)] == ["persist", "persist", "dense"] * 2     # the l1 move penalty
    assert A.default_path(4096, 201, move_penalty=True) == "persist" and A.default_path(2, 2000, move_penalty=True) == "dense"
    assert A.default_path(1, 2000) == "dense"
    monkeypatch.setenv("ASCENT_SMALL_BATCH", "off")
    assert A.default_path(1, 2000) == "persist"
    monkeypatch.setenv("ASCENT_PIPELINE", "split")
    assert A.default_path(4096, 201) == "split_wide"
    assert A.default_path(4096, 201, move_penalty=True) == "dense"        # (the split pipeline does not carry the penalty)
    assert A.default_path(4096, 201, scheme=2) == "dense"                  # (... nor Hermite-Simpson)


def test_default_path_matches_route_table(lib, monkeypatch):
    """ascent_default_path over batch sizes on both sides of every threshold it shows (6 NLPs, 400 intervals, 4096, 24576), all
    option combinations and the routing overrides, against tests/golden/route_table.json (scripts/make_route_table.py, written by
    the library before its routing moved into one function)."""
    import itertools
    import json
    with open(os.path.join(ROOT, "tests", "golden", "route_table.json")) as f:
        table = json.load(f)
    f = lib.ascent_default_path
    routing = sorted({k for env in table["env"] for k in env})
    got = []
    for env in table["env"]:
        for k in routing:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for b, nn, sc, fo, mp, te, sp in itertools.product(*table["axes"].values()):
            o = _lib.AscentOptsC(n_nodes=nn, scheme=sc, max_iter=300, warm_start=0, tol=1e-9, mu_init=0.0, formulation=fo,
                                 coarse_nodes=0, terminal=te, solver_path=sp, move_penalty=mp, reserved=0)
            got.append(f(b, C.byref(o)))
    assert len(got) == len(table["paths"])
    bad = [i for i, (g, w) in enumerate(zip(got, table["paths"])) if g != w]
    assert not bad, f"{len(bad)} routes differ from the table, first at entry {bad[0]}: {got[bad[0]]} instead of {table['paths'][bad[0]]}"


def test_persistent_workspace_regions_fit_the_allocation(lib):
    """The two workspace regions of the persistent kernel's nested iteration (levels alternate between them) lie inside the
    allocation for every batch and grid combination -- the second region starts at a 256-byte boundary behind the first, and
    the last NLP's record of the largest level living there ends before the allocation does (round 2's layout allocated the
    unaligned sum and overran by up to 255 bytes).  With and without the move penalty's five extra rows."""
    out = (C.c_int64 * 4)()
    for mp in (0, 1):
        for nt in (40, 60, 200, 201, 600, 2000):
            for batch in (1, 3, 4, 5, 63, 4096, 32768, 262144):
                o = _lib.AscentOptsC(n_nodes=nt, scheme=0, max_iter=10, warm_start=0, tol=1e-8, mu_init=0.0, move_penalty=mp)
                nlev = lib.ascent_workspace_layout(batch, C.byref(o), out)
                total, used0, off1, used1 = out
                assert nlev >= 2 and used0 > 0 and used1 > 0
                assert used0 <= off1 and off1 % 256 == 0 and off1 + used1 <= total, (mp, nt, batch, list(out))
                # every NLP's record is a whole number of 128-byte lines (its node rows are padded to 16 nodes, its scalar record to 64
                # doubles): a 16-node row of any NLP is ONE cache line, not two
                assert used0 % batch == 0 and (used0 // batch) % 128 == 0 and used1 % batch == 0 and (used1 // batch) % 128 == 0, (mp, nt, batch, list(out))
    o = _lib.AscentOptsC(n_nodes=200, scheme=0, max_iter=10, warm_start=0, tol=1e-8, mu_init=0.0, coarse_nodes=-1)
    assert lib.ascent_workspace_layout(7, C.byref(o), out) == 1 and out[1] <= out[0] and out[2] == 0


def test_one_hip_runtime_per_process(lib):
    """libascent.so and PyTorch-ROCm each ship / need a libamdhip64; the package maps the one torch will use before it loads
    libascent.so, so that a later `import torch` does not bring a second runtime into the process (device pointers and
    streams of one are meaningless to the other) -- VERDICT r02 weak 7."""
    import subprocess, sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from lunar_module_ascent_trajectory_optimiser_amd import _lib\n"
            "_lib.load(); a = _lib.hip_runtimes_mapped()\n"
            "import torch; b = _lib.hip_runtimes_mapped()\n"
            "_lib.require_single_hip_runtime(); print(len(a), len(b))\n") % ROOT
    env = {k: v for k, v in os.environ.items() if k != "ASCENT_HIP_RUNTIME"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["1", "1"]
    env["ASCENT_HIP_RUNTIME"] = "system"      # the explicit opt-out: the device-pointer entry points then refuse
    code2 = code.replace("_lib.require_single_hip_runtime(); print(len(a), len(b))",
                         "\ntry:\n    _lib.require_single_hip_runtime(); print('no error')\nexcept _lib.AscentLibraryError as e:\n    print('refused' if 'two HIP runtimes' in str(e) else e)")
    out = subprocess.run([sys.executable, "-c", code2], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "refused", (out.stdout, out.stderr)


# The five entry points that work on a solve's results: (name, call(lib, a, o, **changes)) where `a` holds the pointers of one
# complete call (a changed entry replaces its pointer or integer) and `o` the options.
def _post_solve_calls():
    def sens(L, a, o): return L.ascent_param_sensitivity(a["p"], a["batch"], o, a["blob"], a["out"], 0, None, 0)
    def fly(L, a, o): return L.ascent_fly_batch(a["p"], a["batch"], o, a["blob"], a["substeps"], a["opt"], a["opt"], a["out"], 0, None, 0)
    def jac(L, a, o): return L.ascent_flight_jacobian(a["p"], a["batch"], o, a["blob"], a["substeps"], a["out"], a["opt"], 0, None, 0)
    def trim(L, a, o): return L.ascent_trim_batch(a["p"], a["batch"], o, a["blob"], a["substeps"], a["rounds"], 0.0, a["out"], a["out2"], 0, None, 0)
    def coast(L, a, o): return L.ascent_coast_batch(a["p"], a["batch"], a["blob"], a["coast_nodes"], a["out"], a["out2"], a["out3"], 0, None, 0)
    return dict(ascent_param_sensitivity=sens, ascent_fly_batch=fly, ascent_flight_jacobian=jac, ascent_trim_batch=trim,
                ascent_coast_batch=coast)


@pytest.mark.parametrize("name", sorted(_post_solve_calls()))
def test_post_solve_entry_points_refuse_bad_arguments_before_the_device(lib, name):
    """Every argument error of the entry points that work on a solve's results is ASCENT_E_ARG with its own message, on a
    machine with or without a GPU: refusals come before the device is looked at.  A refused call touches none of its arrays."""
    call = _post_solve_calls()[name]
    P = np.vstack([A.AscentParams().as_row()] * 2)
    P0 = P.copy()
    P0[1, 15] = 0.0
    arrays = {k: np.full(8, 7.25) for k in ("blob", "out", "out2", "out3", "opt")}
    good = dict({k: v.ctypes.data_as(C.c_void_p) for k, v in arrays.items()}, p=P.ctypes.data_as(C.c_void_p), batch=2, substeps=0,
                rounds=0, coast_nodes=10)
    coast, flight_like = name == "ascent_coast_batch", name in ("ascent_flight_jacobian", "ascent_trim_batch")

    def opts(**kw):
        return C.byref(_lib.AscentOptsC(**dict(dict(n_nodes=50, scheme=0, max_iter=0, warm_start=0, tol=1.0, mu_init=0.0), **kw)))

    def refused(what, o=None, **changes):
        rc = call(lib, dict(good, **changes), opts() if o is None else o)
        msg = lib.ascent_strerror(rc)
        assert rc == -1 and what in msg, (name, changes, rc, msg)

    refused(b"null", p=None)
    refused(b"batch <= 0", batch=0)
    refused(b"null", blob=None)
    refused(b"null", out=None)
    if name == "ascent_trim_batch" or coast:
        refused(b"null", out2=None)
    if coast:
        refused(b"null", out3=None)
        refused(b"coast_nodes", coast_nodes=0)
        refused(b"coast_nodes", coast_nodes=65536)
    else:
        refused(b"null", o=C.POINTER(_lib.AscentOptsC)())
        refused(b"scheme", o=opts(scheme=7))
        refused(b"dcost", o=opts(move_penalty=1), p=P0.ctypes.data_as(C.c_void_p))
    if not coast and name != "ascent_param_sensitivity":
        refused(b"substeps", substeps=-1)
        refused(b"substeps", substeps=4097)
    if name == "ascent_trim_batch":
        refused(b"rounds", rounds=33)
    if flight_like:
        refused(b"terminal 2", o=opts(terminal=2))
    for k, v in arrays.items():
        assert (v == 7.25).all(), k
