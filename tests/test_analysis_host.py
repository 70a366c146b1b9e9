"""The argument checks of the nine calls on a solution blob (include/ascent.h: ascent_param_sensitivity, ascent_fly_batch,
ascent_flight_jacobian, ascent_trim_batch, ascent_disperse_batch, ascent_guidance_gains, ascent_disperse_guided_batch,
ascent_guidance_feedforward, ascent_disperse_navigated_batch) against tests/golden/analysis_arg_errors.json
(scripts/make_analysis_arg_errors.py, written by the library before the nine shared one host path).  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analysis_arg_errors.json")


@pytest.fixture(scope="module")
def lib():
    from lunar_module_ascent_trajectory_optimiser_amd import _lib, build
    build.build()
    return _lib.load()


def test_one_defect_gives_the_recorded_code_and_text(lib):
    """Every call of the table has exactly one defect and is refused before the device is looked at: the same return code and the
    same ascent_strerror text with or without a GPU, and none of its arrays touched."""
    import lunar_module_ascent_trajectory_optimiser_amd as A
    from lunar_module_ascent_trajectory_optimiser_amd import _lib
    doc = json.load(open(GOLDEN))
    assert len(doc["signatures"]) == 9 and set(doc["signatures"]) <= set(_lib.SYMBOLS)
    assert len(doc["cases"]) >= 9 * 8
    for case in doc["cases"]:
        sig = doc["signatures"][case["entry"]]
        assert len(sig) == len(getattr(lib, case["entry"]).argtypes), case["entry"]
        P = np.vstack([A.AscentParams().as_row()] * doc["batch"])
        if case["dcost"] is not None:
            P[-1, 15] = case["dcost"]
        o = _lib.AscentOptsC(**dict(doc["good_opts"], **case["opts"]))
        buffers, args = [], []
        for name in sig:
            if name in case["null"]:
                args.append(None)
            elif name == "p":
                args.append(P.ctypes.data_as(C.c_void_p))
            elif name == "o":
                args.append(C.byref(o))
            elif name in doc["good_scalars"]:
                args.append(case["scalars"].get(name, doc["good_scalars"][name]))
            else:
                buffers.append(np.full(doc["buffer_doubles"], 7.25))
                args.append(buffers[-1].ctypes.data_as(C.c_void_p))
        rc = getattr(lib, case["entry"])(*args)
        msg = lib.ascent_strerror(rc).decode()
        assert (rc, msg) == (case["rc"], case["message"]), (case["entry"], case["defect"], rc, msg)
        assert all((b == 7.25).all() for b in buffers), (case["entry"], case["defect"])
