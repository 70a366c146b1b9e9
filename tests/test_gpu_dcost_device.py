"""The move-penalty weight of device-resident parameters is validated on the device (p_init / p_transfer, d_init): a problem whose
dcost is zero, negative or NaN comes back with status 4 (ASCENT_INVALID_PROBLEM), 0 iterations and its finite starting point, the
other problems of the batch are solved to the bits they have without it, and solve_batch_torch(move_penalty=True) reads nothing
back to the host.  Grids 14 -> 41, so that p_transfer carries the refusal to the finer grid.  (One child process for all cases:
torch has to bring up its HIP runtime before the library binds to one.)"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import os, sys, numpy as np, torch
torch.cuda.set_device(0)
sys.path.insert(0, %r)
import lunar_module_ascent_trajectory_optimiser_amd as A
dev = torch.device("cuda", 0)
NT = 41
S = A.sweep_isp_drymass(4, 2)
assert S.shape == (8, 16)
S[:, 15] = 1e-5
BAD = {1: 0.0, 4: -1e-5, 6: float("nan")}
for i, w in BAD.items():
    S[i, 15] = w
GOOD = [i for i in range(8) if i not in BAD]

def run(P, **kw):
    o = A.solve_batch_torch(torch.from_numpy(np.ascontiguousarray(P)).to(dev), NT, tol=1e-9, max_iter=500, move_penalty=True,
                            want_blob=True, sync=True, **kw)
    return {k: v.cpu().numpy() for k, v in o.items()}

def check(name, full, alone, bad, good):
    for k in ("tf", "traj", "blob"):
        assert np.isfinite(full[k][..., bad]).all(), (name, k)
    assert np.all(full["status"][bad] == 4) and np.all(full["iters"][bad] == 0), (name, full["status"], full["iters"])
    assert np.all(alone["status"] == 0), (name, alone["status"])
    for k in ("tf", "status", "iters", "traj", "blob"):
        a, b = np.ascontiguousarray(full[k][..., good]), np.ascontiguousarray(alone[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (name, k)
    print(name + "-ok")

for wide in ("0", "1"):
    os.environ["ASCENT_PERSIST_WIDE"] = wide
    assert A.default_path(8, NT, move_penalty=True) == "persist"
    check("persist-wide" + wide, run(S), run(S[GOOD]), sorted(BAD), GOOD)
del os.environ["ASCENT_PERSIST_WIDE"]
assert A.default_path(4, NT, scheme=2, move_penalty=True) == "dense"
D = S[[0, 1, 4, 6]]
check("dense", run(D, scheme=2), run(D[[0]], scheme=2), [1, 2, 3], [0])

# enqueue-only: no host read in solve_batch_torch, good weights or bad (a caller stream: the library waits for nothing either)
Pg, Pb = torch.from_numpy(np.ascontiguousarray(S[GOOD])).to(dev), torch.from_numpy(S).to(dev)
st = torch.cuda.Stream(dev)
torch.cuda.synchronize(dev)
torch.cuda.set_sync_debug_mode("error")
try:
    with torch.cuda.stream(st):
        og = A.solve_batch_torch(Pg, NT, tol=1e-9, max_iter=500, move_penalty=True)
        ob = A.solve_batch_torch(Pb, NT, tol=1e-9, max_iter=500, move_penalty=True)
finally:
    torch.cuda.set_sync_debug_mode("default")
torch.cuda.synchronize(dev)
assert og["status"].cpu().tolist() == [0] * 5 and ob["status"].cpu().tolist() == [4 if i in BAD else 0 for i in range(8)]
print("launch-only-ok")
"""

CASES = ("persist-wide0", "persist-wide1", "dense", "launch-only")


@pytest.fixture(scope="module")
def child():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([sys.executable, "-c", _SCRIPT % root], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("case", CASES)
def test_bad_weights_are_refused_on_the_device(child, case):
    assert case + "-ok" in child.stdout, child.stdout[-2000:] + child.stderr[-3000:]


def test_child_ran_to_the_end(child):
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-3000:]
