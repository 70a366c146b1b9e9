"""The CPU reference of the linear covariance corridor (tests/lincov_reference.py) checked against what it linearises: its S_j
against central differences of history_reference.fly_history, one flight pair per constant, and its noise part against a
brute-force sum over the K execution errors taken as K more constants.  No GPU."""
import numpy as np
import pytest

import guidance_reference as gr
import history_reference as hr
import lincov_reference as lr
from reference_cases import blob as _blob, law as _law, p16 as _p16

NT, K, M = 18, 17, 2
LD = np.longdouble


def _fly(p16, rec, nodes, c, law, form, noise=None):
    """the ten quantities at every node (K, 10), longdouble, of the flight whose 32 constants are c"""
    know = law.get("know")
    th = c[lr.C_E] + (0.0 if know is None else float(np.dot(know, c[lr.C_P:lr.C_TF])))
    h, clipped, _ = hr.fly_history(p16 + c[lr.C_P:lr.C_TF], c[:7], rec["us"], np.zeros(K) if noise is None else noise, rec["tf"] + c[lr.C_TF],
                                   rec["m"], nodes, law.get("gain_u"), law.get("gain_t"), law.get("smax", 0.0), law.get("ff_u"), law.get("ff_t"),
                                   th, c[lr.C_NU:lr.C_E], np.ones(7, dtype=bool), form, LD)
    assert not clipped.any()
    return h


def _column_steps(p16):
    """central-difference steps of the 32 constants: 1e-6 of the field (1e-6 where it is zero), 1e-6 in scaled units, 1e-6 of
    the thrust for the error of theta-hat; each rounded so that p + h is a float64"""
    h = np.full(lr.NC, 1e-6)
    h[lr.C_P:lr.C_TF] = np.where(p16 != 0, 1e-6 * np.abs(p16), 1e-6)
    h[lr.C_P:lr.C_TF] = (p16 + h[lr.C_P:lr.C_TF]) - p16
    h[lr.C_E] = 1e-6 * p16[3]
    return h


@pytest.mark.parametrize("kind", ["open", "guided", "navigated"])
@pytest.mark.parametrize("form", [0, 1])
def test_jacobian_is_the_central_difference_of_the_flight(form, kind):
    """Every entry of S_j, all K nodes, longdouble throughout.  Each entry is taken per unit step of its column and in the scale
    of its row (lincov_reference.row_scales); the central difference at a relative step of 1e-6 carries a truncation error of
    about 1e-12 of the second-order terms, and the bound is 1e-8 of the row's largest such entry (1e-8 absolute where the row is
    smaller than 1).  An unsaturated blob control steers, a saturated one has a zero gain row, so no command clips."""
    p16, blob = _p16(), _blob()
    rec = gr.records(p16, blob, NT, form, M, LD)
    law = _law(kind, rec, p16)
    ref = lr.corridor(p16, blob, NT, np.zeros(24), formulation=form, substeps=M, dtype=LD, rec=rec, **law)
    nodes = gr.nominal_nodes(p16, rec["us"], rec["tf"], rec["m"], form, LD)
    steps = _column_steps(p16)
    fd = np.zeros((K, lr.NQ, lr.NC), dtype=LD)
    for c in range(lr.NC):
        e = np.zeros(lr.NC)
        e[c] = steps[c]
        fd[:, :, c] = (_fly(p16, rec, nodes, e, law, form) - _fly(p16, rec, nodes, -e, law, form)) / (2 * LD(steps[c]))
    scale = lr.row_scales(p16, law.get("gain_u"), law.get("ff_u"), K)[:, :, None] / steps[None, None, :]
    a, b = (ref["S"] / scale).astype(np.float64), (fd / scale).astype(np.float64)
    big = np.maximum(1.0, np.abs(a).max(axis=2, keepdims=True))
    err = float((np.abs(a - b) / big).max())
    print(form, kind, "largest difference", err)
    assert err <= 1e-8
    assert np.all(ref["S"][:, 9] == 0) if kind == "open" else np.any(ref["S"][:, 9] != 0)
    # the nominal rows are the unperturbed flight's
    nom = _fly(p16, rec, nodes, np.zeros(lr.NC), law, form)
    assert np.abs((ref["nominal"][:, :9] - nom[:, :9]).astype(np.float64)).max() <= 1e-15 * p16[9] and np.all(nom[:, 9] == 0)


@pytest.mark.parametrize("kind", ["open", "navigated"])
def test_noise_part_is_the_sum_over_the_execution_errors(kind):
    """N_j by brute force: the execution error of every step as one more constant, its column of d y_j / d eps_k propagated through
    the closed-loop step maps one step at a time, N_j = sum_k sigma_u,k^2 s_jk s_jk' -- no Q.  Float64 against float64, within 1e-12
    of sqrt(N_aa N_bb); and the column of one step against a central difference of the flight.  sigma_u is zero at one step."""
    p16, blob = _p16(), _blob()
    rec = gr.records(p16, blob, NT, 0, M)
    law = _law(kind, gr.records(p16, blob, NT, 0, M, LD), p16)
    su = np.full(K, 1e-3)
    su[5] = 0.0
    sigma = np.zeros(24)
    ref = lr.corridor(p16, blob, NT, sigma, su, formulation=0, substeps=M, rec=rec, **law)
    assert np.array_equal(ref["cov"], ref["noise"])          # all other sigmas are zero
    Ku = law.get("gain_u", np.zeros((K, 7)))
    kt = law.get("gain_t", np.zeros(7)) if law.get("smax", 0.0) > 0 else np.zeros(7)
    brute = np.zeros((K, lr.NQ, lr.NQ))
    cols = np.zeros((K, K, lr.NQ))                           # [k - 1, j - 1]: d y_j / d eps_k
    for k in range(1, K + 1):
        dz = None
        for j in range(k, K + 1):
            ga, _ = lr.altitude_gradient(p16, rec["nodes"][j])
            if j == k:
                dzn, du, corr = rec["g"][j - 1], 1.0, 0.0
            else:
                corr = Ku[j - 1] @ dz
                du = -corr
                dzn = rec["Phi"][j - 1] @ dz + rec["g"][j - 1] * du
                if j == K:
                    dzn = dzn - rec["gamma"] * (kt @ dz)
            dz = dzn
            s = np.concatenate([dz, [ga @ dz, du, corr]])
            cols[k - 1, j - 1] = s
            brute[j - 1] += su[k - 1] ** 2 * np.outer(s, s)
    sd = np.sqrt(np.einsum("jaa->ja", brute))
    den = np.where(sd[:, :, None] * sd[:, None, :] > 0, sd[:, :, None] * sd[:, None, :], 1.0)
    err = float((np.abs(ref["noise"] - brute) / den).max())
    print(kind, "noise part against the brute-force sum", err)
    assert err <= 1e-12
    assert np.array_equal(ref["noise"], ref["noise"].transpose(0, 2, 1)) and np.all(ref["noise"][:, 9, 9] == 0) == (kind == "open")
    # one column against the flight itself: the execution error of step 3
    nodes = gr.nominal_nodes(p16, rec["us"], rec["tf"], rec["m"], 0, LD)
    e = np.zeros(K)
    e[2] = 1e-6
    fd = (_fly(p16, rec, nodes, np.zeros(lr.NC), law, 0, e) - _fly(p16, rec, nodes, np.zeros(lr.NC), law, 0, -e)) / LD(2e-6)
    scale = lr.row_scales(p16, law.get("gain_u"), law.get("ff_u"), K)
    d = np.abs((fd.astype(np.float64)[2:] - cols[2, 2:]) / scale[2:])
    assert d.max() <= 1e-8 * max(1.0, np.abs(cols[2] / scale).max()), d.max()
