"""The two-body reference (tests/coast_reference.py) proved before anything is compared with it: against DOP853 of the
two-body ODE, against the textbook closed form (elements -> anomaly -> state), at the apoapsis, its gradient against central
differences -- and the margin of tests/test_gpu_coast.py shown to be one that a plain float64 implementation of the same
algorithm meets.  Also the host-side BatchResult.orbit() against the reference's apsides.  No GPU."""
import functools

import numpy as np
import pytest

import coast_reference as cr

MP, mpf = cr.MP, cr.mpf
CASES = cr.case_matrix()
NODES = 4                       # the arc to the apoapsis is sampled at j / NODES of its duration, as the device test samples it


def _rhs(GM):
    def f(t, s):
        r3 = (s[0] * s[0] + s[1] * s[1]) ** 1.5
        return [s[2], s[3], -GM * s[0] / r3, -GM * s[1] / r3]
    return f


@pytest.mark.parametrize("e,nu", [(0.9, 0.7), (0.6, 2.5), (0.03, 3.6), (1e-7, 0.7), (0.3, -1e-3)])
def test_propagate_agrees_with_dop853(e, nu):
    """DOP853 at rtol 1e-13 over the arc to the apoapsis (1e5 s at e = 0.9) and over a quarter of it: the integrator's own
    noise was measured as <= 3e-5 m and <= 2e-9 m/s; bounded at 1e-4 m and 1e-8 m/s."""
    from scipy.integrate import solve_ivp
    p = cr.NOMINAL
    s = cr.orbit_state(p, e, nu)
    GM, R0, S = p[0] * p[1], p[2], p[9]
    T = float(cr.time_to_apoapsis(p, s))
    y0 = [s[0] * S, s[1] * S + R0, s[2] * S, s[3] * S]
    for t in (0.25 * T, T):
        r = solve_ivp(_rhs(GM), (0.0, t), y0, method="DOP853", rtol=1e-13, atol=[1e-7, 1e-7, 1e-11, 1e-11])
        assert r.success
        ref = cr.to_float(cr.propagate(p, s, t))
        dp = np.hypot(r.y[0, -1] - ref[0] * S, r.y[1, -1] - (ref[1] * S + R0))
        dv = np.hypot(r.y[2, -1] - ref[2] * S, r.y[3, -1] - ref[3] * S)
        print(f"e {e} nu {nu} t {t:.1f} s: position {dp:.2e} m, velocity {dv:.2e} m/s")
        assert dp <= 1e-4 and dv <= 1e-8


def _textbook(p16, s4, t):
    """elements -> true anomaly -> eccentric anomaly -> mean anomaly + n t -> Kepler's equation -> perifocal frame -> state;
    every division by e that propagate() avoids is made here (at 50 digits and e = 0.03 they cost nothing)"""
    GM, R0, S, X, Y, VX, VY = cr._si(p16, s4)
    el = cr.elements(p16, s4)
    a, e, h = el["a"], el["e"], el["h"]
    px, py = el["ex"] / e, el["ey"] / e
    sg = 1 if h >= 0 else -1
    qx, qy = -sg * py, sg * px
    nu0 = MP.atan2(X * qx + Y * qy, X * px + Y * py)
    E0 = 2 * MP.atan(MP.sqrt((1 - e) / (1 + e)) * MP.tan(nu0 / 2))
    M = E0 - e * MP.sin(E0) + el["n"] * mpf(float(t))
    E = MP.findroot(lambda E_: E_ - e * MP.sin(E_) - M, M)
    b = a * MP.sqrt(1 - e * e)
    r = a * (1 - e * MP.cos(E))
    xp, yp = a * (MP.cos(E) - e), b * MP.sin(E)
    vxp, vyp = -MP.sqrt(GM * a) / r * MP.sin(E), MP.sqrt(GM * a) / r * MP.sqrt(1 - e * e) * MP.cos(E)
    Xn, Yn, VXn, VYn = xp * px + yp * qx, xp * py + yp * qy, vxp * px + vyp * qx, vxp * py + vyp * qy
    return [Xn / S, (Yn - R0) / S, VXn / S, VYn / S]


@pytest.mark.parametrize("retro", [False, True])
def test_propagate_agrees_with_the_textbook_closed_form(retro):
    p = cr.NOMINAL
    for nu in cr.ANOMALIES:
        s = cr.orbit_state(p, 0.03, nu, retrograde=retro)
        for t in (0.0, 17.0, 1234.5, 9000.0):
            got, want = cr.propagate(p, s, t), _textbook(p, s, t)
            for g, w in zip(got, want):
                assert abs(g - w) <= mpf(10) ** -40 * (1 + abs(w)), (nu, t)


@pytest.mark.parametrize("e", [0.9, 0.03, 1e-5, 1e-11])
def test_propagate_to_the_apoapsis_lands_on_it(e):
    """at t = time_to_apoapsis the radius is a (1 + e) and r.v = 0, to 1e-30 relative; the time is below one period"""
    p = cr.NOMINAL
    for nu in cr.ANOMALIES:
        s = cr.orbit_state(p, e, nu)
        el = cr.elements(p, s)
        T = cr.time_to_apoapsis(p, s)
        assert 0 <= T < cr.period(p, s)
        # the time itself is not a float64 here: propagate at the mp time through the same code path
        GM, R0, S, X, Y, VX, VY = cr._si(p, s)
        dE = cr._kepler_difference(el["ec"], el["es"], el["n"] * T)
        sn, omc = MP.sin(dE), 1 - MP.cos(dE)
        a, r0 = el["a"], el["r"]
        r = a * (1 - el["ec"] * MP.cos(dE) + el["es"] * sn)
        f, g = 1 - a / r0 * omc, a * el["rv"] / GM * omc + r0 * MP.sqrt(a / GM) * sn
        fd, gd = -MP.sqrt(GM * a) / (r * r0) * sn, 1 - a / r * omc
        Xn, Yn, VXn, VYn = f * X + g * VX, f * Y + g * VY, fd * X + gd * VX, fd * Y + gd * VY
        rad = MP.sqrt(Xn * Xn + Yn * Yn)
        assert abs(rad - a * (1 + el["e"])) <= mpf(10) ** -30 * rad
        assert abs(Xn * VXn + Yn * VYn) <= mpf(10) ** -30 * rad * MP.sqrt(VXn * VXn + VYn * VYn)
        # ... and the public function at the float64 time next to it is within that rounding of the time
        end = cr.to_float(cr.propagate(p, s, float(T)))
        assert abs(np.hypot(end[0] * p[9], end[1] * p[9] + p[2]) - float(rad)) <= 1e-6


@pytest.mark.parametrize("e", [0.6, 0.03, 1e-5, 1e-8])
def test_apsides_gradient_agrees_with_central_differences(e):
    """central differences of apsides() at 50 digits with a relative step of 1e-20 (truncation ~ step^2 / e^2)"""
    p = cr.NOMINAL
    s = cr.orbit_state(p, e, 2.5)
    g = cr.apsides_gradient(p, s)
    ax = cr.axis_gradient(p, s)
    pt = [mpf(float(v)) for v in s] + [mpf(float(p[i])) for i in cr.P_READ]
    fp, fa = cr._aps_of(-1), cr._aps_of(+1)
    for j in range(8):
        h = abs(pt[j]) * mpf(10) ** -20
        up, dn = list(pt), list(pt)
        up[j] += h
        dn[j] -= h
        dpj, daj = (fp(*up) - fp(*dn)) / (2 * h), (fa(*up) - fa(*dn)) / (2 * h)
        assert abs(g[0][j] - dpj) <= mpf(10) ** -15 * abs(dpj) and abs(g[1][j] - daj) <= mpf(10) ** -15 * abs(daj)
        assert abs(ax[j] - (dpj + daj)) <= mpf(10) ** -15 * abs(ax[j])


# ---- a plain float64 implementation of the propagate algorithm: what a correct kernel can reach ----

def propagate_float64(p16, s4, t):
    GM, R0, S = p16[0] * p16[1], p16[2], p16[9]
    x, y, vx, vy = s4
    X, Y, VX, VY = x * S, y * S + R0, vx * S, vy * S
    r0 = np.sqrt(X * X + Y * Y)
    v2, rv = VX * VX + VY * VY, X * VX + Y * VY
    a = 1.0 / (2.0 / r0 - v2 / GM)
    sa = np.sqrt(GM * a)
    n = sa / (a * a)
    ec, es = 1.0 - r0 / a, rv / sa
    m = n * t
    M0 = np.arctan2(es, ec) - es
    dE = m + np.hypot(ec, es) * (np.sin(M0 + m) - np.sin(M0))
    for _ in range(16):
        sh = np.sin(0.5 * dE)
        omc = 2.0 * sh * sh
        dE -= (dE - ec * np.sin(dE) + es * omc - m) / (1.0 - ec * (1.0 - omc) + es * np.sin(dE))
    sn, sh = np.sin(dE), np.sin(0.5 * dE)
    omc = 2.0 * sh * sh
    rr = r0 + a * (ec * omc + es * sn)
    fm1, g = -a / r0 * omc, a * (rv / GM) * omc + r0 * (a / sa) * sn
    fd, gdm1 = -sa / (rr * r0) * sn, -a / rr * omc
    rho0 = R0 / S
    return np.array([x + (fm1 * x + g * vx), y + (fm1 * (y + rho0) + g * vy), vx + (fd * x + gdm1 * vx),
                     vy + (fd * (y + rho0) + gdm1 * vy)])


@functools.lru_cache(maxsize=None)
def _node_times(i):
    _, _, p, s = CASES[i]
    T = float(cr.time_to_apoapsis(p, s))
    return [T * j / NODES for j in range(NODES + 1)]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_float64_implementation_stays_within_16_floors(i):
    """The device test allows 64 x floor; a float64 transcription of the algorithm, at the nodes the device test samples, stays
    within 16 x floor of the 50-digit result on every case of the matrix: the margin is one a correct implementation meets.
    At t = 0 it returns the input bit for bit."""
    name, e, p, s = CASES[i]
    S = p[9]
    assert np.array_equal(propagate_float64(p, s, 0.0), s)
    worst = 0.0
    for t in _node_times(i)[1:]:
        ref = cr.to_float(cr.propagate(p, s, t))
        fl = cr.floor(cr.propagate, p, s, t)
        got = propagate_float64(p, s, t)
        rp = np.hypot(*(got[:2] - ref[:2])) / np.hypot(*fl[:2])
        rv = np.hypot(*(got[2:] - ref[2:])) / np.hypot(*fl[2:])
        worst = max(worst, rp, rv)
    print(name, "float64 error / floor", worst, "floor of the last node (m)", S * np.hypot(*fl[:2]))
    assert worst <= 16.0


@pytest.mark.parametrize("e", [0.6, 0.03, 1e-6, 1e-9, 0.0])
def test_orbit_of_a_batch_result_against_the_reference_apsides(e):
    """BatchResult.orbit() (host side, numpy) from synthetic traj and params: periapsis and apoapsis to 1e-6 m of the 50-digit
    values, at every anomaly of the matrix and under the other parameter rows; energy >= 0: the device's convention"""
    from lunar_module_ascent_trajectory_optimiser_amd.solver import BatchResult
    rows = [(cr.NOMINAL, cr.orbit_state(cr.NOMINAL, e, nu)) for nu in cr.ANOMALIES]
    rows += [(p, cr.orbit_state(p, e, 0.7, phase=-0.4)) for p in cr.other_params()]
    rows.append((cr.NOMINAL, cr.orbit_state(cr.NOMINAL, e, 2.5, retrograde=True)))
    fast = cr.orbit_state(cr.NOMINAL, 0.03, 0.7) * np.array([1.0, 1.0, 1.5, 1.5])      # above the escape speed
    rows.append((cr.NOMINAL, fast))
    B = len(rows)
    traj = np.zeros((10, 2, B))
    traj[:4, -1, :] = np.array([s for _, s in rows]).T
    r = BatchResult(np.array([p for p, _ in rows]), 2, traj, np.ones(B), np.zeros(B, np.int32), np.zeros(B, np.int32), None, 0.0)
    o = r.orbit()
    worst = 0.0
    for j, (p, s) in enumerate(rows[:-1]):
        peri, apo = cr.to_float(cr.apsides(p, s))
        worst = max(worst, abs(o["periapsis_alt"][j] - peri), abs(o["apoapsis_alt"][j] - apo))
        assert abs(o["eccentricity"][j] - float(cr.elements(p, s)["e"])) <= 1e-12
    print("e", e, "orbit() against the reference apsides (m)", worst)
    assert worst <= 1e-6
    peri, apo = cr.apsides(*rows[-1])
    assert apo == MP.inf and o["apoapsis_alt"][-1] == np.inf and abs(o["periapsis_alt"][-1] - float(peri)) <= 1e-6
