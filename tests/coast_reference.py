"""Two-body reference of the coast arc and the orbit apsides (include/ascent.h: ascent_coast_batch, rows 2..5 of
ascent_fly_batch, rows 7 / 8 of ascent_flight_jacobian), in mpmath at 50 significant digits.

The inputs are the float64 values handed to the kernel, taken as exact numbers: the 16 parameter fields (G, M, R0, r_peri are
read; T_scale only converts the duration and is left to the caller) and the scaled state (x, y, xdot, ydot) with
X = x S, Y = y S + R0, V = v S, S = r_peri.  Times are seconds, apsides metres above R0, propagated states scaled as the input.

Nothing is taken from the kernels.  propagate() solves Kepler's equation in the difference dE of the eccentric anomaly and
applies Lagrange's f and g coefficients to the input state, which needs no division by the eccentricity and no perifocal frame;
tests/test_coast_reference.py proves it against DOP853 of the two-body ODE and against the textbook closed form
(elements -> anomaly -> state).

floor(fn, ...) measures how well-posed a question is: every float64 input, one after the other, is moved to its two float64
neighbours (1 ulp), and the largest change of each output that the pair causes is summed over the inputs -- to first order the
largest change when all inputs move by +-1 ulp at once, in the worst combination of signs.  It is computed by this reference
alone.  Where the answer is ill-determined (the place of the apsides of a nearly circular orbit, hence the time to the apoapsis
and the gradient of the apsides, all like 1 / e) it grows by itself.
"""
from __future__ import annotations

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 50
mpf = MP.mpf

IG, IM, IR0, IS, IT = 0, 1, 2, 9, 11       # fields of ascent_params that the two-body formulas read
P_READ = (IG, IM, IR0, IS)


def _si(p16, s4):
    G, M, R0, S = (mpf(float(p16[i])) for i in P_READ)
    x, y, vx, vy = (mpf(float(v)) for v in s4)
    return G * M, R0, S, x * S, y * S + R0, vx * S, vy * S


def _elements(GM, X, Y, VX, VY):
    r = MP.sqrt(X * X + Y * Y)
    v2, rv = VX * VX + VY * VY, X * VX + Y * VY
    energy = v2 / 2 - GM / r
    h = X * VY - Y * VX
    c = v2 / GM - 1 / r
    ex, ey = c * X - rv / GM * VX, c * Y - rv / GM * VY
    e = MP.sqrt(ex * ex + ey * ey)
    out = dict(r=r, rv=rv, energy=energy, h=h, ex=ex, ey=ey, e=e)
    if energy >= 0:
        out.update(a=(MP.inf if energy == 0 else -GM / (2 * energy)), E0=MP.nan, ec=MP.nan, es=MP.nan, n=MP.nan)
        return out
    a = -GM / (2 * energy)
    ec, es = 1 - r / a, rv / MP.sqrt(GM * a)            # e cos E0, e sin E0
    E0 = mpf(0) if (ec == 0 and es == 0) else MP.atan2(es, ec)
    out.update(a=a, ec=ec, es=es, E0=E0, n=MP.sqrt(GM / a ** 3))
    return out


def elements(p16, state4):
    """dict: a (m), ex, ey, e, h (m^2/s, signed), energy (J/kg), E0 (eccentric anomaly of the state, (-pi, pi]; 0 where
    e cos E0 = e sin E0 = 0), and r, rv, ec = e cos E0, es = e sin E0, n (mean motion, 1/s).  Energy >= 0: a = -GM / (2 energy)
    (negative; inf on the parabola) and E0, ec, es, n NaN."""
    GM, R0, S, X, Y, VX, VY = _si(p16, state4)
    return _elements(GM, X, Y, VX, VY)


def apsides(p16, state4):
    """(periapsis, apoapsis) altitude above R0, m.  Energy >= 0: (h^2 / (GM (1 + e)) - R0, +inf)."""
    GM, R0, S, X, Y, VX, VY = _si(p16, state4)
    el = _elements(GM, X, Y, VX, VY)
    if el["energy"] >= 0:
        return el["h"] ** 2 / (GM * (1 + el["e"])) - R0, MP.inf
    return el["a"] * (1 - el["e"]) - R0, el["a"] * (1 + el["e"]) - R0


def time_to_apoapsis(p16, state4):
    """seconds from the state to the next apoapsis of its orbit, in [0, one period): (pi - M0) / n, M0 = E0 - e sin E0; half a
    period where E0 is undefined (see elements).  NaN for energy >= 0."""
    el = elements(p16, state4)
    return (MP.pi - (el["E0"] - el["es"])) / el["n"]


def period(p16, state4):
    return 2 * MP.pi / elements(p16, state4)["n"]


def _kepler_difference(ec, es, m):
    """dE with dE - ec sin dE + es (1 - cos dE) = m: Newton from a float64 solution"""
    fec, fes, fm = float(ec), float(es), float(m)
    d = fm
    lo, hi = fm - 2.5, fm + 2.5   # |dE - m| <= 2 e; the left side is increasing in dE (slope r / a > 0): bisect where Newton leaves
    for _ in range(200):
        F = d - fec * np.sin(d) + fes * (1.0 - np.cos(d)) - fm
        if F > 0:
            hi = min(hi, d)
        else:
            lo = max(lo, d)
        dn = d - F / (1.0 - fec * np.cos(d) + fes * np.sin(d))
        if not (lo < dn < hi):
            dn = 0.5 * (lo + hi)
        if abs(dn - d) <= 4e-16 * max(1.0, abs(d)):
            d = dn
            break
        d = dn
    dE = mpf(d)
    for _ in range(8):
        step = (dE - ec * MP.sin(dE) + es * (1 - MP.cos(dE)) - m) / (1 - ec * MP.cos(dE) + es * MP.sin(dE))
        dE -= step
        if abs(step) < mpf(10) ** -45:
            break
    else:
        raise ArithmeticError("Kepler's equation did not converge")
    return dE


def propagate(p16, state4, t):
    """the scaled state (x, y, xdot, ydot) after t seconds (t >= 0) of two-body motion, as four mpf; NaN for energy >= 0"""
    GM, R0, S, X, Y, VX, VY = _si(p16, state4)
    el = _elements(GM, X, Y, VX, VY)
    if el["energy"] >= 0:
        return [MP.nan] * 4
    t = mpf(float(t))
    a, r0, rv, ec, es = el["a"], el["r"], el["rv"], el["ec"], el["es"]
    dE = _kepler_difference(ec, es, el["n"] * t)
    s, omc = MP.sin(dE), 1 - MP.cos(dE)
    r = a * (1 - ec * MP.cos(dE) + es * s)
    f = 1 - a / r0 * omc
    g = a * rv / GM * omc + r0 * MP.sqrt(a / GM) * s
    fd = -MP.sqrt(GM * a) / (r * r0) * s
    gd = 1 - a / r * omc
    Xn, Yn, VXn, VYn = f * X + g * VX, f * Y + g * VY, fd * X + gd * VX, fd * Y + gd * VY
    return [Xn / S, (Yn - R0) / S, VXn / S, VYn / S]


GRAD_COLUMNS = ("x", "y", "xdot", "ydot", "G", "M", "R0", "r_peri")


def _grad(fn, p16, z):
    """gradient of a scalar mp function of (x, y, xdot, ydot, G, M, R0, r_peri) by mpmath's high-precision differences"""
    pt = [mpf(float(v)) for v in z[:4]] + [mpf(float(p16[i])) for i in P_READ]
    return [MP.diff(fn, pt, tuple(1 if i == j else 0 for i in range(8))) for j in range(8)]


def _aps_of(which):
    def fn(x, y, vx, vy, G, M, R0, S):
        GM = G * M
        el = _elements(GM, x * S, y * S + R0, vx * S, vy * S)
        if el["energy"] >= 0:
            return el["h"] ** 2 / (GM * (1 + el["e"])) - R0 if which < 0 else MP.nan
        return el["a"] * (1 + which * el["e"]) - R0
    return fn


def apsides_gradient(p16, z):
    """(2, 8) mpf: d(periapsis, apoapsis altitude in m) / d(scaled x, y, xdot, ydot, G, M, R0, r_peri), the scaled state held
    fixed while a parameter moves.  Undefined at e = 0 exactly (a kink); the apoapsis row is NaN for energy >= 0."""
    return [_grad(_aps_of(-1), p16, z), _grad(_aps_of(+1), p16, z)]


def axis_gradient(p16, z):
    """(8,) mpf: d(2 a - 2 R0) / d(the same eight) -- the sum of the two apsides, smooth through e = 0"""
    def fn(x, y, vx, vy, G, M, R0, S):
        return 2 * _elements(G * M, x * S, y * S + R0, vx * S, vy * S)["a"] - 2 * R0
    return _grad(fn, p16, z)


def _flat(v):
    if isinstance(v, (list, tuple)):
        return [w for u in v for w in _flat(u)]
    return [v]


def floor(fn, p16, state4, *t):
    """The largest change of every output of fn(p16, state4, *t) -- one of the functions above -- when every float64 input it
    reads (G, M, R0, r_peri, the four state values and, if given, the time) is moved by +-1 ulp: per input the larger of the
    two changes, summed over the inputs.  Returns a flat float64 array (nested outputs in row-major order); NaN and infinite
    outputs give NaN there."""
    p16 = np.array(p16, dtype=np.float64)
    s4 = np.array(state4, dtype=np.float64)
    tt = np.array([float(v) for v in t], dtype=np.float64)
    base = _flat(fn(p16, s4, *tt))
    bad = [not MP.isfinite(b) for b in base]
    total = [mpf(0)] * len(base)
    slots = [(p16, i) for i in P_READ] + [(s4, i) for i in range(4)] + [(tt, i) for i in range(len(tt))]
    for arr, i in slots:
        keep = arr[i]
        worst = [mpf(0)] * len(base)
        for to in (np.inf, -np.inf):
            arr[i] = np.nextafter(keep, to)
            out = _flat(fn(p16, s4, *tt))
            for k, (o, b) in enumerate(zip(out, base)):
                if bad[k] or not MP.isfinite(o):
                    bad[k] = True
                elif abs(o - b) > worst[k]:
                    worst[k] = abs(o - b)
        arr[i] = keep
        total = [a + w for a, w in zip(total, worst)]
    return np.array([np.nan if bd else float(v) for v, bd in zip(total, bad)])


def to_float(v):
    return np.array([float(u) for u in _flat(v)])


# ---- the case matrix shared by tests/test_coast_reference.py (CPU) and tests/test_gpu_coast.py (device) ----

NOMINAL = np.array([6.674e-11, 7.346e22, 1738100.0, 15346.0, 4821.0, 5.053, 2376.0, 2376.0, 5e-4, 17703.0, 88615.0, 470.0,
                    np.pi / 3, 0.0, 1.0, 0.0])
ECCENTRICITIES = (0.9, 0.6, 0.3, 0.03, 1e-3, 1e-5, 1e-7, 1e-9, 1e-11, 1e-13, 0.0)
ANOMALIES = (0.0, 0.7, 2.5, np.pi - 1e-4, 3.6, -1e-3)
WELL_POSED = (0.9, 0.6, 0.3, 0.03, 1e-3, 1e-5)         # the eccentricities >= 1e-6: duration and end point are checked there


def other_params():
    """two parameter rows in which every field the two-body formulas read (and T_scale) differs from the nominal"""
    a, b = NOMINAL.copy(), NOMINAL.copy()
    a[[IG, IM, IR0, IS, IT]] = 8.1e-11, 3.9e22, 1.2e6, 25000.0, 600.0
    b[[IG, IM, IR0, IS, IT]] = 6.6743e-11, 5.972e24, 6.378e6, 2.0e5, 1000.0
    return a, b


def orbit_state(p16, e, nu, phase=0.2, retrograde=False):
    """scaled float64 state at true anomaly nu of an orbit of eccentricity e whose periapsis lies at polar angle `phase` (from +y
    towards -x, as the ascent flies); periapsis 20 km above R0 for e >= 0.3, semi-major axis R0 + 60 km below"""
    GM, R0, S = p16[IG] * p16[IM], p16[IR0], p16[IS]
    a = (R0 + 20e3) / (1.0 - e) if e >= 0.3 else R0 + 60e3
    sl = a * (1.0 - e * e)
    r = sl / (1.0 + e * np.cos(nu))
    vr, vt = np.sqrt(GM / sl) * e * np.sin(nu), np.sqrt(GM / sl) * (1.0 + e * np.cos(nu))
    ph = phase + nu
    X, Y = -r * np.sin(ph), r * np.cos(ph)
    VX, VY = -vr * np.sin(ph) - vt * np.cos(ph), vr * np.cos(ph) - vt * np.sin(ph)
    if retrograde:
        VX, VY = -VX, -VY
    return np.array([X / S, (Y - R0) / S, VX / S, VY / S])


def case_matrix():
    """list of (name, e, p16, state4): every eccentricity x every anomaly on the nominal Moon, the retrograde twin of three of
    them (angular momentum < 0), and two states under each of other_params()"""
    out = []
    for e in ECCENTRICITIES:
        for k, nu in enumerate(ANOMALIES):
            out.append((f"e{e:g}_nu{k}", e, NOMINAL, orbit_state(NOMINAL, e, nu)))
    for e, k in ((0.3, 1), (1e-7, 2), (0.03, 4)):
        out.append((f"e{e:g}_nu{k}_retrograde", e, NOMINAL, orbit_state(NOMINAL, e, ANOMALIES[k], retrograde=True)))
    for i, p in enumerate(other_params()):
        for e, k in ((0.03, 2), (1e-7, 1)):
            out.append((f"e{e:g}_nu{k}_params{i}", e, p, orbit_state(p, e, ANOMALIES[k], phase=-0.4)))
    return out
