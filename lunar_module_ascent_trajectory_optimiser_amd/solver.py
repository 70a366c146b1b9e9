"""Host-side API over libascent (include/ascent.h): the replacement of the reference's
`m.solve()` call (/root/reference/Launch_Optimiser.py:177) for batches of ascent NLPs."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from .params import PARAM_FIELDS, AscentParams, pack

TRAJ_FIELDS = ("x", "y", "xdot", "ydot", "xdoubledot", "ydoubledot", "angle", "angledot",
               "angledoubledot", "mass")
STATUS_NAMES = {0: "converged", 1: "max_iter", 2: "linesearch_failed", 3: "regularisation_failed", 4: "invalid_problem"}


def blob_rows(nt: int) -> int:
    return 21 * (nt - 1) + 10


SCHEMES = {"backward_euler": 0, "trapezoid": 1, "hermite_simpson": 2}
TERMINALS = {"reference": 0, "ellipse": 1, "ellipse_free": 2}


FORMULATIONS = {"current": 0, "v1": 1}


def _opts(nt, max_iter, tol, warm_start, mu_init, scheme=0, formulation=0, coarse_nodes=0, terminal=0, path="auto", move_penalty=False):
    scheme = SCHEMES.get(scheme, scheme)
    formulation = FORMULATIONS.get(formulation, formulation)
    terminal = TERMINALS.get(terminal, terminal)
    if path not in ("auto", "dense"):
        raise ValueError('solver path must be "auto" or "dense"')
    return _lib.AscentOptsC(n_nodes=nt, scheme=int(scheme), max_iter=max_iter, warm_start=warm_start, tol=tol,
                            mu_init=mu_init, formulation=int(formulation), coarse_nodes=int(coarse_nodes),
                            terminal=int(terminal), solver_path=_lib.PATHS[path], move_penalty=int(bool(move_penalty)), reserved=0)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _blob_call(params, sol_blob, nt, scheme=0, formulation=0, terminal=0, move_penalty=False, what="sol_blob"):
    """What every call at a blob begins with: (L, P, B, K, blob, o) -- the library, the packed parameters, batch and intervals,
    the blob as a contiguous (21K+10, batch) float64 array (checked) and the options of a call that does not iterate."""
    P = pack(params)
    B = P.shape[0]
    blob = np.ascontiguousarray(sol_blob, dtype=np.float64)
    if blob.shape != (blob_rows(nt), B):
        raise ValueError(f"sol_blob must have shape {(blob_rows(nt), B)}" if what == "sol_blob" else f"{what} has the wrong shape")
    o = _opts(nt, 0, 1.0, 0, 0.0, scheme, formulation, terminal=terminal, move_penalty=move_penalty)
    return _lib.load(), P, B, nt - 1, blob, o


FLIGHT_ROWS = ("miss_position", "miss_velocity", "flown_periapsis_alt", "flown_apoapsis_alt", "nlp_periapsis_alt",
               "nlp_apoapsis_alt", "max_local_position_error", "max_local_velocity_error", "max_local_step", "substeps")


@dataclasses.dataclass
class FlightResult:
    """What every solution's control reaches when it is flown (fly_batch; include/ascent.h: ascent_fly_batch).  Problem index first."""
    traj: np.ndarray | None         # (batch, 10, nt) the flown trajectory, scaled, fields TRAJ_FIELDS
    local_error: np.ndarray | None  # (batch, K, 7) eta_k = (the NLP's z_{k-1} flown over step k) - z_k, scaled
    summary: np.ndarray             # (batch, 10) SI units, columns FLIGHT_ROWS


for _i, _n in enumerate(FLIGHT_ROWS):   # the summary columns by name: .miss_position (m), .miss_velocity (m/s), ... -> (batch,)
    setattr(FlightResult, _n, property(lambda self, _i=_i: self.summary[:, _i]))


JACOBIAN_ROWS = ("x", "y", "xdot", "ydot", "angle", "angledot", "mass", "periapsis_alt", "apoapsis_alt")
TRIM_ROWS = ("status", "rounds", "residual", "residual_before", "delta_tf_seconds", "max_delta_u", "free_controls",
             "flown_periapsis_alt", "flown_apoapsis_alt", "angle_violation")
TRIM_STATUS_NAMES = {0: "converged", 1: "rounds_exhausted", 2: "frozen"}


@dataclasses.dataclass
class FlightJacobian:
    """Derivative of what a blob's control reaches when it is flown (flight_jacobian; include/ascent.h:
    ascent_flight_jacobian).  Rows JACOBIAN_ROWS: the flown z_K in scaled units, then the flown periapsis / apoapsis altitude
    in metres.  Problem index first."""
    dz0: np.ndarray                 # (batch, 9, 7) with respect to the initial state, scaled units
    dparams: np.ndarray             # (batch, 9, 16) per SI unit of every parameter field (PARAM_FIELDS order), blob held fixed
    dtf: np.ndarray                 # (batch, 9) with respect to the scaled t_f
    dcontrols: np.ndarray | None    # (batch, 9, K) column k-1: with respect to u_k

    def predict(self, dparams=None, dtf=None, dcontrols=None, dz0=None) -> np.ndarray:
        """(batch, 9) first-order change of the nine end quantities under the given changes: dparams (16,) or (batch, 16) in
        SI units, dtf scalar or (batch,) scaled, dcontrols (K,) or (batch, K), dz0 (7,) or (batch, 7); each may be None."""
        out = np.zeros(self.dtf.shape)
        if dparams is not None:
            out += np.einsum("bqc,bc->bq", self.dparams, np.broadcast_to(np.asarray(dparams, dtype=np.float64), self.dparams[:, 0].shape))
        if dtf is not None:
            out += self.dtf * np.broadcast_to(np.asarray(dtf, dtype=np.float64), self.dtf.shape[:1])[:, None]
        if dcontrols is not None:
            if self.dcontrols is None:
                raise ValueError("this FlightJacobian was computed without the control columns")
            out += np.einsum("bqk,bk->bq", self.dcontrols, np.broadcast_to(np.asarray(dcontrols, dtype=np.float64), self.dcontrols[:, 0].shape))
        if dz0 is not None:
            out += np.einsum("bqc,bc->bq", self.dz0, np.broadcast_to(np.asarray(dz0, dtype=np.float64), self.dz0[:, 0].shape))
        return out

    def sigma(self, param_sigma=None, control_sigma=None) -> np.ndarray:
        """(batch, 9) root-sum-square 1-sigma of every row for independent errors: param_sigma (16,) or (batch, 16) the
        standard deviation of every parameter field in SI units, control_sigma a scalar, (K,) or (batch, K) per-step standard
        deviation of u."""
        var = np.zeros(self.dtf.shape)
        if param_sigma is not None:
            var += ((self.dparams * np.broadcast_to(np.asarray(param_sigma, dtype=np.float64), self.dparams[:, 0].shape)[:, None, :]) ** 2).sum(axis=2)
        if control_sigma is not None:
            if self.dcontrols is None:
                raise ValueError("this FlightJacobian was computed without the control columns")
            var += ((self.dcontrols * np.broadcast_to(np.asarray(control_sigma, dtype=np.float64), self.dcontrols[:, 0].shape)[:, None, :]) ** 2).sum(axis=2)
        return np.sqrt(var)


def _sigma_rows(v, n, B, what):
    """(B, n) from None (zeros), a scalar, (n,) or (B, n)"""
    if v is None:
        return np.zeros((B, n))
    a = np.asarray(v, dtype=np.float64)
    try:
        return np.ascontiguousarray(np.broadcast_to(a, (B, n)))
    except ValueError:
        raise ValueError(f"{what} must broadcast to {(B, n)}") from None


def _cov_from_upper(rows):
    """(batch, 9, 9) symmetric from the 45 rows of the upper triangle, row-major: (batch, 45)"""
    B = rows.shape[0]
    cov = np.empty((B, 9, 9))
    iu = np.triu_indices(9)
    cov[:, iu[0], iu[1]] = rows
    cov[:, iu[1], iu[0]] = rows
    return cov


@dataclasses.dataclass
class DispersionResult:
    """Monte Carlo dispersion of flown solutions (disperse_batch; include/ascent.h: ascent_disperse_batch): the statistics of the
    nine end quantities of the flight (columns JACOBIAN_ROWS: the flown z_K in scaled units, the flown periapsis / apoapsis
    altitude in metres) over the valid samples.  Problem index first."""
    n_valid: np.ndarray             # (batch,) samples with nine finite rows; the others are left out of every statistic
    nominal: np.ndarray             # (batch, 9) the unperturbed flight
    mean: np.ndarray                # (batch, 9)
    cov: np.ndarray                 # (batch, 9, 9) unbiased sample covariance, symmetric; NaN where n_valid < 2
    min: np.ndarray                 # (batch, 9) NaN where n_valid = 0
    max: np.ndarray                 # (batch, 9)
    samples: np.ndarray | None      # (batch, samples, 9) every sample's rows, invalid ones as they came out (keep_samples=True)
    xi: np.ndarray                  # (24 + K, samples) the draws, shared by every problem
    z0_sigma: np.ndarray            # (batch, 7) scaled units
    param_sigma: np.ndarray         # (batch, 16) SI units
    tf_sigma: np.ndarray            # (batch,) scaled units
    control_sigma: np.ndarray       # (batch, K)
    effort: np.ndarray | None = None    # (batch, samples, 3) guided flights with keep_samples: EFFORT_ROWS
    xi_nav: np.ndarray | None = None    # (8, samples) the navigation draws (ascent_disperse_navigated_batch), shared by every problem
    nav_sigma: np.ndarray | None = None     # (batch, 8): 7 state-knowledge biases (scaled units), the error of theta-hat
    quantile_probs: np.ndarray | None = None    # (n_probs,) disperse_batch(quantiles=...): the probabilities of the quantile rows
    quantiles: np.ndarray | None = None         # (batch, n_probs, 9) numpy's "linear" quantiles of the nine end quantities over the valid samples
    effort_quantiles: np.ndarray | None = None  # (batch, n_probs, 3) those of EFFORT_ROWS, guided flights
    below: np.ndarray | None = None             # (batch, n_limits, 9) disperse_batch(limits=...): valid samples at or below the limit; 0 where it is NaN
    effort_below: np.ndarray | None = None      # (batch, n_limits, 3)
    xi_drift: np.ndarray | None = None      # (8, K, samples) the driving draws of the drifting knowledge errors (nav_tau, knowledge_tau)
    nav_phi: np.ndarray | None = None       # (batch, 8) their per-step decay exp(-dt / tau); 1 where frozen
    nav_q: np.ndarray | None = None         # (batch, 8) their per-step drive steady * sqrt(1 - phi^2); 0 where frozen
    history: "DispersionHistory | None" = None      # disperse_batch(history=...): the statistics at the nodes on the way

    @property
    def std(self) -> np.ndarray:
        """(batch, 9)"""
        return np.sqrt(np.diagonal(self.cov, axis1=1, axis2=2))

    def linear_covariance(self, J: FlightJacobian, J_nav: np.ndarray | None = None) -> np.ndarray:
        """(batch, 9, 9) J D C_xi D J': the first-order prediction of `cov` from a FlightJacobian of the same blob, D the sigmas of
        this result and C_xi the unbiased sample covariance of the rows of this very `xi` -- no sampling noise between the two.
        J_nav (batch, 9, 8), GuidanceResult.jacobian_nav: the navigation block, with this result's nav_sigma and xi_nav, is added
        (the two tables of draws are taken as one sample)."""
        A = [J.dz0 * self.z0_sigma[:, None, :], J.dparams * self.param_sigma[:, None, :], (J.dtf * self.tf_sigma[:, None])[:, :, None]]
        n = 24
        if self.control_sigma.any():
            if J.dcontrols is None:
                raise ValueError("this FlightJacobian was computed without the control columns")
            A.append(J.dcontrols * self.control_sigma[:, None, :])
            n += self.control_sigma.shape[1]
        draws = self.xi[:n]
        if J_nav is not None:
            if self.nav_sigma is None or self.xi_nav is None:
                raise ValueError("this dispersion was flown without navigation errors")
            A.append(np.asarray(J_nav, dtype=np.float64) * self.nav_sigma[:, None, :])
            draws = np.concatenate([draws, self.xi_nav], axis=0)
        A = np.concatenate(A, axis=2)
        C = np.atleast_2d(np.cov(draws))
        return np.einsum("bqc,cd,brd->bqr", A, C, A)


HISTORY_ROWS = ("x", "y", "xdot", "ydot", "angle", "angledot", "mass", "altitude", "control", "correction")


@dataclasses.dataclass
class DispersionHistory:
    """The dispersion corridor of a flight (disperse_batch(history=...); include/ascent.h: ascent_disperse_history_batch): the
    statistics over the samples of the ten quantities HISTORY_ROWS -- the flown state in scaled units, the altitude in metres,
    the executed control and the feedback's correction of the step that ends at the node -- at every stride-th node and the last.
    A sample is valid at a node if its ten quantities there are finite (an escaping sample is valid here).  Problem index first."""
    nodes: np.ndarray               # (NJ,) the node numbers, 1-based (node 0 is not reported); the last one is K
    n_valid: np.ndarray             # (batch, NJ)
    nominal: np.ndarray             # (batch, NJ, 10) the unperturbed flight: fly_batch's trajectory, the blob's control, correction 0
    mean: np.ndarray                # (batch, NJ, 10)
    var: np.ndarray                 # (batch, NJ, 10) unbiased; NaN where n_valid < 2
    min: np.ndarray                 # (batch, NJ, 10) NaN where n_valid = 0
    max: np.ndarray                 # (batch, NJ, 10)
    clipped: np.ndarray             # (batch, NJ) valid samples whose command of the step was clipped; 0 in open loop
    samples: np.ndarray | None      # (batch, samples, NJ, 10) every sample's quantities (keep_history_samples=True)
    quantiles: np.ndarray | None = None     # (batch, NJ, n_probs, 10) disperse_batch(quantiles=...), over the samples valid at the node
    below: np.ndarray | None = None         # (batch, NJ, n_limits, 10) disperse_batch(history_limits=...): valid samples at or below the limit

    @property
    def std(self) -> np.ndarray:
        """(batch, NJ, 10)"""
        return np.sqrt(self.var)


def history_nodes(K: int, stride: int) -> np.ndarray:
    """The 1-based nodes a history of this stride reports: every stride-th and always node K."""
    nj = K // stride + (K % stride != 0)
    return np.minimum((np.arange(nj) + 1) * stride, K)


EFFORT_ROWS = ("clipped_steps", "max_feedback", "stretch")
GUIDE_ROWS = ("status", "free_controls", "max_gain", "max_cutoff_gain", "substeps")
GUIDE_FF_ROWS = GUIDE_ROWS + ("max_feedforward", "max_cutoff_feedforward")
GUIDE_STATUS_NAMES = {0: "ok", 2: "frozen"}


@dataclasses.dataclass
class GuidanceResult:
    """Neighbouring-optimal feedback gains about a flown solution (guidance_gains; include/ascent.h: ascent_guidance_gains).
    Step k commands u_k - gain_u[:, k-1] . (z - z_{k-1}^nominal); the last step's duration is stretched by the relative amount
    -gain_t . (z - z_{K-1}^nominal), clipped to +-stretch_max.  Problem index first."""
    gain_u: np.ndarray              # (batch, K, 7); the row of a saturated control is exactly zero
    gain_t: np.ndarray              # (batch, 7) zero where stretch_max = 0
    summary: np.ndarray             # (batch, 5) columns GUIDE_ROWS; (batch, 7), columns GUIDE_FF_ROWS, with a feed-forward
    stretch_max: np.ndarray         # (batch,)
    jacobian: FlightJacobian | None     # the flight Jacobian of the closed loop, clips ignored; dcontrols: execution errors
    # with a feed-forward (guidance_gains(feedforward=...); include/ascent.h: ascent_guidance_feedforward): step k commands, beyond
    # the feedback, -ff_u[:, k-1] * theta-hat and the stretch -ff_t * theta-hat; summary is then (batch, 7), columns GUIDE_FF_ROWS
    ff_u: np.ndarray | None = None      # (batch, K); exactly zero for a saturated control
    ff_t: np.ndarray | None = None      # (batch,)
    ff_dir: np.ndarray | None = None    # (batch, 16) the direction d of the parameter deviation theta * d, SI units
    ff_know: np.ndarray | None = None   # (batch, 16) the row w of theta-hat = w . (the vehicle's 16 parameter deviations)
    jacobian_nav: np.ndarray | None = None      # (batch, 9, 8): 7 state-knowledge biases (scaled units), the error of theta-hat


for _i, _n in enumerate(GUIDE_FF_ROWS):    # the summary columns by name: .status, .free_controls, ... -> (batch,)
    setattr(GuidanceResult, _n, property(lambda self, _i=_i: self.summary[:, _i]))


@dataclasses.dataclass
class TrimResult:
    """A batch of trimmed solutions (trim_batch; include/ascent.h: ascent_trim_batch)."""
    blob: np.ndarray       # (21K+10, batch) the trimmed blob: u, t_f and the flown states replaced; multipliers stale
    summary: np.ndarray    # (batch, 10) columns TRIM_ROWS
    nt: int

    @property
    def tf(self) -> np.ndarray:
        return self.blob[21 * (self.nt - 1)]

    @property
    def controls(self) -> np.ndarray:
        """(batch, K)"""
        K = self.nt - 1
        return np.ascontiguousarray(self.blob[7 * K:8 * K].T)

    @property
    def converged(self) -> np.ndarray:
        return self.summary[:, 0] == 0


for _i, _n in enumerate(TRIM_ROWS):     # the summary columns by name: .status, .rounds, .residual, ... -> (batch,)
    setattr(TrimResult, _n, property(lambda self, _i=_i: self.summary[:, _i]))


@dataclasses.dataclass
class BatchResult:
    """Solutions of a batch. Arrays keep the library's layout: problem index last."""
    params: np.ndarray          # (batch, 16)
    nt: int
    traj: np.ndarray            # (10, nt, batch) scaled, fields TRAJ_FIELDS (reference .value lists)
    tf: np.ndarray              # (batch,)  scaled final time (tf.value[0])
    status: np.ndarray          # (batch,) int32, see STATUS_NAMES
    iters: np.ndarray           # (batch,) int32
    blob: np.ndarray | None     # (21K+10, batch) primal-dual solution (warm-start material)
    kernel_ms: float            # device time of the solve kernel
    sensitivity: np.ndarray | None = None   # (batch, 16) d(T_scale J*)/dp, s per SI unit (solve_batch(sensitivity=True))
    flight: FlightResult | None = None      # the solutions' controls flown with RK4 (solve_batch(flight=True))
    trim: TrimResult | None = None          # the solutions trimmed so that the flown control reaches the orbit (solve_batch(trim=True))

    @property
    def converged(self) -> np.ndarray:
        return self.status == 0

    def field(self, name: str) -> np.ndarray:
        """(nt, batch) array of one of TRAJ_FIELDS, in the reference's scaled units."""
        return self.traj[TRAJ_FIELDS.index(name)]

    def final_time(self) -> np.ndarray:
        """seconds: tf.value[0]*final_time (Launch_Optimiser.py:194)."""
        return self.tf * self.params[:, 11]

    def orbit(self) -> dict:
        """Kepler-exact two-body orbit through every problem's final state (the reference's
        v1 script propagated the end state with explicit Euler, PDF p28-29; this is the closed form).  Returns
        periapsis / apoapsis altitudes above R0 (m), semi-major axis (m), eccentricity and flight-path angle (rad).
        Note for the reference's own target: it asks for the circular speed of the *mean* radius at the
        17.7 km insertion altitude (Launch_Optimiser.py:72-78), which is below the local circular speed."""
        P = self.params
        S, R0, GM = P[:, 9], P[:, 2], P[:, 0] * P[:, 1]
        X, Y = self.traj[0, -1] * S, self.traj[1, -1] * S + R0
        VX, VY = self.traj[2, -1] * S, self.traj[3, -1] * S
        r, v2, rv = np.hypot(X, Y), VX * VX + VY * VY, X * VX + Y * VY
        h = X * VY - Y * VX
        # the device's formulas (apsides_of): eccentricity from the eccentricity vector -- 1 - h^2 / (GM a) loses eps / e near
        # the circle --, periapsis from the semi-latus rectum; specific energy >= 0: apoapsis +inf
        ex, ey = (v2 / GM - 1.0 / r) * X - rv / GM * VX, (v2 / GM - 1.0 / r) * Y - rv / GM * VY
        e = np.hypot(ex, ey)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = 1.0 / (2.0 / r - v2 / GM)
            apo = np.where(0.5 * v2 - GM / r < 0.0, a * (1 + e) - R0, np.inf)
        return dict(periapsis_alt=h * h / (GM * (1 + e)) - R0, apoapsis_alt=apo, semi_major_axis=a, eccentricity=e,
                    flight_path_angle=np.arcsin(np.clip(rv / (r * np.sqrt(v2)), -1, 1)))

    def coast(self, coast_nodes: int = 200, device: int = 0, flown: bool = False) -> dict:
        """The second phase: coast from every problem's burnout state to the apoapsis of its orbit, propagated on the
        device (Kepler-exact; see coast_batch).  With terminal="ellipse" the arc ends at r_apo above the surface.
        flown: start from the burnout state the control actually reaches (solve_batch(flight=True)) instead of the NLP's."""
        if not flown:
            return coast_batch(self.params, np.ascontiguousarray(self.traj[:4, -1, :]), coast_nodes, device)
        if self.flight is None or self.flight.traj is None:
            raise ValueError("coast(flown=True) needs the flown trajectory: solve_batch(..., flight=True)")
        return coast_batch(self.params, np.ascontiguousarray(self.flight.traj[:, :4, -1].T), coast_nodes, device)

    def disperse(self, **kw) -> "DispersionResult":
        """Monte Carlo dispersion of these solutions' flights: disperse_batch(self.params, the blob, self.nt, **kw), with
        guidance=<a GuidanceResult of the same blob> under that feedback.  A result
        does not keep the options it was solved with: repeat scheme, formulation, terminal and move_penalty in kw as for
        disperse_batch -- a formulation-1 solution dispersed without formulation=1 is flown as formulation 0."""
        return disperse_batch(self.params, self.blob if self.blob is not None else self.flight_blob(), self.nt, **kw)

    def flight_blob(self) -> np.ndarray:
        """The part of a solution blob that fly_batch reads -- states, control and tf -- rebuilt from the trajectory (the rest
        zero): (21K+10, batch).  For results that were returned without their blob."""
        K, B = self.nt - 1, self.params.shape[0]
        blob = np.zeros((blob_rows(self.nt), B))
        blob[:7 * K] = self.traj[[0, 1, 2, 3, 6, 7, 9], 1:].transpose(1, 0, 2).reshape(7 * K, B)
        blob[7 * K:8 * K] = self.traj[8, 1:]
        blob[21 * K] = self.tf
        return blob

    def outputs(self, i: int = 0) -> dict:
        """The quantities the reference prints/plots for problem i (Launch_Optimiser.py:178-202):
        physical t, x_pos (sign flipped as :200), y_pos (:201), theta in degrees (:202), mass, and
        the polar (r, theta_polar) of north_star."""
        P = self.params[i]
        S, R0, T, M0, ms = P[9], P[2], P[11], P[4], P[7]
        tr = self.traj[:, :, i]
        x, y = tr[0], tr[1]
        X, Y = x * S, y * S + R0
        return dict(
            t=np.linspace(0.0, 1.0, self.nt) * self.tf[i] * T,
            x_pos=-X, y_pos=Y, theta_deg=3.0 * tr[6] * 180.0 / np.pi,
            r=np.hypot(X, Y), theta_polar=np.arctan2(-X, Y), control_angle=3.0 * tr[6],
            mass_kg=M0 - ms * tr[9],
            final_y=y[-1] * S, final_x=x[-1] * S, final_ydot=tr[3, -1] * S, final_xdot=tr[2, -1] * S,
            final_ydoubledot=tr[5, -1] * S, final_xdoubledot=tr[4, -1] * S,
            final_time=self.tf[i] * T, tf=self.tf[i],
        )


def solve_batch(params, nt: int = 200, tol: float = 1e-9, max_iter: int = 300, guess: np.ndarray | None = None,
                warm_start: int | None = None, mu_init: float = 0.0, device: int = 0, want_traj: bool = True,
                want_blob: bool = False, scheme=0, formulation=0, coarse_nodes: int = 0, terminal=0,
                path: str = "auto", move_penalty: bool = False, sensitivity: bool = False, flight: bool = False,
                trim: bool = False) -> BatchResult:
    """Solve a batch of ascent NLPs on one GPU.  params: AscentParams | list | (batch,16) array.
    guess: (21K+10, batch) blob, with warm_start 1 (primal only) or 2 (primal-dual).
    scheme: 0 / "backward_euler" (the reference's NODES=2), 1 / "trapezoid" or 2 / "hermite_simpson" (both with the
    control held over the step; scheme 2 runs in a persistent kernel of its own, with the move penalty on the dense-block path).
    terminal: 0 / "reference" (Launch_Optimiser.py:72-78), 1 / "ellipse" (the (r_peri, r_apo) ellipse proper: vis-viva
    speed at its periapsis; `BatchResult.coast()` then ends at its apoapsis) or 2 / "ellipse_free" (burnout anywhere on that
    ellipse: its angular momentum and energy, no r.v = 0; the coast starts at whatever true anomaly the burn ends at).
    path: "auto" or "dense" (the dense-block path for any scheme).
    move_penalty: apply the reference's MV DCOST (Launch_Optimiser.py:99): objective tf + dcost * sum |u_k - u_{k-1}| with the
    `dcost` of each parameter set (schemes 0 / 1: inside the persistent kernel, the control as the eighth state of a stage;
    scheme 2: dense-block path; default off: `dcost` is then ignored).
    formulation: 0 / "current" or 1 / "v1" (the PDF appendix script: the angle is the MV; see include/ascent.h).
    coarse_nodes: nested iteration for cold starts (0 automatic, -1 single grid, > 0 explicit coarse grid);
    `iters` then counts the iterations of all grid levels.
    sensitivity: also set `BatchResult.sensitivity`, (batch, 16) d(T_scale J*)/dp in seconds per SI unit of every parameter
    field (param_sensitivity at the solution; the T_scale column is J* + T_scale dJ*/dT_scale); rows of problems that did not
    converge are NaN.  Without the move penalty this is d t_f*/dp; with it, the penalised objective in seconds.
    flight: also set `BatchResult.flight`, a FlightResult: every solution's control flown with RK4 on the device (fly_batch,
    automatic substeps) -- the flown trajectory, the local error of every step and the miss at burnout; rows of problems that
    did not converge are NaN.
    trim: also set `BatchResult.trim`, a TrimResult: (t_f, u) of every solution corrected so that the flown control meets the
    terminal conditions (trim_batch with its defaults; terminal 0 / 1 only); problems that did not converge are trimmed from
    whatever their blob holds and usually end with status 2."""
    L = _lib.load()
    P = pack(params)
    B = P.shape[0]
    rows = blob_rows(nt)
    if guess is not None:
        guess = np.ascontiguousarray(guess, dtype=np.float64)
        if guess.shape != (rows, B):
            raise ValueError(f"guess must have shape {(rows, B)}")
        if warm_start is None:
            warm_start = 1
    warm_start = warm_start or 0
    traj = np.empty((10, nt, B)) if want_traj else None
    blob = np.empty((rows, B)) if (want_blob or sensitivity or flight or trim) else None
    tf = np.empty(B)
    status = np.empty(B, dtype=np.int32)
    iters = np.empty(B, dtype=np.int32)
    o = _opts(nt, max_iter, tol, warm_start, mu_init, scheme, formulation, coarse_nodes, terminal, path, move_penalty)
    _lib.check(L.ascent_solve_batch(_ptr(P), B, C.byref(o), _ptr(guess), _ptr(traj), _ptr(tf), _ptr(status),
                                    _ptr(iters), _ptr(blob), device, None, 0))
    kms = L.ascent_last_kernel_ms(device)
    sens = None
    if sensitivity:
        g = param_sensitivity(P, blob, nt, scheme=scheme, formulation=formulation, terminal=terminal,
                              move_penalty=move_penalty, device=device)
        sens = _seconds(P, blob, nt, g, formulation, move_penalty)
        sens[status != 0] = np.nan
    fl = None
    if flight:
        fl = fly_batch(P, blob, nt, scheme=scheme, formulation=formulation, terminal=terminal, move_penalty=move_penalty,
                       device=device)
        for a in (fl.traj, fl.local_error, fl.summary):
            a[status != 0] = np.nan
    tr = None
    if trim:
        tr = trim_batch(P, blob, nt, scheme=scheme, formulation=formulation, terminal=terminal, move_penalty=move_penalty,
                        device=device)
    return BatchResult(P, nt, traj, tf, status, iters, blob if want_blob else None, kms, sens, fl, tr)


def _penalised_objective(P, blob, K, formulation):
    """tf + w sum_k |u_k - u_{k-1}| of every problem at its blob, (batch,): the weight w of the movement in the scaled objective
    and u_{-1} depend on the formulation (include/ascent.h: ascent_opts.move_penalty).  P (batch, 16) and blob (21K+10, batch)
    are numpy arrays or torch tensors alike.  The movements are laid out as (K, batch) rows and summed over the rows, u_0 - u_{-1}
    first: the order of additions of a sum over the K + 1 controls with u_{-1} put in front."""
    form = FORMULATIONS.get(formulation, formulation)
    w, u0 = (P[:, 15] * P[:, 12] * 0.5, -1.0) if form == 1 else (P[:, 15], 0.0)
    U = blob[7 * K:8 * K]
    dU = abs(U - u0)
    dU[1:] = abs(U[1:] - U[:-1])
    return blob[21 * K] + w * dU.sum(0)


def objective(params, sol_blob, nt: int, formulation=0, move_penalty: bool = False) -> np.ndarray:
    """J* of every problem at its solution blob (rows, batch): the scaled objective as solved -- tf, plus the move penalty
    dcost * sum_k |u_k - u_{k-1}| taken from the blob's controls when move_penalty is on."""
    if move_penalty:
        return _penalised_objective(pack(params), np.asarray(sol_blob, dtype=np.float64), nt - 1, formulation)
    return np.array(sol_blob[21 * (nt - 1)], dtype=np.float64)


def _seconds(P, blob, nt, g, formulation, move_penalty):
    """(batch, 16) d(T J*)/dp from dJ*/dp: T g, and J* + T g for the T_scale column."""
    sens = P[:, 11:12] * g
    sens[:, 11] += objective(P, blob, nt, formulation, move_penalty)
    return sens


def param_sensitivity(params, sol_blob: np.ndarray, nt: int, scheme=0, formulation=0, terminal=0,
                      move_penalty: bool = False, device: int = 0) -> np.ndarray:
    """Post-optimal sensitivity (envelope theorem, include/ascent.h: ascent_param_sensitivity): (batch, 16) dJ*/dp of the
    scaled objective J* to every ascent_params field (PARAM_FIELDS order, per SI unit), at the solution blob (21K+10, batch)
    that solve_batch returned with the same options.  One read of the blob on the device, no extra solve.  Rows of problems
    that did not converge are computed at whatever the blob holds and are meaningless."""
    L, P, B, K, blob, o = _blob_call(params, sol_blob, nt, scheme, formulation, terminal, move_penalty)
    g = np.empty((16, B))
    _lib.check(L.ascent_param_sensitivity(_ptr(P), B, C.byref(o), _ptr(blob), _ptr(g), device, None, 0))
    return np.ascontiguousarray(g.T)


def fly_batch(params, sol_blob: np.ndarray, nt: int, scheme=0, formulation=0, terminal=0, move_penalty: bool = False,
              substeps: int = 0, device: int = 0, want_traj: bool = True, want_local: bool = True) -> FlightResult:
    """Flight verification (include/ascent.h: ascent_fly_batch): integrate the model's ODEs on the device under the control of
    the solution blob (21K+10, batch) that solve_batch returned with the same options -- u_k held over step k, classical RK4 with
    `substeps` steps per collocation step (0: automatic, substeps of at most 0.5 s) -- and compare with the NLP's own
    trajectory.  Returns a FlightResult: the flown trajectory, the local discretisation error of every step (each step flown
    from the NLP's own z_{k-1}), and per problem the miss at the last node, the flown and the NLP's burnout orbit and the largest
    local error (FLIGHT_ROWS).  Rows of problems that did not converge are computed from whatever the blob holds."""
    L, P, B, K, blob, o = _blob_call(params, sol_blob, nt, scheme, formulation, terminal, move_penalty)
    traj = np.empty((10, nt, B)) if want_traj else None
    local = np.empty((K, 7, B)) if want_local else None
    summ = np.empty((len(FLIGHT_ROWS), B))
    _lib.check(L.ascent_fly_batch(_ptr(P), B, C.byref(o), _ptr(blob), int(substeps), _ptr(traj), _ptr(local), _ptr(summ),
                                  device, None, 0))
    return FlightResult(None if traj is None else np.ascontiguousarray(traj.transpose(2, 0, 1)),
                        None if local is None else np.ascontiguousarray(local.transpose(2, 0, 1)),
                        np.ascontiguousarray(summ.T))


def flight_jacobian(params, sol_blob: np.ndarray, nt: int, scheme=0, formulation=0, terminal=0, move_penalty: bool = False,
                    substeps: int = 0, device: int = 0, want_controls: bool = True) -> FlightJacobian:
    """Flight Jacobian (include/ascent.h: ascent_flight_jacobian): the exact derivative of the discrete RK4 flight of fly_batch
    -- the flown last state (scaled) and the flown periapsis / apoapsis altitude (m) -- with respect to the initial state, the
    16 parameter fields (blob held fixed), t_f and every control u_k, at the blob (21K+10, batch).  The open-loop counterpart
    of param_sensitivity: what a dispersed vehicle does under the nominal control.  terminal 2 is refused."""
    L, P, B, K, blob, o = _blob_call(params, sol_blob, nt, scheme, formulation, terminal, move_penalty)
    jac = np.empty((9, 24, B))
    ju = np.empty((9, K, B)) if want_controls else None
    _lib.check(L.ascent_flight_jacobian(_ptr(P), B, C.byref(o), _ptr(blob), int(substeps), _ptr(jac), _ptr(ju), device, None, 0))
    j = jac.transpose(2, 0, 1)
    return FlightJacobian(np.ascontiguousarray(j[:, :, :7]), np.ascontiguousarray(j[:, :, 7:23]), np.ascontiguousarray(j[:, :, 23]),
                          None if ju is None else np.ascontiguousarray(ju.transpose(2, 0, 1)))


def trim_batch(params, sol_blob: np.ndarray, nt: int, scheme=0, formulation=0, terminal=0, move_penalty: bool = False,
               substeps: int = 0, rounds: int = 0, tol: float = 0.0, device: int = 0) -> TrimResult:
    """Trim (include/ascent.h: ascent_trim_batch): least-norm Newton corrections of (t_f, u) of every blob that drive the
    flown terminal conditions to zero, saturated controls (|u_k| >= 0.999) kept where they are; `rounds` rounds (0: 6) to
    `tol` (0: 1e-10) entirely on the device.  Returns a TrimResult: the trimmed blob (states = the flown states of the trimmed
    control; multipliers stale) and the summary (TRIM_ROWS).  terminal 2 is refused."""
    L, P, B, K, blob, o = _blob_call(params, sol_blob, nt, scheme, formulation, terminal, move_penalty)
    out = np.empty_like(blob)
    summ = np.empty((len(TRIM_ROWS), B))
    _lib.check(L.ascent_trim_batch(_ptr(P), B, C.byref(o), _ptr(blob), int(substeps), int(rounds), float(tol), _ptr(out), _ptr(summ),
                                   device, None, 0))
    return TrimResult(out, np.ascontiguousarray(summ.T), nt)


def _history_stride(history, keep_history_samples, K):
    """the node stride of disperse_batch's `history`: 0 for none, 1 for True, else the stride, checked"""
    if history is False or history is None:
        if keep_history_samples:
            raise ValueError("keep_history_samples needs history")
        return 0
    stride = 1 if history is True else int(history)
    if not 1 <= stride <= K:
        raise ValueError(f"history: the node stride must be in 1 .. K = {K}")
    return stride


def _dispersion_draws(xi, seed, samples, K):
    """xi (24 + K, samples) of disperse_batch, contiguous and checked; None draws it from the seed"""
    if xi is None:
        xi = np.random.default_rng(seed).standard_normal((24 + K, int(samples)))
    xi = np.ascontiguousarray(xi, dtype=np.float64)
    if xi.ndim != 2 or xi.shape[0] != 24 + K:
        raise ValueError(f"xi must have shape (24 + K, samples) = ({24 + K}, samples)")
    return xi


def _drift_draws(xi_drift, drift_seed, K, S):
    """xi_drift (8, K, samples) of the drifting flight, contiguous and checked; None draws it from the seed"""
    if xi_drift is None:
        xi_drift = np.random.default_rng(drift_seed).standard_normal((8, K, S))
    xi_drift = np.ascontiguousarray(xi_drift, dtype=np.float64)
    if xi_drift.shape != (8, K, S):
        raise ValueError(f"xi_drift must have shape (8, K, samples) = {(8, K, S)}")
    return xi_drift


def _dispersion_sigmas(z0_sigma, param_sigma, tf_sigma, control_sigma, K, B):
    """The sigma arguments of disperse_batch and linear_corridor, broadcast: -> z0 (B, 7), params (B, 16), tf (B, 1), controls
    (B, K), and the arrays the C ABI takes: sigma [24][B], sigma_u [K][B] or None where control_sigma is None"""
    zs, ps = _sigma_rows(z0_sigma, 7, B, "z0_sigma"), _sigma_rows(param_sigma, 16, B, "param_sigma")
    ts = _sigma_rows(None if tf_sigma is None else np.asarray(tf_sigma, dtype=np.float64)[..., None], 1, B, "tf_sigma")
    us = _sigma_rows(control_sigma, K, B, "control_sigma")
    sig = np.ascontiguousarray(np.concatenate([zs, ps, ts], axis=1).T)
    sig_u = np.ascontiguousarray(us.T) if control_sigma is not None else None
    return zs, ps, ts, us, sig, sig_u


def _feedback_arrays(guidance, K, B):
    """gain_u [7][K][B], gain_t [7][B] or None, stretch_max [B] or None of a GuidanceResult-like object, as the C ABI takes them"""
    gu = np.ascontiguousarray(np.asarray(guidance.gain_u, dtype=np.float64).transpose(2, 1, 0))
    if gu.shape != (7, K, B):
        raise ValueError(f"guidance.gain_u must have shape {(B, K, 7)}")
    gt = None if guidance.gain_t is None else np.ascontiguousarray(np.asarray(guidance.gain_t, dtype=np.float64).T)
    if gt is not None and gt.shape != (7, B):
        raise ValueError(f"guidance.gain_t must have shape {(B, 7)}")
    sm = None if gt is None else _sigma_rows(np.asarray(guidance.stretch_max, dtype=np.float64)[..., None], 1, B, "stretch_max")[:, 0].copy()
    return gu, gt, sm


def _feedforward_arrays(guidance, K, B):
    """ff_u [K][B], ff_t [B], ff_know [16][B] of a GuidanceResult-like object, None where it has none"""
    ffu = getattr(guidance, "ff_u", None)
    fu = ft = fk = None
    if ffu is not None:
        fu = np.ascontiguousarray(np.asarray(ffu, dtype=np.float64).T)
        if fu.shape != (K, B):
            raise ValueError(f"guidance.ff_u must have shape {(B, K)}")
        ft, fk = getattr(guidance, "ff_t", None), getattr(guidance, "ff_know", None)
        if ft is not None:
            ft = np.ascontiguousarray(np.asarray(ft, dtype=np.float64))
            if ft.shape != (B,):
                raise ValueError(f"guidance.ff_t must have shape {(B,)}")
        if fk is not None:
            fk = np.ascontiguousarray(np.asarray(fk, dtype=np.float64).T)
            if fk.shape != (16, B):
                raise ValueError(f"guidance.ff_know must have shape {(B, 16)}")
    return fu, ft, fk


def _nav_sigma_rows(nav_sigma, knowledge_sigma, B):
    """(B, 8): the 1-sigma biases of the state knowledge and the 1-sigma error of theta-hat"""
    ks = _sigma_rows(None if knowledge_sigma is None else np.asarray(knowledge_sigma, dtype=np.float64)[..., None], 1, B,
                     "knowledge_sigma")
    return np.concatenate([_sigma_rows(nav_sigma, 7, B, "nav_sigma"), ks], axis=1)


def _nav_drift(nav_tau, knowledge_tau, nav_steady_sigma, knowledge_steady_sigma, nav_s, dt, B):
    """phi and q (B, 8) of the drifting knowledge channels (include/ascent.h: ascent_disperse_drifting_batch), or (None, None)
    where no time constant is given: phi = exp(-dt / tau), q = steady * sqrt(1 - phi^2), per problem with its own step dt (B,)
    in seconds.  tau None or inf, or a dt that is not finite: frozen, exactly (1, 0).  steady None: the channel's initial sigma of nav_s (B, 8) -- stationary."""
    if nav_tau is None and knowledge_tau is None:
        if nav_steady_sigma is not None or knowledge_steady_sigma is not None:
            raise ValueError("nav_steady_sigma and knowledge_steady_sigma need nav_tau or knowledge_tau")
        return None, None
    tau = np.concatenate([_sigma_rows(np.inf if nav_tau is None else nav_tau, 7, B, "nav_tau"),
                          _sigma_rows(np.asarray(np.inf if knowledge_tau is None else knowledge_tau, dtype=np.float64)[..., None], 1, B,
                                      "knowledge_tau")], axis=1)
    if not np.all(tau > 0):
        raise ValueError("nav_tau and knowledge_tau must be positive (inf or None: frozen)")
    steady = np.zeros((B, 8)) if nav_s is None else nav_s.copy()
    if nav_steady_sigma is not None:
        steady[:, :7] = _sigma_rows(nav_steady_sigma, 7, B, "nav_steady_sigma")
    if knowledge_steady_sigma is not None:
        steady[:, 7:] = _sigma_rows(np.asarray(knowledge_steady_sigma, dtype=np.float64)[..., None], 1, B, "knowledge_steady_sigma")
    if not np.all(steady >= 0):
        raise ValueError("nav_steady_sigma and knowledge_steady_sigma must not be negative")
    dt = np.broadcast_to(np.asarray(dt, dtype=np.float64)[:, None], tau.shape)
    frozen = np.isinf(tau) | ~(np.isfinite(dt) & (dt >= 0))      # a blob without a final time: frozen; the kernels treat that problem as the parent calls do
    with np.errstate(divide="ignore", over="ignore"):
        phi = np.where(frozen, 1.0, np.exp(-np.where(frozen, 0.0, dt) / np.where(frozen, 1.0, tau)))
    q = np.where(frozen, 0.0, steady * np.sqrt(1.0 - phi * phi))
    return np.ascontiguousarray(phi), np.ascontiguousarray(q)


def _guidance_arrays(P, blob, K, B, guidance, nav_sigma, knowledge_sigma, drift=(None,) * 4, S=None, xi_nav=None, nav_seed=1):
    """A guidance law and its navigation error as the C ABI takes them, None where there is none: law = [gain_u, gain_t,
    stretch_max, ff_u, ff_t, ff_know], sigma_nav [8][B] beside nav_s (B, 8), and phi and q (B, 8) of the time constants drift =
    (nav_tau, knowledge_tau, nav_steady_sigma, knowledge_steady_sigma) (_nav_drift).  S: the samples of a Monte Carlo call, which
    takes xi_nav (8, S) with a navigation error -- None draws np.random.default_rng(nav_seed) -- and None without one."""
    law = [*_feedback_arrays(guidance, K, B), *_feedforward_arrays(guidance, K, B)]
    nav_s = sn = None
    if nav_sigma is not None or knowledge_sigma is not None:
        nav_s = _nav_sigma_rows(nav_sigma, knowledge_sigma, B)
        sn = np.ascontiguousarray(nav_s.T)
        if S is not None:
            if xi_nav is None:
                xi_nav = np.random.default_rng(nav_seed).standard_normal((8, S))
            xi_nav = np.ascontiguousarray(xi_nav, dtype=np.float64)
            if xi_nav.shape != (8, S):
                raise ValueError(f"xi_nav must have shape (8, samples) = {(8, S)}")
    else:
        xi_nav = None
    phi = q = None
    if any(v is not None for v in drift):
        phi, q = _nav_drift(*drift, nav_s, blob[21 * K] * P[:, 11] / K, B)
    return law, sn, nav_s, xi_nav, phi, q


def _dispersion_result(stats, smp, effort, xi, sigmas, xi_nav, nav_s, *drift, history=None):
    """DispersionResult from stats_out [82][batch] and samples_out [9 or 12][samples][batch] or None; effort: rows 9.. are EFFORT_ROWS"""
    st, (zs, ps, ts, us) = stats.T, sigmas[:4]
    return DispersionResult(st[:, 0].astype(np.int64), np.ascontiguousarray(st[:, 1:10]), np.ascontiguousarray(st[:, 10:19]),
                            _cov_from_upper(st[:, 19:64]), np.ascontiguousarray(st[:, 64:73]), np.ascontiguousarray(st[:, 73:82]),
                            None if smp is None else np.ascontiguousarray(smp[:9].transpose(2, 1, 0)), xi, zs, ps, ts[:, 0].copy(), us,
                            None if smp is None or not effort else np.ascontiguousarray(smp[9:].transpose(2, 1, 0)),
                            xi_nav if nav_s is not None else None, nav_s, **dict(zip(("xi_drift", "nav_phi", "nav_q"), drift)), history=history)


LINCOV_COLS = tuple(f"z0_{n}" for n in HISTORY_ROWS[:7]) + PARAM_FIELDS + ("tf",) + tuple(f"nav_{n}" for n in HISTORY_ROWS[:7]) + (
    "knowledge",)


@dataclasses.dataclass
class LinearCorridor:
    """The linear covariance corridor of a flight (linear_corridor; include/ascent.h: ascent_covariance_history_batch): the
    first-order covariance of the ten quantities HISTORY_ROWS at every stride-th node and the last -- what
    disperse_batch(history=...) samples, without sampling noise and with the covariances between the quantities.  Problem first."""
    nodes: np.ndarray               # (NJ,) the node numbers, 1-based; the last one is K
    nominal: np.ndarray             # (batch, NJ, 10) the bits of DispersionHistory.nominal
    cov: np.ndarray                 # (batch, NJ, 10, 10) symmetric
    jacobian: np.ndarray | None     # (batch, NJ, 10, 32) d HISTORY_ROWS / d LINCOV_COLS (want_jacobian=True)
    # with a navigation filter (linear_corridor(filter=...); include/ascent.h: ascent_covariance_filtered_batch): the estimation
    # error e = z-hat - z after the update at the node, scaled units; columns 24..30 of both jacobians are then e_0
    # (plain attributes, set by linear_corridor: the dataclass keeps its four fields, so dataclasses.replace, asdict and == do not
    # see them -- copy them by hand)
    nav_cov = None                  # (batch, NJ, 7, 7) its true covariance, symmetric; None without a filter
    nav_jacobian = None             # (batch, NJ, 7, 32) d e / d LINCOV_COLS (want_jacobian=True); None without a filter

    @property
    def std(self) -> np.ndarray:
        """(batch, NJ, 10)"""
        return np.sqrt(np.diagonal(self.cov, axis1=2, axis2=3))

    @property
    def nav_std(self) -> np.ndarray | None:
        """(batch, NJ, 7); None without a filter"""
        return None if self.nav_cov is None else np.sqrt(np.diagonal(self.nav_cov, axis1=2, axis2=3))


NAVFILTER_ROWS = ("status", "first_bad", "meas_nodes", "substeps")
NAVFILTER_MAX_MEAS = 4


def _sym7(rows):
    """(..., 7, 7) symmetric from (..., 28), the upper triangle row by row"""
    iu = np.triu_indices(7)
    full = np.empty(rows.shape[:-1] + (7, 7))
    full[..., iu[0], iu[1]] = rows
    full[..., iu[1], iu[0]] = rows
    return full


@dataclasses.dataclass
class NavigationFilter:
    """A linear Kalman filter designed along a flown solution (navigation_filter; include/ascent.h: ascent_navigation_filter).
    At node k, measurement i corrects the estimate by gain_l[:, k-1, i] times its innovation.  Problem index first."""
    gain_l: np.ndarray              # (batch, K, M, 7); exactly zero at the nodes without a measurement
    cov: np.ndarray                 # (batch, K, 7, 7) the filter's own covariance P-hat after the update at node k = 1 .. K
    status: np.ndarray              # (batch,) 0 ok, 2 frozen: an innovation variance was <= 0 or not finite
    first_bad: np.ndarray           # (batch,) the first such node, 0: none; gain_l and cov are NaN from it on
    meas_nodes: np.ndarray          # (batch,) the number of measurement nodes
    substeps: np.ndarray            # (batch,)
    # the inputs it was designed with
    nav_sigma: np.ndarray           # (batch, 7)
    meas_rows: np.ndarray           # (batch, M, 7)
    meas_sigma: np.ndarray          # (batch, M)
    meas_stride: int
    control_sigma: np.ndarray | None    # (batch, K)
    process_sigma: np.ndarray | None    # (batch, 7)

    @property
    def std(self) -> np.ndarray:
        """(batch, K, 7)"""
        return np.sqrt(np.diagonal(self.cov, axis1=2, axis2=3))


def _measurement_arrays(meas_rows, meas_sigma, B):
    """meas_rows (M, 7) or (batch, M, 7) and meas_sigma (M,) or (batch, M), M in 1 .. 4 -> (rows (B, M, 7), sigma (B, M))"""
    h = np.asarray(meas_rows, dtype=np.float64)
    if h.ndim == 1:
        h = h[None]
    if h.ndim not in (2, 3) or h.shape[-1] != 7 or not 1 <= h.shape[-2] <= NAVFILTER_MAX_MEAS:
        raise ValueError(f"meas_rows must have shape (M, 7) or (batch, M, 7), M in 1 .. {NAVFILTER_MAX_MEAS}")
    M = h.shape[-2]
    try:
        h = np.ascontiguousarray(np.broadcast_to(h, (B, M, 7)))
    except ValueError:
        raise ValueError(f"meas_rows must broadcast to {(B, M, 7)}") from None
    sg = _sigma_rows(meas_sigma, M, B, "meas_sigma")
    if meas_sigma is None or not np.all((sg > 0) & np.isfinite(sg)):
        raise ValueError("meas_sigma must be positive and finite")
    if not np.isfinite(h).all():
        raise ValueError("meas_rows must be finite")
    return h, sg


def navigation_filter(params, sol_blob: np.ndarray, nt: int, *, nav_sigma, meas_rows, meas_sigma, meas_stride: int = 1,
                      control_sigma=None, process_sigma=None, scheme=0, formulation=0, terminal=0, move_penalty: bool = False,
                      substeps: int = 0, device: int = 0) -> NavigationFilter:
    """Designs a linear Kalman filter along the flight of fly_batch (include/ascent.h: ascent_navigation_filter): the forward Riccati
    sweep P-hat_k^- = Phi_k P-hat_{k-1} Phi_k' + control_sigma_k^2 g_k g_k' + diag(process_sigma^2) from P-hat_0 = diag(nav_sigma^2),
    with M scalar measurements meas_rows . z of standard deviation meas_sigma, scaled units, processed one after the other at every
    meas_stride-th node (a stride above K: none).  nav_sigma (7,) or (batch, 7); meas_rows (M, 7) or (batch, M, 7), M in 1 .. 4;
    meas_sigma (M,) or (batch, M), positive; control_sigma a scalar, (K,) or (batch, K) or None; process_sigma (7,) or (batch, 7) or
    None.  Returns a NavigationFilter, which linear_corridor(filter=...) takes."""
    L, P, B, K, blob, o = _blob_call(params, sol_blob, nt, scheme, formulation, terminal, move_penalty)
    stride = int(meas_stride)
    if stride < 1:
        raise ValueError("meas_stride must be at least 1")
    if nav_sigma is None:
        raise ValueError("nav_sigma is required")
    ns = _sigma_rows(nav_sigma, 7, B, "nav_sigma")
    h, sg = _measurement_arrays(meas_rows, meas_sigma, B)
    M = h.shape[1]
    us = None if control_sigma is None else _sigma_rows(control_sigma, K, B, "control_sigma")
    qs = None if process_sigma is None else _sigma_rows(process_sigma, 7, B, "process_sigma")
    if not np.isfinite(ns).all() or (qs is not None and not np.isfinite(qs).all()):
        raise ValueError("nav_sigma and process_sigma must be finite")
    t = lambda a: None if a is None else np.ascontiguousarray(np.moveaxis(a, 0, -1))
    ns_c, us_c, qs_c, h_c, sg_c = t(ns), t(us), t(qs), t(h), t(sg)
    gl, pf, summ = np.empty((M, 7, K, B)), np.empty((28, K, B)), np.empty((len(NAVFILTER_ROWS), B))
    _lib.check(L.ascent_navigation_filter(_ptr(P), B, C.byref(o), _ptr(blob), int(substeps), _ptr(ns_c), _ptr(us_c), _ptr(qs_c),
                                          _ptr(h_c), _ptr(sg_c), M, stride, _ptr(gl), _ptr(pf), _ptr(summ), device, None, 0))
    col = lambda r: summ[r].astype(np.int64)
    return NavigationFilter(np.ascontiguousarray(gl.transpose(3, 2, 0, 1)), _sym7(pf.transpose(2, 1, 0)), col(0), col(1), col(2), col(3),
                            ns, h, sg, stride, us, qs)


def linear_corridor(params, sol_blob: np.ndarray, nt: int, *, param_sigma=None, control_sigma=None, tf_sigma=None, z0_sigma=None,
                    guidance: GuidanceResult | None = None, nav_sigma=None, knowledge_sigma=None, history=True,
                    want_jacobian: bool = True, scheme=0, formulation=0, terminal=0, move_penalty: bool = False, substeps: int = 0,
                    device: int = 0, nav_tau=None, knowledge_tau=None, nav_steady_sigma=None,
                    knowledge_steady_sigma=None, filter: NavigationFilter | None = None) -> LinearCorridor:
    """Linear covariance analysis (include/ascent.h: ascent_covariance_history_batch): the flight disperse_batch(history=...)
    samples, linearised about the nominal flight and swept forward once per problem -- clips ignored, the execution errors of
    control_sigma independent white noise.  The sigmas broadcast as disperse_batch's and `guidance` is taken as there: None the
    open loop, a GuidanceResult the guided flight, with its feed-forward where it carries one; nav_sigma and knowledge_sigma
    need guidance.  history: True, or a node stride in 1 .. K.  Returns a LinearCorridor; jacobian None unless want_jacobian.
    terminal 2 is accepted.
    nav_tau, knowledge_tau, nav_steady_sigma, knowledge_steady_sigma: the time-varying navigation error of disperse_batch, taken
    as there (include/ascent.h: ascent_covariance_drifting_batch); the nav columns of the jacobian stay the derivative with
    respect to the initial errors.  Without them the call is ascent_covariance_history_batch, exactly as before.
    filter: a NavigationFilter (or anything with gain_l (batch, K, M, 7), meas_rows, meas_sigma, meas_stride and nav_sigma): the
    knowledge error the law steers on is that filter's estimation error (include/ascent.h: ascent_covariance_filtered_batch), and
    the result gains nav_cov, nav_std and nav_jacobian.  nav_sigma, the 1-sigma of the initial error, is the filter's unless
    given; guidance None is the open loop, which the filter does not touch.  Not with knowledge_sigma, a feed-forward guidance or
    the nav_tau keywords."""
    L, P, B, K, blob, o = _blob_call(params, sol_blob, nt, scheme, formulation, terminal, move_penalty)
    stride = 1 if history is True else int(history) if history is not False and history is not None else 0
    if not 1 <= stride <= K:
        raise ValueError(f"history: the node stride must be in 1 .. K = {K}")
    _, _, _, _, sig, sig_u = _dispersion_sigmas(z0_sigma, param_sigma, tf_sigma, control_sigma, K, B)
    if filter is not None:
        return _filtered_corridor(L, P, B, K, blob, o, int(substeps), device, stride, sig, sig_u, guidance, filter, nav_sigma, want_jacobian,
                                  knowledge_sigma, (nav_tau, knowledge_tau, nav_steady_sigma, knowledge_steady_sigma))
    if guidance is None and (nav_sigma is not None or knowledge_sigma is not None):
        raise ValueError("nav_sigma and knowledge_sigma need guidance")
    drifting = any(v is not None for v in (nav_tau, knowledge_tau, nav_steady_sigma, knowledge_steady_sigma))
    if guidance is None and drifting:
        raise ValueError("nav_tau, knowledge_tau, nav_steady_sigma and knowledge_steady_sigma need guidance")
    law, sn, phi, q = [None] * 6, None, None, None
    if guidance is not None:
        law, sn, _, _, phi, q = _guidance_arrays(P, blob, K, B, guidance, nav_sigma, knowledge_sigma,
                                                 (nav_tau, knowledge_tau, nav_steady_sigma, knowledge_steady_sigma))
    nodes = history_nodes(K, stride)
    NJ = len(nodes)
    nom, cov = np.empty((10, NJ, B)), np.empty((55, NJ, B))
    jac = np.empty((10, len(LINCOV_COLS), NJ, B)) if want_jacobian else None
    head = (_ptr(P), B, C.byref(o), _ptr(blob), int(substeps), _ptr(sig), _ptr(sig_u), *[_ptr(x) for x in law], _ptr(sn))
    tail = (stride, _ptr(nom), _ptr(cov), _ptr(jac), device, None, 0)
    if phi is not None:
        phi_c, q_c = np.ascontiguousarray(phi.T), np.ascontiguousarray(q.T)
        _lib.check(L.ascent_covariance_drifting_batch(*head, _ptr(phi_c), _ptr(q_c), *tail))
    else:
        _lib.check(L.ascent_covariance_history_batch(*head, *tail))
    full = np.empty((B, NJ, 10, 10))
    iu = np.triu_indices(10)
    full[:, :, iu[0], iu[1]] = cov.transpose(2, 1, 0)
    full[:, :, iu[1], iu[0]] = cov.transpose(2, 1, 0)
    return LinearCorridor(nodes, np.ascontiguousarray(nom.transpose(2, 1, 0)), full,
                          None if jac is None else np.ascontiguousarray(jac.transpose(3, 2, 0, 1)))


def _filtered_corridor(L, P, B, K, blob, o, substeps, device, stride, sig, sig_u, guidance, nf, nav_sigma, want_jacobian, knowledge_sigma,
                       drift):
    """linear_corridor(filter=nf): ascent_covariance_filtered_batch"""
    if knowledge_sigma is not None:
        raise ValueError("knowledge_sigma cannot be combined with filter (the filter does not estimate theta)")
    if any(v is not None for v in drift):
        raise ValueError("nav_tau, knowledge_tau, nav_steady_sigma and knowledge_steady_sigma cannot be combined with filter")
    if guidance is not None and getattr(guidance, "ff_u", None) is not None:
        raise ValueError("a feed-forward guidance cannot be combined with filter")
    gl = np.asarray(nf.gain_l, dtype=np.float64)
    if gl.ndim != 4 or gl.shape[0] != B or gl.shape[1] != K or gl.shape[3] != 7 or not 1 <= gl.shape[2] <= NAVFILTER_MAX_MEAS:
        raise ValueError(f"filter.gain_l must have shape (batch, K, M, 7) = {(B, K, 'M', 7)}, M in 1 .. {NAVFILTER_MAX_MEAS}")
    M = gl.shape[2]
    h, sg = _measurement_arrays(nf.meas_rows, nf.meas_sigma, B)
    if h.shape[1] != M:
        raise ValueError("filter.meas_rows and filter.gain_l disagree on the number of measurements")
    ms = int(nf.meas_stride)
    if ms < 1:
        raise ValueError("filter.meas_stride must be at least 1")
    ns = _sigma_rows(nf.nav_sigma if nav_sigma is None else nav_sigma, 7, B, "nav_sigma")
    if not np.isfinite(ns).all():
        raise ValueError("nav_sigma must be finite")
    law = [None] * 3 if guidance is None else list(_feedback_arrays(guidance, K, B))
    t = lambda a: np.ascontiguousarray(np.moveaxis(a, 0, -1))
    ns_c, h_c, sg_c, gl_c = t(ns), t(h), t(sg), np.ascontiguousarray(gl.transpose(2, 3, 1, 0))
    nodes = history_nodes(K, stride)
    NJ = len(nodes)
    nom, cov, ncov = np.empty((10, NJ, B)), np.empty((55, NJ, B)), np.empty((28, NJ, B))
    jac = np.empty((10, len(LINCOV_COLS), NJ, B)) if want_jacobian else None
    njac = np.empty((7, len(LINCOV_COLS), NJ, B)) if want_jacobian else None
    _lib.check(L.ascent_covariance_filtered_batch(_ptr(P), B, C.byref(o), _ptr(blob), substeps, _ptr(sig), _ptr(sig_u), *[_ptr(x) for x in law],
                                                  _ptr(ns_c), _ptr(gl_c), _ptr(h_c), _ptr(sg_c), M, ms, stride, _ptr(nom), _ptr(cov),
                                                  _ptr(ncov), _ptr(jac), _ptr(njac), device, None, 0))
    full = np.empty((B, NJ, 10, 10))
    iu = np.triu_indices(10)
    full[:, :, iu[0], iu[1]] = cov.transpose(2, 1, 0)
    full[:, :, iu[1], iu[0]] = cov.transpose(2, 1, 0)
    lc = LinearCorridor(nodes, np.ascontiguousarray(nom.transpose(2, 1, 0)), full,
                        None if jac is None else np.ascontiguousarray(jac.transpose(3, 2, 0, 1)))
    lc.nav_cov = _sym7(ncov.transpose(2, 1, 0))
    lc.nav_jacobian = None if njac is None else np.ascontiguousarray(njac.transpose(3, 2, 0, 1))
    return lc


def disperse_batch(params, sol_blob: np.ndarray, nt: int, *, param_sigma=None, control_sigma=None, tf_sigma=None, z0_sigma=None,
                   samples: int = 256, seed: int = 0, xi=None, keep_samples: bool = False, scheme=0, formulation=0, terminal=0,
                   move_penalty: bool = False, substeps: int = 0, device: int = 0, guidance: GuidanceResult | None = None,
                   nav_sigma=None, knowledge_sigma=None, xi_nav=None, nav_seed: int = 1, history=False,
                   keep_history_samples: bool = False, nav_tau=None, knowledge_tau=None, nav_steady_sigma=None,
                   knowledge_steady_sigma=None, xi_drift=None, drift_seed: int = 2, quantiles=None, limits=None, history_limits=None,
                   max_workspace_bytes: int = 2**31) -> DispersionResult:
    """Monte Carlo dispersion (include/ascent.h: ascent_disperse_batch): every blob's control flown `samples` times on the
    device as fly_batch flies it, with the initial state, the 16 parameter fields, t_f and every control perturbed by
    sigma * xi, and the nine end quantities reduced on the device to count, mean, covariance and extrema.  The blob is shared
    by the samples, not tiled.  param_sigma (16,) or (batch, 16) in SI units and control_sigma a scalar, (K,) or (batch, K)
    broadcast like FlightJacobian.sigma's; tf_sigma a scalar or (batch,) in scaled units; z0_sigma (7,) or (batch, 7) in scaled
    units; None: not perturbed.  xi (24 + K, samples): the draws, shared by every problem of the batch (common random numbers);
    None draws np.random.default_rng(seed).standard_normal((24 + K, samples)).  The substeps picked at the nominal blob are held
    for every sample.  keep_samples: also return every sample's rows.  terminal 2 is accepted.
    guidance: a GuidanceResult (or anything with gain_u (batch, K, 7), gain_t (batch, 7) or None and stretch_max): every sample
    steers by that feedback (include/ascent.h: ascent_disperse_guided_batch) and, with keep_samples, `effort` (batch, samples, 3)
    holds EFFORT_ROWS.  None: the open-loop call.
    Where `guidance` carries a feed-forward (ff_u, ff_t, ff_know; guidance_gains(feedforward=...)) or a navigation error is given,
    the call is ascent_disperse_navigated_batch: nav_sigma (7,) or (batch, 7), scaled units, the 1-sigma bias of each sample's state
    knowledge; knowledge_sigma a scalar or (batch,), the 1-sigma error of theta-hat in the units of theta; xi_nav (8, samples) their
    draws, None draws np.random.default_rng(nav_seed).standard_normal((8, samples)).
    history: True, or a node stride in 1 .. K: the same flight through ascent_disperse_history_batch, and `history` of the result a
    DispersionHistory of every stride-th node and the last; everything else of the result has the bits of the call without it.
    keep_history_samples: also every sample's ten quantities at those nodes (the one array of size samples x K).  False: the
    entry points above, exactly as without the keyword.
    Time-varying navigation error (include/ascent.h: ascent_disperse_drifting_batch; needs guidance): nav_tau, seconds, a scalar,
    (7,) or (batch, 7), and knowledge_tau, a scalar or (batch,), make each knowledge error a first-order Gauss-Markov sequence with
    that correlation time, phi = exp(-dt / tau) per step of dt = t_f T_scale / K seconds; None or inf: frozen, the bias per flight
    of the navigated call.  nav_steady_sigma and knowledge_steady_sigma: the stationary 1-sigma the channel relaxes to, q = steady
    sqrt(1 - phi^2); None: the channel's initial sigma (a stationary process), 0: pure decay.  xi_drift (8, K, samples): the
    driving draws, None draws np.random.default_rng(drift_seed).standard_normal((8, K, samples)).  The result keeps xi_drift,
    nav_phi and nav_q.  Without `history` the call runs with stride K and the result's history is None.  Without these keywords
    the calls are exactly those above.
    quantiles: a sequence of 1 .. 16 probabilities in [0, 1]; limits (n_limits, 12) or (batch, n_limits, 12), n_limits 1 .. 16, in
    the units of the nine end quantities and EFFORT_ROWS, NaN: no limit here; history_limits likewise with the 10 columns of
    HISTORY_ROWS (needs history, and as many limits as `limits` where both are given).  The flight runs through
    ascent_disperse_quantiles_batch, which selects behind it on the device: the result gains quantile_probs, quantiles,
    effort_quantiles (guided flights), below and effort_below, its history quantiles and below -- order statistics over the valid
    samples, exact (include/ascent.h: ascent_sample_quantiles); everything else has the bits of the call without the keywords.
    Limits without quantiles report the median.  The call keeps (12 + 10 NJ) samples batch doubles on the device: where
    ascent_disperse_quantiles_bytes exceeds max_workspace_bytes the batch is flown in runs of consecutive problems that fit
    (quantile_chunks; a problem's rows do not depend on the batch), ValueError where one problem does not.  keep_samples and
    keep_history_samples with these keywords fly the flight a second time through the calls above for the samples.
    The analysis workspace of a device only grows: after such a call up to max_workspace_bytes stay claimed on the device for
    the life of the process.  Without the three keywords the calls are exactly those above."""
    L, P, B, K, blob, o = _blob_call(params, sol_blob, nt, scheme, formulation, terminal, move_penalty)
    if quantiles is not None or limits is not None or history_limits is not None:
        if history_limits is not None and (history is False or history is None):
            raise ValueError("history_limits needs history")
        kw = dict(param_sigma=param_sigma, control_sigma=control_sigma, tf_sigma=tf_sigma, z0_sigma=z0_sigma, samples=samples, seed=seed,
                  xi=xi, scheme=scheme, formulation=formulation, terminal=terminal, move_penalty=move_penalty, substeps=substeps,
                  device=device, guidance=guidance, nav_sigma=nav_sigma, knowledge_sigma=knowledge_sigma, xi_nav=xi_nav,
                  nav_seed=nav_seed, history=history, nav_tau=nav_tau, knowledge_tau=knowledge_tau, nav_steady_sigma=nav_steady_sigma,
                  knowledge_steady_sigma=knowledge_steady_sigma, xi_drift=xi_drift, drift_seed=drift_seed)
        return _disperse_quantiles(params, sol_blob, nt, kw, keep_samples, keep_history_samples, quantiles, limits, history_limits,
                                   int(max_workspace_bytes))
    stride = _history_stride(history, keep_history_samples, K)
    xi = _dispersion_draws(xi, seed, samples, K)
    S = xi.shape[1]
    zs, ps, ts, us, sig, sig_u = _dispersion_sigmas(z0_sigma, param_sigma, tf_sigma, control_sigma, K, B)
    ffu = getattr(guidance, "ff_u", None)
    navigated = ffu is not None or nav_sigma is not None or knowledge_sigma is not None
    if navigated and guidance is None:
        raise ValueError("nav_sigma and knowledge_sigma need guidance")
    nav_s = None
    sigmas = (zs, ps, ts, us, sig, sig_u)
    drifting = any(v is not None for v in (nav_tau, knowledge_tau, nav_steady_sigma, knowledge_steady_sigma, xi_drift))
    if drifting:
        if guidance is None:
            raise ValueError("nav_tau, knowledge_tau, nav_steady_sigma, knowledge_steady_sigma and xi_drift need guidance")
        return _disperse_drifting(L, P, B, K, blob, o, int(substeps), device, xi, sigmas, guidance, nav_sigma,
                                  knowledge_sigma, xi_nav, nav_seed, nav_tau, knowledge_tau, nav_steady_sigma, knowledge_steady_sigma,
                                  xi_drift, drift_seed, stride, keep_samples, keep_history_samples)
    stats = np.empty((82, B))
    smp = np.empty((9 if guidance is None and not stride else 12, S, B)) if keep_samples else None
    hist = hsmp = None
    if stride:
        NJ = len(history_nodes(K, stride))
        hist = np.empty((52, NJ, B))
        hsmp = np.empty((10, NJ, S, B)) if keep_history_samples else None

    def with_history(*a):      # the arguments from gain_u to sigma_nav, as the navigated call takes them
        _lib.check(L.ascent_disperse_history_batch(_ptr(P), B, C.byref(o), _ptr(blob), int(substeps), S, _ptr(xi), _ptr(sig), _ptr(sig_u),
                                                   *[_ptr(x) for x in a], stride, _ptr(stats), _ptr(smp), _ptr(hist), _ptr(hsmp),
                                                   device, None, 0))
    if guidance is None and stride:
        with_history(*[None] * 8)
    elif guidance is None:
        _lib.check(L.ascent_disperse_batch(_ptr(P), B, C.byref(o), _ptr(blob), int(substeps), S, _ptr(xi), _ptr(sig), _ptr(sig_u),
                                           _ptr(stats), _ptr(smp), device, None, 0))
    else:
        law, sn, nav_s, xi_nav, _, _ = _guidance_arrays(P, blob, K, B, guidance, nav_sigma, knowledge_sigma, S=S, xi_nav=xi_nav,
                                                        nav_seed=nav_seed)
        if stride:
            with_history(*law, xi_nav, sn)
        elif not navigated:
            _lib.check(L.ascent_disperse_guided_batch(_ptr(P), B, C.byref(o), _ptr(blob), int(substeps), S, _ptr(xi), _ptr(sig), _ptr(sig_u),
                                                      *[_ptr(x) for x in law[:3]], _ptr(stats), _ptr(smp), device, None, 0))
        else:
            _lib.check(L.ascent_disperse_navigated_batch(_ptr(P), B, C.byref(o), _ptr(blob), int(substeps), S, _ptr(xi), _ptr(sig), _ptr(sig_u),
                                                         *[_ptr(x) for x in law], _ptr(xi_nav), _ptr(sn), _ptr(stats), _ptr(smp),
                                                         device, None, 0))
    return _dispersion_result(stats, smp, guidance is not None, xi, sigmas, xi_nav, nav_s,
                              history=_history_result(K, stride, hist, hsmp) if stride else None)


def _history_result(K, stride, hist, hsmp):
    """DispersionHistory from hist_out [52][NJ][batch] and hist_samples_out [10][NJ][samples][batch] or None"""
    h = hist.transpose(2, 1, 0)      # (batch, NJ, 52)
    return DispersionHistory(history_nodes(K, stride), h[:, :, 0].astype(np.int64), np.ascontiguousarray(h[:, :, 1:11]),
                             np.ascontiguousarray(h[:, :, 11:21]), np.ascontiguousarray(h[:, :, 21:31]),
                             np.ascontiguousarray(h[:, :, 31:41]), np.ascontiguousarray(h[:, :, 41:51]), h[:, :, 51].astype(np.int64),
                             None if hsmp is None else np.ascontiguousarray(hsmp.transpose(3, 2, 1, 0)))


def _disperse_drifting(L, P, B, K, blob, o, substeps, device, xi, sigmas, guidance, nav_sigma, knowledge_sigma, xi_nav, nav_seed, nav_tau,
                       knowledge_tau, nav_steady_sigma, knowledge_steady_sigma, xi_drift, drift_seed, stride, keep_samples,
                       keep_history_samples):
    """disperse_batch with the time-varying navigation error: one call of ascent_disperse_drifting_batch"""
    sig, sig_u = sigmas[4:]
    S = xi.shape[1]
    law, sn, nav_s, xi_nav, phi, q = _guidance_arrays(P, blob, K, B, guidance, nav_sigma, knowledge_sigma,
                                                      (nav_tau, knowledge_tau, nav_steady_sigma, knowledge_steady_sigma), S, xi_nav, nav_seed)
    if phi is None:
        raise ValueError("xi_drift needs nav_tau or knowledge_tau")
    xi_drift = _drift_draws(xi_drift, drift_seed, K, S)
    call_stride = stride if stride else K
    NJ = len(history_nodes(K, call_stride))
    stats = np.empty((82, B))
    smp = np.empty((12, S, B)) if keep_samples else None
    hist = np.empty((52, NJ, B))
    hsmp = np.empty((10, NJ, S, B)) if keep_history_samples else None
    phi_c, q_c = np.ascontiguousarray(phi.T), np.ascontiguousarray(q.T)
    _lib.check(L.ascent_disperse_drifting_batch(_ptr(P), B, C.byref(o), _ptr(blob), substeps, S, _ptr(xi), _ptr(sig), _ptr(sig_u),
                                                *[_ptr(x) for x in law], _ptr(xi_nav), _ptr(sn), _ptr(phi_c), _ptr(q_c), _ptr(xi_drift),
                                                call_stride, _ptr(stats), _ptr(smp), _ptr(hist), _ptr(hsmp), device, None, 0))
    return _dispersion_result(stats, smp, True, xi, sigmas, xi_nav, nav_s, xi_drift, phi, q,
                              history=_history_result(K, stride, hist, hsmp) if stride else None)


def quantile_chunks(batch: int, bytes_of, max_bytes: int) -> list:
    """Runs (start, stop) of consecutive problems that tile range(batch), each with bytes_of(stop - start) <= max_bytes; bytes_of
    does not decrease with the number of problems.  The runs are as long as fits and equal but for the last.  ValueError where
    one problem does not fit."""
    if batch < 1:
        raise ValueError("batch must be at least 1")
    one = int(bytes_of(1))
    if one > max_bytes:
        raise ValueError(f"one problem needs a device workspace of {one} bytes, more than max_workspace_bytes = {max_bytes}")
    lo, hi = 1, batch      # bytes_of(lo) fits
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if int(bytes_of(mid)) <= max_bytes:
            lo = mid
        else:
            hi = mid - 1
    return [(a, min(a + lo, batch)) for a in range(0, batch, lo)]


def _quantile_probs(quantiles):
    probs = np.ascontiguousarray([0.5] if quantiles is None else quantiles, dtype=np.float64).reshape(-1)
    if not 1 <= probs.size <= 16:
        raise ValueError("quantiles: 1 .. 16 probabilities")
    if not np.all((probs >= 0.0) & (probs <= 1.0)):
        raise ValueError("quantiles: every probability must be in [0, 1]")
    return probs


def _limit_rows(limits, cols, B, what):
    """limits (n_limits, cols) or (batch, n_limits, cols) -> [n_limits][cols][batch] as the C ABI takes them, or None"""
    if limits is None:
        return None
    a = np.asarray(limits, dtype=np.float64)
    if a.ndim == 2:
        a = np.broadcast_to(a[None], (B,) + a.shape)
    if a.ndim != 3 or a.shape[0] != B or a.shape[2] != cols or not 1 <= a.shape[1] <= 16:
        raise ValueError(f"{what} must have shape (n_limits, {cols}) or (batch, n_limits, {cols}) with 1 .. 16 limits")
    return np.ascontiguousarray(a.transpose(1, 2, 0))


def _disperse_quantiles(params, sol_blob, nt, kw, keep_samples, keep_history_samples, quantiles, limits, history_limits, max_bytes):
    """disperse_batch with quantiles / limits / history_limits: ascent_disperse_quantiles_batch on runs of problems that fit"""
    L, P, B, K, blob, o = _blob_call(params, sol_blob, nt, kw["scheme"], kw["formulation"], kw["terminal"], kw["move_penalty"])
    guidance, device, substeps = kw["guidance"], kw["device"], int(kw["substeps"])
    stride = _history_stride(kw["history"], keep_history_samples, K)
    probs = _quantile_probs(quantiles)
    lim, hlim = _limit_rows(limits, 12, B, "limits"), _limit_rows(history_limits, 10, B, "history_limits")
    if lim is not None and hlim is not None and lim.shape[0] != hlim.shape[0]:
        raise ValueError("limits and history_limits must hold the same number of limits")
    NL = lim.shape[0] if lim is not None else hlim.shape[0] if hlim is not None else 0
    xi = _dispersion_draws(kw["xi"], kw["seed"], kw["samples"], K)
    S = xi.shape[1]
    sigmas = _dispersion_sigmas(kw["z0_sigma"], kw["param_sigma"], kw["tf_sigma"], kw["control_sigma"], K, B)
    sig, sig_u = sigmas[4:]
    drift = (kw["nav_tau"], kw["knowledge_tau"], kw["nav_steady_sigma"], kw["knowledge_steady_sigma"])
    xi_drift, xi_nav = kw["xi_drift"], kw["xi_nav"]
    drifting = any(v is not None for v in drift + (xi_drift,))
    navigated = getattr(guidance, "ff_u", None) is not None or kw["nav_sigma"] is not None or kw["knowledge_sigma"] is not None
    if guidance is None and navigated:
        raise ValueError("nav_sigma and knowledge_sigma need guidance")
    if guidance is None and drifting:
        raise ValueError("nav_tau, knowledge_tau, nav_steady_sigma, knowledge_steady_sigma and xi_drift need guidance")
    law, sn, nav_s, phi, q = [None] * 6, None, None, None, None
    if guidance is not None:
        law, sn, nav_s, xi_nav, phi, q = _guidance_arrays(P, blob, K, B, guidance, kw["nav_sigma"], kw["knowledge_sigma"],
                                                          drift if drifting else (None,) * 4, S, xi_nav, kw["nav_seed"])
    else:
        xi_nav = None
    phi_c = q_c = None
    if drifting:
        if phi is None:
            raise ValueError("xi_drift needs nav_tau or knowledge_tau")
        xi_drift = _drift_draws(xi_drift, kw["drift_seed"], K, S)
        phi_c, q_c = np.ascontiguousarray(phi.T), np.ascontiguousarray(q.T)
    call_stride = stride if stride or not drifting else K      # (the drifting call has no form without history)
    NJ = len(history_nodes(K, call_stride)) if call_stride else 0
    NP = probs.size

    def bytes_of(n):
        return L.ascent_disperse_quantiles_bytes(n, nt, S, call_stride)
    if bytes_of(1) < 0:
        _lib.check(int(bytes_of(1)))
    stats, hist = np.empty((82, B)), np.empty((52, NJ, B)) if call_stride else None
    quant, below = np.empty((NP, 12, B)), np.empty((NL, 12, B)) if lim is not None else None
    hquant = np.empty((NP, 10, NJ, B)) if stride else None
    hbelow = np.empty((NL, 10, NJ, B)) if hlim is not None else None
    per_problem = [blob, sig, sig_u, *law, sn, phi_c, q_c, lim, hlim]
    outs = [stats, hist, quant, below, hquant, hbelow]
    for a, b in quantile_chunks(B, bytes_of, max_bytes):
        whole = a == 0 and b == B
        cut = [x if x is None or whole else np.ascontiguousarray(x[..., a:b]) for x in per_problem]
        part = [x if x is None or whole else np.empty(x.shape[:-1] + (b - a,)) for x in outs]
        cb, cs, csu, *claw = cut[:9]
        csn, cphi, cq, clim, chlim = cut[9:]
        _lib.check(L.ascent_disperse_quantiles_batch(
            _ptr(np.ascontiguousarray(P[a:b])), b - a, C.byref(o), _ptr(cb), substeps, S, _ptr(xi), _ptr(cs), _ptr(csu),
            *[_ptr(x) for x in claw], _ptr(xi_nav), _ptr(csn), _ptr(cphi), _ptr(cq), _ptr(xi_drift if drifting else None), call_stride,
            _ptr(part[0]), _ptr(part[1]), _ptr(probs), NP, _ptr(clim), _ptr(chlim), NL, _ptr(part[2]), _ptr(part[3]), _ptr(part[4]),
            _ptr(part[5]), device, None, 0))
        if not whole:
            for x, y in zip(outs, part):
                if x is not None:
                    x[..., a:b] = y
    if keep_samples or keep_history_samples:      # the samples themselves: the calls without the keywords
        res = disperse_batch(params, sol_blob, nt, keep_samples=keep_samples, keep_history_samples=keep_history_samples,
                             **{**kw, "xi": xi, "xi_nav": xi_nav, "xi_drift": xi_drift if drifting else None})
    else:
        tail = (xi_drift, phi, q) if drifting else ()
        res = _dispersion_result(stats, None, guidance is not None, xi, sigmas, xi_nav, nav_s, *tail,
                                 history=_history_result(K, stride, hist, None) if stride else None)
    res.quantile_probs = probs
    res.quantiles = np.ascontiguousarray(quant[:, :9].transpose(2, 0, 1))
    if guidance is not None:
        res.effort_quantiles = np.ascontiguousarray(quant[:, 9:].transpose(2, 0, 1))
    if below is not None:
        res.below = np.ascontiguousarray(below[:, :9].transpose(2, 0, 1)).astype(np.int64)
        if guidance is not None:
            res.effort_below = np.ascontiguousarray(below[:, 9:].transpose(2, 0, 1)).astype(np.int64)
    if stride:
        res.history.quantiles = np.ascontiguousarray(hquant.transpose(3, 2, 0, 1))
        if hbelow is not None:
            res.history.below = np.ascontiguousarray(hbelow.transpose(3, 2, 0, 1)).astype(np.int64)
    return res


def sample_quantiles(values, probs, valid_quantities: int, limits=None, device: int = 0):
    """Order statistics of sample rows on the device (include/ascent.h: ascent_sample_quantiles).  values (Q, G, samples, batch) or
    (Q, samples, batch), the layouts of the C ABI's hist_samples_out and samples_out; a sample is valid where its first
    valid_quantities rows are finite.  probs: 1 .. 16 probabilities; limits (n_limits, Q) or (n_limits, Q, batch), None: no counts.
    Returns (count, quantiles, below): count (G, batch) int64 the valid samples, quantiles (n_probs, Q, G, batch) numpy's "linear"
    quantiles over them (NaN where there is none), below (n_limits, Q, G, batch) int64 the valid samples at or below each limit or
    None; without the G axis where values came without it."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    flat = v.ndim == 3
    if flat:
        v = v[:, None]
    if v.ndim != 4 or 0 in v.shape:
        raise ValueError("values must have shape (Q, G, samples, batch) or (Q, samples, batch)")
    Q, G, S, B = v.shape
    probs = _quantile_probs(probs)
    lim = None
    if limits is not None:
        lim = np.asarray(limits, dtype=np.float64)
        if lim.ndim == 2:
            lim = np.broadcast_to(lim[:, :, None], lim.shape + (B,))
        if lim.ndim != 3 or lim.shape[1:] != (Q, B) or not 1 <= lim.shape[0] <= 16:
            raise ValueError("limits must have shape (n_limits, Q) or (n_limits, Q, batch) with 1 .. 16 limits")
        lim = np.ascontiguousarray(lim)
    NL = 0 if lim is None else lim.shape[0]
    count, quant = np.empty((G, B)), np.empty((probs.size, Q, G, B))
    below = np.empty((NL, Q, G, B)) if lim is not None else None
    _lib.check(_lib.load().ascent_sample_quantiles(_ptr(v), Q, G, int(valid_quantities), S, B, _ptr(probs), probs.size, _ptr(lim), NL,
                                                   _ptr(count), _ptr(quant), _ptr(below), device, None, 0))
    count = count.astype(np.int64)
    if below is not None:
        below = below.astype(np.int64)
    if flat:
        return count[0], quant[:, :, 0], None if below is None else below[:, :, 0]
    return count, quant, below


def guidance_gains(params, sol_blob: np.ndarray, nt: int, scheme=0, formulation=0, terminal=0, move_penalty: bool = False,
                   substeps: int = 0, device: int = 0, cond_weights=(1e6, 1e6, 1e6), control_weight=1.0, cutoff_weight=1.0,
                   stretch_max=0.5, want_jacobian: bool = True, feedforward=None, knowledge=None) -> GuidanceResult:
    """Guidance gains (include/ascent.h: ascent_guidance_gains): the linear-quadratic feedback about the flight of a blob
    (21K+10, batch) -- normally a trimmed one, since the target is what the nominal control reaches -- from a backward Riccati
    sweep over the step records of the flight Jacobian.  cond_weights (3,) or (batch, 3): the weights q of the squared
    deviations of the trim's three conditions at the last node; control_weight r_u and cutoff_weight r_t, scalars or (batch,),
    weigh du_k^2 and the squared relative stretch tau^2 of the last step; stretch_max bounds |tau| (0: steering only).  In double
    precision the gains lose digits as q grows (about 1e-12 at 1e6, 3e-5 at 1e12).  Returns a GuidanceResult; pass it to
    disperse_batch(..., guidance=...).  terminal 2 is refused.
    feedforward: a PARAM_FIELDS name (the unit direction in that field: "Ft" is newtons of thrust), (16,) or (batch, 16): the
    direction d of a constant parameter deviation theta * d the vehicle has an estimate theta-hat of; the result then carries the
    feed-forward gains ff_u, ff_t (include/ascent.h: ascent_guidance_feedforward; the feedback gains are unchanged bit for bit),
    a (batch, 7) summary and, with want_jacobian, jacobian_nav and a closed-loop Jacobian whose parameter columns account for
    theta-hat = knowledge . (the 16 parameter deviations); knowledge (16,) or (batch, 16), None: d / (d . d), the vehicle knows
    theta exactly."""
    L, P, B, K, blob, o = _blob_call(params, sol_blob, nt, scheme, formulation, terminal, move_penalty)
    w = np.ascontiguousarray(np.concatenate([_sigma_rows(cond_weights, 3, B, "cond_weights")] + [
        _sigma_rows(np.asarray(v, dtype=np.float64)[..., None], 1, B, n)
        for v, n in ((control_weight, "control_weight"), (cutoff_weight, "cutoff_weight"), (stretch_max, "stretch_max"))], axis=1).T)
    gu, gt, summ = np.empty((7, K, B)), np.empty((7, B)), np.empty((len(GUIDE_ROWS), B))
    jac = np.empty((9, 24, B)) if want_jacobian else None
    ju = np.empty((9, K, B)) if want_jacobian else None
    ff = {}
    if feedforward is None:
        if knowledge is not None:
            raise ValueError("knowledge needs feedforward")
        _lib.check(L.ascent_guidance_gains(_ptr(P), B, C.byref(o), _ptr(blob), int(substeps), _ptr(w), _ptr(gu), _ptr(gt), _ptr(summ),
                                           _ptr(jac), _ptr(ju), device, None, 0))
    else:
        if isinstance(feedforward, str):
            if feedforward not in PARAM_FIELDS:
                raise ValueError(f"feedforward must be one of {PARAM_FIELDS} or a direction of 16 fields")
            feedforward = np.eye(16)[PARAM_FIELDS.index(feedforward)]
        dirs = _sigma_rows(feedforward, 16, B, "feedforward")
        if knowledge is None:
            dd = np.einsum("bi,bi->b", dirs, dirs)[:, None]
            with np.errstate(all="ignore"):
                know = np.where(dd > 0, dirs / np.where(dd > 0, dd, 1.0), dirs * 0.0)
        else:
            know = _sigma_rows(knowledge, 16, B, "knowledge")
        dT, kT = np.ascontiguousarray(dirs.T), np.ascontiguousarray(know.T)
        summ = np.empty((len(GUIDE_FF_ROWS), B))
        fu, ft = np.empty((K, B)), np.empty(B)
        jn = np.empty((9, 8, B)) if want_jacobian else None
        _lib.check(L.ascent_guidance_feedforward(_ptr(P), B, C.byref(o), _ptr(blob), int(substeps), _ptr(w), _ptr(dT), _ptr(kT), _ptr(gu),
                                                 _ptr(gt), _ptr(fu), _ptr(ft), _ptr(summ), _ptr(jac), _ptr(ju), _ptr(jn), device, None, 0))
        ff = dict(ff_u=np.ascontiguousarray(fu.T), ff_t=ft, ff_dir=dirs, ff_know=know,
                  jacobian_nav=None if jn is None else np.ascontiguousarray(jn.transpose(2, 0, 1)))
    J = None
    if want_jacobian:
        j = jac.transpose(2, 0, 1)
        J = FlightJacobian(np.ascontiguousarray(j[:, :, :7]), np.ascontiguousarray(j[:, :, 7:23]), np.ascontiguousarray(j[:, :, 23]),
                           np.ascontiguousarray(ju.transpose(2, 0, 1)))
    return GuidanceResult(np.ascontiguousarray(gu.transpose(2, 1, 0)), np.ascontiguousarray(gt.T), np.ascontiguousarray(summ.T),
                          w[5].copy(), J, **ff)


def eval_nodes(params, iterate: np.ndarray, nt: int = 200, device: int = 0, path="auto", scheme=0, formulation=0):
    """Per-step defects (7K,batch), Jacobian blocks (8K,batch), Hessian blocks (10K,batch).
    path: "auto" (the kernels solve_batch would run for this batch), "fused", "split_lane", "split_wide"
    (enum ascent_path, include/ascent.h); the split paths take scheme 1 and formulation 1 as well."""
    L, P, B, K, it, o = _blob_call(params, iterate, nt, scheme, formulation, what="iterate")
    d, j, h = np.empty((7 * K, B)), np.empty((8 * K, B)), np.empty((10 * K, B))
    _lib.check(L.ascent_eval_nodes_path(_ptr(P), B, C.byref(o), _ptr(it), _ptr(d), _ptr(j), _ptr(h), device,
                                        _lib.PATHS[path]))
    return d, j, h


def kkt_step(params, iterate: np.ndarray, mu, delta_w, nt: int = 200, device: int = 0, path="auto", scheme=0,
             formulation=0, terminal=0, move_penalty: bool = False):
    """One Newton step of the barrier problem at `iterate` -> (step blob, inertia flags); `path` as in eval_nodes.
    move_penalty (paths "persist" and "dense"): with the l1 move penalty; the slack pairs, which the blob does not carry, are
    set around the iterate's own movement (p = max(du, 0) + 1e-4, n = max(-du, 0) + 1e-4, z_p = z_n = dcost, lambda_u = 0)."""
    L, P, B, K, it, o = _blob_call(params, iterate, nt, scheme, formulation, terminal, move_penalty, what="iterate")
    mu = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float64), (B,)))
    dw = np.ascontiguousarray(np.broadcast_to(np.asarray(delta_w, dtype=np.float64), (B,)))
    step = np.empty_like(it)
    inertia = np.empty(B, dtype=np.int32)
    _lib.check(L.ascent_kkt_step_path(_ptr(P), B, C.byref(o), _ptr(it), _ptr(mu), _ptr(dw), _ptr(step), _ptr(inertia),
                                      device, _lib.PATHS[path]))
    return step, inertia


def dense_records(params, iterate: np.ndarray, nt: int = 200, scheme=2, device: int = 0) -> np.ndarray:
    """The dense stage records of the dense-block path at `iterate`: (batch, K, 6, 8, 8) -- grids d c_k/d z_{k-1}, d c_k/d z_k,
    the three Hessian blocks of lambda_k'c_k and the vector grid (rows c_k, d c_k/du_k, d c_k/d tf, the two (z, tf) Hessian
    columns); see ascent_dense_records in include/ascent.h."""
    L, P, B, K, it, o = _blob_call(params, iterate, nt, scheme, what="iterate")
    rec = np.empty((B, K, 6, 8, 8))
    _lib.check(L.ascent_dense_records(_ptr(P), B, C.byref(o), _ptr(it), _ptr(rec), device))
    return rec


def coast_batch(params, final_state: np.ndarray, coast_nodes: int = 200, device: int = 0) -> dict:
    """Kepler-exact coast arc from every problem's burnout state (4, batch: scaled x, y, xdot, ydot) to the next apoapsis of
    its orbit (ascent_coast_batch): dict(traj (4, coast_nodes+1, batch), tf (batch,) = duration / T_scale,
    periapsis_alt, apoapsis_alt (m)).  Node 0 is the input state; a state of specific energy >= 0 gives a NaN arc and duration
    and an apoapsis of +inf (include/ascent.h)."""
    L = _lib.load()
    P = pack(params)
    B = P.shape[0]
    fs = np.ascontiguousarray(final_state, dtype=np.float64)
    if fs.shape != (4, B):
        raise ValueError(f"final_state must have shape {(4, B)}")
    traj = np.empty((4, coast_nodes + 1, B)); tf = np.empty(B); aps = np.empty((2, B))
    _lib.check(L.ascent_coast_batch(_ptr(P), B, _ptr(fs), coast_nodes, _ptr(traj), _ptr(tf), _ptr(aps), device, None, 0))
    return dict(traj=traj, tf=tf, periapsis_alt=aps[0], apoapsis_alt=aps[1])


def kkt_solve(diag, lower, upper, rhs, border=None, border_diag=None, algo="pcr", device: int = 0):
    """Generic bordered block-tridiagonal solve on the GPU (ascent_kkt_solve, include/ascent.h).
    diag / lower / upper: (batch, n, bs, bs); rhs: (batch, n*bs + nb); border: (batch, n, bs, nb); border_diag: (batch, nb, nb).
    algo: "thomas" (block elimination serial in the node index) or "pcr" (parallel cyclic reduction over the nodes).
    Returns (solution (batch, n*bs + nb), device milliseconds of the solve)."""
    L = _lib.load()
    D = np.ascontiguousarray(diag, dtype=np.float64)
    B, n, bs, _ = D.shape
    Lo = np.ascontiguousarray(lower, dtype=np.float64); Up = np.ascontiguousarray(upper, dtype=np.float64)
    nb = 0 if border is None else int(np.shape(border)[-1])
    r = np.ascontiguousarray(rhs, dtype=np.float64)
    if Lo.shape != D.shape or Up.shape != D.shape or r.shape != (B, n * bs + nb):
        raise ValueError("inconsistent shapes")
    bo = bd = None
    if nb:
        bo = np.ascontiguousarray(border, dtype=np.float64); bd = np.ascontiguousarray(border_diag, dtype=np.float64)
        if bo.shape != (B, n, bs, nb) or bd.shape != (B, nb, nb):
            raise ValueError("inconsistent border shapes")
    sol = np.empty_like(r)
    _lib.check(L.ascent_kkt_solve(B, n, bs, nb, _ptr(D), _ptr(Lo), _ptr(Up), _ptr(bo), _ptr(bd), _ptr(r), _ptr(sol), device,
                                  {"thomas": 0, "pcr": 1}[algo]))
    return sol, L.ascent_last_kernel_ms(device)


def solve_batch_torch(params_t, nt: int = 200, tol: float = 1e-9, max_iter: int = 300, guess_t=None,
                      warm_start: int = 0, mu_init: float = 0.0, want_traj: bool = True, want_blob: bool = False,
                      out: dict | None = None, sync: bool = False, coarse_nodes: int = 0, scheme=0,
                      formulation=0, move_penalty: bool = False, terminal=0, path: str = "auto",
                      sensitivity: bool = False, flight: bool = False) -> dict:
    """Device-resident variant: `params_t` is a torch float64 CUDA tensor (batch,16); all outputs are
    torch CUDA tensors (allocated here unless passed in `out`).  Enqueues on torch's current stream
    and returns without waiting unless sync=True.  torch is only the owner of device memory/streams.
    Options as solve_batch (scheme, formulation, terminal, path, move_penalty: the weights params_t[:, 15] must be
    positive then -- checked by the kernels that set the starting point, with no host read: a problem whose weight is
    zero, negative or NaN comes back with status 4 (invalid_problem), 0 iterations and its starting point in tf / traj /
    blob, and the rest of the batch is solved as without it).
    sensitivity: also out["sensitivity"], (batch, 16) d(T_scale J*)/dp as solve_batch(sensitivity=True) computes it (NaN rows
    for problems that did not converge), enqueued on the same stream right after the solve: no host read.
    flight: also out["flight_summary"] (batch, 10), out["flight_traj"] (batch, 10, nt) and out["flight_local"] (batch, K, 7) as
    solve_batch(flight=True) computes them (NaN rows for problems that did not converge), enqueued on the same stream after
    the solve: no host read."""
    import torch
    L = _lib.load()
    _lib.require_single_hip_runtime()
    if not (params_t.is_cuda and params_t.dtype == torch.float64 and params_t.is_contiguous()):
        raise ValueError("params_t must be a contiguous float64 CUDA tensor")
    B = params_t.shape[0]
    dev = params_t.device
    rows = blob_rows(nt)
    out = out if out is not None else {}
    def buf(name, shape, dtype):
        t = out.get(name)
        if t is None:
            t = out[name] = torch.empty(shape, dtype=dtype, device=dev)
        elif not (t.device == dev and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
            raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}")
        return t
    if params_t.dim() != 2 or params_t.shape[1] != 16:
        raise ValueError("params_t must have shape (batch, 16)")
    if warm_start not in (0, 1, 2) or (warm_start and guess_t is None):
        raise ValueError("warm_start 1/2 needs guess_t")
    if guess_t is not None and not (guess_t.device == dev and guess_t.dtype == torch.float64 and guess_t.is_contiguous()
                                    and tuple(guess_t.shape) == (rows, B)):
        raise ValueError(f"guess_t must be a contiguous float64 tensor of shape {(rows, B)} on {dev}")
    tf = buf("tf", (B,), torch.float64)
    status = buf("status", (B,), torch.int32)
    iters = buf("iters", (B,), torch.int32)
    traj = buf("traj", (10, nt, B), torch.float64) if want_traj else None
    blob = buf("blob", (rows, B), torch.float64) if want_blob else None
    if (sensitivity or flight) and blob is None:       # the solve's blob, needed by the sensitivity / flight kernels only
        blob = torch.empty((rows, B), dtype=torch.float64, device=dev)
    sens = buf("sensitivity", (B, 16), torch.float64) if sensitivity else None
    if flight:
        fsum, ftraj = buf("flight_summary", (B, len(FLIGHT_ROWS)), torch.float64), buf("flight_traj", (B, 10, nt), torch.float64)
        floc = buf("flight_local", (B, nt - 1, 7), torch.float64)
    o = _opts(nt, max_iter, tol, warm_start, mu_init, scheme, formulation, coarse_nodes, terminal, path, move_penalty)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(L.ascent_solve_batch(params_t.data_ptr(), B, C.byref(o),
                                    guess_t.data_ptr() if guess_t is not None else None,
                                    traj.data_ptr() if traj is not None else None, tf.data_ptr(), status.data_ptr(),
                                    iters.data_ptr(), blob.data_ptr() if blob is not None else None,
                                    dev.index or 0, C.c_void_p(stream), 1))
    if sensitivity:
        g = torch.empty((16, B), dtype=torch.float64, device=dev)
        _lib.check(L.ascent_param_sensitivity(params_t.data_ptr(), B, C.byref(o), blob.data_ptr(), g.data_ptr(),
                                              dev.index or 0, C.c_void_p(stream), 1))
        J = _penalised_objective(params_t, blob, nt - 1, formulation) if move_penalty else blob[21 * (nt - 1)]
        s_ = g.t() * params_t[:, 11:12]
        s_[:, 11] += J
        sens.copy_(torch.where((status == 0)[:, None], s_, torch.full_like(s_, float("nan"))))
    if flight:
        K = nt - 1
        rs = torch.empty((len(FLIGHT_ROWS), B), dtype=torch.float64, device=dev)
        rt = torch.empty((10, nt, B), dtype=torch.float64, device=dev)
        rl = torch.empty((K, 7, B), dtype=torch.float64, device=dev)
        _lib.check(L.ascent_fly_batch(params_t.data_ptr(), B, C.byref(o), blob.data_ptr(), 0, rt.data_ptr(), rl.data_ptr(),
                                      rs.data_ptr(), dev.index or 0, C.c_void_p(stream), 1))
        ok, nan = status == 0, torch.full((), float("nan"), dtype=torch.float64, device=dev)
        fsum.copy_(torch.where(ok[:, None], rs.t(), nan))
        ftraj.copy_(torch.where(ok[:, None, None], rt.permute(2, 0, 1), nan))
        floc.copy_(torch.where(ok[:, None, None], rl.permute(2, 0, 1), nan))
    if sync:
        torch.cuda.synchronize(dev)
    return out


class _FinalTime:
    """torch.autograd.Function of final_time (built on first use: torch is imported lazily)."""
    fn = None

    @classmethod
    def get(cls):
        if cls.fn is None:
            import torch

            class FinalTime(torch.autograd.Function):
                @staticmethod
                def forward(ctx, params_t, kw):
                    out = solve_batch_torch(params_t.detach().contiguous(), sensitivity=True, want_traj=False,
                                            want_blob=kw.get("move_penalty", False), **kw)
                    T = params_t[:, 11].detach()
                    if kw.get("move_penalty", False):       # (the blob's own tf row holds the bits of out["tf"])
                        y = T * _penalised_objective(params_t.detach(), out["blob"], kw.get("nt", 200) - 1, kw.get("formulation", 0))
                    else:
                        y = T * out["tf"]
                    y = torch.where(out["status"] == 0, y, torch.full_like(y, float("nan")))
                    ctx.save_for_backward(out["sensitivity"])
                    return y

                @staticmethod
                def backward(ctx, grad_out):
                    (sens,) = ctx.saved_tensors
                    return grad_out[:, None] * sens, None

            cls.fn = FinalTime
        return cls.fn


def final_time(params_t, **solve_kw):
    """Differentiable optimal final time: (batch,) t_f* in seconds of the NLPs of `params_t` (a float64 CUDA tensor
    (batch, 16), solved by solve_batch_torch with `solve_kw`); backward gives grad_out * d t_f*/dp from the post-optimal
    sensitivity (no extra solve).  With move_penalty=True the value is the penalised objective T_scale J* in seconds and
    the gradient is its own.  NLPs that did not converge give NaN values and NaN gradients."""
    return _FinalTime.get().apply(params_t, dict(solve_kw))


def default_path(batch: int, nt: int = 200, scheme=0, formulation=0, move_penalty: bool = False, terminal=0) -> str:
    """The kernels solve_batch runs for a batch of this size (include/ascent.h: ascent_default_path): a key of _lib.PATHS."""
    o = _opts(nt, 300, 1e-9, 0, 0.0, scheme, formulation, move_penalty=move_penalty, terminal=terminal)
    code = _lib.load().ascent_default_path(int(batch), C.byref(o))
    return {v: k for k, v in _lib.PATHS.items()}[code]


def last_kernel_ms(device: int = 0) -> float:
    """HIP-event time of the most recent solve kernel on `device` (waits for it)."""
    return _lib.load().ascent_last_kernel_ms(device)
