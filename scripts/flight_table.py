"""The flight-verification table of DESIGN.md section 11, measured on the device: nominal Apollo 11 parameters solved by the
library with every scheme on several grids and with the three terminal modes, each solution flown by ascent_fly_batch.
Prints markdown rows; --out FILE writes the numbers as JSON."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = {0: "backward Euler", 1: "trapezoid", 2: "Hermite-Simpson"}


def main():
    from lunar_module_ascent_trajectory_optimiser_amd import AscentParams, solve_batch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    cases = [(0, 200, 0), (0, 400, 0), (1, 200, 0), (1, 400, 0), (2, 50, 0), (2, 100, 0), (2, 200, 0), (2, 2000, 0),
             (0, 200, 1), (1, 200, 1), (2, 200, 1), (0, 200, 2), (1, 200, 2), (2, 200, 2)]
    rows = []
    print("| scheme | terminal | N | t_f (s) | miss (m, m/s) | flown orbit peri / apo (m) | NLP's own (m) | max local error (m) at step | m |")
    print("|---|---|---|---|---|---|---|---|---|")
    for scheme, nt, term in cases:
        r = solve_batch(AscentParams(), nt, tol=1e-10 if scheme == 2 else 1e-9, max_iter=500, scheme=scheme, terminal=term, flight=True)
        f = r.flight
        row = dict(scheme=scheme, nt=nt, terminal=term, status=int(r.status[0]), final_time=float(r.final_time()[0]),
                   **{k: float(getattr(f, k)[0]) for k in ("miss_position", "miss_velocity", "flown_periapsis_alt", "flown_apoapsis_alt",
                                                           "nlp_periapsis_alt", "nlp_apoapsis_alt", "max_local_position_error",
                                                           "max_local_velocity_error", "max_local_step", "substeps")})
        rows.append(row)
        print(f"| {NAMES[scheme]} | {term} | {nt} | {row['final_time']:.4f} | {row['miss_position']:.4g}, {row['miss_velocity']:.3g} | "
              f"{row['flown_periapsis_alt']:.0f} / {row['flown_apoapsis_alt']:.0f} | {row['nlp_periapsis_alt']:.0f} / {row['nlp_apoapsis_alt']:.0f} | "
              f"{row['max_local_position_error']:.3g} at {int(row['max_local_step'])} | {int(row['substeps'])} |", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
