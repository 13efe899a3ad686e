"""The stated fp32 tolerance (BASELINE.json north_star: "state trajectories match ... within a
stated fp32 tolerance"): the HIP path's divergence from the fp64 oracle
under random actions, against the oracle's OWN divergence when its fp32-stored state is
perturbed at fp32 precision (tests/fp32_envelope.py: one fp32 ulp once, or the fp32-stored
fields rounded to fp32 every step).

Random-action flight of this model is chaotic: any difference grows roughly
exponentially with the horizon, so no fixed per-horizon tolerance separates "fp32 round-off,
amplified" from "a small systematic difference". The envelope does: if HIP-vs-oracle stays within
a fixed factor of oracle-vs-perturbed-oracle at every horizon, the divergence is the dynamics'
amplification of fp32-level differences; a systematic defect would leave it early.

Assertion, per frame component c (lat*R .. psi) and horizon t in HORIZONS, over the lanes still
running on both sides (p99 over lanes):
    p99_hip(c, t) <= FACTOR * max(p99_ulp1(c, t), p99_round(c, t)) + (TOL_RAND30[c] if t <= 30 else 0)
(TOL_RAND30, the 30-step frame tolerance, is the floor where the envelope is still below the
fp32 arithmetic's own per-step rounding: t <= 30, and only there). Up to step 30 that floor is
nearly the whole bound, so of these horizons only step 100 tests the physics; the 300 and 1199 rows
are saturated -- both sides are decorrelated there (the envelope's phi p99 is 0.74 rad at 300, 24
lanes are left at 1199) -- and assert nothing about the physics: they are kept as a record. The
check with teeth is tests/test_gpu_trajectory_envelope.py: every step 1 .. 120, every step-kernel
instance, the number format as the only floor. The numbers behind the assertion are written to
$F16_ENVELOPE_JSON when set (profiles/r06_fp32_envelope.json)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from fp32_envelope import run  # noqa: E402
from parity_tools import FRAME_NAMES  # noqa: E402
from test_gpu_parity import TOL_RAND30  # noqa: E402

HORIZONS = (1, 10, 30, 100, 300, 1199)
FACTOR = 3.0
FLOOR_UNTIL = 30


@pytest.mark.parametrize("cfg5", [False, True], ids=["reference_task", "cfg5"])
def test_hip_divergence_within_fp32_envelope(gpu, cfg5):
    """cfg5: BASELINE cfg5's random ICs (up to 1 200 fps, 3 000-30 000 ft) and Gauss-Markov gusts
    on the same lanes; the envelope's `round` variant then also rounds the steady-wind and gust
    states (fp32 columns of the wind kernels)."""
    out = run(n=256, steps=1199, horizons=HORIZONS, variants=("ulp1", "round"), hip=True, cfg5=cfg5)
    table = {}
    worst = {}
    for t in HORIZONS:
        if t not in out["hip"]:
            continue
        row = {"lanes": out["hip"][t]["lanes"]}
        for c, nm in enumerate(FRAME_NAMES[:12]):
            env = max(out["ulp1"][t][nm][1], out["round"][t][nm][1])
            hip = out["hip"][t][nm][1]
            bound = FACTOR * env + (TOL_RAND30[c] if t <= FLOOR_UNTIL else 0.0)
            row[nm] = {"hip_p99": hip, "envelope_p99": env, "bound": bound,
                       "ratio_to_envelope": hip / env if env > 0 else None}
            worst[(t, nm)] = (hip, bound)
        table[t] = row
    path = os.environ.get("F16_ENVELOPE_JSON")
    if path and cfg5:
        path = path.replace(".json", "_cfg5.json")
    if path:
        with open(path, "w") as f:
            json.dump({"test": "tests/test_gpu_fp32_envelope.py", "factor": FACTOR,
                       "floor": dict(zip(FRAME_NAMES[:12], map(float, TOL_RAND30[:12]))), "floor_until_step": FLOOR_UNTIL,
                       "table": {str(t): r for t, r in table.items()},
                       "raw": {v: {str(t): d for t, d in per.items()} for v, per in out.items()}}, f, indent=1)
    for t in HORIZONS:
        assert t in out["hip"], "no lane running on both sides at step %d" % t
    bad = [(k, v) for k, v in worst.items() if not v[0] <= v[1]]
    assert not bad, "HIP-vs-oracle p99 outside %.0fx the fp32 envelope: %s" % (FACTOR, bad[:6])
