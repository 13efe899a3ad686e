"""The fp32 envelope machinery on the CPU (tests/fp32_envelope.py; the GPU comparison is
tests/test_gpu_fp32_envelope.py): the get_state / set_state control leaves the oracle's
trajectory bit-identical over the compared horizon, the perturbed variants are perturbed, and
their divergence grows with the horizon -- the yardstick the HIP path's divergence is held to."""
from __future__ import annotations

import numpy as np
import pytest

import fp32_envelope as fe
from fp32_envelope import F32_FIELDS, one_ulp, run, to_f32_storage

from f16_jsb_amd.abi import F16C_ELE
from test_gpu_parity import TOL_RAND30  # (the module imports without a GPU)


@pytest.mark.parametrize("cfg5", [False, True], ids=["reference_task", "cfg5"])
def test_envelope_control_is_exact_and_perturbations_grow(cfg5):
    out = run(n=64, steps=100, horizons=(1, 10, 30, 100), cfg5=cfg5)
    for t in (1, 10, 30, 100):
        d = out["control"][t]
        assert d["lanes"] == 64
        assert all(d[c][2] == 0.0 for c in d if c != "lanes"), (t, d)
    for v in ("ulp1", "round"):
        h10, h100 = out[v][10]["h_m"][1], out[v][100]["h_m"][1]
        a10, a100 = out[v][10]["alpha"][1], out[v][100]["alpha"][1]
        assert h100 > h10 and a100 > a10 > 0.0, (v, out[v])


def test_state_perturbations_touch_only_fp32_fields():
    from oracle_ref import OracleEnvs
    e = OracleEnvs(8, stack_k=4, seed=5)
    e.reset()
    for _ in range(3):
        e.step(e.sample_actions(99, 0))
    s = e.get_state()
    e.close()
    r = to_f32_storage(s)
    u = one_ulp(s, np.random.default_rng(0))
    others = np.setdiff1d(np.arange(s.shape[1]), F32_FIELDS)
    # fp32 storage: the fp64 fields (ECI position / velocity, Earth angle, episode return) are kept,
    # except the AB3 velocity history, which becomes fp32 deltas from the fp64 velocity
    keep = np.setdiff1d(others, np.r_[6:12])
    np.testing.assert_array_equal(r[:, keep], s[:, keep])
    np.testing.assert_array_equal(r[:, F32_FIELDS], s[:, F32_FIELDS].astype(np.float32).astype(np.float64))
    np.testing.assert_array_equal(u[:, others], s[:, others])
    f = s[:, F32_FIELDS].astype(np.float32)
    moved = u[:, F32_FIELDS].astype(np.float32)
    up, dn = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
    assert np.all((moved == up) | (moved == dn))  # one fp32 ulp either way (through 0 too)


# ------------------------------------------------------------------------------------------
# The dense envelope (fp32_envelope.dense / check): what keeps it honest. The oracle alone passes
# it with perturbations that are not in it; three planted defects are rejected within the first
# steps. If the envelope is ever widened, the defects must still be rejected at these steps.
# ------------------------------------------------------------------------------------------
WORKLOADS = {"reference_task": fe.Workload(), "cfg5": fe.Workload(cfg5=True),
             "ds2": fe.Workload(down_sample=2), "ds1": fe.Workload(down_sample=1),
             "steady_wind": fe.Workload(wind=True),
             "edges": fe.edge_workload(False), "edges_cfg5_wind": fe.edge_workload(True)}
TASKS = ("reference_task", "cfg5")
DT = 1.0 / 120.0
NO_J2 = 0x8  # oracle/f16ref.h: the physics mask bit that drops the J2 gravity term


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_dense_envelope_accepts_the_oracle_alone(name):
    """ulp1 and frame_ulp seeds that are not in the envelope and the one-off fp32 rounding meet
    the assertion at every step, in every group; the get / set round trip stays exactly on the
    reference, and so does the frame-by-frame replay the frame-level variants are made with."""
    w = WORKLOADS[name]
    d = fe.dense(w)
    assert d.E.shape == d.F.shape == (len(d.groups), w.steps, 12)
    assert (d.E[:, -1] > d.E[:, 0]).any() and (d.F > 0).all()
    worst = {}
    held = fe.HELD_OUT_SEEDS
    for what, var, seed in [("ulp1 seed %d" % s, "ulp1", s) for s in held] + [
            ("round1", "round1", None), ("frame_ulp seed %d" % held[0], "frame_ulp", held[0])]:
        frames, done, _ = fe.variant(w, var, seed)
        worst[what] = fe.assert_within(d, frames, done, "%s, %s" % (name, what)).worst
    print("%s: worst held-out ratios %s" % (name, worst))
    frames, done, _ = fe.variant(w, "control")
    # exactly 0 in the envelope's statistic at every step. (Not in every lane-step: set_state
    # recomputes the Earth angle from its cosine / sine, 1e-16 rad = 1e-9 m of longitude, which
    # moves an fp32 rounding of lon*R in 3 of 122 880 lane-steps of the reference task: one ulp,
    # or 1e-8 m where lon*R passes through 0.)
    rep = fe.check(d, frames, done)
    assert np.nanmax(rep.p99) == 0.0 and np.array_equal(fe.running(done), fe.running(d.done))
    alive = fe.running(d.done)
    other = [c for c in range(12) if c != 1]
    assert np.array_equal(frames[alive][:, other], d.frames[alive][:, other])
    lon, ref = frames[alive][:, 1], d.frames[alive][:, 1]
    assert (np.abs(lon - ref) <= np.spacing(np.abs(ref).astype(np.float32)) + 1e-8).all()
    frames, done, _ = fe.variant(w, "frames")
    rep = fe.check(d, frames, done)
    assert np.nanmax(rep.p99) == 0.0 and np.array_equal(fe.running(done), fe.running(d.done))
    assert np.abs(frames - d.frames)[alive].max() <= 1e-8


def _scaled_elevator(s):
    s = s.copy()
    s[:, F16C_ELE] *= 1.0 + 1e-4
    return s


DEFECTS = {  # name: (trajectory keywords, the step by which it must be rejected)
    "dt_1e-5": (dict(dt=DT * (1.0 + 1e-5)), 3),
    "no_J2": (dict(physics_mask=NO_J2), 3),
    "elevator_1e-4": (dict(every_step=_scaled_elevator), 6),
}


@pytest.mark.parametrize("task", TASKS)
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_dense_envelope_rejects_planted_defects(task, defect):
    """A wrong constant, a missing small term and a gain error, planted in one side of an
    oracle-vs-oracle run (no oracle source changes), leave the bound within the first steps."""
    w = WORKLOADS[task]
    kw, by = DEFECTS[defect]
    d = fe.dense(w)
    frames, done, _ = fe.trajectory(w, **kw)
    rep = fe.check(d, frames, done)
    first = rep.first_step_over()
    print("%s, %s: first step over the bound %s, worst ratio over 30 steps %.3g, over all %s" % (
        task, defect, first, np.nanmax(rep.ratio[:, :30]), rep.worst))
    assert first is not None and first <= by, (first, rep.worst)
    if defect == "dt_1e-5":
        assert np.nanmax(rep.ratio[:, :30]) > 1.0
    with pytest.raises(AssertionError):
        fe.assert_within(d, frames, done, defect)


@pytest.mark.parametrize("task", TASKS)
def test_blanket_floor_hid_the_dt_defect(task):
    """What tests/test_gpu_fp32_envelope.py's form let through: the dt (1 + 1e-5) run satisfies
    3 * E + TOL_RAND30 at steps 1, 10 and 30, the horizons where that floor applies."""
    w = WORKLOADS[task]
    d = fe.dense(w)
    frames, done, _ = fe.trajectory(w, dt=DT * (1.0 + 1e-5))
    old = fe.check(d, frames, done, floor=TOL_RAND30[None, None, :12])
    for t in (1, 10, 30):
        assert np.nanmax(old.ratio[:, t - 1]) <= 1.0, (t, np.nanmax(old.ratio[:, t - 1]))
    assert fe.check(d, frames, done).first_step_over() <= 3  # (the same run, the dense bound)
