"""The fp64 oracle against itself: how fast does a perturbation at fp32 storage precision grow
on the reference task under random actions? (BASELINE.json north_star:
"state trajectories match ... within a stated fp32 tolerance".)

TEST INFRASTRUCTURE (runs the CPU oracle only): the envelope the HIP-vs-oracle divergence is
judged against (tests/test_gpu_fp32_envelope.py).

    python tests/fp32_envelope.py [--n 256] [--steps 1199] [--json profiles/r06_fp32_envelope.json]

The workload is tests/parity_report.py's random-action trajectories: OracleEnvs(n, K=4,
seed=5), goals default_rng(0) uniform over [-5000, 5000]^2 x [1000, 4000] m, actions
sample_actions(99, t) (the same Philox stream the HIP path draws), the reference IC
(jsbsim_gym.py:166-170). Runs, every one bit-deterministic:

  ref      the oracle as it runs (the trajectory the HIP path is compared with);
  control  its state passed through get_state / set_state at every step and nothing else
           (set_state recomputes the Earth angle from its cosine / sine): what the mechanism
           of the `round` variant costs by itself;
  round1   the state's fp32-stored fields rounded to fp32 once, after the reset (the HIP
           kernel's storage: f16_device.h keeps the ECI position / velocity and the Earth
           angle in fp64, everything else -- attitude, rates, AB histories as velocity deltas,
           FCS, engine, latch -- in fp32);
  ulp1     the same fields moved by one fp32 ulp once (random sign per field and lane);
  round    the fp32-stored fields rounded to fp32 after EVERY step (fp32 storage, fp64
           arithmetic: the part of the kernel's error that storage alone causes);
  hip      (with --gpu / run(hip=True)) the HIP path, F16Envs with the same seed, goals and
           in-kernel-identical Philox actions: the divergence the envelope is for.

Per variant and horizon: p50 / p99 / max over the lanes still running on both sides of
|variant - ref| per frame component (angles wrapped), plus the lane count. A lane leaves the
comparison at its first done on either side (as parity_report.py).

dense() (below) is the same yardstick at EVERY step 1 .. 120 with the number format as the only
floor, per workload and lane group, and check() the assertion made against it
(tests/test_gpu_trajectory_envelope.py, tests/test_fp32_envelope_cpu.py)."""
from __future__ import annotations

import argparse
import functools
import json
import os
import sys
from typing import NamedTuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from f16_jsb_amd.abi import (F16C_AI, F16C_AIP, F16C_BA, F16C_EP_COUNT, F16C_EP_RET, F16C_GUST,  # noqa: E402
                             F16C_LAST_D, F16C_LX, F16C_Q, F16C_RI, F16C_STEP, F16C_TEF, F16C_VI, F16C_VIH1,
                             F16C_VIH2, F16C_WI, F16C_WID, F16C_WIND, F16L_N)
from parity_tools import ANGLE_COLS, FRAME_NAMES, edge_ics, frame_err  # noqa: E402

HORIZONS = (1, 3, 10, 30, 100, 300, 1199)
VARIANTS = ("control", "round1", "ulp1", "round")
# fields the HIP kernel holds in fp32: attitude, rates and their derivatives, the
# AB2 acceleration history, FCS actuators + PID states, engine, the auxiliary latch
F32_FIELDS = np.r_[F16C_AI:F16C_AI + 3, F16C_AIP:F16C_AIP + 3, F16C_Q:F16C_Q + 4, F16C_WI:F16C_WI + 3,
                   F16C_WID:F16C_WID + 3, F16C_BA:F16C_BA + 3, F16C_TEF:F16C_LX + F16L_N,
                   F16C_WIND:F16C_GUST + 3]  # (cfg5: steady wind and gust, fp32 columns of the wind kernels)


def workload(n):
    rng = np.random.default_rng(0)
    goals = rng.uniform([-5000, -5000, 1000], [5000, 5000, 4000], size=(n, 3)).astype(np.float32)
    return goals


def to_f32_storage(s):
    """The canonical state as the kernel stores it: fp32 fields rounded; the AB3 velocity
    history kept as fp32 deltas from the fp64 velocity (vI - vIh1, vIh1 - vIh2)."""
    s = s.copy()
    s[:, F32_FIELDS] = s[:, F32_FIELDS].astype(np.float32).astype(np.float64)
    vi, h1, h2 = s[:, F16C_VI:F16C_VI + 3], s[:, F16C_VIH1:F16C_VIH1 + 3], s[:, F16C_VIH2:F16C_VIH2 + 3]
    d1 = (vi - h1).astype(np.float32).astype(np.float64)
    d2 = (h1 - h2).astype(np.float32).astype(np.float64)
    s[:, F16C_VIH1:F16C_VIH1 + 3] = vi - d1
    s[:, F16C_VIH2:F16C_VIH2 + 3] = vi - d1 - d2
    return s


def one_ulp(s, rng):
    """Every fp32-stored field moved by one fp32 ulp (random sign)."""
    s = s.copy()
    f = s[:, F32_FIELDS].astype(np.float32)
    sign = rng.choice([-1.0, 1.0], size=f.shape)
    up = np.nextafter(f, np.float32(np.inf))
    dn = np.nextafter(f, np.float32(-np.inf))
    s[:, F32_FIELDS] = np.where(sign > 0, up, dn).astype(np.float64)
    return s


def run(n=256, steps=1199, horizons=HORIZONS, variants=VARIANTS, seed=5, act_seed=99, hip=False, cfg5=False):
    """{variant: {horizon: {"lanes": m, component: [p50, p99, max]}}} -- see the module doc.
    cfg5: BASELINE cfg5's randomised ICs + Gauss-Markov gusts (the same goals)."""
    from oracle_ref import OracleEnvs
    goals = workload(n)
    envs = {"ref": OracleEnvs(n, stack_k=4, seed=seed, cfg5=cfg5)}
    for v in variants:
        envs[v] = OracleEnvs(n, stack_k=4, seed=seed, cfg5=cfg5)
    for e in envs.values():
        e.reset(goals=goals)
    g = None
    if hip:
        import torch
        from f16_jsb_amd.env import F16Envs
        g = F16Envs(n, stack_k=4, seed=seed, obs_layout="window", cfg5=cfg5)
        g.reset(goals=torch.as_tensor(goals))
        variants = tuple(variants) + ("hip",)
    rng = np.random.default_rng(1234)
    if "round1" in envs:
        envs["round1"].set_state(to_f32_storage(envs["round1"].get_state()))
    if "ulp1" in envs:
        envs["ulp1"].set_state(one_ulp(envs["ulp1"].get_state(), rng))
    alive = {v: np.ones(n, bool) for v in variants}
    out = {v: {} for v in variants}
    hz = set(horizons)
    for t in range(1, steps + 1):
        a = envs["ref"].sample_actions(act_seed, t)
        res = {}
        for name, e in envs.items():
            if name in ("control", "round"):
                s = e.get_state()
                e.set_state(to_f32_storage(s) if name == "round" else s)
            o, _, te, tr, *_ = e.step(a)
            res[name] = (o[:, -1], te | tr)
        if g is not None:
            out_g = g.step(g.sample_actions(act_seed, t))
            res["hip"] = (out_g.obs[:, -1].cpu().numpy(),
                          (out_g.terminated.cpu().numpy() != 0) | (out_g.truncated.cpu().numpy() != 0))
        for v in variants:
            alive[v] &= ~(res["ref"][1] | res[v][1])
            if t in hz and alive[v].any():
                err = frame_err(res[v][0][alive[v]], res["ref"][0][alive[v]])
                d = {"lanes": int(alive[v].sum())}
                for c, nm in enumerate(FRAME_NAMES[:12]):
                    col = err[:, c]
                    d[nm] = [float(np.percentile(col, 50)), float(np.percentile(col, 99)), float(col.max())]
                out[v][t] = d
    for e in envs.values():
        e.close()
    if g is not None:
        g.close()
    return out


# ------------------------------------------------------------------------------------------
# The dense envelope: every step 1 .. steps, no blanket floor (tests/test_gpu_trajectory_envelope.py,
# tests/test_fp32_envelope_cpu.py).
#
#   E[g, t, c]  p99 over the lanes of group g still running on both sides of |variant - ref|,
#               the maximum over `round`, four `ulp1` runs with different seeds (one seed is not
#               enough: a held-out ulp1 seed reached 1.34 x a one-seed bound on cfg5), and the two
#               frame-level variants `frame32` and `frame_ulp` (variant(): the kernel rounds at
#               every frame of a step, and normalises its quaternion to 2 ulps, not once a step);
#   F[g, t, c]  FLOOR_ULPS = 4 fp32 spacings at the largest |reference value| of the component over the
#               running lanes of the group: the observation's own number format (phi, theta, psi:
#               at least at 2 pi, a heading just below 2 pi against one just above 0; lat*R,
#               lon*R, h_m: at least as many fp64 spacings at the Earth's radius, 3.7e-9 m -- they are
#               differences of fp64 ECI coordinates of that size, so that is the reference's own
#               resolution: at step 1 of the reference IC lon*R is 5e-13 m of such round-off);
#   assertion   p99_got[g, t, c] <= FACTOR * E[g, t, c] + F[g, t, c] at every step.
#
# Nothing in the bound comes from the path under test. Beyond ~150 steps the envelope reaches the
# variables' ranges, hence 120.
# ------------------------------------------------------------------------------------------
FACTOR = 3.0   # the project's factor over the oracle's own divergence (tests/state_corners.py)
# 2 spacings cover one rounding of the observation on each side. 4, state_corners.floors' count:
# half an ulp of storage on each side plus the few fp32 operations that make a value from
# bit-identical inputs. The first frame needs them: every lane of the reference task starts from
# one and the same state, so at step 1 of down_sample = 1 the envelope of the body rates is a
# single ulp of a rate that is one frame's increment, dt * (a sum of moments) -- two products and
# a sum away from its inputs on the device (q: 6 ulps of 4.7e-10 rad/s at p99).
FLOOR_ULPS = 4.0
ENVELOPE_SEEDS = (1234, 2345, 3456, 4567)   # the four ulp1 runs inside the envelope
FRAME_ULP_SEED = 5678                       # the frame_ulp run inside the envelope
EARTH_RADIUS_M = 6.378e6
HELD_OUT_SEEDS = (9001, 9002)               # ulp1 runs that are not (tests/test_fp32_envelope_cpu.py)
RECORD_STEPS = (1, 3, 10, 30, 60, 100, 120)
EDGE_GROUPS = ("stratosphere", "supersonic", "alpha_beta", "attitude", "crash_floor")


class Workload(NamedTuple):
    """kind "random": goals workload(n), env seed 5, actions sample_actions(99, t), the reference
    IC (cfg5: the cfg5 box and gusts; wind: a steady N/E wind on every lane through the reset IC,
    no gusts). kind "edges": tests/test_gpu_envelope.py's lanes -- parity_tools.edge_ics in five
    groups, goals at 60 km, env seed 23, action seed 31 (cfg5: steady wind and gusts on the same
    states); statistics per group."""
    kind: str = "random"
    cfg5: bool = False
    down_sample: int = 4
    wind: bool = False
    n: int = 1024
    steps: int = 120


def edge_workload(cfg5):
    return Workload("edges", cfg5, n=1280, steps=30)


def setup(w):
    """{"goals", "ic", "env_kw", "act_seed", "groups" (name, lane index array)} of a workload."""
    if w.kind == "edges":
        rng = np.random.default_rng(17)
        ic = edge_ics(w.n, rng)
        if w.cfg5:  # steady wind on the same states (the gust is the model's own draw)
            ic[:, 16:18] = rng.uniform(-30.0, 30.0, (w.n, 2))
        goals = rng.uniform(-5000, 5000, (w.n, 3)).astype(np.float32)
        goals[:, 2] = 60000.0  # no goal capture: the lanes end by crashing or not at all
        q = w.n // 5
        groups = [(nm, np.arange(i * q, (i + 1) * q if i < 4 else w.n)) for i, nm in enumerate(EDGE_GROUPS)]
        return {"goals": goals, "ic": ic, "env_kw": dict(seed=23, cfg5=w.cfg5, down_sample=w.down_sample),
                "act_seed": 31, "groups": groups}
    assert w.kind == "random"
    ic = None
    if w.wind:
        from oracle_ref import default_ic
        ic = np.tile(default_ic(), (w.n, 1))
        ic[:, 16:18] = np.random.default_rng(3).uniform(-30.0, 30.0, (w.n, 2))
    return {"goals": workload(w.n), "ic": ic, "env_kw": dict(seed=5, cfg5=w.cfg5, down_sample=w.down_sample),
            "act_seed": 99, "groups": [("all", np.arange(w.n))]}


def trajectory(w, init=None, every_step=None, physics_mask=0, **env_over):
    """One oracle run of a workload: (frames (steps, n, 12) float64, done (steps, n) bool,
    actions (steps, n, 4) float32). init(state) -> state once after the reset, every_step(state)
    -> state before every step (both through get_state / set_state); physics_mask: the oracle's
    process-global test mask, set around this run's step() calls only; env_over: OracleEnvs
    keywords over the workload's (dt=...)."""
    from oracle_ref import OracleEnvs, lib
    su = setup(w)
    e = OracleEnvs(w.n, stack_k=1, **dict(su["env_kw"], **env_over))
    frames = np.empty((w.steps, w.n, 12))
    done = np.empty((w.steps, w.n), bool)
    acts = np.empty((w.steps, w.n, 4), np.float32)
    try:
        e.reset(goals=su["goals"], ic=su["ic"])
        if init is not None:
            e.set_state(init(e.get_state()))
        for t in range(1, w.steps + 1):
            acts[t - 1] = e.sample_actions(su["act_seed"], t)
            if every_step is not None:
                e.set_state(every_step(e.get_state()))
            if physics_mask:
                lib().f16ref_set_physics_mask(physics_mask)
            try:
                o, _, te, tr, *_ = e.step(acts[t - 1])
            finally:
                if physics_mask:
                    lib().f16ref_set_physics_mask(0)
            frames[t - 1] = o[:, -1, :12]
            done[t - 1] = te | tr
    finally:
        e.close()
    return frames, done, acts


def fp32_increments(prev, new, dt):
    """The device's integration of its fp64 fields, one frame: the ECI velocity and position stay
    in fp64 but gain fp32 increments (f16_device.h frame(): vI += (double)dv, rI += dt vI +
    (double)corr), which rounding the stored state cannot model: vI and rI are not fp32 fields."""
    s = new.copy()
    v0, r0 = prev[:, F16C_VI:F16C_VI + 3], prev[:, F16C_RI:F16C_RI + 3]
    dv = (new[:, F16C_VI:F16C_VI + 3] - v0).astype(np.float32).astype(np.float64)
    corr = (new[:, F16C_RI:F16C_RI + 3] - r0 - dt * v0).astype(np.float32).astype(np.float64)
    s[:, F16C_VI:F16C_VI + 3] = v0 + dv
    s[:, F16C_RI:F16C_RI + 3] = r0 + dt * v0 + corr
    return s


def quat_ulp(s, rng):
    """The attitude quaternion moved by one fp32 ulp, random sign per component and lane."""
    s = s.copy()
    q = s[:, F16C_Q:F16C_Q + 4].astype(np.float32)
    sign = rng.choice([-1.0, 1.0], size=q.shape)
    s[:, F16C_Q:F16C_Q + 4] = np.where(sign > 0, np.nextafter(q, np.float32(np.inf)),
                                       np.nextafter(q, np.float32(-np.inf))).astype(np.float64)
    return s


# env-layer bookkeeping of the canonical state: kept from the production oracle in trajectory_frames
_ENV_LAYER = [F16C_STEP, F16C_EP_RET, F16C_EP_COUNT, F16C_LAST_D]


def trajectory_frames(w, after_frame=None):
    """trajectory() with a hook after every FRAME of every step: after_frame(prev, new, dt) ->
    state. A production step is its down_sample frames replayed one by one, bit for bit
    (tests/test_state_corners_cpu.py), so: the production oracle makes each step's start, its gust
    draw (cfg5: one per step, held over the step's frames, as state_corners.replay) and its
    bookkeeping; a down_sample = 1 oracle without gust draws replays the frames from that start
    with the hook between them, makes the observed frame, and its end state goes back into the
    production oracle. done: the production step's flags or any replayed frame's."""
    from oracle_ref import OracleEnvs
    su = setup(w)
    kw = su["env_kw"]
    dt = 1.0 / 120.0
    prod = OracleEnvs(w.n, stack_k=1, **kw)
    one = OracleEnvs(w.n, stack_k=1, seed=kw["seed"], down_sample=1)
    frames = np.empty((w.steps, w.n, 12))
    done = np.zeros((w.steps, w.n), bool)
    try:
        prod.reset(goals=su["goals"], ic=su["ic"])
        one.reset(goals=su["goals"])
        for t in range(1, w.steps + 1):
            a = prod.sample_actions(su["act_seed"], t)
            cur = prod.get_state()
            _, _, te, tr, *_ = prod.step(a)
            post = prod.get_state()
            done[t - 1] = te | tr
            cur[:, F16C_GUST:F16C_GUST + 3] = post[:, F16C_GUST:F16C_GUST + 3]
            for _ in range(w.down_sample):
                one.set_state(cur)
                o, _, te, tr, *_ = one.step(a)
                done[t - 1] |= te | tr
                new = one.get_state()
                cur = new if after_frame is None else after_frame(cur, new, dt)
            frames[t - 1] = o[:, -1, :12]
            keep = ~done[t - 1]   # (a finished lane has left the comparison: the production reset stands)
            cur[:, _ENV_LAYER] = post[:, _ENV_LAYER]
            post[keep] = cur[keep]
            prod.set_state(post)
    finally:
        prod.close()
        one.close()
    return frames, done


def variant(w, name, seed=None):
    """trajectory() of one of the module doc's variants (ulp1: default_rng(seed)), or
      frame32  the device's number formats at every FRAME: fp32 increments into the fp64 velocity
               and position (fp32_increments), then the fp32-stored fields rounded. The kernel
               rounds every field at every frame of a step -- its arithmetic is fp32 -- where
               `round` rounds once per step: after one down_sample = 4 step of the edge lanes the
               kernel's quaternion is 2 fp32 ulps (p99) from the oracle's, `round`'s 0.3;
      frame_ulp  frame32, and the quaternion moved by one fp32 ulp (random sign, default_rng(seed))
               at every frame: its update is a chain of fp32 operations ending in a v_rsq
               normalisation that leaves |q| = 1 +- 4 u = 2 fp32 ulps by f16_device.h's own count
               (state_corners.floors), which no rounding of a stored value models. Attitude error
               is sideslip error at once: beta is the one component without a format floor of
               its own size (psi, phi and theta have 2 ulps at 2 pi)."""
    if name == "frame32":
        return trajectory_frames(w, lambda prev, new, dt: to_f32_storage(fp32_increments(prev, new, dt))) + (None,)
    if name == "frame_ulp":
        rng = np.random.default_rng(seed)
        return trajectory_frames(w, lambda prev, new, dt: quat_ulp(
            to_f32_storage(fp32_increments(prev, new, dt)), rng)) + (None,)
    if name == "frames":   # (no hook: must reproduce the reference run)
        return trajectory_frames(w) + (None,)
    if name == "control":
        return trajectory(w, every_step=lambda s: s)
    if name == "round":
        return trajectory(w, every_step=to_f32_storage)
    if name == "round1":
        return trajectory(w, init=to_f32_storage)
    assert name == "ulp1"
    return trajectory(w, init=lambda s: one_ulp(s, np.random.default_rng(seed)))


def running(ref_done, got_done=None):
    """(steps, n) lanes still running: a lane leaves at its first done (on either side)."""
    d = ref_done if got_done is None else ref_done | got_done
    return ~np.logical_or.accumulate(d, axis=0)


def p99_by_group(groups, frames, done, ref_frames, ref_done):
    """(p99 (G, steps, 12), lanes (G, steps), worst_lane (G, steps, 12)) of |frames - ref_frames|
    over the lanes of each group running on both sides; NaN / -1 where a group has none left."""
    err = frame_err(frames, ref_frames)
    alive = running(ref_done, done)
    steps = err.shape[0]
    p99 = np.full((len(groups), steps, 12), np.nan)
    lanes = np.zeros((len(groups), steps), int)
    worst = np.full((len(groups), steps, 12), -1)
    for g, (_, idx) in enumerate(groups):
        for t in range(steps):
            sel = idx[alive[t, idx]]
            lanes[g, t] = len(sel)
            if len(sel):
                p99[g, t] = np.percentile(err[t, sel], 99, axis=0)
                worst[g, t] = sel[np.argmax(err[t, sel], axis=0)]
    return p99, lanes, worst


def format_floor(groups, ref_frames, ref_done):
    """F (G, steps, 12): FLOOR_ULPS fp32 spacings at the component's largest reference magnitude
    over the running lanes of the group (the angles: at least at 2 pi; the positions: at least as many
    fp64 spacings at the Earth's radius)."""
    alive = running(ref_done)
    steps = ref_frames.shape[0]
    m = np.zeros((len(groups), steps, 12))
    for g, (_, idx) in enumerate(groups):
        for t in range(steps):
            sel = idx[alive[t, idx]]
            if len(sel):
                m[g, t] = np.abs(ref_frames[t, sel]).max(axis=0)
    m[..., list(ANGLE_COLS)] = np.maximum(m[..., list(ANGLE_COLS)], 2 * np.pi)
    F = FLOOR_ULPS * np.spacing(m.astype(np.float32)).astype(np.float64)
    F[..., :3] = np.maximum(F[..., :3], FLOOR_ULPS * np.spacing(EARTH_RADIUS_M))
    return F


class Dense(NamedTuple):
    workload: Workload
    groups: list      # [(name, lane indices)]
    frames: np.ndarray   # (steps, n, 12) the reference trajectory
    done: np.ndarray     # (steps, n)
    actions: np.ndarray  # (steps, n, 4) the actions it took
    E: np.ndarray        # (G, steps, 12)
    F: np.ndarray        # (G, steps, 12)


@functools.lru_cache(maxsize=None)
def dense(w=Workload()):
    """The reference trajectory, envelope and format floor of a workload at every step (oracle
    only; cached per workload and read-only, so that several GPU cases share one oracle run)."""
    groups = setup(w)["groups"]
    frames, done, acts = trajectory(w)
    E = np.zeros((len(groups), w.steps, 12))
    for name, seed in [("round", None), ("frame32", None), ("frame_ulp", FRAME_ULP_SEED)] + \
            [("ulp1", s) for s in ENVELOPE_SEEDS]:
        vf, vd, _ = variant(w, name, seed)
        E = np.fmax(E, p99_by_group(groups, vf, vd, frames, done)[0])
    F = format_floor(groups, frames, done)
    for a in (frames, done, acts, E, F):
        a.setflags(write=False)
    return Dense(w, groups, frames, done, acts, E, F)


class Report(NamedTuple):
    ratio: np.ndarray   # (G, steps, 12) p99 / bound, NaN where no lane is left
    p99: np.ndarray
    lanes: np.ndarray   # (G, steps)
    worst_lane: np.ndarray
    worst: tuple        # (ratio, group name, t, component name, lane) of the largest ratio

    def first_step_over(self):
        """The first step (1-based) at which some component of some group is over its bound."""
        over = np.flatnonzero(np.nan_to_num(self.ratio).max(axis=(0, 2)) > 1.0)
        return int(over[0]) + 1 if len(over) else None


def check(d, frames, done, factor=FACTOR, floor=None):
    """The assertion's arithmetic, written once: p99_got <= factor * E + F per group, step and
    component. Returns the Report; raises nothing (assert_within does). floor: instead of F."""
    p99, lanes, worst_lane = p99_by_group(d.groups, frames, done, d.frames, d.done)
    bound = factor * d.E + (d.F if floor is None else floor)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(np.isnan(p99), np.nan, np.where(p99 == 0.0, 0.0, p99 / bound))
    g, t, c = np.unravel_index(np.nanargmax(ratio), ratio.shape)
    worst = (float(ratio[g, t, c]), d.groups[g][0], int(t) + 1, FRAME_NAMES[c], int(worst_lane[g, t, c]))
    return Report(ratio, p99, lanes, worst_lane, worst)


def assert_within(d, frames, done, what):
    """check() as an assertion. Returns the Report."""
    rep = check(d, frames, done)
    bad = np.argwhere(np.nan_to_num(rep.ratio) > 1.0)
    if len(bad):
        g, t, c = bad[np.argsort(bad[:, 1], kind="stable")][0]
        raise AssertionError(
            "%s: p99 over %d lanes outside %.0f x envelope + floor first at (group %s, t %d, %s): %.3e > %.0f * %.3e "
            "+ %.3e, largest on lane %d; %d (group, step, component) entries over; worst ratio %.3g at "
            "(group %s, t %d, %s, lane %d)" % (
                (what, rep.lanes[g, t], FACTOR, d.groups[g][0], t + 1, FRAME_NAMES[c], rep.p99[g, t, c], FACTOR,
                 d.E[g, t, c], d.F[g, t, c], rep.worst_lane[g, t, c], len(bad)) + rep.worst))
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1199)
    ap.add_argument("--json", default=None)
    ap.add_argument("--gpu", action="store_true", help="also the HIP path on cuda:0 (the GPU box)")
    ap.add_argument("--cfg5", action="store_true", help="BASELINE cfg5: random ICs + gusts")
    args = ap.parse_args()
    out = run(args.n, args.steps, hip=args.gpu, cfg5=args.cfg5)
    for v, per in out.items():
        for t, d in per.items():
            print("%-7s t=%-5d lanes=%-4d h_m p99 %.3e max %.3e | alpha p99 %.3e | phi p99 %.3e | lat*R p99 %.3e"
                  % (v, t, d["lanes"], d["h_m"][1], d["h_m"][2], d["alpha"][1], d["phi"][1], d["lat*R"][1]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"workload": "tests/fp32_envelope.py: %d lanes, OracleEnvs(K=4, seed=5), goals default_rng(0), "
                                   "actions sample_actions(99, t), the reference IC" % args.n,
                       "stats": "per frame component [p50, p99, max] of |variant - ref| over lanes running on both sides",
                       "variants": {"control": "get_state / set_state every step, nothing else",
                                    "hip": "the HIP path (F16Envs, windowed layout) against the same oracle run",
                                    "round1": "fp32-stored fields rounded to fp32 once after the reset",
                                    "ulp1": "fp32-stored fields moved by one fp32 ulp once after the reset",
                                    "round": "fp32-stored fields rounded to fp32 after every step"},
                       "envelope": {v: {str(t): d for t, d in per.items()} for v, per in out.items()}}, f, indent=1)


if __name__ == "__main__":
    main()
