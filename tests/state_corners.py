"""State parity: every carried field of the canonical state against the fp64 oracle.

TEST INFRASTRUCTURE (runs the CPU oracle only). The physics tests compare the HIP step with the
oracle through the 12 observed quantities of the newest frame; the other carried fields
(actuators, PID states, N2 / AUG, the Adams-Bashforth histories, the auxiliary latch) reach an
observation only after they have been integrated. This module makes states that sit on the
corners of the FCS / engine code whose device form departs from the oracle's (f16_device.h:
kin_tef, kin2, the wave-wide TEF skip, the impact-pressure switches, pidf, seekf, the AUG
transitions, the LEF selects), and compares whole states field by field:

  corner_states   planted states, their actions and the corner names of every lane;
  replay          the oracle's state before every FRAME of a production step (one down_sample=4
                  step is four down_sample=1 steps bit for bit, tests/test_state_corners_cpu.py);
  guarded         lanes whose switch inputs come within a relative 1e-3 of a threshold at some
                  frame: a different branch there is a legitimate fp32 outcome, so their values
                  are not compared (flags and integer bookkeeping still are);
  envelope        the oracle's own divergence per field when its fp32-stored state moves by one
                  fp32 ulp (fp32_envelope.one_ulp, exact zeros kept);
  check_state     err <= FACTOR * envelope[field] + floor[field] per unguarded lane.

The bound is never calibrated from the HIP output: FACTOR is test_gpu_fp32_envelope.py's, the
floors are derived below from the number formats and the operations involved.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from f16_jsb_amd.abi import (F16_IC_CMD_THR, F16_IC_H_SL_FT, F16_IC_N, F16_IC_P_RPS, F16_IC_PHI_RAD,  # noqa: E402
                             F16_IC_PSI_RAD, F16_IC_THETA_RAD, F16_IC_U_FPS, F16_IC_V_FPS, F16_IC_W_FPS,
                             F16C_AI, F16C_AIL, F16C_AIP, F16C_AUG, F16C_BA, F16C_CMD, F16C_ELE, F16C_EP_COUNT,
                             F16C_EP_RET, F16C_EPA_C, F16C_EPA_S, F16C_GOAL, F16C_GUST, F16C_LAST_D, F16C_LEF,
                             F16C_LX, F16C_N, F16C_N1, F16C_N2, F16C_PID_P_I, F16C_PID_P_P, F16C_PID_R_I,
                             F16C_PID_R_P, F16C_PID_Y_I, F16C_PID_Y_P, F16C_Q, F16C_RI, F16C_RUD, F16C_SB,
                             F16C_STEP, F16C_TEF, F16C_VI, F16C_VIH1, F16C_VIH2, F16C_WI, F16C_WID, F16C_WIND,
                             F16L_ALPHA, F16L_BETA, F16L_MACH, F16L_NPY, F16L_NPZ, F16L_P_AERO, F16L_Q_AERO,
                             F16L_R_AERO, F16L_VC_KTS, F16L_VG_FPS)
from fp32_envelope import F32_FIELDS, to_f32_storage  # noqa: E402

DT = 1.0 / 120.0
EPS32 = float(np.finfo(np.float32).eps)
RAD2DEG = 180.0 / np.pi
FACTOR = 3.0  # tests/test_gpu_fp32_envelope.py's factor over the oracle's own envelope
GUARD_REL = 1e-3
GUARD_CAP = 0.02
GOAL_GAIN = 1e-2

# one frame's travel of each FGKinematic (detent span / transition time * dt, f16.xml)
TEF_STEP = DT / 3.0
LIM = {F16C_AIL: DT * 2.0 / 0.3, F16C_ELE: DT * 2.0 / 0.3, F16C_RUD: DT * 2.0 / 0.4, F16C_LEF: DT * 2.0 / 3.0,
       F16C_SB: DT * 60.0}
# the TEF detents as the device's fp32 constants (0.349f * 2.864789f, -0.0349f * 2.864789f)
TEF_POS = float(np.float32(0.349) * np.float32(2.864789))
TEF_NEG = float(np.float32(-0.0349) * np.float32(2.864789))
A1, A2, A3 = 0.0873, 0.2618, 53.0 / RAD2DEG  # latch-alpha switches: LEF, LEF, speedbrake
VC_SWITCHES = (250.0, 20.0, 10.0, 5.0)
LX = F16C_LX

NAMES = {}
for _nm, _c, _w in (("RI", F16C_RI, 3), ("VI", F16C_VI, 3), ("VIH1", F16C_VIH1, 3), ("VIH2", F16C_VIH2, 3),
                    ("AI", F16C_AI, 3), ("AIP", F16C_AIP, 3), ("Q", F16C_Q, 4), ("WI", F16C_WI, 3),
                    ("WID", F16C_WID, 3), ("BA", F16C_BA, 3), ("CMD", F16C_CMD, 4), ("GOAL", F16C_GOAL, 3),
                    ("WIND", F16C_WIND, 3), ("GUST", F16C_GUST, 3)):
    for _j in range(_w):
        NAMES[_c + _j] = "%s[%d]" % (_nm, _j)
for _nm, _c in (("EPA_C", F16C_EPA_C), ("EPA_S", F16C_EPA_S), ("TEF", F16C_TEF), ("AIL", F16C_AIL),
                ("ELE", F16C_ELE), ("RUD", F16C_RUD), ("LEF", F16C_LEF), ("SB", F16C_SB),
                ("PID_R_I", F16C_PID_R_I), ("PID_R_P", F16C_PID_R_P), ("PID_P_I", F16C_PID_P_I),
                ("PID_P_P", F16C_PID_P_P), ("PID_Y_I", F16C_PID_Y_I), ("PID_Y_P", F16C_PID_Y_P), ("N1", F16C_N1),
                ("N2", F16C_N2), ("AUG", F16C_AUG), ("LAST_D", F16C_LAST_D), ("STEP", F16C_STEP),
                ("EP_RET", F16C_EP_RET), ("EP_COUNT", F16C_EP_COUNT)):
    NAMES[_c] = _nm
for _nm, _l in (("ALPHA", F16L_ALPHA), ("BETA", F16L_BETA), ("MACH", F16L_MACH), ("VC_KTS", F16L_VC_KTS),
                ("VG_FPS", F16L_VG_FPS), ("P_AERO", F16L_P_AERO), ("Q_AERO", F16L_Q_AERO), ("R_AERO", F16L_R_AERO),
                ("NPY", F16L_NPY), ("NPZ", F16L_NPZ)):
    NAMES[LX + _l] = "LX_" + _nm

# compared exactly, on every lane (guarded ones too)
EXACT = [F16C_AUG, F16C_STEP, F16C_EP_COUNT] + list(range(F16C_GOAL, F16C_GOAL + 3)) + \
    list(range(F16C_WIND, F16C_WIND + 3))
# not carried by the device (f16_device.h column map): FGTurbine's N1, the g-load PID's previous
# input (kd = 0), the body force's x component, the command properties. get_state reports 0.
NOT_CARRIED = [F16C_N1, F16C_PID_P_P, F16C_BA] + list(range(F16C_CMD, F16C_CMD + 4))
# latch entries the device recomputes from the state at load instead of keeping what set_state
# gave it (latch_from_state; tests/test_gpu_state.py): never planted
RECOMPUTED = [LX + F16L_P_AERO, LX + F16L_Q_AERO, LX + F16L_R_AERO, LX + F16L_VG_FPS]
VALUE = [c for c in range(F16C_N) if c not in EXACT and c not in NOT_CARRIED]

# Report groups (DESIGN.md 2 quotes the worst ratio of each)
FIELD_GROUPS = {
    "actuators": [F16C_TEF, F16C_AIL, F16C_ELE, F16C_RUD, F16C_LEF, F16C_SB],
    "pid": [F16C_PID_R_I, F16C_PID_R_P, F16C_PID_P_I, F16C_PID_Y_I, F16C_PID_Y_P],
    "engine": [F16C_N2],
    "ab_history": list(range(F16C_VIH1, F16C_AIP + 3)) + list(range(F16C_WID, F16C_WID + 3)),
    "latch": list(range(LX, LX + 10)),
    "propagated": list(range(F16C_RI, F16C_VI + 3)) + list(range(F16C_Q, F16C_WI + 3)) + [F16C_EPA_C, F16C_EPA_S],
    "body_accel": [F16C_BA + 1, F16C_BA + 2],
    "env_layer": [F16C_LAST_D, F16C_EP_RET],
    "gust": list(range(F16C_GUST, F16C_GUST + 3)),
}

# floor[field] = 4 fp32 ulps at max(|ref|, SCALE[field]), SCALE = the field's range. Why 4: half
# an ulp of fp32 storage on each side of the few fp32 operations that make the field from planted
# (bit-identical) inputs -- kin2 is a clamp, a subtraction and an addition, pidf two products and
# two sums, seekf a product, a sum and a min / max -- plus f16_device.h's documented "up to 2
# fp32 ulps short" where kin2 does not restate FGKinematic's eq_roundoff.
SCALE = np.ones(F16C_N)
SCALE[F16C_SB] = 60.0    # degrees
SCALE[F16C_N2] = 100.0   # per cent
SCALE[F16C_AI:F16C_AIP + 3] = 32.0   # ft/s^2: one g
SCALE[F16C_BA:F16C_BA + 3] = 32.0
# fp64 on the device with fp32 increments (f16_device.h frame(): rI += dt vI + (double)corr,
# vI += (double)dv): the rounding is that of the per-frame increment, not of the value, so these
# floors are 4 fp32 ulps of the increment's range PER FRAME: dv = dt (1.5 a - 0.5 ap) < 4 ft/s
# up to 15 g; corr = dt/12 (16 dv1 + 5 dv2) < 1 ft. The velocity history is stored as the fp32
# deltas vI - vIh1 (one dv) and vI - vIh2 (two).
INCR = {}
for _j in range(3):
    INCR[F16C_RI + _j] = 1.0
    INCR[F16C_VI + _j] = 4.0
    SCALE[F16C_VIH1 + _j] = 4.0
    SCALE[F16C_VIH2 + _j] = 8.0
SCALE[LX + F16L_VG_FPS] = 1000.0  # ft/s: |v|^2 - (v.r)^2 of fp32 velocities of that size
# the Earth angle is fp64 on both sides (epa += w dt) and exported as cos / sin: fp64 round-off
EPA_FLOOR = 1e-12
MACH_ULPS = 13.0  # (floors(): the latch Mach's operation count)


def ulp32(x):
    """The fp32 ulp at |x| (x >= the smallest normal)."""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), float(np.finfo(np.float32).tiny))
    return np.exp2(np.floor(np.log2(x)) - 23.0)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def to_device_storage(s):
    """The canonical state as the device keeps it: fp32_envelope.to_f32_storage, with the older
    velocity history as the fp32 delta the device stores (dv2 = vIh2 - vI, f16_set_state_kernel),
    so that a device set_state / get_state returns these values bit for bit."""
    s = to_f32_storage(s)
    vi = s[:, F16C_VI:F16C_VI + 3]
    s[:, F16C_VIH2:F16C_VIH2 + 3] = vi + _f32(s[:, F16C_VIH2:F16C_VIH2 + 3] - vi)
    return s


def device_roundtrip(s):
    """numpy model of f16_set_state_kernel -> f16_get_state_kernel for the fields the device
    keeps (the recomputed latch entries, the vc encoding and the Earth angle aside): what
    get_state must return for a planted state."""
    o = s.copy()
    o[:, F32_FIELDS] = _f32(s[:, F32_FIELDS])
    vi = s[:, F16C_VI:F16C_VI + 3]
    o[:, F16C_VIH1:F16C_VIH1 + 3] = vi + _f32(s[:, F16C_VIH1:F16C_VIH1 + 3] - vi)
    o[:, F16C_VIH2:F16C_VIH2 + 3] = vi + _f32(s[:, F16C_VIH2:F16C_VIH2 + 3] - vi)
    o[:, F16C_LAST_D] = _f32(s[:, F16C_LAST_D])
    o[:, NOT_CARRIED] = 0.0
    return o


def one_ulp(s, rng):
    """fp32_envelope.one_ulp with this change: a field that is exactly 0 stays 0 (a denormal TEF
    would change its FGKinematic segment, which no fp32 rounding of a stored 0 can do)."""
    s = s.copy()
    f = s[:, F32_FIELDS].astype(np.float32)
    sign = rng.choice([-1.0, 1.0], size=f.shape)
    up = np.nextafter(f, np.float32(np.inf))
    dn = np.nextafter(f, np.float32(-np.inf))
    s[:, F32_FIELDS] = np.where(f == 0, f, np.where(sign > 0, up, dn)).astype(np.float64)
    return s


# ------------------------------------------------------------------------------------------
# planted states
# ------------------------------------------------------------------------------------------
# (the last one only in the waves that sit on their detent: the Mach > 0.9 target)
TEF_STARTS = ("-0.1", "-0.05", "0", "within", "beyond", "0.5", "+detent", "1.0", "-detent")
TEF_START_VALUES = (-0.1, -0.05, 0.0, 0.72 * TEF_STEP, 1.62 * TEF_STEP, 0.5, TEF_POS, 1.0, TEF_NEG)
TEF_TARGETS = ("vc<250", "mach>0.9", "neither")
ACT_MODES = ("far", "within", "on", "clamp-", "clamp+")
SB_STARTS = (0.0, 0.6 * DT * 60.0, 30.0, 60.0)
VC_LOW = (3.0, 7.0, 15.0, 25.0, 200.0)   # every integrate trigger on and off, below the flap switch
VC_HIGH = (260.0, 400.0)
ALPHAS = (-0.05, 0.02, A1 * 0.99, A1 * 1.01, A2 * 0.99, A2 * 1.01, A3 * 0.99, A3 * 1.01, 1.05)
PID_I = {F16C_PID_R_I: (0.0, 0.01, -0.02, 1.5, -1.5), F16C_PID_P_I: (0.0, 0.05, -0.05, 2.0, -2.0),
         F16C_PID_Y_I: (0.0, 0.01, -0.01, 1.5, -1.5)}
THROTTLES = (0.05, 0.3, 0.45, 0.49, 0.51, 0.6, 0.8, 1.0)
N2_MODES = ("above", "below", "within", "on", "96.5", "99", "100")
WAVE_KINDS = ("skip", "none", "mixed")
SKIP_WAVES, NONE_WAVES = range(0, 6), range(6, 12)
FAR_GOAL = (30000.0, 30000.0, 3000.0)  # m: 42 km from every lane, out of reach


def _ics(n, rng):
    ic = np.zeros((n, F16_IC_N))
    ic[:, F16_IC_H_SL_FT] = rng.uniform(2000.0, 50000.0, n)
    ic[:, F16_IC_U_FPS] = rng.uniform(200.0, 2000.0, n)
    ic[:, F16_IC_V_FPS] = rng.uniform(-30.0, 30.0, n)
    ic[:, F16_IC_W_FPS] = rng.uniform(-40.0, 60.0, n)
    ic[:, F16_IC_PHI_RAD] = rng.uniform(-0.6, 0.6, n)
    ic[:, F16_IC_THETA_RAD] = rng.uniform(-0.3, 0.3, n)
    ic[:, F16_IC_PSI_RAD] = rng.uniform(0.0, 2 * np.pi, n)
    ic[:, F16_IC_P_RPS:F16_IC_P_RPS + 3] = rng.uniform(-0.2, 0.2, (n, 3))
    ic[:, F16_IC_CMD_THR] = rng.uniform(0.2, 1.0, n)
    return ic


def far_goals(n):
    return np.tile(np.float32(FAR_GOAL), (n, 1))


def _one_frame(state, actions):
    """The oracle's state one frame after `state` (steady wind and gust held, no gust draw)."""
    from oracle_ref import OracleEnvs
    e = OracleEnvs(len(state), stack_k=1, down_sample=1)
    e.reset(goals=far_goals(len(state)))
    e.set_state(state)
    _, _, te, tr, *_ = e.step(actions)
    assert not (te | tr).any()
    out = e.get_state()
    e.close()
    return out


def _targets(s, actions):
    """The aileron / elevator / rudder commands of the first frame, from the oracle itself: the
    command does not depend on the actuator's position, and a traverse that starts within one
    frame's travel lands exactly on it. 80 start values 0.025 apart (< every frame's travel)."""
    n = len(s)
    cols = [F16C_AIL, F16C_ELE, F16C_RUD]
    tgt = np.full((n, 3), np.nan)
    for g in np.linspace(-1.0, 1.0, 81):
        t = s.copy()
        t[:, cols] = g
        out = _one_frame(to_device_storage(t), actions)[:, cols]
        for j, c in enumerate(cols):
            hit = np.abs(out[:, j] - g) < LIM[c] * (1.0 - 1e-6)
            tgt[hit, j] = out[hit, j]
    assert np.isfinite(tgt).all()
    return tgt


def corner_states(n, rng, cfg5=False, seed=7):
    """(state, actions, groups): n planted canonical states at device storage precision, the
    (n, 4) float32 actions that go with them, and per corner family an int array naming each
    lane's corner (index into the tuple of the same name above; see describe())."""
    from oracle_ref import OracleEnvs
    assert n >= 64 * (max(NONE_WAVES) + 4)
    e = OracleEnvs(n, stack_k=1, seed=seed, cfg5=cfg5)
    e.reset(goals=far_goals(n), ic=_ics(n, rng))
    for t in range(1, 4):
        _, _, te, tr, *_ = e.step(e.sample_actions(seed + 4, t))
        assert not (te | tr).any()
    s = e.get_state()
    e.close()
    g = {}
    lane = np.arange(n)
    wave = lane // 64

    # actions: stick and pedals anywhere, some centred; throttle on both sides of the augmentor
    act = rng.uniform(-1.0, 1.0, (n, 4))
    act[rng.random(n) < 0.15, 0] = 0.0
    act[rng.random(n) < 0.15, 2] = 0.0
    g["throttle"] = rng.integers(0, len(THROTTLES), n)
    act[:, 3] = np.take(THROTTLES, g["throttle"])
    act = act.astype(np.float32)
    g["aug_prev"] = rng.integers(0, 2, n)
    s[:, F16C_AUG] = g["aug_prev"]

    # latch: the TEF target class picks vc and Mach; alpha, n-pilot independent
    g["tef_target"] = rng.integers(0, 3, n)
    low = g["tef_target"] == 0
    vc = np.where(low, np.take(VC_LOW, rng.integers(0, len(VC_LOW), n)),
                  np.take(VC_HIGH, rng.integers(0, len(VC_HIGH), n)))
    mach = np.where(g["tef_target"] == 1, np.take((0.91, 0.95, 1.3), rng.integers(0, 3, n)),
                    np.take((0.3, 0.6, 0.85, 0.89), rng.integers(0, 4, n)))
    hi_any = low & (rng.random(n) < 0.4)   # (below 250 kts the flap switch ignores Mach)
    mach[hi_any] = np.take((0.91, 0.95), rng.integers(0, 2, int(hi_any.sum())))
    g["alpha"] = rng.integers(0, len(ALPHAS), n)
    s[:, LX + F16L_VC_KTS] = vc
    s[:, LX + F16L_MACH] = mach
    s[:, LX + F16L_ALPHA] = np.take(ALPHAS, g["alpha"])
    s[:, LX + F16L_NPY] = rng.uniform(-0.5, 0.5, n)
    s[:, LX + F16L_NPZ] = rng.uniform(-3.0, 4.0, n)

    # TEF: lane order is part of the design (the skip is a wave ballot)
    target_val = np.take((TEF_POS, TEF_NEG, 0.0), g["tef_target"])
    g["tef_start"] = rng.integers(0, 8, n)
    tef = np.take(TEF_START_VALUES, g["tef_start"])
    g["wave_kind"] = np.full(n, 2)
    on = np.isin(wave, list(SKIP_WAVES))
    g["wave_kind"][on] = 0
    tef[on] = target_val[on]
    g["tef_start"][on] = np.where(g["tef_target"][on] == 0, 6, np.where(g["tef_target"][on] == 2, 2, 8))
    off = np.isin(wave, list(NONE_WAVES))
    g["wave_kind"][off] = 1
    clash = off & (tef == target_val)
    tef[clash] = 0.5
    g["tef_start"][clash] = 5
    s[:, F16C_TEF] = tef

    # PID integrators (saturating and small), previous inputs of the two with a derivative term
    for c, vals in PID_I.items():
        g[NAMES[c]] = rng.integers(0, len(vals), n)
        s[:, c] = np.take(vals, g[NAMES[c]])
    s[:, F16C_PID_R_P] = rng.uniform(-0.5, 0.5, n)
    s[:, F16C_PID_Y_P] = rng.uniform(-0.5, 0.5, n)

    # N2 against its target 60 + 40 min(2 throttle, 1)
    n2t = 60.0 + 40.0 * np.minimum(2.0 * act[:, 3].astype(np.float64), 1.0)
    g["n2"] = rng.integers(0, len(N2_MODES), n)
    n2 = np.select([g["n2"] == 0, g["n2"] == 1, g["n2"] == 2, g["n2"] == 3, g["n2"] == 4, g["n2"] == 5],
                   [np.minimum(n2t + 10.0, 100.0), np.maximum(n2t - 10.0, 60.0),
                    np.clip(n2t + rng.choice([-0.02, 0.02], n), 60.0, 100.0), n2t, 96.5, 99.0], 100.0)
    s[:, F16C_N2] = n2

    # speedbrake, LEF: the schedule is a function of the planted latch
    g["sb"] = rng.integers(0, len(SB_STARTS), n)
    s[:, F16C_SB] = np.take(SB_STARTS, g["sb"])
    al = s[:, LX + F16L_ALPHA]
    lef_t = np.clip(np.where(al > A2, 0.436, np.where(al > A1, 0.262, np.where(mach > 0.9, -0.0349, 0.0))) * 2.293578,
                    -1.0, 1.0)
    tgt = np.column_stack([_targets(s, act), lef_t])
    for j, c in enumerate((F16C_AIL, F16C_ELE, F16C_RUD, F16C_LEF)):
        m = g[NAMES[c]] = rng.integers(0, len(ACT_MODES), n)
        t = tgt[:, j]
        away = np.where(t > 0.0, -1.0, 1.0)
        s[:, c] = np.select([m == 0, m == 1, m == 2, m == 3],
                            [t + away * 5.0 * LIM[c], np.clip(t + rng.choice([-0.4, 0.4], n) * LIM[c], -1.0, 1.0), t,
                             -1.0], 1.0)
    s = to_device_storage(s)
    return s, act, g


def describe(groups, lane):
    names = {"tef_start": TEF_STARTS, "tef_target": TEF_TARGETS, "wave_kind": WAVE_KINDS, "n2": N2_MODES,
             "throttle": THROTTLES, "alpha": ["%.4f" % a for a in ALPHAS], "sb": SB_STARTS}
    out = []
    for k, v in groups.items():
        tab = names.get(k, ACT_MODES if k in ("AIL", "ELE", "RUD", "LEF") else PID_I.get(
            {"PID_R_I": F16C_PID_R_I, "PID_P_I": F16C_PID_P_I, "PID_Y_I": F16C_PID_Y_I}.get(k)))
        out.append("%s=%s" % (k, tab[int(v[lane])] if tab is not None else int(v[lane])))
    return "lane %d (wave %d): %s" % (lane, lane // 64, ", ".join(out))


# ------------------------------------------------------------------------------------------
# the oracle frame by frame
# ------------------------------------------------------------------------------------------
def _actions_per_step(actions, steps):
    a = np.asarray(actions, np.float32)
    return [a] * steps if a.ndim == 2 else [a[t] for t in range(steps)]


def replay(state, actions, down_sample, steps=1, cfg5=False, seed=7):
    """(final, pre): the oracle's state after `steps` production steps from `state` (final), and
    its state before every frame of them (pre: steps * down_sample arrays). The production
    oracle (down_sample as given) makes the step starts and `final`; the frames inside a step
    are single-frame replays of it with the gust the step drew (cfg5 draws one gust per step,
    with a coefficient of the step's length) held."""
    from oracle_ref import OracleEnvs
    n = len(state)
    prod = OracleEnvs(n, stack_k=1, seed=seed, cfg5=cfg5, down_sample=down_sample)
    prod.reset(goals=far_goals(n))
    prod.set_state(state)
    pre = []
    for a in _actions_per_step(actions, steps):
        cur = prod.get_state()
        pre.append(cur)
        _, _, te, tr, *_ = prod.step(a)
        assert not (te | tr).any(), "a lane finished: the goals are meant to be out of reach"
        if down_sample > 1:
            cur = cur.copy()
            cur[:, F16C_GUST:F16C_GUST + 3] = prod.get_state()[:, F16C_GUST:F16C_GUST + 3]
            for f in range(1, down_sample):
                cur = _one_frame(cur, a)
                pre.append(cur)
    final = prod.get_state()
    prod.close()
    return final, pre


def _near(x, thr):
    return np.abs(x - thr) <= GUARD_REL * abs(thr)


def guarded(oracle_states_per_frame, actions):
    """Lane mask: a switch input within a relative 1e-3 of its threshold before any frame (TEF:
    within 1e-3 of its range of the detent at 0, an exact 0 aside -- that one is a stored value,
    the same on both sides)."""
    pre = oracle_states_per_frame
    a = np.asarray(actions, np.float32)
    thr = a[..., 3].astype(np.float64)
    m = _near(thr, 0.5) if thr.ndim == 1 else _near(thr, 0.5).any(axis=0)
    for s in pre:
        al, ma, vc, tef = s[:, LX + F16L_ALPHA], s[:, LX + F16L_MACH], s[:, LX + F16L_VC_KTS], s[:, F16C_TEF]
        m = m | _near(al, A1) | _near(al, A2) | _near(al * RAD2DEG, 53.0) | _near(ma, 0.9)
        for v in VC_SWITCHES:
            m = m | _near(vc, v)
        m = m | ((tef != 0.0) & (np.abs(tef) <= GUARD_REL))
    return m


# ------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------
def field_errors(a, b):
    """(n, F16C_N) |a - b| in the encodings the comparison uses: the velocity history as the
    deltas the device stores (vI - vIh1, vI - vIh2), the Earth angle as an angle (both of its
    columns), the latch airspeed relative."""
    err = np.abs(a - b)
    for h in (F16C_VIH1, F16C_VIH2):
        da = a[:, F16C_VI:F16C_VI + 3] - a[:, h:h + 3]
        db = b[:, F16C_VI:F16C_VI + 3] - b[:, h:h + 3]
        err[:, h:h + 3] = np.abs(da - db)
    ang = np.arctan2(a[:, F16C_EPA_S], a[:, F16C_EPA_C]) - np.arctan2(b[:, F16C_EPA_S], b[:, F16C_EPA_C])
    ang = np.abs((ang + np.pi) % (2 * np.pi) - np.pi)
    err[:, F16C_EPA_C] = err[:, F16C_EPA_S] = ang
    vc = LX + F16L_VC_KTS
    with np.errstate(divide="ignore", invalid="ignore"):
        err[:, vc] = np.where(b[:, vc] != 0, np.abs(a[:, vc] - b[:, vc]) / np.abs(b[:, vc]), np.abs(a[:, vc]))
    return err


def envelope(states, actions, down_sample, steps=1, cfg5=False, seed=7, mask=None, ref=None, rng=None):
    """(F16C_N,) the oracle's own divergence per field: max over unguarded lanes of |oracle -
    oracle started one fp32 ulp away| after `steps` steps, in field_errors' encodings."""
    rng = rng or np.random.default_rng(20261)
    if ref is None or mask is None:
        ref, pre = replay(states, actions, down_sample, steps, cfg5, seed)
        mask = guarded(pre, actions) if mask is None else mask
    pert, _ = replay(one_ulp(states, rng), actions, down_sample, steps, cfg5, seed)
    return field_errors(pert, ref)[~mask].max(axis=0)


def floors(ref, frames=1, steps=1):
    """(n, F16C_N) the fp32 floor of every field at the reference values (SCALE's derivation)."""
    fl = 4.0 * ulp32(np.maximum(np.abs(ref), SCALE[None, :]))
    dv = np.abs(ref[:, F16C_VI:F16C_VI + 3] - ref[:, F16C_VIH1:F16C_VIH1 + 3])  # the last frame's increment
    for c, inc in INCR.items():
        big = dv[:, c - F16C_VI] if c >= F16C_VI else 0.0   # (a lane beyond 15 g: its own dv)
        fl[:, c] = frames * 4.0 * ulp32(np.maximum(inc, big))
    for h, k in ((F16C_VIH1, 1), (F16C_VIH2, 2)):  # deltas, not values
        fl[:, h:h + 3] = 4.0 * ulp32(SCALE[h])
    fl[:, F16C_EPA_C] = fl[:, F16C_EPA_S] = EPA_FLOOR
    # Latch Mach = vt * rcp(a) ends a long fp32 chain (f16_device.h derive / frame / atmosphere),
    # counted in u = 2^-24, the relative error of one rounded operation (v_rcp / v_rsq / v_sqrt: 2 u):
    #   vt 16 u: the quaternion is normalised with v_rsq (sum of four squares 1 u after the root,
    #     v_rsq 2 u, the product 1 u: |q| = 1 +- 4 u) and quat_T is quadratic in q, so |Ti2b v|
    #     carries 8 u where the oracle's fp64 normalisation leaves 1e-16; the entries of Ti2b 2 u;
    #     vI - w x rI rounded to fp32 1 u; the three-term rows of mvec 2 u; the sum of squares 1 u
    #     after the root; v_sqrt 2 u;
    #   a 6.5 u: geopotential height 5 u (two products, v_rcp, a sum), weighted by lapse * H / T
    #     <= 0.33 in T, T's own sum 1 u, 1.4 R T 2 u, halved by the root; v_sqrt 2 u; the unit
    #     conversion and its constant 2 u;
    #   v_rcp and the product 3 u.
    # 25.5 u = 13 fp32 ulps at max(|ref|, 1), a worst-case count, instead of the 4 of a field that
    # is a few operations away from its inputs.
    ma = LX + F16L_MACH
    fl[:, ma] = MACH_ULPS * ulp32(np.maximum(np.abs(ref[:, ma]), 1.0))
    # Latch airspeed, relative. The device latches the impact pressure qc = p (f(Mach) - 1) as
    # the fp32 difference pt - p, and the canonical vc is its sea-level airspeed. Three terms:
    #   Mach's own floor, relative, times d ln vc / d ln Mach <= 1.22 (evaluated over Mach <= 2.6,
    #     p / p_sl in 0.08 .. 1; 1.25 here);
    #   half (d ln vc / d ln qc <= 0.5) of the static pressure's 1e-7 (atmosphere(): "v_log/v_exp
    #     keep P within ~1e-7 relative");
    #   half of the difference's rounding, 4 ulps of pt <= p_sl + qc relative to qc, qc from the
    #     reference vc at sea level.
    vc = LX + F16L_VC_KTS
    m = np.abs(ref[:, vc]) / 661.4786  # vc / a_sl (kts)
    x = np.where(m < 1.0, (1.0 + 0.2 * m * m) ** 3.5, 166.92158 * m ** 7 / np.maximum(7.0 * m * m - 1.0, 1e-9) ** 2.5) - 1.0
    fl[:, vc] = 1.25 * MACH_ULPS * EPS32 + 0.5e-7 + 2.0 * EPS32 * (1.0 + 1.0 / np.maximum(x, 1e-12))
    # Env layer. LAST_D is an fp32 norm of fp32 frame differences: its 4 ulps. EP_RET sums
    # goal_gain * (last_d - d) per step, each an fp32 difference of two such norms.
    fl[:, F16C_EP_RET] = 4.0 * ulp32(np.maximum(np.abs(ref[:, F16C_EP_RET]), 1.0)) + \
        GOAL_GAIN * 2.0 * fl[:, F16C_LAST_D] * steps
    return fl


def check_state(got, ref, env, mask, frames=1, steps=1, skip=(), not_carried_zero=False):
    """Field-by-field comparison. Returns the report {field name: {"ratio": max err / bound over
    unguarded lanes, "lane", "err", "bound"}} with report["failed"] the names over their bound
    (exact fields: any lane that differs, guarded lanes included). skip: columns left out."""
    err = field_errors(got, ref)
    bound = FACTOR * np.asarray(env)[None, :] + floors(ref, frames, steps)
    ok_lanes = np.flatnonzero(~mask)
    rep, failed = {}, []
    for c in VALUE:
        if c in skip:
            continue
        with np.errstate(invalid="ignore"):
            ratio = err[ok_lanes, c] / bound[ok_lanes, c]
        ratio = np.where(np.isnan(err[ok_lanes, c]), np.inf, ratio)
        k = int(np.argmax(ratio))
        rep[NAMES[c]] = {"ratio": float(ratio[k]), "lane": int(ok_lanes[k]), "err": float(err[ok_lanes[k], c]),
                         "bound": float(bound[ok_lanes[k], c])}
        if not ratio[k] <= 1.0:
            failed.append(NAMES[c])
    for c in EXACT:
        if c in skip:
            continue
        bad = np.flatnonzero(got[:, c] != ref[:, c])
        rep[NAMES[c]] = {"ratio": float(len(bad) > 0), "lane": int(bad[0]) if len(bad) else -1,
                         "err": float(len(bad)), "bound": 0.0}
        if len(bad):
            failed.append(NAMES[c])
    if not_carried_zero:
        for c in NOT_CARRIED:
            if np.any(got[:, c] != 0.0):
                failed.append(NAMES[c] + " (not carried: must read 0)")
    rep["failed"] = failed
    return rep


def group_ratios(rep):
    """{group: worst ratio of its fields} of a check_state report."""
    out = {}
    for gname, cols in FIELD_GROUPS.items():
        r = [rep[NAMES[c]]["ratio"] for c in cols if NAMES[c] in rep]
        if r:
            out[gname] = max(r)
    return out


# ------------------------------------------------------------------------------------------
# the cases tests/test_gpu_state_parity.py runs; the oracle side of each is computed once and
# shared (read-only) with tests/test_state_corners_cpu.py
# ------------------------------------------------------------------------------------------
N_LANES = 4133  # 64 whole waves and a ragged tail of 37 lanes
SEED = 7
STEADY_WIND = (20.0, -15.0, 2.0)  # NED fps, planted on every other lane of the "wind" states
# (states, down_sample, steps)
ORACLE_CASES = [("plain", 1, 1), ("plain", 2, 1), ("plain", 4, 1), ("wind", 1, 1), ("wind", 4, 1), ("cfg5", 4, 1),
                ("plain", 4, 2)]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def planted(kind):
    """(state, actions, groups) of the "plain", "wind" or "cfg5" corner states."""
    s, a, g = corner_states(N_LANES, np.random.default_rng(2026), cfg5=kind == "cfg5", seed=SEED)
    if kind == "wind":
        s[::2, F16C_WIND:F16C_WIND + 3] = STEADY_WIND
        s = to_device_storage(s)
    _frozen(s, a, *g.values())
    return s, a, g


@functools.lru_cache(maxsize=None)
def oracle_case(kind, down_sample, steps=1):
    """(ref, pre, mask, env): the oracle's final state, its state before every frame, the
    guarded lanes and the oracle's own envelope of one case."""
    s, a, _ = planted(kind)
    ref, pre = replay(s, a, down_sample, steps, cfg5=kind == "cfg5", seed=SEED)
    mask = guarded(pre, a)
    env = envelope(s, a, down_sample, steps, cfg5=kind == "cfg5", seed=SEED, mask=mask, ref=ref)
    _frozen(ref, mask, env, *pre)
    return ref, pre, mask, env
