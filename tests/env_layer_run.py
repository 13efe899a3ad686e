"""Fixed workload for tests/test_gpu_env_layer.py (TEST INFRASTRUCTURE; a child process with
F16ENV_LIB naming the library under test, and F16ENV_OCC=2 for the two-waves-per-SIMD kernels):
the env layer's wave-uniform fast paths (f16_env_layer.h euler_norm, env_reward_sel) must not change a
bit, so every library built from this source -- the product, the reference forms
(-DF16_ENV_LAYER_REF), the -O1 and the debug builds -- must print the same sha256 per case.

(a) n = 197 envs (three full waves and a five-lane one), K = 4 and 1, windowed and contiguous,
    cfg3 and cfg5, and a NaN-guarded run with one NaN body rate: 96 steps with max_steps = 24, so
    every lane truncates and auto-resets four times; lanes of wave 1 start around the crash
    altitude. State, observation, rewards, flags, ep_return and ep_len are hashed every step.
(b) down_sample = 0 (no FDM frame: the observation is that of the set state exactly), n = 128:
    set_state puts wave 0's lanes on every slow path of the angle code -- both gimbal poles, a roll
    of exactly 180 deg, the attitude of the local frame (angles +-0 or below 2^-24), a heading
    just west of north -- among ordinary lanes, and gives wave 1 ordinary attitudes only, half of
    them with a heading west of north (the fp64 form of the fast path). The classes found in the
    newest frame's angles are reported for the test to assert on.

    F16ENV_LIB=f16_jsb_amd/libf16env_o1.so python tests/env_layer_run.py
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_A, N_B = 197, 128
LANE_NAN = 128 + 3
WGS_A = 20925646.32546
# canonical state columns (include/f16env.h F16C_*)
C_RI, C_Q, C_WI, C_EPA_C, C_EPA_S = 0, 18, 22, 31, 32
f32 = np.float32
PI_F = f32(3.14159265358979323846)
ORD_MIN = f32(2.0 ** -24)

CASES_A = [dict(tag="%s%s_k%d" % ("cfg5_" if cfg5 else "", layout, k), stack_k=k, obs_layout=layout, cfg5=cfg5)
           for cfg5 in (False, True) for layout in ("window", "contiguous") for k in (4, 1)]
CASES_A.append(dict(tag="nan_guard_window_k4", stack_k=4, obs_layout="window", nan_guard=True))
CASES_B = [dict(tag="set_state_window_k4", stack_k=4, obs_layout="window"),
           dict(tag="set_state_contiguous_k1", stack_k=1, obs_layout="contiguous")]


def low_altitudes(s, crash_alt_m=10.0):
    """Every fourth lane of wave 1 to -5 .. +60 m around the crash altitude (the ICs sit on the
    equator at longitude 0: the altitude is the ECI x coordinate less the equatorial radius)."""
    s = s.copy()
    for i, lane in enumerate(range(64, 128, 4)):
        dm = (-5.0, 1.0, 3.0, 10.0, 30.0, 60.0)[i % 6]
        s[lane, C_RI:C_RI + 3] = (WGS_A + (crash_alt_m + dm) / 0.3048, 0.0, 0.0)
    return s


# ECI -> local (north, east, down) at ECI position (r, 0, 0)
TI2L = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])


def quat_of(T):
    """FGMatrix33::GetQuaternion (as apply_ic): the ECI -> body quaternion of the matrix."""
    t = [1.0 + T[0, 0] + T[1, 1] + T[2, 2], 1.0 + T[0, 0] - T[1, 1] - T[2, 2],
         1.0 - T[0, 0] + T[1, 1] - T[2, 2], 1.0 - T[0, 0] - T[1, 1] + T[2, 2]]
    i = int(np.argmax(t))
    q = np.zeros(4)
    q[i] = 0.5 * np.sqrt(t[i])
    d = 0.25 / q[i]
    if i == 0:
        q[1], q[2], q[3] = (T[1, 2] - T[2, 1]) * d, (T[2, 0] - T[0, 2]) * d, (T[0, 1] - T[1, 0]) * d
    elif i == 1:
        q[0], q[2], q[3] = (T[1, 2] - T[2, 1]) * d, (T[0, 1] + T[1, 0]) * d, (T[0, 2] + T[2, 0]) * d
    elif i == 2:
        q[0], q[1], q[3] = (T[2, 0] - T[0, 2]) * d, (T[0, 1] + T[1, 0]) * d, (T[1, 2] + T[2, 1]) * d
    else:
        q[0], q[1], q[2] = (T[0, 1] - T[1, 0]) * d, (T[0, 2] + T[2, 0]) * d, (T[1, 2] + T[2, 1]) * d
    return q / np.linalg.norm(q)


def quat_euler(phi, tht, psi):
    """ECI -> body quaternion of a body with these Euler angles against the local frame at (r, 0, 0)."""
    cp, sp, ct, st, cs, ss = np.cos(phi), np.sin(phi), np.cos(tht), np.sin(tht), np.cos(psi), np.sin(psi)
    tl = np.array([[ct * cs, ct * ss, -st],
                   [sp * st * cs - cp * ss, sp * st * ss + cp * cs, sp * ct],
                   [cp * st * cs + sp * ss, cp * st * ss - sp * cs, cp * ct]])
    return quat_of(tl @ TI2L)


def attitudes(s):
    """Case (b)'s states. Every lane at ECI (2^25 ft, 0, 0), Earth angle 0: there the fp32 local
    frame is exact (its direction cosines are 0 and +-1), so Tl2b's entries are single entries of
    the quaternion's matrix and the special lanes below reach their exact values."""
    s = s.copy()
    s[:, C_RI:C_RI + 3] = (2.0 ** 25, 0.0, 0.0)
    s[:, C_EPA_C], s[:, C_EPA_S] = 1.0, 0.0
    rng = np.random.default_rng(4)
    for lane in range(N_B):  # ordinary attitudes: every angle well inside [2^-24, PI_F)
        sg = rng.choice([-1.0, 1.0], 3)
        psi = sg[2] * rng.uniform(0.01, 3.0)
        if lane >= 64:
            psi = abs(psi) * (-1.0 if lane % 2 else 1.0)  # wave 1: every other lane west of north
        s[lane, C_Q:C_Q + 4] = quat_euler(sg[0] * rng.uniform(0.01, 3.0), sg[1] * rng.uniform(0.01, 1.5), psi)
    c = float(f32(np.sqrt(0.5)))
    cu = float(np.nextafter(f32(c), f32(1.0)))
    z, e = 0.0, 1e-9
    special = [
        (1.0, z, z, z), (z, z, 1.0, z),        # Tl2b[2] = -1, +1: the gimbal arms (theta = +-PI_F/2)
        (cu, cu, z, z), (z, z, cu, cu),        # Tl2b[2] = -1.0000001, +1.0000001
        (c, z, c, z), (c, -z, c, z), (c, z, c, -z), (c, -z, c, -z),  # roll of +-180 deg exactly (Tl2b[5] = -+0)
        (c, z, -c, z), (c, -z, -c, z), (c, z, -c, -z), (c, -z, -c, -z),  # the local frame's attitude: angles +-0
        (c, e, -c, z), (c, -e, -c, z), (c, z, -c, e), (c, z, -c, -e),  # ... and a few 1e-9 rad off it
    ]
    for i, q in enumerate(special):
        s[3 + 3 * i, C_Q:C_Q + 4] = q
    for i, psi in enumerate((-1e-3, -1e-6, -2.0 ** -24, -1e-7)):  # just west of north, nose and wings off level
        s[52 + 3 * i, C_Q:C_Q + 4] = quat_euler(0.05, 0.03, psi)
    return s


def angle_classes(ang):
    """The slow / fast path classes in (N_B, 3) float32 observed angles (phi, theta, psi)."""
    m = np.abs(ang)
    w1 = m[64:]
    return {"tiny": int((m < ORD_MIN).sum()), "tiny_nonzero": int(((m < ORD_MIN) & (m > 0)).sum()),
            "minus_pi": int((ang == f32(-3.1415925)).sum()),
            "theta_half_pi": int((m[:, 1] == PI_F / f32(2)).sum()),
            # euler() wraps a heading west of north by 2*PI_F (psi above PI_F); normalised it is negative
            "psi_wrapped_wave0": int((ang[:64, 2] < 0).sum()), "psi_wrapped_wave1": int((ang[64:, 2] < 0).sum()),
            "wave1_ordinary": bool(((w1 >= ORD_MIN) & (w1 < f32(3.1))).all())}


def run_case(c, n, steps, prepare, **kw):
    import torch
    from f16_jsb_amd._lib import lib
    from f16_jsb_amd.env import F16Envs
    c = dict(c)
    tag = c.pop("tag")
    e = F16Envs(n, seed=21, **c, **kw)
    e.reset()
    e.set_state(prepare(e.get_state().cpu().numpy(), c))
    h = hashlib.sha256()
    n_term = n_trunc = n_crash = 0
    for t in range(steps):
        o = e.step(e.sample_actions(9, t))
        rew, te, tr = (x.detach().cpu().numpy() for x in (o.rew, o.terminated, o.truncated))
        n_term += int((te != 0).sum())
        n_trunc += int((tr != 0).sum())
        n_crash += int(((te != 0) & (rew < -5.0)).sum())
        for x in (e.get_state().cpu().numpy(), o.obs.contiguous().cpu().numpy(), rew, te, tr,
                  o.ep_return.cpu().numpy(), o.ep_len.cpu().numpy()):
            h.update(x.tobytes())
    v = ctypes.c_uint32()
    is_debug = lib().f16env_debug_checks(e._h, None, ctypes.byref(v))
    torch.cuda.synchronize()
    res = {"sha256": h.hexdigest(), "kernel": e.step_kernel_name, "is_debug": int(is_debug), "violations": int(v.value),
           "nonfinite": e.nonfinite_count if c.get("nan_guard") else 0, "terminated": n_term, "truncated": n_trunc,
           "crashed": n_crash, "last_angles": o.obs[:, -1, 9:12].contiguous().cpu().numpy()}
    e.close()
    return tag, res


def main():
    res = {}

    def prep_a(s, c):
        s = low_altitudes(s)
        if c.get("nan_guard"):
            s[LANE_NAN, C_WI + 1] = np.nan  # a NaN body rate: quarantined by F16_FLAG_NAN_GUARD
        return s

    for c in CASES_A:
        tag, r = run_case(c, N_A, 96, prep_a, max_steps=24)
        del r["last_angles"]
        res[tag] = r
    for c in CASES_B:
        tag, r = run_case(c, N_B, 2, lambda s, c: attitudes(s), down_sample=0)
        r["classes"] = angle_classes(r.pop("last_angles"))
        res[tag] = r
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
