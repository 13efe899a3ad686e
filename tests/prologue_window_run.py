"""Fixed workload for tests/test_gpu_prologue_window.py (TEST INFRASTRUCTURE; a child process with
F16ENV_LIB naming the library under test): the step kernel's counted prologue waits and windowed
breakpoint counts must not change a bit, so every library built from this source -- the product,
the reference form (-DF16_PROLOGUE_ONE_WAIT -DF16_BRACKET_FULL), the -O1 and the debug builds --
must print the same sha256 per case.

Each case: n = 197 envs (three full waves and a partial one of 5 lanes), reset, then set_state
puts lanes outside every breakpoint window -- wave 0 one lane pitched 30 deg (alpha), wave 1 one
lane yawed 12 deg (beta), wave 2 one lane at Mach 1.3 -- while wave 3 (the partial one) keeps
every lane inside; 64 steps with auto-resets; the state, observation, rewards and flags are
hashed. The perturbed lanes' first-frame alpha / beta / Mach are reported so the test can see
that they did leave the windows.

    F16ENV_LIB=f16_jsb_amd/libf16env_o1.so python tests/prologue_window_run.py
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

N = 197
LANE_ALPHA, LANE_BETA, LANE_MACH, LANE_NAN = 7, 64 + 21, 128 + 40, 64 + 3
OMEGA_E = 0.00007292115
# canonical state columns (include/f16env.h F16C_*)
C_RI, C_VI, C_VIH1, C_VIH2, C_Q, C_WI, C_LX = 0, 3, 6, 9, 18, 22, 48

CASES = [dict(tag="window_k4", stack_k=4, obs_layout="window"),
         dict(tag="window_k1", stack_k=1, obs_layout="window"),
         dict(tag="contiguous_k4", stack_k=4, obs_layout="contiguous"),
         dict(tag="contiguous_k1", stack_k=1, obs_layout="contiguous"),
         dict(tag="cfg5_window_k4", stack_k=4, obs_layout="window", cfg5=True),
         dict(tag="cfg5_contiguous_k4", stack_k=4, obs_layout="contiguous", cfg5=True),
         dict(tag="nan_guard_window_k4", stack_k=4, obs_layout="window", nan_guard=True)]


def qmul(a, b):  # Hamilton product
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def perturb(s, nan_lane=False):
    """s: (N, F16C_N) float64 canonical state after a reset (every lane inside the windows)."""
    s = s.copy()
    # a rotation of the body about its own y axis by 30 deg moves alpha by 30 deg, about its z
    # axis by 12 deg moves beta by 12 deg (the frame derives both from the attitude and velocity)
    for lane, axis, deg in ((LANE_ALPHA, 2, 30.0), (LANE_BETA, 3, 12.0)):
        r = np.zeros(4)
        r[0], r[axis] = np.cos(np.radians(deg) / 2), np.sin(np.radians(deg) / 2)
        s[lane, C_Q:C_Q + 4] = qmul(s[lane, C_Q:C_Q + 4], r)
    # Mach 1.3: scale the velocity relative to the rotating Earth (and its AB3 history alike)
    m0 = s[LANE_MACH, C_LX + 2]
    rI = s[LANE_MACH, C_RI:C_RI + 3]
    we = OMEGA_E * np.array([-rI[1], rI[0], 0.0])  # omega x r
    for c in (C_VI, C_VIH1, C_VIH2):
        s[LANE_MACH, c:c + 3] = we + (s[LANE_MACH, c:c + 3] - we) * (1.3 / m0)
    if nan_lane:
        s[LANE_NAN, C_WI + 1] = np.nan  # a NaN body rate: quarantined by F16_FLAG_NAN_GUARD
    return s


def main():
    import torch
    from f16_jsb_amd._lib import lib
    from f16_jsb_amd.env import F16Envs
    res = {}
    for c in CASES:
        c = dict(c)
        tag = c.pop("tag")
        e = F16Envs(N, seed=21, max_steps=20, **c)
        e.reset()
        e.set_state(perturb(e.get_state().cpu().numpy(), nan_lane=c.get("nan_guard", False)))
        h = hashlib.sha256()
        first = None
        for t in range(64):
            o = e.step(e.sample_actions(9, t))
            for x in (o.rew, o.terminated, o.truncated):
                h.update(x.detach().cpu().numpy().tobytes())
            if t == 0:
                first = e.get_state().cpu().numpy()[:, C_LX:C_LX + 3].copy()
        st = e.get_state().cpu().numpy()
        for x in (st, o.obs.contiguous().cpu().numpy()):
            h.update(x.tobytes())
        v = ctypes.c_uint32()
        is_debug = lib().f16env_debug_checks(e._h, None, ctypes.byref(v))
        torch.cuda.synchronize()
        res[tag] = {"sha256": h.hexdigest(), "kernel": e.step_kernel_name, "is_debug": int(is_debug),
                    "violations": int(v.value), "nonfinite": e.nonfinite_count if c.get("nan_guard") else 0,
                    "alpha": float(first[LANE_ALPHA, 0]), "beta": float(first[LANE_BETA, 1]),
                    "mach": float(first[LANE_MACH, 2]),
                    # the untouched lanes after the first step (wave 3 is among them)
                    "clean_alpha": [float(np.delete(first[:, 0], [LANE_ALPHA, LANE_BETA, LANE_MACH, LANE_NAN]).min()),
                                    float(np.delete(first[:, 0], [LANE_ALPHA, LANE_BETA, LANE_MACH, LANE_NAN]).max())],
                    "clean_beta_abs": float(np.abs(np.delete(first[:, 1], [LANE_ALPHA, LANE_BETA, LANE_MACH, LANE_NAN])).max()),
                    "clean_mach": [float(np.delete(first[:, 2], [LANE_ALPHA, LANE_BETA, LANE_MACH, LANE_NAN]).min()),
                                   float(np.delete(first[:, 2], [LANE_ALPHA, LANE_BETA, LANE_MACH, LANE_NAN]).max())]}
        e.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
