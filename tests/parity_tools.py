"""Shared helpers for HIP-vs-oracle parity checks (test infrastructure)."""
from __future__ import annotations

import numpy as np

from f16_jsb_amd.abi import (F16C_AI, F16C_AIP, F16C_BA, F16C_CMD, F16C_EP_COUNT, F16C_EP_RET,
                             F16C_EPA_C, F16C_GOAL, F16C_LX, F16C_N, F16C_Q, F16C_RI, F16C_STEP,
                             F16C_VI, F16C_VIH1, F16C_VIH2, F16C_WI, F16C_WID, F16C_WIND,
                             F16L_N)

FRAME_NAMES = ["lat*R", "lon*R", "h_m", "mach", "alpha", "beta", "p", "q", "r", "phi", "theta", "psi",
               "goal_x", "goal_y", "goal_z"]
ANGLE_COLS = (9, 10, 11)


def frame_err(a, b):
    """|a-b| per frame component (angles wrapped to [-pi, pi))."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    d = np.abs(a - b)
    for c in ANGLE_COLS:
        w = np.abs((a[..., c] - b[..., c] + np.pi) % (2 * np.pi) - np.pi)
        d[..., c] = w
    return d


def edge_ics(n, rng):
    """Flight-envelope edge ICs in five groups of n // 5 lanes (tests/test_gpu_envelope.py names
    them; tests/fp32_envelope.py's edge workload draws the same)."""
    from oracle_ref import default_ic
    ic = np.tile(default_ic(), (n, 1))
    q = n // 5
    # 0: stratosphere and above, transonic to supersonic
    ic[:q, 2] = rng.uniform(36089.0, 75000.0, q)
    ic[:q, 3] = rng.uniform(700.0, 2100.0, q)
    # 1: supersonic at low / mid altitude
    ic[q:2 * q, 2] = rng.uniform(5000.0, 35000.0, q)
    ic[q:2 * q, 3] = rng.uniform(1300.0, 2300.0, q)
    # 2: alpha / beta outside the tables (large w, v body velocities)
    ic[2 * q:3 * q, 3] = rng.uniform(250.0, 700.0, q)
    ic[2 * q:3 * q, 4] = rng.uniform(-450.0, 450.0, q)
    ic[2 * q:3 * q, 5] = rng.uniform(-350.0, 700.0, q)
    ic[2 * q:3 * q, 2] = rng.uniform(8000.0, 30000.0, q)
    # 3: inverted / near-vertical attitudes, high body rates
    ic[3 * q:4 * q, 6] = rng.uniform(-np.pi, np.pi, q)
    ic[3 * q:4 * q, 7] = rng.uniform(-1.48, 1.48, q)
    ic[3 * q:4 * q, 9:12] = rng.uniform(-4.0, 4.0, (q, 3))
    ic[3 * q:4 * q, 2] = rng.uniform(10000.0, 40000.0, q)
    # 4: just above the 10 m crash floor (jsbsim_gym.py:245), nose down
    ic[4 * q:, 2] = rng.uniform(40.0, 130.0, n - 4 * q)
    ic[4 * q:, 7] = rng.uniform(-0.8, -0.3, n - 4 * q)
    ic[:, 8] = rng.uniform(0.0, 2 * np.pi, n)
    ic[:, 15] = rng.uniform(0.0, 1.0, n)  # throttle at IC (augmentor above 0.5 x 2)
    return ic


def report(name, err):
    """Max error per frame component as a dict."""
    err = np.asarray(err)
    flat = err.reshape(-1, err.shape[-1])
    return {name + ":" + FRAME_NAMES[i]: float(flat[:, i].max()) for i in range(flat.shape[-1])}


# Canonical-state fields the two paths are compared on (the HIP path does not keep the last
# command or double-precision AB histories; those are excluded or compared loosely).
def state_err(gpu, ref):
    g = np.asarray(gpu, np.float64)
    r = np.asarray(ref, np.float64)
    out = {}
    out["rI_ft"] = np.abs(g[:, F16C_RI:F16C_RI + 3] - r[:, F16C_RI:F16C_RI + 3]).max()
    out["vI_fps"] = np.abs(g[:, F16C_VI:F16C_VI + 3] - r[:, F16C_VI:F16C_VI + 3]).max()
    out["q"] = np.abs(g[:, F16C_Q:F16C_Q + 4] - r[:, F16C_Q:F16C_Q + 4]).max()
    out["wI"] = np.abs(g[:, F16C_WI:F16C_WI + 3] - r[:, F16C_WI:F16C_WI + 3]).max()
    out["aI"] = np.abs(g[:, F16C_AI:F16C_AI + 3] - r[:, F16C_AI:F16C_AI + 3]).max()
    fcs = [c for c in range(33, 45) if c != 42]  # PID_P_P: not carried by the HIP path (kd = 0)
    out["fcs"] = np.abs(g[:, fcs] - r[:, fcs]).max()
    out["n2"] = np.abs(g[:, 46] - r[:, 46]).max()
    out["lx_alpha"] = np.abs(g[:, F16C_LX] - r[:, F16C_LX]).max()
    out["lx_mach"] = np.abs(g[:, F16C_LX + 2] - r[:, F16C_LX + 2]).max()
    out["lx_vc"] = np.abs(g[:, F16C_LX + 3] - r[:, F16C_LX + 3]).max()
    out["lx_npz"] = np.abs(g[:, F16C_LX + 9] - r[:, F16C_LX + 9]).max()
    return {k: float(v) for k, v in out.items()}
