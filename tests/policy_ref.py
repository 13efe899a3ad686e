"""Checker of the device policy (f16env_policy_forward): an fp64 numpy restatement of the
actor-critic MLP forward and of the policy noise stream (include/f16env.h), independent of the
kernel, its blob layout and torch."""
from __future__ import annotations

import numpy as np

from rng_ref import MASK, philox4x32

LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def policy_normals(seed, gid, step):
    """(N, 4) float64: Philox4x32-10 keyed by seed, counter (gid, gid_hi ^ 'POLI', step, step_hi),
    two Box-Muller pairs from 24-bit uniforms (the first of a pair offset by half a step)."""
    gid = np.asarray(gid, np.uint64)
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    o = philox4x32(np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32), (gid & MASK).astype(np.uint32),
                   (gid >> np.uint64(32)).astype(np.uint32) ^ np.uint32(0x504F4C49),
                   np.uint32(step & 0xFFFFFFFF), np.uint32(step >> 32))
    s24 = 1.0 / 16777216.0
    u1 = ((o[0] >> 8).astype(np.float64) + 0.5) * s24
    u2 = (o[1] >> 8).astype(np.float64) * s24
    u3 = ((o[2] >> 8).astype(np.float64) + 0.5) * s24
    u4 = (o[3] >> 8).astype(np.float64) * s24
    r1, r2 = np.sqrt(-2.0 * np.log(u1)), np.sqrt(-2.0 * np.log(u3))
    return np.stack([r1 * np.cos(2 * np.pi * u2), r1 * np.sin(2 * np.pi * u2),
                     r2 * np.cos(2 * np.pi * u4), r2 * np.sin(2 * np.pi * u4)], -1)


def _mlp(x, layers, activation):
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    for w, b in layers:
        x = act(x @ np.asarray(w, np.float64).T + np.asarray(b, np.float64))
    return x


def log_prob_eps(eps, log_std):
    return (-0.5 * eps * eps - np.asarray(log_std, np.float64) - LOG_SQRT_2PI).sum(-1)


def forward(obs, pi, vf, act_head, val_head, log_std, eps, activation="tanh"):
    """obs (n, K, D); pi / vf lists of (W[out][in], b); heads (W, b); log_std[4]; eps (n, 4).
    Returns fp64 (actions (n, 4), values (n,), log_probs (n,), mean (n, 4))."""
    x = np.asarray(obs, np.float64).reshape(len(obs), -1)
    mean = _mlp(x, pi, activation) @ np.asarray(act_head[0], np.float64).T + np.asarray(act_head[1], np.float64)
    values = (_mlp(x, vf, activation) @ np.asarray(val_head[0], np.float64).T + np.asarray(val_head[1], np.float64))[:, 0]
    eps = np.asarray(eps, np.float64)
    ls = np.asarray(log_std, np.float64)
    return mean + np.exp(ls) * eps, values, log_prob_eps(eps, ls), mean
