"""Checker of the device policy (f16env_policy_forward): an fp64 numpy restatement of the
actor-critic MLP forward and of the policy noise stream (include/f16env.h), independent of the
kernel and torch; the documented blob layout read back (unpack_blob), the documented rule that
picks the kernel instance (kernel_instance), and the architecture matrix the CPU and GPU tests
share (MATRIX). Nothing here imports f16_jsb_amd."""
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


# ---------------------------------------------------------------------------------------------
# the weight blob and the kernel instance, restated from include/f16env.h and DESIGN.md section 4
HEAD_TILE = 32             # a head is stored as one tile of 32 outputs
ACT_DIM, VAL_DIM = 4, 1
LDS_BYTES = 160 * 1024     # the blob goes to LDS when it fits there with the images
WAVES, ROWS, OBS_STRIDE = 4, 32, 33


def _blob_pieces(k, d, pi_widths, vf_widths):
    """[(name, rows stored, outputs used, fan_in)] in blob order: the hidden layers of pi, then of
    vf, then the action head and the value head (one tile each)."""
    pieces = []
    for name, widths in (("pi", pi_widths), ("vf", vf_widths)):
        fan_in = k * d
        for l, w in enumerate(widths):
            pieces.append(("%s%d" % (name, l), int(w), int(w), fan_in))
            fan_in = int(w)
    pieces.append(("act_head", HEAD_TILE, ACT_DIM, int(pi_widths[-1])))
    pieces.append(("val_head", HEAD_TILE, VAL_DIM, int(vf_widths[-1])))
    return pieces


def blob_floats(k, d, pi_widths, vf_widths):
    """Length of the blob: per piece rows/32 tiles x ceil(fan_in/2) k-steps x 64 weights and `rows`
    biases, then log_std[4]."""
    return sum((rows // 32) * ((fan_in + 1) // 2) * 64 + rows
               for _, rows, _, fan_in in _blob_pieces(k, d, pi_widths, vf_widths)) + 4


def kernel_instance(k, d, pi_widths, vf_widths):
    """(D, wlds) of the f16_policy_forward_kernel<D, WLDS> a descriptor runs on, by DESIGN
    section 4's rule: the blob is copied into LDS when its bytes and the four waves' images
    (observation image: K D rounded up to even inputs at a row stride of 33 floats; hidden image:
    the widest layer x 32 rows) fit 160 KiB together."""
    in_dim = k * d
    images = WAVES * ((in_dim + in_dim % 2) * OBS_STRIDE + max(list(pi_widths) + list(vf_widths)) * ROWS)
    return int(d), 4 * (blob_floats(k, d, pi_widths, vf_widths) + images) <= LDS_BYTES


def unpack_blob(k, d, pi_widths, vf_widths, blob):
    """The layers a blob holds, read back by the documented element map alone:
    weight element W[o][i] of a piece with nks = ceil(fan_in/2) k-steps sits at
    ((o // 32 * nks + i // 2) * 2 + i % 2) * 32 + o % 32 from the piece's start, its bias follows.
    Returns {"pi": [(W, b)], "vf": [(W, b)], "act_head": (W, b), "val_head": (W, b), "log_std",
    "zero": the positions that must hold zero (the pad input of an odd fan-in, head rows and head
    biases past 4 / 1), "claims": per blob float, how many of the above claim it (all 1 when the
    pieces account for the blob exactly)}."""
    blob = np.asarray(blob)
    claims = np.zeros(blob.shape[0], np.int64)
    zero, out, p = [], {"pi": [], "vf": []}, 0
    for name, rows, used, fan_in in _blob_pieces(k, d, pi_widths, vf_widths):
        assert p % 4 == 0, "a piece starts on a multiple of 4 floats"
        nks = (fan_in + 1) // 2
        o, i = np.arange(rows)[:, None], np.arange(2 * nks)[None, :]
        pos = p + ((o // 32 * nks + i // 2) * 2 + i % 2) * 32 + o % 32
        p += (rows // 32) * nks * 64
        bpos = p + np.arange(rows)
        p += rows
        np.add.at(claims, pos.ravel(), 1)
        np.add.at(claims, bpos, 1)
        zero += [pos[used:, :].ravel(), pos[:used, fan_in:].ravel(), bpos[used:]]
        layer = (blob[pos[:used, :fan_in]], blob[bpos[:used]])
        if name in ("act_head", "val_head"):
            out[name] = layer
        else:
            out[name[:2]].append(layer)
    assert p % 4 == 0
    out["log_std"] = blob[p:p + 4]
    claims[p:p + 4] += 1
    assert p + 4 == blob_floats(k, d, pi_widths, vf_widths)
    out["zero"] = np.concatenate(zero)
    out["claims"] = claims
    return out


# name: (K, D, pi widths, vf widths, (D, wlds) of the kernel instance it reaches)
MATRIX = {
    "A": (1, 17, [32], [128], (17, True)),               # one-layer branches, 1 and 4 tiles, fan-in 17 (9 k-steps)
    "B": (2, 15, [96], [32, 32, 32], (15, True)),        # 15 k-steps (3 mod 4), 3 tiles, three-layer vf
    "C": (10, 15, [64, 64], [64, 64], (15, False)),      # SB3's default net at the reference stack
    "D": (10, 17, [64, 64], [128, 64], (17, False)),     # the reference's training network
    "E": (4, 15, [64, 64], [128, 64], (15, False)),      # the architecture of tools/policy_ab.py
    "F": (10, 17, [128, 128, 128], [128, 128, 128], (17, False)),  # the largest images and blob
    "G": (4, 17, [64, 64], [64, 64], (17, True)),
    "H": (7, 17, [96, 32], [64, 128, 96], (17, False)),  # mixed tile counts, 60 k-steps
    "I": (9, 17, [32], [32], (17, True)),                # odd fan-in 153 at large K
}
