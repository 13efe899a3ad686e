"""Checker for the device minibatch sampler: a numpy restatement of stable_baselines3's
RolloutBuffer.get / _get_samples (common/buffers.py:481-521) and swap_and_flatten (:36-50),
written here. It works on the materialised observations (rebuild_observations' output) and the
buffer's own arrays, so it shares no code with the kernel under test, which never builds them.
"""
from __future__ import annotations

import numpy as np
import torch

from f16_jsb_amd.rollout import env_major, rebuild_observations

NAMES = ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns")
_SOURCES = ("observations", "actions", "values", "log_probs", "advantages", "returns")  # buffers.py:486-493


def swap_and_flatten(arr: np.ndarray) -> np.ndarray:
    """buffers.py:36-50: (n_steps, n_envs, ...) -> (n_steps * n_envs, ...), env-major."""
    shape = arr.shape
    if len(shape) < 3:
        shape = (*shape, 1)
    return arr.swapaxes(0, 1).reshape(shape[0] * shape[1], *shape[2:])


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def flat_fields(src, k: int):
    """The six flattened arrays get() indexes (buffers.py:495-496), from a buffer's state dict
    (T, N, ...) or gather_to_rank0's rank-major dict (world, T, N, ...; env_major of each field,
    obs0's shards side by side). Computed on the arrays' own device, returned as numpy."""
    sd = src.state_dict() if hasattr(src, "state_dict") else src
    if sd["frames"].dim() == 4:
        obs0 = sd["obs0"].reshape((-1,) + tuple(sd["obs0"].shape[2:]))  # (world * N, K, 15): global env order
        sd = {f: env_major(x) for f, x in sd.items() if f != "obs0"}
        sd["obs0"] = obs0
    obs = rebuild_observations(sd["frames"], sd["obs0"], sd["episode_starts"], k)
    arrays = {"observations": obs, **{f: sd[f] for f in _SOURCES[1:]}}
    return {f: swap_and_flatten(_np(arrays[f])) for f in _SOURCES}


def get_samples(flat, batch_inds):
    """buffers.py:508-521 over flat_fields' arrays."""
    i = _np(batch_inds)
    return (flat["observations"][i], flat["actions"][i], flat["values"][i].flatten(), flat["log_probs"][i].flatten(),
            flat["advantages"][i].flatten(), flat["returns"][i].flatten())


def get(flat, indices, batch_size=None):
    """buffers.py:481-506 with the permutation given (SB3 draws np.random.permutation there)."""
    indices = _np(indices)
    total = flat["actions"].shape[0]
    if batch_size is None:
        batch_size = total
    start_idx = 0
    while start_idx < total:
        yield get_samples(flat, indices[start_idx:start_idx + batch_size])
        start_idx += batch_size


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(_np(x), dtype=np.float32).view(np.int32)


def assert_same_bits(got, want, what=""):
    """Every field of a RolloutSamples equal to the checker's, as int32 views (bits)."""
    assert len(got) == len(want) == 6
    for name, g, w in zip(NAMES, got, want):
        assert tuple(g.shape) == tuple(w.shape), (what, name, tuple(g.shape), tuple(w.shape))
        gi = g.contiguous().view(torch.int32).cpu()
        wi = torch.from_numpy(bits(w))
        assert torch.equal(gi, wi), "%s %s: %d of %d words differ" % (what, name, int((gi != wi).sum()), gi.numel())
