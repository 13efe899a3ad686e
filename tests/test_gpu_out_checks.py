"""The caller's `out` of features.features and telemetry.poses goes through buffers.need_tensor
like every other caller buffer: a CPU, float16, wrong-shape or non-contiguous `out` is refused
with ValueError before any launch (it stays as it was, f16env_last_error stays as it was), and
the right one receives the bits of the out=None call. Both arms of features(): a contiguous
block (f16env_features) and a windowed observation view read in place (f16env_features_strided).
poses(): (N, 15) frames, a contiguous stack, and the window view (its base pointer and row stride).
"""
from __future__ import annotations

import pytest

N, K = 64, 2


def _obs(torch, kind):
    """A (64, 2, 15) contiguous block, the strided window view of a windowed handle, or (64, 15) frames."""
    if kind == "window":
        from f16_jsb_amd.env import F16Envs
        e = F16Envs(N, stack_k=K, obs_layout="window", seed=3)
        e.reset()
        for t in range(3):
            e.step(e.sample_actions(5, t))
        assert not e.obs.is_contiguous() and tuple(e.obs.shape) == (N, K, 15)
        return e, e.obs
    g = torch.Generator().manual_seed(11)
    shape = (N, 15) if kind == "frames" else (N, K, 15)
    return None, (torch.randn(shape, generator=g) * 1000).cuda()


def _refused(torch, call, bad):
    from f16_jsb_amd._lib import lib
    before, err = bad.clone(), lib().f16env_last_error()
    with pytest.raises(ValueError, match="out must be a contiguous"):
        call(bad)
    torch.cuda.synchronize()
    assert torch.equal(bad, before) and lib().f16env_last_error() == err


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["contiguous", "window"])
def test_features_out_is_checked(gpu, kind):
    import torch
    from f16_jsb_amd.features import features
    e, obs = _obs(torch, kind)
    want = features(obs)
    assert tuple(want.shape) == (N, K, 17)
    full = lambda shape, **kw: torch.full(shape, 7.0, **kw)  # noqa: E731
    for bad in (full((N, K, 17), dtype=torch.float32), full((N, K, 17), dtype=torch.float16, device=gpu),
                full((N, K, 16), dtype=torch.float32, device=gpu), full((N * K, 17), dtype=torch.float32, device=gpu),
                full((N, K, 34), dtype=torch.float32, device=gpu)[..., ::2]):
        _refused(torch, lambda out: features(obs, out=out), bad)
    out = full((N, K, 17), dtype=torch.float32, device=gpu)
    assert features(obs, out=out) is out and torch.equal(out, want)
    if e is not None:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["frames", "contiguous", "window"])
def test_poses_out_is_checked(gpu, kind):
    import torch
    from f16_jsb_amd.telemetry import poses
    e, obs = _obs(torch, kind)
    want = poses(obs)
    assert tuple(want.shape) == (N, 10)
    full = lambda shape, **kw: torch.full(shape, 7.0, **kw)  # noqa: E731
    for bad in (full((N, 10), dtype=torch.float32), full((N, 10), dtype=torch.float16, device=gpu),
                full((N, 4), dtype=torch.float32, device=gpu), full((N + 1, 10), dtype=torch.float32, device=gpu),
                full((N, 20), dtype=torch.float32, device=gpu)[:, ::2]):
        _refused(torch, lambda out: poses(obs, out=out), bad)
    out = full((N, 10), dtype=torch.float32, device=gpu)
    assert poses(obs, out=out) is out and torch.equal(out, want)
    if e is not None:
        e.close()
