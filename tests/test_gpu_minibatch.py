"""The device minibatch sampler (f16env_rollout_minibatch, DeviceRolloutBuffer.get, minibatches)
against tests/minibatch_ref.py's restatement of SB3's RolloutBuffer.get over the materialised
observations: every comparison is torch.equal on int32 views, i.e. bits."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import minibatch_ref

pytestmark = pytest.mark.gpu

T, N = 7, 5
KS = (1, 2, 4, 10)  # 10 > T: most stacks reach deep into obs0
VARIANTS = {"w1_planted": (1, True), "w1_random": (1, False), "w3": (3, True)}
BATCH_SIZES = (1, 63, 64, 65, 257, None)
QNAN = 0x7FC00000
SPECIALS = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7FA00000,   # quiet NaNs with payloads, a signalling one
                     0x7F800000, 0xFF800000, 0x80000000, 0x00000001], np.uint32).view(np.float32)  # +-inf, -0, denormal


def _planted_starts(k):
    """(T, N) starts, one planted case per column: none at all; one at t = 0; two on consecutive
    steps; a single one at step 1, which the full permutation samples from exactly K-1 and exactly
    K-2 steps later (where those steps exist); one at T-1."""
    s = np.zeros((T, N), np.float32)
    s[0, 1] = 1
    s[2, 2] = s[3, 2] = 1
    s[1, 3] = 1
    s[T - 1, 4] = 1
    return s


def _synthetic(gpu, k, world, planted, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    sd = {"frames": f(world, T, N, 15), "obs0": f(world, N, k, 15), "actions": f(world, T, N, 4),
          "rewards": f(world, T, N), "values": f(world, T, N), "log_probs": f(world, T, N),
          "advantages": f(world, T, N), "returns": f(world, T, N),
          "episode_starts": (rng.random((world, T, N)) < 0.3).astype(np.float32)}
    if planted:
        sd["episode_starts"][0] = _planted_starts(k)
    for name in ("frames", "obs0", "actions", "values"):  # special bit patterns, a tenth of the entries
        flat = sd[name].reshape(-1)
        where = rng.choice(flat.size, max(1, flat.size // 10), replace=False)
        flat[where] = SPECIALS[rng.integers(0, len(SPECIALS), where.size)]
    sd = {n: torch.from_numpy(x).to(gpu) for n, x in sd.items()}
    return sd


@pytest.fixture(scope="module")
def sources(gpu):
    """Per (variant, K): the source handed to the sampler, its flattened reference arrays
    (computed once, never modified) and its number of transitions."""
    from f16_jsb_amd.rollout import DeviceRolloutBuffer
    out = {}
    for vi, (name, (world, planted)) in enumerate(VARIANTS.items()):
        for k in KS:
            sd = _synthetic(gpu, k, world, planted, 1000 * vi + k)
            if world == 1:  # a local buffer, filled field by field
                src = DeviceRolloutBuffer(T, N, k, gpu)
                for f, x in sd.items():
                    getattr(src, f).copy_(x[0])
                src.pos = T
            else:           # gather_to_rank0's rank-major dict
                src = sd
            flat = minibatch_ref.flat_fields(src, k)
            for a in flat.values():
                a.setflags(write=False)
            out[(name, k)] = (src, flat, world * T * N)
    return out


def _get(src, k, **kw):
    from f16_jsb_amd.rollout import minibatches
    return src.get(**kw) if hasattr(src, "get") and not isinstance(src, dict) else minibatches(src, k, **kw)


def test_planted_columns_are_what_they_claim(sources):
    """The checker's own stacks on the planted columns (K = 4): a start K-1 steps back leaves the
    stack untouched, one K-2 steps back repeats the start frame once; no start reads obs0."""
    src, flat, _ = sources[("w1_planted", 4)]
    obs = flat["observations"].reshape(N, T, 4, 15).view(np.int32)
    fr, o0 = src.frames.cpu().numpy().view(np.int32), src.obs0.cpu().numpy().view(np.int32)
    assert np.array_equal(obs[0, 1], np.stack([o0[0, 1], o0[0, 2], fr[0, 0], fr[1, 0]]))      # no start: obs0
    assert np.array_equal(obs[1, 2], np.stack([fr[0, 1], fr[0, 1], fr[1, 1], fr[2, 1]]))      # start at 0
    assert np.array_equal(obs[2, 4], np.stack([fr[3, 2], fr[3, 2], fr[3, 2], fr[4, 2]]))      # consecutive: the later one
    assert np.array_equal(obs[3, 4], np.stack([fr[1, 3], fr[2, 3], fr[3, 3], fr[4, 3]]))      # exactly K-1 back
    assert np.array_equal(obs[3, 3], np.stack([fr[1, 3], fr[1, 3], fr[2, 3], fr[3, 3]]))      # exactly K-2 back
    assert np.array_equal(obs[4, 6], np.stack([fr[6, 4]] * 4))                                # start at T-1


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_epochs_equal_the_checker(sources, variant, k):
    """A full permutation at every batch size: each minibatch equals buffers.py:481-521 on the
    materialised arrays; the epoch covers every index once; the last minibatch is short."""
    src, flat, total = sources[(variant, k)]
    for bi, bs in enumerate(BATCH_SIZES):
        perm = np.random.default_rng(7 * k + bi).permutation(total)
        forms = (perm, torch.from_numpy(perm), torch.from_numpy(perm).to(src["frames"].device if isinstance(src, dict)
                                                                            else src.device))
        got = list(_get(src, k, batch_size=bs, indices=forms[bi % 3]))
        want = list(minibatch_ref.get(flat, perm, bs))
        step = total if bs is None else bs
        assert len(got) == len(want) == -(-total // step)
        sizes = [g.observations.shape[0] for g in got]
        assert sum(sizes) == total and all(s == step for s in sizes[:-1])
        assert sizes[-1] == (total % step or min(step, total))  # the short last minibatch, as it is
        for j, (g, w) in enumerate(zip(got, want)):
            assert g.observations.shape == (sizes[j], k, 15) and g.actions.shape == (sizes[j], 4)
            minibatch_ref.assert_same_bits(g, w, "%s K=%d batch_size=%s minibatch %d" % (variant, k, bs, j))
        # each yield is fresh storage
        ptrs = [x.data_ptr() for g in got for x in g if x.numel()]
        assert len(set(ptrs)) == len(ptrs)


@pytest.mark.parametrize("variant", ["w1_random", "w3"])
def test_device_permutation_covers_every_index_once(gpu, sources, variant):
    """No caller indices: torch.randperm on the device. The values field carries each
    transition's own flat index, so the epoch's old_values are the permutation that was drawn."""
    from f16_jsb_amd.rollout import flat_index
    k = 4
    src, _, total = sources[(variant, k)]
    sd = dict(src.state_dict() if hasattr(src, "state_dict") else src)
    W = total // (T * N)
    w, t, n = torch.meshgrid(torch.arange(W), torch.arange(T), torch.arange(N), indexing="ij")
    ids = flat_index(t, w * N + n, T).to(torch.float32).to(gpu)
    sd["values"] = ids if sd["frames"].dim() == 4 else ids[0]
    flat = minibatch_ref.flat_fields(sd, k)
    assert np.array_equal(flat["values"][:, 0], np.arange(total, dtype=np.float32))
    from f16_jsb_amd.rollout import minibatches
    epochs = []
    for seed in (3, 3, 4):
        gen = torch.Generator(device=gpu).manual_seed(seed)
        got = list(minibatches(sd, k, batch_size=64, generator=gen))
        drawn = torch.cat([g.old_values for g in got]).cpu().numpy().astype(np.int64)
        assert np.array_equal(np.sort(drawn), np.arange(total))  # every index exactly once
        assert got[-1].old_values.numel() == (total % 64 or 64)
        for g, w_ in zip(got, minibatch_ref.get(flat, drawn, 64)):
            minibatch_ref.assert_same_bits(g, w_, variant)
        epochs.append(drawn)
    assert np.array_equal(epochs[0], epochs[1]) and not np.array_equal(epochs[0], epochs[2])
    assert not np.array_equal(epochs[0], np.arange(total))


@pytest.mark.parametrize("variant", ["w1_planted", "w3"])
def test_out_of_range_indices_read_nothing(gpu, sources, variant):
    """-1, W*N*T, 2^40 and the int64 extremes among valid indices, across a block boundary: those
    rows are quiet NaN in all six outputs, every other row keeps its bits."""
    from f16_jsb_amd.rollout import rollout_minibatch
    k = 4
    src, flat, total = sources[(variant, k)]
    rng = np.random.default_rng(5)
    idx = rng.integers(0, total, 131)
    bad = {0: -1, 5: total, 63: 2 ** 40, 64: -(2 ** 63), 65: 2 ** 63 - 1, 100: total + 7, 130: -total}
    for pos, v in bad.items():
        idx[pos] = v
    got = rollout_minibatch(src, torch.from_numpy(idx).to(gpu), k)
    good = np.array([p not in bad for p in range(idx.size)])
    want = minibatch_ref.get_samples(flat, np.where(good, idx, 0))
    for name, g, w in zip(minibatch_ref.NAMES, got, want):
        gi = g.view(torch.int32).cpu().numpy()
        assert np.array_equal(gi[good], minibatch_ref.bits(w)[good]), name
        assert np.all(gi[~good] == QNAN), name
        assert torch.isnan(g[torch.from_numpy(~good).to(gpu)]).all()
    # all of a batch out of range, and a batch of one
    got = rollout_minibatch(src, torch.full((3,), total, dtype=torch.int64, device=gpu), k)
    assert all(bool(torch.all(x.view(torch.int32) == QNAN)) for x in got)


def test_caller_storage_side_stream_and_graph_replay(gpu, sources):
    from f16_jsb_amd.rollout import RolloutSamples, _View, rollout_minibatch
    k = 4
    src, flat, total = sources[("w3", k)]
    B = 50  # of 105 transitions
    e = lambda *s: torch.full(s, -7.0, device=gpu)  # noqa: E731
    out = RolloutSamples(e(B, k, 15), e(B, 4), e(B), e(B), e(B), e(B))
    perm = np.random.default_rng(1).permutation(total)
    idx = torch.from_numpy(perm[:B]).to(gpu)
    # caller-owned storage: the same tensors come back, written in place
    back = rollout_minibatch(src, idx, k, out=out)
    assert all(a is b for a, b in zip(back, out))
    minibatch_ref.assert_same_bits(out, minibatch_ref.get_samples(flat, perm[:B]), "out=")
    for bad in (out._replace(actions=e(B, 5)), out._replace(returns=e(B + 1)), out._replace(observations=e(B, k, 15).cpu()),
                out._replace(old_values=e(B).double()), out._replace(observations=e(B, 15, k).transpose(1, 2))):
        with pytest.raises(ValueError):
            rollout_minibatch(src, idx, k, out=bad)
    with pytest.raises(ValueError):
        rollout_minibatch(src, idx.cpu(), k)
    with pytest.raises(ValueError):
        rollout_minibatch(src, idx.to(torch.int32), k)
    with pytest.raises(ValueError):  # a non-contiguous source field
        rollout_minibatch(dict(src, values=src["values"].transpose(1, 2)), idx, k)
    # a side stream
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    idx2 = torch.from_numpy(perm[B:2 * B]).to(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = rollout_minibatch(src, idx2, k)
    side.synchronize()
    minibatch_ref.assert_same_bits(got, minibatch_ref.get_samples(flat, perm[B:2 * B]), "side stream")
    # one launch captured in a graph; replayed after the index tensor's contents change
    view = _View(src, k)
    static_idx = idx.clone()
    with torch.cuda.stream(side):
        rollout_minibatch(view, static_idx, out=out)  # warm-up outside the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rollout_minibatch(view, static_idx, out=out)
    for lo in (total - B, 0):
        static_idx.copy_(torch.from_numpy(perm[lo:lo + B]))
        g.replay()
        torch.cuda.synchronize()
        fresh = rollout_minibatch(src, static_idx.clone(), k)
        minibatch_ref.assert_same_bits(out, fresh, "graph replay")
        minibatch_ref.assert_same_bits(out, minibatch_ref.get_samples(flat, perm[lo:lo + B]), "graph replay vs checker")


@pytest.mark.parametrize("layout", ["window", "contiguous"])
def test_real_rollout_equals_the_checker(gpu, layout):
    """130 envs under TimeLimit 5 for 12 steps (every lane auto-resets at least twice), a
    DevicePolicy in the loop, GAE, then get(64) in numpy's permutation order."""
    import bench
    from f16_jsb_amd.env import F16Envs
    from f16_jsb_amd.policy import DevicePolicy
    from f16_jsb_amd.rollout import DeviceRolloutBuffer, collect_rollout
    n, k, steps = 130, 4, 12
    net = bench.MlpActorCritic(k * 15, "cpu", seed=2)
    dev = lambda layers: [(w.to(gpu), b.to(gpu)) for w, b in layers]  # noqa: E731
    pol = DevicePolicy.from_layers(dev(net.pi), dev(net.vf), dev([net.act_w])[0], dev([net.val_w])[0],
                                   torch.ones(4, device=gpu), stack_k=k, seed=21)
    envs = F16Envs(n, stack_k=k, device=gpu, seed=5, obs_layout=layout, max_steps=5)
    envs.reset()
    buf = DeviceRolloutBuffer(steps, n, k, gpu)
    last_v, last_d = collect_rollout(envs, buf, 21, 1000, policy_fn=pol)
    buf.compute_returns_and_advantage(last_v, last_d)
    envs.close()
    assert buf.full and buf.episode_starts[1:].sum(0).min() >= 2  # resets inside the rollout, every lane
    assert buf.values.abs().sum() > 0 and buf.log_probs.abs().sum() > 0 and buf.advantages.abs().sum() > 0
    flat = minibatch_ref.flat_fields(buf, k)
    perm = np.random.default_rng(0).permutation(steps * n)
    got = list(buf.get(64, indices=perm))
    want = list(minibatch_ref.get(flat, perm, 64))
    assert len(got) == len(want) == 25 and got[-1].returns.numel() == 1560 % 64
    for j, (g, w) in enumerate(zip(got, want)):
        minibatch_ref.assert_same_bits(g, w, "%s minibatch %d" % (layout, j))


def test_epoch_memory_stays_far_below_the_materialised_grid(gpu):
    """T = 64, N = 256, K = 10: the stacked observations alone would be 9.8 MB. A whole
    get(1024) epoch may raise the peak by the permutation (8 B per transition), three
    minibatches and 64 KiB: about 2.5 MB, so a sampler that rebuilds the grid fails."""
    from f16_jsb_amd.rollout import DeviceRolloutBuffer
    steps, n, k, bs = 64, 256, 10, 1024
    buf = DeviceRolloutBuffer(steps, n, k, gpu)
    g = torch.Generator(device=gpu).manual_seed(1)
    for f in ("frames", "obs0", "actions", "values", "log_probs", "advantages", "returns"):
        getattr(buf, f).normal_(generator=g)
    buf.episode_starts.copy_((torch.rand(steps, n, device=gpu, generator=g) < 0.1).float())
    buf.pos = steps
    minibatch_bytes = bs * (k * 15 + 4 + 4) * 4
    bound = 8 * steps * n + 3 * minibatch_bytes + 64 * 1024
    assert steps * n * k * 15 * 4 == 9830400 and bound < 2.6e6
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    base = torch.cuda.memory_allocated(gpu)
    count, seen = 0, 0.0
    for mb in buf.get(bs, generator=g):
        count += 1
        seen += float(mb.observations.shape[0])
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(gpu) - base
    print("epoch peak rise %d B, bound %d B" % (rise, bound))
    assert count == steps * n // bs and seen == steps * n
    assert rise <= bound, (rise, bound)
