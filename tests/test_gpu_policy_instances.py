"""GPU checks of every instance of the device policy kernel (f16_policy_forward_kernel<D, WLDS>),
every tile count and the edge inputs: the architecture matrix of tests/policy_ref.py on exact
integer data and on tanh nets against fp64, the kernel's tanh alone through a one-hot probe net,
non-finite rows, in-place reads of the feature window and of broadcast views, the high word of
the Philox counter, and graphs / streams on the instance that reads its weights from L2 (with a
replay after DevicePolicy.load)."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import policy_ref
from test_gpu_policy_forward import _int_forward, _int_net  # noqa: E402

pytestmark = pytest.mark.gpu

MATRIX = policy_ref.MATRIX
LOG_STD = np.array([-0.5, 0.0, 0.25, 0.5], np.float32)
N_TANH = 257


def _reaches(name):
    """The case's descriptor and, asserted, the kernel instance DESIGN section 4's rule gives it."""
    k, d, pi_w, vf_w, inst = MATRIX[name]
    assert policy_ref.kernel_instance(k, d, pi_w, vf_w) == inst, name
    return k, d, pi_w, vf_w


def _policy(net, gpu, k, d, activation="tanh", **kw):
    from f16_jsb_amd.policy import DevicePolicy
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=gpu)  # noqa: E731
    pair = lambda wb: (t(wb[0]), t(wb[1]))  # noqa: E731
    return DevicePolicy.from_layers([pair(l) for l in net["pi"]], [pair(l) for l in net["vf"]], pair(net["act"]),
                                    pair(net["val"]), t(net["log_std"]), stack_k=k, frame_dim=d,
                                    activation=activation, **kw)


def _load_args(net, gpu):
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=gpu)  # noqa: E731
    pair = lambda wb: (t(wb[0]), t(wb[1]))  # noqa: E731
    return ([pair(l) for l in net["pi"]], [pair(l) for l in net["vf"]], pair(net["act"]), pair(net["val"]),
            t(net["log_std"]))


# ---------------------------------------------------------------------------------------------
# (a) exact integer layout over the matrix
@pytest.mark.parametrize("n", [1, 129, 257])
@pytest.mark.parametrize("name", list(MATRIX))
def test_exact_integer_layout_over_the_matrix(gpu, name, n):
    """test_exact_integer_layout's method on every matrix case: integer weights and inputs, ReLU,
    eps = 0, every sum exact in float32, bit equality with the integer reference. n = 129 leaves
    one row alone in a second block, n = 257 a last wave with one live row."""
    k, d, pi_w, vf_w = _reaches(name)
    rng = np.random.default_rng(7000 + 100 * ord(name) + n)
    pi, vf, act, val = _int_net(rng, k * d, pi_w, vf_w)
    x = rng.integers(-2, 3, (n, k, d)).astype(np.int64)
    mean, b1 = _int_forward(x.reshape(n, -1), pi, act)
    value, b2 = _int_forward(x.reshape(n, -1), vf, val)
    assert max(b1, b2) < 2 ** 24, "test data: a sum may not be exact in float32"
    assert np.abs(mean).max() > 0 and np.abs(value).max() > 0 and len(np.unique(mean)) >= min(4, n)
    net = {"pi": pi, "vf": vf, "act": act, "val": val, "log_std": np.zeros(4)}
    pol = _policy(net, gpu, k, d, "relu")
    a, v, lp = pol(torch.as_tensor(x.astype(np.float32), device=gpu), eps=torch.zeros((n, 4), device=gpu))
    assert np.array_equal(a.cpu().numpy(), mean.astype(np.float32))
    assert np.array_equal(v.cpu().numpy(), value[:, 0].astype(np.float32))
    assert np.abs(lp.cpu().numpy() - 4 * -0.9189385332046727).max() < 1e-6  # eps = 0, log_std = 0


# ---------------------------------------------------------------------------------------------
# (b) tanh nets against fp64 over the matrix
@functools.lru_cache(maxsize=None)
def _dense_case(name, variant=0):
    """Case `name` with dense random float32 weights N(0, 2 / fan_in), biases N(0, 0.01), 257
    standard-normal observations and a fixed standard-normal eps: made once, shared, not changed."""
    k, d, pi_w, vf_w, _ = MATRIX[name]
    rng = np.random.default_rng(31000 + 100 * ord(name) + variant)

    def lin(o, i):
        return ((rng.standard_normal((o, i)) * math.sqrt(2.0 / i)).astype(np.float32),
                (rng.standard_normal(o) * 0.1).astype(np.float32))

    def branch(widths):
        out, fan_in = [], k * d
        for w in widths:
            out.append(lin(w, fan_in))
            fan_in = w
        return out
    net = {"pi": branch(pi_w), "vf": branch(vf_w), "act": lin(4, pi_w[-1]), "val": lin(1, vf_w[-1]), "log_std": LOG_STD}
    net["x"] = rng.standard_normal((N_TANH, k, d)).astype(np.float32)
    net["eps"] = rng.standard_normal((N_TANH, 4)).astype(np.float32)
    return net


def _ref64(net, x, eps, activation="tanh"):
    with np.errstate(invalid="ignore"):
        return policy_ref.forward(x, net["pi"], net["vf"], net["act"], net["val"], net["log_std"], eps, activation)[:3]


def _torch32(net, x, eps, activation="tanh"):
    """The same net in torch CPU float32 (the yardstick of the 4 x rule)."""
    act = torch.tanh if activation == "tanh" else torch.relu
    lin = lambda h, wb: torch.nn.functional.linear(h, torch.from_numpy(wb[0]), torch.from_numpy(wb[1]))  # noqa: E731

    def mlp(layers):
        h = torch.from_numpy(np.ascontiguousarray(x)).reshape(len(x), -1)
        for wb in layers:
            h = act(lin(h, wb))
        return h
    e, ls = torch.from_numpy(eps), torch.from_numpy(net["log_std"])
    return ((lin(mlp(net["pi"]), net["act"]) + ls.exp() * e).numpy(), lin(mlp(net["vf"]), net["val"])[:, 0].numpy(),
            (-0.5 * e * e - ls - 0.5 * math.log(2 * math.pi)).sum(-1).numpy())


def _beyond_4x_torch(label, got, t32, ref, rows=None, kinds=("actions", "values", "log_probs")):
    """The project's precision rule (test_tanh_net_error_against_fp64_within_4x_torch): per output
    kind the kernel's max abs error against fp64 is at most 4 x that of torch CPU float32, with
    2^-24 max|reference| as the floor of torch's figure. Prints the figures; returns the misses."""
    bad = []
    for name, g, tt, r in zip(("actions", "values", "log_probs"), got, t32, ref):
        if name not in kinds:
            continue
        g, tt = np.asarray(g, np.float64), np.asarray(tt, np.float64)
        if rows is not None:
            g, tt, r = g[rows], tt[rows], r[rows]
        e_k, e_t = np.abs(g - r).max(), np.abs(tt - r).max()
        floor = 2.0 ** -24 * np.abs(r).max()
        print("%s %s: kernel %.3e torch %.3e floor %.3e ratio %.2f" % (label, name, e_k, e_t, floor, e_k / max(e_t, floor)))
        if not (np.all(np.isfinite(g)) and e_k <= 4.0 * max(e_t, floor)):
            bad.append((name, e_k, e_t, floor))
    return bad


def _cpu(out):
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("name", list(MATRIX))
def test_tanh_net_against_fp64_over_the_matrix(gpu, name):
    """Every instance and tile count with tanh, dense weights and inputs in tanh's curved range.
    Measured on an MI355X (kernel / torch per case): DESIGN.md section 4."""
    k, d, pi_w, vf_w = _reaches(name)
    net = _dense_case(name)
    out = _policy(net, gpu, k, d)(torch.from_numpy(net["x"]).to(gpu), eps=torch.from_numpy(net["eps"]).to(gpu))
    bad = _beyond_4x_torch("case " + name, _cpu(out), _torch32(net, net["x"], net["eps"]), _ref64(net, net["x"], net["eps"]))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# (c) the kernel's tanh alone
PROBE_K, PROBE_D = 1, 15


def _probe_net(dense_first_layer=False):
    """K = 1, D = 15, [32] / [32], biases 0: pi unit c reads input c (c < 4), vf unit 0 reads input
    4, all with weight 1.0; action c = pi unit c, value = vf unit 0. Every product is exact, so a
    deterministic forward returns the kernel's tanh of inputs 0..4. dense_first_layer: every
    hidden unit reads every input with weight 1.0 instead (each output = tanh(sum of the row))."""
    w_pi, w_vf = np.zeros((32, PROBE_D), np.float32), np.zeros((32, PROBE_D), np.float32)
    w_pi[np.arange(4), np.arange(4)] = 1.0
    w_vf[0, 4] = 1.0
    if dense_first_layer:
        w_pi[:], w_vf[:] = 1.0, 1.0
    act, val = np.zeros((4, 32), np.float32), np.zeros((1, 32), np.float32)
    act[np.arange(4), np.arange(4)] = 1.0
    val[0, 0] = 1.0
    z = lambda n: np.zeros(n, np.float32)  # noqa: E731
    return {"pi": [(w_pi, z(32))], "vf": [(w_vf, z(32))], "act": (act, z(4)), "val": (val, z(1)), "log_std": z(4)}


def _probe(pol, rows, gpu):
    """(n, 5): the four action means and the value of each row."""
    a, v, _ = pol(torch.from_numpy(rows).to(gpu), deterministic=True)
    return np.concatenate([a.cpu().numpy(), v.cpu().numpy()[:, None]], 1)


def test_policy_tanh_error_symmetry_and_range(gpu):
    """policy_tanh on 20 480 inputs (|v| log-spaced over 1e-30 .. 150, and 0, 1e-40, 88, 1e30, in
    both signs): within 2^-22 of tanh in fp64, odd bit for bit, never beyond 1.
    The bound: sign(v) (1 - t) / (1 + t), t = exp(-2|v|), evaluated in float32 with a correctly
    rounded exp2 and reciprocal errs by 1.25e-7 at most, by 1.92e-7 with either an ulp off (the
    hardware's stated accuracy); 2^-22 = 2.38e-7 is the next power of two.
    Measured on an MI355X: DESIGN.md section 4."""
    mags = np.concatenate([np.logspace(-30, math.log10(150.0), 10236), [0.0, 1e-40, 88.0, 1e30]]).astype(np.float32)
    v = np.concatenate([mags, -mags])
    rows = np.zeros((len(v) // 5, PROBE_K, PROBE_D), np.float32)
    rows[:, 0, :5] = v.reshape(-1, 5)
    assert len(rows) == 4096 and np.all(np.isfinite(v)) and np.all(np.signbit(v[len(mags):]))
    got = _probe(_policy(_probe_net(), gpu, PROBE_K, PROBE_D), rows, gpu).reshape(-1)
    err = np.abs(got.astype(np.float64) - np.tanh(v.astype(np.float64)))
    worst = int(err.argmax())
    print("policy_tanh: max abs error %.3e at v = %.9g (2^-22 = %.3e)" % (err[worst], v[worst], 2.0 ** -22))
    assert np.all(np.isfinite(got)) and np.abs(got).max() <= 1.0
    assert err.max() <= 2.0 ** -22
    # tanh(-v) = -tanh(v) bit for bit. The head returns 0 + 1.0 * tanh, which turns a -0 into +0:
    # the expected bits are those of that sum, so a zero result is +0 on both sides.
    pos, neg = got[:len(mags)], got[len(mags):]
    assert np.array_equal(neg.view(np.uint32), (np.float32(0.0) + -pos).view(np.uint32))
    assert np.all(pos >= 0) and pos[-1] == 1.0 and pos[-2] == 1.0 and np.all(pos[mags > 2.0 ** -21] > 0)


def test_policy_tanh_non_finite(gpu):
    """+-inf gives exactly +-1 and NaN passes. In the one-hot probe net a non-finite input also
    meets the zero weights of every other unit of both branches (0 * inf = NaN), which the
    one-hot heads then sum (0 * NaN), so every output of such a row is NaN in kernel and fp64
    reference alike: that pattern is asserted against the reference. The exact +-1 is asserted
    on the net whose hidden units all read every input with weight 1.0 (each output =
    tanh(sum of the row), the sum being the row's one non-zero input)."""
    specials = np.array([np.inf, -np.inf, np.nan, 3.0, -0.5], np.float32)
    rows = np.zeros((5 * len(specials), PROBE_K, PROBE_D), np.float32)
    for i in range(5):  # special s at probed input i, the other inputs zero
        rows[i * len(specials):(i + 1) * len(specials), 0, i] = specials
    one_hot = _probe_net()
    got = _probe(_policy(one_hot, gpu, PROBE_K, PROBE_D), rows, gpu)
    a, v, _ = _ref64(one_hot, rows, np.zeros((len(rows), 4)))
    ref = np.concatenate([a, v[:, None]], 1)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    fin = ~np.isnan(ref)
    assert np.abs(got[fin] - ref[fin]).max() <= 2.0 ** -22
    for i in range(5):  # a non-finite input leaves no output of its row finite; the finite rows are untouched
        r = ref[i * len(specials):(i + 1) * len(specials)]
        assert np.all(np.isnan(r[:3])) and np.all(np.isfinite(r[3:])) and abs(r[3, i]) > 0.99 and np.all(np.delete(r[3], i) == 0)

    dense = _probe_net(dense_first_layer=True)
    got = _probe(_policy(dense, gpu, PROBE_K, PROBE_D), rows, gpu)
    want = np.tanh(specials.astype(np.float64))
    for i in range(5):
        r = got[i * len(specials):(i + 1) * len(specials)]
        assert np.all(r[0] == 1.0) and np.all(r[1] == -1.0) and np.all(np.isnan(r[2]))
        assert np.abs(r[3:] - want[3:, None]).max() <= 2.0 ** -22


# ---------------------------------------------------------------------------------------------
# (d) non-finite rows in a dense net
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_non_finite_rows_stay_in_their_rows(gpu, activation):
    """Case E's dense net, n = 130: a NaN in row 5 (frame 2), +inf in row 40, -inf in row 129
    (alone in its block). Every other row keeps its bits; row 5's means and value are NaN under
    both activations (a ReLU compiled to a max would return a finite row); rows 40 and 129 have
    the fp64 reference's NaN pattern, and under tanh -- the dense first layer saturates to +-1 --
    finite outputs within the 4 x torch rule."""
    k, d, pi_w, vf_w = _reaches("E")
    net, n = _dense_case("E"), 130
    clean, eps = net["x"][:n].copy(), net["eps"][:n]
    dirty = clean.copy()
    dirty[5, 2, 7], dirty[40, 1, 3], dirty[129, 3, 14] = np.nan, np.inf, -np.inf
    touched = np.array([5, 40, 129])
    others = np.setdiff1d(np.arange(n), touched)
    pol = _policy(net, gpu, k, d, activation)
    e = torch.from_numpy(eps).to(gpu)
    out_c, out_d = _cpu(pol(torch.from_numpy(clean).to(gpu), eps=e)), _cpu(pol(torch.from_numpy(dirty).to(gpu), eps=e))
    assert all(np.all(np.isfinite(o)) for o in out_c)
    for c, g in zip(out_c, out_d):
        assert np.array_equal(c[others].view(np.uint32), g[others].view(np.uint32))
    assert np.array_equal(out_c[2].view(np.uint32), out_d[2].view(np.uint32))  # log-probs do not read obs
    assert np.all(np.isnan(out_d[0][5])) and np.isnan(out_d[1][5])
    ref = _ref64(net, dirty, eps, activation)
    assert np.all(np.isnan(ref[0][5])) and np.isnan(ref[1][5])
    for g, r in zip(out_d[:2], ref[:2]):
        assert np.array_equal(np.isnan(g[[40, 129]]), np.isnan(r[[40, 129]]))
        inf = np.isinf(r[[40, 129]])
        assert np.array_equal(g[[40, 129]][inf], r[[40, 129]][inf])
    if activation == "tanh":
        assert all(np.all(np.isfinite(r[[40, 129]])) for r in ref)
        bad = _beyond_4x_torch("tanh rows 40, 129", out_d, _torch32(net, dirty, eps), ref, rows=[40, 129],
                               kinds=("actions", "values"))
        assert not bad, bad
    else:
        print("relu rows 40, 129: NaN pattern", np.isnan(ref[0][[40, 129]]).tolist(), np.isnan(ref[1][[40, 129]]).tolist())


# ---------------------------------------------------------------------------------------------
# (e) reading in place
def test_feature_window_read_in_place(gpu):
    """Case G on the (n, K, 17) feature window of a stepped fused-features F16Envs: the view (not
    contiguous) gives the bits of its contiguous copy, within the 4 x torch rule of fp64."""
    from f16_jsb_amd.env import F16Envs
    k, d, pi_w, vf_w = _reaches("G")
    net = _dense_case("G")
    envs = F16Envs(N_TANH, stack_k=k, device=gpu, seed=3, obs_layout="window", fused_features=True)
    try:
        envs.reset()
        for t in range(6):
            envs.step(envs.sample_actions(9, t))
        feat = envs.obs_features()
        assert tuple(feat.shape) == (N_TANH, k, d) and not feat.is_contiguous() and feat.stride(2) == 1
        copy = feat.contiguous()
        pol, eps = _policy(net, gpu, k, d), torch.from_numpy(net["eps"]).to(gpu)
        a, b = pol(feat, eps=eps), pol(copy, eps=eps)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert torch.equal(pol.value(feat), b[1])
        x = copy.cpu().numpy()
        assert np.all(np.isfinite(x)) and np.abs(x).max() > 0.5
        bad = _beyond_4x_torch("feature window", _cpu(a), _torch32(net, x, net["eps"]), _ref64(net, x, net["eps"]))
        assert not bad, bad
    finally:
        envs.close()


def test_broadcast_strides_and_empty_batch(gpu):
    """Row stride 0 and frame stride 0 (f16env_policy_forward accepts both): a row-broadcast view
    gives every row the bits of row 0, a frame-broadcast view those of its materialised copy.
    n = 0 returns three empty tensors (a launch of zero blocks would be refused by the runtime)."""
    k, d, pi_w, vf_w = _reaches("G")
    net = _dense_case("G")
    pol = _policy(net, gpu, k, d)
    x = torch.from_numpy(net["x"]).to(gpu)
    eps = torch.from_numpy(net["eps"]).to(gpu)
    full = pol(x, eps=eps)
    rows = x[:1].expand(N_TANH, k, d)
    assert rows.stride(0) == 0
    out = pol(rows, eps=eps[:1].expand(N_TANH, 4).contiguous())
    for o, f in zip(out, full):
        assert torch.equal(o, f[:1].expand_as(o))
    assert torch.equal(pol.value(rows), full[1][:1].expand(N_TANH))
    frames = x[:, :1].expand(N_TANH, k, d)
    assert frames.stride(1) == 0 and frames.stride(0) == k * d
    a, b = pol(frames, eps=eps), pol(frames.contiguous(), eps=eps)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and not torch.equal(a[1], full[1])
    assert torch.equal(pol.value(frames), b[1])
    empty = pol(x[:0], eps=eps[:0])
    assert [tuple(o.shape) for o in empty] == [(0, 4), (0,), (0,)]
    assert tuple(pol(x[:0])[0].shape) == (0, 4) and tuple(pol.value(x[:0]).shape) == (0,)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# (f) the Philox counter's high word
def test_philox_counter_high_word(gpu):
    """env_id_base = 2^33 + 5: gid's high word enters the counter (xor 'POLI'). A zero action
    head and log_std make the actions the drawn eps."""
    k, d, pi_w, vf_w = _reaches("A")
    net = dict(_dense_case("A"))
    net["act"] = (np.zeros((4, pi_w[-1]), np.float32), np.zeros(4, np.float32))
    net["log_std"] = np.zeros(4, np.float32)
    x = torch.from_numpy(net["x"]).to(gpu)
    base, seed, step = (1 << 33) + 5, 4321, 11
    hi = _policy(net, gpu, k, d, seed=seed, env_id_base=base)(x, step=step)[0].cpu().numpy()
    lo = _policy(net, gpu, k, d, seed=seed, env_id_base=5)(x, step=step)[0].cpu().numpy()
    want = policy_ref.policy_normals(seed, base + np.arange(N_TANH), step)
    assert np.abs(hi.astype(np.float64) - want).max() < 1e-5
    assert np.abs(lo.astype(np.float64) - policy_ref.policy_normals(seed, 5 + np.arange(N_TANH), step)).max() < 1e-5
    assert not np.array_equal(hi, lo) and np.abs(hi - lo).max() > 1.0


# ---------------------------------------------------------------------------------------------
# (g) graphs and streams on the instance that reads its weights from L2
@pytest.fixture(scope="module")
def frames_k10(gpu):
    """The frame window (n, 10, 15) of a stepped windowed F16Envs, read in place."""
    from f16_jsb_amd.env import F16Envs
    envs = F16Envs(N_TANH, stack_k=10, device=gpu, seed=3, obs_layout="window")
    envs.reset()
    for t in range(6):
        envs.step(envs.sample_actions(9, t))
    obs = envs.obs
    assert tuple(obs.shape) == (N_TANH, 10, 15) and not obs.is_contiguous() and obs.stride(2) == 1
    yield obs
    envs.close()


def test_graph_replay_follows_load(gpu, frames_k10):
    """Case C (<15, false>) on the frame window: a captured forward_into + value replays the eager
    result, and after DevicePolicy.load() of other weights the SAME graph gives what a fresh
    policy built from those weights gives (load() promises captured graphs stay valid)."""
    k, d, pi_w, vf_w = _reaches("C")
    first, second = _dense_case("C"), _dense_case("C", 1)
    obs, n = frames_k10, N_TANH
    pol = _policy(first, gpu, k, d, seed=5)
    eager = pol(obs, step=5)
    outs = (torch.zeros((n, 4), device=gpu), torch.zeros(n, device=gpu), torch.zeros(n, device=gpu))
    vout = torch.zeros(n, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pol.forward_into(obs, 5, *outs)
        pol.value(obs, out=vout)
    for o in outs + (vout,):
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(outs, eager)) and torch.equal(vout, eager[1])
    replay1 = [o.clone() for o in outs]

    blob_ptr = pol.blob.data_ptr()
    pol.load(*_load_args(second, gpu))
    assert pol.blob.data_ptr() == blob_ptr
    for o in outs + (vout,):
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    fresh = _policy(second, gpu, k, d, seed=5)(obs, step=5)
    assert all(torch.equal(x, y) for x, y in zip(outs, fresh)) and torch.equal(vout, fresh[1])
    assert not torch.equal(outs[0], replay1[0]) and not torch.equal(outs[1], replay1[1])
    assert torch.equal(outs[2], replay1[2])  # the log-probs: the same eps, the same log_std


def test_side_stream_equals_default_stream(gpu, frames_k10):
    k, d, pi_w, vf_w = _reaches("C")
    pol = _policy(_dense_case("C"), gpu, k, d, seed=5)
    obs = frames_k10
    want = pol(obs, step=2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        got = pol(obs, step=2)
        v = pol.value(obs)
    side.synchronize()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and torch.equal(v, want[1])
