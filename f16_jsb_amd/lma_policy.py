"""The reference's training policy on the device: the LMA features extractor in front of the two
MLPs, forward only (f16env_policy_lma_forward, include/f16env.h ABI 7).

Every run of the reference's train.py builds its policy with features_extractor_class =
StackedLMAFeaturesExtractor (train.py:21-32; jsbsim_gym/LMA_features.py): the per-frame 15 -> 17
transform, a small latent-attention transformer over the K frames, and the pi / vf MLPs on its
flattened output. `DeviceLMAPolicy` holds those weights as one packed device blob and runs the
whole eval-mode forward (dropout is the identity under set_training_mode(False), which
collect_rollouts and predict run under) as ONE HIP launch. It is a `DevicePolicy`, so
`collect_rollout`'s fast path and the deferred bootstrap take it as `policy_fn` unchanged.

    pol = DeviceLMAPolicy.from_state_dict(model.policy.state_dict(), stack_k=10)
    last_v, last_d = collect_rollout(envs, buf, policy_fn=pol)
    feats = pol.extract_features(envs.obs)          # (n, L_new * 32): what extract_features returns

`DeviceLMAPolicy` is forward only: every gradient entry point refuses by name. The gradient is
opt-in through `DeviceLMATrainPolicy` (f16env_policy_lma_backward): the same blob and forward, and
the EVAL-MODE backward over it -- the reference's gradient at lma_dropout = 0.0, not at the 0.1 it
trains with. DevicePPO refuses both classes until dropout is built.

    pol = DeviceLMATrainPolicy.from_state_dict(sd, stack_k=10).requires_grad_()
    opt = torch.optim.Adam(pol.parameters(), lr=3e-4, eps=1e-5)
    v, log_prob, entropy = pol.evaluate_actions(mb.observations, mb.actions)
    loss = ...; opt.zero_grad(); loss.backward(); clip_grad_norm_(pol.parameters(), 0.5); opt.step()
"""
from __future__ import annotations

import ctypes
import math

import torch

from .abi import (F16_LMA_BLK_ATTN_B, F16_LMA_BLK_ATTN_W, F16_LMA_BLK_FC_B, F16_LMA_BLK_FC_W, F16_LMA_BLK_LN1_B,
                  F16_LMA_BLK_LN1_W, F16_LMA_BLK_LN2_B, F16_LMA_BLK_LN2_W, F16_LMA_BLK_PROJ2_B, F16_LMA_BLK_PROJ2_W,
                  F16_LMA_BLK_PROJ_B, F16_LMA_BLK_PROJ_W, F16_LMA_BLOCK_SLOTS, F16_LMA_OFF_BLOCK0, F16_LMA_OFF_PE,
                  F16_LMA_OFF_W2_B, F16_LMA_OFF_W2_W, F16_LMA_OFF_WE_B, F16_LMA_OFF_WE_W, F16_POLICY_OFF_LOG_STD,
                  F16_POLICY_VALUE_ONLY, LMA_FEATURES, lma_blob_layout, lma_desc, policy_blob_layout, policy_desc)
from .buffers import need_tensor
from .policy import (ACT_DIM, DevicePolicy, _pack_bias, _pack_weight, _unpack_weight, layers_from_state_dict,
                     pack_blob, state_dict_from_layers, unpack_blob)

NO_BACKWARD = ("the LMA backward is not built: DeviceLMAPolicy runs the rollout and predict forward only "
               "(train the extractor in torch, then load_state_dict; or opt in to the eval-mode gradient with "
               "DeviceLMATrainPolicy)")
EXTRACTOR = "features_extractor.lma_extractor."
ALIASES = ("pi_features_extractor.", "vf_features_extractor.")
# block piece -> (its module under lma_blocks.{i}., weight slot, bias slot, is a LayerNorm)
BLOCK_PIECES = (("ln_1", F16_LMA_BLK_LN1_W, F16_LMA_BLK_LN1_B, True),
                ("attn.c_attn", F16_LMA_BLK_ATTN_W, F16_LMA_BLK_ATTN_B, False),
                ("attn.c_proj", F16_LMA_BLK_PROJ_W, F16_LMA_BLK_PROJ_B, False),
                ("ln_2", F16_LMA_BLK_LN2_W, F16_LMA_BLK_LN2_B, True),
                ("mlp.c_fc", F16_LMA_BLK_FC_W, F16_LMA_BLK_FC_B, False),
                ("mlp.c_proj", F16_LMA_BLK_PROJ2_W, F16_LMA_BLK_PROJ2_B, False))


def positional_encoding(stack_k: int, embed_dim: int) -> torch.Tensor:
    """The sinusoidal (K, embed_dim) table the extractor adds to its embedding, in float32 on the
    host, op for op as LMA_features.py:214-218, so the kernel adds the values torch adds."""
    position = torch.arange(stack_k, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, embed_dim, 2).float() * (-math.log(10000.0) / embed_dim))
    pe = torch.zeros(stack_k, embed_dim)
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def _shape_of(m):
    """(in, out) per block piece and for the two embeddings, from the descriptor."""
    return {"embed": (LMA_FEATURES, m.embed_dim), "embed2": (m.C_new, m.d_new), "ln_1": (None, m.d_new),
            "attn.c_attn": (m.d_new, 3 * m.d_new), "attn.c_proj": (m.d_new, m.d_new), "ln_2": (None, m.d_new),
            "mlp.c_fc": (m.d_new, m.ff_hidden), "mlp.c_proj": (m.ff_hidden, m.d_new)}


def extractor_from_state_dict(sd):
    """{"embed": (W, b), "embed2": (W, b), "blocks": [{piece: (W, b)}]} from SB3's key names under
    features_extractor.lma_extractor.*; a missing bias (lma_bias=False) is None. When the
    pi_features_extractor.* / vf_features_extractor.* aliases of a shared extractor are present
    they must hold the same values."""
    shared = {k: v for k, v in sd.items() if k.startswith("features_extractor.")}
    if EXTRACTOR + "initial_transform.input_embedding.weight" not in sd:
        raise KeyError("state dict has no %sinitial_transform.input_embedding.weight" % EXTRACTOR)
    for alias in ALIASES:
        mine = {k[len(alias):]: v for k, v in sd.items() if k.startswith(alias)}
        if not mine:
            continue
        theirs = {k[len("features_extractor."):]: v for k, v in shared.items()}
        if set(mine) != set(theirs):
            raise ValueError("%s* and features_extractor.* name different tensors: a non-shared extractor is not "
                             "built" % alias)
        for k, v in mine.items():
            if v.shape != theirs[k].shape or not torch.equal(torch.as_tensor(v).cpu(), torch.as_tensor(theirs[k]).cpu()):
                raise ValueError("%s%s differs from features_extractor.%s: a non-shared extractor "
                                 "(share_features_extractor=False) is not built" % (alias, k, k))

    def pair(name):
        return sd[EXTRACTOR + name + ".weight"], sd.get(EXTRACTOR + name + ".bias")
    blocks, i = [], 0
    while EXTRACTOR + "lma_blocks.%d.ln_1.weight" % i in sd:
        blocks.append({piece: pair("lma_blocks.%d.%s" % (i, piece)) for piece, *_ in BLOCK_PIECES})
        i += 1
    return {"embed": pair("initial_transform.input_embedding"), "embed2": pair("initial_transform.embed_layer_2"),
            "blocks": blocks}


def state_dict_from_extractor(ext):
    """The extractor under SB3's key names, with the pi_ / vf_ aliases of a shared extractor."""
    flat = {"initial_transform.input_embedding": ext["embed"], "initial_transform.embed_layer_2": ext["embed2"]}
    for i, blk in enumerate(ext["blocks"]):
        for piece, *_ in BLOCK_PIECES:
            flat["lma_blocks.%d.%s" % (i, piece)] = blk[piece]
    sd = {}
    for prefix in ("features_extractor.",) + ALIASES:
        for name, (w, b) in flat.items():
            sd[prefix + "lma_extractor." + name + ".weight"] = w
            sd[prefix + "lma_extractor." + name + ".bias"] = b
    return sd


def pack_lma_blob(desc, lma, ext, pe, pi, vf, act_head, val_head, log_std) -> torch.Tensor:
    """The kernel's blob (f16env_policy_lma_blob_layout): the MLP blob with a first fan-in of
    L_new d_new, then the PE table, W_e, W_2 and the blocks, each weight in the MLP's operand form."""
    off, total = lma_blob_layout(desc, lma)
    shapes = _shape_of(lma)
    f32 = lambda t: torch.as_tensor(t).detach().to(torch.float32)  # noqa: E731
    mlp = pack_blob(desc, pi, vf, act_head, val_head, log_std, fan_in0=lma.L_new * lma.d_new)
    dev = mlp.device
    pieces, pos = [mlp], mlp.numel()

    def put(slot, t):
        nonlocal pos
        if off[slot] != pos:
            raise AssertionError("blob layout: slot %d at %d, packer at %d" % (slot, off[slot], pos))
        pieces.append(t.to(dev))
        pos += t.numel()

    def linear(what, wb, slot_w, slot_b):
        fan_in, out = shapes[what.split("/")[-1]]
        w = f32(wb[0])
        if tuple(w.shape) != (out, fan_in):
            raise ValueError("%s.weight has shape %s where %s was expected" % (what, tuple(w.shape), (out, fan_in)))
        b = torch.zeros(out) if wb[1] is None else f32(wb[1])
        if b.numel() != out:
            raise ValueError("%s.bias holds %d values where %d were expected" % (what, b.numel(), out))
        put(slot_w, _pack_weight(w, fan_in, out))
        put(slot_b, _pack_bias(b, out))

    pe = f32(pe)
    if tuple(pe.shape) != (lma.K, lma.embed_dim):
        raise ValueError("pe has shape %s where %s was expected" % (tuple(pe.shape), (lma.K, lma.embed_dim)))
    put(F16_LMA_OFF_PE, pe.reshape(-1))
    linear("embed", ext["embed"], F16_LMA_OFF_WE_W, F16_LMA_OFF_WE_B)
    linear("embed2", ext["embed2"], F16_LMA_OFF_W2_W, F16_LMA_OFF_W2_B)
    if len(ext["blocks"]) != lma.n_layers:
        raise ValueError("%d blocks given, descriptor has n_layers = %d" % (len(ext["blocks"]), lma.n_layers))
    for i, blk in enumerate(ext["blocks"]):
        s = F16_LMA_OFF_BLOCK0 + F16_LMA_BLOCK_SLOTS * i
        for piece, sw, sb, is_ln in BLOCK_PIECES:
            if not is_ln:
                linear("lma_blocks.%d/%s" % (i, piece), blk[piece], s + sw, s + sb)
                continue
            w, b = f32(blk[piece][0]).reshape(-1), blk[piece][1]
            b = torch.zeros(lma.d_new) if b is None else f32(b).reshape(-1)
            if w.numel() != lma.d_new or b.numel() != lma.d_new:
                raise ValueError("lma_blocks.%d.%s must hold %d values" % (i, piece, lma.d_new))
            put(s + sw, w)
            put(s + sb, b)
    blob = torch.cat(pieces)
    assert blob.numel() == total
    return blob


def unpack_lma_blob(desc, lma, blob):
    """The inverse of pack_lma_blob: (ext, pe, pi, vf, act_head, val_head, log_std); copies."""
    off, total = lma_blob_layout(desc, lma)
    blob = torch.as_tensor(blob).detach()
    if blob.dim() != 1 or blob.numel() != total:
        raise ValueError("a blob of %d floats was expected, got shape %s" % (total, tuple(blob.shape)))
    shapes = _shape_of(lma)
    n_mlp = policy_blob_layout(desc, lma.L_new * lma.d_new)[1]
    mlp = unpack_blob(desc, blob[:n_mlp], fan_in0=lma.L_new * lma.d_new)

    def linear(what, slot_w, slot_b):
        fan_in, out = shapes[what]
        return _unpack_weight(blob, off[slot_w], fan_in, out).clone(), blob[off[slot_b]:off[slot_b] + out].clone()
    pe = blob[off[F16_LMA_OFF_PE]:off[F16_LMA_OFF_PE] + lma.K * lma.embed_dim].reshape(lma.K, lma.embed_dim).clone()
    ext = {"embed": linear("embed", F16_LMA_OFF_WE_W, F16_LMA_OFF_WE_B),
           "embed2": linear("embed2", F16_LMA_OFF_W2_W, F16_LMA_OFF_W2_B), "blocks": []}
    for i in range(lma.n_layers):
        s, blk = F16_LMA_OFF_BLOCK0 + F16_LMA_BLOCK_SLOTS * i, {}
        for piece, sw, sb, is_ln in BLOCK_PIECES:
            if is_ln:
                blk[piece] = (blob[off[s + sw]:off[s + sw] + lma.d_new].clone(), blob[off[s + sb]:off[s + sb] + lma.d_new].clone())
            else:
                blk[piece] = linear(piece, s + sw, s + sb)
        ext["blocks"].append(blk)
    return (ext, pe) + tuple(mlp)


class DeviceLMAPolicy(DevicePolicy):
    """The reference's LMA policy (shared extractor, eval mode) as one HIP launch per forward.
    Inherits forward_into, __call__, value and predict; adds extract_features. Forward only."""

    def __init__(self, desc, lma, device, seed: int = 0, env_id_base: int = 0):
        self.lma, self._lma_ref = lma, ctypes.byref(lma)
        self.features_dim = int(lma.L_new * lma.d_new)
        super().__init__(desc, device, seed, env_id_base)

    # DevicePolicy's hooks: the forward's symbol and its features_out, the second descriptor, the LMA blob
    _FWD, _FWD_MORE = "f16env_policy_lma_forward", 1

    def _desc_args(self):
        return (self._desc_ref, self._lma_ref)

    def _layout(self):
        return lma_blob_layout(self.desc, self.lma)

    # ------------------------------------------------------------------------------------------
    @classmethod
    def from_layers(cls, ext, pi, vf, act_head, val_head, log_std, stack_k: int, frame_dim: int = 15,
                    activation: str = "tanh", heads_stacking: int = 4, pe=None, device=None, seed: int = 0,
                    env_id_base: int = 0):
        """ext: extractor_from_state_dict's form; pi / vf / heads / log_std as DevicePolicy.from_layers.
        embed_dim, ff_hidden and the block count come from the shapes. pe: another (K, embed_dim)
        table in place of the sinusoidal one (tests)."""
        desc = policy_desc(stack_k, frame_dim, [w.shape[0] for w, _ in pi], [w.shape[0] for w, _ in vf], activation)
        blocks = ext["blocks"]
        if ext["embed"][0].shape[1] != LMA_FEATURES:
            raise ValueError("input_embedding reads %d features per frame, the extractor's per-frame transform gives %d"
                             % (ext["embed"][0].shape[1], LMA_FEATURES))
        lma = lma_desc(stack_k, frame_dim, embed_dim=ext["embed"][0].shape[0], heads_stacking=heads_stacking,
                       d_new=ext["embed2"][0].shape[0],
                       ff_hidden=blocks[0]["mlp.c_fc"][0].shape[0] if blocks else 128, n_layers=len(blocks))
        p = cls(desc, lma, device if device is not None else pi[0][0].device, seed, env_id_base)
        p.load(ext, pi, vf, act_head, val_head, log_std, pe=pe)
        return p

    @classmethod
    def from_state_dict(cls, sd, stack_k: int, frame_dim: int = 15, activation: str = "tanh", heads_stacking: int = 4,
                        device=None, seed: int = 0, env_id_base: int = 0):
        """From model.policy.state_dict() of a reference run (key names only; SB3 not imported)."""
        return cls.from_layers(extractor_from_state_dict(sd), *layers_from_state_dict(sd), stack_k=stack_k,
                               frame_dim=frame_dim, activation=activation, heads_stacking=heads_stacking, device=device,
                               seed=seed, env_id_base=env_id_base)

    def load(self, ext, pi, vf, act_head, val_head, log_std, pe=None):
        """Repack into the same device blob: one stream-ordered copy; captured graphs stay valid."""
        if pe is None:
            pe = positional_encoding(self.k, int(self.lma.embed_dim))
        with torch.no_grad():
            self.blob.copy_(pack_lma_blob(self.desc, self.lma, ext, pe, pi, vf, act_head, val_head, log_std),
                            non_blocking=True)
        return self

    def load_state_dict(self, sd):
        return self.load(extractor_from_state_dict(sd), *layers_from_state_dict(sd))

    def state_dict(self):
        """The blob's layers under SB3's key names, the extractor under all three prefixes."""
        ext, _, *mlp = unpack_lma_blob(self.desc, self.lma, self.blob)
        sd = state_dict_from_extractor(ext)
        sd.update(state_dict_from_layers(*mlp))
        return sd

    # ------------------------------------------------------------------------------------------
    def extract_features(self, obs, out=None):
        """The extractor's output (n, L_new * 32), what ActorCriticPolicy.extract_features returns."""
        n = self._check_obs(obs)
        if out is None:
            out = torch.empty((n, self.features_dim), dtype=torch.float32, device=self.device)
        else:
            need_tensor(out, (n, self.features_dim), torch.float32, self.device, "out", 16)
        if n:
            values = torch.empty(n, dtype=torch.float32, device=self.device)
            self._launch(obs, n, 0, None, None, values, None, F16_POLICY_VALUE_ONLY, out)
        return out

    def forward_with_features(self, obs, step, eps=None, deterministic=False):
        """(actions, values, log_probs, features) of one launch."""
        from .abi import F16_POLICY_DETERMINISTIC
        n = self._check_obs(obs)
        actions = torch.empty((n, ACT_DIM), dtype=torch.float32, device=self.device)
        values = torch.empty(n, dtype=torch.float32, device=self.device)
        log_probs = torch.empty(n, dtype=torch.float32, device=self.device)
        feats = torch.empty((n, self.features_dim), dtype=torch.float32, device=self.device)
        if eps is not None:
            need_tensor(eps, (n, ACT_DIM), torch.float32, self.device, "eps", 16)
        if n:
            self._launch(obs, n, step, eps, actions, values, log_probs, F16_POLICY_DETERMINISTIC if deterministic else 0,
                         feats)
        return actions, values, log_probs, feats

    # ------------------------------------------------------------------------------------------
    # forward only: every gradient entry point refuses by name
    def requires_grad_(self, flag: bool = True):
        if flag:
            raise NotImplementedError(NO_BACKWARD)
        return self

    def backward_blob(self, *args, **kwargs):
        raise NotImplementedError(NO_BACKWARD)

    def reserve_backward(self, *args, **kwargs):
        raise NotImplementedError(NO_BACKWARD)

    def mean_and_value(self, obs):
        if torch.is_grad_enabled() and self.blob.requires_grad:
            raise NotImplementedError(NO_BACKWARD)
        return self._mean_and_value(obs)

    def evaluate_actions(self, obs, actions):
        if torch.is_grad_enabled() and self.blob.requires_grad:
            raise NotImplementedError(NO_BACKWARD)
        with torch.no_grad():
            mean, values = self._mean_and_value(obs)
            ls = self.offsets[F16_POLICY_OFF_LOG_STD]
            dist = torch.distributions.Normal(mean, torch.ones_like(mean) * self.blob[ls:ls + ACT_DIM].exp())
            return values, dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1)


class DeviceLMATrainPolicy(DeviceLMAPolicy):
    """DeviceLMAPolicy with the eval-mode backward (f16env_policy_lma_backward): the same
    constructors, blob and forward, so one object serves collect_rollout and the update.

    This is the EVAL-MODE network: dropout is the identity in the forward and in the gradient, which
    is therefore the reference's gradient at lma_dropout = 0.0 (the reference trains with 0.1; the
    training-mode dropout is not built, and DevicePPO refuses this class as it refuses the parent).
    The blob is the parameter; the PE table, log_std's slots of the kernel's gradient and every pad
    receive +0 from the kernel (log_std's gradient reaches blob.grad through autograd's own slice
    backward in evaluate_actions). An optimiser with weight decay would move the PE table: use none."""

    # DevicePolicy's own gradient entry points in place of the parent's refusals: they differ only in
    # the two symbols (backward_blob's +0 positions include the PE table)
    _BWD = ("f16env_policy_lma_backward_workspace", "f16env_policy_lma_backward")

    parameters = DevicePolicy.parameters
    requires_grad_ = DevicePolicy.requires_grad_
    reserve_backward = DevicePolicy.reserve_backward
    backward_blob = DevicePolicy.backward_blob
    mean_and_value = DevicePolicy.mean_and_value
    evaluate_actions = DevicePolicy.evaluate_actions
