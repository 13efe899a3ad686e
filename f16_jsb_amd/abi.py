"""Python mirror of include/f16env.h (constants, config struct, defaults).

Pure ctypes/numpy: no torch, no library load. The defaults are the reference's constants
(jsbsim_gym/jsbsim_gym.py:56-58,157-170,532).
"""
from __future__ import annotations

import ctypes

F16ENV_ABI_VERSION = 7  # include/f16env.h (checked against f16env_abi_version() at load)
F16_OBS_DIM = 15
F16_ACT_DIM = 4

(F16_IC_LAT_GEOD_RAD, F16_IC_LON_RAD, F16_IC_H_SL_FT, F16_IC_U_FPS, F16_IC_V_FPS, F16_IC_W_FPS,
 F16_IC_PHI_RAD, F16_IC_THETA_RAD, F16_IC_PSI_RAD, F16_IC_P_RPS, F16_IC_Q_RPS, F16_IC_R_RPS,
 F16_IC_CMD_AIL, F16_IC_CMD_ELE, F16_IC_CMD_RUD, F16_IC_CMD_THR,
 F16_IC_WIND_N_FPS, F16_IC_WIND_E_FPS, F16_IC_WIND_D_FPS, F16_IC_N) = range(20)

F16C_RI, F16C_VI, F16C_VIH1, F16C_VIH2, F16C_AI, F16C_AIP = 0, 3, 6, 9, 12, 15
F16C_Q, F16C_WI, F16C_WID, F16C_BA = 18, 22, 25, 28
F16C_EPA_C, F16C_EPA_S = 31, 32
F16C_TEF, F16C_AIL, F16C_ELE, F16C_RUD, F16C_LEF, F16C_SB = 33, 34, 35, 36, 37, 38
F16C_PID_R_I, F16C_PID_R_P, F16C_PID_P_I, F16C_PID_P_P, F16C_PID_Y_I, F16C_PID_Y_P = range(39, 45)
F16C_N1, F16C_N2, F16C_AUG = 45, 46, 47
F16C_LX = 48
F16C_CMD = 58
F16C_GOAL = 62
F16C_LAST_D, F16C_STEP, F16C_EP_RET, F16C_EP_COUNT = 65, 66, 67, 68
F16C_WIND = 69
F16C_GUST = 72
F16C_N = 75

(F16L_ALPHA, F16L_BETA, F16L_MACH, F16L_VC_KTS, F16L_VG_FPS, F16L_P_AERO, F16L_Q_AERO,
 F16L_R_AERO, F16L_NPY, F16L_NPZ, F16L_N) = range(11)

F16_FLAG_NO_AUTORESET = 0x1
F16_FLAG_RANDOM_IC = 0x2  # cfg5: reset IC drawn from the [ic_lo, ic_hi] box
F16_FLAG_GUSTS = 0x4      # cfg5: Gauss-Markov gusts on top of the steady wind
F16_FLAG_NAN_GUARD = 0x8  # quarantine lanes whose frame goes non-finite (terminated = 3, counted)
F16_FLAG_OBS_CHECK = 0x10  # count lane-steps whose new frame has a finite value outside the obs space

# jsbsim_gym.py:28-53 observation bounds (per frame)
EPSILON = 1e-5


class EnvConfig(ctypes.Structure):
    _fields_ = [
        ("n_envs", ctypes.c_int32),
        ("stack_k", ctypes.c_int32),
        ("down_sample", ctypes.c_int32),
        ("max_steps", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("dt", ctypes.c_double),
        ("dg_m", ctypes.c_double),
        ("goal_gain", ctypes.c_double),
        ("crash_alt_m", ctypes.c_double),
        ("seed", ctypes.c_uint64),
        ("env_id_base", ctypes.c_int64),
        ("ic", ctypes.c_double * F16_IC_N),
        ("ic_lo", ctypes.c_double * F16_IC_N),
        ("ic_hi", ctypes.c_double * F16_IC_N),
        ("gust_sigma_fps", ctypes.c_double),
        ("gust_tau_s", ctypes.c_double),
    ]


def default_ic_values():
    ic = [0.0] * F16_IC_N
    ic[F16_IC_H_SL_FT] = 5000.0  # jsbsim_gym.py:170 ic/h-sl-ft
    ic[F16_IC_U_FPS] = 900.0     # jsbsim_gym.py:169 ic/u-fps
    return ic


def config_default(n_envs=1, stack_k=10, down_sample=4, max_steps=1200, flags=0,
                   dt=1.0 / 120.0, dg_m=100.0, goal_gain=1e-2, crash_alt_m=10.0, seed=0,
                   env_id_base=0, ic=None, cfg5=False) -> EnvConfig:
    """f16env_config_default with overrides; cfg5=True adds the BASELINE cfg5 random-IC box
    and gusts (config_cfg5)."""
    c = EnvConfig()
    c.n_envs = int(n_envs)
    c.stack_k = int(stack_k)          # NUM_STACKED_FRAMES (:58)
    c.down_sample = int(down_sample)  # (:157)
    c.max_steps = int(max_steps)      # (:159, TimeLimit :541)
    c.flags = int(flags)
    c.dt = float(dt)                  # JSBSim default frame
    c.dg_m = float(dg_m)              # (:163)
    c.goal_gain = float(goal_gain)    # (:532)
    c.crash_alt_m = float(crash_alt_m)  # (:245)
    c.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c.env_id_base = int(env_id_base)
    vals = default_ic_values() if ic is None else list(ic)
    for i in range(F16_IC_N):
        c.ic[i] = c.ic_lo[i] = c.ic_hi[i] = float(vals[i])
    c.gust_sigma_fps = 0.0
    c.gust_tau_s = 2.0
    if cfg5:
        config_cfg5(c)
    return c


# BASELINE cfg5 box (include/f16env.h f16env_config_cfg5; SURVEY.md 8c cfg5 ranges)
CFG5_BOX = {
    F16_IC_H_SL_FT: (3000.0, 30000.0),
    F16_IC_U_FPS: (600.0, 1200.0),
    F16_IC_PHI_RAD: (-0.17453292519943295, 0.17453292519943295),
    F16_IC_THETA_RAD: (-0.17453292519943295, 0.17453292519943295),
    F16_IC_PSI_RAD: (0.0, 6.283185307179586),
    F16_IC_CMD_THR: (0.3, 1.0),
    F16_IC_WIND_N_FPS: (-30.0, 30.0),
    F16_IC_WIND_E_FPS: (-30.0, 30.0),
}
CFG5_GUST_SIGMA_FPS = 10.0
CFG5_GUST_TAU_S = 2.0


def config_cfg5(c: EnvConfig) -> EnvConfig:
    """Python twin of f16env_config_cfg5: random-IC box + gusts on top of ``c``."""
    c.flags = int(c.flags) | F16_FLAG_RANDOM_IC | F16_FLAG_GUSTS
    for i in range(F16_IC_N):
        lo, hi = CFG5_BOX.get(i, (c.ic[i], c.ic[i]))
        c.ic_lo[i], c.ic_hi[i] = lo, hi
    c.gust_sigma_fps = CFG5_GUST_SIGMA_FPS
    c.gust_tau_s = CFG5_GUST_TAU_S
    return c


def algorithmic_bytes_per_env_step(stack_k: int, state_bytes: int, layout: str = "contiguous") -> int:
    """Bytes one env step must move. Contiguous stacks, SURVEY.md 8(d):
    B(K) = 16 + 60K + 60(K-1) + 4 + 2 + 2S (action, the new stack written, the previous K-1
    frames read, reward, flags, state read + written). Windowed observations
    (f16env_step_window): B_win = 16 + 2*60 + 4 + 2 + S + (S - 16), independent of K -- the
    new frame written to both histories, no frames read (a reset lane's fresh window aside), the
    state read whole and written back without its per-episode column (goal, episode count),
    which only a lane the step resets rewrites (round 5; ~0.1 % of lanes per step in the bench's
    steady state)."""
    if layout == "window":
        return 16 + 2 * 60 + 4 + 2 + 2 * state_bytes - 16
    if layout != "contiguous":
        raise ValueError("layout must be 'contiguous' or 'window'")
    return 16 + 60 * stack_k + 60 * (stack_k - 1) + 4 + 2 + 2 * state_bytes


F16_SLOT_CLIP = 0x1  # the env steps np.clip(act, low, high); the slot keeps act unclipped
F16_SLOT_FEATURE_WINDOW = 0x2  # the windowed rollout-slot step also updates the bound feature histories
F16_STEP_FEATURE_WINDOW = 0x2  # f16env_window_step_ex: the plain windowed step updates them too (ABI 4)
F16_STEP_POSES = 0x4  # f16env_window_step_ex: the step writes the bound N x 10 pose export (ABI 5)


class RolloutSlot(ctypes.Structure):
    """f16env_rollout_slot (include/f16env.h): one slot of a device rollout buffer filled by
    f16env_step_rollout / f16env_window_step_rollout; NULL pointers are not written."""
    _fields_ = [
        ("act_seed", ctypes.c_uint64),
        ("act_step", ctypes.c_uint64),
        ("frame", ctypes.c_void_p),
        ("actions", ctypes.c_void_p),
        ("rewards", ctypes.c_void_p),
        ("next_start", ctypes.c_void_p),
        ("features", ctypes.c_void_p),
        ("next_frame", ctypes.c_void_p),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class RolloutView(ctypes.Structure):
    """F16RolloutView (include/f16env.h): the finished rollout f16env_rollout_minibatch samples,
    one device's buffer (world 1) or the rank-major gather of `world` shards."""
    _fields_ = [
        ("world", ctypes.c_int32),
        ("K", ctypes.c_int32),
        ("n_steps", ctypes.c_int64),
        ("n_envs", ctypes.c_int64),
        ("frames", ctypes.c_void_p),
        ("obs0", ctypes.c_void_p),
        ("episode_starts", ctypes.c_void_p),
        ("values", ctypes.c_void_p),
        ("log_probs", ctypes.c_void_p),
        ("advantages", ctypes.c_void_p),
        ("returns", ctypes.c_void_p),
        ("actions", ctypes.c_void_p),
    ]


# ABI 7: the device policy (f16env_policy_forward)
F16_POLICY_ACT_TANH = 0
F16_POLICY_ACT_RELU = 1
F16_POLICY_DETERMINISTIC = 0x1  # eps = 0: the action is the mean
F16_POLICY_VALUE_ONLY = 0x2     # the vf branch alone; actions / log_probs not touched
F16_POLICY_N_OFFSETS = 17       # f16env_policy_blob_layout: 6 b + 2 l (+ 1) weight (bias) of layer l, branch b
F16_POLICY_OFF_ACT_W, F16_POLICY_OFF_ACT_B, F16_POLICY_OFF_VAL_W, F16_POLICY_OFF_VAL_B = 12, 13, 14, 15
F16_POLICY_OFF_LOG_STD = 16
F16_PPO_NORMALIZE_ADV = 0x1     # f16env_ppo_loss_head: (A - mean(A)) / (std(A) + 1e-8) when n > 1
# the device hyper array both PPO kernels read, and f16env_ppo_adam_step's stats (include/f16env.h)
PPO_HYPER = ("lr", "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "beta1", "beta2", "eps")
(F16_PPO_HYPER_LR, F16_PPO_HYPER_CLIP_RANGE, F16_PPO_HYPER_ENT_COEF, F16_PPO_HYPER_VF_COEF, F16_PPO_HYPER_MAX_GRAD_NORM,
 F16_PPO_HYPER_BETA1, F16_PPO_HYPER_BETA2, F16_PPO_HYPER_EPS, F16_PPO_N_HYPER) = range(9)
F16_PPO_N_STATS = 8
PPO_STATS = ("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction", "grad_norm", "clip_coef")
# AM-PPO (f16env_ppo_dynago_update, f16env_ppo_loss_head_am, f16env_ppo_dag_step): the flags and the
# named orders of the device arrays `dynago`, `am_stats` and `dag` (include/f16env.h)
F16_PPO_AM_NORMALIZE = 0x1      # (mod - mean(mod)) / (std(mod) + 1e-8) when n > 1
F16_PPO_DAG_FIXED_ALPHA = 0x1   # f16env_ppo_dag_step as AlphaGrad
PPO_DYNAGO = ("tau", "p_star", "kappa_controller", "eta", "rho", "eps", "alpha_min", "alpha_max", "rho_sat", "kappa",
              "v_shift")
(F16_PPO_DYNAGO_TAU, F16_PPO_DYNAGO_P_STAR, F16_PPO_DYNAGO_KAPPA_CONTROLLER, F16_PPO_DYNAGO_ETA, F16_PPO_DYNAGO_RHO,
 F16_PPO_DYNAGO_EPS, F16_PPO_DYNAGO_ALPHA_MIN, F16_PPO_DYNAGO_ALPHA_MAX, F16_PPO_DYNAGO_RHO_SAT, F16_PPO_DYNAGO_KAPPA,
 F16_PPO_DYNAGO_V_SHIFT, F16_PPO_N_DYNAGO) = range(12)
F16_PPO_N_AM_STATS = 4
PPO_AM_STATS = ("mean_raw_adv", "mean_mod_adv", "adv_norm", "alpha")
PPO_DAG = ("tau", "p_star", "kappa", "beta", "eta", "rho", "eps", "alpha_min", "alpha_max", "k_val", "lambda_rms",
           "s_min", "gamma", "ema_beta", "warmup_steps", "sat_every", "alpha")
(F16_PPO_DAG_TAU, F16_PPO_DAG_P_STAR, F16_PPO_DAG_KAPPA, F16_PPO_DAG_BETA, F16_PPO_DAG_ETA, F16_PPO_DAG_RHO,
 F16_PPO_DAG_EPS, F16_PPO_DAG_ALPHA_MIN, F16_PPO_DAG_ALPHA_MAX, F16_PPO_DAG_K_VAL, F16_PPO_DAG_LAMBDA_RMS,
 F16_PPO_DAG_S_MIN, F16_PPO_DAG_GAMMA, F16_PPO_DAG_EMA_BETA, F16_PPO_DAG_WARMUP_STEPS, F16_PPO_DAG_SAT_EVERY,
 F16_PPO_DAG_ALPHA, F16_PPO_N_DAG) = range(18)
F16_PPO_DAG_MAX_SEGMENTS = 17
POLICY_WIDTHS = (32, 64, 96, 128)
POLICY_MAX_LAYERS = 3


class PolicyDesc(ctypes.Structure):
    """f16_policy_desc (include/f16env.h): the shape of an actor-critic MLP policy."""
    _fields_ = [
        ("K", ctypes.c_int32),
        ("D", ctypes.c_int32),
        ("n_pi", ctypes.c_int32),
        ("n_vf", ctypes.c_int32),
        ("pi_width", ctypes.c_int32 * 3),
        ("vf_width", ctypes.c_int32 * 3),
        ("activation", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


# the LMA features extractor in front of the MLPs (f16env_policy_lma_forward): blob slots past the MLP's
F16_LMA_N_OFFSETS = 58
F16_LMA_OFF_PE, F16_LMA_OFF_WE_W, F16_LMA_OFF_WE_B, F16_LMA_OFF_W2_W, F16_LMA_OFF_W2_B = 17, 18, 19, 20, 21
F16_LMA_OFF_BLOCK0 = 22   # block i's slots start at F16_LMA_OFF_BLOCK0 + F16_LMA_BLOCK_SLOTS * i
F16_LMA_BLOCK_SLOTS = 12
(F16_LMA_BLK_LN1_W, F16_LMA_BLK_LN1_B, F16_LMA_BLK_ATTN_W, F16_LMA_BLK_ATTN_B, F16_LMA_BLK_PROJ_W, F16_LMA_BLK_PROJ_B,
 F16_LMA_BLK_LN2_W, F16_LMA_BLK_LN2_B, F16_LMA_BLK_FC_W, F16_LMA_BLK_FC_B, F16_LMA_BLK_PROJ2_W,
 F16_LMA_BLK_PROJ2_B) = range(12)
LMA_EMBED_DIM, LMA_D_NEW, LMA_HEADS_LATENT, LMA_FEATURES, LMA_MAX_LAYERS, LMA_MAX_L_NEW = 64, 32, 4, 17, 3, 5


class LmaDesc(ctypes.Structure):
    """f16_lma_desc (include/f16env.h): the shape of the LMA features extractor; sixteen int32,
    passed to the library by address."""
    _fields_ = [
        ("K", ctypes.c_int32),
        ("D", ctypes.c_int32),
        ("embed_dim", ctypes.c_int32),
        ("heads_stacking", ctypes.c_int32),
        ("L_new", ctypes.c_int32),
        ("C_new", ctypes.c_int32),
        ("d_new", ctypes.c_int32),
        ("heads_latent", ctypes.c_int32),
        ("ff_hidden", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 6),
    ]


# the header's struct names and their mirrors (tests/test_abi_cpu.py holds every field's offset and size together)
STRUCTS = {"f16env_config": EnvConfig, "f16env_rollout_slot": RolloutSlot, "F16RolloutView": RolloutView,
           "f16_policy_desc": PolicyDesc}


def policy_desc(stack_k: int, frame_dim: int, pi_widths, vf_widths, activation="tanh") -> PolicyDesc:
    acts = {"tanh": F16_POLICY_ACT_TANH, "relu": F16_POLICY_ACT_RELU}
    if activation not in acts:
        raise ValueError("activation must be 'tanh' or 'relu', got %r" % (activation,))
    pi_widths, vf_widths = [int(w) for w in pi_widths], [int(w) for w in vf_widths]
    if not 1 <= int(stack_k) <= 10 or int(frame_dim) not in (15, 17):
        raise ValueError("stack_k must be in 1..10 and frame_dim 15 or 17")
    for ws in (pi_widths, vf_widths):
        if not 1 <= len(ws) <= POLICY_MAX_LAYERS or any(w not in POLICY_WIDTHS for w in ws):
            raise ValueError("each branch has 1 to 3 hidden layers of width 32, 64, 96 or 128, got %s" % (ws,))
    d = PolicyDesc()
    d.K, d.D, d.n_pi, d.n_vf = int(stack_k), int(frame_dim), len(pi_widths), len(vf_widths)
    for i, w in enumerate(pi_widths):
        d.pi_width[i] = w
    for i, w in enumerate(vf_widths):
        d.vf_width[i] = w
    d.activation = acts[activation]
    return d


def policy_blob_layout(d: PolicyDesc, fan_in0=None):
    """Python twin of f16env_policy_blob_layout: (offsets[F16_POLICY_N_OFFSETS], n_floats).
    fan_in0: the first layers' fan-in when it is not K D (the LMA extractor's features)."""
    off = [-1] * F16_POLICY_N_OFFSETS
    p = 0
    for heads in (False, True):  # the hidden layers of both branches, then the two heads (one tile each)
        for b in range(2):
            fan_in = d.K * d.D if fan_in0 is None else int(fan_in0)
            widths = list(d.vf_width[:d.n_vf]) if b else list(d.pi_width[:d.n_pi])
            for l, width in enumerate(widths + [32]):
                head = l == len(widths)
                if head == heads:
                    slot = (F16_POLICY_OFF_VAL_W if b else F16_POLICY_OFF_ACT_W) if head else 6 * b + 2 * l
                    off[slot] = p
                    p += (width // 32) * ((fan_in + 1) // 2) * 64
                    off[slot + 1] = p
                    p += width
                fan_in = width
    off[F16_POLICY_OFF_LOG_STD] = p
    return off, p + 4


def policy_segments(d: PolicyDesc):
    """f16env_ppo_dag_step's segment table for a policy's blob: [(offset, padded length, true element
    count)] per parameter tensor in blob order -- weight and bias of every hidden layer of the pi
    branch, then of the vf branch, the action head, the value head, log_std. The pieces tile the
    blob: each ends where the next begins."""
    off, total = policy_blob_layout(d)
    pieces = []
    for b in range(2):
        fan_in = d.K * d.D
        for l, width in enumerate(list(d.vf_width[:d.n_vf]) if b else list(d.pi_width[:d.n_pi])):
            pieces += [(off[6 * b + 2 * l], width * fan_in), (off[6 * b + 2 * l + 1], width)]
            fan_in = width
    pieces += [(off[F16_POLICY_OFF_ACT_W], F16_ACT_DIM * d.pi_width[d.n_pi - 1]), (off[F16_POLICY_OFF_ACT_B], F16_ACT_DIM),
               (off[F16_POLICY_OFF_VAL_W], d.vf_width[d.n_vf - 1]), (off[F16_POLICY_OFF_VAL_B], 1),
               (off[F16_POLICY_OFF_LOG_STD], F16_ACT_DIM)]
    ends = [o for o, _ in pieces[1:]] + [total]
    return [(o, e - o, count) for (o, count), e in zip(pieces, ends)]


def lma_new_dims(stack_k: int, embed_dim: int = LMA_EMBED_DIM):
    """(L_new, C_new) of the extractor's re-chunk: L_new is the divisor of K embed_dim closest to
    max(K // 2, 1); at a distance delta the candidate below the target is tried before the one
    above (so K = 7, target 3, takes 2, not 4). C_new = K embed_dim / L_new."""
    total, target = int(stack_k) * int(embed_dim), max(int(stack_k) // 2, 1)
    if total < 1:
        raise ValueError("stack_k and embed_dim must be positive")
    for delta in range(total + 1):
        for cand in (target - delta, target + delta):
            if cand > 0 and total % cand == 0:
                return cand, total // cand
    raise AssertionError("unreachable: 1 divides everything")


def lma_desc(stack_k: int, frame_dim: int, embed_dim: int = LMA_EMBED_DIM, heads_stacking: int = 4,
             d_new: int = LMA_D_NEW, heads_latent: int = LMA_HEADS_LATENT, ff_hidden: int = 128,
             n_layers: int = 2) -> LmaDesc:
    """The descriptor of the reference's extractor at a stack length; every field outside the
    kernel's family is refused by name."""
    k, d, hs = int(stack_k), int(frame_dim), int(heads_stacking)
    if not 1 <= k <= 10:
        raise ValueError("stack_k must be in 1..10, got %d" % k)
    if d not in (15, 17):
        raise ValueError("frame_dim must be 15 or 17, got %d" % d)
    if int(embed_dim) != LMA_EMBED_DIM:
        raise ValueError("embed_dim must be %d, got %d" % (LMA_EMBED_DIM, embed_dim))
    if hs < 1 or LMA_EMBED_DIM % hs or (LMA_EMBED_DIM // hs) % 2:
        raise ValueError("heads_stacking must divide embed_dim into an even dk, got %d" % hs)
    if int(d_new) != LMA_D_NEW:
        raise ValueError("d_new must be %d, got %d" % (LMA_D_NEW, d_new))
    if int(heads_latent) != LMA_HEADS_LATENT:
        raise ValueError("heads_latent must be %d, got %d" % (LMA_HEADS_LATENT, heads_latent))
    if int(ff_hidden) not in POLICY_WIDTHS:
        raise ValueError("ff_hidden must be 32, 64, 96 or 128, got %d" % ff_hidden)
    if not 0 <= int(n_layers) <= LMA_MAX_LAYERS:
        raise ValueError("n_layers must be in 0..%d, got %d" % (LMA_MAX_LAYERS, n_layers))
    m = LmaDesc()
    m.K, m.D, m.embed_dim, m.heads_stacking = k, d, LMA_EMBED_DIM, hs
    m.L_new, m.C_new = lma_new_dims(k, LMA_EMBED_DIM)
    m.d_new, m.heads_latent, m.ff_hidden, m.n_layers = LMA_D_NEW, LMA_HEADS_LATENT, int(ff_hidden), int(n_layers)
    return m


def lma_blob_layout(d: PolicyDesc, m: LmaDesc):
    """Python twin of f16env_policy_lma_blob_layout: (offsets[F16_LMA_N_OFFSETS], n_floats)."""
    if (m.K, m.D) != (d.K, d.D):
        raise ValueError("the LMA descriptor's K and D must equal the policy descriptor's")
    if m.L_new * m.C_new != m.K * m.embed_dim:
        raise ValueError("L_new * C_new must equal K * embed_dim")
    off, p = policy_blob_layout(d, m.L_new * m.d_new)
    off = off + [-1] * (F16_LMA_N_OFFSETS - F16_POLICY_N_OFFSETS)

    def put(slot, floats):
        nonlocal p
        off[slot] = p
        p += floats
    nks_d = m.d_new // 2
    put(F16_LMA_OFF_PE, m.K * m.embed_dim)
    put(F16_LMA_OFF_WE_W, (m.embed_dim // 32) * ((LMA_FEATURES + 1) // 2) * 64)
    put(F16_LMA_OFF_WE_B, m.embed_dim)
    put(F16_LMA_OFF_W2_W, (m.C_new // 2) * 64)
    put(F16_LMA_OFF_W2_B, m.d_new)
    for i in range(m.n_layers):
        s = F16_LMA_OFF_BLOCK0 + F16_LMA_BLOCK_SLOTS * i
        for slot, floats in ((F16_LMA_BLK_LN1_W, m.d_new), (F16_LMA_BLK_LN1_B, m.d_new),
                             (F16_LMA_BLK_ATTN_W, 3 * nks_d * 64), (F16_LMA_BLK_ATTN_B, 3 * m.d_new),
                             (F16_LMA_BLK_PROJ_W, nks_d * 64), (F16_LMA_BLK_PROJ_B, m.d_new),
                             (F16_LMA_BLK_LN2_W, m.d_new), (F16_LMA_BLK_LN2_B, m.d_new),
                             (F16_LMA_BLK_FC_W, (m.ff_hidden // 32) * nks_d * 64), (F16_LMA_BLK_FC_B, m.ff_hidden),
                             (F16_LMA_BLK_PROJ2_W, (m.ff_hidden // 2) * 64), (F16_LMA_BLK_PROJ2_B, m.d_new)):
            put(s + slot, floats)
    return off, p
