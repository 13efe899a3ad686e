"""ctypes binding of libf16env.so (the HIP product path).

The library is built in-tree (f16_jsb_amd/libf16env.so, see build.py). torch is imported
first so that the process has exactly one HIP runtime (torch's libamdhip64.so.7, which
libf16env.so's NEEDED entry then resolves to). There is no CPU fallback: if the library is
missing, or no GPU is visible, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os

from .abi import F16ENV_ABI_VERSION, EnvConfig, PolicyDesc, RolloutSlot, RolloutView

LIB_PATH = os.environ.get("F16ENV_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libf16env.so")

_lib = None


class F16EnvError(RuntimeError):
    pass


_vp, _i32, _u32, _i64, _u64, _f64 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64,
                                     ctypes.c_double)
_str, _P = ctypes.c_char_p, ctypes.POINTER
_cfg, _slot, _view, _desc = _P(EnvConfig), _P(RolloutSlot), _P(RolloutView), _P(PolicyDesc)

# Every entry point of include/f16env.h, in the header's order: name -> (restype, one type per
# parameter). This table is the binding: lib() applies it, EXPORTED_SYMBOLS is its keys, and
# tests/test_abi_cpu.py holds it against the header's prototypes (count, class and width of every
# parameter, the return type). An entry point is added in the header and here, nowhere else.
SIGNATURES = {
    "f16env_config_default": (_i32, (_cfg,)),
    "f16env_config_cfg5": (_i32, (_cfg,)),
    "f16env_create": (_i32, (_cfg, _i32, _P(_vp))),
    "f16env_destroy": (_i32, (_vp,)),
    "f16env_step_mode": (_i32, (_vp,)),
    "f16env_state_bytes": (ctypes.c_size_t, (_vp,)),
    "f16env_state_bytes_per_env": (_i32, ()),
    "f16env_reset": (_i32, (_vp, _vp, _vp, _vp, _vp, _vp)),
    "f16env_step": (_i32, (_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "f16env_step_window": (_i32, (_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "f16env_window_bind": (_i32, (_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp)),
    "f16env_window_step_bound": (_i32, (_vp, _vp, _vp, _i32, _i32)),
    "f16env_window_feature_bind": (_i32, (_vp, _vp, _vp)),
    "f16env_window_poses_bind": (_i32, (_vp, _vp)),
    "f16env_window_step_ex": (_i32, (_vp, _vp, _vp, _i32, _i32, _u32, _u64, _u64)),
    "f16env_window_step_ex_kernel_name": (_str, (_vp, _u32)),
    "f16env_reset_window": (_i32, (_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32)),
    "f16env_window_restart": (_i32, (_vp, _vp, _vp, _vp, _i64, _i32)),
    "f16env_set_window_order": (_i32, (_vp, _i32)),
    "f16env_window_clear_fresh": (_i32, (_vp, _vp)),
    "f16env_step_window_waves_per_simd": (_i32, (_vp,)),
    "f16env_step_window_nt": (_i32, (_vp,)),
    "f16env_window_resets_deferred": (_i32, (_vp,)),
    "f16env_step_rollout": (_i32, (_vp, _vp, _slot, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "f16env_window_step_rollout": (_i32, (_vp, _vp, _slot, _vp, _i32, _i32)),
    "f16env_rollout_random": (_i32, (_vp, _vp, _u64, _u64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "f16env_window_rollout_random": (_i32, (_vp, _vp, _u64, _u64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp)),
    "f16env_bootstrap_timeouts": (_i32, (_vp, _i64, _vp, _vp, _vp, _vp, _f64)),
    "f16env_bootstrap_stash": (_i32, (_vp, _i64, _i32, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64)),
    "f16env_bootstrap_apply": (_i32, (_vp, _i64, _vp, _vp, _vp, _f64)),
    "f16env_abi_version": (_i32, ()),
    "f16env_nonfinite_count": (_i32, (_vp, _vp, _P(_u64))),
    "f16env_debug_checks": (_i32, (_vp, _vp, _P(_u32))),
    "f16env_obs_bounds_count": (_i32, (_vp, _vp, _P(_u64))),
    "f16env_get_state": (_i32, (_vp, _vp, _vp)),
    "f16env_set_state": (_i32, (_vp, _vp, _vp)),
    "f16env_trim": (_i32, (_vp, _vp, _vp, _vp, _vp)),
    "f16env_sample_actions": (_i32, (_vp, _vp, _u64, _u64, _vp)),
    "f16env_sample_actions_steps": (_i32, (_vp, _vp, _u64, _u64, _i32, _vp)),
    "f16env_gae": (_i32, (_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _f64, _f64, _vp, _vp)),
    "f16env_rollout_minibatch": (_i32, (_vp, _view, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "f16env_policy_blob_layout": (_i32, (_desc, _P(_i64), _P(_i64))),
    "f16env_policy_forward": (_i32, (_vp, _desc, _vp, _i64, _vp, _i64, _i64, _u64, _u64, _i64, _vp, _vp, _vp, _vp,
                                     _u32)),
    "f16env_policy_backward_workspace": (_i32, (_desc, _i64, _i32, _P(_i64))),
    "f16env_policy_backward": (_i32, (_vp, _desc, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _i32, _vp)),
    "f16env_policy_lma_blob_layout": (_i32, (_desc, _vp, _P(_i64), _P(_i64))),
    "f16env_policy_lma_forward": (_i32, (_vp, _desc, _vp, _vp, _i64, _vp, _i64, _i64, _u64, _u64, _i64, _vp, _vp, _vp,
                                         _vp, _vp, _u32)),
    "f16env_policy_lma_backward_workspace": (_i32, (_desc, _vp, _i64, _i32, _P(_i64))),
    "f16env_policy_lma_backward": (_i32, (_vp, _desc, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _i32, _vp)),
    "f16env_ppo_workspace": (_i32, (_i64, _i32, _P(_i64))),
    "f16env_ppo_head_blocks": (_i32, (_i64, _i32, _P(_i32))),
    "f16env_ppo_loss_head": (_i32, (_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _i32, _vp, _i64, _vp,
                                    _vp)),
    "f16env_ppo_adam_step": (_i32, (_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _vp)),
    "f16env_ppo_dynago_workspace": (_i32, (_i64, _i32, _P(_i64))),
    "f16env_ppo_dynago_update": (_i32, (_vp, _i64, _vp, _vp, _vp, _i32, _vp, _i64)),
    "f16env_ppo_loss_head_am": (_i32, (_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _i32, _vp,
                                       _i64, _vp, _vp, _vp)),
    "f16env_ppo_dag_step": (_i32, (_vp, _i64, _vp, _vp, _vp, _vp, _P(ctypes.c_int32), _i32, _vp, _vp, _vp, _u32, _i64,
                                   _vp, _i32, _vp)),
    "f16env_features": (_i32, (_vp, _i64, _vp, _vp)),
    "f16env_features_strided": (_i32, (_vp, _i64, _i32, _vp, _i64, _i64, _vp)),
    "f16env_features_window_step": (_i32, (_vp, _i64, _i32, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _i32)),
    "f16env_poses": (_i32, (_vp, _i64, _vp, _i64, _vp)),
    "f16env_step_kernel_name": (_str, (_vp,)),
    "f16env_step_waves_per_simd": (_i32, (_vp,)),
    "f16env_step_variant": (_i32, (_vp,)),
    "f16env_algorithmic_bytes_per_env_step": (_f64, (_i32,)),
    "f16env_profile_begin": (_i32, (_vp, _i32)),
    "f16env_profile_end": (_i32, (_vp, _P(_f64), _P(_f64), _P(_i32))),
    "f16env_profile_times": (_i32, (_vp, _P(_f64), _i32)),
    "f16env_last_error": (_str, ()),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)


def lib():
    """Load libf16env.so (raises F16EnvError if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  -- one HIP runtime per process (torch's)

    if not os.path.exists(LIB_PATH):
        raise F16EnvError(
            "libf16env.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `python -m f16_jsb_amd.build`" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    # a symbol an older build lacks stays unbound (the A/B tools time earlier libraries side by
    # side through F16ENV_LIB; fn() reports its absence, tests check the product exports every one)
    for name, (restype, argtypes) in SIGNATURES.items():
        f = getattr(L, name, None)
        if f is not None:
            f.restype, f.argtypes = restype, argtypes
    # the header's F16ENV_ABI_VERSION must be the library's (a stale build behind a changed
    # signature would be called with the wrong arguments); libraries from before the version
    # export (ABI 2) load only when named explicitly through F16ENV_LIB (tools comparing builds)
    got = L.f16env_abi_version() if hasattr(L, "f16env_abi_version") else 2
    if got != F16ENV_ABI_VERSION and (got != 2 or not os.environ.get("F16ENV_LIB")):
        raise F16EnvError("%s has ABI version %d, this binding expects %d: rebuild it (python -m f16_jsb_amd.build)"
                          % (LIB_PATH, got, F16ENV_ABI_VERSION))
    _lib = L
    return L


def check(status: int, what: str):
    if status != 0:
        msg = lib().f16env_last_error()
        raise F16EnvError("%s failed (%d): %s" % (what, status, msg.decode() if msg else "?"))


def fn(name: str):
    """The bound entry point `name`, or F16EnvError when the loaded library is an older build without it."""
    f = getattr(lib(), name, None)
    if f is None:
        raise F16EnvError("this libf16env.so has no %s: rebuild it (python -m f16_jsb_amd.build)" % name)
    return f
