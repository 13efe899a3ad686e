"""The caller's side of the C ABI: a tensor becomes a raw pointer, the current stream a hipStream_t.
The one place that states what such a tensor must be (as_act, which copies instead of refusing, and
the strided observation checks have rules of their own)."""
from __future__ import annotations

import ctypes

import torch


def need_tensor(x, shape, dtype, device, name, align: int = 4, optional: bool = False) -> None:
    """A buffer a kernel indexes through its raw pointer: a torch.Tensor on exactly `device`, of
    `dtype`, contiguous, of `shape`, its address a multiple of `align` bytes. Anything else would be
    an out-of-bounds, misaligned or host-pointer access on the device, so it is refused here, before
    any launch."""
    if x is None and optional:
        return
    if not isinstance(x, torch.Tensor) or x.device != device or x.dtype != dtype or not x.is_contiguous() \
            or tuple(x.shape) != tuple(shape) or x.data_ptr() % align:
        raise ValueError("%s must be a contiguous %d-byte aligned %s %s tensor on %s"
                         % (name, align, str(dtype).replace("torch.", ""), tuple(shape), device))


def step_flags_bytes(n: int) -> int:
    """Size of the packed per-step outputs of n envs: rewards (f32), terminated, truncated (u8) in
    one uint8 buffer, padded to 16 bytes, so that a host-side consumer moves the three in one copy."""
    return (6 * n + 15) // 16 * 16


def split_step_flags(buf, n: int, f32):
    """(rew, term, trunc) views of a packed step_flags buffer of n envs; `buf` is a uint8 torch tensor
    or numpy array, `f32` its library's float32."""
    return buf[:4 * n].view(f32), buf[4 * n:5 * n], buf[5 * n:6 * n]


def stream_ptr(device) -> ctypes.c_void_p:
    """The caller's current stream on `device`, as the ABI's `void* stream`."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
