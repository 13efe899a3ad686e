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


def stream_ptr(device) -> ctypes.c_void_p:
    """The caller's current stream on `device`, as the ABI's `void* stream`."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
