"""CPU checks of the minibatch sampler's host side: the flat index order against SB3's
swap_and_flatten, the C entry point's argument checks without a device, the Python mirror of
F16RolloutView against the header as a C compiler lays it out, and get()'s own refusals."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import minibatch_ref
from f16_jsb_amd import abi
from f16_jsb_amd.rollout import DeviceRolloutBuffer, RolloutSamples, flat_index, unflatten_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "f16env.h")
A = 4096  # a non-NULL, 16-B aligned stand-in address (never dereferenced: the call is refused first)


@pytest.fixture(scope="module")
def L():
    from f16_jsb_amd.build import build
    build()
    from f16_jsb_amd import _lib
    return _lib.lib()


def _view(**kw):
    v = abi.RolloutView(1, 4, 7, 5, *([A] * 8))
    for key, val in kw.items():
        setattr(v, key, val)
    return v


def test_flat_index_is_swap_and_flatten_order():
    T, N = 7, 5
    t, env = np.meshgrid(np.arange(T), np.arange(N), indexing="ij")
    flat_t, flat_env = minibatch_ref.swap_and_flatten(t), minibatch_ref.swap_and_flatten(env)
    i = np.arange(T * N)
    # position i of the flattened buffer holds transition (flat_t[i], flat_env[i])
    assert np.array_equal(flat_index(flat_t[:, 0], flat_env[:, 0], T), i)
    tt, ee = unflatten_index(i, T)
    assert np.array_equal(tt, flat_t[:, 0]) and np.array_equal(ee, flat_env[:, 0])
    # a grid of flat indices laid out (T, N) flattens to arange, and the same on tensors and ints
    assert np.array_equal(minibatch_ref.swap_and_flatten(flat_index(t, env, T))[:, 0], i)
    ti = torch.arange(T * N)
    assert torch.equal(flat_index(*unflatten_index(ti, T), T), ti)
    assert flat_index(3, 2, T) == 17 and unflatten_index(17, T) == (3, 2)
    assert RolloutSamples._fields == ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns")


def test_entry_point_is_exported_and_bound(L):
    from f16_jsb_amd import _lib
    assert "f16env_rollout_minibatch" in _lib.EXPORTED_SYMBOLS and hasattr(L, "f16env_rollout_minibatch")
    assert L.f16env_rollout_minibatch.restype is ctypes.c_int
    assert L.f16env_abi_version() == abi.F16ENV_ABI_VERSION


def test_bad_arguments_return_errors_without_a_device(L):
    """Every bad argument gives -1 and a message before anything is launched (no device needed)."""
    fn = L.f16env_rollout_minibatch
    err = L.f16env_last_error
    ok = ctypes.byref(_view())
    assert fn(None, None, 4, A, A, A, A, A, A, A) == -1 and b"view" in err()
    assert fn(None, ok, -1, A, A, A, A, A, A, A) == -1 and b"batch" in err()
    for k in (0, 65, -3):
        assert fn(None, ctypes.byref(_view(K=k)), 4, A, A, A, A, A, A, A) == -1 and b"K must be" in err()
    for key in ("world", "n_steps", "n_envs"):
        for bad in (0, -2):
            assert fn(None, ctypes.byref(_view(**{key: bad})), 4, A, A, A, A, A, A, A) == -1 and b">= 1" in err()
    assert fn(None, ctypes.byref(_view(world=2 ** 31 - 1, n_steps=2 ** 40, n_envs=2 ** 40)), 4, A, A, A, A, A, A, A) == -1
    assert b"too large" in err()
    for pos in range(3, 10):  # indices and each of the six outputs NULL
        args = [None, ok, 4] + [A] * 7
        args[pos] = None
        assert fn(*args) == -1 and b"null" in err()
    # alignment: the view's actions and the obs / actions outputs on 16 B, floats on 4, indices on 8
    assert fn(None, ctypes.byref(_view(actions=A + 4)), 4, A, A, A, A, A, A, A) == -1 and b"16-byte" in err()
    assert fn(None, ok, 4, A, A + 4, A, A, A, A, A) == -1 and b"16-byte" in err()
    assert fn(None, ok, 4, A, A, A + 8, A, A, A, A) == -1 and b"16-byte" in err()
    assert fn(None, ok, 4, A, A, A, A + 2, A, A, A) == -1 and b"float-aligned" in err()
    assert fn(None, ctypes.byref(_view(frames=A + 1)), 4, A, A, A, A, A, A, A) == -1 and b"float-aligned" in err()
    assert fn(None, ok, 4, A + 4, A, A, A, A, A, A) == -1 and b"8-byte" in err()
    # an empty batch is no error and launches nothing, NULL arrays or not
    assert fn(None, ok, 0, None, None, None, None, None, None, None) == 0
    assert fn(None, ctypes.byref(_view(frames=None)), 0, A, A, A, A, A, A, A) == 0
    assert fn(None, None, 0, A, A, A, A, A, A, A) == -1


def test_view_mirror_reaches_every_field(L):
    """Each field of the Python mirror lands where the library reads it: a NULL in one pointer
    field is refused by that field's name, and the sizes by theirs."""
    fn = L.f16env_rollout_minibatch
    for f in ("frames", "obs0", "episode_starts", "values", "log_probs", "advantages", "returns", "actions"):
        assert fn(None, ctypes.byref(_view(**{f: None})), 4, A, A, A, A, A, A, A) == -1
        assert L.f16env_last_error() == b"view %s is NULL" % f.encode(), f
    assert [f for f, _ in abi.RolloutView._fields_][:4] == ["world", "K", "n_steps", "n_envs"]


def test_view_mirror_matches_the_header_layout(tmp_path):
    """sizeof / offsetof of F16RolloutView as a C compiler lays the header out, against ctypes."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler builds the test harnesses of this suite"
    fields = [f for f, _ in abi.RolloutView._fields_]
    src = open(HDR).read()
    body = re.search(r"typedef struct F16RolloutView \{(.*?)\} F16RolloutView;", src, re.S).group(1)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert declared == fields  # the same names in the same order
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "f16env.h"\nint main(void) {\n'
                    '  printf("%zu", sizeof(F16RolloutView));\n'
                    + "".join('  printf(" %%zu", offsetof(F16RolloutView, %s));\n' % f for f in fields)
                    + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(abi.RolloutView) == 88
    assert got[1:] == [getattr(abi.RolloutView, f).offset for f in fields]


def _full_buffer(T=7, N=5, K=4):
    buf = DeviceRolloutBuffer(T, N, K, "cpu")
    for _ in range(T):
        assert not buf.full
        with pytest.raises(RuntimeError, match="not full"):
            buf.get(4)
        buf.add(torch.zeros(N, K, 15), torch.zeros(N, 4), torch.zeros(N), torch.zeros(N), torch.zeros(N), torch.zeros(N))
    assert buf.full
    return buf


def test_get_refuses_a_buffer_that_is_not_full_and_indices_out_of_range():
    T, N = 7, 5
    buf = _full_buffer(T, N)
    good = np.random.default_rng(0).permutation(T * N)
    for bad in (-1, T * N):
        for where in (0, 17, T * N - 1):
            idx = good.copy()
            idx[where] = bad
            for form in (idx, torch.from_numpy(idx), idx.tolist()):
                with pytest.raises(ValueError, match=r"indices must lie in \[0, 35\)"):
                    buf.get(8, indices=form)
    with pytest.raises(ValueError, match="batch_size"):
        buf.get(0)
    with pytest.raises(ValueError, match="1-D integer"):
        buf.get(8, indices=good.astype(np.float32))
    # in-range indices pass the range check; a host buffer is then refused as the wrong device
    with pytest.raises(ValueError, match="GPU"):
        buf.get(8, indices=good)


def test_low_level_call_refuses_wrong_sources():
    from f16_jsb_amd.rollout import rollout_minibatch
    buf = _full_buffer()
    idx = torch.arange(4)
    with pytest.raises(ValueError, match="GPU"):
        rollout_minibatch(buf, idx)
    with pytest.raises(ValueError, match="lacks"):
        rollout_minibatch({"frames": buf.frames}, idx)
    with pytest.raises(ValueError, match="frames must be"):
        rollout_minibatch(dict(buf.state_dict(), frames=buf.frames[0]), idx)
