"""Static checks of the step prologue's counted waits in the built gfx950 code object (CPU; no
GPU needed), beside tests/test_isa_lint.py.

The headline step kernel issues the table / template LDS-DMAs and its 17 loads (16 state columns
in first-use order and the action), then waits only for the DMAs -- s_waitcnt vmcnt(k), k the
loads issued behind them -- before the barrier that publishes the table staging; each column's
first use waits with a counted vmcnt of its own. A full drain (vmcnt(0)) ahead of the frames'
first table read would put the whole 272 B per env in front of the physics again."""
from __future__ import annotations

import os
import re

import pytest

from test_isa_lint import LLVM_OBJDUMP, _disassemble, _kernels, build_lib

HEADLINE = "_Z22f16_step_win_nt_kernelILi0ELi1ELb0EEvPK15HIP_vector_typeIfLj4EEPKfS3_l8StepArgs"


def _vmcnt(ln):
    m = re.search(r"\bvmcnt\((\d+)\)", ln)
    return int(m.group(1)) if ln.startswith("s_waitcnt") and m else None


def _entry(body):
    # the compatibility prologue (argument loads for firmware without preload) ends in the first
    # s_branch; the preloaded entry follows it
    return next(j for j, ln in enumerate(body) if ln.startswith("s_branch")) + 1


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LLVM_OBJDUMP):
        pytest.skip("ROCm llvm-objdump not present")
    return dict(_kernels(_disassemble(build_lib(False))))


def test_headline_prologue_waits_are_counted(kernels):
    body = kernels[HEADLINE]
    body = body[_entry(body):]
    state = 0
    at16 = None
    for j, ln in enumerate(body):
        if ln.startswith("global_load_dwordx4"):
            state += 1
            if state == 16:
                at16 = j
                break
    assert at16 is not None, "fewer than 16 state loads (%d)" % state
    first = next(ln for ln in body[at16 + 1:] if ln.startswith("s_waitcnt"))
    assert _vmcnt(first) is not None and _vmcnt(first) > 0, "first wait after the 16th state load: %r" % first
    # no full drain before the frames' first table read (the first LDS read past the barrier)
    bar = next(j for j, ln in enumerate(body) if ln.startswith("s_barrier"))
    read = next(j for j, ln in enumerate(body) if j > bar and ln.startswith("ds_read"))
    drains = [ln for ln in body[:read] if _vmcnt(ln) == 0]
    assert not drains, "vmcnt(0) before the first table read: %r" % drains[:3]
    # ... and the columns the frames read late are still counted there: some wait past the barrier
    # leaves loads in flight
    assert any((_vmcnt(ln) or 0) > 0 for ln in body[bar:read + 400]), "no counted wait after the barrier"


def test_counted_wait_before_the_barrier_covers_the_dmas(kernels):
    """Every step kernel: where the wait in front of the first barrier is a counted one, at least
    that many plain loads were issued behind the last LDS-DMA -- so the DMAs, the oldest entries,
    have landed when the barrier publishes the staging."""
    seen = counted = 0
    for name, body in kernels.items():
        if "f16_step_" not in name:
            continue
        seen += 1
        body = body[_entry(body):]
        bar = next((j for j, ln in enumerate(body) if ln.startswith("s_barrier")), None)
        dmas = [j for j, ln in enumerate(body[:bar]) if ln.startswith("global_load_lds")]
        if bar is None or not dmas:
            continue
        waits = [(j, _vmcnt(ln)) for j, ln in enumerate(body[:bar]) if j > dmas[-1] and _vmcnt(ln) is not None]
        assert waits, "%s: no vector-memory wait between the staging DMAs and the barrier" % name
        j, k = min(waits, key=lambda w: w[1])  # the strictest wait decides what has landed
        behind = sum(1 for ln in body[dmas[-1] + 1:j] if ln.startswith("global_load_dword"))
        assert behind >= k, "%s: vmcnt(%d) with %d loads behind the last DMA" % (name, k, behind)
        counted += k > 0
    assert seen >= 40 and counted >= 1, (seen, counted)
