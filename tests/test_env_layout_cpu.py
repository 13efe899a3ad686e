"""layouts._Derived, the one place that says whether the windowed layout's feature windows and
pose export are current, walked through its transitions without a GPU and checked against a table
written out from the prose of F16Envs.obs_features' docstring:

  a call after each step transforms one frame per env (incremental); a rollout-slot / fused step
  keeps the windows in its own epilogue when they are current (fused: no launch in the call); the
  first call, a call after a reset, set_state, set_obs or rollout_random, the call after the step
  that follows one of those, and a call after a step not followed by a call transform both whole
  windows (full); a second call without an op between launches nothing."""
from __future__ import annotations

import pytest

from f16_jsb_amd.layouts import _Derived


def _walk(ops):
    """Drive a _Derived the way _WindowLayout does; returns what each "call" (obs_features) and each
    "fstep" (a step that may keep the windows itself) did, and the final counters."""
    d, did = _Derived(), []
    for op in ops:
        if op == "call":
            how = d.features_due()
            if how is not None:
                d.features_written(how)
            did.append(how)
        elif op == "step":
            d.windows_changed(by_step=True)
        elif op == "fstep":
            fw = d.can_fuse_features()
            d.windows_changed(by_step=True)
            if fw:
                d.features_written("fused")
            did.append("fused" if fw else "plain")
        elif op == "write":  # reset, set_state, set_obs, rollout_random
            d.windows_changed(by_step=False)
        else:
            raise AssertionError(op)
    return did, d


TABLE = [
    (["call"], ["full"]),                                                  # the first call
    (["step", "call"], ["full"]),                                          # ... also after a step
    (["call", "call"], ["full", None]),                                    # nothing changed: no launch
    (["step", "call", "step", "call", "step", "call"], ["full", "incremental", "incremental"]),
    (["step", "call", "step", "step", "call"], ["full", "full"]),          # a step not followed by a call
    (["step", "call", "step", "step", "call", "step", "call"], ["full", "full", "incremental"]),
    (["step", "call", "write", "call"], ["full", "full"]),                 # after a reset / set_state / ...
    (["write", "call", "step", "call", "step", "call"], ["full", "full", "incremental"]),  # and the step after it
    (["write", "step", "call", "step", "call"], ["full", "incremental"]),  # reset -> step -> call
    (["step", "call", "write", "step", "call", "step", "call"], ["full", "full", "incremental"]),
    (["step", "call", "fstep", "call", "fstep", "fstep", "call"], ["full", "fused", None, "fused", "fused", None]),
    (["fstep", "call", "fstep"], ["plain", "full", "fused"]),              # never written: the step cannot fuse
    (["step", "call", "write", "fstep", "call", "fstep"], ["full", "plain", "full", "fused"]),
    (["write", "call", "fstep", "call", "fstep"], ["full", "plain", "full", "fused"]),  # no ahead fills after a reset
    (["step", "call", "step", "fstep", "call"], ["full", "plain", "full"]),  # one behind: the step cannot fuse
]


@pytest.mark.parametrize("ops,want", TABLE, ids=["-".join(o) for o, _ in TABLE])
def test_feature_window_rule(ops, want):
    did, d = _walk(ops)
    assert did == want
    assert d.calls == {k: want.count(k) for k in ("incremental", "full", "fused")}


def test_ahead_fills_follow_whole_windows_only_after_a_step():
    d = _Derived()
    assert d.features_written(d.features_due()) is False   # first call, no step before it
    d.windows_changed(by_step=True)
    assert d.features_due() == "full" and d.features_written("full") is True
    d.windows_changed(by_step=False)
    assert d.features_due() == "full" and d.features_written("full") is False
    assert not d.can_fuse_features()


def test_restart_moves_only_current_feature_windows():
    d = _Derived()
    assert not d.histories_restarted()                     # never written
    d.windows_changed(by_step=True)
    d.features_written(d.features_due())
    assert d.histories_restarted()                         # current: they move with the frames
    d.windows_changed(by_step=True)
    assert not d.histories_restarted()                     # stale: rewritten whole or in place later
    assert d.features_due() == "incremental"


def test_poses_current_until_the_windows_change():
    d = _Derived()
    assert not d.poses_current()
    d.windows_changed(by_step=True)
    d.poses_written()
    assert d.poses_current()
    d.features_written(d.features_due())                   # a features call is no window change
    assert d.poses_current()
    for by_step in (True, False):
        d.poses_written()
        d.windows_changed(by_step=by_step)
        assert not d.poses_current()
