"""The state-parity method (tests/state_corners.py) on the CPU oracle alone: the planted states
reach every corner they are meant to, the guard stays under its cap in every case the GPU test
runs, a production step is its frames replayed one by one (the licence for the guard), and the
checker fails on small synthetic defects and names the field (it is not vacuous)."""
from __future__ import annotations

import numpy as np
import pytest

import state_corners as sc
from oracle_ref import OracleEnvs
from state_corners import (DT, F16C_AIL, F16C_AUG, F16C_ELE, F16C_LEF, F16C_N2, F16C_PID_P_I, F16C_PID_R_I,
                           F16C_PID_R_P, F16C_PID_Y_I, F16C_RUD, F16C_SB, F16C_TEF, LIM, LX, NAMES, TEF_STEP)

from f16_jsb_amd.abi import (F16C_EP_RET, F16C_LAST_D, F16C_STEP, F16L_ALPHA, F16L_MACH, F16L_VC_KTS)

MIN_LANES = 16


@pytest.fixture(scope="module")
def one_frame(oracle_lib):
    s, a, g = sc.planted("plain")
    ref, pre, mask, env = sc.oracle_case("plain", 1)
    return s, a, g, ref, mask, env


def _count(name, m):
    assert int(m.sum()) >= MIN_LANES, "%s: %d lanes" % (name, int(m.sum()))


def test_planted_states_are_device_storable(one_frame):
    """Both sides start from bit-identical values: the planted state is a fixed point of the
    device's set_state / get_state encodings (fp32 columns, velocity history as fp32 deltas)."""
    for kind in ("plain", "wind", "cfg5"):
        s = sc.planted(kind)[0]
        rt = sc.device_roundtrip(s)
        keep = [c for c in range(s.shape[1]) if c not in sc.NOT_CARRIED]
        assert np.array_equal(rt[:, keep], s[:, keep]), kind
        assert np.isfinite(s).all()
    # the planted values survive the oracle's own set_state / get_state exactly
    e = OracleEnvs(sc.N_LANES, stack_k=1)
    e.reset(goals=sc.far_goals(sc.N_LANES))
    e.set_state(s)
    got = e.get_state()
    enc = [sc.F16C_EPA_C, sc.F16C_EPA_S]
    keep = [c for c in range(s.shape[1]) if c not in enc]
    assert np.array_equal(got[:, keep], s[:, keep])
    np.testing.assert_allclose(got[:, enc], s[:, enc], rtol=0, atol=1e-15)


def test_coverage_after_one_frame(one_frame):
    s, a, g, ref, mask, env = one_frame
    d = ref - s
    # TEF: the three wave kinds, from the planted state (the skip is a wave ballot over "on detent")
    vc, mach = s[:, LX + F16L_VC_KTS], s[:, LX + F16L_MACH]
    target = np.where(vc < 250.0, sc.TEF_POS, np.where(mach > 0.9, sc.TEF_NEG, 0.0))
    on = (s[:, F16C_TEF] == target)[:64 * (sc.N_LANES // 64)].reshape(-1, 64).sum(axis=1)
    assert (on == 64).sum() >= 4 and (on == 0).sum() >= 4 and ((on > 0) & (on < 64)).sum() >= 4
    tef0, tef1 = s[:, F16C_TEF], ref[:, F16C_TEF]
    moved = tef1 != tef0
    _count("TEF partial move", np.isclose(np.abs(tef1 - tef0), TEF_STEP, rtol=1e-6, atol=0))
    _count("TEF jump from below 0", moved & (tef0 < 0))
    _count("TEF jump through 0 (second pass)", moved & (tef0 > 0) & (tef1 < 0))
    _count("TEF jump from 0", moved & (tef0 == 0) & (tef1 < 0))
    _count("TEF hold", ~moved)
    # PID integrators: integrating and holding
    for c in (F16C_PID_R_I, F16C_PID_P_I, F16C_PID_Y_I):
        _count(NAMES[c] + " integrating", d[:, c] != 0)
        _count(NAMES[c] + " holding", d[:, c] == 0)
        _count(NAMES[c] + " saturating", np.abs(s[:, c]) >= 1.5)
    # actuators: rate-limited, landing, holding at a clamp
    for c in (F16C_AIL, F16C_ELE, F16C_RUD, F16C_LEF, F16C_SB):
        step = np.abs(d[:, c])
        clamp = (np.abs(s[:, c]) == 1.0) if c != F16C_SB else ((s[:, c] == 0.0) | (s[:, c] == 60.0))
        _count(NAMES[c] + " rate-limited", np.isclose(step, LIM[c], rtol=1e-6, atol=0))
        _count(NAMES[c] + " landing", (step > 0) & (step < LIM[c] * (1 - 1e-6)))
        _count(NAMES[c] + " holding at a clamp", (step == 0) & clamp)
    for c in (F16C_AIL, F16C_ELE, F16C_RUD):  # both clamps
        _count(NAMES[c] + " holding at -1", (d[:, c] == 0) & (s[:, c] == -1.0))
        _count(NAMES[c] + " holding at +1", (d[:, c] == 0) & (s[:, c] == 1.0))
    _count("speedbrake target > 0", d[:, F16C_SB] > 0)
    _count("speedbrake held at 60", (d[:, F16C_SB] == 0) & (s[:, F16C_SB] == 60.0))
    # engine
    for prev in (0.0, 1.0):
        for new in (0.0, 1.0):
            _count("AUG %d -> %d" % (prev, new), (s[:, F16C_AUG] == prev) & (ref[:, F16C_AUG] == new))
    n2t = 60.0 + 40.0 * np.minimum(2.0 * a[:, 3].astype(np.float64), 1.0)
    _count("N2 accelerating", (d[:, F16C_N2] > 0) & (ref[:, F16C_N2] < n2t))
    _count("N2 decelerating", (d[:, F16C_N2] < 0) & (ref[:, F16C_N2] > n2t))
    _count("N2 landing", (d[:, F16C_N2] != 0) & (ref[:, F16C_N2] == n2t))
    _count("N2 on its target", (d[:, F16C_N2] == 0) & (s[:, F16C_N2] == n2t))
    _count("N2 with nn clamped", s[:, F16C_N2] >= 96.0)
    # latch switches: both sides of each
    al = s[:, LX + F16L_ALPHA]
    for t in (sc.A1, sc.A2, sc.A3):
        _count("alpha just below %.4f" % t, (al < t) & (al > 0.98 * t))
        _count("alpha just above %.4f" % t, (al > t) & (al < 1.02 * t))
    for v in (3.0, 7.0, 15.0, 25.0, 200.0, 260.0):
        _count("vc %g" % v, np.isclose(vc, v, rtol=1e-6))


@pytest.mark.parametrize("case", sc.ORACLE_CASES, ids=lambda c: "%s-ds%d-steps%d" % c)
def test_guard_cap(oracle_lib, case):
    """A condition, not a measurement: at most 2 % of lanes guarded in any case the GPU test runs;
    no lane done (replay asserts it per step), the oracle's states finite, the step counted."""
    kind, ds, steps = case
    ref, pre, mask, env = sc.oracle_case(*case)
    assert mask.mean() <= sc.GUARD_CAP, "%.2f %% of lanes guarded" % (100 * mask.mean())
    assert len(pre) == ds * steps
    assert np.isfinite(ref).all() and np.isfinite(env).all()
    assert np.all(ref[:, F16C_STEP] == sc.planted(kind)[0][:, F16C_STEP] + steps)
    # planted values keep their distance by construction: nothing guarded before the first frame
    assert not sc.guarded(pre[:1], sc.planted(kind)[1]).any()


@pytest.mark.parametrize("kind", ["plain", "cfg5"])
def test_replay_identity(oracle_lib, kind):
    """One down_sample=4 step equals four single-frame steps bit for bit on the physics fields
    (the step count, return and last distance belong to the env layer, which runs per step)."""
    s, a, _ = sc.planted(kind)
    final, pre = sc.replay(s, a, 4, 1, cfg5=kind == "cfg5", seed=sc.SEED)
    last = sc._one_frame(pre[3], a)
    phys = [c for c in range(s.shape[1]) if c not in (F16C_STEP, F16C_EP_RET, F16C_LAST_D)]
    assert np.array_equal(last[:, phys], final[:, phys])
    assert np.array_equal(pre[0], s[:, :]) or np.allclose(pre[0], s, rtol=0, atol=1e-15)  # (Earth angle re-encoded)


def _defect_cases(s, a, ref):
    d = ref - s
    out = {}
    # an aileron that moved 1.01 x one frame's travel
    m = np.isclose(np.abs(d[:, F16C_AIL]), LIM[F16C_AIL], rtol=1e-6, atol=0)
    g = ref.copy()
    g[m, F16C_AIL] = s[m, F16C_AIL] + 1.01 * d[m, F16C_AIL]
    out["AIL"] = (g, m)
    # a roll integrator that integrated where the trigger says hold (ki dt err; err = the new
    # previous input)
    m = s[:, LX + F16L_VC_KTS] >= 20.0
    g = ref.copy()
    g[m, F16C_PID_R_I] += 0.0005 * DT * ref[m, F16C_PID_R_P]
    out["PID_R_I"] = (g, m)
    # N2 spooled down at the acceleration rate (a third of the deceleration rate)
    n2t = 60.0 + 40.0 * np.minimum(2.0 * a[:, 3].astype(np.float64), 1.0)
    m = (d[:, F16C_N2] < 0) & (ref[:, F16C_N2] > n2t)
    g = ref.copy()
    g[m, F16C_N2] = s[m, F16C_N2] + d[m, F16C_N2] / 3.0
    out["N2"] = (g, m)
    # an AUG flag not cleared
    m = (s[:, F16C_AUG] == 1.0) & (ref[:, F16C_AUG] == 0.0)
    g = ref.copy()
    g[m, F16C_AUG] = 1.0
    out["AUG"] = (g, m)
    # a TEF that moved dt/3 toward a negative target instead of jumping
    m = (s[:, F16C_TEF] >= 0) & (ref[:, F16C_TEF] < 0)
    g = ref.copy()
    g[m, F16C_TEF] = s[m, F16C_TEF] - TEF_STEP
    out["TEF"] = (g, m)
    # a latch alpha taken from the previous frame
    g = ref.copy()
    g[:, LX + F16L_ALPHA] = s[:, LX + F16L_ALPHA]
    out["LX_ALPHA"] = (g, np.ones(len(s), bool))
    return out


def test_checker_passes_the_reference_and_names_each_defect(one_frame):
    s, a, _, ref, mask, env = one_frame
    rep = sc.check_state(ref.copy(), ref, env, mask)
    assert rep["failed"] == [] and all(v["ratio"] == 0 for k, v in rep.items() if k != "failed")
    for field, (got, lanes) in _defect_cases(s, a, ref).items():
        assert int(lanes.sum()) >= MIN_LANES, field
        rep = sc.check_state(got, ref, env, mask)
        assert rep["failed"] == [field], (field, rep["failed"])
        assert lanes[rep[field]["lane"]]
    # a single defective lane is enough, and a guarded lane's value is not compared while its
    # flags still are
    lane = int(np.flatnonzero(~mask)[5])
    got = ref.copy()
    got[lane, F16C_ELE] += 2e-5
    rep = sc.check_state(got, ref, env, mask)
    assert rep["failed"] == ["ELE"] and rep["ELE"]["lane"] == lane
    m2 = mask.copy()
    m2[lane] = True
    assert sc.check_state(got, ref, env, m2)["failed"] == []
    got[lane, F16C_AUG] = 1.0 - got[lane, F16C_AUG]
    assert sc.check_state(got, ref, env, m2)["failed"] == ["AUG"]
    # fields the device does not carry must read 0 there
    assert sc.check_state(ref.copy(), ref, env, mask, not_carried_zero=True)["failed"] != []
    got = ref.copy()
    got[:, sc.NOT_CARRIED] = 0.0
    assert sc.check_state(got, ref, env, mask, not_carried_zero=True)["failed"] == []


def test_one_ulp_keeps_exact_zeros(one_frame):
    s = one_frame[0]
    p = sc.one_ulp(s, np.random.default_rng(1))
    f = sc.F32_FIELDS
    zero = s[:, f] == 0
    assert zero.any() and np.all(p[:, f][zero] == 0)
    moved = np.abs(p[:, f][~zero] - s[:, f][~zero])
    assert np.all(moved > 0) and np.all(moved <= sc.ulp32(s[:, f][~zero]) * 1.0000001)


def test_floors_are_fp32_ulps(one_frame):
    """4 fp32 ulps at the field's range: 4.8e-7 for a normalised actuator, 1.5e-5 deg for the
    speedbrake, 3.1e-5 % for N2 (the numbers the issue derives)."""
    ref = one_frame[3]
    fl = sc.floors(ref)
    for c in (F16C_TEF, F16C_AIL, F16C_ELE, F16C_RUD, F16C_LEF, F16C_PID_R_P):
        small = np.abs(ref[:, c]) <= 1.0
        assert np.all(fl[small, c] == 4 * 2.0 ** -23) and np.all(fl[:, c] <= 8 * 2.0 ** -23)
    assert np.all(fl[:, F16C_SB] == 4 * 2.0 ** -18) and np.all(fl[:, F16C_N2] == 4 * 2.0 ** -17)
