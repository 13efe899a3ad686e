"""Bit identity of the env layer's fast paths (f16_env_layer.h euler_norm, env_reward_sel).

The one-wave-per-SIMD kernels take the observation's Euler angles through one wave-uniform test
(no gimbal pole, every angle "ordinary": straight-line code, no fp64 normalisation) and the
reward / termination as selects; neither may change a result bit. A reference library is built
from the same source with -DF16_ENV_LAYER_REF (euler + norm_angle and the branching env_reward in
every kernel); the product, the -O1 and the debug builds must reproduce its sha256 of state,
observation, rewards, flags, ep_return and ep_len for every case of tests/env_layer_run.py, and
the product's two-waves-per-SIMD kernels (F16ENV_OCC=2, which keep the reference forms) must hash
like its one-wave kernels. The set_state cases must have reached every slow path: asserted on the
reference build's own output, so a workload that misses one fails instead of passing vacuously."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_FLAGS = ("-DF16_ENV_LAYER_REF",)
SET_STATE = ("set_state_window_k4", "set_state_contiguous_k1")


def _run(lib_path, occ=None):
    env = dict(os.environ, F16ENV_LIB=lib_path)
    env.pop("F16ENV_OCC", None)
    if occ:
        env["F16ENV_OCC"] = str(occ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "env_layer_run.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, "%s\n--- stdout tail:\n%s\n--- stderr tail:\n%s" % (
        os.path.basename(lib_path), r.stdout[-600:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def results(gpu):
    from f16_jsb_amd.build import OUT, OUT_DEBUG, OUT_O1, build
    for p in (OUT, OUT_O1, OUT_DEBUG):
        assert os.path.exists(p), "build it: python -m f16_jsb_amd.build [--o1 | --debug] (or __graft_entry__.build())"
    ref = build(extra=REF_FLAGS, out=os.path.join(ROOT, "f16_jsb_amd", "libf16env_ab_envref.so"))
    return {"ref": _run(ref), "product": _run(OUT), "o1": _run(OUT_O1), "debug": _run(OUT_DEBUG),
            "product_occ2": _run(OUT, occ=2)}


def _diff(got, ref):
    assert sorted(got) == sorted(ref)
    return {c: (got[c]["sha256"][:16], ref[c]["sha256"][:16]) for c in ref if got[c]["sha256"] != ref[c]["sha256"]}


@pytest.mark.parametrize("lib", ["product", "o1", "debug"])
def test_hashes_equal_the_reference_forms(results, lib):
    diff = _diff(results[lib], results["ref"])
    assert not diff, "%s differs from the -DF16_ENV_LAYER_REF build in %s" % (lib, diff)


def test_two_wave_kernels_hash_like_the_one_wave_kernels(results):
    one, two = results["product"], results["product_occ2"]
    for case in one:
        print(case, one[case]["kernel"], "|", two[case]["kernel"])
    windowed = [c for c in one if "window" in c]
    assert all(", 1," in one[c]["kernel"] and ", 2," in two[c]["kernel"] for c in windowed), \
        [(one[c]["kernel"], two[c]["kernel"]) for c in windowed]
    diff = _diff(two, one)
    assert not diff, "two-waves-per-SIMD kernels differ from the one-wave kernels in %s" % diff


def test_debug_build_records_no_violation(results):
    for case, r in results["debug"].items():
        assert r["is_debug"] == 1 and r["violations"] == 0, (case, r)
    assert all(r["is_debug"] == 0 for r in results["product"].values())


def test_workload_reaches_every_path(results):
    ref = results["ref"]
    for case, r in ref.items():
        print(case, r["kernel"], {k: r[k] for k in ("terminated", "truncated", "crashed", "nonfinite")}, r.get("classes", ""))
    for case in SET_STATE:  # (b): each slow-path class, and a wave that is wholly ordinary
        c = ref[case]["classes"]
        assert c["tiny"] >= 1, (case, "no angle below 2^-24", c)
        assert c["minus_pi"] >= 1, (case, "no angle equal to -3.1415925", c)
        assert c["theta_half_pi"] >= 1, (case, "no |theta| of PI_F/2", c)
        assert c["psi_wrapped_wave0"] >= 1 and c["psi_wrapped_wave1"] >= 1, (case, "no psi above PI_F", c)
        assert c["wave1_ordinary"], (case, "wave 1 is not wholly ordinary", c)
        assert ref[case]["terminated"] == 0 and ref[case]["truncated"] == 0, (case, ref[case])
    for case, r in ref.items():  # (a): every lane truncates four times in 96 steps of max_steps = 24, less its crashes
        if case in SET_STATE:
            continue
        assert r["truncated"] >= 3 * 197 and r["crashed"] >= 1, (case, r)
    assert ref["nan_guard_window_k4"]["nonfinite"] >= 1
    assert results["product"]["nan_guard_window_k4"]["nonfinite"] == ref["nan_guard_window_k4"]["nonfinite"]
    kernels = {r["kernel"] for r in results["product"].values()}
    assert any("win" in k for k in kernels) and len(kernels) >= 4, kernels
