"""Bit identity of the step kernel's counted prologue waits and windowed breakpoint counts.

The product issues its state columns in first-use order and waits for each where it is first
read (f16_step.h step_body); a -DF16_BRACKET_WINDOW build also counts the alpha / beta / Mach
breakpoints over a window when every lane of a wave is inside it (f16_device.h bracket_window;
measured no faster, so not in the product). Neither may change a result bit.
A reference library is built from the same source with both switched off
(-DF16_PROLOGUE_ONE_WAIT -DF16_BRACKET_FULL: one full drain, the full count); the product, the
windowed-count build, the -O1 and the debug builds must reproduce its sha256 of state, observation, rewards and flags for
every case of tests/prologue_window_run.py: n = 197, K = 4 and 1, windowed and contiguous layouts,
cfg5, and a NaN-guarded run with a NaN body rate -- with lanes set outside every window in three
waves (the mixed-wave full path) and one wave wholly inside (the windowed path)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_FLAGS = ("-DF16_PROLOGUE_ONE_WAIT", "-DF16_BRACKET_FULL")
# window ends (f16_device.h WIN_*; tests/test_bracket_window_cpu.py pins them to the header)
ALPHA_WIN, BETA_WIN, MACH_WIN = (-0.175, 0.349), (-0.175, 0.175), (0.4, 1.0)


def _run(lib_path):
    env = dict(os.environ, F16ENV_LIB=lib_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "prologue_window_run.py")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "%s\n--- stdout tail:\n%s\n--- stderr tail:\n%s" % (
        os.path.basename(lib_path), r.stdout[-600:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def results(gpu):
    from f16_jsb_amd.build import OUT, OUT_DEBUG, OUT_O1, build
    for p in (OUT, OUT_O1, OUT_DEBUG):
        assert os.path.exists(p), "build it: python -m f16_jsb_amd.build [--o1 | --debug] (or __graft_entry__.build())"
    ref = build(extra=REF_FLAGS, out=os.path.join(ROOT, "f16_jsb_amd", "libf16env_ab_ref.so"))
    win = build(extra=("-DF16_BRACKET_WINDOW",), out=os.path.join(ROOT, "f16_jsb_amd", "libf16env_ab_window.so"))
    return {"ref": _run(ref), "product": _run(OUT), "window": _run(win), "o1": _run(OUT_O1), "debug": _run(OUT_DEBUG)}


@pytest.mark.parametrize("lib", ["product", "window", "o1", "debug"])
def test_hashes_equal_the_one_wait_full_count_reference(results, lib):
    ref, got = results["ref"], results[lib]
    assert sorted(got) == sorted(ref)
    diff = {c: (got[c]["sha256"][:16], ref[c]["sha256"][:16]) for c in ref if got[c]["sha256"] != ref[c]["sha256"]}
    assert not diff, "%s differs from the reference build in %s" % (lib, diff)


def test_debug_build_records_no_violation(results):
    for case, r in results["debug"].items():
        assert r["is_debug"] == 1 and r["violations"] == 0, (case, r)
    assert all(r["is_debug"] == 0 for r in results["product"].values())


def test_workload_runs_both_bracket_paths(results):
    """The perturbed lanes did leave the windows (their waves take the full count) and every
    other lane stayed inside (wave 3 takes the windowed count); the NaN lane was quarantined."""
    for case, r in results["ref"].items():
        print(case, r["kernel"], "alpha %.4f beta %.4f mach %.4f" % (r["alpha"], r["beta"], r["mach"]),
              "clean", r["clean_alpha"], r["clean_beta_abs"], r["clean_mach"])
        if case.startswith("cfg5"):  # (random initial conditions and gusts: the lanes are where they are)
            continue
        assert not ALPHA_WIN[0] < r["alpha"] <= ALPHA_WIN[1], (case, r["alpha"])
        assert not BETA_WIN[0] < r["beta"] <= BETA_WIN[1], (case, r["beta"])
        assert not MACH_WIN[0] < r["mach"] <= MACH_WIN[1], (case, r["mach"])
        assert ALPHA_WIN[0] < r["clean_alpha"][0] and r["clean_alpha"][1] <= ALPHA_WIN[1], (case, r["clean_alpha"])
        assert r["clean_beta_abs"] < BETA_WIN[1], (case, r["clean_beta_abs"])
        assert MACH_WIN[0] < r["clean_mach"][0] and r["clean_mach"][1] <= MACH_WIN[1], (case, r["clean_mach"])
    assert results["ref"]["nan_guard_window_k4"]["nonfinite"] >= 1
    assert results["product"]["nan_guard_window_k4"]["nonfinite"] == results["ref"]["nan_guard_window_k4"]["nonfinite"]
    kernels = {r["kernel"] for r in results["product"].values()}
    assert any("win" in k for k in kernels) and len(kernels) >= 3, kernels
