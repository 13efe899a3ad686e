"""The windowed table bracket (f16_device.h bracket_window) against the full sign-bit count
(bracket): a numpy float32 emulation of both for the alpha, beta13 and union Mach grids of the
aerodynamic tables and the windows the device code uses (the WIN_* indices and the constant part
are read from the header). Wherever the wave-uniform predicate x > lo && x <= hi holds for a lane
the two counts must be the same number; a NaN or an infinity never satisfies it, so a wave that
holds one takes the full count. CPU only."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "f16_jsb_amd", "csrc")
f32 = np.float32

GRIDS = {"BP_alpha_bp": ("WIN_ALPHA_LO", "WIN_ALPHA_HI"), "BP_beta13_bp": ("WIN_BETA_LO", "WIN_BETA_HI"),
         "BP_machu": ("WIN_MACH_LO", "WIN_MACH_HI")}


def _bp(name):
    src = open(os.path.join(CSRC, "f16_tables.h")).read()
    m = re.search(r"static constexpr float %s\[(\d+)\] = \{([^}]*)\};" % name, src)
    return np.array([float(v.strip().rstrip("f")) for v in m.group(2).split(",")], dtype=np.float32)


def _window(name):
    src = open(os.path.join(CSRC, "f16_device.h")).read()
    lo, hi = (int(re.search(r"\b%s = (\d+)" % w, src).group(1)) for w in GRIDS[name])
    return lo, hi


def _signbits(bp, ks, x):
    # c += __float_as_uint(bp[k] - x) >> 31, the float32 difference rounded to nearest
    c = np.zeros(x.shape, np.int64)
    with np.errstate(invalid="ignore"):
        for k in ks:
            c += ((f32(bp[k]) - x).astype(np.float32).view(np.uint32) >> 31).astype(np.int64)
    return c


def full_count(bp, x):
    return 1 + _signbits(bp, range(1, len(bp) - 1), x)


def window_const(n, klo):  # bracket_window_const: #{k in 1..n-2 : k <= klo}
    return klo if 0 < klo < n - 2 else (0 if klo <= 0 else n - 2)


def window_count(bp, klo, khi, x):
    n = len(bp)
    return 1 + window_const(n, klo) + _signbits(bp, range(max(klo + 1, 1), min(khi, n - 1)), x)


def in_window(bp, klo, khi, x):
    with np.errstate(invalid="ignore"):
        return (x > bp[klo]) & (x <= bp[khi])  # the device tests the negation of exactly this


def _neighbours(v):
    v = f32(v)
    return [v, np.nextafter(v, f32(-np.inf)), np.nextafter(v, f32(np.inf))]


def _samples(bp, klo, khi):
    xs = []
    for b in bp:
        xs += _neighbours(b)
    xs += _neighbours(bp[klo]) + _neighbours(bp[khi])
    xs += [f32(0.0), f32(-0.0)]
    tiny = np.array([1, 2, 0x7FFFFF, 0x800000], np.uint32)  # denormals and the smallest normal
    xs += list(tiny.view(np.float32)) + list((tiny | np.uint32(0x80000000)).view(np.float32))
    special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32)
    xs += list(special.view(np.float32))
    span = float(bp[-1]) - float(bp[0])
    rnd = np.random.default_rng(7).uniform(float(bp[0]) - span, float(bp[-1]) + span, 100_000).astype(np.float32)
    return np.concatenate([np.array(xs, np.float32), rnd])


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_window_count_equals_full_count_inside_the_window(name):
    bp = _bp(name)
    klo, khi = _window(name)
    assert 0 <= klo < khi <= len(bp) - 1
    x = _samples(bp, klo, khi)
    inside = in_window(bp, klo, khi, x)
    assert inside.sum() > 1000 and (~inside).sum() > 1000  # both sides of the predicate are sampled
    np.testing.assert_array_equal(window_count(bp, klo, khi, x)[inside], full_count(bp, x)[inside])
    # ... and the sign-bit count is FGTable's count of interior breakpoints below x there
    cmp_count = 1 + (bp[1:len(bp) - 1][None, :] < x[inside][:, None]).sum(axis=1)
    np.testing.assert_array_equal(full_count(bp, x)[inside], cmp_count)
    # the window's ends: lo itself is outside (x > lo), hi inside (x <= hi)
    assert not in_window(bp, klo, khi, np.array([bp[klo]]))[0] and in_window(bp, klo, khi, np.array([bp[khi]]))[0]


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_non_finite_x_is_never_in_the_window(name):
    bp = _bp(name)
    klo, khi = _window(name)
    x = _samples(bp, klo, khi)
    bad = ~np.isfinite(x)
    assert bad.sum() >= 6 and np.isnan(x).sum() >= 4 and np.signbit(x[np.isnan(x)]).any()
    assert not in_window(bp, klo, khi, x)[bad].any()


def test_windows_are_the_documented_breakpoints():
    a, b, m = (_bp(n) for n in ("BP_alpha_bp", "BP_beta13_bp", "BP_machu"))
    (al, ah), (bl, bh), (ml, mh) = (_window(n) for n in ("BP_alpha_bp", "BP_beta13_bp", "BP_machu"))
    assert (a[al], a[ah]) == (f32(-0.175), f32(0.349))
    assert (b[bl], b[bh]) == (f32(-0.175), f32(0.175))
    assert (m[ml], m[mh]) == (f32(0.4), f32(1.0))
