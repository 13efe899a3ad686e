"""The observation's angle normalisation without fp64 on the ordinary path (f16_env_layer.h euler_norm)
against the fp64 normalize_angle_mpi_pi it replaces (norm_angle): a numpy restatement of both.

The device code passes phi, theta and a non-negative psi through untouched, and gives a psi that
euler() wrapped by 2*PI_F the form (float)((double)psi - 2*pi), whenever every lane of the wave
has ANGLE_ORD_MIN <= |a| < ANGLE_ORD_END for its three polynomial-atan2 results; any other wave
runs norm_angle itself. So the claims to check are: norm_angle is the identity, bit for bit, on
every float32 that satisfies the predicate; the predicate never admits a NaN or an infinity; and
on [PI_F, 2*PI_F] norm_angle is that one subtraction. Exact equality, the sign of zero included.
CPU only."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "f16_jsb_amd", "csrc")
f32, f64, u32 = np.float32, np.float64, np.uint32

PI_F = f32(3.14159265358979323846)
PI_D = f64(3.14159265358979323846)
TWO_PI_F = f32(2.0) * PI_F  # the device's 2.0f * PI_F (exact doubling)
ORD_MIN = f32(2.0 ** -24)
ORD_END = PI_F
ULPS = 4096


def bits(a):
    return np.asarray(a, f32).view(u32)


def norm_angle_ref(a):
    """f16_env_layer.h norm_angle: the fp64 form, on float32 values."""
    a = np.asarray(a, f32)
    bad = np.isnan(a) | np.isinf(a)
    x = np.where(bad, f64(0.0), a.astype(f64))
    big = ~(np.abs(x) < f64(2.0) * PI_D)
    x = np.where(big, np.fmod(x, f64(2.0) * PI_D), x)
    x = np.where(x < 0.0, x + f64(2.0) * PI_D, x)
    x = np.where(x >= PI_D, x - f64(2.0) * PI_D, x)
    x = np.where(x == 0.0, f64(0.0), x)
    return np.where(bad, f32(0.0), x.astype(f32)).astype(f32)


def ordinary(a):
    """angle_ordinary: false for NaN and Inf."""
    with np.errstate(invalid="ignore"):
        m = np.abs(np.asarray(a, f32))
        return (m >= ORD_MIN) & (m < ORD_END)


def psi_wrapped_new(psi):
    """The ordinary wave's form for a psi that euler() wrapped (p < 0: psi = p + 2*PI_F)."""
    return (np.asarray(psi, f32).astype(f64) - f64(2.0) * PI_D).astype(f32)


def obs_angles_new(phi, tht, p):
    """euler_norm's non-gimbal part per lane (a lane off the ordinary path takes norm_angle, as
    its whole wave does on the device)."""
    phi, tht, p = (np.asarray(v, f32) for v in (phi, tht, p))
    with np.errstate(invalid="ignore"):
        psi = np.where(p < 0, (p + TWO_PI_F).astype(f32), p).astype(f32)
        fast = ordinary(phi) & ordinary(tht) & ordinary(p)
        out_fast = (phi, tht, np.where(p < 0, psi_wrapped_new(psi), p).astype(f32))
    out_ref = tuple(norm_angle_ref(v) for v in (phi, tht, psi))
    return tuple(np.where(fast, a, b).astype(f32) for a, b in zip(out_fast, out_ref)), out_ref, fast


def around(v):
    """Every float32 within ULPS ulps of v, across zero where the walk reaches it."""
    b = int(bits(f32(v)))
    sign, mag = b & 0x80000000, b & 0x7FFFFFFF
    k = np.arange(-ULPS, ULPS + 1, dtype=np.int64) + mag
    same = (k[k >= 0].astype(u32) | u32(sign)).view(f32)
    other = ((-k[k < 0]).astype(u32) | u32(sign ^ 0x80000000)).view(f32)
    return np.concatenate([same, other])


BOUNDARIES = [0.0, 2.0 ** -27, 2.0 ** -26, 2.0 ** -24, float(PI_F) / 2, float(PI_F), float(TWO_PI_F),
              float(np.nextafter(PI_F, f32(0)))]


@pytest.fixture(scope="module")
def samples():
    xs = [around(s * b) for b in BOUNDARIES for s in (1.0, -1.0)] + [around(f32(-0.0))]
    rng = np.random.default_rng(8)
    top = int(bits(TWO_PI_F)) + ULPS  # magnitudes from +0 to a little past 2*PI_F, every exponent
    for sign in (0, 0x80000000):
        xs.append((rng.integers(0, top, 10_000_000, dtype=np.uint32) | u32(sign)).view(f32))
        # ... and as many between the predicate's ends (most of the patterns above are below 2^-24)
        xs.append((rng.integers(int(bits(ORD_MIN)), int(bits(ORD_END)), 10_000_000, dtype=np.uint32) | u32(sign)).view(f32))
        xs.append(rng.uniform(0.0, float(PI_F), 1_000_000).astype(f32) * f32(-1.0 if sign else 1.0))
    xs.append(rng.integers(0, 2 ** 32, 1_000_000, dtype=np.uint32).view(f32))  # NaNs, infinities, huge values
    xs.append(np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], u32).view(f32))
    return np.concatenate(xs)


def test_norm_angle_is_the_identity_on_ordinary_angles(samples):
    o = ordinary(samples)
    assert (o & ~np.signbit(samples)).sum() > 10_000_000 and (o & np.signbit(samples)).sum() > 10_000_000
    np.testing.assert_array_equal(bits(norm_angle_ref(samples[o])), bits(samples[o]))


def test_the_predicate_admits_no_nan_or_infinity(samples):
    bad = ~np.isfinite(samples)
    assert np.isnan(samples).sum() > 1000 and np.isinf(samples).sum() >= 2
    assert not ordinary(samples)[bad].any()


def test_the_predicate_ends_are_where_the_identity_ends():
    """What the slow path is for: values the fp64 form does change, next to the predicate's ends."""
    assert bits(norm_angle_ref(PI_F)) == bits(f32(-3.1415925)) and not ordinary(PI_F)
    assert ordinary(np.nextafter(PI_F, f32(0))) and ordinary(-np.nextafter(PI_F, f32(0)))
    assert not ordinary(-PI_F)
    assert bits(norm_angle_ref(f32(-0.0))) == bits(f32(0.0)) and not ordinary(f32(-0.0)) and not ordinary(f32(0.0))
    assert ordinary(ORD_MIN) and ordinary(-ORD_MIN) and not ordinary(np.nextafter(ORD_MIN, f32(0)))
    # (odd mantissas around 2^-31: their last bits are below the fp64 ulp of 2*pi, 2^-50)
    tiny = np.concatenate([np.array([0xB0000001, 0xAF800003], u32).view(f32), np.array([-1e-30], f32)])
    assert (bits(norm_angle_ref(tiny)) != bits(tiny)).all() and not ordinary(tiny).any()


def test_wrapped_psi_is_one_fp64_subtraction():
    """Every float32 of [PI_F, 2*PI_F], the range of p + 2*PI_F for an ordinary negative p."""
    lo, hi = int(bits(PI_F)), int(bits(TWO_PI_F))
    psi = np.arange(lo, hi + 1, dtype=np.uint32).view(f32)
    assert psi[0] == PI_F and psi[-1] == TWO_PI_F and psi.size > 8_000_000
    np.testing.assert_array_equal(bits(norm_angle_ref(psi)), bits(psi_wrapped_new(psi)))
    # and p + 2*PI_F lands in that range for every ordinary negative p (its ends and a sweep)
    rng = np.random.default_rng(9)
    p = -np.concatenate([np.abs(around(ORD_MIN)), np.abs(around(np.nextafter(PI_F, f32(0)))),
                         rng.uniform(0.0, float(PI_F), 1_000_000).astype(f32)])
    p = p[ordinary(p)]
    w = (p + TWO_PI_F).astype(f32)
    assert p.size > 1_000_000 and (w >= PI_F).all() and (w <= TWO_PI_F).all() and (w == TWO_PI_F).any()


def test_new_observation_angles_equal_the_fp64_form(samples):
    """phi, theta and the unwrapped heading p drawn together: fast lanes and slow lanes."""
    rng = np.random.default_rng(10)
    n = 4_000_000
    pool = samples[np.abs(samples) <= PI_F]  # what the polynomial atan2 can return, and the odd values in it
    phi, tht, p = (pool[rng.integers(0, pool.size, n)] for _ in range(3))
    got, ref, fast = obs_angles_new(phi, tht, p)
    assert fast.sum() > n // 8 and (~fast).sum() > n // 8 and (fast & (p < 0)).sum() > n // 32
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(bits(g), bits(r))


def test_constants_are_the_headers():
    src = open(os.path.join(CSRC, "f16_device.h")).read()
    pi = re.search(r"static constexpr float PI_F = ([0-9.]+)f;", src).group(1)
    assert f32(float(pi)) == PI_F
    lo = re.search(r"static constexpr float ANGLE_ORD_MIN = ([0-9.eE+-]+)f;", src).group(1)
    assert f32(float(lo)) == ORD_MIN and float(lo) == 2.0 ** -24
    assert re.search(r"static constexpr float ANGLE_ORD_END = PI_F;", src)
    env = open(os.path.join(CSRC, "f16_env_layer.h")).read()
    # the device predicate is the one restated here, and the wrapped form the one subtraction
    assert re.search(r"m >= ANGLE_ORD_MIN && m < ANGLE_ORD_END", env)
    assert re.search(r"\(float\)\(\(double\)\(p \+ 2\.0f \* PI_F\) - 2\.0 \* PI_D\)", env)
