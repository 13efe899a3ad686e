// f16_rng.h -- Philox4x32-10 and the streams drawn from it (goals, random ICs, gust normals, the
// uniform random policy's actions), the same stream definitions as oracle/f16ref.c, and numpy's
// clip of an action to the Box. Device code only. Needs f16_device.h (PI_D) and include/f16env.h
// (the F16_IC_* indices).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/f16env.h"
#include "f16_device.h"

using namespace f16;

// ------------------------------------------------------------------------------------------
// Philox4x32-10 (same stream definition as oracle/f16ref.c)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1,
                                       uint32_t c2, uint32_t c3, uint32_t* o) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
    const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}
// goal RNG: jsbsim_gym.py:312-323 formula on a Philox stream keyed by (seed; gid, episode)
__device__ __forceinline__ void rng_goal(uint64_t seed, uint64_t gid, uint32_t ep, float* g) {
  uint32_t o[4], o2[4];
  philox((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gid, (uint32_t)(gid >> 32), ep,
         0x474F414Cu, o);
  philox((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gid, (uint32_t)(gid >> 32), ep,
         0x474F414Cu ^ 1u, o2);
  const double dist = 1000.0 + (10000.0 - 1000.0) * u53(o[0], o[1]);
  const double bear = 0.0 + (2.0 * PI_D - 0.0) * u53(o[2], o[3]);
  const double alt = 1000.0 + (4000.0 - 1000.0) * u53(o2[0], o2[1]);
  double sb, cb;
  sincos(bear, &sb, &cb);  // one argument reduction for both (same values as cos / sin)
  g[0] = (float)(dist * cb);
  g[1] = (float)(dist * sb);
  g[2] = (float)alt;
}

// cfg5 random IC (include/f16env.h F16_FLAG_RANDOM_IC), mirrors oracle rng_ic()
__device__ void rng_ic(uint64_t seed, uint64_t gid, uint32_t ep, const double* lo, const double* hi, double* ic) {
  uint32_t o[4];
#pragma unroll  // constant indices: ic[] and o[] stay in registers (no scratch)
  for (int j = 0; j < F16_IC_N; ++j) {
    if ((j & 3) == 0)
      philox((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gid, (uint32_t)(gid >> 32), ep,
             0x52494300u + (uint32_t)(j >> 2), o);
    const double u = ((double)o[j & 3] + 0.5) * (1.0 / 4294967296.0);
    ic[j] = lo[j] + (hi[j] - lo[j]) * u;
  }
}
// cfg5 gust noise: three Box-Muller normals (fp32), mirrors oracle rng_normals() (fp64)
__device__ __forceinline__ void rng_normals(uint64_t seed, uint64_t gid, uint32_t ep, uint32_t s, float* xi) {
  uint32_t o[4];
  philox((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gid, (uint32_t)(gid >> 32) ^ 0x47555354u, ep, s, o);
  const float s24 = 1.0f / 16777216.0f;
  const float u1 = ((float)(o[0] >> 8) + 0.5f) * s24, u2 = (float)(o[1] >> 8) * s24;
  const float u3 = ((float)(o[2] >> 8) + 0.5f) * s24, u4 = (float)(o[3] >> 8) * s24;
  const float r1 = sqrtf(-2.0f * logf(u1)), r2 = sqrtf(-2.0f * logf(u3));
  float s2, c2, s4, c4;
  sincospif(2.0f * u2, &s2, &c2);
  sincospif(2.0f * u4, &s4, &c4);
  xi[0] = r1 * c2;
  xi[1] = r1 * s2;
  xi[2] = r2 * c4;
}

// uniform action over the Box [-1,-1,-1,0]..[1,1,1,1] (jsbsim_gym.py:143-148) keyed by
// (seed; global env id, step): the f16env_sample_actions stream, also drawn in-kernel by the
// rollout step
__device__ __forceinline__ float4 philox_action(uint64_t seed, uint64_t gid, uint64_t step) {
  uint32_t o[4];
  philox((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)step,
         (uint32_t)(step >> 32), o);
  const float lo[4] = {-1.f, -1.f, -1.f, 0.f}, hi[4] = {1.f, 1.f, 1.f, 1.f};
  float4 v;
  float* pv = &v.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float u = (float)(o[j] >> 8) * (1.0f / 16777216.0f);
    pv[j] = lo[j] + (hi[j] - lo[j]) * u;
  }
  return v;
}

// np.clip(actions, action_space.low, action_space.high) (on_policy_algorithm.py:216: SB3 clips
// the policy's Gaussian sample to the Box before env.step) on float32, as numpy's clip ufunc
// computes it: min(max(x, lo), hi) with max(a, b) = isnan(a) ? a : (a > b ? a : b) and min
// likewise with < (numpy/_core/src/umath/clip.cpp _NPY_CLIP): NaN passes through, -0 clips to +0
// at a 0 bound
__device__ __forceinline__ float np_clip(float x, float lo, float hi) {
  const float m = (x != x) ? x : (x > lo ? x : lo);
  return (m != m) ? m : (m < hi ? m : hi);
}
__device__ __forceinline__ float4 clip_box(float4 a) {  // Box [-1,-1,-1,0]..[1,1,1,1] (jsbsim_gym.py:143-148)
  return make_float4(np_clip(a.x, -1.0f, 1.0f), np_clip(a.y, -1.0f, 1.0f), np_clip(a.z, -1.0f, 1.0f),
                     np_clip(a.w, 0.0f, 1.0f));
}
