// f16_rollout_data.h -- what a PPO rollout's arrays need besides the env steps: the random policy's
// action draws (the sample-actions kernels), GAE, the timeout bootstrap (direct, and deferred by
// stash / apply) and the minibatch sampler (MbArgs, f16_minibatch_kernel); below each handle-free
// kernel the launcher behind its entry point (f16env_gae, _bootstrap_timeouts, _bootstrap_stash,
// _bootstrap_apply, _rollout_minibatch). The sample-actions launches take the handle and are in
// f16env.hip.
// Needs f16_host.h (set_err, HIPCHK, env_int), f16_rng.h (philox_action), f16_stage.h (BLOCK) and
// f16_device.h (st16, F16_CHECK).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/f16env.h"
#include "f16_device.h"
#include "f16_host.h"
#include "f16_rng.h"
#include "f16_stage.h"

using namespace f16;

__global__ void f16_sample_actions_kernel(int64_t n, int64_t id_base, uint64_t seed, uint64_t step, float* act) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  reinterpret_cast<float4*>(act)[k] = philox_action(seed, (uint64_t)(id_base + k), step);
}
// T steps' actions in one launch (f16env_sample_actions_steps, ABI 6): act[t][k] for t < T, the
// same draws as T calls of f16env_sample_actions. One 1-MB batch per launch (65 536 envs) is a
// launch-latency-bound kernel (~0.8 us over an empty launch, at 1 wave per SIMD); here each lane
// draws SA_PER_LANE float4 at a grid stride, so the whole T x N block fills the chip and streams
// out as coalesced 1-KiB wave stores.
constexpr int SA_PER_LANE = 4;
__global__ __launch_bounds__(BLOCK) void f16_sample_actions_steps_kernel(int64_t n, int64_t total, int64_t id_base,
                                                                        uint64_t seed, uint64_t step0, float* act) {
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
#pragma unroll
  for (int u = 0; u < SA_PER_LANE; ++u, i += stride) {
    if (i < total) {
      const int64_t t = i / n, k = i - t * n;
      st16<true>(reinterpret_cast<float4*>(act) + i, philox_action(seed, (uint64_t)(id_base + k), step0 + (uint64_t)t));
    }
  }
}

// GAE(lambda) over a [n_steps][n_envs] rollout, one lane per env, backward in time.
// Restates stable_baselines3/common/buffers.py:403-438 (RolloutBuffer.
// compute_returns_and_advantage) with numpy's float32 per-operation rounding: every product
// and sum is rounded separately (no FMA), gamma and gamma*lambda are rounded to float32
// exactly as numpy casts a Python float against a float32 array.
// The recurrence is serial per env (bit-exactness forbids reassociating it into a scan), and at
// cfg4's 32 768 envs one lane per env is only 512 waves, each walking 2 048 steps. Its loads do
// not depend on the chain, so they are software-pipelined: the rewards / values / starts of the
// next block of U steps are issued before the current block is computed, keeping ~2U steps of
// loads in flight per lane (round 3's loop waited on each step's three loads in turn: 0.13 of
// HBM peak). LPW lanes of each 64-lane wave carry an env (64: full waves, gae_impl below).
// Streaming data: non-temporal loads and stores.
template <int U>
__device__ __forceinline__ void gae_load(int64_t s0, int64_t n_envs, int64_t e, const float* __restrict__ rewards,
                                         const float* __restrict__ values, const float* __restrict__ ep_starts,
                                         float (&r)[U], float (&v)[U], float (&st)[U]) {
#pragma unroll
  for (int i = 0; i < U; ++i) {
    const int64_t idx = (s0 + i) * n_envs + e;
    r[i] = __builtin_nontemporal_load(rewards + idx);
    v[i] = __builtin_nontemporal_load(values + idx);
    st[i] = __builtin_nontemporal_load(ep_starts + idx);
  }
}
template <int U, int LPW>
__global__ __launch_bounds__(64) void f16_gae_kernel(int64_t n_steps, int64_t n_envs, const float* __restrict__ rewards,
                                                     const float* __restrict__ values, const float* __restrict__ ep_starts,
                                                     const float* __restrict__ last_values, const uint8_t* __restrict__ dones,
                                                     float g, float gl, float* __restrict__ adv, float* __restrict__ ret) {
  // float32 per-op rounding as numpy (no FMA contraction; __f*_rn still contract under -O3)
#pragma clang fp contract(off)
  if ((int)threadIdx.x >= LPW) return;
  const int64_t e = (int64_t)blockIdx.x * LPW + threadIdx.x;
  if (e >= n_envs) return;
  float lgl = 0.0f;
  float nv = last_values[e];
  float nnt = 1.0f - (dones[e] ? 1.0f : 0.0f);
  // one backward step of buffers.py:425-436 at step s
  auto step = [&](int64_t s, float r, float v, float st) {
#pragma clang fp contract(off)
    const int64_t i = s * n_envs + e;
    const float t2 = (g * nv) * nnt;
    const float delta = (r + t2) - v;
    lgl = delta + (gl * nnt) * lgl;
    __builtin_nontemporal_store(lgl, adv + i);
    __builtin_nontemporal_store(lgl + v, ret + i);
    nv = v;
    nnt = 1.0f - st;
  };
  const int64_t nb = n_steps / U;  // whole blocks [b U, b U + U); the n_steps % U last steps first
  for (int64_t s = n_steps - 1; s >= nb * U; --s) {
    const int64_t i = s * n_envs + e;
    step(s, rewards[i], values[i], ep_starts[i]);
  }
  if (nb == 0) return;
  float r0[U], v0[U], s0[U];
  gae_load<U>((nb - 1) * U, n_envs, e, rewards, values, ep_starts, r0, v0, s0);
  for (int64_t b = nb - 1; b >= 0; --b) {
    float r1[U], v1[U], s1[U];
    if (b > 0) gae_load<U>((b - 1) * U, n_envs, e, rewards, values, ep_starts, r1, v1, s1);  // next block in flight
#pragma unroll
    for (int i = U - 1; i >= 0; --i) step(b * U + i, r0[i], v0[i], s0[i]);
    if (b > 0) {
#pragma unroll
      for (int i = 0; i < U; ++i) { r0[i] = r1[i]; v0[i] = v1[i]; s0[i] = s1[i]; }
    }
  }
}

static int gae_impl(void* stream, int64_t n_steps, int64_t n_envs, const float* rewards, const float* values,
                    const float* episode_starts, const float* last_values, const uint8_t* dones, double gamma,
                    double gae_lambda, float* advantages, float* returns) {
  if (n_steps <= 0 || n_envs <= 0) return set_err(-1, "n_steps and n_envs must be > 0");
  if (!rewards || !values || !episode_starts || !last_values || !dones || !advantages || !returns)
    return set_err(-1, "null argument");
  const float g = (float)gamma, gl = (float)(gamma * gae_lambda);
  // full waves and 32-step load blocks: at cfg4's 2 048 x 32 768, 0.236 ms (5.69 TB/s) against
  // 0.266 with half-populated waves (1 024 waves, round 4's first version) and 0.29-0.30 with two
  // envs per lane by float2 moves (tools/gae_sweep.py, profiles/r04_gae_sweep.json: per load
  // instruction the full wave moves two 128-B lines instead of one). F16ENV_GAE_LPW=16|32|64 and
  // F16ENV_GAE_U=8|16|32 select the others (A/B only).
  static const int lpw_env = env_int("F16ENV_GAE_LPW", 64);
  static const int u_env = env_int("F16ENV_GAE_U", 32);
  const int lpw = lpw_env == 32 || lpw_env == 16 ? lpw_env : 64;
  const int64_t blocks = (n_envs + lpw - 1) / lpw;
  if (blocks > 0x7fffffffLL) return set_err(-1, "n_envs too large");
  using GaeKernel = void (*)(int64_t, int64_t, const float*, const float*, const float*, const float*, const uint8_t*,
                             float, float, float*, float*);
  static const GaeKernel table[3][3] = {
      {f16_gae_kernel<8, 16>, f16_gae_kernel<8, 32>, f16_gae_kernel<8, 64>},
      {f16_gae_kernel<16, 16>, f16_gae_kernel<16, 32>, f16_gae_kernel<16, 64>},
      {f16_gae_kernel<32, 16>, f16_gae_kernel<32, 32>, f16_gae_kernel<32, 64>}};
  const GaeKernel kern = table[u_env == 8 ? 0 : (u_env == 16 ? 1 : 2)][lpw == 16 ? 0 : (lpw == 32 ? 1 : 2)];
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, n_steps, n_envs, rewards, values,
                     episode_starts, last_values, dones, g, gl, advantages, returns);
  HIPCHK(hipGetLastError());
  return 0;
}

// on_policy_algorithm.py:236-245 over a device batch: rewards[i] += gamma * terminal_values[i]
// where the lane's episode ended by truncation only (TimeLimit.truncated), float32 per-op
// rounding as SB3 (gamma rounded to float32, the product, then the sum; no FMA)
extern "C" {  // (the kernel symbol stays unmangled, as tools and profiles know it)
__global__ void f16_bootstrap_kernel(int64_t n, float* __restrict__ rew, const uint8_t* __restrict__ term,
                                     const uint8_t* __restrict__ trunc, const float* __restrict__ tv, float g) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (trunc[i] && !term[i]) rew[i] = rew[i] + g * tv[i];
}
}  // extern "C"

static int bootstrap_timeouts_impl(void* stream, int64_t n, float* rewards, const uint8_t* terminated,
                                   const uint8_t* truncated, const float* terminal_values, double gamma) {
  if (n < 0) return set_err(-1, "n must be >= 0");
  if (n == 0) return 0;
  if (!rewards || !terminated || !truncated || !terminal_values) return set_err(-1, "null argument");
  hipLaunchKernelGGL(f16_bootstrap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                     rewards, terminated, truncated, terminal_values, (float)gamma);
  HIPCHK(hipGetLastError());
  return 0;
}

// The deferred timeout bootstrap (include/f16env.h): per step, the terminal observations of the
// lanes that ended by truncation alone are appended to a stash (one atomic per wave, ballot
// compaction as the step kernel's done list); after the rollout one value evaluation over the
// stash and a scatter of gamma * V into the rewards.
extern "C" {  // (the kernel symbol stays unmangled, as tools and profiles know it)
__global__ __launch_bounds__(256) void f16_bootstrap_stash_kernel(int64_t n, int32_t K, const float* __restrict__ tobs,
                                                                  int64_t row_stride, int64_t frame_stride,
                                                                  const uint8_t* __restrict__ term,
                                                                  const uint8_t* __restrict__ trunc, int64_t flat_base,
                                                                  float* __restrict__ stash, int64_t* __restrict__ idx,
                                                                  int32_t* count, int64_t cap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool take = i < n && trunc[i] && !term[i];
  const unsigned long long m = __ballot(take);
  if (!m) return;  // wave-uniform
  int base = 0;
  if (lane == 0) base = atomicAdd(count, __popcll(m));
  base = __shfl(base, 0);
  if (!take) return;
  const int64_t slot = (int64_t)base + __popcll(m & ((1ull << lane) - 1ull));
  F16_CHECK(slot >= 0, DBG_DONE_LIST);
  if (slot >= cap) return;
  float* dst = stash + slot * (int64_t)K * F16_OBS_DIM;
  for (int j = 0; j < K; ++j) {
    const float* src = tobs + i * row_stride + (int64_t)j * frame_stride;
#pragma unroll
    for (int c = 0; c < F16_OBS_DIM; ++c) dst[j * F16_OBS_DIM + c] = src[c];
  }
  idx[slot] = flat_base + i;
}

__global__ void f16_bootstrap_apply_kernel(int64_t m, float* __restrict__ rew, const int64_t* __restrict__ idx,
                                           const float* __restrict__ v, float g) {
#pragma clang fp contract(off)
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int64_t r = idx[j];
  rew[r] = rew[r] + g * v[j];
}
}  // extern "C"

static int bootstrap_stash_impl(void* stream, int64_t n, int32_t K, const float* tobs, int64_t row_stride,
                                int64_t frame_stride, const uint8_t* terminated, const uint8_t* truncated,
                                int64_t flat_base, float* stash_obs, int64_t* stash_idx, int32_t* count,
                                int64_t capacity) {
  if (n < 0 || K < 1 || capacity < 0) return set_err(-1, "n >= 0, K >= 1 and capacity >= 0 required");
  if (n == 0) return 0;
  if (!tobs || !terminated || !truncated || !stash_idx || !count || (capacity > 0 && !stash_obs))
    return set_err(-1, "null argument");
  hipLaunchKernelGGL(f16_bootstrap_stash_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     n, K, tobs, row_stride, frame_stride, terminated, truncated, flat_base, stash_obs, stash_idx,
                     count, capacity);
  HIPCHK(hipGetLastError());
  return 0;
}

static int bootstrap_apply_impl(void* stream, int64_t m, float* rewards, const int64_t* idx, const float* values,
                                double gamma) {
  if (m < 0) return set_err(-1, "m must be >= 0");
  if (m == 0) return 0;
  if (!rewards || !idx || !values) return set_err(-1, "null argument");
  hipLaunchKernelGGL(f16_bootstrap_apply_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     m, rewards, idx, values, (float)gamma);
  HIPCHK(hipGetLastError());
  return 0;
}

// One minibatch of the PPO update (include/f16env.h f16env_rollout_minibatch; buffers.py:481-521):
// a 256-thread block takes MB_SAMPLES samples.
// Phase 1, one lane per sample in each of the four waves (every wave decodes the index itself; what
// it then moves is wave-uniform): wave 0 reads the sample's at most K-1 episode starts and writes
// the source of each of its K output frames into the LDS table, waves 1-3 move the float4 action
// and the four scalars.
// Phase 2: the block's 64 K 15 contiguous output floats as float4 stores, each dword loaded
// through the table (a source frame is a 60-B run at 4-B alignment).
// Table entry: >= 0 an element offset into frames, -1 - (element offset into obs0) for a source
// step before step 0, MB_INVALID for a row with nothing to read (index out of range, or a sample
// past the batch): such a row is never turned into an address and reads as quiet NaN.
// THE GUARD: `ok` below is the only place an index becomes coordinates, and it holds only for
// 0 <= i < W N T, hence r < W, n < N, t < T; source steps lie in [t-K+1, t], those >= 0 index
// frames below T, those < 0 index obs0 at step + K-1 in [0, K-2]; starts are read at steps
// t-d >= 0 only. Every store is bounded by the batch (b < batch; e + i < limit).
constexpr int MB_SAMPLES = 64;
constexpr int64_t MB_INVALID = INT64_MIN;
constexpr uint32_t MB_QNAN = 0x7FC00000u;

struct MbArgs {
  F16RolloutView v;
  int64_t batch, total;  // total = W N T
  const int64_t* idx;
  uint32_t* obs;
  uint4* act;
  uint32_t *val, *lp, *adv, *ret;
};

extern "C" {  // (the kernel symbol stays unmangled, as tools and profiles know it)
__global__ __launch_bounds__(256) void f16_minibatch_kernel(MbArgs a) {
  extern __shared__ int64_t mb_src[];  // [MB_SAMPLES * K]
  const int K = a.v.K;
  const int64_t T = a.v.n_steps, N = a.v.n_envs;
  const int tid = threadIdx.x, s = tid & 63, role = tid >> 6;
  const int64_t b = (int64_t)blockIdx.x * MB_SAMPLES + s;
  bool ok = false;
  int64_t t = 0, r = 0, n = 0;
  if (b < a.batch) {
    const int64_t i = a.idx[b];
    ok = (uint64_t)i < (uint64_t)a.total;
    if (ok) {
      if (a.total <= 0xFFFFFFFFll) {  // (uniform) 32-bit divides where the whole rollout allows
        const uint32_t g = (uint32_t)i / (uint32_t)T, rr = g / (uint32_t)N;
        t = (uint32_t)i - g * (uint32_t)T, r = rr, n = g - rr * (uint32_t)N;
      } else {
        const int64_t g = i / T;
        t = i - g * T, r = g / N, n = g - r * N;
      }
    }
  }
  const int64_t cell = (r * T + t) * N + n;  // the transition's place in a (W, T, N) array
  if (role == 0) {
    int64_t* row = mb_src + s * K;
    if (!ok) {
      for (int j = 0; j < K; ++j) row[j] = MB_INVALID;
    } else {
      int64_t last = t - K;  // below every source step: no bound
      const uint32_t* es = reinterpret_cast<const uint32_t*>(a.v.episode_starts) + cell;
      const int look = (int)(t + 1 < (int64_t)(K - 1) ? t + 1 : (int64_t)(K - 1));
#pragma unroll 4
      for (int d = 0; d < look; ++d) {
        // non-zero as torch's .bool(): +-0 is no start, anything else (NaN too) is
        const bool start = (es[-(int64_t)d * N] & 0x7FFFFFFFu) != 0u;
        const int64_t u = start ? t - d : last;
        last = u > last ? u : last;
      }
      const int64_t f0 = (r * T * N + n) * F16_OBS_DIM, fs = N * F16_OBS_DIM;
      const int64_t z0 = (r * N + n) * K * F16_OBS_DIM;
      for (int j = 0; j < K; ++j) {
        const int64_t want = t - (K - 1) + j, step = want > last ? want : last;
        row[j] = step >= 0 ? f0 + step * fs : -1 - (z0 + (step + K - 1) * F16_OBS_DIM);
      }
    }
  } else if (b < a.batch) {
    if (role == 1) {
      uint4 q = {MB_QNAN, MB_QNAN, MB_QNAN, MB_QNAN};
      if (ok) q = reinterpret_cast<const uint4*>(a.v.actions)[cell];
      a.act[b] = q;
    } else {
      const uint32_t* x = reinterpret_cast<const uint32_t*>(role == 2 ? a.v.values : a.v.advantages);
      const uint32_t* y = reinterpret_cast<const uint32_t*>(role == 2 ? a.v.log_probs : a.v.returns);
      uint32_t xv = MB_QNAN, yv = MB_QNAN;
      if (ok) xv = x[cell], yv = y[cell];
      (role == 2 ? a.val : a.adv)[b] = xv;
      (role == 2 ? a.lp : a.ret)[b] = yv;
    }
  }
  __syncthreads();
  const int rows = MB_SAMPLES * K;
  const int64_t blk = (int64_t)blockIdx.x * rows * F16_OBS_DIM;  // floats; a multiple of 4
  const int64_t left = a.batch * K * F16_OBS_DIM - blk;          // floats of the output from blk on
  const int limit = (int)(left < (int64_t)rows * F16_OBS_DIM ? left : (int64_t)rows * F16_OBS_DIM);
  const uint32_t* frames = reinterpret_cast<const uint32_t*>(a.v.frames);
  const uint32_t* obs0 = reinterpret_cast<const uint32_t*>(a.v.obs0);
  uint32_t* out = a.obs + blk;
  for (int e = 4 * tid; e < limit; e += 4 * 256) {
    const int fr = e / F16_OBS_DIM, c = e - fr * F16_OBS_DIM;
    const int64_t o0 = mb_src[fr], o1 = mb_src[fr + 1 < rows ? fr + 1 : rows - 1];
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool wrap = c + i >= F16_OBS_DIM;
      const int64_t off = wrap ? o1 : o0;
      const int cc = wrap ? c + i - F16_OBS_DIM : c + i;
      w[i] = MB_QNAN;
      if (off != MB_INVALID && e + i < limit) w[i] = (off >= 0 ? frames + off : obs0 + (-1 - off))[cc];
    }
    if (e + 3 < limit) {
      *reinterpret_cast<uint4*>(out + e) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (int i = 0; e + i < limit; ++i) out[e + i] = w[i];
    }
  }
}
}  // extern "C"

static int rollout_minibatch_impl(void* stream, const F16RolloutView* view, int64_t batch, const int64_t* indices,
                                  float* obs, float* actions, float* old_values, float* old_log_probs,
                                  float* advantages, float* returns) {
  if (!view) return set_err(-1, "null rollout view");
  if (batch < 0) return set_err(-1, "batch must be >= 0");
  if (view->K < 1 || view->K > 64) return set_err(-1, "view K must be in [1, 64]");
  if (view->world < 1 || view->n_steps < 1 || view->n_envs < 1)
    return set_err(-1, "view world, n_steps and n_envs must be >= 1");
  // the largest element offset (W T N 15, and W N K 15 for obs0) stays far inside int64
  if ((double)view->world * (double)view->n_steps * (double)view->n_envs * (F16_OBS_DIM * 64.0) >= 4.0e18)
    return set_err(-1, "view world x n_steps x n_envs too large");
  if (batch == 0) return 0;
  if (!view->frames) return set_err(-1, "view frames is NULL");
  if (!view->obs0) return set_err(-1, "view obs0 is NULL");
  if (!view->episode_starts) return set_err(-1, "view episode_starts is NULL");
  if (!view->values) return set_err(-1, "view values is NULL");
  if (!view->log_probs) return set_err(-1, "view log_probs is NULL");
  if (!view->advantages) return set_err(-1, "view advantages is NULL");
  if (!view->returns) return set_err(-1, "view returns is NULL");
  if (!view->actions) return set_err(-1, "view actions is NULL");
  if (!indices || !obs || !actions || !old_values || !old_log_probs || !advantages || !returns)
    return set_err(-1, "null argument (indices and the six outputs are required)");
  if ((((uintptr_t)view->actions) | ((uintptr_t)obs) | ((uintptr_t)actions)) & 15)
    return set_err(-1, "view actions and the obs / actions outputs must be 16-byte aligned");
  if ((((uintptr_t)view->frames) | ((uintptr_t)view->obs0) | ((uintptr_t)view->episode_starts) |
       ((uintptr_t)view->values) | ((uintptr_t)view->log_probs) | ((uintptr_t)view->advantages) |
       ((uintptr_t)view->returns) | ((uintptr_t)old_values) | ((uintptr_t)old_log_probs) | ((uintptr_t)advantages) |
       ((uintptr_t)returns)) & 3)
    return set_err(-1, "float arrays must be float-aligned");
  if (((uintptr_t)indices & 7) != 0) return set_err(-1, "indices must be 8-byte aligned");
  const int64_t blocks = (batch + MB_SAMPLES - 1) / MB_SAMPLES;
  if (blocks > 0x7fffffffLL) return set_err(-1, "batch too large");
  MbArgs a;
  a.v = *view;
  a.batch = batch;
  a.total = (int64_t)view->world * view->n_steps * view->n_envs;
  a.idx = indices;
  a.obs = reinterpret_cast<uint32_t*>(obs);
  a.act = reinterpret_cast<uint4*>(actions);
  a.val = reinterpret_cast<uint32_t*>(old_values);
  a.lp = reinterpret_cast<uint32_t*>(old_log_probs);
  a.adv = reinterpret_cast<uint32_t*>(advantages);
  a.ret = reinterpret_cast<uint32_t*>(returns);
  hipLaunchKernelGGL(f16_minibatch_kernel, dim3((unsigned)blocks), dim3(256),
                     (size_t)MB_SAMPLES * view->K * sizeof(int64_t), (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}
