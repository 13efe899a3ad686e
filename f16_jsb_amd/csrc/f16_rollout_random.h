// f16_rollout_random.h -- the persistent rollout under the uniform random policy: RollArgs,
// f16_rollout_kernel (T env steps of every lane in one launch) and the table that picks its
// instance. It spells out its own gust update and cached-row reset beside step_body's: sharing
// them moved the step kernels' schedules (source map).
// Needs f16_device.h, f16_env_layer.h, f16_rng.h and f16_stage.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/f16env.h"
#include "f16_device.h"
#include "f16_env_layer.h"
#include "f16_rng.h"
#include "f16_stage.h"

using namespace f16;

// ------------------------------------------------------------------------------------------
// Persistent rollout under the uniform random policy (f16env_rollout_random /
// f16env_window_rollout_random): T env steps of every lane in ONE launch. The actions come from
// the f16env_sample_actions Philox stream, so no step waits for a host or a policy: each lane
// keeps its state in registers across the whole rollout and per step writes only the rollout
// slot -- the action, reward and next episode start of step t, and the newest frame of the
// observation it returns, which is the frame slot t + 1 acts on (frames[0] is the newest frame
// of the observation before step 0). No frame stack is kept on chip: the final observation is
// rebuilt at the end from the frame log the lane wrote (obs[j] = F[max(T-K+1+j, s)], s the
// lane's last episode start, F[T] the last frame in registers, F[t <= 0] from the observation
// before the rollout -- rollout.py rebuild_observations), so K is not bounded by LDS (round 3's
// ring held K <= 8 frames per lane). cfg5 modes (MODE != 0): gusts per step as the step kernel,
// and a finished lane resets from the reset cache when it holds its next episode's row (the
// first reset of a lane in the rollout; f16_ic_fill_kernel fills it before the launch), else
// by its own RunIC. Same arithmetic, RNG streams and auto-reset as T launches of the fused step
// (f16env_step_rollout / f16env_window_step_rollout): bit-identical results (build.py
// -ffp-contract=on: contraction is fixed per source expression, not per kernel).
// ------------------------------------------------------------------------------------------
struct RollArgs {
  SoA s, tmpl, icc;       // icc: cfg5 reset cache (MODE != 0; c == nullptr: every reset a RunIC)
  // the observation before step 0: frame j of lane k at obs_prev + k * in_row + j * in_pitch
  // (contiguous N x K x 15: K*15, 15; a position-major window: 16, N*16)
  const float* obs_prev;
  int64_t in_row, in_pitch;
  // the observation after step T-1, written the same way to out0 and (when not NULL) out1 --
  // the two window histories -- with out_slot floats per frame (15, or 16: a 64-B slot)
  float* out0;
  float* out1;
  int64_t out_row, out_pitch;
  int32_t out_slot;
  float* frames;          // T x N x 15: frames[t] = newest frame of the observation step t acts on
  float* actions;         // T x N x 4
  float* rewards;         // T x N
  float* next_start;      // (T - 1) x N: 1.0 where the lane finished at step t < T-1
  float* last_start;      // N: the same for step T-1
  unsigned long long* nonfinite;  // [0] F16_FLAG_NAN_GUARD quarantines, [2] F16_FLAG_OBS_CHECK
  uint64_t seed, step0;
  int32_t T;
  int32_t clear_fresh;    // both output windows are whole: no lane needs a FRESH fill next step
  EnvArgs E;
  ModelConsts C;
};
template <int MODE, int OCC>
__global__ __launch_bounds__(BLOCK, OCC) void f16_rollout_kernel(RollArgs a) {
  __shared__ __align__(16) float sT[F16_BLOB_FLOATS];
  __shared__ __align__(16) float4 sTmpl[NCOL + TMPL_FRAME_COLS];
  __shared__ __align__(16) float4 sF[BLOCK * 4];  // per wave: its 64 new frames as [64][4] float4
  constexpr bool GUST = (MODE & 2) != 0;
  const int K = a.E.K, tid = threadIdx.x;
  const int64_t k = (int64_t)blockIdx.x * BLOCK + tid;
  const int64_t N = a.E.n;
  const bool live = k < N;
  stage_tables_issue(sT);
  if (MODE == 0 && tid < NCOL + TMPL_FRAME_COLS)
    dma16(reinterpret_cast<const float*>(a.tmpl.c + (tid < NCOL ? tid : tid + NCOL_ALL - NCOL)),
          reinterpret_cast<float*>(sTmpl));
  Lane L;
  float fn[F16_OBS_DIM];  // newest frame of the lane's current observation
  if (live) {
    lane_load<GUST>(a.s, k, L);
    const float* op = a.obs_prev + k * a.in_row + (int64_t)(K - 1) * a.in_pitch;
#pragma unroll
    for (int c = 0; c < F16_OBS_DIM; ++c) fn[c] = op[c];
  }
  VM_DRAIN();
  __syncthreads();
  if (!live) return;  // no barrier below
  const int wave = tid >> 6, lane = tid & 63;
  const int64_t row0 = (int64_t)blockIdx.x * BLOCK + wave * 64;
  // a full wave writes its 64 frames (3 840 contiguous bytes) as 240 float4 gathered from its
  // LDS staging, instead of fifteen 4-byte stores per lane at a 60-byte stride
  const bool coalesced = N - row0 >= 64 && (N * F16_OBS_DIM) % 4 == 0 && ((uintptr_t)a.frames & 15) == 0;
  float4* stg = sF + wave * 256;
  auto put_frame = [&](int64_t t) {  // frames[t] = fn for every lane of the wave
    if (coalesced) {
      __builtin_amdgcn_wave_barrier();
      stg[lane * 4 + 0] = make_float4(fn[0], fn[1], fn[2], fn[3]);
      stg[lane * 4 + 1] = make_float4(fn[4], fn[5], fn[6], fn[7]);
      stg[lane * 4 + 2] = make_float4(fn[8], fn[9], fn[10], fn[11]);
      stg[lane * 4 + 3] = make_float4(fn[12], fn[13], fn[14], 0.0f);
      __builtin_amdgcn_wave_barrier();
      const float* src = reinterpret_cast<const float*>(stg);
      float4* dst = reinterpret_cast<float4*>(a.frames + (t * N + row0) * F16_OBS_DIM);
      for (int q = lane; q < 64 * F16_OBS_DIM / 4; q += 64) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = 4 * q + i, r = e / F16_OBS_DIM;
          v[i] = src[r * 16 + (e - r * F16_OBS_DIM)];
        }
        dst[q] = make_float4(v[0], v[1], v[2], v[3]);
      }
    } else {
      float* fr = a.frames + (t * N + k) * F16_OBS_DIM;
#pragma unroll
      for (int c = 0; c < F16_OBS_DIM; ++c) fr[c] = fn[c];
    }
  };
  put_frame(0);
  const uint64_t gid = (uint64_t)(a.E.id_base + k);
  int last_s = -(1 << 30);  // index t of the lane's last reset frame F[t] in this rollout (none yet)
  bool cache_fresh = a.icc.c != nullptr;  // the cached row can only serve the lane's first reset
  for (int t = 0; t < a.T; ++t) {
    const float4 av = philox_action(a.seed, gid, a.step0 + (uint64_t)t);
    const float cmd[4] = {av.x, av.y, av.z, av.w};
    L.step += 1;  L.flags &= ~LANE_FLAG_FRESH;                                              // jsbsim_gym.py:215
    if (GUST) {  // cfg5 Gauss-Markov gust update, once per env step before the frames (as step_body)
      float xi[3];
      rng_normals(a.E.seed, gid, (uint32_t)(L.ep_count - 1), (uint32_t)L.step, xi);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        L.gust[j] = __builtin_fmaf(a.E.gust_a, L.gust[j], a.E.gust_b * xi[j]);
        L.wind[j] = L.wst[j] + L.gust[j];
      }
    }
    double ce, se;
    earth_angle(L.epa, ce, se);
    const AltRef A = alt_ref(L, ce, se);
#ifdef F16_STAMPS
    Stamps stamps = {};
#endif
    for (int s = 0; s < a.E.down_sample; ++s)
      frame<OCC == 2, GUST>(L, cmd, ce, se, A, sT, a.C, false F16_STAMP_PASS);  // :225-232
    float f[F16_OBS_DIM];
    make_frame<OCC != 2>(L, ce, se, A, f);                    // :234
    float r32;
    const int fl = env_reward<OCC != 2>(L, f, a.E, r32);
    const int done = fl & 3;
    if (a.E.flags & F16_FLAG_NAN_GUARD) {
      const unsigned long long qm = __ballot(fl & 4);
      if (qm && lane == 0) atomicAdd(a.nonfinite, (unsigned long long)__popcll(qm));
    }
    if (a.E.flags & F16_FLAG_OBS_CHECK) {  // jsbsim_gym.py:268-285 on the new frame
      const unsigned long long om = __ballot(obs_out_of_bounds(f));
      if (om && lane == 0) atomicAdd(a.nonfinite + 2, (unsigned long long)__popcll(om));
    }
    const int64_t row = (int64_t)t * N + k;
    reinterpret_cast<float4*>(a.actions)[row] = av;
    a.rewards[row] = r32;
    if (t + 1 < a.T) a.next_start[row] = done ? 1.0f : 0.0f;
    else a.last_start[k] = done ? 1.0f : 0.0f;
    if (done) {  // dummy_vec_env.py:68-71: the next observation is K x the reset frame
      if (MODE == 0) {
        lane_reset_template(L, sTmpl, a.E, k, fn);
      } else if (cache_fresh && __float_as_int(a.icc.c[(int64_t)15 * a.icc.n + k].w) == L.ep_count + 1) {
        lane_load<GUST>(a.icc, k, L);  // the lane's next reset, evaluated ahead (f16_ic_fill_kernel)
#pragma unroll
        for (int j = 0; j < TMPL_FRAME_COLS; ++j) {
          const float4 v = a.icc.c[(int64_t)(NCOL_ALL + j) * a.icc.n + k];
          fn[4 * j] = v.x; fn[4 * j + 1] = v.y; fn[4 * j + 2] = v.z; fn[4 * j + 3] = v.w;
        }
        fn[12] = L.goal[0]; fn[13] = L.goal[1]; fn[14] = L.goal[2];
        cache_fresh = false;
      } else {
        lane_reset_mode<MODE, OCC == 2>(L, a.E, k, sT, a.C, fn);
        cache_fresh = false;
      }
      last_s = t + 1;
    } else {
#pragma unroll
      for (int c = 0; c < F16_OBS_DIM; ++c) fn[c] = f[c];
    }
    if (t + 1 < a.T) put_frame(t + 1);
  }
  if (a.clear_fresh) L.flags &= ~LANE_FLAG_FRESH;
  lane_store<GUST>(a.s, k, L);
  // the final observation, oldest frame first: F[max(T-K+1+j, last_s)]; F[T] = fn, F[1..T-1] from
  // this wave's own frame-log rows (made visible to the reads by the fence), F[t <= 0] from the
  // observation before the rollout (F[0] is also frames[0])
  __threadfence();
  const int T = a.T;
  for (int j = 0; j < K; ++j) {
    const int idx = max(T - K + 1 + j, last_s);
    float v[F16_OBS_DIM];
    if (idx == T) {
#pragma unroll
      for (int c = 0; c < F16_OBS_DIM; ++c) v[c] = fn[c];
    } else if (idx >= 1) {
      const float* src = a.frames + ((int64_t)idx * N + k) * F16_OBS_DIM;
#pragma unroll
      for (int c = 0; c < F16_OBS_DIM; ++c) v[c] = __builtin_nontemporal_load(src + c);
    } else {
      const float* src = a.obs_prev + k * a.in_row + (int64_t)(idx + K - 1) * a.in_pitch;
#pragma unroll
      for (int c = 0; c < F16_OBS_DIM; ++c) v[c] = src[c];
    }
    F16_CHECK(idx >= 1 - K && idx <= T, DBG_RING_SLOT);
    for (int b = 0; b < 2; ++b) {
      float* o = (b == 0 ? a.out0 : a.out1);
      if (!o) continue;
      o += k * a.out_row + (int64_t)j * a.out_pitch;
#pragma unroll
      for (int c = 0; c < F16_OBS_DIM; ++c) o[c] = v[c];
      if (a.out_slot > F16_OBS_DIM) o[F16_OBS_DIM] = 0.0f;
    }
  }
}

// the instance for a handle's mode, at one or two waves per SIMD
using RollKernel = void (*)(RollArgs);
static RollKernel rollout_kernel_for(int mode, int occ) {
  static const RollKernel table[2][4] = {
      {f16_rollout_kernel<0, 1>, f16_rollout_kernel<1, 1>, f16_rollout_kernel<2, 1>, f16_rollout_kernel<3, 1>},
      {f16_rollout_kernel<0, 2>, f16_rollout_kernel<1, 2>, f16_rollout_kernel<2, 2>, f16_rollout_kernel<3, 2>}};
  return table[occ == 2 ? 1 : 0][mode & 3];
}
