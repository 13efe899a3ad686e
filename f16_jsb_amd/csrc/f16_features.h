// f16_features.h -- what is computed from one observation frame for the policy and the viewer:
// the 15 -> 17 policy features (frame_features, frame_features_part) with their three kernels
// (contiguous, strided, feature window), and the render pose (pose_of_frame) with the poses
// kernel; below each kernel the handle-free launcher behind its entry point (f16env_features,
// _features_strided, _features_window_step, _poses). The step kernel's epilogue calls
// frame_features and pose_of_frame, so f16_step.h includes this file.
// Needs f16_host.h (set_err, HIPCHK), f16_device.h (F16_CHECK) and include/f16env.h (F16_OBS_DIM).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/f16env.h"
#include "f16_device.h"
#include "f16_host.h"

using namespace f16;

#define FEAT_IN 15
#define FEAT_OUT 17
// jsbsim_gym/features.py:37-67 on one frame o[15] -> y[17], float32 with torch's per-op
// rounding (IEEE division / sqrt, no FMA contraction, ~1-ulp atan2 / cos / sin)
__device__ __forceinline__ void frame_features(const float* o, float* y) {
#pragma clang fp contract(off)
  // features.py:39-45 unpack; :47-53 position transform
  const float dx = o[12] - o[0], dy = o[13] - o[1], dz = o[14] - o[2];
  float d2 = dx * dx;
  d2 = __fadd_rn(d2, __fmul_rn(dy, dy));
  const float distance = __fsqrt_rn(d2);
  const float abs_bearing = atan2f(dy, dx);
  const float rel_bearing = abs_bearing - o[11];
  y[0] = __fdiv_rn(1.0f, __fadd_rn(1.0f, __fmul_rn(distance, 1e-3f)));  // :56 dist_norm
  y[1] = __fdiv_rn(dz, 15000.0f);                                         // :59 dz_norm
  y[2] = __fdiv_rn(o[2], 15000.0f);                                       // :60 alt_norm
  y[3] = o[3];                                                            // mach
  y[4] = o[6]; y[5] = o[7]; y[6] = o[8];                                  // angular rates
  y[7] = cosf(o[4]); y[8] = cosf(o[5]);                                   // :63 cos(alpha, beta)
  y[9] = sinf(o[4]); y[10] = sinf(o[5]);                                  //     sin(alpha, beta)
  y[11] = cosf(o[9]); y[12] = cosf(o[10]);                                // :64 cos(phi, theta)
  y[13] = sinf(o[9]); y[14] = sinf(o[10]);                                //     sin(phi, theta)
  y[15] = cosf(rel_bearing); y[16] = sinf(rel_bearing);                   // :65
}

// frame_features split into four parts of about equal cost (the feature-window kernel gives
// each part to a wave): the same expressions, so the same values, as frame_features
__device__ __forceinline__ void frame_features_part(const float* o, float* y, int part) {
#pragma clang fp contract(off)
  const float dx = o[12] - o[0], dy = o[13] - o[1];
  if (part == 0) {
    const float abs_bearing = atan2f(dy, dx);
    const float rel_bearing = abs_bearing - o[11];
    y[15] = cosf(rel_bearing); y[16] = sinf(rel_bearing);
  } else if (part == 1) {
    y[7] = cosf(o[4]); y[8] = cosf(o[5]);
    y[9] = sinf(o[4]); y[10] = sinf(o[5]);
  } else if (part == 2) {
    y[11] = cosf(o[9]); y[12] = cosf(o[10]);
    y[13] = sinf(o[9]); y[14] = sinf(o[10]);
  } else {
    const float dz = o[14] - o[2];
    float d2 = dx * dx;
    d2 = __fadd_rn(d2, __fmul_rn(dy, dy));
    const float distance = __fsqrt_rn(d2);
    y[0] = __fdiv_rn(1.0f, __fadd_rn(1.0f, __fmul_rn(distance, 1e-3f)));
    y[1] = __fdiv_rn(dz, 15000.0f);
    y[2] = __fdiv_rn(o[2], 15000.0f);
    y[3] = o[3];
    y[4] = o[6]; y[5] = o[7]; y[6] = o[8];
  }
}

// Render/telemetry pose of one observation frame x: what JSBSimEnv.render
// (jsbsim_gym/jsbsim_gym.py:381-415) hands the Viewer -- the aircraft position in viewer axes
// (-y, h, x) * 1e-3, its attitude Quaternion.from_euler(phi, theta, psi) (visualization/
// quaternion.py:38-45, q_psi * q_theta * q_phi) remapped (w, -y, -z, x), and the goal position
// in viewer axes -- in float32 with the reference's operation order (no contraction). Shared
// by f16_poses_kernel and the plain step's epilogue (F16_STEP_POSES), so both give the same bits.
__device__ __forceinline__ void quat_mul_ref(const float* a, const float* b, float* o) {
#pragma clang fp contract(off)
  // quaternion.py:11-14: w = a0 b0 - a.b ; v = a0 b + b0 a + a x b  (float32, left to right)
  const float dot = a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  o[0] = a[0] * b[0] - dot;
  const float cx = a[2] * b[3] - a[3] * b[2], cy = a[3] * b[1] - a[1] * b[3], cz = a[1] * b[2] - a[2] * b[1];
  o[1] = a[0] * b[1] + b[0] * a[1] + cx;
  o[2] = a[0] * b[2] + b[0] * a[2] + cy;
  o[3] = a[0] * b[3] + b[0] * a[3] + cz;
}
__device__ __forceinline__ void pose_of_frame(const float* x, float* o) {
#pragma clang fp contract(off)
  const float s = 1e-3f;
  o[0] = -x[1] * s; o[1] = x[2] * s; o[2] = x[0] * s;
  const float hp = x[9] / 2.0f, ht = x[10] / 2.0f, hs = x[11] / 2.0f;
  float sp, cp, st, ct, ss, cs;
  sincosf(hp, &sp, &cp);
  sincosf(ht, &st, &ct);
  sincosf(hs, &ss, &cs);
  const float q1[4] = {cp, sp, 0.0f, 0.0f};
  const float q2[4] = {ct, 0.0f, st, 0.0f};
  const float q3[4] = {cs, 0.0f, 0.0f, ss};
  float q32[4], q[4];
  quat_mul_ref(q3, q2, q32);
  quat_mul_ref(q32, q1, q);
  o[3] = q[0]; o[4] = -q[2]; o[5] = -q[3]; o[6] = q[1];
  o[7] = -x[13] * s; o[8] = x[14] * s; o[9] = x[12] * s;
}

// Per-frame policy features: jsbsim_gym/features.py:37-67
// JSBSimFeatureExtractor.forward, 15 observation floats -> 17 features, float32 throughout
// (torch float32 semantics: IEEE division / sqrt, ~1-ulp atan2 / cos / sin), applied to every
// frame of a (..., 15) block, e.g. the (N, K, 15) stack as the first stage of
// LMA_features.py:744-776 StackedLMAFeaturesExtractor does. HBM-bound (60 B in, 68 B out per
// frame): each 256-thread block moves its 256 frames as coalesced float4 through LDS (frame
// strides 15 and 17 are odd, so the per-thread LDS reads/writes are bank-conflict free).
__global__ __launch_bounds__(256) void f16_features_kernel(int64_t n_frames, const float* __restrict__ obs,
                                                           float* __restrict__ feat) {
  __shared__ __align__(16) float sIn[256 * FEAT_IN];
  __shared__ __align__(16) float sOut[256 * FEAT_OUT];
  const int64_t f0 = (int64_t)blockIdx.x * 256;
  const int nf = (int)(n_frames - f0 < 256 ? n_frames - f0 : 256);
  const int t = threadIdx.x;
  const float* gin = obs + f0 * FEAT_IN;
  float* gout = feat + f0 * FEAT_OUT;
  // whole-block float4 moves need 16-byte alignment of the block's slice (base % 16 == 0 and
  // a full block: 256 * 15 * 4 and 256 * 17 * 4 bytes are multiples of 16)
  const bool vin = nf == 256 && (((uintptr_t)gin) & 15) == 0;
  const bool vout = nf == 256 && (((uintptr_t)gout) & 15) == 0;
  if (vin) {
    for (int q = t; q < 256 * FEAT_IN / 4; q += 256)
      reinterpret_cast<float4*>(sIn)[q] = reinterpret_cast<const float4*>(gin)[q];
  } else {
    for (int q = t; q < nf * FEAT_IN; q += 256) sIn[q] = gin[q];
  }
  __syncthreads();
  if (t < nf) frame_features(sIn + t * FEAT_IN, sOut + t * FEAT_OUT);
  __syncthreads();
  if (vout) {
    for (int q = t; q < 256 * FEAT_OUT / 4; q += 256)
      reinterpret_cast<float4*>(gout)[q] = reinterpret_cast<const float4*>(sOut)[q];
  } else {
    for (int q = t; q < nf * FEAT_OUT; q += 256) gout[q] = sOut[q];
  }
}

static int features_impl(void* stream, int64_t n_frames, const float* obs, float* feat) {
  if (n_frames < 0) return set_err(-1, "n_frames must be >= 0");
  if (n_frames == 0) return 0;
  if (!obs || !feat) return set_err(-1, "null argument");
  if (((uintptr_t)obs & 3) != 0 || ((uintptr_t)feat & 3) != 0) return set_err(-1, "obs and feat must be float-aligned");
  const int64_t blocks = (n_frames + 255) / 256;
  if (blocks > 0x7fffffffLL) return set_err(-1, "n_frames too large");
  hipLaunchKernelGGL(f16_features_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n_frames, obs,
                     feat);
  HIPCHK(hipGetLastError());
  return 0;
}

// The same per-frame transform on a strided (B, K, 15) block -- e.g. a windowed observation
// (env rows 16 floats apart, frames N*16 apart: position-major 64-B slots) read in place, no
// copy to a contiguous stack.
// One lane per frame (16-B vector reads of its slot when the strides allow); the (B, K, 17)
// output leaves through LDS as coalesced float4, as in f16_features_kernel.
__global__ __launch_bounds__(256) void f16_features_strided_kernel(int64_t n_rows, int32_t K, const float* __restrict__ obs,
                                                                   int64_t row_stride, int64_t frame_stride,
                                                                   float* __restrict__ feat) {
  __shared__ __align__(16) float sOut[256 * FEAT_OUT];
  const int64_t n_frames = n_rows * K;
  const int64_t f0 = (int64_t)blockIdx.x * 256;
  const int nf = (int)(n_frames - f0 < 256 ? n_frames - f0 : 256);
  const int t = threadIdx.x;
  if (t < nf) {
    const int64_t i = f0 + t;
    const int64_t r = i / K, kk = i - r * K;
    F16_CHECK(i < n_frames && r < n_rows && kk < K, DBG_FRAME_INDEX);
    const float* o = obs + r * row_stride + kk * frame_stride;
    float x[FEAT_IN];
    if ((frame_stride & 3) == 0 && (row_stride & 3) == 0 && ((uintptr_t)obs & 15) == 0) {  // 16-B aligned frames
      const float4* q = reinterpret_cast<const float4*>(o);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float4 v = q[j];
        x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
      }
      const float2 v2 = *reinterpret_cast<const float2*>(o + 12);
      x[12] = v2.x; x[13] = v2.y; x[14] = o[14];
    } else {
#pragma unroll
      for (int j = 0; j < FEAT_IN; ++j) x[j] = o[j];
    }
    frame_features(x, sOut + t * FEAT_OUT);
  }
  __syncthreads();
  float* gout = feat + f0 * FEAT_OUT;
  if (nf == 256 && (((uintptr_t)gout) & 15) == 0) {
    for (int q = t; q < 256 * FEAT_OUT / 4; q += 256)
      reinterpret_cast<float4*>(gout)[q] = reinterpret_cast<const float4*>(sOut)[q];
  } else {
    for (int q = t; q < nf * FEAT_OUT; q += 256) gout[q] = sOut[q];
  }
}

static int features_strided_impl(void* stream, int64_t n_rows, int32_t K, const float* obs, int64_t row_stride,
                                 int64_t frame_stride, float* feat) {
  if (n_rows < 0 || K < 1) return set_err(-1, "n_rows >= 0 and K >= 1 required");
  if (n_rows == 0) return 0;
  if (!obs || !feat) return set_err(-1, "null argument");
  if (frame_stride < 0 || row_stride < 0) return set_err(-1, "strides must be non-negative");
  if (((uintptr_t)obs & 3) != 0 || ((uintptr_t)feat & 3) != 0) return set_err(-1, "obs and feat must be float-aligned");
  const int64_t blocks = (n_rows * K + 255) / 256;
  if (blocks > 0x7fffffffLL) return set_err(-1, "too many frames");
  hipLaunchKernelGGL(f16_features_strided_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n_rows, K,
                     obs, row_stride, frame_stride, feat);
  HIPCHK(hipGetLastError());
  return 0;
}

// Feature window (windowed layout): the policy features of both frame histories kept beside
// them, position-major [T][N][17], so that after a windowed step only the frame the step wrote
// needs transforming -- the features of a K-frame observation cost one frame per step instead
// of K (f16env_features_strided over the view). The step wrote position p of both histories:
// wx[p] = the new frame, or the reset frame of a lane reset by the step (which also fills
// wx[p-K+1 .. p-1] with it), wy[p] = the new frame (the reset lane's final frame). Here
// fx[p] = fy[p] = y = feat(wx[p]), and a reset lane writes y over fx[p-K+1 .. p-1] too -- and
// over fy[p-K+2 .. p]: the window fill the NEXT step will make of that lane (FRESH: wx' = wy
// gets wx[p] at positions p-K+2 .. p, step_body) applied ahead, so no call needs the previous
// step's resets or a second transform; fy's window then holds the next step's view, not the
// terminal observation's (whose features nobody asks for). No dependent load. 64 envs per
// 256-thread block: the block's 64 frame slots come in as one float4 per thread (coalesced),
// then each of the 4 waves computes one quarter of every env's 17 features from LDS
// (frame_features_part: the work per wave a quarter, four waves per SIMD at 65 536 envs instead
// of one -- the one-lane-per-env form was latency-bound at 6.2 us, gpurun fw r04), and the
// block's rows p (64 * 17 contiguous floats in each history) leave as float4. transform = 0:
// only the ahead fills of the step's reset lanes, y read from fx[p] (after both windows were
// transformed whole following a step).
struct FeatWinArgs {
  const float* wx;
  int64_t wrow, wenv;  // frame-history strides (floats) between positions, between envs
  float* fx;
  float* fy;           // [T][N][17]
  int64_t n;
  int32_t K, p, autoreset, transform;
  const uint8_t* term;
  const uint8_t* trunc;
};
static constexpr int FW_ENVS = 64;     // envs per block
static constexpr int FW_IN = 17;       // LDS pitch of a frame (odd: conflict-free per-env reads)
__global__ __launch_bounds__(256) void f16_feature_window_kernel(FeatWinArgs a) {
  __shared__ __align__(16) float sIn[FW_ENVS * FW_IN];
  __shared__ __align__(16) float sY[FW_ENVS * FEAT_OUT];
  const int t = threadIdx.x, w = t >> 6, e = t & 63;
  const int64_t k0 = (int64_t)blockIdx.x * FW_ENVS, k = k0 + e;
  const int nb = (int)(a.n - k0 < FW_ENVS ? a.n - k0 : FW_ENVS);
  const int64_t rowN = a.n * FEAT_OUT;  // floats between feature positions
  F16_CHECK(nb > 0 && a.p >= a.K - 1, DBG_FRAME_INDEX);
  const bool done = e < nb && a.autoreset && (a.term[k] | a.trunc[k]) != 0;
  if (a.transform) {
    const int le = t >> 2, qq = t & 3;  // the block's slots: thread t loads quarter qq of env le
    if (le < nb) {
      const float4 v = *reinterpret_cast<const float4*>(a.wx + (k0 + le) * a.wenv + (int64_t)a.p * a.wrow + 4 * qq);
      float* d = sIn + le * FW_IN + 4 * qq;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    if (e < nb) frame_features_part(sIn + e * FW_IN, sY + e * FEAT_OUT, w);
    __syncthreads();
  }
  // rare: the window fills of the block's reset envs (rows below p in fx, ahead in fy). Every
  // wave sees the same done mask (env e = lane); wave w takes every 4th reset env and spreads
  // its (row, feature) pairs over its 64 lanes: whole-wave stores, not one lane per env walking
  // 2K-2 rows a page apart (gpurun fw r04: +3.3 us at K = 10 for 0.13 % of lanes reset)
  const uint64_t dm = __ballot(done);
  if (dm && a.K > 1) {
    const int nrx = a.K - 1;                          // fx rows p-K+1 .. p-1
    const int nry = a.transform ? a.K - 2 : a.K - 1;  // fy rows p-K+2 .. p-1 (.. p without transform)
    const int items = (nrx + nry) * FEAT_OUT;
    int idx = 0;
    for (uint64_t m = dm; m; m &= m - 1, ++idx) {
      if ((idx & 3) != w) continue;
      const int ee = __builtin_ctzll(m);
      const int64_t kk = k0 + ee;
      for (int it = e; it < items; it += 64) {
        const int ri = it / FEAT_OUT, j = it - ri * FEAT_OUT;
        const float v = a.transform ? sY[ee * FEAT_OUT + j] : a.fx[(int64_t)a.p * rowN + kk * FEAT_OUT + j];
        float* d = ri < nrx ? a.fx + (int64_t)(a.p - a.K + 1 + ri) * rowN
                            : a.fy + (int64_t)(a.p - a.K + 2 + (ri - nrx)) * rowN;
        d[kk * FEAT_OUT + j] = v;
      }
    }
  }
  if (!a.transform) return;
  float* gx = a.fx + (int64_t)a.p * rowN + k0 * FEAT_OUT;
  float* gy = a.fy + (int64_t)a.p * rowN + k0 * FEAT_OUT;
  if (nb == FW_ENVS && ((((uintptr_t)gx) | ((uintptr_t)gy)) & 15) == 0) {
    for (int q = t; q < FW_ENVS * FEAT_OUT / 4; q += 256) {
      const float4 v = reinterpret_cast<const float4*>(sY)[q];
      reinterpret_cast<float4*>(gx)[q] = v;
      reinterpret_cast<float4*>(gy)[q] = v;
    }
  } else {
    for (int q = t; q < nb * FEAT_OUT; q += 256) {
      gx[q] = sY[q];
      gy[q] = sY[q];
    }
  }
}

static int features_window_step_impl(void* stream, int64_t n, int32_t K, int32_t pos, const float* hist_cur,
                                     int64_t pos_stride, int64_t env_stride, float* feat_cur, float* feat_other,
                                     const uint8_t* terminated, const uint8_t* truncated, int32_t autoreset,
                                     int32_t transform) {
  if (n < 0 || K < 1 || pos < K - 1) return set_err(-1, "n >= 0, K >= 1 and pos >= K - 1 required");
  if (n == 0) return 0;
  if (!hist_cur || !feat_cur || !feat_other || !terminated || !truncated) return set_err(-1, "null argument");
  if ((pos_stride & 15) || (env_stride & 15) || pos_stride < 16 || env_stride < 16 || (((uintptr_t)hist_cur) & 15) != 0)
    return set_err(-1, "frame history must be 16-byte aligned with 16-float slots");
  if (((((uintptr_t)feat_cur) | ((uintptr_t)feat_other)) & 3) != 0) return set_err(-1, "feature histories must be float-aligned");
  FeatWinArgs a;
  a.wx = hist_cur; a.wrow = pos_stride; a.wenv = env_stride;
  a.fx = feat_cur; a.fy = feat_other; a.n = n; a.K = K; a.p = pos;
  a.autoreset = autoreset ? 1 : 0; a.transform = transform ? 1 : 0;
  a.term = terminated; a.trunc = truncated;
  const int64_t blocks = (n + FW_ENVS - 1) / FW_ENVS;
  if (blocks > 0x7fffffffLL) return set_err(-1, "too many envs");
  hipLaunchKernelGGL(f16_feature_window_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// Render/telemetry poses of one frame per env (pose_of_frame above). One
// lane per env; frames are read with a caller stride so obs[:, -1, :] of a (N, K, 15) stack needs
// no copy.
// 256 envs per block; 16-B aligned frames (the windowed layout's 64-B slots) are read as
// 3 x float4 + float2 + float, and the block's 256 x 10 poses leave through LDS as contiguous
// float4 (a 40-B row per lane would be 10 partial-line dword stores)
__global__ __launch_bounds__(256) void f16_poses_kernel(int64_t n, const float* __restrict__ frames, int64_t stride,
                                                        float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ __align__(16) float sOut[256 * 10];
  const int t = threadIdx.x;
  const int64_t k0 = (int64_t)blockIdx.x * 256, k = k0 + t;
  const int nb = (int)(n - k0 < 256 ? n - k0 : 256);
  if (t < nb) {
    const float* f = frames + k * stride;
    float x[F16_OBS_DIM];
    if ((stride & 3) == 0 && ((uintptr_t)frames & 15) == 0) {
      const float4* q4 = reinterpret_cast<const float4*>(f);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float4 v = q4[j];
        x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
      }
      const float2 v2 = *reinterpret_cast<const float2*>(f + 12);
      x[12] = v2.x; x[13] = v2.y; x[14] = f[14];
    } else {
#pragma unroll
      for (int j = 0; j < F16_OBS_DIM; ++j) x[j] = f[j];
    }
    pose_of_frame(x, sOut + t * 10);
  }
  __syncthreads();
  float* g = out + k0 * 10;
  if (nb == 256 && ((uintptr_t)g & 15) == 0) {
    for (int q = t; q < 256 * 10 / 4; q += 256)
      reinterpret_cast<float4*>(g)[q] = reinterpret_cast<const float4*>(sOut)[q];
  } else {
    for (int q = t; q < nb * 10; q += 256) g[q] = sOut[q];
  }
}

static int poses_impl(void* stream, int64_t n, const float* frames, int64_t frame_stride, float* out) {
  if (n < 0 || frame_stride < F16_OBS_DIM) return set_err(-1, "n >= 0 and frame_stride >= 15 required");
  if (n == 0) return 0;
  if (!frames || !out) return set_err(-1, "null argument");
  hipLaunchKernelGGL(f16_poses_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, frames,
                     frame_stride, out);
  HIPCHK(hipGetLastError());
  return 0;
}
