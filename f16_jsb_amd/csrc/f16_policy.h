// f16_policy.h -- the actor-critic MLP forward of a rollout as one HIP kernel (gfx950), and the
// host side of f16env_policy_blob_layout / f16env_policy_forward (include/f16env.h, ABI 7); below
// it the backward of the two MLPs in the blob's layout (f16env_policy_backward).
// Needs f16_host.h (set_err, HIPCHK) and f16_rng.h (philox).
//
// actions, values, log_probs = policy(obs) for stable_baselines3's ActorCriticPolicy with separate
// pi / vf MLPs (common/policies.py:ActorCriticPolicy.forward, torch_layers.py:MlpExtractor, a
// DiagGaussianDistribution with a state-independent log_std), float32 throughout.
//
// Tile: one wave owns 32 observation rows; a block is 4 waves (128 rows). Every layer is
// H^T = W X^T on v_mfma_f32_32x32x2_f32 (an exact k-ordered f32 fma chain per output, so a row's
// result does not depend on the rows beside it): the MFMA's rows are 32 hidden units, its columns
// the wave's 32 observation rows.
//   A operand (weights): lane l holds W[32 to + (l & 31)][2 s + (l >> 5)] for output tile `to`,
//     k-step s -- the blob stores each layer in exactly that order, [to][s][64 lanes], so the
//     operand is one coalesced 256-B read per MFMA (from LDS when the blob fits, else L2).
//   B operand (activations): lane l holds X[2 s + (l >> 5)][l & 31] from the wave's own LDS image
//     [k][row]; the observation is staged there once (stride 33, the 32 rows of a k contiguous),
//     a layer's output replaces the hidden image in place (stride 32) after its last MFMA.
//   C/D: lane l, register r of tile `to` = unit 32 to + (r & 3) + 8 (r >> 2) + 4 (l >> 5) of row l & 31;
//     the bias is the accumulator's initial value, the activation runs on the registers.
// The heads are layers of one tile (rows past 4 / 1 are zero weights); lanes 0..31 hold their
// row's action mean in registers 0..3 and its value in register 0, and sample / store from there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/f16env.h"
#include "f16_host.h"
#include "f16_rng.h"

namespace f16 {

typedef float pol_f32x16 __attribute__((ext_vector_type(16)));
typedef float pol_f32x4 __attribute__((ext_vector_type(4)));

constexpr int POL_WAVES = 4;           // waves (row tiles) per block
constexpr int POL_ROWS = 32;           // rows per wave
constexpr int POL_XS = 33;             // row stride of the staged observation image (floats)
constexpr int POL_LDS_BYTES = 160 * 1024;
constexpr int POL_MAX_LAYERS = 3;
constexpr int POL_OPS = 2 * (POL_MAX_LAYERS + 1);  // pi layers, pi head, vf layers, vf head

struct PolicyOp {
  int32_t w_off, b_off;  // floats into the blob
  int32_t nks;           // k-steps (pairs of inputs)
  int32_t tout;          // output tiles of 32 units
};
struct PolicyArgs {
  const float* blob;
  const float* obs;
  const float* eps;
  float* actions;
  float* values;
  float* log_probs;
  int64_t n, row_stride, frame_stride, id_base;
  uint64_t seed, step;
  int32_t K, in_dim, obs_floats, hid_floats, blob_floats, n_pi, n_vf, relu, flags, logstd_off;
  PolicyOp ops[POL_OPS];
};

__device__ __forceinline__ int pol_unit(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// f(std::integral_constant<int, T>()) for the T = op.tout tiles (1..4) of a hidden layer: the one
// place where a width of the descriptor picks a template instance
template <class F>
__device__ __forceinline__ void policy_tiles(const PolicyOp op, F&& f) {
  switch (op.tout) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
  }
}

// acc[to] = bias + W[to] X over nks k-steps (see the operand maps above)
template <int TOUT>
__device__ __forceinline__ void policy_gemm(const float* __restrict__ wb, const PolicyOp op, const float* xin,
                                            const int xstride, const int lane, pol_f32x16 (&acc)[4]) {
  const int j = lane & 31, h = lane >> 5;
  const float* bias = wb + op.b_off;
#pragma unroll
  for (int to = 0; to < TOUT; ++to) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[to][r] = bias[32 * to + pol_unit(r, h)];
  }
  const float* xp = xin + h * xstride + j;
  const float* wp = wb + op.w_off + lane;
  const int nks = op.nks;
  // batches of four k-steps; the next batch's operands are loaded ahead of this batch's MFMAs
  // (the last batch re-reads itself: no branch, nothing out of bounds)
  const int nb = nks >> 2;
  float b[4], w[TOUT][4];
  if (nb > 0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      b[u] = xp[2 * u * xstride];
#pragma unroll
      for (int to = 0; to < TOUT; ++to) w[to][u] = wp[(to * nks + u) * 64];
    }
  }
  for (int q = 0; q < nb; ++q) {
    const int sn = 4 * (q + 1 < nb ? q + 1 : q);
    float bn[4], wn[TOUT][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      bn[u] = xp[2 * (sn + u) * xstride];
#pragma unroll
      for (int to = 0; to < TOUT; ++to) wn[to][u] = wp[(to * nks + sn + u) * 64];
    }
    __builtin_amdgcn_sched_barrier(0);  // keep the loads a whole batch ahead (the scheduler sinks them otherwise)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int to = 0; to < TOUT; ++to) acc[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[to][u], b[u], acc[to], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      b[u] = bn[u];
#pragma unroll
      for (int to = 0; to < TOUT; ++to) w[to][u] = wn[to][u];
    }
  }
  int s = 4 * nb;
  for (; s < nks; ++s) {
    const float b = xp[2 * s * xstride];
#pragma unroll
    for (int to = 0; to < TOUT; ++to)
      acc[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[(to * nks + s) * 64], b, acc[to], 0, 0, 0);
  }
}

// tanh(v) = sign(v) (1 - t) / (1 + t), t = exp(-2 |v|), on the hardware exp2 and reciprocal (about
// 1 ulp each): absolute error <= ~2e-7 everywhere (the relative error grows below |v| ~ 0.1, where
// 1 - t cancels), NaN passes, +-inf gives +-1. libm's tanhf, inlined 128 times per row, was the
// largest single cost of the kernel.
__device__ __forceinline__ float policy_tanh(const float v) {
  const float t = __builtin_amdgcn_exp2f(-2.8853900817779268f * fabsf(v));  // 2 log2(e)
  return copysignf((1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t), v);
}

// one hidden layer: the activation of the accumulators replaces the hidden image (stride 32)
template <int TOUT>
__device__ __forceinline__ void policy_hidden(const float* __restrict__ wb, const PolicyOp op, const float* xin,
                                              const int xstride, float* hs, const int relu, const int lane,
                                              pol_f32x16 (&acc)[4]) {
  policy_gemm<TOUT>(wb, op, xin, xstride, lane, acc);
  __builtin_amdgcn_wave_barrier();  // every read of the input image is ahead of the writes below
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int to = 0; to < TOUT; ++to) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = acc[to][r];
      hs[(32 * to + pol_unit(r, h)) * POL_ROWS + j] = relu ? (v < 0.0f ? 0.0f : v) : policy_tanh(v);
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// The policy's noise stream (include/f16env.h): Philox4x32-10 keyed by seed, counter
// (gid, gid_hi ^ 'POLI', step), two Box-Muller pairs formed as rng_normals forms its own.
__device__ __forceinline__ void policy_normals(uint64_t seed, uint64_t gid, uint64_t step, float* e) {
  uint32_t o[4];
  philox((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gid, (uint32_t)(gid >> 32) ^ 0x504F4C49u, (uint32_t)step,
         (uint32_t)(step >> 32), o);
  const float s24 = 1.0f / 16777216.0f;
  const float u1 = ((float)(o[0] >> 8) + 0.5f) * s24, u2 = (float)(o[1] >> 8) * s24;
  const float u3 = ((float)(o[2] >> 8) + 0.5f) * s24, u4 = (float)(o[3] >> 8) * s24;
  const float r1 = sqrtf(-2.0f * logf(u1)), r2 = sqrtf(-2.0f * logf(u3));
  float s2, c2, s4, c4;
  sincospif(2.0f * u2, &s2, &c2);
  sincospif(2.0f * u4, &s4, &c4);
  e[0] = r1 * c2;
  e[1] = r1 * s2;
  e[2] = r2 * c4;
  e[3] = r2 * s4;
}

// A row's epilogue, by the lane that holds its action mean: eps from the caller, from the policy's
// Philox stream, or zero (deterministic); action = mean + exp(log_std) eps and its log-prob, stored.
// A: PolicyArgs or LmaArgs (the same fields); wb: where the kernel reads the blob.
template <class A>
__device__ __forceinline__ void policy_sample(const A& a, const float* wb, const int64_t row, const float (&mean)[4]) {
  float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!(a.flags & F16_POLICY_DETERMINISTIC)) {
    if (a.eps) {
      const float4 ev = reinterpret_cast<const float4*>(a.eps)[row];
      e[0] = ev.x; e[1] = ev.y; e[2] = ev.z; e[3] = ev.w;
    } else {
      policy_normals(a.seed, (uint64_t)(a.id_base + row), a.step, e);
    }
  }
  const float4 ls = *reinterpret_cast<const float4*>(wb + a.logstd_off);
  const float lsv[4] = {ls.x, ls.y, ls.z, ls.w};
  float av[4], lp = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    av[c] = mean[c] + expf(lsv[c]) * e[c];
    lp += -0.5f * e[c] * e[c] - lsv[c] - 0.91893853320467274f;  // 0.5 log(2 pi)
  }
  reinterpret_cast<float4*>(a.actions)[row] = make_float4(av[0], av[1], av[2], av[3]);
  a.log_probs[row] = lp;
}

template <int D, bool WLDS>
__global__ __launch_bounds__(64 * POL_WAVES) void f16_policy_forward_kernel(const PolicyArgs a) {
  extern __shared__ float4 pol_sm4[];
  float* sm = reinterpret_cast<float*>(pol_sm4);
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* wb = a.blob;
  if (WLDS) {  // the whole blob into LDS, shared by the block's waves
    const pol_f32x4* src = reinterpret_cast<const pol_f32x4*>(a.blob);
    pol_f32x4* dst = reinterpret_cast<pol_f32x4*>(pol_sm4);
    const int n4 = a.blob_floats >> 2;
    constexpr int NT = 64 * POL_WAVES, U = 8;  // eight 16-B loads in flight per thread, then their LDS writes
    for (int i0 = tid; i0 < n4; i0 += NT * U) {
      pol_f32x4 t[U];
      // (indices past the end repeat the last element, load and write alike: no branch per element)
#pragma unroll
      for (int u = 0; u < U; ++u) t[u] = src[i0 + NT * u < n4 ? i0 + NT * u : n4 - 1];
      __builtin_amdgcn_sched_barrier(0);  // all the loads issue before the first write waits for its own
#pragma unroll
      for (int u = 0; u < U; ++u) dst[i0 + NT * u < n4 ? i0 + NT * u : n4 - 1] = t[u];
    }
    __syncthreads();
    wb = sm;
  }
  const int64_t row0 = ((int64_t)blockIdx.x * POL_WAVES + wave) * POL_ROWS;
  if (row0 >= a.n) return;  // (after the block's only barrier)
  float* xs = sm + (WLDS ? a.blob_floats : 0) + wave * (a.obs_floats + a.hid_floats);
  float* hs = xs + a.obs_floats;
  const int j = lane & 31, h = lane >> 5;

  // the wave's 32 rows, flattened (K, D) each, into xs[k * D + d][row]; rows past n - 1 repeat it
  // (two frames' loads in flight, then their LDS writes; indices past the end repeat the last
  // element or frame, load and write alike: no branch per element)
  constexpr int NE = (POL_ROWS * D + 63) / 64;
  for (int k0 = 0; k0 < a.K; k0 += 2) {
    float v[2][NE];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const float* fk = a.obs + (int64_t)(k0 + kk < a.K ? k0 + kk : a.K - 1) * a.frame_stride;
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const int e0 = lane + 64 * i, e = e0 < POL_ROWS * D ? e0 : POL_ROWS * D - 1, rj = e / D, d = e - rj * D;
        int64_t row = row0 + rj;
        row = row < a.n ? row : a.n - 1;
        v[kk][i] = fk[row * a.row_stride + d];  // (always a valid element: no branch per load)
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const int e0 = lane + 64 * i, e = e0 < POL_ROWS * D ? e0 : POL_ROWS * D - 1, rj = e / D, d = e - rj * D;
        xs[((k0 + kk < a.K ? k0 + kk : a.K - 1) * D + d) * POL_XS + rj] = v[kk][i];
      }
    }
  }
  if ((a.in_dim & 1) && lane < POL_ROWS) xs[a.in_dim * POL_XS + lane] = 0.0f;  // the zero-weight pad input
  __builtin_amdgcn_wave_barrier();

  pol_f32x16 acc[4];
  float mean[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float value = 0.0f;
  for (int br = (a.flags & F16_POLICY_VALUE_ONLY) ? 1 : 0; br < 2; ++br) {
    const int base = br * (POL_MAX_LAYERS + 1);
    const int nl = br ? a.n_vf : a.n_pi;
    const float* xin = xs;
    int xstride = POL_XS;
    for (int l = 0; l < nl; ++l) {
      const PolicyOp op = a.ops[base + l];
      policy_tiles(op, [&](auto t) { policy_hidden<decltype(t)::value>(wb, op, xin, xstride, hs, a.relu, lane, acc); });
      xin = hs;
      xstride = POL_ROWS;
    }
    policy_gemm<1>(wb, a.ops[base + POL_MAX_LAYERS], xin, xstride, lane, acc);
    __builtin_amdgcn_wave_barrier();
    if (br == 0) {
      mean[0] = acc[0][0]; mean[1] = acc[0][1]; mean[2] = acc[0][2]; mean[3] = acc[0][3];
    } else {
      value = acc[0][0];
    }
  }

  const int64_t row = row0 + j;
  if (h != 0 || row >= a.n) return;
  a.values[row] = value;
  if (a.flags & F16_POLICY_VALUE_ONLY) return;
  policy_sample(a, wb, row, mean);
}

// ------------------------------------------------------------------------------------------
// The backward (f16env_policy_backward): grad_blob = sum over rows of d_mean . d mean / d blob +
// d_values d value / d blob, in the blob's own layout. A wave owns 32 rows at a time, as in the
// forward, and keeps per tile in its own LDS: the observation image, ONE branch's recomputed
// activations (an image per layer) and a delta image [unit][row], all at the row stride POL_XS
// (33: a lane walks them across units as well as across rows). Per layer, from the head down:
//   dW^T = X^T Delta   MFMA rows = 32 inputs, columns = 32 units, k = the tile's 32 rows
//     A: lane l holds X[row 2 s + (l >> 5)] of input 32 ti + (l & 31)   (input image, across inputs)
//     B: lane l holds Delta[row 2 s + (l >> 5)] of unit 32 to + (l & 31) (delta image, across units)
//     C: register r = input 32 ti + pol_unit(r, l >> 5), unit 32 to + (l & 31): blob element
//        w_off + ((to 2 nks + input) 32 + unit), so a register of 32 lanes is one 128-B line
//   Delta_prev^T = W^T Delta^T   MFMA rows = 32 inputs, k = units, columns = the 32 rows
//     A: lane l holds W[unit 32 to + 16 (l >> 5) + s][input 32 ti + (l & 31)], s = 0..15: sixteen
//        consecutive floats of the packed layer (k runs over the units in that order; B agrees)
//     B: lane l holds Delta[unit 32 to + 16 (l >> 5) + s][row l & 31]
//     C: as the forward's; times the activation's derivative on the stored h, into the delta image
//   db = the delta image summed along its rows.
// The wave accumulates into its own slice of the workspace (slot = block * waves + wave; tiles
// slot, slot + slots, ...), first tile stored, later tiles added in tile order; a second kernel
// sums the slices that got a tile in slot order. No atomics: the bits depend on (desc, n,
// max_blocks) alone.
constexpr int POL_BWD_BLOCKS = 256;  // default grid limit: the MI355X's CU count
constexpr int POL_OFF_VF0 = 6;       // policy_layout's slot of the vf branch's first hidden layer (6 b + 2 l, b = 1)

struct PolicyBwdArgs {
  const float* blob;
  const float* obs;
  const float* d_mean;
  const float* d_values;
  float* ws;
  int64_t n, row_stride, frame_stride, ntiles, nslots;
  int32_t K, in_dim, obs_floats, act_floats, wave_floats, blob_floats, n_pi, n_vf, relu, waves;
  PolicyOp ops[POL_OPS];
};

// one hidden layer of the recompute: the forward's chain and activation, into the layer's own image
template <int TOUT>
__device__ __forceinline__ void policy_bwd_hidden(const float* __restrict__ wb, const PolicyOp op, const float* xin,
                                                  float* hout, const int relu, const int lane, pol_f32x16 (&acc)[4]) {
  policy_gemm<TOUT>(wb, op, xin, POL_XS, lane, acc);
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int to = 0; to < TOUT; ++to) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = acc[to][r];
      hout[(32 * to + pol_unit(r, h)) * POL_XS + j] = relu ? (v < 0.0f ? 0.0f : v) : policy_tanh(v);
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// the slice's weight piece (+)= X^T Delta over the tile's rows (inputs past the piece are not stored)
template <int TOUT>
__device__ __forceinline__ void policy_bwd_dw(float* g, const PolicyOp op, const float* xin, const float* dl,
                                              const bool first, const int lane) {
  const int j = lane & 31, h = lane >> 5;
  const int nin = 2 * op.nks;
  float* gp = g + op.w_off + j;
  const float* dp = dl + j * POL_XS + h;
  for (int i0 = 0; i0 < nin; i0 += 32) {
    pol_f32x16 acc[TOUT];
#pragma unroll
    for (int to = 0; to < TOUT; ++to) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = i0 + pol_unit(r, h);
        acc[to][r] = (first || i >= nin) ? 0.0f : gp[(to * nin + i) * 32];
      }
    }
    const int ia = i0 + j < nin ? i0 + j : nin - 1;  // (rows of the MFMA past the piece repeat its last input)
    const float* xp = xin + ia * POL_XS + h;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float x = xp[2 * s];
#pragma unroll
      for (int to = 0; to < TOUT; ++to)
        acc[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, dp[to * 32 * POL_XS + 2 * s], acc[to], 0, 0, 0);
    }
#pragma unroll
    for (int to = 0; to < TOUT; ++to) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = i0 + pol_unit(r, h);
        if (i < nin) gp[(to * nin + i) * 32] = acc[to][r];
      }
    }
  }
}

// the 32 row values of one unit summed in row order (f16env_policy_backward's bias sum)
struct PolicyRowSum {
  __device__ __forceinline__ float operator()(const float* src) const {
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < POL_ROWS; ++r) s += src[r];
    return s;
  }
};

// the slice's bias piece (+)= the delta image summed over the tile's rows by SUM (each backward
// kernel keeps its own order of that sum: the bits differ)
template <class SUM>
__device__ __forceinline__ void policy_bwd_db(float* g, const PolicyOp op, const float* dl, const bool first,
                                              const int lane) {
  for (int u = lane; u < 32 * op.tout; u += 64) {
    const float s = SUM()(dl + u * POL_XS);
    float* p = g + op.b_off + u;
    *p = first ? s : *p + s;
  }
}

// the delta image <- (W^T Delta) act'(h) for the layer below `op` (TIN tiles wide, image hprev);
// rows past n - 1 (valid == false for the lane's row) are forced to 0
template <int TIN>
__device__ __forceinline__ void policy_bwd_delta(const float* __restrict__ wb, const PolicyOp op, const float* hprev,
                                                 float* dl, const int relu, const bool valid, const int lane) {
  const int j = lane & 31, h = lane >> 5;
  pol_f32x16 acc[TIN];
#pragma unroll
  for (int ti = 0; ti < TIN; ++ti) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ti][r] = 0.0f;
  }
  for (int to = 0; to < op.tout; ++to) {
    float b[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) b[s] = dl[(32 * to + 16 * h + s) * POL_XS + j];
#pragma unroll
    for (int ti = 0; ti < TIN; ++ti) {
      const pol_f32x4* wp =
          reinterpret_cast<const pol_f32x4*>(wb + op.w_off + ((to * 2 * op.nks + 32 * ti + j) * 32 + 16 * h));
      const pol_f32x4 w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3];
      const float w[16] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3],
                           w2[0], w2[1], w2[2], w2[3], w3[0], w3[1], w3[2], w3[3]};
#pragma unroll
      for (int s = 0; s < 16; ++s) acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[s], b[s], acc[ti], 0, 0, 0);
    }
  }
  __builtin_amdgcn_wave_barrier();  // every read of the delta image is ahead of the writes below
#pragma unroll
  for (int ti = 0; ti < TIN; ++ti) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = 32 * ti + pol_unit(r, h);
      const float hv = hprev[i * POL_XS + j], d = acc[ti][r];
      const float v = relu ? (hv > 0.0f ? d : 0.0f) : d * (1.0f - hv * hv);
      dl[i * POL_XS + j] = valid ? v : 0.0f;
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// One branch (br: 0 pi, 1 vf) of a tile's backward, from the first layers' input image x0 (stride
// POL_XS): recompute the branch's activation images into `as`, write the head's delta into dl, then
// for l = nl .. 0 the layer's dW and db (db summed by SUM) and, above layer 0, the delta of the layer
// below. On return dl holds layer 0's delta: what it hands down, if anything, is the caller's.
// A: PolicyBwdArgs or LmaBwdArgs (the same fields).
template <class SUM, class A>
__device__ __forceinline__ void policy_bwd_branch(const A& a, const int br, const float* x0, float* as, float* dl, float* g,
                                                  const int64_t row, const bool valid, const bool first, const int lane,
                                                  pol_f32x16 (&acc)[4]) {
  const int j = lane & 31, h = lane >> 5;
  const float* wb = a.blob;
  const float* dout = br ? a.d_values : a.d_mean;
  const int base = br * (POL_MAX_LAYERS + 1);
  const int nl = br ? a.n_vf : a.n_pi;
  // recompute the branch's activations, layer l into the image at as + 32 POL_XS (tiles below l)
  {
    const float* xin = x0;
    float* hout = as;
    for (int l = 0; l < nl; ++l) {
      const PolicyOp op = a.ops[base + l];
      policy_tiles(op, [&](auto t) { policy_bwd_hidden<decltype(t)::value>(wb, op, xin, hout, a.relu, lane, acc); });
      xin = hout;
      hout += 32 * op.tout * POL_XS;
    }
  }
  // the head's delta: d_mean (units 0..3) or d_values (unit 0) of the rows inside n, zero elsewhere
  {
    float dv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (valid && h == 0) {
      if (br == 0) {
        const float4 m = reinterpret_cast<const float4*>(dout)[row];
        dv[0] = m.x; dv[1] = m.y; dv[2] = m.z; dv[3] = m.w;
      } else {
        dv[0] = dout[row];
      }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) dl[(16 * h + q) * POL_XS + j] = q < 4 ? dv[q] : 0.0f;
    __builtin_amdgcn_wave_barrier();
  }
  for (int l = nl; l >= 0; --l) {
    const PolicyOp op = a.ops[base + (l == nl ? POL_MAX_LAYERS : l)];
    int below = 0;  // tiles of the layers under layer l - 1: where its image starts
    for (int m = 0; m + 1 < l; ++m) below += a.ops[base + m].tout;
    const float* xin = l == 0 ? x0 : as + 32 * below * POL_XS;
    policy_tiles(op, [&](auto t) { policy_bwd_dw<decltype(t)::value>(g, op, xin, dl, first, lane); });
    policy_bwd_db<SUM>(g, op, dl, first, lane);
    if (l == 0) break;
    policy_tiles(a.ops[base + l - 1],
                 [&](auto t) { policy_bwd_delta<decltype(t)::value>(wb, op, xin, dl, a.relu, valid, lane); });
  }
}

template <int D>
__global__ __launch_bounds__(64 * POL_WAVES) void f16_policy_backward_kernel(const PolicyBwdArgs a) {
  extern __shared__ float4 pol_sm4[];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j = lane & 31;
  float* xs = reinterpret_cast<float*>(pol_sm4) + wave * a.wave_floats;
  float* as = xs + a.obs_floats;
  float* dl = as + a.act_floats;
  const int64_t slot = (int64_t)blockIdx.x * a.waves + wave;
  float* g = a.ws + slot * a.blob_floats;
  pol_f32x16 acc[4];
  bool first = true;
  for (int64_t t = slot; t < a.ntiles; t += a.nslots) {
    const int64_t row0 = t * POL_ROWS;
    // the tile's 32 rows, flattened (K, D) each, into xs[k * D + d][row]; rows past n - 1 repeat it
    for (int k = 0; k < a.K; ++k) {
      const float* fk = a.obs + (int64_t)k * a.frame_stride;
      for (int e = lane; e < POL_ROWS * D; e += 64) {
        const int rj = e / D, d = e - rj * D;
        int64_t row = row0 + rj;
        row = row < a.n ? row : a.n - 1;
        xs[(k * D + d) * POL_XS + rj] = fk[row * a.row_stride + d];
      }
    }
    if ((a.in_dim & 1) && lane < POL_ROWS) xs[a.in_dim * POL_XS + lane] = 0.0f;  // the zero-weight pad input
    __builtin_amdgcn_wave_barrier();
    const int64_t row = row0 + j;
    const bool valid = row < a.n;

    // (no gradient to the observation: the branch's backward ends after the first layer's dW and db)
    for (int br = 0; br < 2; ++br)
      if (br ? a.d_values : a.d_mean) policy_bwd_branch<PolicyRowSum>(a, br, xs, as, dl, g, row, valid, first, lane, acc);
    __builtin_amdgcn_wave_barrier();  // the next tile's staging follows every read of this one's images
    first = false;
  }
}

// grad[p] = the slots' partials (slot_floats apart) summed in slot order. +0 where nothing is
// trained: p in [zero0, zero1) (log_std to the blob's end for the MLP policy; log_std and the PE
// table, neighbours in the LMA blob) and the MLP pieces of a branch without an upstream gradient
// (bit br of skip), which no slot wrote.
__global__ __launch_bounds__(256) void f16_policy_backward_reduce_kernel(const float* __restrict__ ws,
                                                                         float* __restrict__ grad, const int nf,
                                                                         const int64_t slot_floats, const int64_t nact,
                                                                         const int vf0, const int act_w, const int val_w,
                                                                         const int zero0, const int zero1, const int skip) {
  const int p = (int)(blockIdx.x * 256 + threadIdx.x);
  if (p >= nf) return;
  float s = 0.0f;
  bool sum = p < zero0 || p >= zero1;
  if (p < zero0) {
    const int br = p >= val_w ? 1 : (p >= act_w ? 0 : (p >= vf0 ? 1 : 0));
    sum = !((skip >> br) & 1);
  }
  if (sum)
    for (int64_t k = 0; k < nact; ++k) s += ws[k * slot_floats + p];
  grad[p] = s;
}

// both backward launchers' reduce: skip from the NULL upstream gradients, the branch boundaries from `off`
static void policy_launch_reduce(hipStream_t stream, const float* ws, float* grad_blob, const int64_t nf,
                                 const int64_t slot_floats, const int64_t nact, const int64_t* off, const int64_t zero1,
                                 const float* d_mean, const float* d_values) {
  const int skip = (d_mean ? 0 : 1) | (d_values ? 0 : 2);
  hipLaunchKernelGGL(f16_policy_backward_reduce_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, stream, ws,
                     grad_blob, (int)nf, slot_floats, nact, (int)off[POL_OFF_VF0], (int)off[F16_POLICY_OFF_ACT_W],
                     (int)off[F16_POLICY_OFF_VAL_W], (int)off[F16_POLICY_OFF_LOG_STD], (int)zero1, skip);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static const char* policy_desc_error(const f16_policy_desc* d) {
  if (!d) return "null policy descriptor";
  if (d->K < 1 || d->K > 10) return "policy K must be in [1, 10]";
  if (d->D != 15 && d->D != 17) return "policy D must be 15 (frames) or 17 (features)";
  if (d->n_pi < 1 || d->n_pi > POL_MAX_LAYERS || d->n_vf < 1 || d->n_vf > POL_MAX_LAYERS)
    return "each policy branch has 1 to 3 hidden layers";
  for (int b = 0; b < 2; ++b)
    for (int l = 0; l < (b ? d->n_vf : d->n_pi); ++l) {
      const int w = b ? d->vf_width[l] : d->pi_width[l];
      if (w != 32 && w != 64 && w != 96 && w != 128) return "hidden widths must be 32, 64, 96 or 128";
    }
  if (d->activation != F16_POLICY_ACT_TANH && d->activation != F16_POLICY_ACT_RELU)
    return "policy activation must be F16_POLICY_ACT_TANH or F16_POLICY_ACT_RELU";
  return nullptr;
}

// The blob: per branch (pi, then vf) each hidden layer's weight as [tiles of 32 outputs][k-steps][2][32]
// (element = W[32 to + i][2 s + h], inputs past the layer's fan-in zero) then its bias; then the
// action head and the value head in the same form as one tile each (outputs past 4 / 1 zero, a bias of
// 32); then log_std[4]. Every piece starts on a multiple of 4 floats. fan_in0: the first layers'
// fan-in when it is not K D (the LMA extractor's features, f16_policy_lma.h).
static int64_t policy_layout(const f16_policy_desc* d, int64_t* off, PolicyOp* ops, const int fan_in0 = 0) {
  int64_t p = 0;
  for (int i = 0; i < F16_POLICY_N_OFFSETS; ++i) off[i] = -1;
  for (int pass = 0; pass < 2; ++pass) {  // the hidden layers of both branches, then the two heads
    for (int b = 0; b < 2; ++b) {
      int fan_in = fan_in0 ? fan_in0 : d->K * d->D;
      const int nl = b ? d->n_vf : d->n_pi;
      for (int l = 0; l <= nl; ++l) {  // l == nl: the branch's head
        const bool head = l == nl;
        const int width = head ? 32 : (b ? d->vf_width[l] : d->pi_width[l]);
        if (head == (pass == 1)) {
          const int nks = (fan_in + 1) / 2, tout = width / 32;
          const int slot = head ? (b ? F16_POLICY_OFF_VAL_W : F16_POLICY_OFF_ACT_W) : 6 * b + 2 * l;
          off[slot] = p;
          p += (int64_t)tout * nks * 64;
          off[slot + 1] = p;
          p += width;
          if (ops) {
            PolicyOp& o = ops[b * (POL_MAX_LAYERS + 1) + (head ? POL_MAX_LAYERS : l)];
            o.w_off = (int32_t)off[slot]; o.b_off = (int32_t)off[slot + 1]; o.nks = nks; o.tout = tout;
          }
        }
        fan_in = width;
      }
    }
  }
  off[F16_POLICY_OFF_LOG_STD] = p;
  return p + 4;
}

// the widest hidden layer (at least one tile) and each branch's sum of widths
struct PolicyWidths {
  int max_w, sum[2];
};
static PolicyWidths policy_widths(const f16_policy_desc* d) {
  PolicyWidths w{32, {0, 0}};
  for (int b = 0; b < 2; ++b)
    for (int l = 0; l < (b ? d->n_vf : d->n_pi); ++l) {
      const int x = b ? d->vf_width[l] : d->pi_width[l];
      w.sum[b] += x;
      w.max_w = x > w.max_w ? x : w.max_w;
    }
  return w;
}

// More than 64 KB of dynamic LDS is opted into once per kernel instance and device (word: the
// instance's bit per device). A launcher does this and nothing else at n == 0: a caller about to
// capture a graph prepares the instance ahead of it.
static int policy_prepare_instance(const void* fn, uint64_t* word) {
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !(__atomic_load_n(word, __ATOMIC_ACQUIRE) >> dev & 1)) {
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, POL_LDS_BYTES));
    if (dev >= 0 && dev < 64) __atomic_fetch_or(word, 1ull << dev, __ATOMIC_RELEASE);
  }
  return 0;
}

// the arguments of the two forward entry points (entry: which one; features_out: the LMA's, else NULL)
static int policy_forward_check(const char* entry, uint32_t flags, int64_t n, const float* blob, const float* obs,
                                int64_t row_stride, int64_t frame_stride, const float* eps, const float* actions,
                                const float* values, const float* log_probs, const float* features_out) {
  if (flags & ~(uint32_t)(F16_POLICY_DETERMINISTIC | F16_POLICY_VALUE_ONLY))
    return set_err(-1, (std::string("unknown ") + entry + " flags").c_str());
  if (n < 0) return set_err(-1, "n must be >= 0");
  if (n == 0) return 0;
  const bool vonly = (flags & F16_POLICY_VALUE_ONLY) != 0;
  if (!blob || !obs || !values || (!vonly && (!actions || !log_probs))) return set_err(-1, "null argument");
  if (((uintptr_t)blob & 15) != 0) return set_err(-1, "the weight blob must be 16-byte aligned");
  if (((uintptr_t)obs & 3) != 0 || ((uintptr_t)values & 3) != 0 || ((uintptr_t)log_probs & 3) != 0)
    return set_err(-1, "obs, values and log_probs must be float-aligned");
  if (!vonly && (((uintptr_t)actions & 15) != 0 || ((uintptr_t)eps & 15) != 0))
    return set_err(-1, "actions and eps must be 16-byte aligned");
  if (((uintptr_t)features_out & 15) != 0) return set_err(-1, "features_out must be 16-byte aligned");
  if (row_stride < 0 || frame_stride < 0) return set_err(-1, "strides must be non-negative");
  return 0;
}

// the arguments of the two backward entry points at n > 0 (ws_entry: the one that sizes the workspace)
static int policy_backward_check(const char* ws_entry, const float* blob, const float* obs, int64_t row_stride,
                                 int64_t frame_stride, const float* d_mean, const float* d_values, const void* workspace,
                                 int64_t workspace_bytes, int64_t need_bytes, const float* grad_blob) {
  if (!blob || !obs || !workspace || !grad_blob) return set_err(-1, "null argument");
  if (!d_mean && !d_values) return set_err(-1, "d_mean and d_values are both NULL");
  if (((uintptr_t)blob & 15) != 0 || ((uintptr_t)grad_blob & 15) != 0 || ((uintptr_t)d_mean & 15) != 0 ||
      ((uintptr_t)workspace & 15) != 0)
    return set_err(-1, "blob, grad_blob, d_mean and the workspace must be 16-byte aligned");
  if (((uintptr_t)obs & 3) != 0 || ((uintptr_t)d_values & 3) != 0)
    return set_err(-1, "obs and d_values must be float-aligned");
  if (row_stride < 0 || frame_stride < 0) return set_err(-1, "strides must be non-negative");
  if (workspace_bytes < need_bytes)
    return set_err(-1, (std::string("the workspace is smaller than ") + ws_entry + " says").c_str());
  return 0;
}

static int policy_forward_impl(void* stream, const f16_policy_desc* desc, const float* blob, int64_t n, const float* obs,
                               int64_t row_stride, int64_t frame_stride, uint64_t seed, uint64_t step, int64_t id_base,
                               const float* eps, float* actions, float* values, float* log_probs, uint32_t flags) {
  if (const char* m = policy_desc_error(desc)) return set_err(-1, m);
  if (int rc = policy_forward_check("f16env_policy_forward", flags, n, blob, obs, row_stride, frame_stride, eps, actions,
                                    values, log_probs, nullptr))
    return rc;
  const bool vonly = (flags & F16_POLICY_VALUE_ONLY) != 0;
  PolicyArgs a{};
  int64_t off[F16_POLICY_N_OFFSETS];
  const int64_t nf = policy_layout(desc, off, a.ops);
  a.K = desc->K;
  a.in_dim = desc->K * desc->D;
  a.obs_floats = (a.in_dim + (a.in_dim & 1)) * POL_XS;
  a.hid_floats = policy_widths(desc).max_w * POL_ROWS;
  a.blob_floats = (int32_t)nf;
  const int64_t tiles = (int64_t)POL_WAVES * (a.obs_floats + a.hid_floats) * 4;
  const bool wlds = nf * 4 + tiles <= POL_LDS_BYTES;
  const int64_t lds = tiles + (wlds ? nf * 4 : 0);
  const void* fn = desc->D == 15
      ? (wlds ? (const void*)f16_policy_forward_kernel<15, true> : (const void*)f16_policy_forward_kernel<15, false>)
      : (wlds ? (const void*)f16_policy_forward_kernel<17, true> : (const void*)f16_policy_forward_kernel<17, false>);
  const int64_t blocks = (n + POL_WAVES * POL_ROWS - 1) / (POL_WAVES * POL_ROWS);
  if (blocks > 0x7fffffffLL) return set_err(-1, "n too large");
  static uint64_t prepared[4];
  if (int rc = policy_prepare_instance(fn, &prepared[(desc->D == 17 ? 2 : 0) + (wlds ? 1 : 0)])) return rc;
  if (n == 0) return 0;
  a.blob = blob; a.obs = obs; a.eps = vonly ? nullptr : eps;
  a.actions = actions; a.values = values; a.log_probs = log_probs;
  a.n = n; a.row_stride = row_stride; a.frame_stride = frame_stride; a.id_base = id_base;
  a.seed = seed; a.step = step;
  a.n_pi = desc->n_pi; a.n_vf = desc->n_vf;
  a.relu = desc->activation == F16_POLICY_ACT_RELU ? 1 : 0;
  a.flags = (int32_t)flags;
  a.logstd_off = (int32_t)off[F16_POLICY_OFF_LOG_STD];
  void* kargs[] = {&a};
  HIPCHK(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(64 * POL_WAVES), kargs, (size_t)lds, (hipStream_t)stream));
  return 0;
}

// The backward's launch shape, from the descriptor alone. LDS per wave: the observation image
// (K D rounded up to even inputs), the wider branch's activation images (the sum of its widths)
// and a delta image (the widest layer), all x POL_XS floats; waves per block: the most of 4, 2, 1
// whose images fit POL_LDS_BYTES. grid = min(ceil(tiles / waves), max_blocks or POL_BWD_BLOCKS).
struct PolicyBwdPlan {
  int32_t obs_floats, act_floats, wave_floats, waves;
  int64_t nf, ntiles, grid;
};
static int policy_bwd_plan(const f16_policy_desc* desc, int64_t n, int32_t max_blocks, PolicyBwdPlan* p,
                           int64_t* off, PolicyOp* ops) {
  if (const char* m = policy_desc_error(desc)) return set_err(-1, m);
  if (n < 0) return set_err(-1, "n must be >= 0");
  if (max_blocks < 0) return set_err(-1, "max_blocks must be >= 0 (0: the default)");
  p->nf = policy_layout(desc, off, ops);
  const PolicyWidths w = policy_widths(desc);
  const int in_dim = desc->K * desc->D;
  p->obs_floats = (in_dim + (in_dim & 1)) * POL_XS;
  p->act_floats = (w.sum[0] > w.sum[1] ? w.sum[0] : w.sum[1]) * POL_XS;
  p->wave_floats = p->obs_floats + p->act_floats + w.max_w * POL_XS;
  const int64_t per_wave = (int64_t)p->wave_floats * 4;
  if (per_wave > POL_LDS_BYTES) return set_err(-1, "the policy's backward images do not fit the LDS for one wave");
  p->waves = 4 * per_wave <= POL_LDS_BYTES ? 4 : (2 * per_wave <= POL_LDS_BYTES ? 2 : 1);
  p->ntiles = n / POL_ROWS + (n % POL_ROWS != 0);
  const int64_t want = (p->ntiles + p->waves - 1) / p->waves, lim = max_blocks ? max_blocks : POL_BWD_BLOCKS;
  p->grid = want < lim ? want : lim;
  return 0;
}

static int policy_backward_workspace_impl(const f16_policy_desc* desc, int64_t n, int32_t max_blocks, int64_t* bytes_out) {
  PolicyBwdPlan p;
  int64_t off[F16_POLICY_N_OFFSETS];
  if (int rc = policy_bwd_plan(desc, n, max_blocks, &p, off, nullptr)) return rc;
  if (!bytes_out) return set_err(-1, "null argument");
  *bytes_out = p.grid * p.waves * p.nf * 4;
  return 0;
}

static int policy_backward_impl(void* stream, const f16_policy_desc* desc, const float* blob, int64_t n, const float* obs,
                                int64_t row_stride, int64_t frame_stride, const float* d_mean, const float* d_values,
                                void* workspace, int64_t workspace_bytes, int32_t max_blocks, float* grad_blob) {
  PolicyBwdArgs a{};
  PolicyBwdPlan p;
  int64_t off[F16_POLICY_N_OFFSETS];
  if (int rc = policy_bwd_plan(desc, n, max_blocks, &p, off, a.ops)) return rc;
  if (n > 0)
    if (int rc = policy_backward_check("f16env_policy_backward_workspace", blob, obs, row_stride, frame_stride, d_mean,
                                       d_values, workspace, workspace_bytes, p.grid * p.waves * p.nf * 4, grad_blob))
      return rc;
  const void* fn = desc->D == 15 ? (const void*)f16_policy_backward_kernel<15> : (const void*)f16_policy_backward_kernel<17>;
  static uint64_t prepared[2];
  if (int rc = policy_prepare_instance(fn, &prepared[desc->D == 17 ? 1 : 0])) return rc;
  if (n == 0) return 0;
  a.blob = blob; a.obs = obs; a.d_mean = d_mean; a.d_values = d_values;
  a.ws = static_cast<float*>(workspace);
  a.n = n; a.row_stride = row_stride; a.frame_stride = frame_stride;
  a.ntiles = p.ntiles; a.nslots = p.grid * p.waves;
  a.K = desc->K; a.in_dim = desc->K * desc->D;
  a.obs_floats = p.obs_floats; a.act_floats = p.act_floats; a.wave_floats = p.wave_floats;
  a.blob_floats = (int32_t)p.nf;
  a.n_pi = desc->n_pi; a.n_vf = desc->n_vf;
  a.relu = desc->activation == F16_POLICY_ACT_RELU ? 1 : 0;
  a.waves = p.waves;
  void* kargs[] = {&a};
  HIPCHK(hipLaunchKernel(fn, dim3((unsigned)p.grid), dim3(64 * p.waves), kargs, (size_t)p.waves * p.wave_floats * 4,
                         (hipStream_t)stream));
  // (the slots that got a tile; nothing from log_std to the blob's end is trained here)
  policy_launch_reduce((hipStream_t)stream, a.ws, grad_blob, p.nf, p.nf, p.ntiles < a.nslots ? p.ntiles : a.nslots, off,
                       p.nf, d_mean, d_values);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace f16
