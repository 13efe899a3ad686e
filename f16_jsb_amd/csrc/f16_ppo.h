// f16_ppo.h -- what lies between the policy's forward and its new weights in a PPO minibatch
// update, as HIP kernels (gfx950): the loss head (f16env_ppo_loss_head) and the clipped Adam step on
// the blob (f16env_ppo_adam_step); include/f16env.h, still ABI 7. Needs f16_host.h (set_err,
// HIPCHK).
//
// stable_baselines3/ppo/ppo.py:355-388 with a DiagGaussianDistribution (distributions.py): float32
// gradients per row, the ratio and the statistics' terms in fp64 (include/f16env.h says where that
// differs from torch), every sum over rows or over the blob in fp64 and in a fixed order:
//   head, launch 1 (normalised advantages, n > 1): one block of 1024 threads; thread t adds
//     A[t], A[t + 1024], ... in index order, the 1024 sums meet in a halving tree (stride 512, 256,
//     ..., 1); the mean, then the same again over (A - mean)^2 for the unbiased std.
//   head, launch 2: blocks of 256 threads, thread t of block b takes rows 256 (b + k grid) + t,
//     k = 0, 1, ... in that order, and keeps eight fp64 sums of its own; the block's 256 meet in the
//     same halving tree; the block writes its eight sums to the workspace.
//   step: ONE block of 1024 threads. It adds the head's partials in block order, writes d_log_std
//     into grad_blob and the statistics, forms the squared norm (thread t adds g[t]^2,
//     g[t + 1024]^2, ... in index order, then the halving tree) and applies clip and Adam element by
//     element. One block, because the norm must be known before the first element moves and a blob
//     is 26 k to 117 k floats: a second launch or a grid-wide wait would cost more than the pass.
// No atomics, no inline assembly; the bits depend on the arguments and the data alone.
// AM-PPO (f16_ppo_am.h, which includes this file) shares two things defined here: the head kernel, a template
// whose <false> instance is the standard head above and whose <true> instance takes the modulated
// advantage of ppo_am_mod, and the step's prologue (ppo_step_prologue), which the DAG step repeats.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/f16env.h"
#include "f16_host.h"

namespace f16 {

constexpr int PPO_HEAD_THREADS = 256;
constexpr int PPO_HEAD_BLOCKS = 256;   // default limit of the head's grid
constexpr int PPO_WIDE = 1024;         // threads of the one-block kernels
constexpr int PPO_SUMS = 8;            // d_log_std[4], policy, value, approx_kl, clip count
constexpr int PPO_HEADER = 4;          // doubles ahead of the partials: adv mean, adv std, n, 0

struct PpoHeadArgs {
  const float* mean; const float* values; const float* actions;
  const float* old_log_prob; const float* advantages; const float* target_values;
  const float* log_std; const float* hyper;
  float* d_mean; float* d_values;
  double* ws;
  int64_t n;
  int32_t normalize;
  // the AM instance alone (f16_ppo_am.h): target_values holds old_values, ws[0], ws[1], ws[3] the
  // modulated advantages' mean, std and the minibatch's norm
  const float* dynago; const float* am_state;
};

// red[t] over t = 0 .. T-1 -> red[0], halving tree (T a power of two); every thread of the block calls it
template <int T>
__device__ __forceinline__ double ppo_block_sum(double* red, const int t, const double mine) {
  red[t] = mine;
  __syncthreads();
#pragma unroll
  for (int s = T / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();  // (red is reused by the caller)
  return out;
}

__global__ __launch_bounds__(PPO_WIDE) void f16_ppo_adv_stats_kernel(const float* __restrict__ adv, const int64_t n,
                                                                      double* __restrict__ ws) {
  __shared__ double red[PPO_WIDE];
  const int t = (int)threadIdx.x;
  double s = 0.0;
  for (int64_t i = t; i < n; i += PPO_WIDE) s += (double)adv[i];
  const double mean = ppo_block_sum<PPO_WIDE>(red, t, s) / (double)n;
  double q = 0.0;
  for (int64_t i = t; i < n; i += PPO_WIDE) {
    const double d = (double)adv[i] - mean;
    q += d * d;
  }
  const double ss = ppo_block_sum<PPO_WIDE>(red, t, q);
  if (t == 0) {
    ws[0] = mean;
    ws[1] = sqrt(ss / (double)(n - 1));
  }
}

// AM-PPO's modulated advantage (ppo.py:87-97 with update_ema = False), the one place it is formed:
// the AM head's statistics launch (f16_ppo_am.h) and its rows both call ppo_am_mod.
//   mod = |A| (kappa tanh(alpha A / (N + eps)) + v_shift), fp64 from the float32 inputs, alpha the
//   controller's state[0] as stored, N the minibatch's norm; n <= 1: mod = A (ppo.py:40-41)
struct PpoAmCoef {
  double alpha, den, kappa, v_shift;
  int32_t identity;
};

__device__ __forceinline__ PpoAmCoef ppo_am_coef(const float* dynago, const float* state, const double norm,
                                                 const int64_t n) {
  PpoAmCoef c;
  c.alpha = (double)state[0];
  c.den = norm + (double)dynago[F16_PPO_DYNAGO_EPS];
  c.kappa = (double)dynago[F16_PPO_DYNAGO_KAPPA];
  c.v_shift = (double)dynago[F16_PPO_DYNAGO_V_SHIFT];
  c.identity = n <= 1;
  return c;
}

__device__ __forceinline__ double ppo_am_mod(const float A, const PpoAmCoef& c) {
  const double a = (double)A;
  return c.identity ? a : fabs(a) * (c.kappa * tanh(c.alpha * a / c.den) + c.v_shift);
}

// AM = false: standard PPO's head. AM = true: f16env_ppo_loss_head_am's, the advantage and the value
// target from ppo_am_mod; every line outside the two `if constexpr` is shared
template <bool AM>
__global__ __launch_bounds__(PPO_HEAD_THREADS) void f16_ppo_head_kernel(const PpoHeadArgs a) {
  __shared__ double red[PPO_HEAD_THREADS];
  const int t = (int)threadIdx.x;
  const float clip = a.hyper[1], vf_coef = a.hyper[3];
  const double lo = 1.0 - (double)clip, hi = 1.0 + (double)clip;
  const float inv_n = 1.0f / (float)a.n;
  const double half_log_2pi = 0.918938533204672742;
  // the log-probability, the log-ratio, the ratio, the normalised advantage and the row's terms of
  // the statistics are formed in fp64 from the float32 inputs (the ratio's relative error is the
  // absolute error of a difference of two numbers near -5); the ratio and the advantage are then
  // rounded once, and the gradients are float32 from there
  float sigma[4], var[4];
  double ls[4], half_inv_var[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ls[j] = (double)a.log_std[j];
    const double s = exp(ls[j]);
    half_inv_var[j] = 0.5 / (s * s);
    sigma[j] = (float)s;
    var[j] = (float)(s * s);
  }
  double a_mean = 0.0, a_den = 1.0;
  if (a.normalize) {
    a_mean = a.ws[0];
    a_den = a.ws[1] + 1e-8;
  }
  double acc[PPO_SUMS];
#pragma unroll
  for (int k = 0; k < PPO_SUMS; ++k) acc[k] = 0.0;
  PpoAmCoef am{};
  if constexpr (AM) am = ppo_am_coef(a.dynago, a.am_state, a.ws[3], a.n);
  const int64_t stride = (int64_t)gridDim.x * PPO_HEAD_THREADS;
  for (int64_t row = (int64_t)blockIdx.x * PPO_HEAD_THREADS + t; row < a.n; row += stride) {
    const float4 m4 = reinterpret_cast<const float4*>(a.mean)[row];
    const float4 x4 = reinterpret_cast<const float4*>(a.actions)[row];
    const float mu[4] = {m4.x, m4.y, m4.z, m4.w}, ac[4] = {x4.x, x4.y, x4.z, x4.w};
    float d[4];
    double lp = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d[j] = ac[j] - mu[j];
      const double dd = (double)ac[j] - (double)mu[j];
      lp += -(dd * dd) * half_inv_var[j] - ls[j] - half_log_2pi;
    }
    const double log_r = lp - (double)a.old_log_prob[row];
    const double r64 = exp(log_r);
    const float r = (float)r64;
    float A;
    double mod = 0.0;
    if constexpr (AM) {
      mod = ppo_am_mod(a.advantages[row], am);
      A = a.normalize ? (float)((mod - a_mean) / a_den) : (float)mod;
    } else {
      A = a.normalize ? (float)(((double)a.advantages[row] - a_mean) / a_den) : a.advantages[row];
    }
    // torch.min over (s1, s2) with torch.clamp under autograd: the clamp passes the gradient on
    // [lo, hi] inclusive; outside it only the unclipped arm carries one, and only where it is the smaller
    const double s1 = (double)A * r64, s2 = (double)A * fmin(fmax(r64, lo), hi);
    const float ds_dr = ((r64 >= lo && r64 <= hi) || s1 < s2) ? A : 0.0f;
    const float g = (-inv_n * ds_dr) * r;
    float dm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dm[j] = g * (d[j] / var[j]);
      const float z = d[j] / sigma[j];
      acc[j] += (double)g * ((double)z * (double)z - 1.0);
    }
    reinterpret_cast<float4*>(a.d_mean)[row] = make_float4(dm[0], dm[1], dm[2], dm[3]);
    float dv;
    if constexpr (AM) dv = (float)((double)a.values[row] - (mod + (double)a.target_values[row]));
    else dv = a.values[row] - a.target_values[row];
    a.d_values[row] = (vf_coef * 2.0f * inv_n) * dv;
    acc[4] += -fmin(s1, s2);
    acc[5] += (double)dv * (double)dv;
    acc[6] += (r64 - 1.0) - log_r;
    acc[7] += fabs(r64 - 1.0) > (double)clip ? 1.0 : 0.0;
  }
#pragma unroll
  for (int k = 0; k < PPO_SUMS; ++k) {
    const double s = ppo_block_sum<PPO_HEAD_THREADS>(red, t, acc[k]);
    if (t == 0) a.ws[PPO_HEADER + (int64_t)blockIdx.x * PPO_SUMS + k] = s;
  }
  if (blockIdx.x == 0 && t == 0) {
    a.ws[2] = (double)a.n;
    if constexpr (!AM) a.ws[3] = 0.0;
  }
}

struct PpoStepArgs {
  float* blob; float* grad; float* exp_avg; float* exp_avg_sq;
  int32_t* step;
  const float* hyper;
  const double* head_ws;
  float* stats;
  int64_t nf, logstd;
  int32_t head_blocks;
};

// What every optimiser step does ahead of its own arithmetic (f16_ppo_adam_kernel, f16_ppo_dag_kernel
// of f16_ppo_am.h), by every thread of the one block: with a head workspace the head's partials in
// block order, d_log_std into grad (and dls) and stats[0..5]; always the gradient's norm and the
// clip factor, stats[6..7]. Returns the clip factor; ends on a barrier.
__device__ __forceinline__ double ppo_step_prologue(double* red, double* sums, float* dls, const int t, const float* blob,
                                                    float* grad, const float* hyper, const double* head_ws,
                                                    const int32_t head_blocks, float* stats, const int64_t nf,
                                                    const int64_t logstd) {
  const float ent_coef = hyper[2], vf_coef = hyper[3], max_norm = hyper[4];
  const bool head = head_ws != nullptr;
  if (head) {
    if (t < PPO_SUMS) {
      double s = 0.0;
      for (int b = 0; b < head_blocks; ++b) s += head_ws[PPO_HEADER + (int64_t)b * PPO_SUMS + t];
      sums[t] = s;
    }
    __syncthreads();
    if (t < 4) {
      dls[t] = (float)(sums[t] - (double)ent_coef);
      grad[logstd + t] = dls[t];
    }
    __syncthreads();
  }
  double q = 0.0;
  for (int64_t i = t; i < nf; i += PPO_WIDE) {
    // (the four slots just written are read from LDS, not back from memory)
    const float g = (head && i >= logstd && i < logstd + 4) ? dls[i - logstd] : grad[i];
    q += (double)g * (double)g;
  }
  const double total_norm = sqrt(ppo_block_sum<PPO_WIDE>(red, t, q));
  const double coef = fmin(1.0, (double)max_norm / (total_norm + 1e-6));
  if (t == 0 && stats) {
    if (head) {
      const double n = head_ws[2];
      double ent = 0.0;
      for (int j = 0; j < 4; ++j) ent += 0.5 + 0.918938533204672742 + (double)blob[logstd + j];
      const double pl = sums[4] / n, vl = sums[5] / n;
      stats[0] = (float)pl;
      stats[1] = (float)vl;
      stats[2] = (float)-ent;
      stats[3] = (float)(pl + (double)ent_coef * -ent + (double)vf_coef * vl);
      stats[4] = (float)(sums[6] / n);
      stats[5] = (float)(sums[7] / n);
    }
    stats[6] = (float)total_norm;
    stats[7] = (float)coef;
  }
  __syncthreads();  // (the statistics read log_std ahead of its update)
  return coef;
}

__global__ __launch_bounds__(PPO_WIDE) void f16_ppo_adam_kernel(const PpoStepArgs a) {
  __shared__ double red[PPO_WIDE];
  __shared__ double sums[PPO_SUMS];
  __shared__ float dls[4];
  const int t = (int)threadIdx.x;
  const int32_t step_next = *a.step + 1;  // (stored back by thread 0 after the block's barriers)
  const float lr = a.hyper[0];
  const float beta1 = a.hyper[5], beta2 = a.hyper[6], eps = a.hyper[7];
  const bool head = a.head_ws != nullptr;
  const double coef = ppo_step_prologue(red, sums, dls, t, a.blob, a.grad, a.hyper, a.head_ws, a.head_blocks, a.stats,
                                        a.nf, a.logstd);
  auto g_at = [&](const int64_t i) -> float {
    return (head && i >= a.logstd && i < a.logstd + 4) ? dls[i - a.logstd] : a.grad[i];
  };
  // torch.optim.Adam's single-tensor step on float32 state, each element's arithmetic in fp64 and
  // rounded once per stored value: a clip factor rounded to float32 would put one common relative
  // error on every element of a step, twice over in the second moment
  const double bc1 = 1.0 - pow((double)beta1, (double)step_next);
  const double bc2_sqrt = sqrt(1.0 - pow((double)beta2, (double)step_next));
  const double step_size = (double)lr / bc1;
  const double w1 = 1.0 - (double)beta1, w2 = 1.0 - (double)beta2;
  for (int64_t i = t; i < a.nf; i += PPO_WIDE) {
    const double g = (double)g_at(i) * coef;
    const double m0 = (double)a.exp_avg[i];
    const double m = m0 + w1 * (g - m0);
    const double v = (double)a.exp_avg_sq[i] * (double)beta2 + w2 * g * g;
    a.exp_avg[i] = (float)m;
    a.exp_avg_sq[i] = (float)v;
    a.blob[i] = (float)((double)a.blob[i] - step_size * (m / (sqrt(v) / bc2_sqrt + (double)eps)));
  }
  if (t == 0) *a.step = step_next;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int ppo_head_grid(int64_t n, int32_t max_blocks, int64_t* grid) {
  if (n < 0) return set_err(-1, "n must be >= 0");
  if (max_blocks < 0) return set_err(-1, "max_blocks must be >= 0 (0: the default)");
  const int64_t want = n / PPO_HEAD_THREADS + (n % PPO_HEAD_THREADS != 0), lim = max_blocks ? max_blocks : PPO_HEAD_BLOCKS;
  *grid = want < lim ? want : lim;
  return 0;
}

static int ppo_workspace_impl(int64_t n, int32_t max_blocks, int64_t* bytes_out) {
  int64_t grid = 0;
  if (int rc = ppo_head_grid(n, max_blocks, &grid)) return rc;
  if (!bytes_out) return set_err(-1, "null argument");
  *bytes_out = grid ? (int64_t)sizeof(double) * (PPO_HEADER + PPO_SUMS * grid) : 0;
  return 0;
}

static int ppo_head_blocks_impl(int64_t n, int32_t max_blocks, int32_t* blocks_out) {
  int64_t grid = 0;
  if (int rc = ppo_head_grid(n, max_blocks, &grid)) return rc;
  if (!blocks_out) return set_err(-1, "null argument");
  *blocks_out = (int32_t)grid;
  return 0;
}

static int ppo_loss_head_impl(void* stream, int64_t n, const float* mean, const float* values, const float* actions,
                              const float* old_log_prob, const float* advantages, const float* target_values,
                              const float* log_std, const float* hyper, uint32_t flags, int32_t max_blocks,
                              void* workspace, int64_t workspace_bytes, float* d_mean, float* d_values) {
  int64_t grid = 0;
  if (int rc = ppo_head_grid(n, max_blocks, &grid)) return rc;
  if (flags & ~(uint32_t)F16_PPO_NORMALIZE_ADV) return set_err(-1, "unknown f16env_ppo_loss_head flags");
  if (n == 0) return 0;
  if (!mean || !values || !actions || !old_log_prob || !advantages || !target_values || !log_std || !hyper ||
      !workspace || !d_mean || !d_values)
    return set_err(-1, "null argument");
  if (((uintptr_t)mean & 15) != 0 || ((uintptr_t)actions & 15) != 0 || ((uintptr_t)d_mean & 15) != 0)
    return set_err(-1, "mean, actions and d_mean must be 16-byte aligned");
  if (((uintptr_t)workspace & 7) != 0) return set_err(-1, "the workspace must be 8-byte aligned");
  if ((((uintptr_t)values | (uintptr_t)old_log_prob | (uintptr_t)advantages | (uintptr_t)target_values |
        (uintptr_t)log_std | (uintptr_t)hyper | (uintptr_t)d_values) & 3) != 0)
    return set_err(-1, "values, old_log_prob, advantages, target_values, log_std, hyper and d_values must be float-aligned");
  if (workspace_bytes < (int64_t)sizeof(double) * (PPO_HEADER + PPO_SUMS * grid))
    return set_err(-1, "the workspace is smaller than f16env_ppo_workspace says");
  PpoHeadArgs a{};
  a.mean = mean; a.values = values; a.actions = actions; a.old_log_prob = old_log_prob;
  a.advantages = advantages; a.target_values = target_values; a.log_std = log_std; a.hyper = hyper;
  a.d_mean = d_mean; a.d_values = d_values; a.ws = static_cast<double*>(workspace); a.n = n;
  a.normalize = ((flags & F16_PPO_NORMALIZE_ADV) && n > 1) ? 1 : 0;
  if (a.normalize)
    hipLaunchKernelGGL(f16_ppo_adv_stats_kernel, dim3(1), dim3(PPO_WIDE), 0, (hipStream_t)stream, advantages, n, a.ws);
  hipLaunchKernelGGL(f16_ppo_head_kernel<false>, dim3((unsigned)grid), dim3(PPO_HEAD_THREADS), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

static int ppo_adam_step_impl(void* stream, int64_t n_floats, float* blob, float* grad_blob, float* exp_avg,
                              float* exp_avg_sq, int32_t* step, const float* hyper, int64_t log_std_offset,
                              const void* head_workspace, int32_t head_blocks, float* stats) {
  if (n_floats < 0) return set_err(-1, "n_floats must be >= 0");
  if (n_floats == 0) return 0;
  if (!blob || !grad_blob || !exp_avg || !exp_avg_sq || !step || !hyper) return set_err(-1, "null argument");
  if ((((uintptr_t)blob | (uintptr_t)grad_blob | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)step |
        (uintptr_t)hyper | (uintptr_t)stats) & 3) != 0)
    return set_err(-1, "blob, grad_blob, exp_avg, exp_avg_sq, step, hyper and stats must be 4-byte aligned");
  if (head_workspace) {
    if (((uintptr_t)head_workspace & 7) != 0) return set_err(-1, "the head's workspace must be 8-byte aligned");
    if (head_blocks < 1) return set_err(-1, "head_blocks must be >= 1 with a head workspace (f16env_ppo_head_blocks)");
    if (log_std_offset < 0 || log_std_offset > n_floats - 4)
      return set_err(-1, "log_std_offset must lie in [0, n_floats - 4]");
  }
  PpoStepArgs a{};
  a.blob = blob; a.grad = grad_blob; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq;
  a.step = step; a.hyper = hyper; a.head_ws = static_cast<const double*>(head_workspace); a.stats = stats;
  a.nf = n_floats; a.logstd = head_workspace ? log_std_offset : 0; a.head_blocks = head_workspace ? head_blocks : 0;
  hipLaunchKernelGGL(f16_ppo_adam_kernel, dim3(1), dim3(PPO_WIDE), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace f16
