// f16_ppo_am.h -- AM-PPO on the device (gfx950): the DynAGO controller over a finished rollout's
// advantages (f16env_ppo_dynago_update), the loss head on modulated advantages
// (f16env_ppo_loss_head_am) and the DAG / AlphaGrad step on the blob (f16env_ppo_dag_step);
// include/f16env.h, still ABI 7. Needs f16_ppo.h (the head kernel, ppo_step_prologue), whose rules hold here:
// every sum in fp64 and in a fixed order, float32 results rounded once, no atomics, no inline
// assembly, partial sums combined in the next launch's prologue.
//
// The reference: stable_baselines3/ppo/ppo.py:29-99 (dynago_transform_advantages), :289-306 (once
// per train()), :327-352, :368-372 (per minibatch) and ppo/optim/sgd.py:219-344 (DAG.step),
// :437-498 (AlphaGrad.step).
//
//   controller, launch 1 (moments): blocks of 256 threads read the array as float4; thread g of the
//     grid takes vectors g, g + G, g + 2 G, ... (G = 256 grid) in that order, four strides to a batch of
//     loads; the vector past the last whole one is the 1 .. 3 tail elements. Each thread keeps fp64
//     sums of x and x^2; the block's 256 meet in a halving tree; two doubles per block go to the
//     workspace.
//   controller, launch 2 (saturation): every block first adds the blocks' moments (thread t adds
//     partials t, t + 256, ... in order, then the tree) and forms alpha' -- the same instructions
//     on the same numbers in every block --, then counts |alpha' A / (N + eps)| > tau over its
//     vectors; one count per block goes to the workspace. The state is not written here: another
//     block may still be reading it.
//   controller, launch 3: one block repeats the moments' sum, adds the counts the same way and
//     writes state[0], state[1].
//   AM head: f16_ppo_am_stats_kernel (one block of 1024, as f16_ppo_adv_stats_kernel) forms the
//     minibatch's norm and mean, then mean and unbiased std of the modulated advantages, and
//     f16_ppo_head_kernel<true> takes the rows.
//   DAG step: ONE block of 1024 threads, f16_ppo_adam_kernel's prologue, then per parameter tensor
//     (segment) the clipped gradient's norm, the tensor's alpha, the tanh update in place; the
//     per-tensor sums are taken by the 16 waves (lane l adds lanes l + 32, 16, ..., 1 by
//     __shfl_down, fixed) and the 16 wave sums are added in wave order.
#pragma once
#include "f16_ppo.h"

namespace f16 {

constexpr int DYN_THREADS = 256;
constexpr int DYN_BLOCKS = 2048;  // default limit of the controller's grid: 8 blocks of 256 per CU
constexpr int DAG_MAX_SEGMENTS = 17;
constexpr int DAG_WAVES = PPO_WIDE / 64;

// ------------------------------------------------------------------------------------------
// the controller
// ------------------------------------------------------------------------------------------
// f(x) over the array in the order stated above; nv = ceil(n / 4) vectors, the last maybe partial
template <typename F>
__device__ __forceinline__ void dyn_sweep(const float* __restrict__ adv, const int64_t n, F&& f) {
  const int64_t full = n / 4, nv = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * DYN_THREADS;
  const float4* __restrict__ v4 = reinterpret_cast<const float4*>(adv);
  int64_t v = (int64_t)blockIdx.x * DYN_THREADS + threadIdx.x;
  for (; v + 3 * stride < full; v += 4 * stride) {
    const float4 a = v4[v], b = v4[v + stride], c = v4[v + 2 * stride], d = v4[v + 3 * stride];
    f(a.x); f(a.y); f(a.z); f(a.w);
    f(b.x); f(b.y); f(b.z); f(b.w);
    f(c.x); f(c.y); f(c.z); f(c.w);
    f(d.x); f(d.y); f(d.z); f(d.w);
  }
  for (; v < nv; v += stride) {
    if (v < full) {
      const float4 a = v4[v];
      f(a.x); f(a.y); f(a.z); f(a.w);
    } else {
      for (int64_t i = 4 * v; i < n; ++i) f(adv[i]);
    }
  }
}

struct DynMoments {
  double norm, alpha;  // N; alpha' as stored (the float32 value)
};

// the blocks' moments in a fixed order, then ppo.py:54-81; every thread of a 256-thread block calls it
__device__ __forceinline__ DynMoments dyn_alpha(double* red, const int t, const double* __restrict__ ws, const int grid,
                                                const int64_t n, const float* __restrict__ dynago,
                                                const float* __restrict__ state) {
  double s = 0.0, q = 0.0;
  for (int b = t; b < grid; b += DYN_THREADS) {
    s += ws[2 * b];
    q += ws[2 * b + 1];
  }
  s = ppo_block_sum<DYN_THREADS>(red, t, s);
  q = ppo_block_sum<DYN_THREADS>(red, t, q);
  const double eps = (double)dynago[F16_PPO_DYNAGO_EPS];
  const double var = fmax(q - s * s / (double)n, 0.0) / (double)(n - 1);
  const double norm = sqrt(q), sigma = sqrt(var) + eps;
  const double a_hat = (double)dynago[F16_PPO_DYNAGO_KAPPA_CONTROLLER] * (norm + eps) / (sigma + eps) *
                       pow((double)dynago[F16_PPO_DYNAGO_P_STAR] / ((double)state[1] + eps),
                           (double)dynago[F16_PPO_DYNAGO_ETA]);
  const double rho = (double)dynago[F16_PPO_DYNAGO_RHO];
  const double a_new = fmin(fmax((1.0 - rho) * (double)state[0] + rho * a_hat, (double)dynago[F16_PPO_DYNAGO_ALPHA_MIN]),
                            (double)dynago[F16_PPO_DYNAGO_ALPHA_MAX]);
  DynMoments m;
  m.norm = norm;
  m.alpha = (double)(float)a_new;
  return m;
}

__global__ __launch_bounds__(DYN_THREADS) void f16_dynago_moments_kernel(const float* __restrict__ adv, const int64_t n,
                                                                         double* __restrict__ ws) {
  __shared__ double red[DYN_THREADS];
  const int t = (int)threadIdx.x;
  double s = 0.0, q = 0.0;
  dyn_sweep(adv, n, [&](const float x) {
    const double d = (double)x;
    s += d;
    q += d * d;
  });
  s = ppo_block_sum<DYN_THREADS>(red, t, s);
  q = ppo_block_sum<DYN_THREADS>(red, t, q);
  if (t == 0) {
    ws[2 * (int64_t)blockIdx.x] = s;
    ws[2 * (int64_t)blockIdx.x + 1] = q;
  }
}

__global__ __launch_bounds__(DYN_THREADS) void f16_dynago_saturation_kernel(const float* __restrict__ adv, const int64_t n,
                                                                            const float* __restrict__ dynago,
                                                                            const float* __restrict__ state,
                                                                            double* __restrict__ ws) {
  __shared__ double red[DYN_THREADS];
  const int t = (int)threadIdx.x;
  const int grid = (int)gridDim.x;
  const DynMoments m = dyn_alpha(red, t, ws, grid, n, dynago, state);
  // (one division per thread, not per element: |Z| = |A| (alpha' / (N + eps)), an fp64 rounding from the quotient)
  const double scale = m.alpha / (m.norm + (double)dynago[F16_PPO_DYNAGO_EPS]), tau = (double)dynago[F16_PPO_DYNAGO_TAU];
  int64_t count = 0;
  dyn_sweep(adv, n, [&](const float x) { count += fabs((double)x) * scale > tau ? 1 : 0; });
  const double c = ppo_block_sum<DYN_THREADS>(red, t, (double)count);  // (whole numbers below 2^53: exact)
  if (t == 0) ws[2 * (int64_t)grid + blockIdx.x] = c;
}

__global__ __launch_bounds__(DYN_THREADS) void f16_dynago_state_kernel(const int64_t n, const int grid,
                                                                       const float* __restrict__ dynago,
                                                                       float* __restrict__ state,
                                                                       const double* __restrict__ ws) {
  __shared__ double red[DYN_THREADS];
  const int t = (int)threadIdx.x;
  const DynMoments m = dyn_alpha(red, t, ws, grid, n, dynago, state);
  double c = 0.0;
  for (int b = t; b < grid; b += DYN_THREADS) c += ws[2 * (int64_t)grid + b];
  c = ppo_block_sum<DYN_THREADS>(red, t, c);
  if (t == 0) {  // (dyn_alpha's reads of the state lie before ppo_block_sum's barriers)
    const double rho_sat = (double)dynago[F16_PPO_DYNAGO_RHO_SAT];
    state[1] = (float)((1.0 - rho_sat) * (double)state[1] + rho_sat * (c / (double)n));
    state[0] = (float)m.alpha;
  }
}

// ------------------------------------------------------------------------------------------
// the AM head's statistics
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PPO_WIDE) void f16_ppo_am_stats_kernel(const float* __restrict__ adv, const int64_t n,
                                                                    const float* __restrict__ dynago,
                                                                    const float* __restrict__ state, double* __restrict__ ws,
                                                                    float* __restrict__ am_stats) {
  __shared__ double red[PPO_WIDE];
  const int t = (int)threadIdx.x;
  double s = 0.0, q = 0.0;
  for (int64_t i = t; i < n; i += PPO_WIDE) {
    const double a = (double)adv[i];
    s += a;
    q += a * a;
  }
  const double mean_a = ppo_block_sum<PPO_WIDE>(red, t, s) / (double)n;
  const double norm = sqrt(ppo_block_sum<PPO_WIDE>(red, t, q));
  const PpoAmCoef c = ppo_am_coef(dynago, state, norm, n);
  double sm = 0.0;
  for (int64_t i = t; i < n; i += PPO_WIDE) sm += ppo_am_mod(adv[i], c);
  const double mean = ppo_block_sum<PPO_WIDE>(red, t, sm) / (double)n;
  double qm = 0.0;
  for (int64_t i = t; i < n; i += PPO_WIDE) {
    const double d = ppo_am_mod(adv[i], c) - mean;
    qm += d * d;
  }
  const double ss = ppo_block_sum<PPO_WIDE>(red, t, qm);
  if (t == 0) {
    ws[0] = mean;
    ws[1] = n > 1 ? sqrt(ss / (double)(n - 1)) : 0.0;
    ws[3] = norm;
    if (am_stats) {
      am_stats[0] = (float)mean_a;
      am_stats[1] = (float)mean;
      am_stats[2] = (float)norm;
      am_stats[3] = state[0];
    }
  }
}

// ------------------------------------------------------------------------------------------
// the DAG / AlphaGrad step
// ------------------------------------------------------------------------------------------
struct DagSegment {
  int32_t offset, length, count;  // floats into the blob, padded length, true elements d_s
};

struct DagStepArgs {
  float* blob; float* grad;
  const float* hyper; const float* dag;
  float* seg_state;       // (alpha_s, sat_s) per segment
  double* dag_state;      // s_t, rms_t_ema, rms0_ema, 0
  int32_t* dag_counters;  // global_step, rms_t_ema set, rms0_ema set, 0
  const double* head_ws;
  float* stats;
  int64_t nf, logstd;
  int32_t head_blocks, n_segments, fixed_alpha;
  DagSegment seg[DAG_MAX_SEGMENTS];
};

// the wave's sum in lane 0: lane l adds lane l + 32, then l + 16, ..., l + 1
__device__ __forceinline__ double dag_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(PPO_WIDE) void f16_ppo_dag_kernel(const DagStepArgs a) {
  __shared__ double red[PPO_WIDE];
  __shared__ double sums[PPO_SUMS];
  __shared__ float dls[4];
  __shared__ double part_q[DAG_MAX_SEGMENTS][DAG_WAVES], part_c[DAG_MAX_SEGMENTS][DAG_WAVES], part_u[DAG_WAVES];
  __shared__ double seg_norm[DAG_MAX_SEGMENTS], seg_horiz[DAG_MAX_SEGMENTS];
  const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
  const bool head = a.head_ws != nullptr, fixed = a.fixed_alpha != 0;
  const double lr = (double)a.hyper[0];
  const double eps = (double)a.dag[F16_PPO_DAG_EPS], tau = (double)a.dag[F16_PPO_DAG_TAU];
  // (the state is read ahead of the block's barriers and stored back by single threads after them)
  const double s_t = fixed ? 1.0 : a.dag_state[0], k_val = fixed ? 1.0 : (double)a.dag[F16_PPO_DAG_K_VAL];
  const int32_t global_step = a.dag_counters[0];
  const double coef = ppo_step_prologue(red, sums, dls, t, a.blob, a.grad, a.hyper, a.head_ws, a.head_blocks, a.stats,
                                        a.nf, a.logstd);
  auto g_at = [&](const int64_t i) -> double {
    return (double)((head && i >= a.logstd && i < a.logstd + 4) ? dls[i - a.logstd] : a.grad[i]) * coef;
  };
  // 1. ||coef g_s|| per segment
  for (int s = 0; s < a.n_segments; ++s) {
    const int64_t lo = a.seg[s].offset, hi = lo + a.seg[s].length;
    double q = 0.0;
    for (int64_t i = lo + t; i < hi; i += PPO_WIDE) {
      const double g = g_at(i);
      q += g * g;
    }
    q = dag_wave_sum(q);
    if (lane == 0) part_q[s][wave] = q;
  }
  __syncthreads();
  // 2. the segment's alpha (sgd.py:253-274), one thread each
  if (t < a.n_segments) {
    double q = 0.0, d_total = 0.0;
    for (int w = 0; w < DAG_WAVES; ++w) q += part_q[t][w];
    for (int s = 0; s < a.n_segments; ++s) d_total += (double)a.seg[s].count;
    const double norm = sqrt(q);
    double alpha;
    if (fixed) {
      alpha = (double)a.dag[F16_PPO_DAG_ALPHA];
    } else {
      const double d = (double)a.seg[t].count, sigma = norm / sqrt(d);
      const double a_hat = (double)a.dag[F16_PPO_DAG_KAPPA] * (norm + eps) / (sigma + eps) *
                           pow(d / d_total, (double)a.dag[F16_PPO_DAG_BETA]) *
                           pow((double)a.dag[F16_PPO_DAG_P_STAR] / ((double)a.seg_state[2 * t + 1] + eps),
                               (double)a.dag[F16_PPO_DAG_ETA]) * s_t;
      const double rho = (double)a.dag[F16_PPO_DAG_RHO];
      const float stored = (float)fmin(fmax((1.0 - rho) * (double)a.seg_state[2 * t] + rho * a_hat,
                                            (double)a.dag[F16_PPO_DAG_ALPHA_MIN]), (double)a.dag[F16_PPO_DAG_ALPHA_MAX]);
      a.seg_state[2 * t] = stored;
      alpha = (double)stored;
    }
    seg_norm[t] = norm;
    seg_horiz[t] = alpha / s_t;
  }
  __syncthreads();
  // 3. the update (sgd.py:277-320): x = (alpha / s_t) coef g / (||.|| + eps), u = k s_t tanh(x)
  double usq = 0.0;
  for (int s = 0; s < a.n_segments; ++s) {
    const int64_t lo = a.seg[s].offset, hi = lo + a.seg[s].length;
    const double horiz = seg_horiz[s], den = seg_norm[s] + eps;
    double count = 0.0;
    for (int64_t i = lo + t; i < hi; i += PPO_WIDE) {
      const double x = horiz * g_at(i) / den;
      const double u = k_val * s_t * tanh(x);
      a.blob[i] = (float)((double)a.blob[i] - lr * u);
      usq += u * u;
      count += fabs(x) > tau ? 1.0 : 0.0;
    }
    count = dag_wave_sum(count);
    if (lane == 0) part_c[s][wave] = count;
  }
  usq = dag_wave_sum(usq);
  if (lane == 0) part_u[wave] = usq;
  __syncthreads();
  if (fixed) return;
  // 4. the saturation of a sampled step (sgd.py:292-295) and the global RMS shrink (:326-343)
  const int32_t sat_every = max(1, (int32_t)a.dag[F16_PPO_DAG_SAT_EVERY]);
  if (t < a.n_segments && global_step % sat_every == 0) {
    double c = 0.0;
    for (int w = 0; w < DAG_WAVES; ++w) c += part_c[t][w];
    a.seg_state[2 * t + 1] = (float)(c / (double)a.seg[t].count);
  }
  if (t == 0) {
    double u = 0.0, d_total = 0.0;
    for (int w = 0; w < DAG_WAVES; ++w) u += part_u[w];
    for (int s = 0; s < a.n_segments; ++s) d_total += (double)a.seg[s].count;
    const double rms_now = sqrt(u / d_total), beta = (double)a.dag[F16_PPO_DAG_EMA_BETA];
    const double rms_t = a.dag_counters[1] ? beta * a.dag_state[1] + (1.0 - beta) * rms_now : rms_now;
    a.dag_state[1] = rms_t;
    a.dag_counters[1] = 1;
    if (global_step < (int32_t)a.dag[F16_PPO_DAG_WARMUP_STEPS]) {
      a.dag_state[2] = a.dag_counters[2] ? beta * a.dag_state[2] + (1.0 - beta) * rms_t : rms_t;
      a.dag_counters[2] = 1;
    } else {
      if (!a.dag_counters[2]) {
        a.dag_state[2] = rms_t;
        a.dag_counters[2] = 1;
      }
      // (0 / 0 after gradients of zeros: fmin and fmax pass the number, the ratio is 1)
      const double ratio = fmax(0.0, fmin(1.0, rms_t / ((double)a.dag[F16_PPO_DAG_LAMBDA_RMS] * a.dag_state[2])));
      const double s_min = (double)a.dag[F16_PPO_DAG_S_MIN];
      a.dag_state[0] = s_min + (1.0 - s_min) * pow(ratio, (double)a.dag[F16_PPO_DAG_GAMMA]);
    }
    a.dag_counters[0] = global_step + 1;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int dyn_grid(int64_t n, int32_t max_blocks, int64_t* grid) {
  if (n < 0) return set_err(-1, "n must be >= 0");
  if (max_blocks < 0) return set_err(-1, "max_blocks must be >= 0 (0: the default)");
  const int64_t nv = n / 4 + (n % 4 != 0);
  const int64_t want = nv / DYN_THREADS + (nv % DYN_THREADS != 0), lim = max_blocks ? max_blocks : DYN_BLOCKS;
  *grid = n <= 1 ? 0 : (want < lim ? want : lim);
  return 0;
}

static int ppo_dynago_workspace_impl(int64_t n, int32_t max_blocks, int64_t* bytes_out) {
  int64_t grid = 0;
  if (int rc = dyn_grid(n, max_blocks, &grid)) return rc;
  if (!bytes_out) return set_err(-1, "null argument");
  *bytes_out = grid ? (int64_t)sizeof(double) * 3 * grid : 0;
  return 0;
}

static int ppo_dynago_update_impl(void* stream, int64_t n, const float* advantages, const float* dynago, float* state,
                                  int32_t max_blocks, void* workspace, int64_t workspace_bytes) {
  int64_t grid = 0;
  if (int rc = dyn_grid(n, max_blocks, &grid)) return rc;
  if (n <= 1) return 0;  // (ppo.py:40-41 returns before any update)
  if (!advantages || !dynago || !state || !workspace) return set_err(-1, "null argument");
  if (((uintptr_t)advantages & 15) != 0) return set_err(-1, "advantages must be 16-byte aligned");
  if (((uintptr_t)workspace & 7) != 0) return set_err(-1, "the workspace must be 8-byte aligned");
  if ((((uintptr_t)dynago | (uintptr_t)state) & 3) != 0) return set_err(-1, "dynago and state must be float-aligned");
  if (workspace_bytes < (int64_t)sizeof(double) * 3 * grid)
    return set_err(-1, "the workspace is smaller than f16env_ppo_dynago_workspace says");
  double* ws = static_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(f16_dynago_moments_kernel, dim3((unsigned)grid), dim3(DYN_THREADS), 0, s, advantages, n, ws);
  hipLaunchKernelGGL(f16_dynago_saturation_kernel, dim3((unsigned)grid), dim3(DYN_THREADS), 0, s, advantages, n, dynago,
                     (const float*)state, ws);
  hipLaunchKernelGGL(f16_dynago_state_kernel, dim3(1), dim3(DYN_THREADS), 0, s, n, (int)grid, dynago, state,
                     (const double*)ws);
  HIPCHK(hipGetLastError());
  return 0;
}

static int ppo_loss_head_am_impl(void* stream, int64_t n, const float* mean, const float* values, const float* actions,
                                 const float* old_log_prob, const float* advantages, const float* old_values,
                                 const float* log_std, const float* hyper, const float* dynago, const float* state,
                                 uint32_t flags, int32_t max_blocks, void* workspace, int64_t workspace_bytes,
                                 float* d_mean, float* d_values, float* am_stats) {
  int64_t grid = 0;
  if (int rc = ppo_head_grid(n, max_blocks, &grid)) return rc;
  if (flags & ~(uint32_t)F16_PPO_AM_NORMALIZE) return set_err(-1, "unknown f16env_ppo_loss_head_am flags");
  if (n == 0) return 0;
  if (!mean || !values || !actions || !old_log_prob || !advantages || !old_values || !log_std || !hyper || !dynago ||
      !state || !workspace || !d_mean || !d_values)
    return set_err(-1, "null argument");
  if (((uintptr_t)mean & 15) != 0 || ((uintptr_t)actions & 15) != 0 || ((uintptr_t)d_mean & 15) != 0)
    return set_err(-1, "mean, actions and d_mean must be 16-byte aligned");
  if (((uintptr_t)workspace & 7) != 0) return set_err(-1, "the workspace must be 8-byte aligned");
  if ((((uintptr_t)values | (uintptr_t)old_log_prob | (uintptr_t)advantages | (uintptr_t)old_values |
        (uintptr_t)log_std | (uintptr_t)hyper | (uintptr_t)dynago | (uintptr_t)state | (uintptr_t)d_values |
        (uintptr_t)am_stats) & 3) != 0)
    return set_err(-1, "values, old_log_prob, advantages, old_values, log_std, hyper, dynago, state, d_values and "
                       "am_stats must be float-aligned");
  if (workspace_bytes < (int64_t)sizeof(double) * (PPO_HEADER + PPO_SUMS * grid))
    return set_err(-1, "the workspace is smaller than f16env_ppo_workspace says");
  PpoHeadArgs a{};
  a.mean = mean; a.values = values; a.actions = actions; a.old_log_prob = old_log_prob;
  a.advantages = advantages; a.target_values = old_values; a.log_std = log_std; a.hyper = hyper;
  a.d_mean = d_mean; a.d_values = d_values; a.ws = static_cast<double*>(workspace); a.n = n;
  a.normalize = ((flags & F16_PPO_AM_NORMALIZE) && n > 1) ? 1 : 0;
  a.dynago = dynago; a.am_state = state;
  hipLaunchKernelGGL(f16_ppo_am_stats_kernel, dim3(1), dim3(PPO_WIDE), 0, (hipStream_t)stream, advantages, n, dynago,
                     state, a.ws, am_stats);
  hipLaunchKernelGGL(f16_ppo_head_kernel<true>, dim3((unsigned)grid), dim3(PPO_HEAD_THREADS), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

static int ppo_dag_step_impl(void* stream, int64_t n_floats, float* blob, float* grad_blob, const float* hyper,
                             const float* dag, const int32_t* segments, int32_t n_segments, float* seg_state,
                             double* dag_state, int32_t* dag_counters, uint32_t flags, int64_t log_std_offset,
                             const void* head_workspace, int32_t head_blocks, float* stats) {
  if (n_floats < 0) return set_err(-1, "n_floats must be >= 0");
  if (flags & ~(uint32_t)F16_PPO_DAG_FIXED_ALPHA) return set_err(-1, "unknown f16env_ppo_dag_step flags");
  if (n_floats == 0) return 0;
  if (n_floats > INT32_MAX) return set_err(-1, "n_floats must fit the segment table's int32");
  if (!blob || !grad_blob || !hyper || !dag || !segments || !seg_state || !dag_state || !dag_counters)
    return set_err(-1, "null argument");
  if ((((uintptr_t)blob | (uintptr_t)grad_blob | (uintptr_t)hyper | (uintptr_t)dag | (uintptr_t)seg_state |
        (uintptr_t)dag_counters | (uintptr_t)stats) & 3) != 0)
    return set_err(-1, "blob, grad_blob, hyper, dag, seg_state, dag_counters and stats must be 4-byte aligned");
  if (((uintptr_t)dag_state & 7) != 0) return set_err(-1, "dag_state must be 8-byte aligned");
  if (n_segments < 1 || n_segments > DAG_MAX_SEGMENTS) return set_err(-1, "n_segments must be in 1 .. 17");
  DagStepArgs a{};
  int64_t end = 0;
  for (int s = 0; s < n_segments; ++s) {
    const int32_t off = segments[3 * s], len = segments[3 * s + 1], count = segments[3 * s + 2];
    if (off < end || len < 1 || (int64_t)off + len > n_floats || count < 1 || count > len)
      return set_err(-1, "bad segment table: segments ascend without overlap inside [0, n_floats) and hold "
                         "1 <= count <= length");
    end = (int64_t)off + len;
    a.seg[s] = DagSegment{off, len, count};
  }
  if (head_workspace) {
    if (((uintptr_t)head_workspace & 7) != 0) return set_err(-1, "the head's workspace must be 8-byte aligned");
    if (head_blocks < 1) return set_err(-1, "head_blocks must be >= 1 with a head workspace (f16env_ppo_head_blocks)");
    if (log_std_offset < 0 || log_std_offset > n_floats - 4)
      return set_err(-1, "log_std_offset must lie in [0, n_floats - 4]");
  }
  a.blob = blob; a.grad = grad_blob; a.hyper = hyper; a.dag = dag; a.seg_state = seg_state;
  a.dag_state = dag_state; a.dag_counters = dag_counters;
  a.head_ws = static_cast<const double*>(head_workspace); a.stats = stats;
  a.nf = n_floats; a.logstd = head_workspace ? log_std_offset : 0; a.head_blocks = head_workspace ? head_blocks : 0;
  a.n_segments = n_segments; a.fixed_alpha = (flags & F16_PPO_DAG_FIXED_ALPHA) ? 1 : 0;
  hipLaunchKernelGGL(f16_ppo_dag_kernel, dim3(1), dim3(PPO_WIDE), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace f16
