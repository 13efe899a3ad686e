// f16_reset.h -- the kernels that put state into lanes outside a step: the deferred reset behind
// a cfg5 step (ResetDoneArgs, f16_reset_done_kernel), the reset cache's fill (f16_ic_fill_kernel
// and the table that picks its instance), the caller's reset (ResetArgs, f16_reset_kernel), the
// window restart, the IC template (f16_ic_kernel), get / set state, clear-fresh and the trim
// solver. Device code and that table only: every launch takes the handle and is in f16env.hip.
// Needs f16_device.h, f16_env_layer.h and f16_stage.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/f16env.h"
#include "f16_device.h"
#include "f16_env_layer.h"
#include "f16_stage.h"

using namespace f16;

// cfg5 auto-reset of the lanes a deferred-mode step finished (done list from its ballot
// compaction): full RunIC (random IC box, gust start) and K x frame 0 into their obs rows.
struct ResetDoneArgs {
  SoA s, tmpl;
  const int32_t* done_idx;
  const int32_t* n_done;
  float* obs;       // frame r of env k at obs + k * obs_row + obs_off + r * obs_pitch, obs_slot
                    // floats written per frame (contiguous: K*15, 0, 15, 15; window:
                    // 16, (p-K+1)*N*16, N*16, 16)
  int64_t obs_row, obs_off, obs_pitch;
  int32_t obs_slot;
  int32_t* zero_next;  // the handle's other done counter (the next step's): zeroed here, so a
                       // step needs no memset of its counter
  EnvArgs E;
  ModelConsts C;
};
__global__ __launch_bounds__(BLOCK) void f16_reset_done_kernel(ResetDoneArgs a) {
  __shared__ __align__(16) float sT[F16_BLOB_FLOATS];
  if (a.zero_next && blockIdx.x == 0 && threadIdx.x == 0) *a.zero_next = 0;
  // one round trip before the work: the table DMA, the done count and this thread's first list
  // entry in flight together (the list holds N entries, so the speculative read is in bounds)
  stage_tables_issue(sT);
  const int64_t i0 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int nd = *a.n_done;
  const int32_t k0 = i0 < a.E.n ? a.done_idx[i0] : -1;
  VM_DRAIN();
  __syncthreads();
  if ((int64_t)blockIdx.x * BLOCK >= nd) return;  // after the only barrier
  for (int64_t i = i0; i < nd; i += (int64_t)gridDim.x * BLOCK) {
    const int64_t k = i == i0 ? k0 : a.done_idx[i];
    F16_CHECK(k >= 0 && k < a.E.n, DBG_RESET_INDEX);
    if (k < 0 || k >= a.E.n) continue;
    Lane L;
    lane_load<true>(a.s, k, L);
    float f0[F16_OBS_DIM];
    lane_reset(L, a.tmpl, nullptr, nullptr, a.E, k, sT, a.C, f0);
    lane_store<true>(a.s, k, L);
    float* o = a.obs + k * a.obs_row + a.obs_off;
    for (int r = 0; r < a.E.K; ++r)
      for (int j = 0; j < a.obs_slot; ++j) o[r * a.obs_pitch + j] = j < F16_OBS_DIM ? f0[j] : 0.0f;
  }
}

// cfg5 reset cache (windowed layout): a lane's next reset -- RunIC of its random IC, gust
// start, goal, frame 0 -- is a pure function of (seed, global env id, episode), so it is
// evaluated ahead, here, for every lane whose cached row is not the one of its next episode
// (tag: the row's episode count = the lane's + 1), and the windowed step copies it into a
// finished lane like MODE 0's template reset. Run every ICC_PERIOD windowed steps (and at the
// first): the lanes that reset since the last fill are refilled; a lane that finishes again
// before that runs its RunIC inside the step. Columns: NCOL_ALL state columns, then frame 0
// without the goal (TMPL_FRAME_COLS).
enum { ICC_COLS = NCOL_ALL + TMPL_FRAME_COLS };
template <int MODE>
__global__ __launch_bounds__(BLOCK) void f16_ic_fill_kernel(SoA s, SoA cache, EnvArgs E, ModelConsts C) {
  __shared__ __align__(16) float sT[F16_BLOB_FLOATS];
  stage_tables(sT);
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= E.n) return;
  const int32_t ep = __float_as_int(s.c[(int64_t)15 * s.n + k].w);
  if (__float_as_int(cache.c[(int64_t)15 * cache.n + k].w) == ep + 1) return;
  Lane L;
  L.ep_count = ep;
  L.flags = 0;
  float f0[F16_OBS_DIM];
  lane_reset_mode<MODE>(L, E, k, sT, C, f0);
  lane_store<true>(cache, k, L);
  for (int j = 0; j < TMPL_FRAME_COLS; ++j)
    cache.c[(int64_t)(NCOL_ALL + j) * cache.n + k] = make_float4(f0[4 * j], f0[4 * j + 1], f0[4 * j + 2], f0[4 * j + 3]);
}

using FillKernel = void (*)(SoA, SoA, EnvArgs, ModelConsts);
static FillKernel ic_fill_kernel_for(int mode) {
  static const FillKernel fills[4] = {f16_ic_fill_kernel<0>, f16_ic_fill_kernel<1>, f16_ic_fill_kernel<2>,
                                      f16_ic_fill_kernel<3>};
  return fills[mode & 3];
}

struct ResetArgs {
  SoA s, tmpl;
  const uint8_t* mask;
  const float* goals;
  const double* ic;
  float* obs;       // frame addressing as ResetDoneArgs
  int64_t obs_row, obs_off, obs_pitch;
  int32_t obs_slot;
  int* wind_any;    // per-lane IC given: set if a lane got wind (the handle needs the wind kernels)
  EnvArgs E;
  ModelConsts C;
};
__global__ __launch_bounds__(BLOCK) void f16_reset_kernel(ResetArgs a) {
  __shared__ __align__(16) float sT[F16_BLOB_FLOATS];
  stage_tables(sT);
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= a.E.n) return;
  if (a.mask && !a.mask[k]) return;
  Lane L;
  lane_load<true>(a.s, k, L);
  float f0[F16_OBS_DIM];
  // a goal row whose x is NaN draws the lane's goal from the device stream (mixed seeded /
  // unseeded resets in ONE call: the episode counter advances once per reset)
  const float* g = a.goals ? a.goals + 3 * k : nullptr;
  if (g && isnan(g[0])) g = nullptr;
  lane_reset(L, a.tmpl, a.ic ? a.ic + (int64_t)F16_IC_N * k : nullptr, g, a.E, k, sT, a.C, f0);
  lane_store<true>(a.s, k, L);
  if (a.wind_any && (L.wst[0] != 0.0f || L.wst[1] != 0.0f || L.wst[2] != 0.0f)) atomicOr(a.wind_any, 1);
  if (a.obs) {
    float* o = a.obs + k * a.obs_row + a.obs_off;
    for (int r = 0; r < a.E.K; ++r)
      for (int j = 0; j < a.obs_slot; ++j) o[r * a.obs_pitch + j] = j < F16_OBS_DIM ? f0[j] : 0.0f;
  }
}

// windowed observations: the histories' last K-1 frame positions (p_old-K+2 .. p_old) move to
// the front (0 .. K-2) of both histories, so the next step writes its frame at K-1. One lane
// per float4 of a slot; (wenv, wpos) as StepArgs (wrow, wenv).
__global__ void f16_window_restart_kernel(int64_t n, int32_t K, int64_t wenv, int64_t wpos, int32_t p_src, float* h0,
                                          float* h1) {
  const int64_t per = (int64_t)(K - 1) * n * 4;  // float4 per history
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * per) return;
  const int64_t b = i >= per, t = i - b * per;
  F16_CHECK(p_src >= 1, DBG_WINDOW_POS);
  float* h = b ? h1 : h0;
  if (wenv == 4 * 4 && wpos == n * 16) {  // position-major: the K-1 positions are one block
    float4* h4 = reinterpret_cast<float4*>(h);
    h4[t] = h4[(int64_t)p_src * n * 4 + t];
    return;
  }
  const int64_t q = t & 3, u = t >> 2;
  const int64_t k = u % n, r = u / n;
  float* d = h + k * wenv + r * wpos + 4 * q;
  *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(d + (int64_t)p_src * wpos);
}

// IC -> state (used once at create to build the reset template, n = 1)
__global__ void f16_ic_kernel(SoA dst, const double* ic, ModelConsts C) {
  __shared__ __align__(16) float sT[F16_BLOB_FLOATS];
  stage_tables(sT);
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Lane L;
  memset(&L, 0, sizeof L);
  apply_ic(L, ic, sT, C);
  L.ep_ret = 0.0; L.step = 0; L.ep_count = 0; L.last_d = 0.0f;
  L.goal[0] = L.goal[1] = L.goal[2] = 0.0f;
  lane_store<true>(dst, 0, L);  // with the config IC's wind columns (read by wind-kernel resets)
  // frame 0 of the template (goal excluded): what every template auto-reset would evaluate
  float f[F16_OBS_DIM];
  make_frame(L, 1.0, 0.0, alt_ref(L, 1.0, 0.0), f);
  for (int j = 0; j < TMPL_FRAME_COLS; ++j)
    dst.c[NCOL_ALL + j] = make_float4(f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3]);
}

__global__ void f16_get_state_kernel(SoA s, double* c, ModelConsts C) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= s.n) return;
  Lane L;
  lane_load<true>(s, k, L);
  double* o = c + (int64_t)F16C_N * k;
  for (int j = 0; j < 3; ++j) {
    o[F16C_RI + j] = L.rI[j]; o[F16C_VI + j] = L.vI[j];
    o[F16C_VIH1 + j] = L.vI[j] - (double)L.ndv1[j];  // vI + dv1
    o[F16C_VIH2 + j] = L.vI[j] + (double)L.dv2[j];
    o[F16C_AI + j] = L.aI[j]; o[F16C_AIP + j] = L.aIp[j]; o[F16C_WI + j] = L.wI[j];
    o[F16C_WID + j] = L.wId[j]; o[F16C_BA + j] = L.ba[j]; o[F16C_GOAL + j] = L.goal[j];
    o[F16C_WIND + j] = L.wst[j];
    o[F16C_GUST + j] = L.gust[j];
  }
  for (int j = 0; j < 4; ++j) { o[F16C_Q + j] = L.q[j]; o[F16C_CMD + j] = 0.0; }
  o[F16C_EPA_C] = cos(L.epa); o[F16C_EPA_S] = sin(L.epa);
  o[F16C_TEF] = L.tef; o[F16C_AIL] = L.ail; o[F16C_ELE] = L.ele; o[F16C_RUD] = L.rud;
  o[F16C_LEF] = L.lef; o[F16C_SB] = L.sb;
  o[F16C_PID_R_I] = L.pri; o[F16C_PID_R_P] = L.prp; o[F16C_PID_P_I] = L.ppi;
  o[F16C_PID_P_P] = L.ppp; o[F16C_PID_Y_I] = L.pyi; o[F16C_PID_Y_P] = L.pyp;
  o[F16C_N1] = L.n1; o[F16C_N2] = L.n2; o[F16C_AUG] = (L.flags & LANE_FLAG_AUG) ? 1.0 : 0.0;
  for (int j = 0; j < F16L_N; ++j) o[F16C_LX + j] = L.lx[j];
  o[F16C_LX + F16L_VC_KTS] = vcas_from_qc(L.lx[F16L_VC_KTS], C);  // the latch holds qc
  o[F16C_LAST_D] = L.last_d; o[F16C_STEP] = L.step; o[F16C_EP_RET] = L.ep_ret;
  o[F16C_EP_COUNT] = (double)(uint32_t)L.ep_count;
}

__global__ void f16_set_state_kernel(SoA s, const double* c, ModelConsts C, int* wind_any) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= s.n) return;
  Lane L;
  const double* o = c + (int64_t)F16C_N * k;
  for (int j = 0; j < 3; ++j) {
    L.rI[j] = o[F16C_RI + j]; L.vI[j] = o[F16C_VI + j];
    L.ndv1[j] = -(float)(o[F16C_VIH1 + j] - o[F16C_VI + j]);
    L.dv2[j] = (float)(o[F16C_VIH2 + j] - o[F16C_VI + j]);
    L.aI[j] = (float)o[F16C_AI + j]; L.aIp[j] = (float)o[F16C_AIP + j]; L.wI[j] = (float)o[F16C_WI + j];
    L.wId[j] = (float)o[F16C_WID + j]; L.ba[j] = (float)o[F16C_BA + j]; L.goal[j] = (float)o[F16C_GOAL + j];
    L.wst[j] = (float)o[F16C_WIND + j];
    L.gust[j] = (float)o[F16C_GUST + j];
    L.wind[j] = L.wst[j] + L.gust[j];
  }
  for (int j = 0; j < 4; ++j) L.q[j] = (float)o[F16C_Q + j];
  L.epa = atan2(o[F16C_EPA_S], o[F16C_EPA_C]);
  L.tef = (float)o[F16C_TEF]; L.ail = (float)o[F16C_AIL]; L.ele = (float)o[F16C_ELE];
  L.rud = (float)o[F16C_RUD]; L.lef = (float)o[F16C_LEF]; L.sb = (float)o[F16C_SB];
  L.pri = (float)o[F16C_PID_R_I]; L.prp = (float)o[F16C_PID_R_P]; L.ppi = (float)o[F16C_PID_P_I];
  L.ppp = (float)o[F16C_PID_P_P]; L.pyi = (float)o[F16C_PID_Y_I]; L.pyp = (float)o[F16C_PID_Y_P];
  L.n1 = (float)o[F16C_N1]; L.n2 = (float)o[F16C_N2];
  // FRESH (the lane's other window history still lacks its reset frames) describes the
  // handle's observation histories, not the physics state, so it survives a set_state: a
  // reset -> set_state -> step sequence still fills the new window from the reset frame
  // (f16env_window_clear_fresh drops it once the caller has written whole windows)
  const bool fresh = sign_flag(s.c[(int64_t)14 * s.n + k].x);
  L.flags = (o[F16C_AUG] != 0.0 ? LANE_FLAG_AUG : 0) | (fresh ? LANE_FLAG_FRESH : 0);
  for (int j = 0; j < F16L_N; ++j) L.lx[j] = (float)o[F16C_LX + j];
  L.lx[F16L_VC_KTS] = qc_from_vcas(o[F16C_LX + F16L_VC_KTS], C);
  L.last_d = (float)o[F16C_LAST_D]; L.step = (int32_t)o[F16C_STEP]; L.ep_ret = o[F16C_EP_RET];
  L.ep_count = (int32_t)(uint32_t)o[F16C_EP_COUNT];
  lane_store<true>(s, k, L);
  // a lane with wind needs the wind kernels (f16env_set_state switches the handle)
  bool w = false;
  for (int j = 0; j < 3; ++j) w = w || L.wst[j] != 0.0f || L.gust[j] != 0.0f;
  if (w) atomicOr(wind_any, 1);
}

// the caller wrote whole observation windows into both histories (F16Envs.set_obs): no lane
// needs its window filled from a reset frame any more (the FRESH sign bit of column 14's x)
__global__ void f16_clear_fresh_kernel(SoA s) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= s.n) return;
  float* y = &s.c[(int64_t)14 * s.n + k].x;
  *y = without_sign_flag(*y);
}

// Trim: Newton on (alpha, elevator cmd, throttle cmd), mirrors oracle trim_one()
__device__ void trim_residual(const double* icb, const float* x, const float* T, const ModelConsts& C,
                              float* res) {
  double ic[F16_IC_N];
  for (int j = 0; j < F16_IC_N; ++j) ic[j] = icb[j];
  const double vt = icb[F16_IC_U_FPS];
  ic[F16_IC_U_FPS] = vt * cos((double)x[0]);
  ic[F16_IC_V_FPS] = 0.0;
  ic[F16_IC_W_FPS] = vt * sin((double)x[0]);
  ic[F16_IC_THETA_RAD] = x[0];
  ic[F16_IC_PHI_RAD] = 0.0;
  ic[F16_IC_P_RPS] = ic[F16_IC_Q_RPS] = ic[F16_IC_R_RPS] = 0.0;
  ic[F16_IC_CMD_AIL] = 0.0; ic[F16_IC_CMD_RUD] = 0.0;
  ic[F16_IC_CMD_ELE] = x[1];
  ic[F16_IC_CMD_THR] = x[2];
  Lane L;
  L.gust[0] = L.gust[1] = L.gust[2] = 0.0f;
  apply_ic(L, ic, T, C);
  // FGAccelerations::CalculateUVWdot: specific force + gravity - (pqr + 2 w_b) x uvw
  // - Ti2b (w x (w x rI))
  Derived d;
  derive(L, 1.0, 0.0, alt_ref(L, 1.0, 0.0), d);
  float gb[3];
  mvec(d.Ti2b, d.gI, gb);
  const float we = (float)OMEGA_E;
  const float wb[3] = {d.Ti2b[2] * we, d.Ti2b[5] * we, d.Ti2b[8] * we};
  const float t[3] = {d.pqr[0] + 2.0f * wb[0], d.pqr[1] + 2.0f * wb[1], d.pqr[2] + 2.0f * wb[2]};
  float c1[3];
  crossf(t, d.uvw, c1);
  const double w2 = OMEGA_E * OMEGA_E;
  const float wxwxr[3] = {(float)(-w2 * L.rI[0]), (float)(-w2 * L.rI[1]), 0.0f};
  float cent[3];
  mvec(d.Ti2b, wxwxr, cent);
  res[0] = L.ba[0] + gb[0] - c1[0] - cent[0];
  res[1] = L.ba[2] + gb[2] - c1[2] - cent[2];
  res[2] = L.wId[1];
}
__device__ void inv3f(const float* M, float* I, bool& ok) {
  const float a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], k = M[8];
  const float A = e * k - f * h, B = -(d * k - f * g), Cc = d * h - e * g;
  const float det = a * A + b * B + c * Cc;
  ok = det != 0.0f;
  const float r = ok ? 1.0f / det : 0.0f;
  I[0] = A * r; I[1] = -(b * k - c * h) * r; I[2] = (b * f - c * e) * r;
  I[3] = B * r; I[4] = (a * k - c * g) * r; I[5] = -(a * f - c * d) * r;
  I[6] = Cc * r; I[7] = -(a * h - b * g) * r; I[8] = (a * e - b * d) * r;
}
__global__ __launch_bounds__(BLOCK) void f16_trim_kernel(int64_t n, const double* ic_in, double* ic_out,
                                                         double* resid, ModelConsts C) {
  __shared__ __align__(16) float sT[F16_BLOB_FLOATS];
  stage_tables(sT);
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= n) return;
  const double* icb = ic_in + (int64_t)F16_IC_N * k;
  // Newton on x = (alpha, elevator cmd, throttle cmd) as the oracle's trim_one, with what the
  // fp32 residual needs to converge to its own noise floor (~1e-4 ft/s^2): central differences
  // (the forward ones of the fp64 oracle carry an O(h) bias at the step size fp32 allows), up
  // to 24 iterations, and the iterate with the smallest residual kept (fp32 noise can make the
  // last step a slightly worse one)
  float x[3] = {0.05f, 0.0f, 0.5f};
  const float hs[3] = {2e-3f, 2e-3f, 2e-3f};
  float r[3], best[3] = {x[0], x[1], x[2]}, best_r = 3.4e38f;
  for (int it = 0;; ++it) {
    trim_residual(icb, x, sT, C, r);
    const float rmax = fmaxf(fabsf(r[0]), fmaxf(fabsf(r[1]), fabsf(r[2])));
    if (rmax < best_r) { best_r = rmax; best[0] = x[0]; best[1] = x[1]; best[2] = x[2]; }
    if (rmax < 2e-5f || it == 24) break;
    float Jm[9], Ji[9];
    for (int j = 0; j < 3; ++j) {
      float xp[3] = {x[0], x[1], x[2]}, xm[3] = {x[0], x[1], x[2]}, rp[3], rm[3];
      xp[j] += hs[j];
      xm[j] -= hs[j];
      trim_residual(icb, xp, sT, C, rp);
      trim_residual(icb, xm, sT, C, rm);
      for (int i = 0; i < 3; ++i) Jm[3 * i + j] = (rp[i] - rm[i]) / (2.0f * hs[j]);
    }
    bool ok;
    inv3f(Jm, Ji, ok);
    if (!ok) break;
    float dx[3];
    mvec(Ji, r, dx);
    for (int i = 0; i < 3; ++i) x[i] -= dx[i];
    x[0] = clipf(x[0], -0.3f, 0.6f);
    x[1] = clipf(x[1], -1.0f, 0.44f);
    x[2] = clipf(x[2], 0.0f, 1.0f);
  }
  x[0] = best[0]; x[1] = best[1]; x[2] = best[2];
  trim_residual(icb, x, sT, C, r);
  double* o = ic_out + (int64_t)F16_IC_N * k;
  for (int j = 0; j < F16_IC_N; ++j) o[j] = icb[j];
  const double vt = icb[F16_IC_U_FPS];
  o[F16_IC_U_FPS] = vt * cos((double)x[0]);
  o[F16_IC_V_FPS] = 0.0;
  o[F16_IC_W_FPS] = vt * sin((double)x[0]);
  o[F16_IC_THETA_RAD] = x[0];
  o[F16_IC_PHI_RAD] = 0.0;
  o[F16_IC_P_RPS] = o[F16_IC_Q_RPS] = o[F16_IC_R_RPS] = 0.0;
  o[F16_IC_CMD_AIL] = 0.0; o[F16_IC_CMD_RUD] = 0.0;
  o[F16_IC_CMD_ELE] = x[1];
  o[F16_IC_CMD_THR] = x[2];
  if (resid)
    for (int i = 0; i < 3; ++i) resid[3 * k + i] = fabsf(r[i]);
}
