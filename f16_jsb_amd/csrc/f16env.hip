// f16env.hip -- the host side of libf16env.so: the handle, and the extern "C" ABI declared in
// include/f16env.h. It holds no device code: every kernel is in one of the per-subject headers
// included below (source map), which this single translation unit compiles together.
//
// Hot path: f16_step.h's kernel = one VecEnv step for N envs in ONE launch: 4 FDM frames per lane
// with the state in VGPRs (f16_device.h), then the env layer of jsbsim_gym/jsbsim_gym.py
// (:172-197 frame, :237-261 reward/termination, :487-509 shaping, TimeLimit, Monitor
// stats) and the DummyVecEnv auto-reset (dummy_vec_env.py:56-73) for lanes that finished,
// with the ordered K-frame stack rebuilt by a coalesced per-wave row copy.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/f16env.h"
#include "f16_host.h"
#include "f16_device.h"
#include "f16_env_layer.h"
#include "f16_step.h"
#include "f16_rollout_random.h"
#include "f16_reset.h"
#include "f16_features.h"
#include "f16_rollout_data.h"
#include "f16_policy.h"
#include "f16_policy_lma.h"
#include "f16_policy_lma_grad.h"
#include "f16_ppo.h"
#include "f16_ppo_am.h"

using namespace f16;

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// The buffers of a windowed step. In the handle (f16env_window_bind) hist[] is indexed by parity;
// as step_window_impl's argument hist[0] is this step's history and hist[1] the other.
struct WindowBufs {
  float* hist[2] = {nullptr, nullptr};
  int64_t T = 0;
  float* rew = nullptr;
  uint8_t *term = nullptr, *trunc = nullptr;
  double* ep_ret = nullptr;
  int32_t* ep_len = nullptr;
};

// (every device pointer starts null, so env_free takes a handle at any stage of f16env_create)
struct f16env {
  f16env_config cfg;
  int device;
  void* mem = nullptr;       // state SoA
  void* tmem = nullptr;      // template SoA (n = 1)
  double* ic_dev = nullptr;  // default IC, RANDOM_IC box lo, hi (3 x F16_IC_N)
  int32_t* done_buf = nullptr;  // deferred modes: own done list (N) + two counts, when the caller gives none
  int done_par;       // which of the two counts the next step uses
  unsigned long long* nonfinite = nullptr;  // F16_FLAG_NAN_GUARD quarantine counter (device, 8 B) + a
                                            // scratch word (the wind probe's)
  int mode;           // step kernel variant: bit 0 RANDOM_IC, bit 1 wind (GUSTS, or lanes with
                      // steady wind: config / random-IC box / set_state)
  int occ;            // waves per SIMD the step kernel is compiled for (1 or 2)
  int win_occ;        // the same for the windowed-observation step kernel
  int win_env_major;  // window histories [N][T][16] (1) instead of the default [T][N][16] (0)
  int win_nt;         // windowed step: non-temporal output stores
  float* fw[2];       // f16env_window_feature_bind: the feature histories (parity 0, 1)
  float* poses;       // f16env_window_poses_bind: N x 10 pose export of F16_STEP_POSES steps
  WindowBufs wb;      // f16env_window_bind: the buffers of f16env_window_step_bound
  SoA soa, tmpl;
  // cfg5 modes: reset cache (f16_ic_fill_kernel), allocated at create (or at the first use by a
  // handle that gained wind later); refilled every icc_period windowed steps, and at the next
  // one after anything that changes the lanes' episode counters (icc_steps = 0)
  SoA icc = {nullptr, 0};
  int64_t icc_steps;
  int icc_period;
  ModelConsts C;
  size_t bytes;
  int lds_image;   // step kernel stack-rebuild mode (LDS image when it fits)
  int gt;          // 1: the global-table step kernel (the image needs all of LDS, large K)
  size_t dyn_lds;  // dynamic LDS bytes per step-kernel block
  // kernel timing (f16env_profile_begin/end): start/stop events recorded by the step
  // kernel's own dispatch (hipExtLaunchKernel), one pair per launch
  std::vector<hipEvent_t> prof_ev;
  int prof_next = 0;
};

static void soa_carve(void* base, int64_t n, SoA& s) {
  s.n = n;
  s.c = (float4*)base;
}
static size_t soa_bytes(int64_t n) { return (size_t)n * NCOL_ALL * 16; }

// Same constants derivation as oracle init_consts() (f16.xml:37-83,245-300); the mass
// properties are compile-time constants (f16_device.h f16_mass_props, shared with the kernels).
static void build_consts(const f16env_config& cfg, ModelConsts& C) {
  C.inv_gref = (float)((WGS_A * WGS_A) / GM_E);
  // US-76 sea level in JSBSim units
  const double R = 8.31432 / 0.0289644;
  C.rho_sl = (float)(101325.0 / (R * 288.15) / 515.3788183931961);
  C.a_sl = (float)(sqrt(1.4 * R * 288.15) / 0.3048);
  C.p_sl = (float)(101325.0 / 47.88025898033584);
  C.inv_rho_sl = (float)(1.0 / (101325.0 / (R * 288.15) / 515.3788183931961));
  C.inv_p_sl = (float)(47.88025898033584 / 101325.0);
  C.kts_per_fps = (float)(1.0 / (1852.0 / (3600.0 * 0.3048)));
  // impact pressure at the FCS's calibrated-airspeed thresholds (f16.xml: TEF switch, PID
  // triggers), subsonic pitot (all four are far below calibrated Mach 1)
  const double a_sl = sqrt(1.4 * R * 288.15) / 0.3048, p_sl = 101325.0 / 47.88025898033584;
  auto qc_at = [&](double kts) {
    const double m = kts * (1852.0 / (3600.0 * 0.3048)) / a_sl;
    return (float)(p_sl * (pow(1.0 + 0.2 * m * m, 3.5) - 1.0));
  };
  C.qc_vc250 = qc_at(250.0); C.qc_vc20 = qc_at(20.0); C.qc_vc10 = qc_at(10.0); C.qc_vc5 = qc_at(5.0);
  C.dt = cfg.dt;
  C.cos_dE = cos(OMEGA_E * cfg.dt);
  C.sin_dE = sin(OMEGA_E * cfg.dt);
  C.epa_dt = OMEGA_E * cfg.dt;
  // fp32 products the frames formerly formed per frame (f16_device.h kin2 / pidf / frame): the
  // same single fp32 roundings, here in host IEEE arithmetic
  const float dt = (float)cfg.dt;
  C.dt_f = dt;
  C.half_dt = 0.5f * dt;
  C.dt_12 = dt * (1.0f / 12.0f);
  C.lim_ail = dt * (2.0f / 0.3f);
  C.lim_rud = dt * (2.0f / 0.4f);
  C.lim_lef = dt * (2.0f / 3.0f);
  C.lim_sb = dt * 60.0f;
  C.kidt_roll = 0.0005f * dt;
  C.kidt_pitch = 0.025f * dt;
  C.kidt_yaw = 0.00001f * dt;
}

static EnvArgs env_args(const f16env* h) {
  EnvArgs E;
  E.n = h->cfg.n_envs;
  E.K = h->cfg.stack_k;
  E.down_sample = h->cfg.down_sample;
  E.max_steps = h->cfg.max_steps;
  E.flags = h->cfg.flags;
  E.dg = (float)h->cfg.dg_m;
  E.crash = (float)h->cfg.crash_alt_m;
  E.gain = h->cfg.goal_gain;
  E.seed = h->cfg.seed;
  E.id_base = h->cfg.env_id_base;
  E.ic_cfg = h->ic_dev;
  E.ic_lo = h->ic_dev + F16_IC_N;
  E.ic_hi = h->ic_dev + 2 * F16_IC_N;
  // a = exp(-T/tau), b = sigma sqrt(1 - a^2) over the env step T = down_sample dt (oracle gust_coeffs)
  const double ga = h->cfg.gust_tau_s > 0.0 ? exp(-(double)h->cfg.down_sample * h->cfg.dt / h->cfg.gust_tau_s) : 0.0;
  E.gust_a = (float)ga;
  E.gust_b = (float)(h->cfg.gust_sigma_fps * sqrt(1.0 - ga * ga));
  E.gust_sigma = (float)h->cfg.gust_sigma_fps;
  if (!(h->cfg.flags & F16_FLAG_GUSTS)) {  // wind kernels without gusts: the gust term holds still
    E.gust_a = 1.0f; E.gust_b = 0.0f; E.gust_sigma = 0.0f;
  }
  return E;
}

static inline unsigned nblocks(int64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// How a step resets the lanes it finishes. MODE 0 copies the IC template inside the step kernel.
// The cfg5 modes need a RunIC per lane: the windowed step takes it from the reset cache, also
// inside the kernel (RESET_CACHE); with F16ENV_ICC_PERIOD=0, and always in the contiguous layout,
// f16_reset_done_kernel rewrites the step's done list behind it (RESET_DEFERRED).
enum ResetMode { RESET_NONE, RESET_TEMPLATE, RESET_CACHE, RESET_DEFERRED };
static ResetMode reset_mode(const f16env* h, bool windowed) {
  if (h->cfg.flags & F16_FLAG_NO_AUTORESET) return RESET_NONE;
  if (!h->mode) return RESET_TEMPLATE;
  return windowed && h->icc_period > 0 ? RESET_CACHE : RESET_DEFERRED;
}

// Where the K frames of an env's observation lie in a caller's buffer: frame j of env k at
// base + k * row + off + j * pitch, `slot` floats each.
struct FrameView {
  float* base;
  int64_t row, off, pitch;
  int32_t slot;
  float* first() const { return base + off; }  // env 0's oldest frame
};
static FrameView contiguous_view(const f16env* h, float* obs) {  // N x K x 15
  return {obs, (int64_t)h->cfg.stack_k * F16_OBS_DIM, 0, F16_OBS_DIM, F16_OBS_DIM};
}
// the K positions up to `pos` of a window history of T positions, in the handle's order:
// [T][N][16], or [N][T][16] after f16env_set_window_order(1)
static FrameView window_view(const f16env* h, float* hist, int64_t T, int32_t pos) {
  const int64_t pitch = h->win_env_major ? WPITCH : (int64_t)h->cfg.n_envs * WPITCH;
  const int64_t row = h->win_env_major ? T * WPITCH : WPITCH;
  return {hist, row, (int64_t)(pos - h->cfg.stack_k + 1) * pitch, pitch, WPITCH};
}
template <class Args>  // ResetArgs, ResetDoneArgs
static void set_obs_view(Args& a, const FrameView& v) {
  a.obs = v.base; a.obs_row = v.row; a.obs_off = v.off; a.obs_pitch = v.pitch; a.obs_slot = v.slot;
}

static void prof_free(f16env* h) {
  for (hipEvent_t e : h->prof_ev) hipEventDestroy(e);
  h->prof_ev.clear();
  h->prof_next = 0;
}

// The one teardown: f16env_destroy's, and every failure path's of f16env_create
static void env_free(f16env* h) {
  hipSetDevice(h->device);
  if (h->mem) hipFree(h->mem);
  if (h->tmem) hipFree(h->tmem);
  if (h->ic_dev) hipFree(h->ic_dev);
  if (h->done_buf) hipFree(h->done_buf);
  if (h->icc.c) hipFree(h->icc.c);
  if (h->nonfinite) hipFree(h->nonfinite);
  prof_free(h);
  delete h;
}

// cfg5 modes: the reset cache's memory, zeroed (tag 0: no row valid yet) and counted in
// f16env_state_bytes
static int icc_alloc(f16env* h, hipStream_t st) {
  const size_t b = (size_t)ICC_COLS * 16 * (size_t)h->cfg.n_envs;
  if (hipMalloc((void**)&h->icc.c, b) != hipSuccess) {
    h->icc.c = nullptr;
    return set_err(-3, "hipMalloc(reset cache) failed");
  }
  HIPCHK(hipMemsetAsync(h->icc.c, 0, b, st));
  h->bytes += b;
  return 0;
}

// "Can any lane carry wind now?", asked of a launch that writes lanes: the handle's scratch word
// is zeroed, `launch(word)` issues the kernel (which sets it for a lane with wind), the word is
// read back (this waits for the stream: neither caller is on the hot path) and a handle that got
// wind runs the wind kernels from now on (mode bit 1).
template <class Launch>
static int wind_probe(f16env* h, hipStream_t st, Launch launch) {
  int* wind_any = reinterpret_cast<int*>(h->nonfinite + 1);
  HIPCHK(hipMemsetAsync(wind_any, 0, sizeof(int), st));
  launch(wind_any);
  HIPCHK(hipGetLastError());
  int w = 0;
  HIPCHK(hipMemcpyAsync(&w, wind_any, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (w) h->mode |= 2;
  return 0;
}

extern "C" {

int f16env_config_default(f16env_config* c) {
  if (!c) return set_err(-1, "null config");
  memset(c, 0, sizeof *c);
  c->n_envs = 1;
  c->stack_k = 10;
  c->down_sample = 4;
  c->max_steps = 1200;
  c->dt = 1.0 / 120.0;
  c->dg_m = 100.0;
  c->goal_gain = 1e-2;
  c->crash_alt_m = 10.0;
  c->ic[F16_IC_H_SL_FT] = 5000.0;
  c->ic[F16_IC_U_FPS] = 900.0;
  for (int j = 0; j < F16_IC_N; ++j) c->ic_lo[j] = c->ic_hi[j] = c->ic[j];
  c->gust_sigma_fps = 0.0;
  c->gust_tau_s = 2.0;
  return 0;
}

int f16env_config_cfg5(f16env_config* c) {
  if (!c) return set_err(-1, "null config");
  c->flags |= F16_FLAG_RANDOM_IC | F16_FLAG_GUSTS;
  for (int j = 0; j < F16_IC_N; ++j) c->ic_lo[j] = c->ic_hi[j] = c->ic[j];
  const double deg10 = 0.17453292519943295;
  c->ic_lo[F16_IC_H_SL_FT] = 3000.0;  c->ic_hi[F16_IC_H_SL_FT] = 30000.0;
  c->ic_lo[F16_IC_U_FPS] = 600.0;     c->ic_hi[F16_IC_U_FPS] = 1200.0;
  c->ic_lo[F16_IC_PHI_RAD] = -deg10;  c->ic_hi[F16_IC_PHI_RAD] = deg10;
  c->ic_lo[F16_IC_THETA_RAD] = -deg10; c->ic_hi[F16_IC_THETA_RAD] = deg10;
  c->ic_lo[F16_IC_PSI_RAD] = 0.0;     c->ic_hi[F16_IC_PSI_RAD] = 6.283185307179586;
  c->ic_lo[F16_IC_CMD_THR] = 0.3;     c->ic_hi[F16_IC_CMD_THR] = 1.0;
  c->ic_lo[F16_IC_WIND_N_FPS] = -30.0; c->ic_hi[F16_IC_WIND_N_FPS] = 30.0;
  c->ic_lo[F16_IC_WIND_E_FPS] = -30.0; c->ic_hi[F16_IC_WIND_E_FPS] = 30.0;
  c->gust_sigma_fps = 10.0;
  c->gust_tau_s = 2.0;
  return 0;
}

// f16env_create behind the handle's allocation (cfg and device are set): the device memory, the
// kernel choices and the IC template. On an error the caller frees the handle (env_free).
static int env_init(f16env* h) {
  const f16env_config* cfg = &h->cfg;
  const int device = h->device;
  build_consts(*cfg, h->C);
  h->bytes = soa_bytes(cfg->n_envs);
  if (hipMalloc(&h->mem, h->bytes) != hipSuccess) return set_err(-3, "hipMalloc(state) failed");
  HIPCHK(hipMemset(h->mem, 0, h->bytes));
  soa_carve(h->mem, cfg->n_envs, h->soa);
  bool wind = false;  // can any lane carry wind? (then the wind kernels: MODE bit 1)
  for (int j = F16_IC_WIND_N_FPS; j <= F16_IC_WIND_D_FPS; ++j)
    wind = wind || cfg->ic[j] != 0.0 ||
           ((cfg->flags & F16_FLAG_RANDOM_IC) && (cfg->ic_lo[j] != 0.0 || cfg->ic_hi[j] != 0.0));
  h->mode = ((cfg->flags & F16_FLAG_RANDOM_IC) ? 1 : 0) | (((cfg->flags & F16_FLAG_GUSTS) || wind) ? 2 : 0);
  h->icc.n = cfg->n_envs;
  h->icc_steps = 0;
  // same-box sweep, 2 048 cfg5 steps: 27.5 / 27.0 / 27.0 / 26.8 / 27.7 us at 32..512
  h->icc_period = env_int("F16ENV_ICC_PERIOD", 64);
  if (hipMalloc(&h->tmem, (size_t)TMPL_COLS * 16) != hipSuccess ||
      hipMalloc((void**)&h->ic_dev, sizeof(double) * 3 * F16_IC_N) != hipSuccess ||
      hipMalloc((void**)&h->done_buf, sizeof(int32_t) * ((size_t)cfg->n_envs + 2)) != hipSuccess)
    return set_err(-3, "hipMalloc(template) failed");
  soa_carve(h->tmem, 1, h->tmpl);
  HIPCHK(hipMemset(h->done_buf + cfg->n_envs, 0, 2 * sizeof(int32_t)));
  h->done_par = 0;
  if (hipMalloc((void**)&h->nonfinite, 4 * sizeof(unsigned long long)) != hipSuccess)
    return set_err(-3, "hipMalloc(counter) failed");
  HIPCHK(hipMemset(h->nonfinite, 0, 4 * sizeof(unsigned long long)));
  {
    const int KC = cfg->stack_k * F16_OBS_DIM;
    const size_t img = sizeof(float) * (BLOCK / 64) * ((size_t)64 * KC + 16);
    const size_t fallback = sizeof(float) * 2 * BLOCK * FRAME_PITCH;
    const size_t static_gt = 16 * (NCOL + TMPL_FRAME_COLS) + sizeof(int) * BLOCK + 64;
    const size_t static_lds = sizeof(float) * F16_BLOB_FLOATS + static_gt;
    // the stack image with LDS tables if both fit, else with global tables, else the
    // chunked flat copy (LDS tables)
    h->lds_image = (img + static_lds <= 160 * 1024) ? 1 : (img + static_gt <= 160 * 1024 ? 1 : 0);
    h->gt = (h->lds_image && img + static_lds > 160 * 1024) ? 1 : 0;
    if (h->lds_image) h->gt = env_int("F16ENV_GT", h->gt) ? 1 : 0;
    h->dyn_lds = h->lds_image ? img : fallback;
    // two waves per SIMD only pay when there are more waves than SIMDs and two workgroups'
    // LDS (tables + stack image) fit in one CU
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
      cus = 256;
    const int64_t waves = ((int64_t)cfg->n_envs + 63) / 64;
    h->occ = (!h->gt && waves > 4 * (int64_t)cus && 2 * (static_lds + h->dyn_lds) <= 160 * 1024) ? 2 : 1;
    h->occ = env_int("F16ENV_OCC", h->occ) == 2 ? 2 : 1;
    h->win_occ = (waves > 4 * (int64_t)cus && 2 * (static_lds + WIN_DYN_LDS) <= 160 * 1024) ? 2 : 1;
    h->win_occ = env_int("F16ENV_OCC", h->win_occ) == 2 ? 2 : 1;
    // non-temporal output stores pay in the windowed step when its whole grid is resident at
    // once (one round of waves); with more rounds they cost (st16)
    h->win_nt = waves <= (int64_t)h->win_occ * 4 * cus ? 1 : 0;
    h->win_nt = env_int("F16ENV_WIN_NT", h->win_nt) ? 1 : 0;
    for (int v = 0; v <= 2; ++v) {
      const size_t st_v = v == 2 ? static_gt : static_lds;
      for (int m = 0; m < 8; ++m) {
        const size_t dyn = h->dyn_lds;
        if (st_v + dyn > 160 * 1024) continue;  // not launchable in this configuration
        if (hipFuncSetAttribute((const void*)step_kernel_for(m & 3, v, m >= 4), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)dyn) != hipSuccess) {
          (void)hipGetLastError();
          return set_err(-2, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
        }
      }
    }
  }
  // cfg5 modes: the reset cache up front (its bytes are part of f16env_state_bytes); a handle
  // that only gains wind later (set_state / a per-lane IC) allocates it at its first use
  // (with F16ENV_ICC_PERIOD=0 too, where only the rollout kernel reads it)
  if (reset_mode(h, false) == RESET_DEFERRED)
    if (int e = icc_alloc(h, nullptr)) return e;
  HIPCHK(hipMemcpy(h->ic_dev, cfg->ic, sizeof(double) * F16_IC_N, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->ic_dev + F16_IC_N, cfg->ic_lo, sizeof(double) * F16_IC_N, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->ic_dev + 2 * F16_IC_N, cfg->ic_hi, sizeof(double) * F16_IC_N, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(f16_ic_kernel, dim3(1), dim3(BLOCK), 0, 0, h->tmpl, (const double*)h->ic_dev, h->C);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return set_err(-2, hipGetErrorString(e));
  return 0;
}

int f16env_create(const f16env_config* cfg, int device, f16env_t* out) {
  if (!cfg || !out) return set_err(-1, "null argument");
  if (cfg->n_envs <= 0) return set_err(-1, "n_envs must be > 0");
  if (cfg->stack_k < 1 || cfg->stack_k > 64) return set_err(-1, "stack_k must be in [1, 64]");
  if (cfg->down_sample < 0) return set_err(-1, "down_sample must be >= 0");
  if (!(cfg->dt > 0.0)) return set_err(-1, "dt must be > 0");
  if ((cfg->flags & F16_FLAG_GUSTS) && !(cfg->gust_sigma_fps >= 0.0 && cfg->gust_tau_s > 0.0))
    return set_err(-1, "gusts need gust_sigma_fps >= 0 and gust_tau_s > 0");
  HIPCHK(hipSetDevice(device));
  f16env* h = new f16env();
  h->cfg = *cfg;
  h->device = device;
  if (int e = env_init(h)) {
    env_free(h);  // (leaves the thread's error message alone)
    return e;
  }
  *out = h;
  return 0;
}

int f16env_profile_begin(f16env_t h, int max_launches) {
  if (!h || max_launches <= 0 || max_launches > 100000) return set_err(-1, "max_launches must be in [1, 100000]");
  prof_free(h);
  h->prof_ev.resize((size_t)2 * max_launches);
  for (auto& e : h->prof_ev) HIPCHK(hipEventCreate(&e));
  return 0;
}

int f16env_profile_end(f16env_t h, double* avg_ms, double* min_ms, int* launches) {
  if (!h) return set_err(-1, "null handle");
  const int n = h->prof_next;
  double sum = 0.0, mn = 0.0;
  for (int i = 0; i < n; ++i) {
    HIPCHK(hipEventSynchronize(h->prof_ev[2 * i + 1]));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, h->prof_ev[2 * i], h->prof_ev[2 * i + 1]));
    sum += ms;
    mn = (i == 0 || ms < mn) ? ms : mn;
  }
  if (avg_ms) *avg_ms = n ? sum / n : 0.0;
  if (min_ms) *min_ms = mn;
  if (launches) *launches = n;
  prof_free(h);
  return 0;
}

int f16env_profile_times(f16env_t h, double* t_ms, int max_launches) {
  if (!h || !t_ms) return set_err(-1, "null argument");
  const int n = h->prof_next < max_launches ? h->prof_next : max_launches;
  for (int i = 0; i < n; ++i) {
    HIPCHK(hipEventSynchronize(h->prof_ev[2 * i + 1]));
    float a = 0.0f, b = 0.0f;
    HIPCHK(hipEventElapsedTime(&a, h->prof_ev[0], h->prof_ev[2 * i]));
    HIPCHK(hipEventElapsedTime(&b, h->prof_ev[0], h->prof_ev[2 * i + 1]));
    t_ms[2 * i] = a;
    t_ms[2 * i + 1] = b;
  }
  return n;
}

int f16env_destroy(f16env_t h) {
  if (h) env_free(h);
  return 0;
}

size_t f16env_state_bytes(f16env_t h) { return h ? h->bytes : 0; }
int f16env_state_bytes_per_env(void) { return STATE_BYTES; }

// The reset of f16env_reset / f16env_reset_window into the frames of `v`. A per-lane IC may carry
// wind: a handle that runs the still-air kernels then asks (wind_probe).
static int reset_launch(f16env_t h, hipStream_t st, const uint8_t* mask, const float* goals, const double* ic,
                        const FrameView& v) {
  h->icc_steps = 0;  // the lanes' episode counters move: the next windowed step refills the reset cache
  ResetArgs a;
  a.s = h->soa; a.tmpl = h->tmpl; a.mask = mask; a.goals = goals; a.ic = ic;
  set_obs_view(a, v);
  a.E = env_args(h);
  a.C = h->C;
  auto launch = [&](int* wind_any) {
    a.wind_any = wind_any;
    hipLaunchKernelGGL(f16_reset_kernel, dim3(nblocks(a.E.n)), dim3(BLOCK), 0, st, a);
  };
  if (ic && !(h->mode & 2)) return wind_probe(h, st, launch);
  launch(nullptr);
  HIPCHK(hipGetLastError());
  return 0;
}

int f16env_reset(f16env_t h, void* stream, const uint8_t* mask, const float* goals, const double* ic, float* obs) {
  if (!h) return set_err(-1, "null handle");
  return reset_launch(h, (hipStream_t)stream, mask, goals, ic, contiguous_view(h, obs));
}

// The done list of a step: the caller's (its count zeroed here), else, in deferred modes, the
// handle's own with two alternating counts -- the step's deferred-reset kernel zeroes the one
// the next step uses, so an auto-resetting step issues no memset (one GPU operation fewer).
static int done_counter(f16env_t h, int32_t* done_idx, int32_t*& list, int32_t*& count, int32_t*& zero_next,
                        hipStream_t st) {
  zero_next = nullptr;
  if (h->mode && !done_idx) {  // deferred resets need the done list
    list = h->done_buf;
    count = h->done_buf + h->cfg.n_envs + h->done_par;
    if (!(h->cfg.flags & F16_FLAG_NO_AUTORESET)) {  // the reset kernel follows: it zeroes the other
      zero_next = h->done_buf + h->cfg.n_envs + (h->done_par ^ 1);
      h->done_par ^= 1;
      return 0;
    }
  }
  if (count) HIPCHK(hipMemsetAsync(count, 0, sizeof(int32_t), st));
  return 0;
}

// One step-kernel launch: timed by the dispatch packet's own events while a profile is armed
// (f16env_profile_*), else plain
static int launch_step(f16env_t h, StepKernel kern, dim3 grid, size_t dyn_lds, hipStream_t st, const StepArgs& a) {
  const dim3 blk(BLOCK);
  const float4* sc = a.s.c;
  const float4* tc = a.tmpl.c;
  if (h->prof_next < (int)h->prof_ev.size() / 2) {
    const int i = h->prof_next++;
    hipExtLaunchKernelGGL(kern, grid, blk, (std::uint32_t)dyn_lds, st, h->prof_ev[2 * i], h->prof_ev[2 * i + 1], 0u,
                          sc, a.act, tc, a.E.n, a);
  } else {
    hipLaunchKernelGGL(kern, grid, blk, dyn_lds, st, sc, a.act, tc, a.E.n, a);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// The deferred reset behind a step (cfg5 modes): f16_reset_done_kernel rewrites the rows of the
// step's done list in the returned observation `v`
static int launch_reset_done(f16env_t h, hipStream_t st, const StepArgs& a, const FrameView& v, int32_t* zero_next) {
  ResetDoneArgs r;
  r.s = h->soa; r.tmpl = h->tmpl; r.done_idx = a.done_idx; r.n_done = a.n_done;
  set_obs_view(r, v);
  r.zero_next = zero_next;
  r.E = a.E; r.C = h->C;
  const unsigned g = nblocks(a.E.n) < 64u ? nblocks(a.E.n) : 64u;
  hipLaunchKernelGGL(f16_reset_done_kernel, dim3(g), dim3(BLOCK), 0, st, r);
  HIPCHK(hipGetLastError());
  return 0;
}

// A rollout slot's layout-independent fields into the step's arguments (the frame pointer is the
// layout's own: r_frame / r_next_frame); returns where the slot wants the policy features
static float* slot_args(const f16env_rollout_slot* slot, StepArgs& a) {
  a.clip_act = (slot->flags & F16_SLOT_CLIP) ? 1 : 0;
  a.act_seed = slot->act_seed; a.act_step = slot->act_step;
  a.r_act = slot->actions; a.r_rew = slot->rewards;
  a.r_next_start = slot->next_start;
  return slot->features;
}

static int step_impl(f16env_t h, void* stream, const f16env_rollout_slot* slot, const float* act,
                     const float* obs_prev, float* obs, float* rew, uint8_t* terminated, uint8_t* truncated,
                     float* terminal_obs, double* ep_return, int32_t* ep_len, int32_t* done_idx, int32_t* n_done) {
  if (!h) return set_err(-1, "null handle");
  if ((!act && !slot) || !obs_prev || !obs || !rew || !terminated || !truncated)
    return set_err(-1, "act (or a rollout slot)/obs_prev/obs/rew/terminated/truncated are required");
  if (done_idx && !n_done) return set_err(-1, "done_idx requires n_done");
  if (act && ((uintptr_t)act & 15) != 0) return set_err(-1, "act must be 16-byte aligned");
  StepArgs a = {};
  a.s = h->soa; a.tmpl = h->tmpl; a.act = act; a.obs_prev = obs_prev; a.obs = obs; a.rew = rew;
  a.term = terminated; a.trunc = truncated; a.tobs = terminal_obs; a.ep_ret = ep_return; a.ep_len = ep_len;
  a.done_idx = done_idx; a.n_done = n_done;
  a.nonfinite = h->nonfinite;
  a.sample_act = act ? 0 : 1;
  float* feat = nullptr;
  if (slot) {
    if (slot->next_frame)
      return set_err(-1, "rollout slot next_frame is the windowed layout's (f16env_window_step_rollout); "
                         "the contiguous layout writes frame");
    a.r_frame = slot->frame;
    feat = slot_args(slot, a);
  }
  if ((a.r_frame && ((uintptr_t)a.r_frame & 15) != 0) || (a.r_act && ((uintptr_t)a.r_act & 15) != 0))
    return set_err(-1, "rollout slot frame/actions must be 16-byte aligned");
  a.E = env_args(h);
  a.C = h->C;
  a.lds_image = h->lds_image;
  if (((uintptr_t)obs & 15) != 0 || ((uintptr_t)obs_prev & 15) != 0)
    return set_err(-1, "obs and obs_prev must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int32_t* zero_next = nullptr;
  if (int e = done_counter(h, done_idx, a.done_idx, a.n_done, zero_next, st)) return e;
  const StepKernel kern = step_kernel_for(h->mode, h->gt ? 2 : (h->occ == 2 ? 1 : 0), slot != nullptr);
  if (int e = launch_step(h, kern, dim3(nblocks(a.E.n)), h->dyn_lds, st, a)) return e;
  if (reset_mode(h, false) == RESET_DEFERRED)
    if (int e = launch_reset_done(h, st, a, contiguous_view(h, obs), zero_next)) return e;
  if (feat) {  // policy features of the returned obs (after any deferred reset rewrote rows)
    const int64_t nf = (int64_t)a.E.n * a.E.K;
    hipLaunchKernelGGL(f16_features_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, nf,
                       (const float*)obs, feat);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

int f16env_step(f16env_t h, void* stream, const float* act, const float* obs_prev, float* obs, float* rew,
                uint8_t* terminated, uint8_t* truncated, float* terminal_obs, double* ep_return, int32_t* ep_len,
                int32_t* done_idx, int32_t* n_done) {
  return step_impl(h, stream, nullptr, act, obs_prev, obs, rew, terminated, truncated, terminal_obs, ep_return,
                   ep_len, done_idx, n_done);
}

int f16env_set_window_order(f16env_t h, int env_major) {
  if (!h) return set_err(-1, "null handle");
  h->win_env_major = env_major ? 1 : 0;
  return 0;
}

// cfg5 modes: the reset cache, allocated if this handle has none yet (it gained wind after
// create), refilled now if `fill` (f16_ic_fill_kernel: every lane whose cached row is not its
// next episode's)
static int icc_prepare(f16env_t h, hipStream_t st, bool fill) {
  const int64_t n = h->cfg.n_envs;
  if (!h->icc.c) {
    if (int e = icc_alloc(h, st)) return e;
    fill = true;
  }
  h->icc.n = n;
  if (fill) {
    hipLaunchKernelGGL(ic_fill_kernel_for(h->mode), dim3(nblocks(n)), dim3(BLOCK), 0, st, h->soa, h->icc, env_args(h),
                       h->C);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

static int window_check(f16env_t h, const float* hist_cur, const float* hist_other, int64_t T, int32_t pos) {
  const int K = h->cfg.stack_k;
  if (!hist_cur || (hist_other == nullptr && hist_cur == nullptr)) return set_err(-1, "null history");
  if (((uintptr_t)hist_cur & 15) != 0 || ((uintptr_t)hist_other & 15) != 0)
    return set_err(-1, "histories must be 16-byte aligned");
  if (T < 2 * (int64_t)K) return set_err(-1, "history length T must be >= 2K");
  if (pos < K - 1 || (int64_t)pos >= T) return set_err(-1, "window position must be in [K-1, T-1]");
  return 0;
}

// The feature window in a step's epilogue (`flag`: F16_SLOT_FEATURE_WINDOW or
// F16_STEP_FEATURE_WINDOW, named at the head of each message): the bound feature histories of
// this step's parity and the other
static int feature_window_args(f16env_t h, const char* flag, const float* hist_cur, StepArgs& a) {
  const char* why = nullptr;
  if (!h->fw[0] || !h->fw[1]) why = ": f16env_window_feature_bind first";
  else if (hist_cur != h->wb.hist[0] && hist_cur != h->wb.hist[1]) why = ": the step's histories must be the bound ones";
  else if (reset_mode(h, true) == RESET_DEFERRED) why = ": not with the deferred-reset step (F16ENV_ICC_PERIOD=0)";
  if (why) return set_err(-1, (std::string(flag) + why).c_str());  // (the message is built on a refusal only)
  const int b = hist_cur == h->wb.hist[0] ? 0 : 1;
  a.fwx = h->fw[b]; a.fwy = h->fw[b ^ 1];
  return 0;
}

// w: hist[0] is this step's history (parity), hist[1] the other
static int step_window_impl(f16env_t h, void* stream, const f16env_rollout_slot* slot, const float* act,
                            const WindowBufs& w, int32_t pos, int32_t* done_idx, int32_t* n_done, bool ex = false,
                            uint32_t xflags = 0, uint64_t act_seed = 0, uint64_t act_step = 0) {
  if (!h) return set_err(-1, "null handle");
  float* const hist_cur = w.hist[0];
  float* const hist_other = w.hist[1];
  if ((!act && !slot && !ex) || !hist_other || !w.rew || !w.term || !w.trunc)
    return set_err(-1, "act (or a rollout slot)/hist_cur/hist_other/rew/terminated/truncated are required");
  if (int e = window_check(h, hist_cur, hist_other, w.T, pos)) return e;
  if (hist_cur == hist_other) return set_err(-1, "the two histories must be distinct buffers");
  if (done_idx && !n_done) return set_err(-1, "done_idx requires n_done");
  if (act && ((uintptr_t)act & 15) != 0) return set_err(-1, "act must be 16-byte aligned");
  StepArgs a = {};
  a.s = h->soa; a.tmpl = h->tmpl; a.act = act; a.rew = w.rew;
  a.term = w.term; a.trunc = w.trunc; a.ep_ret = w.ep_ret; a.ep_len = w.ep_len;
  a.done_idx = done_idx; a.n_done = n_done;
  a.nonfinite = h->nonfinite;
  float* feat = nullptr;
  if (slot) {
    if (slot->frame)
      return set_err(-1, "rollout slot frame is the contiguous layout's; the windowed layout writes next_frame "
                         "(the newest frame of the returned observation)");
    a.sample_act = act ? 0 : 1;
    a.r_next_frame = slot->next_frame;
    feat = slot_args(slot, a);
    if ((a.r_next_frame && ((uintptr_t)a.r_next_frame & 3) != 0) || (a.r_act && ((uintptr_t)a.r_act & 15) != 0))
      return set_err(-1, "rollout slot next_frame must be 4-byte and actions 16-byte aligned");
    if (slot->flags & F16_SLOT_FEATURE_WINDOW)
      if (int e = feature_window_args(h, "F16_SLOT_FEATURE_WINDOW", hist_cur, a)) return e;
  } else if (ex) {  // f16env_window_step_ex: the winx build (in-kernel actions, feature window)
    a.sample_act = act ? 0 : 1;
    a.act_seed = act_seed; a.act_step = act_step;
    if (xflags & ~(uint32_t)(F16_STEP_FEATURE_WINDOW | F16_STEP_POSES))
      return set_err(-1, "unknown f16env_window_step_ex flags");
    if (xflags & F16_STEP_POSES) {
      if (!h->poses) return set_err(-1, "F16_STEP_POSES: f16env_window_poses_bind first");
      if (reset_mode(h, true) == RESET_DEFERRED)
        return set_err(-1, "F16_STEP_POSES: not with the deferred-reset step (F16ENV_ICC_PERIOD=0)");
      a.poses = h->poses;
    }
    if (xflags & F16_STEP_FEATURE_WINDOW)
      if (int e = feature_window_args(h, "F16_STEP_FEATURE_WINDOW", hist_cur, a)) return e;
  }
  // cfg5 modes: finished lanes are reset inside the step from the reset cache (period 0 or
  // F16ENV_ICC_PERIOD=0: the deferred f16_reset_done_kernel instead)
  const ResetMode resets = reset_mode(h, true);
  // the deferred reset rewrites finished lanes' windows after the step kernel, so a slot frame or
  // features written by the step would describe the pre-reset window: rejected here, before any
  // launch, so that a refused call leaves the device state untouched
  if (resets == RESET_DEFERRED && slot && (slot->next_frame || feat))
    return set_err(-1, "the deferred-reset windowed step (F16ENV_ICC_PERIOD=0) writes no next_frame / features");
  const FrameView v = window_view(h, hist_cur, w.T, pos);  // the returned observation
  a.wx = hist_cur; a.wy = hist_other; a.wrow = v.pitch; a.wenv = v.row; a.wpos = pos;
  a.E = env_args(h);
  a.C = h->C;
  hipStream_t st = (hipStream_t)stream;
  int32_t* zero_next = nullptr;
  a.icc.n = a.E.n;
  if (resets == RESET_CACHE) {
    if (int e = icc_prepare(h, st, h->icc_steps % h->icc_period == 0)) return e;
    ++h->icc_steps;
    a.icc = h->icc;
    if (n_done) HIPCHK(hipMemsetAsync(n_done, 0, sizeof(int32_t), st));  // the caller's done list only
  } else if (int e = done_counter(h, done_idx, a.done_idx, a.n_done, zero_next, st)) {
    return e;
  }
  const WinKernel kern = ex ? step_winx_kernel_for(h->mode, h->win_occ, h->win_nt, a.fwx != nullptr)
                            : step_win_kernel_for(h->mode, h->win_occ, h->win_nt, slot != nullptr);
  if (int e = launch_step(h, kern, dim3(nblocks(a.E.n)), WIN_DYN_LDS, st, a)) return e;
  if (resets == RESET_DEFERRED)
    if (int e = launch_reset_done(h, st, a, v, zero_next)) return e;
  if (feat) {  // policy features of the returned observation, read in place from the window
    const int64_t blocks = ((int64_t)a.E.n * a.E.K + 255) / 256;
    hipLaunchKernelGGL(f16_features_strided_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (int64_t)a.E.n,
                       (int32_t)a.E.K, (const float*)v.first(), v.row, v.pitch, feat);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// the plain windowed step: f16env_step_window, and the bound entry points with nothing extra
static int step_window_plain(f16env_t h, void* stream, const float* act, const WindowBufs& w, int32_t pos,
                             int32_t* done_idx, int32_t* n_done) {
  if (!act) return set_err(-1, "act is required");
  return step_window_impl(h, stream, nullptr, act, w, pos, done_idx, n_done);
}

// the handle's bound buffers as a step of `parity` takes them
static WindowBufs bound_window(const f16env* h, int32_t parity) {
  WindowBufs w = h->wb;
  w.hist[0] = h->wb.hist[parity & 1];
  w.hist[1] = h->wb.hist[(parity & 1) ^ 1];
  return w;
}

int f16env_step_window(f16env_t h, void* stream, const float* act, float* hist_cur, float* hist_other, int64_t T,
                       int32_t pos, float* rew, uint8_t* terminated, uint8_t* truncated, double* ep_return,
                       int32_t* ep_len, int32_t* done_idx, int32_t* n_done) {
  const WindowBufs w = {{hist_cur, hist_other}, T, rew, terminated, truncated, ep_return, ep_len};
  return step_window_plain(h, stream, act, w, pos, done_idx, n_done);
}

int f16env_window_bind(f16env_t h, float* hist0, float* hist1, int64_t T, float* rew, uint8_t* terminated,
                       uint8_t* truncated, double* ep_return, int32_t* ep_len) {
  if (!h) return set_err(-1, "null handle");
  if (!hist0 || !hist1 || hist0 == hist1 || !rew || !terminated || !truncated)
    return set_err(-1, "two distinct histories and rew/terminated/truncated are required");
  if (int e = window_check(h, hist0, hist1, T, h->cfg.stack_k - 1)) return e;
  h->wb.hist[0] = hist0; h->wb.hist[1] = hist1; h->wb.T = T;
  h->wb.rew = rew; h->wb.term = terminated; h->wb.trunc = truncated;
  h->wb.ep_ret = ep_return; h->wb.ep_len = ep_len;
  return 0;
}

int f16env_window_feature_bind(f16env_t h, float* feat0, float* feat1) {
  if (!h) return set_err(-1, "null handle");
  if ((!feat0) != (!feat1) || (feat0 && feat0 == feat1)) return set_err(-1, "two distinct feature histories (or none)");
  if (((((uintptr_t)feat0) | ((uintptr_t)feat1)) & 3) != 0) return set_err(-1, "feature histories must be float-aligned");
  h->fw[0] = feat0; h->fw[1] = feat1;
  return 0;
}

int f16env_window_poses_bind(f16env_t h, float* poses) {
  if (!h) return set_err(-1, "null handle");
  if (((uintptr_t)poses & 3) != 0) return set_err(-1, "poses must be float-aligned");
  h->poses = poses;
  return 0;
}

int f16env_window_step_bound(f16env_t h, void* stream, const float* act, int32_t parity, int32_t pos) {
  if (!h) return set_err(-1, "null handle");
  if (!h->wb.hist[0]) return set_err(-1, "f16env_window_bind first");
  return step_window_plain(h, stream, act, bound_window(h, parity), pos, nullptr, nullptr);
}

int f16env_window_step_ex(f16env_t h, void* stream, const float* act, int32_t parity, int32_t pos, uint32_t flags,
                          uint64_t act_seed, uint64_t act_step) {
  if (!h) return set_err(-1, "null handle");
  if (!h->wb.hist[0]) return set_err(-1, "f16env_window_bind first");
  const WindowBufs w = bound_window(h, parity);
  if (act && !flags)  // nothing extra: the plain windowed step (the headline instance)
    return step_window_plain(h, stream, act, w, pos, nullptr, nullptr);
  // (rew/terminated/truncated are required by the impl; act may be NULL here)
  return step_window_impl(h, stream, nullptr, act, w, pos, nullptr, nullptr, true, flags, act_seed, act_step);
}

const char* f16env_window_step_ex_kernel_name(f16env_t h, uint32_t flags) {
  static thread_local char buf[64];
  if (!h) return "";
  snprintf(buf, sizeof buf, "f16_step_winx_kernel<%d, %d, %s, %d>", h->mode & 3, h->win_occ, h->win_nt ? "true" : "false",
           (flags & F16_STEP_FEATURE_WINDOW) ? (XV_X | XV_FEAT) : XV_X);
  return buf;
}

int f16env_window_step_rollout(f16env_t h, void* stream, const f16env_rollout_slot* slot, const float* act,
                               int32_t parity, int32_t pos) {
  if (!h) return set_err(-1, "null handle");
  if (!slot) return set_err(-1, "null rollout slot");
  if (!h->wb.hist[0]) return set_err(-1, "f16env_window_bind first");
  return step_window_impl(h, stream, slot, act, bound_window(h, parity), pos, nullptr, nullptr);
}

int f16env_reset_window(f16env_t h, void* stream, const uint8_t* mask, const float* goals, const double* ic,
                        float* hist_cur, int64_t T, int32_t pos) {
  if (!h) return set_err(-1, "null handle");
  if (int e = window_check(h, hist_cur, nullptr, T, pos)) return e;
  return reset_launch(h, (hipStream_t)stream, mask, goals, ic, window_view(h, hist_cur, T, pos));
}

int f16env_window_restart(f16env_t h, void* stream, float* hist0, float* hist1, int64_t T, int32_t pos_old) {
  if (!h) return set_err(-1, "null handle");
  if (!hist1) return set_err(-1, "null history");
  if (int e = window_check(h, hist0, hist1, T, pos_old)) return e;
  const int K = h->cfg.stack_k;
  if (K < 2) return 0;
  if (pos_old - K + 2 <= K - 2) return set_err(-1, "restart source and destination overlap (pos_old < 2K-3)");
  const FrameView v = window_view(h, hist0, T, pos_old);  // (for the strides)
  const int64_t blocks = (2 * (int64_t)(K - 1) * h->cfg.n_envs * 4 + 255) / 256;
  if (blocks > 0x7fffffffLL) return set_err(-1, "history too large for one restart launch");
  hipLaunchKernelGGL(f16_window_restart_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     (int64_t)h->cfg.n_envs, (int32_t)K, v.row, v.pitch, pos_old - K + 2, hist0, hist1);
  HIPCHK(hipGetLastError());
  return 0;
}

int f16env_step_window_waves_per_simd(f16env_t h) { return h ? h->win_occ : 0; }
int f16env_step_window_nt(f16env_t h) { return h ? h->win_nt : -1; }

int f16env_step_rollout(f16env_t h, void* stream, const f16env_rollout_slot* slot, const float* act,
                        const float* obs_prev, float* obs, float* rew, uint8_t* terminated, uint8_t* truncated,
                        float* terminal_obs, double* ep_return, int32_t* ep_len, int32_t* done_idx,
                        int32_t* n_done) {
  if (!slot) return set_err(-1, "null rollout slot");
  return step_impl(h, stream, slot, act, obs_prev, obs, rew, terminated, truncated, terminal_obs, ep_return,
                   ep_len, done_idx, n_done);
}

int f16env_nonfinite_count(f16env_t h, void* stream, uint64_t* count) {
  if (!h || !count) return set_err(-1, "null argument");
  unsigned long long v = 0;
  HIPCHK(hipMemcpyAsync(&v, h->nonfinite, sizeof v, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  *count = (uint64_t)v;
  return 0;
}

int f16env_debug_checks(f16env_t h, void* stream, uint32_t* violations) {
  if (!h || !violations) return set_err(-1, "null argument");
#ifdef F16_DEBUG_CHECKS
  unsigned int v = 0;
  HIPCHK(hipMemcpyFromSymbolAsync(&v, HIP_SYMBOL(g_f16_violations), sizeof v, 0, hipMemcpyDeviceToHost,
                                  (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  *violations = v;
  return 1;
#else
  (void)stream;
  *violations = 0;
  return 0;
#endif
}

int f16env_obs_bounds_count(f16env_t h, void* stream, uint64_t* count) {
  if (!h || !count) return set_err(-1, "null argument");
  unsigned long long v = 0;
  HIPCHK(hipMemcpyAsync(&v, h->nonfinite + 2, sizeof v, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  *count = (uint64_t)v;
  return 0;
}

// persistent rollout launch shared by the contiguous and windowed entry points: from the
// observation `in` to the observation `out` (and the same frames of `out_other`, a window's
// second history, when not NULL)
static int rollout_launch(f16env_t h, hipStream_t st, RollArgs& a, const FrameView& in, const FrameView& out,
                          float* out_other) {
  a.obs_prev = in.first(); a.in_row = in.row; a.in_pitch = in.pitch;
  a.out0 = out.first(); a.out1 = out_other ? out_other + out.off : nullptr;
  a.out_row = out.row; a.out_pitch = out.pitch; a.out_slot = out.slot;
  if (a.T < 1) return set_err(-1, "T must be >= 1");
  if (!a.frames || !a.actions || !a.rewards || !a.last_start || (a.T > 1 && !a.next_start))
    return set_err(-1, "frames/actions/rewards/last_start (and next_start for T > 1) are required");
  if (((uintptr_t)a.actions & 15) != 0) return set_err(-1, "actions must be 16-byte aligned");
  if (h->cfg.flags & F16_FLAG_NO_AUTORESET) return set_err(-1, "rollout_random needs auto-reset");
  a.s = h->soa; a.tmpl = h->tmpl; a.nonfinite = h->nonfinite;
  a.E = env_args(h);
  a.C = h->C;
  a.icc.c = nullptr; a.icc.n = a.E.n;
  if (h->mode) {  // cfg5 modes: every lane's next reset cached before the launch (its first reset in it)
    if (int e = icc_prepare(h, st, true)) return e;
    a.icc = h->icc;
    h->icc_steps = 0;  // the rollout consumed rows: the next windowed step refills
  }
  // two waves per SIMD when there are more waves than SIMDs (the 256-register build)
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus <= 0) cus = 256;
  int occ = ((int64_t)a.E.n + 63) / 64 > 4 * (int64_t)cus ? 2 : 1;
  occ = env_int("F16ENV_ROLL_OCC", occ) == 2 ? 2 : 1;
  hipLaunchKernelGGL(rollout_kernel_for(h->mode, occ), dim3(nblocks(a.E.n)), dim3(BLOCK), 0, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

int f16env_rollout_random(f16env_t h, void* stream, uint64_t seed, uint64_t step0, int32_t T, const float* obs_prev,
                          float* obs, float* frames, float* actions, float* rewards, float* next_start,
                          float* last_start) {
  if (!h) return set_err(-1, "null handle");
  if (!obs_prev || !obs) return set_err(-1, "obs_prev/obs are required");
  RollArgs a;
  memset(&a, 0, sizeof a);
  a.frames = frames; a.actions = actions; a.rewards = rewards; a.next_start = next_start; a.last_start = last_start;
  a.seed = seed; a.step0 = step0; a.T = T;
  a.clear_fresh = 0;
  // (obs_prev is only read)
  return rollout_launch(h, (hipStream_t)stream, a, contiguous_view(h, const_cast<float*>(obs_prev)),
                        contiguous_view(h, obs), nullptr);
}

int f16env_window_rollout_random(f16env_t h, void* stream, uint64_t seed, uint64_t step0, int32_t T, int32_t parity,
                                 int32_t pos, int32_t pos_out, float* frames, float* actions, float* rewards,
                                 float* next_start, float* last_start) {
  if (!h) return set_err(-1, "null handle");
  if (!h->wb.hist[0]) return set_err(-1, "f16env_window_bind first");
  const int K = h->cfg.stack_k;
  const int64_t Th = h->wb.T;
  if (pos < K - 1 || pos >= Th || pos_out < K - 1 || pos_out >= Th)
    return set_err(-1, "window positions must be in [K-1, T-1]");
  if (pos_out - K + 1 <= pos && pos - K + 1 <= pos_out)
    return set_err(-1, "the output window must not overlap the input window");
  RollArgs a;
  memset(&a, 0, sizeof a);
  a.frames = frames; a.actions = actions; a.rewards = rewards; a.next_start = next_start; a.last_start = last_start;
  a.seed = seed; a.step0 = step0; a.T = T;
  a.clear_fresh = 1;  // both histories hold the whole final window
  return rollout_launch(h, (hipStream_t)stream, a, window_view(h, h->wb.hist[parity & 1], Th, pos),
                        window_view(h, h->wb.hist[0], Th, pos_out), h->wb.hist[1]);
}

int f16env_bootstrap_timeouts(void* stream, int64_t n, float* rewards, const uint8_t* terminated,
                              const uint8_t* truncated, const float* terminal_values, double gamma) {
  return bootstrap_timeouts_impl(stream, n, rewards, terminated, truncated, terminal_values, gamma);
}

int f16env_bootstrap_stash(void* stream, int64_t n, int32_t K, const float* tobs, int64_t row_stride,
                           int64_t frame_stride, const uint8_t* terminated, const uint8_t* truncated,
                           int64_t flat_base, float* stash_obs, int64_t* stash_idx, int32_t* count,
                           int64_t capacity) {
  return bootstrap_stash_impl(stream, n, K, tobs, row_stride, frame_stride, terminated, truncated, flat_base, stash_obs,
                              stash_idx, count, capacity);
}

int f16env_bootstrap_apply(void* stream, int64_t m, float* rewards, const int64_t* idx, const float* values,
                           double gamma) {
  return bootstrap_apply_impl(stream, m, rewards, idx, values, gamma);
}

int f16env_abi_version(void) { return F16ENV_ABI_VERSION; }

int f16env_get_state(f16env_t h, void* stream, double* canon) {
  if (!h || !canon) return set_err(-1, "null argument");
  hipLaunchKernelGGL(f16_get_state_kernel, dim3(nblocks(h->soa.n)), dim3(BLOCK), 0, (hipStream_t)stream, h->soa, canon, h->C);
  HIPCHK(hipGetLastError());
  return 0;
}

int f16env_set_state(f16env_t h, void* stream, const double* canon) {
  if (!h || !canon) return set_err(-1, "null argument");
  hipStream_t st = (hipStream_t)stream;
  h->icc_steps = 0;  // episode counters may change: the next windowed step refills the reset cache
  return wind_probe(h, st, [&](int* wind_any) {
    hipLaunchKernelGGL(f16_set_state_kernel, dim3(nblocks(h->soa.n)), dim3(BLOCK), 0, st, h->soa, canon, h->C, wind_any);
  });
}

int f16env_window_clear_fresh(f16env_t h, void* stream) {
  if (!h) return set_err(-1, "null handle");
  hipLaunchKernelGGL(f16_clear_fresh_kernel, dim3(nblocks(h->soa.n)), dim3(BLOCK), 0, (hipStream_t)stream, h->soa);
  HIPCHK(hipGetLastError());
  return 0;
}

int f16env_trim(f16env_t h, void* stream, const double* ic_in, double* ic_out, double* residual_out) {
  if (!h || !ic_in || !ic_out) return set_err(-1, "null argument");
  hipLaunchKernelGGL(f16_trim_kernel, dim3(nblocks(h->soa.n)), dim3(BLOCK), 0, (hipStream_t)stream,
                     (int64_t)h->soa.n, ic_in, ic_out, residual_out, h->C);
  HIPCHK(hipGetLastError());
  return 0;
}

int f16env_sample_actions(f16env_t h, void* stream, uint64_t seed, uint64_t step, float* act) {
  if (!h || !act) return set_err(-1, "null argument");
  if (((uintptr_t)act & 15) != 0) return set_err(-1, "act must be 16-byte aligned");
  hipLaunchKernelGGL(f16_sample_actions_kernel, dim3(nblocks(h->soa.n)), dim3(BLOCK), 0, (hipStream_t)stream,
                     (int64_t)h->soa.n, (int64_t)h->cfg.env_id_base, seed, step, act);
  HIPCHK(hipGetLastError());
  return 0;
}

int f16env_sample_actions_steps(f16env_t h, void* stream, uint64_t seed, uint64_t step0, int32_t T, float* act) {
  if (!h || !act) return set_err(-1, "null argument");
  if (T <= 0) return set_err(-1, "T must be > 0");
  if (((uintptr_t)act & 15) != 0) return set_err(-1, "act must be 16-byte aligned");
  const int64_t total = (int64_t)T * h->soa.n;
  const int64_t per_block = (int64_t)BLOCK * SA_PER_LANE;
  const int64_t blocks = (total + per_block - 1) / per_block;
  if (blocks > 0x7fffffff) return set_err(-1, "T x N too large");
  hipLaunchKernelGGL(f16_sample_actions_steps_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream,
                     (int64_t)h->soa.n, total, (int64_t)h->cfg.env_id_base, seed, step0, act);
  HIPCHK(hipGetLastError());
  return 0;
}

int f16env_window_resets_deferred(f16env_t h) {
  if (!h) return set_err(-1, "null handle");
  // cfg5 modes with F16ENV_ICC_PERIOD=0: finished lanes are reset by f16_reset_done_kernel after
  // the step kernel
  return reset_mode(h, true) == RESET_DEFERRED ? 1 : 0;
}

int f16env_gae(void* stream, int64_t n_steps, int64_t n_envs, const float* rewards, const float* values,
               const float* episode_starts, const float* last_values, const uint8_t* dones, double gamma,
               double gae_lambda, float* advantages, float* returns) {
  return gae_impl(stream, n_steps, n_envs, rewards, values, episode_starts, last_values, dones, gamma, gae_lambda,
                  advantages, returns);
}

int f16env_rollout_minibatch(void* stream, const F16RolloutView* view, int64_t batch, const int64_t* indices,
                             float* obs, float* actions, float* old_values, float* old_log_probs,
                             float* advantages, float* returns) {
  return rollout_minibatch_impl(stream, view, batch, indices, obs, actions, old_values, old_log_probs, advantages,
                                returns);
}

int f16env_policy_blob_layout(const f16_policy_desc* desc, int64_t* offsets_out, int64_t* n_floats_out) {
  if (const char* m = policy_desc_error(desc)) return set_err(-1, m);
  if (!offsets_out || !n_floats_out) return set_err(-1, "null argument");
  *n_floats_out = policy_layout(desc, offsets_out, nullptr);
  return 0;
}

int f16env_policy_forward(void* stream, const f16_policy_desc* desc, const float* blob, int64_t n, const float* obs,
                          int64_t row_stride, int64_t frame_stride, uint64_t seed, uint64_t step, int64_t id_base,
                          const float* eps, float* actions, float* values, float* log_probs, uint32_t flags) {
  return policy_forward_impl(stream, desc, blob, n, obs, row_stride, frame_stride, seed, step, id_base, eps, actions,
                             values, log_probs, flags);
}

int f16env_policy_backward_workspace(const f16_policy_desc* desc, int64_t n, int32_t max_blocks, int64_t* bytes_out) {
  return policy_backward_workspace_impl(desc, n, max_blocks, bytes_out);
}

int f16env_policy_backward(void* stream, const f16_policy_desc* desc, const float* blob, int64_t n, const float* obs,
                           int64_t row_stride, int64_t frame_stride, const float* d_mean, const float* d_values,
                           void* workspace, int64_t workspace_bytes, int32_t max_blocks, float* grad_blob) {
  return policy_backward_impl(stream, desc, blob, n, obs, row_stride, frame_stride, d_mean, d_values, workspace,
                              workspace_bytes, max_blocks, grad_blob);
}

int f16env_policy_lma_blob_layout(const f16_policy_desc* desc, const int32_t* lma, int64_t* offsets_out,
                                  int64_t* n_floats_out) {
  const f16_lma_desc* m = reinterpret_cast<const f16_lma_desc*>(lma);
  if (const char* e = policy_desc_error(desc)) return set_err(-1, e);
  if (const char* e = lma_desc_error(desc, m)) return set_err(-1, e);
  if (!offsets_out || !n_floats_out) return set_err(-1, "null argument");
  *n_floats_out = lma_layout(desc, m, offsets_out, nullptr);
  return 0;
}

int f16env_policy_lma_forward(void* stream, const f16_policy_desc* desc, const int32_t* lma, const float* blob, int64_t n,
                              const float* obs, int64_t row_stride, int64_t frame_stride, uint64_t seed, uint64_t step,
                              int64_t id_base, const float* eps, float* actions, float* values, float* log_probs,
                              float* features_out, uint32_t flags) {
  return policy_lma_forward_impl(stream, desc, reinterpret_cast<const f16_lma_desc*>(lma), blob, n, obs, row_stride,
                                 frame_stride, seed, step, id_base, eps, actions, values, log_probs, features_out, flags);
}

int f16env_policy_lma_backward_workspace(const f16_policy_desc* desc, const int32_t* lma, int64_t n, int32_t max_blocks,
                                         int64_t* bytes_out) {
  return policy_lma_backward_workspace_impl(desc, reinterpret_cast<const f16_lma_desc*>(lma), n, max_blocks, bytes_out);
}

int f16env_policy_lma_backward(void* stream, const f16_policy_desc* desc, const int32_t* lma, const float* blob, int64_t n,
                               const float* obs, int64_t row_stride, int64_t frame_stride, const float* d_mean,
                               const float* d_values, void* workspace, int64_t workspace_bytes, int32_t max_blocks,
                               float* grad_blob) {
  return policy_lma_backward_impl(stream, desc, reinterpret_cast<const f16_lma_desc*>(lma), blob, n, obs, row_stride,
                                  frame_stride, d_mean, d_values, workspace, workspace_bytes, max_blocks, grad_blob);
}

int f16env_ppo_workspace(int64_t n, int32_t max_blocks, int64_t* bytes_out) {
  return ppo_workspace_impl(n, max_blocks, bytes_out);
}

int f16env_ppo_head_blocks(int64_t n, int32_t max_blocks, int32_t* blocks_out) {
  return ppo_head_blocks_impl(n, max_blocks, blocks_out);
}

int f16env_ppo_loss_head(void* stream, int64_t n, const float* mean, const float* values, const float* actions,
                         const float* old_log_prob, const float* advantages, const float* target_values,
                         const float* log_std, const float* hyper, uint32_t flags, int32_t max_blocks, void* workspace,
                         int64_t workspace_bytes, float* d_mean, float* d_values) {
  return ppo_loss_head_impl(stream, n, mean, values, actions, old_log_prob, advantages, target_values, log_std, hyper,
                            flags, max_blocks, workspace, workspace_bytes, d_mean, d_values);
}

int f16env_ppo_adam_step(void* stream, int64_t n_floats, float* blob, float* grad_blob, float* exp_avg,
                         float* exp_avg_sq, int32_t* step, const float* hyper, int64_t log_std_offset,
                         const void* head_workspace, int32_t head_blocks, float* stats) {
  return ppo_adam_step_impl(stream, n_floats, blob, grad_blob, exp_avg, exp_avg_sq, step, hyper, log_std_offset,
                            head_workspace, head_blocks, stats);
}

int f16env_ppo_dynago_workspace(int64_t n, int32_t max_blocks, int64_t* bytes_out) {
  return ppo_dynago_workspace_impl(n, max_blocks, bytes_out);
}

int f16env_ppo_dynago_update(void* stream, int64_t n, const float* advantages, const float* dynago, float* state,
                             int32_t max_blocks, void* workspace, int64_t workspace_bytes) {
  return ppo_dynago_update_impl(stream, n, advantages, dynago, state, max_blocks, workspace, workspace_bytes);
}

int f16env_ppo_loss_head_am(void* stream, int64_t n, const float* mean, const float* values, const float* actions,
                            const float* old_log_prob, const float* advantages, const float* old_values,
                            const float* log_std, const float* hyper, const float* dynago, const float* state,
                            uint32_t flags, int32_t max_blocks, void* workspace, int64_t workspace_bytes, float* d_mean,
                            float* d_values, float* am_stats) {
  return ppo_loss_head_am_impl(stream, n, mean, values, actions, old_log_prob, advantages, old_values, log_std, hyper,
                               dynago, state, flags, max_blocks, workspace, workspace_bytes, d_mean, d_values, am_stats);
}

int f16env_ppo_dag_step(void* stream, int64_t n_floats, float* blob, float* grad_blob, const float* hyper,
                        const float* dag, const int32_t* segments, int32_t n_segments, float* seg_state,
                        double* dag_state, int32_t* dag_counters, uint32_t flags, int64_t log_std_offset,
                        const void* head_workspace, int32_t head_blocks, float* stats) {
  return ppo_dag_step_impl(stream, n_floats, blob, grad_blob, hyper, dag, segments, n_segments, seg_state, dag_state,
                           dag_counters, flags, log_std_offset, head_workspace, head_blocks, stats);
}

int f16env_features(void* stream, int64_t n_frames, const float* obs, float* feat) {
  return features_impl(stream, n_frames, obs, feat);
}

int f16env_features_strided(void* stream, int64_t n_rows, int32_t K, const float* obs, int64_t row_stride,
                            int64_t frame_stride, float* feat) {
  return features_strided_impl(stream, n_rows, K, obs, row_stride, frame_stride, feat);
}

int f16env_features_window_step(void* stream, int64_t n, int32_t K, int32_t pos, const float* hist_cur,
                                int64_t pos_stride, int64_t env_stride, float* feat_cur, float* feat_other,
                                const uint8_t* terminated, const uint8_t* truncated, int32_t autoreset,
                                int32_t transform) {
  return features_window_step_impl(stream, n, K, pos, hist_cur, pos_stride, env_stride, feat_cur, feat_other,
                                   terminated, truncated, autoreset, transform);
}

int f16env_poses(void* stream, int64_t n, const float* frames, int64_t frame_stride, float* out) {
  return poses_impl(stream, n, frames, frame_stride, out);
}

// The step kernel instance a handle launches in its observation layout: the windowed one once
// f16env_window_bind has been called, else the contiguous one (step_kernel_for's table).
const char* f16env_step_kernel_name(f16env_t h) {
  static thread_local char buf[64];
  if (!h) return "";
  if (h->wb.hist[0]) {
    // (as rocprofv3 demangles it: the plain step, not the rollout-slot build <.., true>)
    snprintf(buf, sizeof buf, "f16_step_win%s_kernel<%d, %d, false>", h->win_nt ? "_nt" : "", h->mode & 3, h->win_occ);
  } else if (h->gt) {
    snprintf(buf, sizeof buf, "f16_step_gt_kernel<%d, false>", h->mode & 3);  // as rocprofv3 demangles it
  } else if ((h->mode & 3) == 0 && h->occ == 1) {
    snprintf(buf, sizeof buf, "f16_step_kernel");
  } else {
    snprintf(buf, sizeof buf, "f16_step_var_kernel<%d, %d, false>", h->mode & 3, h->occ);
  }
  return buf;
}
int f16env_step_waves_per_simd(f16env_t h) { return h ? h->occ : 0; }
int f16env_step_mode(f16env_t h) { return h ? h->mode : -1; }
int f16env_step_variant(f16env_t h) { return h ? (h->gt ? 2 : (h->occ == 2 ? 1 : 0)) : -1; }

double f16env_algorithmic_bytes_per_env_step(int stack_k) {
  return 16.0 + 60.0 * stack_k + 60.0 * (stack_k - 1) + 4.0 + 2.0 + 2.0 * STATE_BYTES;
}

const char* f16env_last_error(void) { return g_err.c_str(); }

#ifdef F16_STAMPS
// diagnostic build only: copy per-wave section cycle totals (waves x ST_N u64) to host
int f16env_diag_stamps(unsigned long long* host, int max_waves) {
  const int n = max_waves < (1 << 14) ? max_waves : (1 << 14);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * ST_N * n, 0,
                             hipMemcpyDeviceToHost));
  return ST_N;
}
#endif

}  // extern "C"
