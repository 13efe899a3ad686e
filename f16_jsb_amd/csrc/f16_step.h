// f16_step.h -- the step kernel: one VecEnv step of N envs in one launch. StepArgs and StepPre (the
// kernel arguments), the window and epilogue helpers, step_body, its six __global__ wrappers
// (f16_step_kernel, _var, _gt, _win, _win_nt, _winx: 88 instances) and the tables that pick an
// instance (step_kernel_for, step_win_kernel_for, step_winx_kernel_for), with the LDS sizes the
// host needs to launch them (FRAME_PITCH, WIN_DYN_LDS). Device code and those tables only: the
// launch itself takes the handle and is in f16env.hip.
// Needs f16_device.h (the flight model), f16_env_layer.h (frame, reward, resets), f16_rng.h
// (actions, gusts), f16_stage.h (BLOCK, LDS-DMA, tables) and f16_features.h (the epilogue's
// feature window and pose export).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/f16env.h"
#include "f16_device.h"
#include "f16_env_layer.h"
#include "f16_features.h"
#include "f16_rng.h"
#include "f16_stage.h"

using namespace f16;

#define FRAME_PITCH 16
// The previous stack block lands in the wave's LDS image IMG_OFF floats past its 16-byte
// aligned base. IMG_OFF = 1 makes the shifted copy-out out[j] = img[IMG_OFF + j + 15] whole
// aligned float4s (ds_read_b128 instead of four dwords), but the misaligned LDS-DMA landing
// costs more than it saves (measured 23.0 vs 23.3 us per step at 65 536 envs, K = 4; 31.2 vs
// 32.3 at K = 10: profiles/r01_variants_w.json), so the image stays aligned.
#ifndef IMG_OFF
#define IMG_OFF 0
#endif
// loads in flight per lane and chunk of the large-K fallback's flat copy (step_body)
#ifndef F16_FALLBACK_CH
#define F16_FALLBACK_CH 16
#endif

struct StepArgs {
  SoA s, tmpl;
  const float* act;
  const float* obs_prev;
  float* obs;
  float* rew;
  uint8_t* term;
  uint8_t* trunc;
  float* tobs;
  double* ep_ret;
  int32_t* ep_len;
  int32_t* done_idx;
  int32_t* n_done;
  unsigned long long* nonfinite;  // F16_FLAG_NAN_GUARD quarantine count (handle-owned); [2]:
                                  // F16_FLAG_OBS_CHECK out-of-bounds lane-steps
  int32_t lds_image;
  // rollout slot (f16env_step_rollout; all NULL / 0 for f16env_step)
  int32_t sample_act;          // act == NULL: draw the actions in-kernel (seed, step)
  int32_t clip_act;            // F16_SLOT_CLIP: the env steps np.clip(act, low, high), r_act keeps act
  uint64_t act_seed, act_step;
  float* r_frame;              // N x 15: newest frame of obs_prev (contiguous layout)
  float* r_next_frame;         // N x 15: newest frame of the returned obs (windowed layout)
  float* r_act;                // N x 4: the actions (as given: unclipped)
  float* r_rew;                // N: rewards
  float* r_next_start;         // N: done as 0/1 float (episode_starts of the next slot)
  // windowed observations (f16env_step_window): the frame histories of this step (wx, the one
  // whose window is the returned observation) and of the other parity (wy), [T][N][16] each
  // (position-major: the N slots of one position are contiguous)
  float* wx;
  float* wy;
  int64_t wrow;                // floats between positions (position-major: N * 16; env-major: 16)
  int64_t wenv;                // floats between envs (position-major: 16; env-major: T * 16)
  int32_t wpos;                // newest frame position p (window = p-K+1 .. p)
  // the feature window in the rollout-slot build (F16_SLOT_FEATURE_WINDOW): the feature
  // histories [T][N][17] of this step's parity (fwx) and the other (fwy); nullptr: none
  float* fwx;
  float* fwy;
  // cfg5 modes, windowed layout: the reset cache (f16_ic_fill_kernel): per lane the state and
  // frame 0 (without the goal) of its NEXT reset, ICC_COLS columns; c == nullptr: deferred
  // resets by f16_reset_done_kernel instead
  SoA icc;
  EnvArgs E;
  ModelConsts C;
  // the plain step's pose export (f16env_window_step_ex with F16_STEP_POSES): N x 10 floats, the
  // pose of the returned observation's newest frame per env; nullptr: none
  float* poses;
};

#ifdef F16_STAMPS
__device__ unsigned long long g_stamps[1 << 14][ST_N];  // per wave (diagnostic build)
#endif


// Dynamic LDS: image mode holds, per wave, the previous stack block of its 64 rows
// (64*KC floats) + one spare frame; fallback mode holds the final/reset frames per lane.
__device__ __forceinline__ size_t image_floats_per_wave(int KC) { return (size_t)64 * KC + 16; }

// MODE bit 0: F16_FLAG_RANDOM_IC, bit 1: F16_FLAG_GUSTS. MODE 0 (the reference's task) resets
// finished lanes inline from the IC template; other modes leave finished lanes to
// f16_reset_done_kernel (a full RunIC per lane is too long to run divergently in-wave).
// GT: tables read from the global blob (L1/L2-resident, 12 KB) instead of an LDS copy, which
// frees the LDS for the stack image at large K (K = 10: four 38.5 KB images + the blob exceed
// 160 KB). sT is then unused.
// Windowed observations (WIN, f16env_step_window): two frame histories [T][N][16] (wx: this
// step's parity, wy: the other; position-major 16-float = 64-B frame slots, the 16th float 0),
// the observation of a step being the view wx[p-K+1 .. p][k][0..15) (strides 16, N*16, 1). A step
// writes its new frame at position p of BOTH histories -- no stack shift copy, no
// previous-stack read -- as four aligned 16-B stores filling one whole 64-B sector (a 60-B
// frame at a 60-B pitch leaves partial sectors, which cost as much as the whole-row rewrite
// they replace: 22.6 vs 18.5 us per step at 65 536 envs, K = 4, gpurun r02n). Lanes reset right
// before this step (FRESH) fill wx[p-K+1 .. p-1] with their reset frame (LDS-DMA'd from
// wy[p-1], which that reset wrote); lanes reset by this step fill wx[p-K+1 .. p] with the new
// reset frame and keep their final frame in wy[p], so wy's window IS the terminal observation
// (no copy). The other parity's window is untouched by a step, so an observation stays valid
// until the step after next, as with the ping-pong buffers of f16env_step.
static constexpr int WPITCH = 16;  // floats per history frame slot
template <bool NT = false>
__device__ __forceinline__ void put_slot(float* d, const float* f) {
  float4* q = reinterpret_cast<float4*>(d);
  st16<NT>(q, make_float4(f[0], f[1], f[2], f[3]));
  st16<NT>(q + 1, make_float4(f[4], f[5], f[6], f[7]));
  st16<NT>(q + 2, make_float4(f[8], f[9], f[10], f[11]));
  st16<NT>(q + 3, make_float4(f[12], f[13], f[14], 0.0f));
}
static constexpr int WFRESH = 16 * 64;  // LDS floats per wave for the fresh-frame DMA ([4][64] float4)
static constexpr int WSTASH = 16 * 64;  // ... and for the env-field stash of the 256-register builds
static constexpr int WIN_WAVE_FLOATS = WFRESH + WSTASH;

// ------------------------------------------------------------------------------------------
// Pieces of step_body's epilogue (what a wave writes after its reward and state stores). `stg` is
// the wave's LDS staging area (WIN_WAVE_FLOATS), `img` its stack image.
// Only what leaves every kernel's instruction stream as it was stands here (tools/isa_diff.py
// against the in-line form). The three layout arms themselves -- window, LDS image, large-K
// fallback -- and the feature window stay in line in step_body: a function is simplified on its
// own before it is inlined, and one that reads the lane's frames (f, f0: registers in step_body,
// memory behind a pointer argument) or computes under `if (live)` came out as other code in every
// kernel that carries it, the headline instances included.
// ------------------------------------------------------------------------------------------
// A lane's frame slot into the staging area, transposed for the wave's slot stores: quarter j
// of slot r at float4 r*4 + (j ^ (r>>2 & 3)), conflict-free on both the per-lane writes here and
// the per-slot reads
__device__ __forceinline__ void stage_slot(float4* st4, int lane, int sw, const float* fr) {
  st4[lane * 4 + (0 ^ sw)] = make_float4(fr[0], fr[1], fr[2], fr[3]);
  st4[lane * 4 + (1 ^ sw)] = make_float4(fr[4], fr[5], fr[6], fr[7]);
  st4[lane * 4 + (2 ^ sw)] = make_float4(fr[8], fr[9], fr[10], fr[11]);
  st4[lane * 4 + (3 ^ sw)] = make_float4(fr[12], fr[13], fr[14], 0.0f);
}
// A full wave's 64 rows of PITCH floats leave through its staging area (free after the frame
// stores) as one contiguous block. Each lane writes its row at a PITCH-float pitch (the frames'
// 15 and the features' 17 are odd: conflict-free) ...
template <int PITCH>
__device__ __forceinline__ void wave_rows_stage(float* stg, int lane, const float* vals) {
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < PITCH; ++j) stg[lane * PITCH + j] = vals[j];
  __builtin_amdgcn_wave_barrier();
}
// ... then 16 * PITCH float4 go out linearly to d0 (TWO: and d1, from the same LDS read); a
// destination whose rows are not 16-B aligned (N % 4 != 0) takes dword stores
template <int PITCH, bool TWO = false>
__device__ __forceinline__ void wave_rows_out(const float* stg, int lane, float* d0, float* d1 = nullptr) {
  const uintptr_t both = TWO ? (((uintptr_t)d0) | ((uintptr_t)d1)) : (uintptr_t)d0;
  if ((both & 15) == 0) {
    for (int u = lane; u < 64 * PITCH / 4; u += 64) {
      const float4 v = reinterpret_cast<const float4*>(stg)[u];
      reinterpret_cast<float4*>(d0)[u] = v;
      if (TWO) reinterpret_cast<float4*>(d1)[u] = v;
    }
  } else {
    for (int u = lane; u < 64 * PITCH; u += 64) {
      d0[u] = stg[u];
      if (TWO) d1[u] = stg[u];
    }
  }
}

// Rollout slot frame, contiguous layout = the newest frame of obs_prev (what the policy acted
// on), for every lane of the wave (the windowed build writes the returned observation's newest
// frame instead: r_next_frame)
__device__ __forceinline__ void r_frame_out(const StepArgs& a, const float* img, bool image, int lane, int rows,
                                            int64_t row0, int64_t k, bool live, int KC, int HC) {
  if (image) {
    __builtin_amdgcn_wave_barrier();
    float* dst = a.r_frame + row0 * F16_OBS_DIM;
    if (rows == 64) {  // 960 floats = 240 float4, 16-B aligned (row0 is a multiple of 64)
      for (int q = lane; q < 64 * F16_OBS_DIM / 4; q += 64) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = 4 * q + i, r = j / F16_OBS_DIM, c = j - r * F16_OBS_DIM;
          v[i] = img[IMG_OFF + r * KC + HC + c];
        }
        reinterpret_cast<float4*>(dst)[q] = make_float4(v[0], v[1], v[2], v[3]);
      }
    } else {
      for (int j = lane; j < rows * F16_OBS_DIM; j += 64) {
        const int r = j / F16_OBS_DIM, c = j - r * F16_OBS_DIM;
        dst[j] = img[IMG_OFF + r * KC + HC + c];
      }
    }
    __builtin_amdgcn_wave_barrier();
  } else if (live) {
#pragma unroll
    for (int c = 0; c < F16_OBS_DIM; ++c) a.r_frame[k * F16_OBS_DIM + c] = a.obs_prev[k * KC + HC + c];
  }
}

// The pose export (F16_STEP_POSES, f16_poses_kernel's output written here instead of by a
// second launch): po, the pose of the returned observation's newest frame (computed by the
// caller by f16_features.h's pose_of_frame); the wave's 64 rows are 640 contiguous floats
__device__ __forceinline__ void pose_epilogue(const StepArgs& a, float* stg, int lane, int rows, int64_t row0,
                                              int64_t k, bool live, const float* po) {
  if (rows == 64) {
    wave_rows_stage<10>(stg, lane, po);
    wave_rows_out<10>(stg, lane, a.poses + row0 * 10);
    __builtin_amdgcn_wave_barrier();
  } else if (live) {
#pragma unroll
    for (int j = 0; j < 10; ++j) a.poses[k * 10 + j] = po[j];
  }
}

// The prologue's first loads from kernel arguments preloaded into SGPRs (StepPre, windowed
// kernels): the state, action and template addresses and N are in registers when the wave
// starts, so the state / action loads and the table and template DMA issue without first
// waiting for the scalar load of the argument block (-amdgpu-kernarg-preload-count, build.py).
struct StepPre {
  const float4* sc;
  const float* act;
  const float4* tmpl;
  int64_t n;
};
// XV (windowed plain-step extras, f16_step_winx_kernel / f16env_window_step_ex): XV_FEAT keeps the
// bound feature histories in the step's epilogue (the rollout-slot build's F16_SLOT_FEATURE_WINDOW
// code, without the slot); every winx build draws the actions in-kernel when act == NULL
// (a.sample_act: the f16env_sample_actions stream) and writes the pose export when a.poses is set
// (F16_STEP_POSES, a run-time choice: no further instances). The headline instances (XV = 0)
// carry none of this code.
enum { XV_X = 1, XV_FEAT = 2 };
template <int MODE, bool GT = false, bool ROLL = false, bool LOWREG = false, bool WIN = false, bool NT = false,
          int XV = 0>
__device__ __forceinline__ void step_body(const StepArgs& a, float* sT_lds, float4* sTmpl, int* sDone, float* dynl,
                                          const StepPre* pre = nullptr) {
  const float* sT = GT ? static_cast<const float*>(F16_BLOB_INIT) : sT_lds;
  constexpr bool GUST = (MODE & 2) != 0, DEFER = MODE != 0;
  // builds that may draw the actions in-kernel (act == NULL): the rollout slot's and the winx
  constexpr bool SAMPLE = ROLL || (XV & XV_X) != 0;
  constexpr bool FEATW = ROLL || (XV & XV_FEAT) != 0;  // builds with the feature-window epilogue
#ifdef F16_STAMPS
  Stamps stamps = {};
  stamps.last = memtime();
#endif
  const int KC = a.E.K * F16_OBS_DIM, HC = (a.E.K - 1) * F16_OBS_DIM;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row0 = (int64_t)blockIdx.x * BLOCK + wave * 64;
  const int64_t nE = pre ? pre->n : a.E.n;
  const int rows = (int)(nE - row0 < 64 ? (nE - row0 > 0 ? nE - row0 : 0) : 64);
  // The prologue's form. Counted waits (below) for every build but those that may draw the action
  // in-kernel (the rollout slot's and the winx): their in-kernel-action row lost 0.05-0.15 us on
  // the same-box A/B (profiles/r07_ab_counted_waits.json), so they keep the single wait.
#ifdef F16_PROLOGUE_ONE_WAIT  // (the form before the counted waits, for the same-box A/B)
  constexpr bool ONE_WAIT = true;
#else
  constexpr bool ONE_WAIT = ROLL || (XV & XV_X) != 0;
#endif
  // (the windowed step keeps no stack image: its launcher sets lds_image = 0. The counted-wait
  // builds say so at compile time -- any vector-memory operation on a path between the
  // prologue's loads and a column's first use, even a never-taken one, turns the compiler's
  // counted wait there into a full drain)
  const bool image = (ONE_WAIT || !WIN) && a.lds_image != 0;
  // cfg5 modes in the windowed layout reset finished lanes in the step (reset cache)
  const bool in_step_reset = WIN && DEFER && a.icc.c != nullptr && !(a.E.flags & F16_FLAG_NO_AUTORESET);
  constexpr bool STASH = LOWREG && WIN;
  float* img = dynl + (size_t)wave * image_floats_per_wave(KC);
  // 1) DMA of this wave's previous stack block into LDS (overlaps the physics)
  auto issue_stack_dma = [&]() {
    if (image && rows > 0) {
      const float* prev = a.obs_prev + row0 * KC;
      const int total = rows * KC;  // floats
      const int n16 = total >> 2;   // whole 16-byte pieces (wave blocks are 16-B aligned)
      for (int b = 0; b < n16; b += 64) {
        const int piece = b + lane;
        if (piece < n16) dma16(prev + 4 * piece, img + IMG_OFF + 4 * b);
      }
      if (lane < (total & 3)) dma4(prev + 4 * n16 + lane, img + IMG_OFF + 4 * n16);  // tail, never past the end
    }
  };
  const int64_t k = row0 + lane;
  const bool live = k < nE;
  F16_CHECK(rows >= 0 && rows <= 64 && (!live || row0 + lane < nE), DBG_STATE_INDEX);
  if (WIN) F16_CHECK(a.wpos >= a.E.K - 1 && a.wpos >= 0, DBG_WINDOW_POS);
  int done = 0;
  Lane L;
  float4 av = make_float4(0.f, 0.f, 0.f, 0.f);
  // the loads the physics needs are in flight at once (table DMA, IC template, state and
  // action), then one wait: a single HBM round trip before the physics. The previous stack
  // (only needed by the obs rebuild) is DMA'd after that wait, so it streams in while the
  // first frame runs instead of sharing the prologue's HBM bandwidth.
  if (!GT) stage_tables_issue(sT_lds);
  // IC template: the NCOL state columns, then its frame-0 columns (lane i lands at sTmpl[i])
  if (!DEFER && threadIdx.x < NCOL + TMPL_FRAME_COLS)
    dma16(reinterpret_cast<const float*>((pre ? pre->tmpl : a.tmpl.c) + (threadIdx.x < NCOL ? threadIdx.x : threadIdx.x + NCOL_ALL - NCOL)),
          reinterpret_cast<float*>(sTmpl));
  // (the columns are unpacked after the wait, behind a scheduling barrier: a first use the
  // scheduler hoists between the loads puts a vmcnt(0) there -- the table DMA and the first two
  // columns' round trip, then the other fourteen's. Unconditional loads -- a lane past the end
  // reading env 0 -- let the argument fetches issue before the wait too, but measured no faster
  // at 65 536 envs and 0.5 us slower for cfg5's two-wave kernel: profiles/r06_ab_prologue.json)
  float4 cl[NCOL], wl, gl;
  const bool load_act = !SAMPLE || !a.sample_act;
  constexpr bool C15_EARLY = GUST || STASH;  // builds that read C15 before the frames (FETCH_ORDER)
  if constexpr (ONE_WAIT) {
    if (live) {
      if (pre) {
        const SoA sp = {const_cast<float4*>(pre->sc), pre->n};
        lane_fetch<GUST>(sp, k, cl, wl, gl);
        if (load_act) av = reinterpret_cast<const float4*>(pre->act)[k];
      } else {
        lane_fetch<GUST>(a.s, k, cl, wl, gl);
        if (load_act) av = reinterpret_cast<const float4*>(a.act)[k];
      }
    }
    VM_DRAIN();
    __builtin_amdgcn_sched_barrier(0);
    if (live) lane_unpack<GUST>(cl, wl, gl, L);
    __syncthreads();
  } else {
    // Counted waits: the columns are issued in the order of their first use (FETCH_ORDER) and
    // nothing drains them here. Each first use waits with the compiler's own s_waitcnt vmcnt(k),
    // k the loads issued behind that column, so the Earth angle, the altitude reference, the
    // recomputed latch and the head of the first frame run while the late columns (FCS / engine
    // state, the action, C15) still arrive; C15 is first read by the env layer after the frames.
    // The loads are unconditional -- a lane past the end reads the last env's row and drops it --
    // so every wave issues the same number of them, which the counted wait below relies on, and
    // the loaded values reach their uses without a merge at the end of a branch (the optimiser
    // moves a merged value's first operation up into the branch, next to the loads, where it
    // waits for its column with every later load still to issue).
    {
      // (the addresses through an empty asm: the preloaded ones are __restrict__ kernel
      // arguments, and loads from such memory may be moved anywhere -- the compiler sank ten of
      // the columns below the barrier, behind a full drain for the first seven)
      float4* scp = pre ? const_cast<float4*>(pre->sc) : a.s.c;
      const float* actp = pre ? pre->act : a.act;
      asm volatile("" : "+s"(scp), "+s"(actp));
      // (... and back into the global address space, which the asm forgets: a generic pointer
      // loads with flat_load, which may hit LDS and so waits for the DMAs first)
      const GCol scg = (GCol)scp, actg = (GCol)actp;
      const int64_t kc = k < nE ? k : (nE > 0 ? nE - 1 : 0);
      lane_fetch_ordered<GUST, C15_EARLY, 0>(scg, pre ? pre->n : a.s.n, kc, cl, wl, gl);
      if (load_act) av = fetch_col(actg + kc);
      lane_fetch_ordered<GUST, C15_EARLY, 1>(scg, pre ? pre->n : a.s.n, kc, cl, wl, gl);
    }
    // (every load above is issued before any wait: the count below says how many were)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    // The barrier below publishes the table / template staging, so this wave's own LDS-DMAs must
    // have landed. They are the oldest entries: vmcnt(k), k no more than the number of loads
    // issued behind them, retires them and leaves the state columns in flight. k counts the 16
    // (18) columns and not the action: builds that may draw the action in-kernel issue its load
    // or not (a run-time choice, one count less again for them), and the one load more this
    // retires is the first column, C13, which the frame's first instructions read anyway. (One
    // unconditional wait: after a branch between two counts the compiler drains everything at
    // the barrier.)
    if (!GT || !DEFER) VM_WAIT(NCOL + (GUST ? 2 : 0) - (SAMPLE ? 1 : 0));
    __syncthreads();
    // (no first use hoisted between the wait and the barrier: the compiler's own wait for it
    // there came out as a full drain)
    __builtin_amdgcn_sched_barrier(0);
    // (every lane unpacks what it loaded, a lane past the end its copy of the last env's row:
    // under "if (live)" the unpacked values would merge with nothing at the branch's end, and the
    // copies that merge makes read every column there)
    lane_unpack<GUST, 1>(cl, wl, gl, L);
  }
  // (counted waits: the stack and fresh-frame DMAs go behind the first frame, below, for the
  // reason given at `image` above; they still stream in under the other frames)
  if constexpr (ONE_WAIT) issue_stack_dma();
  if (SAMPLE && a.sample_act && live) av = philox_action(a.act_seed, (uint64_t)(a.E.id_base + k), a.act_step);
  // a lane reset since the last step: the windowed step reads its reset frame (wy[p-1]) now,
  // so the load streams in behind the physics
  // (LDS-DMA into the wave's staging area, [15][64] floats, not registers: nothing stays live
  // across the frames; the vmcnt(0) after the frames retires it)
  double ce = 1.0, se = 0.0;
  AltRef A;
  if constexpr (!ONE_WAIT) {
    // the Earth angle and the exact geodetic altitude (once per env step) from the first columns,
    // ahead of the first read of C14 below (every lane, as the unpack)
    earth_angle(L.epa, ce, se);
    A = alt_ref(L, ce, se);
    __builtin_amdgcn_sched_barrier(0);
    lane_unpack<GUST, 2>(cl, wl, gl, L);
  }
  bool fresh = false;
  float* stg = dynl + (size_t)wave * WIN_WAVE_FLOATS;
  if constexpr (ONE_WAIT) {
    if (live) {
      fresh = (L.flags & LANE_FLAG_FRESH) != 0;
      L.flags &= ~LANE_FLAG_FRESH;
    }
  } else {  // (every lane, as the unpack: no merge at a branch's end)
    fresh = live && (L.flags & LANE_FLAG_FRESH) != 0;
    L.flags &= ~LANE_FLAG_FRESH;
  }
  const auto issue_fresh_dma = [&]() {
    if (WIN && fresh && a.E.K > 1) {
      const float* src = a.wy + k * a.wenv + (int64_t)(a.wpos - 1) * a.wrow;
#pragma unroll
      for (int j = 0; j < 4; ++j) dma16(src + 4 * j, stg + j * 256);  // [j][lane] float4
    }
  };
  if constexpr (ONE_WAIT) issue_fresh_dma();
  F16_STAMP(stamps, ST_LOAD);
  float f[F16_OBS_DIM], f0[F16_OBS_DIM];
  float rew_out = 0.0f;
  int flags_out = 0;
  float cmd[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float4* stash = reinterpret_cast<float4*>(stg + WFRESH);
  // the frames from s0 on, and what follows them in the 256-register windowed builds
  const auto rest_frames = [&](int s0) {
    for (int s = s0; s < a.E.down_sample; ++s)  // :225-232
      frame<LOWREG, GUST>(L, cmd, ce, se, A, sT, a.C, false F16_STAMP_PASS);
    if (STASH) {
      asm volatile("" ::: "memory");
      const float4 g = stash[lane], e = stash[64 + lane];
      L.goal[0] = g.x; L.goal[1] = g.y; L.goal[2] = g.z; L.last_d = g.w;
      L.step = __float_as_int(e.x); L.ep_count = __float_as_int(e.y); L.ep_ret = f2d(e.z, e.w);
      const float4 w = stash[128 + lane];
      L.epa = f2d(w.x, w.y);
      for (int s = 0; s < a.E.down_sample; ++s) L.epa += a.C.epa_dt;  // frame()'s per-frame advance
      if (GUST) {
        const float4 u = stash[192 + lane];
        L.gust[0] = w.z; L.gust[1] = w.w; L.gust[2] = u.x; L.wst[0] = u.y; L.wst[1] = u.z; L.wst[2] = u.w;
      }
    }
  };
  const int peeled = (!ONE_WAIT && a.E.down_sample > 0) ? 1 : 0;
  // what a step does ahead of its frames
  const auto pre_frames = [&]() {
    const float4 ac = (ROLL && a.clip_act) ? clip_box(av) : av;  // the env steps the clipped action
    cmd[0] = ac.x; cmd[1] = ac.y; cmd[2] = ac.z; cmd[3] = ac.w;
    L.step += 1;                                              // jsbsim_gym.py:215
    if (GUST) {  // cfg5 Gauss-Markov gust update, once per env step before the frames
      float xi[3];
      rng_normals(a.E.seed, (uint64_t)(a.E.id_base + k), (uint32_t)(L.ep_count - 1), (uint32_t)L.step, xi);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        L.gust[j] = __builtin_fmaf(a.E.gust_a, L.gust[j], a.E.gust_b * xi[j]);  // explicit: every build alike
        L.wind[j] = L.wst[j] + L.gust[j];
      }
    }
    if constexpr (ONE_WAIT) {
      earth_angle(L.epa, ce, se);
      A = alt_ref(L, ce, se);  // exact geodetic altitude once per env step
    }
    F16_STAMP(stamps, ST_ENVPRE);
    // 256-register windowed builds: the env fields the frames never read (goal, last distance,
    // step, episode count and return) wait in the wave's LDS stash instead of VGPRs, which the
    // frame loop needs (they were part of what spilled to scratch around it)
    if (STASH) {
      stash[lane] = make_float4(L.goal[0], L.goal[1], L.goal[2], L.last_d);
      stash[64 + lane] = make_float4(__int_as_float(L.step), __int_as_float(L.ep_count), dlo(L.ep_ret), dhi(L.ep_ret));
      // the Earth angle: the frames advance it by a constant each (replayed below, the same
      // fp64 adds) and otherwise read only its cos / sin; the gust model's pieces: the frames
      // read the wind sum only
      stash[128 + lane] = make_float4(dlo(L.epa), dhi(L.epa), GUST ? L.gust[0] : 0.0f, GUST ? L.gust[1] : 0.0f);
      if (GUST) stash[192 + lane] = make_float4(L.gust[2], L.wst[0], L.wst[1], L.wst[2]);
      asm volatile("" ::: "memory");
    }
  };
  if constexpr (ONE_WAIT) {
    if (live) {
      pre_frames();
      rest_frames(0);
    }
  } else {
    // Every lane runs the step's head and its first frame, a lane past the end on its copy of the
    // last env's row (dropped at the stores): entering a branch here, the register allocator
    // parks what the frames do not read (C15, parts of C12) in other registers at the branch's
    // head, and those copies wait for the last load. The first frame stands apart from the
    // loop: straight-line code behind the prologue, in which each late column's first use
    // carries its own counted wait (inside the loop the columns are loop-carried values, copied
    // -- and so waited for -- at its head). It unpacks the FCS / engine columns where the FCS
    // first reads them.
    pre_frames();
    const auto late = [&]() { lane_unpack<GUST, 3>(cl, wl, gl, L); };
    if (peeled)
      frame<LOWREG, GUST>(L, cmd, ce, se, A, sT, a.C, false F16_STAMP_PASS, late);
    else
      late();
    // (the stack DMA is the whole wave's, whatever its live lanes)
    if constexpr (!WIN) issue_stack_dma();
    if (live) {
      issue_fresh_dma();
      rest_frames(peeled);
    }
  }
  // Early state store, with no done list to compact (its atomic's return would wait for every
  // store before it): retire the stack DMA and store the state columns the frames left final
  // now, so their drain overlaps the observation frame, reward and obs writes instead of
  // adding to the tail. Two-waves-per-SIMD builds only (gpurun r02m, MODE 0: 131 072 envs
  // 30.35 -> 29.89 us, 262 144 62.35 -> 60.0 us). At one wave per SIMD: the contiguous build
  // gained nothing at 65 536 envs and lost 0.4 us at 4 096; the non-temporal windowed build
  // gained 0.35 us on fresh episodes but lost 0.3-0.4 us in the bench's steady state, where
  // a lane reset by the step stores its row twice (r02_variants_early_store.txt).
  const bool early_store = LOWREG && !a.done_idx;
  if (early_store) {
    VM_DRAIN();
    if (live) lane_store<GUST, 1, NT>(a.s, k, L);
  }
  if (live) {
    make_frame<!LOWREG>(L, ce, se, A, f);  // :234
    F16_STAMP(stamps, ST_FRAME_OBS);
    // reward / termination (:237-261), PositionReward (:493-507)
    float r32;
    flags_out = env_reward<!LOWREG>(L, f, a.E, r32);  // bit 0 terminated, 1 truncated, 2 quarantined
    F16_STAMP(stamps, ST_REWARD);
    done = flags_out & 3;
    rew_out = r32;
  }
  // the stack DMA issued after the prologue has long landed; retire it here, before any
  // store of this step (vmcnt also counts stores on CDNA, so a later wait would drain them)
  // -- unless the early state store above already did
  if (!early_store) VM_DRAIN();
  // compaction of finished lanes (wave64 ballot), before any store of this step so the
  // atomic's return waits on nothing else
  if (a.done_idx) {  // (always set in deferred modes: the handle's own list if the caller gave none)
    const unsigned long long m = __ballot(done);
    if (m) {
      int base = 0;
      if (lane == 0) base = atomicAdd(a.n_done, __popcll(m));
      base = __shfl(base, 0);
      F16_CHECK(base + __popcll(m) <= nE, DBG_DONE_LIST);
      if (done) a.done_idx[base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)k;
    }
  }
  if (a.E.flags & F16_FLAG_NAN_GUARD) {
    const unsigned long long qm = __ballot(flags_out & 4);
    if (qm && lane == 0) atomicAdd(a.nonfinite, (unsigned long long)__popcll(qm));
  }
  if (a.E.flags & F16_FLAG_OBS_CHECK) {  // jsbsim_gym.py:268-285 on the new frame
    const unsigned long long om = __ballot(live && obs_out_of_bounds(f));
    if (om && lane == 0) atomicAdd(a.nonfinite + 2, (unsigned long long)__popcll(om));
  }
  if (live) {
    a.rew[k] = rew_out;
    a.term[k] = (uint8_t)((flags_out & 1) | ((flags_out >> 1) & 2));
    a.trunc[k] = (uint8_t)((flags_out >> 1) & 1);
    if (ROLL) {
      if (a.r_rew) a.r_rew[k] = rew_out;
      if (a.r_act) reinterpret_cast<float4*>(a.r_act)[k] = av;
      if (a.r_next_start) a.r_next_start[k] = done ? 1.0f : 0.0f;
    }
    if (done) {
      if (a.ep_ret) a.ep_ret[k] = L.ep_ret;
      if (a.ep_len) a.ep_len[k] = L.step;
      if (!DEFER && !(a.E.flags & F16_FLAG_NO_AUTORESET)) {
        lane_reset_template(L, sTmpl, a.E, k, f0);
      } else if (in_step_reset) {
        // cfg5 modes, windowed layout: the lane's next reset from the cache when it holds that
        // episode's (tag: the cached row's episode count = this lane's + 1; a reset is a pure
        // function of (seed, env id, episode), so any row with that tag is the one), else the
        // full RunIC here (a lane that finished twice within one fill period)
        if (__float_as_int(a.icc.c[(int64_t)15 * a.icc.n + k].w) == L.ep_count + 1) {
          lane_load<GUST>(a.icc, k, L);
#pragma unroll
          for (int j = 0; j < TMPL_FRAME_COLS; ++j) {
            const float4 v = a.icc.c[(int64_t)(NCOL_ALL + j) * a.icc.n + k];
            f0[4 * j] = v.x; f0[4 * j + 1] = v.y; f0[4 * j + 2] = v.z; f0[4 * j + 3] = v.w;
          }
          f0[12] = L.goal[0]; f0[13] = L.goal[1]; f0[14] = L.goal[2];
        } else {
          lane_reset_mode<MODE, LOWREG>(L, a.E, k, sT, a.C, f0);
        }
      } else {
#pragma unroll
        for (int j = 0; j < F16_OBS_DIM; ++j) f0[j] = f[j];
      }
    }
    F16_STAMP(stamps, ST_RESET);
    // C15 (goal, episode count) changes only in a reset: written back for the lanes reset here
    const bool reset_here = done && (!DEFER || in_step_reset) && !(a.E.flags & F16_FLAG_NO_AUTORESET);
    if (!early_store || reset_here)
      lane_store<GUST, 0, NT>(a.s, k, L, reset_here);  // every column (a lane reset just now rewrites its row)
    else
      lane_store<GUST, 2, NT>(a.s, k, L, false);  // the rest
    F16_STAMP(stamps, ST_STORE);
  }
  sDone[threadIdx.x] = done;
  // deferred modes: f16_reset_done_kernel rewrites finished rows after this kernel, unless the
  // windowed step resets them itself (in_step_reset)
  const bool autoreset = (!DEFER || in_step_reset) && !(a.E.flags & F16_FLAG_NO_AUTORESET);
  // rollout slot frame (contiguous layout): the newest frame of obs_prev, for every lane
  if (ROLL && !WIN && a.r_frame && rows > 0) r_frame_out(a, img, image, lane, rows, row0, k, live, KC, HC);
  if (WIN) {
    const int K = a.E.K, p = a.wpos;
    const bool reset_now = live && done && autoreset;
    if (live && K > 1 && (fresh || reset_now)) {  // rare: whole-window fills of reset lanes
      float* X = a.wx + k * a.wenv;
      if (fresh) {
        float f0p[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 v = reinterpret_cast<const float4*>(stg)[j * 64 + lane];
          f0p[4 * j] = v.x; f0p[4 * j + 1] = v.y; f0p[4 * j + 2] = v.z; f0p[4 * j + 3] = v.w;
        }
        for (int r = p - K + 1; r < p; ++r) put_slot(X + (int64_t)r * a.wrow, f0p);
      }
      if (reset_now)  // after the fresh fill: a one-step episode ends in its own reset window
        for (int r = p - K + 1; r < p; ++r) put_slot(X + (int64_t)r * a.wrow, f0);
    }
    // this step's frame at position p of both histories (wx: the reset frame of a lane reset
    // now, else the new frame; wy: the new frame). The wave's 64 slots are one contiguous
    // 4 KiB block; the wave transposes them through its LDS staging area so that each dwordx4
    // store instruction writes 1 KiB contiguous (16 whole slots, 4 lanes per slot) instead of a
    // 16-B quarter of every slot (stage_slot's swizzle).
    // A wave none of whose lanes was reset now (~94 % of waves in the bench's steady state) has
    // the same 64 slots for both histories: one LDS staging pass, each transposed float4 read
    // once and stored twice (round 6; was two passes for every wave: 4 ds_write_b128 + 4
    // ds_read_b128 and two wave barriers per wave per step saved). The byte count is unchanged:
    // both histories must hold every frame for the (N, K, 15) strided view to alternate parity
    // (DESIGN.md 9 item 7).
    const bool one_pass = !ROLL && rows == 64 && __ballot(reset_now) == 0;
    if (one_pass) {
      float4* st4 = reinterpret_cast<float4*>(stg);
      const int q = lane & 3, sw = (lane >> 2) & 3;
      __builtin_amdgcn_wave_barrier();
      stage_slot(st4, lane, sw, f);
      __builtin_amdgcn_wave_barrier();
      const int64_t off = (int64_t)p * a.wrow + (row0 + (lane >> 2)) * a.wenv + 4 * q;
      float* const dx = a.wx + off;
      float* const dy = a.wy + off;
      float4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 16 * j + (lane >> 2);
        v[j] = st4[r * 4 + (q ^ ((r >> 2) & 3))];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) st16<NT>(reinterpret_cast<float4*>(dx + (int64_t)(16 * j) * a.wenv), v[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) st16<NT>(reinterpret_cast<float4*>(dy + (int64_t)(16 * j) * a.wenv), v[j]);
      __builtin_amdgcn_wave_barrier();
    } else if (rows == 64) {
      float4* st4 = reinterpret_cast<float4*>(stg);
      const int q = lane & 3, sw = (lane >> 2) & 3;
      float* const hist[2] = {a.wx, a.wy};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float* fr = (h == 0 && reset_now) ? f0 : f;
        __builtin_amdgcn_wave_barrier();
        stage_slot(st4, lane, sw, fr);
        __builtin_amdgcn_wave_barrier();
        float* dst = hist[h] + (int64_t)p * a.wrow + (row0 + (lane >> 2)) * a.wenv + 4 * q;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 16 * j + (lane >> 2);
          st16<NT>(reinterpret_cast<float4*>(dst + (int64_t)(16 * j) * a.wenv), st4[r * 4 + (q ^ ((r >> 2) & 3))]);
        }
        if (ROLL && h == 0 && a.r_next_frame) {
          // the rollout's frame log: the returned observation's newest frame (the next slot's
          // frame), the wave's 64 rows as 960 contiguous floats through the (now free) staging area
          wave_rows_stage<F16_OBS_DIM>(stg, lane, fr);
          wave_rows_out<F16_OBS_DIM>(stg, lane, a.r_next_frame + row0 * F16_OBS_DIM);
        }
      }
      __builtin_amdgcn_wave_barrier();
    } else if (live) {
      const int64_t off = k * a.wenv + (int64_t)p * a.wrow;
      put_slot<NT>(a.wx + off, reset_now ? f0 : f);
      put_slot<NT>(a.wy + off, f);
      if (ROLL && a.r_next_frame) {
        const float* fr = reset_now ? f0 : f;
#pragma unroll
        for (int c = 0; c < F16_OBS_DIM; ++c) a.r_next_frame[k * F16_OBS_DIM + c] = fr[c];
      }
    }
    if (FEATW && a.fwx) {
      // the feature window (f16_feature_window_kernel's invariant, written here instead of by a
      // second launch): fx[p] = fy[p] = features of wx[p]; a lane reset now also fills
      // fx[p-K+1 .. p-1] and, ahead of the next step's window fill, fy[p-K+2 .. p-1]. The
      // wave's 64 rows (64 * 17 contiguous floats per history) leave through its staging area
      // (free after the frame stores) as float4.
      const int64_t rowN = a.E.n * FEAT_OUT;
      float y[FEAT_OUT];
      if (live) frame_features(reset_now ? f0 : f, y);
      if (rows == 64) {
        wave_rows_stage<FEAT_OUT>(stg, lane, y);
        wave_rows_out<FEAT_OUT, true>(stg, lane, a.fwx + (int64_t)p * rowN + row0 * FEAT_OUT,
                                      a.fwy + (int64_t)p * rowN + row0 * FEAT_OUT);
        // the window fills of the wave's reset lanes (rare), each lane's (row, feature) pairs
        // spread over the whole wave from the staging area (as f16_feature_window_kernel)
        const uint64_t rm = __ballot(reset_now);
        if (rm && K > 1) {
          const int items = (2 * K - 3) * FEAT_OUT;  // fx rows p-K+1 .. p-1, fy rows p-K+2 .. p-1
          for (uint64_t m = rm; m; m &= m - 1) {
            const int ee = __builtin_ctzll(m);
            const int64_t kk = row0 + ee;
            for (int it = lane; it < items; it += 64) {
              const int ri = it / FEAT_OUT, j = it - ri * FEAT_OUT;
              float* d = ri < K - 1 ? a.fwx + (int64_t)(p - K + 1 + ri) * rowN
                                    : a.fwy + (int64_t)(p - K + 2 + (ri - (K - 1))) * rowN;
              d[kk * FEAT_OUT + j] = stg[ee * FEAT_OUT + j];
            }
          }
        }
        __builtin_amdgcn_wave_barrier();
      } else if (live) {
#pragma unroll
        for (int j = 0; j < FEAT_OUT; ++j) {
          a.fwx[(int64_t)p * rowN + k * FEAT_OUT + j] = y[j];
          a.fwy[(int64_t)p * rowN + k * FEAT_OUT + j] = y[j];
        }
      }
      if (rows != 64 && reset_now && K > 1) {  // a partial wave's reset lanes: one lane each
        for (int r = p - K + 1; r < p; ++r) {
#pragma unroll
          for (int j = 0; j < FEAT_OUT; ++j) {
            a.fwx[(int64_t)r * rowN + k * FEAT_OUT + j] = y[j];
            if (r > p - K + 1) a.fwy[(int64_t)r * rowN + k * FEAT_OUT + j] = y[j];
          }
        }
      }
    }
    if ((XV & XV_X) != 0 && a.poses) {
      float po[10];
      if (live) pose_of_frame(reset_now ? f0 : f, po);
      pose_epilogue(a, stg, lane, rows, row0, k, live, po);
    }
    F16_STAMP(stamps, ST_COPY);
  } else if (image) {
    // 2) splice the new frame of row r into the image at row r+1's first frame, which the
    //    shifted copy never reads: out_flat[j] = img[j + 15] for the whole block. The stack
    //    DMA landed at the prologue wait, and a wave only touches its own image, so the steps
    //    below need no workgroup barrier (a wave's LDS accesses complete in order).
    __builtin_amdgcn_wave_barrier();
    if (live) {
      float* dst = img + IMG_OFF + (size_t)(lane + 1) * KC;
#pragma unroll
      for (int j = 0; j < F16_OBS_DIM; ++j) dst[j] = f[j];
    }
    __builtin_amdgcn_wave_barrier();
    // 3) finished rows: terminal obs = the spliced row; then the row becomes K x frame 0
    if (live && done) {
      float* src = img + IMG_OFF + (size_t)lane * KC + F16_OBS_DIM;
      if (a.tobs) {
        float* t = a.tobs + k * KC;
        if ((KC & 3) == 0) {  // K % 4 == 0: the row is 16-B aligned in HBM, dwordx4 stores
          for (int c = 0; c < KC; c += 4)
            *reinterpret_cast<float4*>(t + c) = make_float4(src[c], src[c + 1], src[c + 2], src[c + 3]);
        } else {
          for (int c = 0; c < KC; ++c) t[c] = src[c];
        }
      }
      if (autoreset)  // frame by frame: f0 indexed by literals (no per-element modulo / select chain)
        for (int r = 0; r < a.E.K; ++r)
#pragma unroll
          for (int j = 0; j < F16_OBS_DIM; ++j) src[r * F16_OBS_DIM + j] = f0[j];
    }
    __builtin_amdgcn_wave_barrier();
    F16_STAMP(stamps, ST_SYNC);
    // 4) one coalesced float4 copy of the block (obs blocks are 16-B aligned per wave)
    if (rows > 0) {
      float* out = a.obs + row0 * KC;
      const int total = rows * KC, n4 = total >> 2;
      float4* out4 = reinterpret_cast<float4*>(out);
      for (int q = lane; q < n4; q += 64) {
#if (IMG_OFF + F16_OBS_DIM) % 4 == 0
        out4[q] = reinterpret_cast<const float4*>(img + IMG_OFF + F16_OBS_DIM)[q];
#else
        const float* p = img + IMG_OFF + 4 * q + F16_OBS_DIM;
        out4[q] = make_float4(p[0], p[1], p[2], p[3]);
#endif
      }
      for (int j = 4 * n4 + lane; j < total; j += 64) out[j] = img[IMG_OFF + j + F16_OBS_DIM];
    }
    F16_STAMP(stamps, ST_COPY);
  } else {
    // fallback (large K): chunked flat copy from obs_prev, frames staged in LDS
    float* sF = dynl;
    float* sR = dynl + BLOCK * FRAME_PITCH;
    if (live) {
#pragma unroll
      for (int j = 0; j < F16_OBS_DIM; ++j) sF[threadIdx.x * FRAME_PITCH + j] = f[j];
      if (done)
#pragma unroll
        for (int j = 0; j < F16_OBS_DIM; ++j) sR[threadIdx.x * FRAME_PITCH + j] = f0[j];
    }
    __syncthreads();
    F16_STAMP(stamps, ST_SYNC);
    // A wave's 64 rows are one contiguous block of 64*K*15 floats in both obs_prev and obs,
    // and out[j] = prev[j + 15] except in each row's last frame: the wave walks the block with
    // flat, coalesced indices j = lane + 64*it; loads are issued in chunks of 16 before their
    // stores, and chunks only read ahead of what earlier chunks wrote (in-place safe).
    if (rows > 0) {
      const float* prev = a.obs_prev + row0 * KC;
      float* out = a.obs + row0 * KC;
      float* tout = a.tobs ? a.tobs + row0 * KC : nullptr;
      const int total = rows * KC;
      int row = lane / KC, col = lane - (lane / KC) * KC;
      constexpr int CH = F16_FALLBACK_CH;
      for (int base = 0; base < total; base += 64 * CH) {
        float v[CH];
        int rw[CH], cl[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
          const int j = base + 64 * u + lane;
          rw[u] = row; cl[u] = col;
          float x = 0.0f;
          if (j < total) {
            const int li = wave * 64 + row;
            x = (col < HC) ? prev[j + F16_OBS_DIM] : sF[li * FRAME_PITCH + (col - HC)];
          }
          v[u] = x;
          col += 64;
          while (col >= KC) { col -= KC; ++row; }
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
          const int j = base + 64 * u + lane;
          if (j < total) {
            const int li = wave * 64 + rw[u];
            if (!sDone[li]) {
              out[j] = v[u];
            } else {
              if (tout) tout[j] = v[u];
              out[j] = autoreset ? sR[li * FRAME_PITCH + (cl[u] % F16_OBS_DIM)] : v[u];
            }
          }
        }
      }
    }
    F16_STAMP(stamps, ST_COPY);
  }
#ifdef F16_STAMPS
  if (lane == 0) {
    const int w = (blockIdx.x * BLOCK + threadIdx.x) >> 6;
    if (w < (1 << 14))
      for (int q = 0; q < ST_N; ++q) g_stamps[w][q] = stamps.acc[q];
  }
#endif
}

#define STEP_SHARED                                       \
  __shared__ __align__(16) float sT[F16_BLOB_FLOATS];   \
  __shared__ __align__(16) float4 sTmpl[NCOL + TMPL_FRAME_COLS]; \
  __shared__ int sDone[BLOCK];                            \
  extern __shared__ __align__(16) float dynl[];

// Occupancy variants. The body needs ~300 registers (VGPR + AGPR), i.e. one wave per SIMD;
// OCC = 2 caps it at 256 (a few spills) so two waves share each SIMD: slower per wave, but
// when there are more waves than SIMDs (N > 64 x 4 x CUs) the pair overlaps one wave's
// memory phases and stalls with the other's VALU work (f16env_step picks per launch).
#define STEP_PRE_ARGS const float4 *__restrict__ sc, const float *__restrict__ act, const float4 *__restrict__ tmpl, int64_t n
__global__ __launch_bounds__(BLOCK, 1) void f16_step_kernel(STEP_PRE_ARGS, StepArgs a) {
  STEP_SHARED
  const StepPre pre = {sc, act, tmpl, n};
  step_body<0>(a, sT, sTmpl, sDone, dynl, &pre);
}
template <int MODE, int OCC, bool ROLL = false>
__global__ __launch_bounds__(BLOCK, OCC) void f16_step_var_kernel(STEP_PRE_ARGS, StepArgs a) {
  STEP_SHARED
  const StepPre pre = {sc, act, tmpl, n};
  step_body<MODE, false, ROLL, OCC == 2>(a, sT, sTmpl, sDone, dynl, &pre);
}
// global-table variant (large K on the LDS-image path): no LDS table copy
template <int MODE, bool ROLL = false>
__global__ __launch_bounds__(BLOCK, 1) void f16_step_gt_kernel(STEP_PRE_ARGS, StepArgs a) {
  __shared__ __align__(16) float4 sTmpl[NCOL + TMPL_FRAME_COLS];
  __shared__ int sDone[BLOCK];
  extern __shared__ __align__(16) float dynl[];
  const StepPre pre = {sc, act, tmpl, n};
  step_body<MODE, true, ROLL>(a, nullptr, sTmpl, sDone, dynl, &pre);
}
// windowed-observation build (f16env_step_window): no stack image, LDS holds the tables and
// the per-wave frame staging
// ROLL: the rollout-slot build (f16env_window_step_rollout: in-kernel Philox or clipped policy
// actions, the slot's actions / rewards / next starts and the returned observation's newest
// frame); the plain windowed step carries none of its code.
template <int MODE, int OCC, bool ROLL = false>
__global__ __launch_bounds__(BLOCK, OCC) void f16_step_win_kernel(STEP_PRE_ARGS, StepArgs a) {
  STEP_SHARED
  const StepPre pre = {sc, act, tmpl, n};
  step_body<MODE, false, ROLL, OCC == 2, true>(a, sT, sTmpl, sDone, dynl, &pre);
}
// ... with non-temporal state and frame-slot stores, for grids resident in one round (st16)
template <int MODE, int OCC, bool ROLL = false>
__global__ __launch_bounds__(BLOCK, OCC) void f16_step_win_nt_kernel(STEP_PRE_ARGS, StepArgs a) {
  STEP_SHARED
  const StepPre pre = {sc, act, tmpl, n};
  step_body<MODE, false, ROLL, OCC == 2, true, true>(a, sT, sTmpl, sDone, dynl, &pre);
}
// the windowed plain step with extras (XV_X | XV_FEAT: the feature window in the epilogue; every
// winx build takes act == NULL as "draw the actions in-kernel"): f16env_window_step_ex. A kernel
// of its own, so the headline instances above keep their instruction stream.
template <int MODE, int OCC, bool NT, int XV>
__global__ __launch_bounds__(BLOCK, OCC) void f16_step_winx_kernel(STEP_PRE_ARGS, StepArgs a) {
  STEP_SHARED
  const StepPre pre = {sc, act, tmpl, n};
  step_body<MODE, false, false, OCC == 2, true, NT, XV>(a, sT, sTmpl, sDone, dynl, &pre);
}
using StepKernel = void (*)(const float4*, const float*, const float4*, int64_t, StepArgs);
using WinKernel = StepKernel;
template <bool ROLL>
static WinKernel step_win_kernel_for_r(int mode, int occ, int nt) {
  static const WinKernel table[2][2][4] = {
      {{f16_step_win_kernel<0, 1, ROLL>, f16_step_win_kernel<1, 1, ROLL>, f16_step_win_kernel<2, 1, ROLL>,
        f16_step_win_kernel<3, 1, ROLL>},
       {f16_step_win_kernel<0, 2, ROLL>, f16_step_win_kernel<1, 2, ROLL>, f16_step_win_kernel<2, 2, ROLL>,
        f16_step_win_kernel<3, 2, ROLL>}},
      {{f16_step_win_nt_kernel<0, 1, ROLL>, f16_step_win_nt_kernel<1, 1, ROLL>, f16_step_win_nt_kernel<2, 1, ROLL>,
        f16_step_win_nt_kernel<3, 1, ROLL>},
       {f16_step_win_nt_kernel<0, 2, ROLL>, f16_step_win_nt_kernel<1, 2, ROLL>, f16_step_win_nt_kernel<2, 2, ROLL>,
        f16_step_win_nt_kernel<3, 2, ROLL>}}};
  return table[nt ? 1 : 0][occ == 2 ? 1 : 0][mode & 3];
}
static WinKernel step_win_kernel_for(int mode, int occ, int nt, bool roll = false) {
  return roll ? step_win_kernel_for_r<true>(mode, occ, nt) : step_win_kernel_for_r<false>(mode, occ, nt);
}
template <int XV>
static WinKernel step_winx_kernel_for_x(int mode, int occ, int nt) {
  static const WinKernel table[2][2][4] = {
      {{f16_step_winx_kernel<0, 1, false, XV>, f16_step_winx_kernel<1, 1, false, XV>,
        f16_step_winx_kernel<2, 1, false, XV>, f16_step_winx_kernel<3, 1, false, XV>},
       {f16_step_winx_kernel<0, 2, false, XV>, f16_step_winx_kernel<1, 2, false, XV>,
        f16_step_winx_kernel<2, 2, false, XV>, f16_step_winx_kernel<3, 2, false, XV>}},
      {{f16_step_winx_kernel<0, 1, true, XV>, f16_step_winx_kernel<1, 1, true, XV>,
        f16_step_winx_kernel<2, 1, true, XV>, f16_step_winx_kernel<3, 1, true, XV>},
       {f16_step_winx_kernel<0, 2, true, XV>, f16_step_winx_kernel<1, 2, true, XV>,
        f16_step_winx_kernel<2, 2, true, XV>, f16_step_winx_kernel<3, 2, true, XV>}}};
  return table[nt ? 1 : 0][occ == 2 ? 1 : 0][mode & 3];
}
static WinKernel step_winx_kernel_for(int mode, int occ, int nt, bool feat) {
  return feat ? step_winx_kernel_for_x<XV_X | XV_FEAT>(mode, occ, nt) : step_winx_kernel_for_x<XV_X>(mode, occ, nt);
}
static constexpr size_t WIN_DYN_LDS = sizeof(float) * (BLOCK / 64) * WIN_WAVE_FLOATS;
// variant: 0 = LDS tables, 1 wave/SIMD; 1 = LDS tables, 2 waves/SIMD; 2 = global tables.
// roll: the rollout-slot build (f16env_step_rollout); the plain step carries none of its code.
static StepKernel step_kernel_for(int mode, int variant, bool roll = false) {
  static const StepKernel table[2][3][4] = {
      {{f16_step_kernel, f16_step_var_kernel<1, 1>, f16_step_var_kernel<2, 1>, f16_step_var_kernel<3, 1>},
       {f16_step_var_kernel<0, 2>, f16_step_var_kernel<1, 2>, f16_step_var_kernel<2, 2>, f16_step_var_kernel<3, 2>},
       {f16_step_gt_kernel<0>, f16_step_gt_kernel<1>, f16_step_gt_kernel<2>, f16_step_gt_kernel<3>}},
      {{f16_step_var_kernel<0, 1, true>, f16_step_var_kernel<1, 1, true>, f16_step_var_kernel<2, 1, true>,
        f16_step_var_kernel<3, 1, true>},
       {f16_step_var_kernel<0, 2, true>, f16_step_var_kernel<1, 2, true>, f16_step_var_kernel<2, 2, true>,
        f16_step_var_kernel<3, 2, true>},
       {f16_step_gt_kernel<0, true>, f16_step_gt_kernel<1, true>, f16_step_gt_kernel<2, true>,
        f16_step_gt_kernel<3, true>}}};
  return table[roll ? 1 : 0][variant < 0 || variant > 2 ? 0 : variant][mode & 3];
}
