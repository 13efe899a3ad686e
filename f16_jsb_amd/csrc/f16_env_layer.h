// f16_env_layer.h -- what surrounds the flight model in one env step: RunIC (apply_ic), the
// observation frame (norm_angle .. euler_norm, make_frame), reward and termination (env_reward,
// EnvArgs), the resets of a lane (lane_reset, lane_reset_mode, lane_reset_template) and the Earth
// position angle. Device code only, shared by the step, rollout, reset and state kernels.
// Needs f16_device.h (Lane, SoA, frame, ModelConsts) and f16_rng.h (rng_goal, rng_ic).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/f16env.h"
#include "f16_device.h"
#include "f16_rng.h"

using namespace f16;

// ------------------------------------------------------------------------------------------
// IC (FGFDMExec::RunIC + InitRunning), mirrors oracle apply_ic()
// ------------------------------------------------------------------------------------------
// LOWREG: the enclosing kernel's register budget (frame<LOWREG>: the two-waves-per-SIMD 256-register
// kernels run their in-kernel RunIC with the same build of the frame as their steps -- round 6;
// before, every RunIC ran the one-wave build's code, also inside the 256-register kernels)
template <bool LOWREG = false>
__device__ void apply_ic(Lane& L, const double* ic, const float* T, const ModelConsts& C) {
  const double lat = ic[F16_IC_LAT_GEOD_RAD], lon = ic[F16_IC_LON_RAD], h = ic[F16_IC_H_SL_FT];
  // (sincos: one argument reduction per angle, the same values as sin / cos)
  double sl, cl, slo, clo;
  sincos(lat, &sl, &cl);
  sincos(lon, &slo, &clo);
  const double N = WGS_A / sqrt(1.0 - E2 * sl * sl);
  const double rE[3] = {(N + h) * cl * clo, (N + h) * cl * slo, (EC2 * N + h) * sl};
  L.epa = 0.0;
  for (int j = 0; j < 3; ++j) L.rI[j] = rE[j];
  const double rxy = sqrt(rE[0] * rE[0] + rE[1] * rE[1]);
  const double r = sqrt(rxy * rxy + rE[2] * rE[2]);
  const double slat = rE[2] / r, clat = rxy / r;
  const double slon = rxy == 0.0 ? 0.0 : rE[1] / rxy, clon = rxy == 0.0 ? 1.0 : rE[0] / rxy;
  const double Lm[9] = {-clon * slat, -slon * slat, clat, -slon, clon, 0.0, -clon * clat, -slon * clat, -slat};
  const double ph = ic[F16_IC_PHI_RAD], th = ic[F16_IC_THETA_RAD], ps = ic[F16_IC_PSI_RAD];
  double cp, sp, ct, st, cs, ss;
  sincos(ph, &sp, &cp);
  sincos(th, &st, &ct);
  sincos(ps, &ss, &cs);
  const double Tl[9] = {ct * cs, ct * ss, -st,
                        sp * st * cs - cp * ss, sp * st * ss + cp * cs, sp * ct,
                        cp * st * cs + sp * ss, cp * st * ss - sp * cs, cp * ct};
  double Ti[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Ti[3 * i + j] = Tl[3 * i] * Lm[j] + Tl[3 * i + 1] * Lm[3 + j] + Tl[3 * i + 2] * Lm[6 + j];
  // FGMatrix33::GetQuaternion
  double t[4] = {1.0 + Ti[0] + Ti[4] + Ti[8], 1.0 + Ti[0] - Ti[4] - Ti[8],
                 1.0 - Ti[0] + Ti[4] - Ti[8], 1.0 - Ti[0] - Ti[4] + Ti[8]};
  int idx = 0;
  for (int i = 1; i < 4; ++i)
    if (t[i] > t[idx]) idx = i;
  double q[4];
  if (idx == 0) {
    q[0] = 0.5 * sqrt(t[0]);
    q[1] = 0.25 * (Ti[5] - Ti[7]) / q[0]; q[2] = 0.25 * (Ti[6] - Ti[2]) / q[0]; q[3] = 0.25 * (Ti[1] - Ti[3]) / q[0];
  } else if (idx == 1) {
    q[1] = 0.5 * sqrt(t[1]);
    q[0] = 0.25 * (Ti[5] - Ti[7]) / q[1]; q[2] = 0.25 * (Ti[1] + Ti[3]) / q[1]; q[3] = 0.25 * (Ti[2] + Ti[6]) / q[1];
  } else if (idx == 2) {
    q[2] = 0.5 * sqrt(t[2]);
    q[0] = 0.25 * (Ti[6] - Ti[2]) / q[2]; q[1] = 0.25 * (Ti[1] + Ti[3]) / q[2]; q[3] = 0.25 * (Ti[5] + Ti[7]) / q[2];
  } else {
    q[3] = 0.5 * sqrt(t[3]);
    q[0] = 0.25 * (Ti[1] - Ti[3]) / q[3]; q[1] = 0.25 * (Ti[2] + Ti[6]) / q[3]; q[2] = 0.25 * (Ti[5] + Ti[7]) / q[3];
  }
  if (q[0] < 0) for (int i = 0; i < 4; ++i) q[i] = -q[i];
  const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) { q[i] /= qn; L.q[i] = (float)q[i]; }
  // Ti2b from the normalised quaternion (double), velocities
  const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
  const double T0 = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, T1 = 2.0 * (q1 * q2 + q0 * q3), T2 = 2.0 * (q1 * q3 - q0 * q2);
  const double T3 = 2.0 * (q1 * q2 - q0 * q3), T4 = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, T5 = 2.0 * (q2 * q3 + q0 * q1);
  const double T6 = 2.0 * (q1 * q3 + q0 * q2), T7 = 2.0 * (q2 * q3 - q0 * q1), T8 = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
  const double u = ic[F16_IC_U_FPS], v = ic[F16_IC_V_FPS], w = ic[F16_IC_W_FPS];
  const double vb[3] = {T0 * u + T3 * v + T6 * w, T1 * u + T4 * v + T7 * w, T2 * u + T5 * v + T8 * w};
  L.vI[0] = vb[0] - OMEGA_E * L.rI[1];
  L.vI[1] = vb[1] + OMEGA_E * L.rI[0];
  L.vI[2] = vb[2];
  L.wI[0] = (float)(ic[F16_IC_P_RPS] + T2 * OMEGA_E);
  L.wI[1] = (float)(ic[F16_IC_Q_RPS] + T5 * OMEGA_E);
  L.wI[2] = (float)(ic[F16_IC_R_RPS] + T8 * OMEGA_E);
  for (int j = 0; j < 3; ++j) {
    L.wId[j] = 0.0f; L.ba[j] = 0.0f; L.aI[j] = 0.0f; L.aIp[j] = 0.0f; L.ndv1[j] = -0.0f; L.dv2[j] = 0.0f;
    L.wst[j] = (float)ic[F16_IC_WIND_N_FPS + j];
    L.wind[j] = L.wst[j] + L.gust[j];  // callers set the gust (0 outside the cfg5 gust mode)
  }
  L.tef = L.ail = L.ele = L.rud = L.lef = L.sb = 0.0f;
  L.pri = L.prp = L.ppi = L.ppp = L.pyi = L.pyp = 0.0f;
  L.n1 = 30.0f; L.n2 = 60.0f; L.flags = 0;
  for (int j = 0; j < F16L_N; ++j) L.lx[j] = 0.0f;
  const float cmd[4] = {(float)ic[F16_IC_CMD_AIL], (float)ic[F16_IC_CMD_ELE], (float)ic[F16_IC_CMD_RUD],
                        (float)ic[F16_IC_CMD_THR]};
  double ce = 1.0, se = 0.0;
#ifdef F16_STAMPS
  Stamps stamps = {};
#endif
  const AltRef A = alt_ref(L, ce, se);
  // three passes, as oracle apply_ic(); a loop, not three inlined copies: the reset kernels run
  // one RunIC per lane from a cold instruction cache, so one copy of the frame code is fetched
  // once and hit twice
#pragma nounroll
  for (int pass = 0; pass < 3; ++pass) frame<LOWREG>(L, cmd, ce, se, A, T, C, true F16_STAMP_PASS);
  for (int j = 0; j < 3; ++j) { L.ndv1[j] = -0.0f; L.dv2[j] = 0.0f; L.aIp[j] = L.aI[j]; }  // (dv1 = +0)
}

// ------------------------------------------------------------------------------------------
// env layer
// ------------------------------------------------------------------------------------------
// normalize_angle_mpi_pi (jsbsim_gym.py:60-78) on a float32 value (numpy-1.x promotion)
__device__ __forceinline__ float norm_angle(float a) {
  if (isnan(a) || isinf(a)) return 0.0f;
  double x = (double)a;
  if (!(fabs(x) < 2.0 * PI_D)) x = fmod(x, 2.0 * PI_D);
  if (x < 0.0) x += 2.0 * PI_D;
  if (x >= PI_D) x -= 2.0 * PI_D;
  if (x == 0.0) x = 0.0;
  return (float)x;
}
// The observation's three angles: euler() and norm_angle() with their tests taken together.
// euler() has two gimbal tests and each norm_angle four (NaN / Inf, the fmod guard, < 0, >= pi,
// in fp64): as exec-mask branches each waits on its compare, on one wave's serial path, and
// they keep three copies of OCML's fmod and two of atan2f between the hot blocks. norm_angle
// is the identity on an ordinary angle (f16_device.h ANGLE_ORD_*), and on a heading that
// euler() wrapped by 2*PI_F it is one fp64 subtraction: x >= pi there, and past 2*pi its fmod
// is that same (exact) subtraction. So one wave-uniform test: a wave with every lane off the
// gimbal poles and all three polynomial results ordinary runs straight-line code, any other
// wave runs euler() and norm_angle() as they are, for all its lanes. The same bits either way.
// The two-waves-per-SIMD (256-register) builds keep euler() + norm_angle() and the branching
// env_reward below: three of them grew 4 to 8 B of scratch with the new forms (FAST = false at
// their call sites). -DF16_ENV_LAYER_REF builds those earlier forms into every kernel from the
// same source, for tests/test_gpu_env_layer.py and same-box A/Bs.
#ifdef F16_ENV_LAYER_REF
constexpr bool ENV_LAYER_FAST = false;
#else
constexpr bool ENV_LAYER_FAST = true;
#endif
__device__ __forceinline__ bool angle_ordinary(float a) {
  const float m = fabsf(a);
  return m >= ANGLE_ORD_MIN && m < ANGLE_ORD_END;  // (false for NaN / Inf)
}
template <bool FAST>
__device__ __forceinline__ void euler_norm(const float* T, float* f) {
  if constexpr (FAST && ENV_LAYER_FAST) {
    const float tht = fatan2<true>(-T[2], fsqrt(__builtin_fmaf(T[5], T[5], T[8] * T[8])));  // as euler()
    const float phi = fatan2<true>(T[5], T[8]);
    const float p = fatan2<true>(T[1], T[0]);
    const bool ord = (fabsf(T[2]) < 1.0f) & angle_ordinary(phi) & angle_ordinary(tht) & angle_ordinary(p);
    if (__builtin_expect(__ballot(!ord) == 0ull, 1)) {
      f[0] = phi; f[1] = tht;
      f[2] = (p < 0.0f) ? (float)((double)(p + 2.0f * PI_F) - 2.0 * PI_D) : p;
      return;
    }
  }
  float phi, tht, psi;
  euler(T, phi, tht, psi);
  f[0] = norm_angle(phi); f[1] = norm_angle(tht); f[2] = norm_angle(psi);
}
// _get_current_single_observation (jsbsim_gym.py:172-197)
// The observation frame (jsbsim_gym.py:172-197) from the derived quantities of the lane's
// state; the latitude / longitude are evaluated here. (Reusing the last FDM frame's Derived
// instead -- the frame's accelerations do not move rI, vI, q, wI -- saved 0.7 us per step at
// 4 096 envs and nothing at 65 536 in the windowed step, r02_variants_keep.json, but the
// two builds then round the observation differently: kept out, the one- and two-waves-per-
// SIMD builds stay bit-identical. Round 8 tried it again in the one-wave builds only, frame()
// handing out its Derived: bit-identical now that derive's products are explicit FMAs, but
// carrying Tl2b and h_ft through the last frame put 128 B of scratch into every one-wave step
// kernel, +1.26 us per step at 65 536 envs, profiles/r08_ab_env_layer.json "s3": kept out.)
template <bool FAST = true>
__device__ void make_frame_from(const Lane& L, double ce, double se, const Derived& d, float* f) {
  // explicit FMAs: with contraction left to the compiler, the one- and two-waves-per-SIMD
  // windowed builds paired these products differently, and yE (a difference of two ~2e7 ft
  // terms near the start meridian) and so the observed longitude differed in the last bits
  // (tests/test_gpu_production.py two-million-env case)
  const double xE = __builtin_fma(ce, L.rI[0], se * L.rI[1]);
  const double yE = __builtin_fma(ce, L.rI[1], -se * L.rI[0]);
  const float xf = (float)xE, yf = (float)yE, zf = (float)L.rI[2];
  const float rxyE = fsqrt(__builtin_fmaf(xf, xf, yf * yf));
  const float lat = atan2f(zf, rxyE);
  const float lon = (rxyE == 0.0f) ? 0.0f : atan2f(yf, xf);
  f[0] = (float)((double)lat * 6.3781e6);
  f[1] = (float)((double)lon * 6.3781e6);
  f[2] = (float)(d.h_ft * 0.3048);
  f[3] = L.lx[F16L_MACH];
  f[4] = L.lx[F16L_ALPHA];
  f[5] = L.lx[F16L_BETA];
  f[6] = d.pqr[0]; f[7] = d.pqr[1]; f[8] = d.pqr[2];
  euler_norm<FAST>(d.Tl2b, f + 9);
  f[12] = L.goal[0]; f[13] = L.goal[1]; f[14] = L.goal[2];
}
template <bool FAST = true>
__device__ void make_frame(const Lane& L, double ce, double se, const AltRef& A, float* f) {
  Derived d;
  derive(L, ce, se, A, d);
  make_frame_from<FAST>(L, ce, se, d, f);
}
__device__ __forceinline__ float norm3f(float a, float b, float c) {
#pragma clang fp contract(off)
  float s = a * a;
  s = s + b * b;
  s = s + c * c;
  return sqrtf(s);
}

// observation_space.contains on one frame, finite values only (jsbsim_gym.py:268-285 against
// SINGLE_OBS_LOW / SINGLE_OBS_HIGH, :28-53, float32 bounds): a component outside its bounds
// that is finite. (The infinite bounds of the other components admit every finite value.)
__device__ __forceinline__ bool obs_out_of_bounds(const float* f) {
  const float pe = (float)(PI_D + 1e-5), he = (float)(0.5 * PI_D + 1e-5);
  bool bad = f[3] < 0.0f;                                 // mach >= 0
  bad = bad || f[4] < -pe || f[4] > pe || f[5] < -pe || f[5] > pe;  // alpha, beta
  bad = bad || f[9] < -pe || f[9] > pe || f[11] < -pe || f[11] > pe;  // phi, psi
  bad = bad || f[10] < -he || f[10] > he;               // theta
  bad = bad || f[14] < 0.0f;                            // goal z >= 0
  return bad;  // NaN compares false: non-finite values never count
}

struct EnvArgs {
  int64_t n;
  int32_t K, down_sample, max_steps, flags;
  float dg, crash;
  double gain;
  uint64_t seed;
  int64_t id_base;
  const double* ic_cfg;  // config IC, RANDOM_IC box lo / hi (device, F16_IC_N each)
  const double* ic_lo;
  const double* ic_hi;
  float gust_a, gust_b, gust_sigma;  // cfg5 Gauss-Markov gust coefficients
};

// reward / termination (jsbsim_gym.py:237-261) in float32, then PositionReward (:493-507), on
// the new frame f; Monitor's return (monitor.py:96-99). Returns the flags: bit 0 terminated,
// 1 truncated, 2 quarantined by F16_FLAG_NAN_GUARD (a non-finite position / Mach / alpha /
// beta / body rate; the angles f[9..11] are already NaN -> 0 by normalize_angle_mpi_pi).
// Branch-free: crash / goal / truncation as selects over the same float32 operations in the same
// order (the IEEE sqrtf of the goal test now runs for a crashed lane too, its result unused), and
// the NaN guard as one wave-uniform arm that puts a quarantined lane's results back.
__device__ __forceinline__ int env_reward_sel(Lane& L, const float* f, const EnvArgs& E, float& r32) {
#pragma clang fp contract(off)
  const float alt = f[2];
  const bool crash = alt < E.crash;
  const float dx = f[0] - f[12], dy = f[1] - f[13];
  float d2 = dx * dx;
  d2 = d2 + dy * dy;
  const bool goal = !crash & (sqrtf(d2) < E.dg) & (fabsf(alt - f[14]) < E.dg);
  double r = crash ? -10.0 : (goal ? 10.0 : 0.0);
  int te = (crash | goal) ? 1 : 0;
  int tr = L.step >= E.max_steps ? 1 : 0;                 // env :260 | TimeLimit
  // (the previous distance in a register of its own: see the reference form below)
  float last_d = L.last_d;
  asm volatile("" : "+v"(last_d));
  float dcur = norm3f(f[12] - f[0], f[13] - f[1], f[14] - f[2]);
  const float ddiff = last_d - dcur;
  r = r + E.gain * (double)ddiff;
  double ret = L.ep_ret + r;                              // monitor.py:96-99
  r32 = (float)r;
  if (E.flags & F16_FLAG_NAN_GUARD) {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 9; ++j) bad = bad | !isfinite(f[j]);
    if (__ballot(bad) != 0ull) {  // terminated + quarantined (bit 2), reported as terminated[i] = 3
      te = bad ? 5 : te;
      tr = bad ? 0 : tr;
      r32 = bad ? 0.0f : r32;
      dcur = bad ? last_d : dcur;  // (the lane's last distance and return stay as they were)
      ret = bad ? L.ep_ret : ret;
    }
  }
  L.last_d = dcur;
  L.ep_ret = ret;
  return te | (tr << 1);
}
// (the form before it)
__device__ __forceinline__ int env_reward_ref(Lane& L, const float* f, const EnvArgs& E, float& r32) {
  int te = 0, tr;
  bool bad = false;
  if (E.flags & F16_FLAG_NAN_GUARD) {
#pragma unroll
    for (int j = 0; j < 9; ++j) bad = bad || !isfinite(f[j]);
  }
  if (bad) {
    te = 5;  // terminated + quarantined (bit 2), reported as terminated[i] = 3
    tr = 0;
    r32 = 0.0f;
  } else {
#pragma clang fp contract(off)
    double r = 0.0;
    const float alt = f[2];
    if (alt < E.crash) { r = -10.0; te = 1; }
    const float dx = f[0] - f[12], dy = f[1] - f[13];
    float d2 = dx * dx;
    d2 = d2 + dy * dy;
    if (!te && sqrtf(d2) < E.dg && fabsf(alt - f[14]) < E.dg) { r = 10.0; te = 1; }
    tr = L.step >= E.max_steps ? 1 : 0;                   // env :260 | TimeLimit
    // The previous distance is moved into a register of its own first. SROA keeps the Lane's
    // {goal.z, last_d, wind.x, wind.y} as one 4-VGPR tuple, and the new distance below is
    // written into the same tuple's last_d lane; in f16_step_win_nt_kernel<2|3, 1> (ROCm 7.2,
    // LLVM 22) the register allocator then placed that write before the read of the old value
    // (`v_sub_f32 v0, v207, v207`: every shaping term, hence every reward, was 0 -- the "all-zero
    // rewards" of round 2). The empty asm breaks the tuple's live range; tests/test_isa_lint.py
    // scans the built code object for x - x subtractions.
    float last_d = L.last_d;
    asm volatile("" : "+v"(last_d));
    const float dcur = norm3f(f[12] - f[0], f[13] - f[1], f[14] - f[2]);
    const float ddiff = last_d - dcur;
    r = r + E.gain * (double)ddiff;
    L.last_d = dcur;
    L.ep_ret += r;                                         // monitor.py:96-99
    r32 = (float)r;
  }
  return te | (tr << 1);
}
template <bool FAST = true>
__device__ __forceinline__ int env_reward(Lane& L, const float* f, const EnvArgs& E, float& r32) {
  if constexpr (FAST && ENV_LAYER_FAST) return env_reward_sel(L, f, E, r32);
  return env_reward_ref(L, f, E, r32);
}

// reset a lane and produce its frame 0: the IC template copy (default config), or the full
// RunIC of a per-lane / random / config IC (cfg5 modes: the gust enters the IC passes)
__device__ void lane_reset(Lane& L, const SoA& tmpl, const double* ic, const float* goal,
                           const EnvArgs& E, int64_t k, const float* T, const ModelConsts& C,
                           float* f0) {
  const int32_t ep = L.ep_count;
  const uint64_t gid = (uint64_t)(E.id_base + k);
  if (ic || (E.flags & (F16_FLAG_RANDOM_IC | F16_FLAG_GUSTS))) {
    double ric[F16_IC_N];
    if (!ic) {
      if (E.flags & F16_FLAG_RANDOM_IC) {
        rng_ic(E.seed, gid, (uint32_t)ep, E.ic_lo, E.ic_hi, ric);
        ic = ric;
      } else {
        ic = E.ic_cfg;
      }
    }
    if (E.flags & F16_FLAG_GUSTS) {
      float xi[3];
      rng_normals(E.seed, gid, (uint32_t)ep, 0u, xi);
      for (int j = 0; j < 3; ++j) L.gust[j] = E.gust_sigma * xi[j];
    } else {
      L.gust[0] = L.gust[1] = L.gust[2] = 0.0f;
    }
    apply_ic(L, ic, T, C);
  } else {
    lane_load<true>(tmpl, 0, L);  // the config IC (its wind included: MODE 0 handles have none)
  }
  if (goal) {
    L.goal[0] = goal[0]; L.goal[1] = goal[1]; L.goal[2] = goal[2];
  } else {
    rng_goal(E.seed, gid, (uint32_t)ep, L.goal);
  }
  L.ep_count = ep + 1;
  L.step = 0;
  L.ep_ret = 0.0;
  L.flags |= LANE_FLAG_FRESH;
  make_frame(L, 1.0, 0.0, alt_ref(L, 1.0, 0.0), f0);
  L.last_d = norm3f(f0[12] - f0[0], f0[13] - f0[1], f0[14] - f0[2]);
}

// lane_reset for a kernel compiled for one MODE (the windowed step's in-step RunIC): the random
// IC stays a register array (lane_reset selects between it and the global config IC through
// one pointer, which puts both in scratch)
template <int MODE, bool LOWREG = false>
__device__ void lane_reset_mode(Lane& L, const EnvArgs& E, int64_t k, const float* T, const ModelConsts& C,
                                float* f0) {
  const int32_t ep = L.ep_count;
  const uint64_t gid = (uint64_t)(E.id_base + k);
  if (E.flags & F16_FLAG_GUSTS) {  // (MODE bit 1 is also set by steady wind alone)
    float xi[3];
    rng_normals(E.seed, gid, (uint32_t)ep, 0u, xi);
    for (int j = 0; j < 3; ++j) L.gust[j] = E.gust_sigma * xi[j];
  } else {
    L.gust[0] = L.gust[1] = L.gust[2] = 0.0f;
  }
  if (MODE & 1) {
    double ric[F16_IC_N];
    rng_ic(E.seed, gid, (uint32_t)ep, E.ic_lo, E.ic_hi, ric);
    apply_ic<LOWREG>(L, ric, T, C);
  } else {
    apply_ic<LOWREG>(L, E.ic_cfg, T, C);
  }
  rng_goal(E.seed, gid, (uint32_t)ep, L.goal);
  L.ep_count = ep + 1;
  L.step = 0;
  L.ep_ret = 0.0;
  L.flags |= LANE_FLAG_FRESH;
  make_frame<!LOWREG>(L, 1.0, 0.0, alt_ref(L, 1.0, 0.0), f0);
  L.last_d = norm3f(f0[12] - f0[0], f0[13] - f0[1], f0[14] - f0[2]);
}

// The template's frame 0 without the goal (12 floats) follows its NCOL_ALL state columns as
// TMPL_FRAME_COLS float4s, written once by f16_ic_kernel with the same make_frame: an
// auto-reset then costs the goal draw only, not a frame evaluation (fp64 altitude, Euler
// angles, atan2s) on the critical path of every wave that holds a finished lane.
enum { TMPL_FRAME_COLS = 3, TMPL_COLS = NCOL_ALL + TMPL_FRAME_COLS };
__device__ __forceinline__ void lane_reset_template(Lane& L, const float4* sTmpl, const EnvArgs& E, int64_t k,
                                                    float* f0) {
  const int32_t ep = L.ep_count;
  lane_load_lds(sTmpl, L);
  rng_goal(E.seed, (uint64_t)(E.id_base + k), (uint32_t)ep, L.goal);
  L.ep_count = ep + 1;
  L.step = 0;
  L.ep_ret = 0.0;
  L.flags |= LANE_FLAG_FRESH;
#pragma unroll
  for (int j = 0; j < TMPL_FRAME_COLS; ++j) {
    const float4 v = sTmpl[NCOL + j];
    f0[4 * j] = v.x; f0[4 * j + 1] = v.y; f0[4 * j + 2] = v.z; f0[4 * j + 3] = v.w;
  }
  f0[12] = L.goal[0]; f0[13] = L.goal[1]; f0[14] = L.goal[2];
  L.last_d = norm3f(f0[12] - f0[0], f0[13] - f0[1], f0[14] - f0[2]);
}

// Earth position angle -> (cos, sin), once per env step (fp64)
__device__ __forceinline__ void earth_angle(double epa, double& ce, double& se) {
  if (fabs(epa) < 0.01) {  // series, exact in fp64 for |epa| < 0.01 (40 s episodes: 3e-3)
    const double e2 = epa * epa;
    ce = 1.0 - e2 * (0.5 - e2 * (1.0 / 24.0 - e2 * (1.0 / 720.0 - e2 * (1.0 / 40320.0))));
    se = epa * (1.0 - e2 * (1.0 / 6.0 - e2 * (1.0 / 120.0 - e2 * (1.0 / 5040.0 - e2 * (1.0 / 362880.0)))));
  } else {
    ce = cos(epa);
    se = sin(epa);
  }
}
