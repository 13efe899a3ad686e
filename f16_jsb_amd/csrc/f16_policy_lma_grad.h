// f16_policy_lma_grad.h -- the eval-mode backward of the LMA policy in the blob's own layout
// (f16env_policy_lma_backward, include/f16env.h ABI 7), one HIP kernel plus a reduce (gfx950).
// Needs f16_policy_lma.h and, through it, f16_policy.h. It reuses, from f16_policy.h: policy_gemm, the
// whole MLP branch of f16_policy_backward_kernel (policy_bwd_branch, with policy_bwd_dw: dW^T =
// X^T Delta and policy_bwd_db summed pairwise; the W^T Delta^T product apart as lmab_wt, one input
// tile at a time) and the reduce kernel; from f16_policy_lma.h, at the row stride POL_XS: the
// forward's own lma_embed_frame, lma_layernorm / lma_ln_stats, lma_probs / lma_attention (k and v
// addressed through LmaKV), lma_gelu / lma_dgelu and lma_tile_out, so the recompute rounds as the
// forward kernel does. float32 throughout.
//
// Tile: ONE wave owns 32 observation rows and walks the whole network for them, every token in
// turn; a block is that wave, a slot of the workspace is that block. So every slot owns every
// piece of the gradient (there is no wave without a token and no wave without a branch): the
// reduce sums all active slots and needs to know only what nobody trains (log_std, PE, a NULL
// branch). Every image is [unit][row] at the row stride POL_XS (33): the first product walks an
// image across units, the second across rows.
//
// The block's LDS, in images of 32 x 33 floats (L = L_new):
//   zs   L      the residual stream of the rows: a block's input while it is differentiated
//   dz   L      its gradient
//   U    the widest of three phases that never overlap:
//        blocks  k, v of every token (2 L), dk, dv (2 L), 8 scratch images (LN1 out, attention out,
//                z after the attention half, q, and LN2 out / c_fc / gelu / delta of ONE 32-unit
//                tile of ff; the last four are reused by the attention half)
//        embed   `flat` (K 64 rows of 33), one frame's features (608 floats) and its embedding (2)
//        heads   one branch's activations (the sum of its widths / 32) and a delta image (widest / 32)
// Budget rule: (2 L + U) x 4224 B <= 160 KiB; the launcher refuses what does not fit (nothing in
// the forward's lattice comes near: L = 5 with blocks takes 38 images, 160 512 B).
//
// Checkpoint and recompute: going up, each block's input z (L images) goes to the slot's own slice
// of the workspace behind its partial gradient (at most 3 x 5 x 4224 B; written and read back by
// the same lanes, L2-resident). Going down, one block at a time is recomputed from its checkpoint:
// k / v of every token first, then per token the attention output, z after the attention half and
// one ff tile at a time, each differentiated as soon as it exists.
//
// Weight gradients: dW of a piece is the MFMA chain over the tile's 32 rows started from the
// slot's partial (first use: from zero), so it sums over the wave's tokens and the slot's later
// tiles in a fixed order: tile, then token. No atomics: the bits depend on (desc, lma, n,
// max_blocks) and the data alone. Rows past n - 1 carry a zero delta from the heads down (every
// step is linear in the delta), so they add exactly nothing.
#pragma once
#include "f16_policy_lma.h"

namespace f16 {

constexpr int LMAB_IMG = 32 * POL_XS;  // floats of one [32 units][33] image
constexpr int LMAB_SCRATCH = 8;        // scratch images of the blocks phase
constexpr int LMAB_BLOCKS = 256;       // default grid limit: the MI355X's CU count

struct LmaBwdArgs : LmaOps {
  const float* blob;
  const float* obs;
  const float* d_mean;
  const float* d_values;
  float* ws;
  int64_t n, row_stride, frame_stride, ntiles, nslots, slot_floats;
  int32_t K, L, C, n_layers, n_pi, n_vf, relu, nf, act_floats;
  uint16_t fmap[LMA_MAX_K * (LMA_EMBED / 2)];  // flat index / 2 of channels 2 s, 2 s + 1 of y[t]
};

__device__ __forceinline__ void lmab_zero(pol_f32x16& a) {
#pragma unroll
  for (int q = 0; q < 16; ++q) a[q] = 0.0f;
}

__host__ __device__ __forceinline__ PolicyOp lmab_op(const int32_t w_off, const int32_t b_off, const int32_t nks) {
  PolicyOp o;
  o.w_off = w_off; o.b_off = b_off; o.nks = nks; o.tout = 1;
  return o;
}

// the 32 row values of one unit summed pairwise (neighbours, then pairs of pairs, ...): five
// roundings deep instead of 31, the order torch's own reductions are closest to
struct LmabRowSum {
  __device__ __forceinline__ float operator()(const float* src) const {
    float v[POL_ROWS];
#pragma unroll
    for (int r = 0; r < POL_ROWS; ++r) v[r] = src[r];
#pragma unroll
    for (int w = 1; w < POL_ROWS; w *= 2) {
#pragma unroll
      for (int r = 0; r < POL_ROWS; r += 2 * w) v[r] += v[r + w];
    }
    return v[0];
  }
};

// The LayerNorm's backward. z: its input image; d: dL / d output in the C/D registers, replaced by
// dL / dz = rstd (g - mean(g) - xhat mean(g xhat)), g = d w (both projection terms, the biased
// variance). The weight's gradient sum_rows d xhat and the bias's sum_rows d go into the slot's
// pieces gw / gb through the images t0, t1 (lane u sums the bias, lane 32 + u the weight, pairwise over the rows).
__device__ __forceinline__ void lmab_ln_backward(const float* z, const float* __restrict__ w, float* gw, float* gb,
                                                 const bool first, float* t0, float* t1, pol_f32x16& d, const int lane) {
  const int j = lane & 31, h = lane >> 5;
  float x[16], mean, rstd;
  lma_ln_stats<POL_XS>(z, lane, mean, rstd, x);
  float xh[16], sg = 0.0f, sgx = 0.0f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int u = pol_unit(q, h);
    xh[q] = (z[u * POL_XS + j] - mean) * rstd;
    t0[u * POL_XS + j] = d[q];
    t1[u * POL_XS + j] = d[q] * xh[q];
    const float g = d[q] * w[u];
    sg += g;
    sgx += g * xh[q];
    d[q] = g;
  }
  sg = lma_xor32(sg) * (1.0f / 32.0f);
  sgx = lma_xor32(sgx) * (1.0f / 32.0f);
#pragma unroll
  for (int q = 0; q < 16; ++q) d[q] = rstd * (d[q] - sg - xh[q] * sgx);
  __builtin_amdgcn_wave_barrier();
  {
    const float s = LmabRowSum()((h ? t1 : t0) + j * POL_XS);
    float* p = (h ? gw : gb) + j;
    *p = first ? s : *p + s;
  }
  __builtin_amdgcn_wave_barrier();
}

// acc += W[every unit of op][inputs 32 ti .. 32 ti + 31]^T Delta^T: the second product of
// f16_policy_backward_kernel for one input tile (C/D: input 32 ti + pol_unit(r, h), row l & 31).
// Inputs past the piece repeat its last one; the caller drops them.
__device__ __forceinline__ void lmab_wt(const float* __restrict__ wb, const PolicyOp op, const int ti, const float* dl,
                                        const int lane, pol_f32x16& acc) {
  const int j = lane & 31, h = lane >> 5;
  const int nin = 2 * op.nks;
  const int in = 32 * ti + j < nin ? 32 * ti + j : nin - 1;
  for (int to = 0; to < op.tout; ++to) {
    float b[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) b[s] = dl[(32 * to + 16 * h + s) * POL_XS + j];
    const pol_f32x4* wp = reinterpret_cast<const pol_f32x4*>(wb + op.w_off + ((to * nin + in) * 32 + 16 * h));
    const pol_f32x4 w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3];
    const float w[16] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3],
                         w2[0], w2[1], w2[2], w2[3], w3[0], w3[1], w3[2], w3[3]};
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[s], b[s], acc, 0, 0, 0);
  }
}

// k and v of the tokens in the images kv ([2 b] k, [2 b + 1] v of token b) as a lane reads them:
// its four dims of head hd are units 8 hd + 4 (l >> 5) .. + 3 of row l & 31 (the C/D map)
__device__ __forceinline__ LmaKV lmab_kv_of(const float* kv, const int lane) {
  const int o = 4 * (lane >> 5) * POL_XS + (lane & 31);
  return {kv + o, kv + LMAB_IMG + o, POL_XS, 8 * POL_XS, 2 * LMAB_IMG};
}

// k and v of every token from the block's input z
__device__ __forceinline__ void lmab_kv(const float* __restrict__ wb, const LmaBlockOps& B, const float* zs, float* kv,
                                        float* ln, const int L, const int lane, pol_f32x16 (&acc)[4]) {
  for (int r = 0; r < L; ++r) {
    lma_layernorm<POL_XS>(zs + r * LMAB_IMG, wb + B.ln1_w, wb + B.ln1_b, ln, lane);
    policy_gemm<2>(wb, B.kv, ln, POL_XS, lane, acc);
    lma_tile_out<POL_XS, false>(kv + (2 * r) * LMAB_IMG, acc[0], lane);
    lma_tile_out<POL_XS, false>(kv + (2 * r + 1) * LMAB_IMG, acc[1], lane);
    __builtin_amdgcn_wave_barrier();
  }
}

// one block of the extractor going up, in place on zs (S: scratch images)
__device__ __forceinline__ void lmab_block_forward(const float* __restrict__ wb, const LmaBlockOps& B, float* zs, float* kv,
                                                   float* S, const int L, const int lane, pol_f32x16 (&acc)[4]) {
  float* ln = S;
  float* ao = S + LMAB_IMG;
  float* ffh = S + 2 * LMAB_IMG;  // (up to four images)
  lmab_kv(wb, B, zs, kv, ln, L, lane, acc);
  for (int r = 0; r < L; ++r) {
    float* z = zs + r * LMAB_IMG;
    lma_layernorm<POL_XS>(z, wb + B.ln1_w, wb + B.ln1_b, ln, lane);
    policy_gemm<1>(wb, B.q, ln, POL_XS, lane, acc);
    lma_attention<POL_XS>(acc[0], lmab_kv_of(kv, lane), L, ao, lane);
    policy_gemm<1>(wb, B.proj, ao, POL_XS, lane, acc);
    lma_tile_out<POL_XS, true>(z, acc[0], lane);
    __builtin_amdgcn_wave_barrier();
    lma_layernorm<POL_XS>(z, wb + B.ln2_w, wb + B.ln2_b, ln, lane);
    for (int tt = 0; tt < B.fc.tout; ++tt) {
      policy_gemm<1>(wb, lmab_op(B.fc.w_off + tt * B.fc.nks * 64, B.fc.b_off + 32 * tt, B.fc.nks), ln, POL_XS, lane, acc);
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[0][q] = lma_gelu(acc[0][q]);
      lma_tile_out<POL_XS, false>(ffh + tt * LMAB_IMG, acc[0], lane);
    }
    __builtin_amdgcn_wave_barrier();
    policy_gemm<1>(wb, B.proj2, ffh, POL_XS, lane, acc);
    lma_tile_out<POL_XS, true>(z, acc[0], lane);
    __builtin_amdgcn_wave_barrier();
  }
}

// one block going down: zs holds its input z (the checkpoint), dz the gradient of its output and,
// on return, of its input. g: the slot's partial gradient.
__device__ __forceinline__ void lmab_block_backward(const float* __restrict__ wb, float* g, const LmaBlockOps& B,
                                                    const float* zs, float* dz, float* kv, float* dkv, float* S, const int L,
                                                    const bool first, const int lane, pol_f32x16 (&acc)[4]) {
  const int j = lane & 31, h = lane >> 5;
  float* ln1 = S;
  float* ao = S + LMAB_IMG;
  float* zm = S + 2 * LMAB_IMG;
  float* qs = S + 3 * LMAB_IMG;
  float* s4 = S + 4 * LMAB_IMG;
  float* s5 = S + 5 * LMAB_IMG;
  float* s6 = S + 6 * LMAB_IMG;
  float* s7 = S + 7 * LMAB_IMG;
  lmab_kv(wb, B, zs, kv, ln1, L, lane, acc);
  for (int e = lane; e < 2 * L * LMAB_IMG; e += 64) dkv[e] = 0.0f;
  __builtin_amdgcn_wave_barrier();

  for (int r = 0; r < L; ++r) {
    const bool f0 = first && r == 0;
    const float* z = zs + r * LMAB_IMG;
    float* dzr = dz + r * LMAB_IMG;
    // recompute the attention half: LN1, q, the attention output, z after its residual update
    lma_layernorm<POL_XS>(z, wb + B.ln1_w, wb + B.ln1_b, ln1, lane);
    policy_gemm<1>(wb, B.q, ln1, POL_XS, lane, acc);
    lma_tile_out<POL_XS, false>(qs, acc[0], lane);
    lma_attention<POL_XS>(acc[0], lmab_kv_of(kv, lane), L, ao, lane);
    policy_gemm<1>(wb, B.proj, ao, POL_XS, lane, acc);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int u = pol_unit(q, h);
      zm[u * POL_XS + j] = z[u * POL_XS + j] + acc[0][q];
    }
    __builtin_amdgcn_wave_barrier();

    // ---- the MLP half, one 32-unit tile of ff at a time: z_out = zm + c_proj2(gelu(c_fc(LN2(zm))))
    float* ln2 = s4;
    lma_layernorm<POL_XS>(zm, wb + B.ln2_w, wb + B.ln2_b, ln2, lane);
    pol_f32x16 dln;
    lmab_zero(dln);
    for (int tt = 0; tt < B.fc.tout; ++tt) {
      const PolicyOp fc = lmab_op(B.fc.w_off + tt * B.fc.nks * 64, B.fc.b_off + 32 * tt, B.fc.nks);
      const PolicyOp p2 = lmab_op(B.proj2.w_off + 32 * tt * 32, B.proj2.b_off, 16);
      policy_gemm<1>(wb, fc, ln2, POL_XS, lane, acc);
      const pol_f32x16 pre = acc[0];
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[0][q] = lma_gelu(pre[q]);
      lma_tile_out<POL_XS, false>(s6, acc[0], lane);
      __builtin_amdgcn_wave_barrier();
      policy_bwd_dw<1>(g, p2, s6, dzr, f0, lane);
      pol_f32x16 d;
      lmab_zero(d);
      lmab_wt(wb, p2, 0, dzr, lane, d);
#pragma unroll
      for (int q = 0; q < 16; ++q) d[q] *= lma_dgelu(pre[q]);
      lma_tile_out<POL_XS, false>(s7, d, lane);
      __builtin_amdgcn_wave_barrier();
      policy_bwd_dw<1>(g, fc, ln2, s7, f0, lane);
      policy_bwd_db<LmabRowSum>(g, fc, s7, f0, lane);
      lmab_wt(wb, fc, 0, s7, lane, dln);
      __builtin_amdgcn_wave_barrier();  // the next tile's images follow every read of this one's
    }
    policy_bwd_db<LmabRowSum>(g, B.proj2, dzr, f0, lane);
    lmab_ln_backward(zm, wb + B.ln2_w, g + B.ln2_w, g + B.ln2_b, f0, s5, s6, dln, lane);
    lma_tile_out<POL_XS, true>(dzr, dln, lane);  // now dL / d zm
    __builtin_amdgcn_wave_barrier();

    // ---- the attention half: zm = z + c_proj(softmax(q . k / sqrt(8)) v)
    policy_bwd_dw<1>(g, B.proj, ao, dzr, f0, lane);
    policy_bwd_db<LmabRowSum>(g, B.proj, dzr, f0, lane);
    pol_f32x16 dao, qv, dq;
    lmab_zero(dao);
    lmab_wt(wb, B.proj, 0, dzr, lane, dao);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      qv[q] = qs[pol_unit(q, h) * POL_XS + j];
      dq[q] = 0.0f;
    }
#pragma unroll
    for (int hd = 0; hd < 4; ++hd) {
      float p[LMA_MAX_L], dp[LMA_MAX_L], dot = 0.0f;
      lma_probs(qv, lmab_kv_of(kv, lane), L, hd, p);
      const int o = (8 * hd + 4 * h) * POL_XS + j;
#pragma unroll
      for (int b = 0; b < LMA_MAX_L; ++b) {
        dp[b] = 0.0f;
        if (b < L) {
          const float* vp = kv + (2 * b + 1) * LMAB_IMG + o;
          float s = dao[4 * hd] * vp[0];
          s += dao[4 * hd + 1] * vp[POL_XS];
          s += dao[4 * hd + 2] * vp[2 * POL_XS];
          s += dao[4 * hd + 3] * vp[3 * POL_XS];
          dp[b] = lma_xor32(s);
          dot += p[b] * dp[b];
        }
      }
#pragma unroll
      for (int b = 0; b < LMA_MAX_L; ++b) {
        if (b < L) {
          const float ds = p[b] * (dp[b] - dot) * LMA_QK_SCALE;  // softmax: P o (dP - sum P dP)
          const float* kp = kv + (2 * b) * LMAB_IMG + o;
          float* dkp = dkv + (2 * b) * LMAB_IMG + o;
          float* dvp = dkv + (2 * b + 1) * LMAB_IMG + o;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            dq[4 * hd + i] += ds * kp[i * POL_XS];
            dkp[i * POL_XS] += ds * qv[4 * hd + i];
            dvp[i * POL_XS] += p[b] * dao[4 * hd + i];
          }
        }
      }
    }
    lma_tile_out<POL_XS, false>(s4, dq, lane);
    __builtin_amdgcn_wave_barrier();
    policy_bwd_dw<1>(g, B.q, ln1, s4, f0, lane);
    policy_bwd_db<LmabRowSum>(g, B.q, s4, f0, lane);
    lmab_zero(dln);
    lmab_wt(wb, B.q, 0, s4, lane, dln);
    lmab_ln_backward(z, wb + B.ln1_w, g + B.ln1_w, g + B.ln1_b, f0, s5, s6, dln, lane);
    lma_tile_out<POL_XS, true>(dzr, dln, lane);  // dL / dz through the residual and q; k and v follow below
    __builtin_amdgcn_wave_barrier();
  }

  // ---- k and v of token b collected every token's dk[b], dv[b]: c_attn's k | v rows and LN1 again
  for (int b = 0; b < L; ++b) {
    const bool f0 = first && b == 0;
    const float* z = zs + b * LMAB_IMG;
    const float* dkb = dkv + (2 * b) * LMAB_IMG;
    lma_layernorm<POL_XS>(z, wb + B.ln1_w, wb + B.ln1_b, ln1, lane);
    policy_bwd_dw<2>(g, B.kv, ln1, dkb, f0, lane);
    policy_bwd_db<LmabRowSum>(g, B.kv, dkb, f0, lane);
    pol_f32x16 dln;
    lmab_zero(dln);
    lmab_wt(wb, B.kv, 0, dkb, lane, dln);
    lmab_ln_backward(z, wb + B.ln1_w, g + B.ln1_w, g + B.ln1_b, false, s5, s6, dln, lane);
    lma_tile_out<POL_XS, true>(dz + b * LMAB_IMG, dln, lane);
    __builtin_amdgcn_wave_barrier();
  }
}

// `flat` of the tile's rows as an image [f][row]: y[t] = relu(W_e x[t] + b_e) + PE[t] at its place
// of the stacking permutation
template <int D>
__device__ __forceinline__ void lmab_flat(const LmaBwdArgs& a, const int64_t rowc, float* flat, float* xf, const int lane,
                                          pol_f32x16 (&acc)[4]) {
  const int j = lane & 31, h = lane >> 5;
  const float* pe = a.blob + a.pe_off;
  if (h == 0) xf[LMA_FEAT * POL_XS + j] = 0.0f;  // the zero-weight pad input
  for (int t = 0; t < a.K; ++t) {
    lma_embed_frame<D>(a.blob, a.we, a.obs + rowc * a.row_stride + (int64_t)t * a.frame_stride, xf, lane, acc);
#pragma unroll
    for (int to = 0; to < 2; ++to) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int u = 32 * to + pol_unit(q, h);
        const int f = 2 * (int)a.fmap[t * (LMA_EMBED / 2) + (u >> 1)] + (u & 1);
        const float v = acc[to][q];
        flat[f * POL_XS + j] = (v < 0.0f ? 0.0f : v) + pe[t * LMA_EMBED + u];
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
}

template <int D>
__global__ __launch_bounds__(64) void f16_policy_lma_backward_kernel(const LmaBwdArgs a) {
  extern __shared__ float4 lmab_sm4[];
  float* sm = reinterpret_cast<float*>(lmab_sm4);
  const int lane = (int)threadIdx.x, j = lane & 31, h = lane >> 5;
  const float* wb = a.blob;
  const int L = a.L, C = a.C;
  float* zs = sm;
  float* dz = zs + L * LMAB_IMG;
  float* U = dz + L * LMAB_IMG;
  // the phases of U
  float* kv = U;
  float* dkv = kv + 2 * L * LMAB_IMG;
  float* S = dkv + 2 * L * LMAB_IMG;
  float* flat = U;
  float* xf = flat + a.K * LMA_EMBED * POL_XS;
  float* ys = xf + LMA_XF;
  float* as = U;
  float* dl = as + a.act_floats;
  float* g = a.ws + (int64_t)blockIdx.x * a.slot_floats;
  float* ck = g + ((a.nf + 3) & ~3);
  pol_f32x16 acc[4];
  bool first = true;
  for (int64_t t = blockIdx.x; t < a.ntiles; t += a.nslots) {
    const int64_t row0 = t * POL_ROWS, row = row0 + j;
    const bool valid = row < a.n;
    const int64_t rowc = valid ? row : a.n - 1;  // rows past n - 1 repeat it (always a valid read)

    // ---- going up: the two embeddings, then the blocks, each from its checkpointed input
    lmab_flat<D>(a, rowc, flat, xf, lane, acc);
    for (int r = 0; r < L; ++r) {
      policy_gemm<1>(wb, a.w2, flat + r * C * POL_XS, POL_XS, lane, acc);
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[0][q] = acc[0][q] < 0.0f ? 0.0f : acc[0][q];
      lma_tile_out<POL_XS, false>(zs + r * LMAB_IMG, acc[0], lane);
    }
    __builtin_amdgcn_wave_barrier();
    for (int layer = 0; layer < a.n_layers; ++layer) {
      float* c = ck + layer * L * LMAB_IMG;
      for (int e = lane; e < L * LMAB_IMG; e += 64) c[e] = zs[e];
      lmab_block_forward(wb, a.blk[layer], zs, kv, S, L, lane, acc);
    }

    // ---- the two MLPs on the features image zs (f16_policy_backward_kernel's branch, whose
    // first layer also hands its delta down: dz = W^T Delta of both branches, pi first)
    bool have = false;
    for (int br = 0; br < 2; ++br) {
      if (!(br ? a.d_values : a.d_mean)) continue;
      policy_bwd_branch<LmabRowSum>(a, br, zs, as, dl, g, row, valid, first, lane, acc);
      const PolicyOp op0 = a.ops[br * (POL_MAX_LAYERS + 1)];  // the branch's first layer: dl holds its delta
      for (int ti = 0; ti < L; ++ti) {
        pol_f32x16 d;
        lmab_zero(d);
        lmab_wt(wb, op0, ti, dl, lane, d);
        if (have) lma_tile_out<POL_XS, true>(dz + ti * LMAB_IMG, d, lane);
        else lma_tile_out<POL_XS, false>(dz + ti * LMAB_IMG, d, lane);
      }
      have = true;
      __builtin_amdgcn_wave_barrier();  // the other branch's images follow every read of this one's
    }

    // ---- going down: the blocks, last first, each recomputed from its checkpoint
    for (int layer = a.n_layers - 1; layer >= 0; --layer) {
      const float* c = ck + layer * L * LMAB_IMG;
      for (int e = lane; e < L * LMAB_IMG; e += 64) zs[e] = c[e];
      __builtin_amdgcn_wave_barrier();
      lmab_block_backward(wb, g, a.blk[layer], zs, dz, kv, dkv, S, L, first, lane, acc);
    }

    // ---- the two embeddings: zs is z = relu(W_2 flat + b_2) again
    for (int r = 0; r < L; ++r) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int e = r * LMAB_IMG + pol_unit(q, h) * POL_XS + j;
        dz[e] = zs[e] > 0.0f ? dz[e] : 0.0f;
      }
    }
    lmab_flat<D>(a, rowc, flat, xf, lane, acc);
    for (int r = 0; r < L; ++r) {
      float* fr = flat + r * C * POL_XS;
      const float* dzr = dz + r * LMAB_IMG;
      policy_bwd_dw<1>(g, a.w2, fr, dzr, first && r == 0, lane);
      policy_bwd_db<LmabRowSum>(g, a.w2, dzr, first && r == 0, lane);
      __builtin_amdgcn_wave_barrier();
      // d flat[r] = W_2^T dz[r] replaces flat[r]: the transpose of the forward's fold, read back per frame below
      for (int ti = 0; 32 * ti < C; ++ti) {
        pol_f32x16 d;
        lmab_zero(d);
        lmab_wt(wb, a.w2, ti, dzr, lane, d);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int i = 32 * ti + pol_unit(q, h);
          if (i < C) fr[i * POL_XS + j] = d[q];
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    for (int tf = 0; tf < a.K; ++tf) {
      lma_embed_frame<D>(wb, a.we, a.obs + rowc * a.row_stride + (int64_t)tf * a.frame_stride, xf, lane, acc);
#pragma unroll
      for (int to = 0; to < 2; ++to) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int u = 32 * to + pol_unit(q, h);
          const int f = 2 * (int)a.fmap[tf * (LMA_EMBED / 2) + (u >> 1)] + (u & 1);
          const float d = flat[f * POL_XS + j];
          ys[u * POL_XS + j] = (valid && acc[to][q] > 0.0f) ? d : 0.0f;
        }
      }
      __builtin_amdgcn_wave_barrier();
      policy_bwd_dw<2>(g, a.we, xf, ys, first && tf == 0, lane);
      policy_bwd_db<LmabRowSum>(g, a.we, ys, first && tf == 0, lane);
      __builtin_amdgcn_wave_barrier();  // the next frame's images follow every read of this one's
    }
    first = false;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct LmaBwdPlan {
  int64_t nf, ntiles, grid, slot_floats, lds_bytes;
  int32_t act_floats;
};

// The launch shape from the descriptors alone (no device): the LDS of the header comment's budget
// rule, the slot's floats (its partial gradient, then a checkpoint of L images per block), and
// grid = min(tiles, max_blocks or LMAB_BLOCKS).
static int lma_bwd_plan(const f16_policy_desc* desc, const f16_lma_desc* m, int64_t n, int32_t max_blocks, LmaBwdPlan* p,
                        int64_t* off, LmaOps* ops) {
  if (const char* e = policy_desc_error(desc)) return set_err(-1, e);
  if (const char* e = lma_desc_error(desc, m)) return set_err(-1, e);
  if (n < 0) return set_err(-1, "n must be >= 0");
  if (max_blocks < 0) return set_err(-1, "max_blocks must be >= 0 (0: the default)");
  p->nf = lma_layout(desc, m, off, ops);
  if (p->nf > 0x7fffffffLL) return set_err(-1, "the blob is too large");
  // what the reduce relies on: the blob is pi hidden | vf hidden | action head | value head | log_std | PE |
  // extractor with no gap between pieces (every float below log_std and past the PE table is a piece some
  // block writes: a gap would be summed from unwritten workspace), and log_std is followed at once by PE
  if (off[0] != 0 || off[POL_OFF_VF0] <= 0 || off[POL_OFF_VF0] >= off[F16_POLICY_OFF_ACT_W] ||
      off[F16_POLICY_OFF_ACT_W] >= off[F16_POLICY_OFF_VAL_W] || off[F16_POLICY_OFF_VAL_W] >= off[F16_POLICY_OFF_LOG_STD] ||
      off[F16_LMA_OFF_PE] != off[F16_POLICY_OFF_LOG_STD] + 4 ||
      off[F16_LMA_OFF_WE_W] != off[F16_LMA_OFF_PE] + (int64_t)m->K * LMA_EMBED)
    return set_err(-1, "internal: the LMA blob layout is not the one the backward's reduce assumes");
  const PolicyWidths w = policy_widths(desc);
  p->act_floats = (w.sum[0] > w.sum[1] ? w.sum[0] : w.sum[1]) * POL_XS;
  const int64_t heads = p->act_floats + w.max_w * POL_XS;
  const int64_t embed = (int64_t)m->K * LMA_EMBED * POL_XS + LMA_XF + 2 * LMAB_IMG;
  const int64_t blocks = m->n_layers > 0 ? (int64_t)(4 * m->L_new + LMAB_SCRATCH) * LMAB_IMG : 0;
  int64_t u = heads > embed ? heads : embed;
  u = blocks > u ? blocks : u;
  p->lds_bytes = ((int64_t)2 * m->L_new * LMAB_IMG + u) * 4;
  if (p->lds_bytes > POL_LDS_BYTES) return set_err(-1, "the LMA policy's backward images do not fit the LDS");
  p->slot_floats = ((p->nf + 3) & ~(int64_t)3) + (int64_t)m->n_layers * m->L_new * LMAB_IMG;
  p->ntiles = n / POL_ROWS + (n % POL_ROWS != 0);
  const int64_t lim = max_blocks ? max_blocks : LMAB_BLOCKS;
  p->grid = p->ntiles < lim ? p->ntiles : lim;
  return 0;
}

static int policy_lma_backward_workspace_impl(const f16_policy_desc* desc, const f16_lma_desc* m, int64_t n,
                                              int32_t max_blocks, int64_t* bytes_out) {
  LmaBwdPlan p;
  int64_t off[F16_LMA_N_OFFSETS];
  if (int rc = lma_bwd_plan(desc, m, n, max_blocks, &p, off, nullptr)) return rc;
  if (!bytes_out) return set_err(-1, "null argument");
  *bytes_out = p.grid * p.slot_floats * 4;
  return 0;
}

static int policy_lma_backward_impl(void* stream, const f16_policy_desc* desc, const f16_lma_desc* m, const float* blob,
                                    int64_t n, const float* obs, int64_t row_stride, int64_t frame_stride,
                                    const float* d_mean, const float* d_values, void* workspace, int64_t workspace_bytes,
                                    int32_t max_blocks, float* grad_blob) {
  LmaBwdPlan p;
  LmaBwdArgs a{};
  int64_t off[F16_LMA_N_OFFSETS];
  if (int rc = lma_bwd_plan(desc, m, n, max_blocks, &p, off, &a)) return rc;
  if (n > 0)
    if (int rc = policy_backward_check("f16env_policy_lma_backward_workspace", blob, obs, row_stride, frame_stride, d_mean,
                                       d_values, workspace, workspace_bytes, p.grid * p.slot_floats * 4, grad_blob))
      return rc;
  const void* fn = desc->D == 15 ? (const void*)f16_policy_lma_backward_kernel<15> : (const void*)f16_policy_lma_backward_kernel<17>;
  static uint64_t prepared[2];
  if (int rc = policy_prepare_instance(fn, &prepared[desc->D == 17 ? 1 : 0])) return rc;
  if (n == 0) return 0;
  a.blob = blob; a.obs = obs; a.d_mean = d_mean; a.d_values = d_values;
  a.ws = static_cast<float*>(workspace);
  a.n = n; a.row_stride = row_stride; a.frame_stride = frame_stride;
  a.ntiles = p.ntiles; a.nslots = p.grid; a.slot_floats = p.slot_floats;
  a.K = m->K; a.L = m->L_new; a.C = m->C_new; a.n_layers = m->n_layers;
  a.n_pi = desc->n_pi; a.n_vf = desc->n_vf;
  a.relu = desc->activation == F16_POLICY_ACT_RELU ? 1 : 0;
  a.nf = (int32_t)p.nf; a.act_floats = p.act_floats;
  for (int t = 0; t < m->K; ++t)
    for (int s = 0; s < LMA_EMBED / 2; ++s) a.fmap[t * (LMA_EMBED / 2) + s] = (uint16_t)(lma_flat_index(m, t, 2 * s) / 2);
  void* kargs[] = {&a};
  HIPCHK(hipLaunchKernel(fn, dim3((unsigned)p.grid), dim3(64), kargs, (size_t)p.lds_bytes, (hipStream_t)stream));
  // (every slot got a tile: grid <= tiles; log_std and the PE table behind it are not trained)
  policy_launch_reduce((hipStream_t)stream, a.ws, grad_blob, p.nf, p.slot_floats, p.grid, off,
                       off[F16_LMA_OFF_PE] + m->K * LMA_EMBED, d_mean, d_values);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace f16
