// f16_policy_lma.h -- the LMA features extractor in front of the actor-critic MLPs as one HIP
// kernel (gfx950), and the host side of f16env_policy_lma_blob_layout / f16env_policy_lma_forward
// (include/f16env.h, ABI 7). Needs f16_features.h (frame_features) and f16_policy.h, whose policy_gemm /
// policy_hidden / policy_tiles / policy_sample, operand forms and C/D register map it reuses.
// The extractor's pieces (lma_layernorm, lma_attention, lma_gelu, lma_embed_frame, lma_tile_out)
// are written once here for this kernel and for the backward's recompute (f16_policy_lma_grad.h).
//
// Tile: a block of 4 waves owns 32 observation rows. Every linear layer of the extractor is per
// token, so it is the MLP's H^T = W X^T with the 32 rows as MFMA columns, once per token, and the
// tokens are dealt to the waves (frame t and new token r to wave t % 4, r % 4): the serial chain of
// ~70 small GEMMs per row tile, each waiting on L2 for its weights, becomes four chains side by
// side. float32 throughout. Block barriers stand only between phases that exchange tokens: after
// the second embedding, after k / v, and at the end of a block. The pi branch runs on wave 0, the
// vf branch on wave 1. The block's LDS, in floats (L = L_new; images are [unit][row], row stride 32):
//   zs   L x 1024   the residual stream z[r][unit][row]; after the blocks it is the features image
//                   [r 32 + unit][row] the first MLP layers read
//   kv   L x 2048   k and v of every token, each lane's own C/D registers (absent without blocks)
//   vsh  32         the value head's output on its way from wave 1 to wave 0
//   and per wave:
//   ln   1024       a LayerNorm's output (the B operand of c_attn / c_fc)
//   ao   1024       a token's attention output (the B operand of c_proj)
//   S    max of     xf 18 x 33 + ys 64 x 32: one token's feature frame with its OWN zeroed pad row
//                     (the 18th input has zero weights; it must not be another token's data:
//                     0 x inf = NaN) and its embedding y[t]
//                   ffh ff_hidden x 32: gelu(c_fc) of one token
//                   hs  widest MLP layer x 32: a branch's hidden image
// At most 159 872 B (L = 5): one block, four waves, per CU.
// Stages 2-4 never form `flat`: token t is embedded alone, and k-step s of y[t] (channels 2 s,
// 2 s + 1) is accumulated into the accumulator tile of the new token r it belongs to (rmap, from
// the descriptor) against the k-step of W_2 that holds its two columns (cmap): dk and C_new are
// even, so channels 2 s and 2 s + 1 are neighbours in `flat` and in one new token. A wave keeps its
// frames' partial z[r] in at most 5 x 16 accumulator registers (wave 0's start from the bias); the
// partials are added into zs in wave order, then relu.
// Attention: the C/D map gives lane l, registers 4 hd .. 4 hd + 3 dims 4 (l >> 5) .. + 3 of head
// hd of row l & 31, so q.k is four products and one add across lanes l and l ^ 32; q stays in
// registers, k and v come back from the lane's own LDS slots. LayerNorm: a lane sums 16 units of
// its row, the moments are one cross-lane add each (both lanes form a + b, the same bits).
#pragma once
#include "f16_features.h"
#include "f16_policy.h"

namespace f16 {

constexpr int LMA_MAX_L = 5;        // L_new at K = 10
constexpr int LMA_MAX_LAYERS = 3;
constexpr int LMA_EMBED = 64;       // D0
constexpr int LMA_DNEW = 32;        // d_new: one output tile
constexpr int LMA_FEAT = 17;        // features per frame
constexpr int LMA_IMG = LMA_DNEW * POL_ROWS;  // floats of one [32 units][32 rows] image
constexpr int LMA_XF = 608;         // 18 x 33 rounded up to a multiple of 16 floats
constexpr int LMA_MAX_K = 10;
constexpr int LMA_WAVES = 4;        // waves per block, all on the same 32 rows
constexpr float LMA_QK_SCALE = 0.35355339059327373f;  // 1 / sqrt(8): a latent head has 8 dims

struct LmaBlockOps {
  int32_t ln1_w, ln1_b, ln2_w, ln2_b;  // floats into the blob
  PolicyOp q, kv, proj, fc, proj2;
};
// where the extractor's and the MLPs' pieces lie in the blob: what lma_layout fills for both kernels
struct LmaOps {
  int32_t pe_off;
  PolicyOp we, w2;
  LmaBlockOps blk[LMA_MAX_LAYERS];
  PolicyOp ops[POL_OPS];
};
struct LmaArgs : LmaOps {
  const float* blob;
  const float* obs;
  const float* eps;
  float* actions;
  float* values;
  float* log_probs;
  float* features;
  int64_t n, row_stride, frame_stride, id_base;
  uint64_t seed, step;
  int32_t K, L, n_layers, n_pi, n_vf, relu, flags, logstd_off, kv_floats, s_floats;
  uint8_t rmap[LMA_MAX_K * (LMA_EMBED / 2)];  // the new token r of k-step s of y[t]
  uint8_t cmap[LMA_MAX_K * (LMA_EMBED / 2)];  // and its k-step of W_2 (column / 2)
};

// The shared pieces below serve the forward kernel (images at row stride POL_ROWS, k / v as each
// lane's own C/D registers) and the backward's recompute (f16_policy_lma_grad.h: images at row
// stride POL_XS): what differs is a template or ordinary parameter, the operations and their order
// are one text, so both kernels round alike.

__device__ __forceinline__ float lma_xor32(const float v) { return v + __shfl_xor(v, 32); }

// img[unit][row] (row stride STRIDE) = or += the accumulator tile
template <int STRIDE, bool ADD>
__device__ __forceinline__ void lma_tile_out(float* img, const pol_f32x16& acc, const int lane) {
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    float* p = img + pol_unit(q, h) * STRIDE + j;
    if (ADD) *p += acc[q];
    else *p = acc[q];
  }
}

// a LayerNorm row's mean and 1 / sqrt(var + eps) over the 32 units (eps 1e-5, the biased variance);
// x: the lane's 16 units less the mean. A lane sums 16 units, the moments are one cross-lane add each.
template <int STRIDE>
__device__ __forceinline__ void lma_ln_stats(const float* z, const int lane, float& mean, float& rstd, float (&x)[16]) {
  const int j = lane & 31, h = lane >> 5;
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    x[i] = z[(16 * h + i) * STRIDE + j];
    s += x[i];
  }
  mean = lma_xor32(s) * (1.0f / 32.0f);
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    x[i] -= mean;
    q += x[i] * x[i];
  }
  rstd = 1.0f / sqrtf(lma_xor32(q) * (1.0f / 32.0f) + 1e-5f);
}

// out[unit][row] = LayerNorm(z[unit][row]), both images at row stride STRIDE
template <int STRIDE>
__device__ __forceinline__ void lma_layernorm(const float* z, const float* __restrict__ w, const float* __restrict__ b,
                                              float* out, const int lane) {
  const int j = lane & 31, h = lane >> 5;
  float x[16], mean, rstd;
  lma_ln_stats<STRIDE>(z, lane, mean, rstd, x);
#pragma unroll
  for (int i = 0; i < 16; ++i) out[(16 * h + i) * STRIDE + j] = x[i] * rstd * w[16 * h + i] + b[16 * h + i];
  __builtin_amdgcn_wave_barrier();
}

// z[unit][row] += acc (the forward's residual update of one token)
__device__ __forceinline__ void lma_residual(float* z, const pol_f32x16& acc, const int lane) {
  __builtin_amdgcn_wave_barrier();
  lma_tile_out<POL_ROWS, true>(z, acc, lane);
  __builtin_amdgcn_wave_barrier();
}

// nn.GELU()'s exact form, and d gelu / dv = Phi(v) + v phi(v)
__device__ __forceinline__ float lma_gelu(const float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }
__device__ __forceinline__ float lma_dgelu(const float v) {
  return 0.5f * (1.0f + erff(v * 0.70710678118654752f)) + v * 0.3989422804014327f * expf(-0.5f * v * v);
}

// ffh[unit][row] = gelu(c_fc(ln))
template <int TOUT>
__device__ __forceinline__ void lma_fc(const float* __restrict__ wb, const PolicyOp op, const float* ln, float* ffh,
                                       const int lane, pol_f32x16 (&acc)[4]) {
  policy_gemm<TOUT>(wb, op, ln, POL_ROWS, lane, acc);
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int to = 0; to < TOUT; ++to) {
#pragma unroll
    for (int r = 0; r < 16; ++r) ffh[(32 * to + pol_unit(r, h)) * POL_ROWS + j] = lma_gelu(acc[to][r]);
  }
  __builtin_amdgcn_wave_barrier();
}

// Where a lane finds k and v of the tokens for its half of a head: dim i of head hd of token b is
// k[b * pitch + hd * head + i * step] (v alike). The forward reads its own C/D registers back
// (step 64, head 256); the backward reads [unit][row] images (step POL_XS, head 8 POL_XS).
struct LmaKV {
  const float* k;
  const float* v;
  int step, head, pitch;
};

// p = softmax(q . k / sqrt(8)) of head hd over the L tokens (q in the C/D registers: lanes l and
// l ^ 32 hold four dims of the head each)
__device__ __forceinline__ void lma_probs(const pol_f32x16& q, const LmaKV kv, const int L, const int hd,
                                          float (&p)[LMA_MAX_L]) {
  float m = -INFINITY;
#pragma unroll
  for (int b = 0; b < LMA_MAX_L; ++b) {
    p[b] = 0.0f;
    if (b < L) {
      const float* kp = kv.k + b * kv.pitch + hd * kv.head;
      float s = q[4 * hd] * kp[0];
      s += q[4 * hd + 1] * kp[kv.step];
      s += q[4 * hd + 2] * kp[2 * kv.step];
      s += q[4 * hd + 3] * kp[3 * kv.step];
      p[b] = lma_xor32(s) * LMA_QK_SCALE;
      m = p[b] > m ? p[b] : m;
    }
  }
  float sum = 0.0f;
#pragma unroll
  for (int b = 0; b < LMA_MAX_L; ++b) {
    if (b < L) {
      p[b] = expf(p[b] - m);
      sum += p[b];
    }
  }
  const float inv = 1.0f / sum;
#pragma unroll
  for (int b = 0; b < LMA_MAX_L; ++b) p[b] *= inv;
}

// ao[unit][row] (row stride STRIDE) = softmax(q . k / sqrt(8)) v of one token
template <int STRIDE>
__device__ __forceinline__ void lma_attention(const pol_f32x16& q, const LmaKV kv, const int L, float* ao, const int lane) {
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int hd = 0; hd < 4; ++hd) {
    float p[LMA_MAX_L];
    lma_probs(q, kv, L, hd, p);
    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int b = 0; b < LMA_MAX_L; ++b) {
      if (b < L) {
        const float* vp = kv.v + b * kv.pitch + hd * kv.head;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] += p[b] * vp[i * kv.step];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) ao[pol_unit(4 * hd + i, h) * STRIDE + j] = o[i];
  }
  __builtin_amdgcn_wave_barrier();
}

// One frame of the tile's rows into xf[feature][row] (row stride POL_XS; lanes 0..31, one row
// each: frame_features of a 15-wide frame, a copy of a 17-wide one; the pad row is the caller's)
// and acc[0..1] = W_e x + b_e. o: the lane's row of the frame.
template <int D>
__device__ __forceinline__ void lma_embed_frame(const float* __restrict__ wb, const PolicyOp we, const float* o, float* xf,
                                                const int lane, pol_f32x16 (&acc)[4]) {
  const int j = lane & 31, h = lane >> 5;
  if (h == 0) {
    if (D == 15) {
      float x[15], y[LMA_FEAT];
#pragma unroll
      for (int d = 0; d < 15; ++d) x[d] = o[d];
      frame_features(x, y);
#pragma unroll
      for (int d = 0; d < LMA_FEAT; ++d) xf[d * POL_XS + j] = y[d];
    } else {
#pragma unroll
      for (int d = 0; d < LMA_FEAT; ++d) xf[d * POL_XS + j] = o[d];
    }
  }
  __builtin_amdgcn_wave_barrier();
  policy_gemm<2>(wb, we, xf, POL_XS, lane, acc);
  __builtin_amdgcn_wave_barrier();
}

template <int D>
__global__ __launch_bounds__(64 * LMA_WAVES) void f16_policy_lma_forward_kernel(const LmaArgs a) {
  extern __shared__ float4 lma_sm4[];
  float* sm = reinterpret_cast<float*>(lma_sm4);
  const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
  const float* wb = a.blob;
  const int L = a.L;
  const int64_t row0 = (int64_t)blockIdx.x * POL_ROWS;
  const int64_t row = row0 + j;
  const int64_t rowc = row < a.n ? row : a.n - 1;  // rows past n - 1 repeat it (always a valid read)
  float* zs = sm;
  float* kv = zs + L * LMA_IMG;
  float* vsh = kv + a.kv_floats;
  float* ln = vsh + POL_ROWS + w * (2 * LMA_IMG + a.s_floats);
  float* ao = ln + LMA_IMG;
  float* S = ao + LMA_IMG;
  pol_f32x16 acc[4];

  // ---- stages 1-4: features, embedding + PE, the stacking permutation folded into W_2
  {
    float* xf = S;
    float* ys = S + LMA_XF;
    pol_f32x16 zacc[LMA_MAX_L];
    const float* b2 = wb + a.w2.b_off;
#pragma unroll
    for (int r = 0; r < LMA_MAX_L; ++r) {
#pragma unroll
      for (int q = 0; q < 16; ++q) zacc[r][q] = w == 0 ? b2[pol_unit(q, h)] : 0.0f;
    }
    if (h == 0) xf[LMA_FEAT * POL_XS + j] = 0.0f;  // the token's own zero-weight pad input
    const float* pe = wb + a.pe_off;
    for (int t = w; t < a.K; t += LMA_WAVES) {
      lma_embed_frame<D>(wb, a.we, a.obs + rowc * a.row_stride + (int64_t)t * a.frame_stride, xf, lane, acc);
#pragma unroll
      for (int to = 0; to < 2; ++to) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int u = 32 * to + pol_unit(q, h);
          const float v = acc[to][q];
          ys[u * POL_ROWS + j] = (v < 0.0f ? 0.0f : v) + pe[t * LMA_EMBED + u];
        }
      }
      __builtin_amdgcn_wave_barrier();
      const float* wp = wb + a.w2.w_off + lane;
      const float* yp = ys + h * POL_ROWS + j;
      const uint8_t* rm = a.rmap + t * (LMA_EMBED / 2);
      const uint8_t* cm = a.cmap + t * (LMA_EMBED / 2);
      for (int s0 = 0; s0 < LMA_EMBED / 2; s0 += 8) {
        float wv[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          wv[u] = wp[cm[s0 + u] * 64];
          b[u] = yp[2 * (s0 + u) * POL_ROWS];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          switch (rm[s0 + u]) {  // (uniform: the accumulator tiles stay in registers)
            case 0: zacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u], b[u], zacc[0], 0, 0, 0); break;
            case 1: zacc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u], b[u], zacc[1], 0, 0, 0); break;
            case 2: zacc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u], b[u], zacc[2], 0, 0, 0); break;
            case 3: zacc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u], b[u], zacc[3], 0, 0, 0); break;
            default: zacc[4] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u], b[u], zacc[4], 0, 0, 0); break;
          }
        }
      }
      __builtin_amdgcn_wave_barrier();  // the next token's images follow every read of this one's
    }
    // z = relu(the waves' partial sums added in wave order): the bits depend on the descriptor alone
    for (int ww = 0; ww < LMA_WAVES; ++ww) {
      if (w == ww) {
#pragma unroll
        for (int r = 0; r < LMA_MAX_L; ++r) {
          if (r < L) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              float* p = zs + r * LMA_IMG + pol_unit(q, h) * POL_ROWS + j;
              float v = zacc[r][q];
              if (ww > 0) v += *p;
              *p = (ww == LMA_WAVES - 1 && v < 0.0f) ? 0.0f : v;
            }
          }
        }
      }
      __syncthreads();
    }
  }

  // ---- the blocks
  for (int layer = 0; layer < a.n_layers; ++layer) {
    const LmaBlockOps B = a.blk[layer];
    // k and v of every token, from the block's input z
    for (int r = w; r < L; r += LMA_WAVES) {
      lma_layernorm<POL_ROWS>(zs + r * LMA_IMG, wb + B.ln1_w, wb + B.ln1_b, ln, lane);
      policy_gemm<2>(wb, B.kv, ln, POL_ROWS, lane, acc);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        kv[(2 * r) * LMA_IMG + q * 64 + lane] = acc[0][q];
        kv[(2 * r + 1) * LMA_IMG + q * 64 + lane] = acc[1][q];
      }
    }
    __syncthreads();
    // z[r] += c_proj(softmax(q[r] . k / sqrt(8)) v)
    const LmaKV own = {kv + lane, kv + LMA_IMG + lane, 64, 4 * 64, 2 * LMA_IMG};  // the lane's C/D registers back
    for (int r = w; r < L; r += LMA_WAVES) {
      lma_layernorm<POL_ROWS>(zs + r * LMA_IMG, wb + B.ln1_w, wb + B.ln1_b, ln, lane);
      policy_gemm<1>(wb, B.q, ln, POL_ROWS, lane, acc);
      __builtin_amdgcn_wave_barrier();
      lma_attention<POL_ROWS>(acc[0], own, L, ao, lane);
      policy_gemm<1>(wb, B.proj, ao, POL_ROWS, lane, acc);
      lma_residual(zs + r * LMA_IMG, acc[0], lane);
    }
    // z[r] += c_proj2(gelu(c_fc(LN2(z[r]))))
    // (token r stays with its wave: no block barrier between the two residual updates)
    float* ffh = S;
    for (int r = w; r < L; r += LMA_WAVES) {
      lma_layernorm<POL_ROWS>(zs + r * LMA_IMG, wb + B.ln2_w, wb + B.ln2_b, ln, lane);
      policy_tiles(B.fc, [&](auto t) { lma_fc<decltype(t)::value>(wb, B.fc, ln, ffh, lane, acc); });
      policy_gemm<1>(wb, B.proj2, ffh, POL_ROWS, lane, acc);
      lma_residual(zs + r * LMA_IMG, acc[0], lane);
    }
    __syncthreads();  // the next block's k / v follow every read of this one's
  }

  // ---- features_out: the flattened z, row-major (n, L 32)
  if (a.features) {
    const int F = L * LMA_DNEW;
    for (int e = tid; e < POL_ROWS * F; e += 64 * LMA_WAVES) {
      const int rj = e / F, f = e - rj * F;
      if (row0 + rj < a.n) a.features[(row0 + rj) * F + f] = zs[f * POL_ROWS + rj];
    }
  }

  // ---- the two MLPs on the features image and the heads, as f16_policy_forward_kernel's (wave 0
  // runs the pi branch, wave 1 the vf branch, each on its own hidden image), then policy_sample
  float* hs = S;
  float mean[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (w < 2 && !(w == 0 && (a.flags & F16_POLICY_VALUE_ONLY))) {
    const int br = w;
    const int base = br * (POL_MAX_LAYERS + 1);
    const int nl = br ? a.n_vf : a.n_pi;
    const float* xin = zs;
    for (int l = 0; l < nl; ++l) {
      const PolicyOp op = a.ops[base + l];
      policy_tiles(op, [&](auto t) { policy_hidden<decltype(t)::value>(wb, op, xin, POL_ROWS, hs, a.relu, lane, acc); });
      xin = hs;
    }
    policy_gemm<1>(wb, a.ops[base + POL_MAX_LAYERS], xin, POL_ROWS, lane, acc);
    __builtin_amdgcn_wave_barrier();
    if (br == 0) {
      mean[0] = acc[0][0]; mean[1] = acc[0][1]; mean[2] = acc[0][2]; mean[3] = acc[0][3];
    } else if (h == 0) {
      vsh[j] = acc[0][0];
    }
  }
  __syncthreads();
  if (w != 0 || h != 0 || row >= a.n) return;
  a.values[row] = vsh[j];
  if (a.flags & F16_POLICY_VALUE_ONLY) return;
  policy_sample(a, wb, row, mean);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static const char* lma_desc_error(const f16_policy_desc* d, const f16_lma_desc* m) {
  if (!m) return "null LMA descriptor";
  if (m->K != d->K || m->D != d->D) return "lma K and D must equal the policy descriptor's";
  if (m->embed_dim != LMA_EMBED) return "lma embed_dim must be 64";
  const int hs = m->heads_stacking;
  if (hs < 1 || LMA_EMBED % hs != 0 || ((LMA_EMBED / hs) & 1)) return "lma heads_stacking must divide embed_dim into an even dk";
  if (m->d_new != LMA_DNEW) return "lma d_new must be 32";
  if (m->heads_latent != 4) return "lma heads_latent must be 4";
  if (m->ff_hidden != 32 && m->ff_hidden != 64 && m->ff_hidden != 96 && m->ff_hidden != 128)
    return "lma ff_hidden must be 32, 64, 96 or 128";
  if (m->n_layers < 0 || m->n_layers > LMA_MAX_LAYERS) return "lma n_layers must be in [0, 3]";
  if (m->L_new < 1 || m->L_new > LMA_MAX_L || m->C_new < 2 || (m->C_new & 1) ||
      (int64_t)m->L_new * m->C_new != (int64_t)m->K * LMA_EMBED)
    return "lma L_new * C_new must equal K * embed_dim (L_new in [1, 5], C_new even)";
  for (int i = 0; i < 6; ++i)
    if (m->reserved[i] != 0) return "lma reserved fields must be zero";
  return nullptr;
}

// f16env_policy_lma_blob_layout: the MLP pieces (first fan-in L_new d_new) and log_std as
// policy_layout places them, then the extractor's pieces (include/f16env.h names the slots)
static int64_t lma_layout(const f16_policy_desc* d, const f16_lma_desc* m, int64_t* off, LmaOps* a) {
  int64_t p = policy_layout(d, off, a ? a->ops : nullptr, m->L_new * m->d_new);
  for (int i = F16_POLICY_N_OFFSETS; i < F16_LMA_N_OFFSETS; ++i) off[i] = -1;
  auto put = [&](int slot, int64_t floats) {
    off[slot] = p;
    p += floats;
    return (int32_t)off[slot];
  };
  const int nks_in = (LMA_FEAT + 1) / 2, nks_d = LMA_DNEW / 2, tff = m->ff_hidden / 32;
  PolicyOp we, w2, q, kv, proj, fc, proj2;
  const int32_t pe = put(F16_LMA_OFF_PE, (int64_t)m->K * LMA_EMBED);
  we.w_off = put(F16_LMA_OFF_WE_W, (LMA_EMBED / 32) * nks_in * 64);
  we.b_off = put(F16_LMA_OFF_WE_B, LMA_EMBED);
  we.nks = nks_in; we.tout = LMA_EMBED / 32;
  w2.w_off = put(F16_LMA_OFF_W2_W, (m->C_new / 2) * 64);
  w2.b_off = put(F16_LMA_OFF_W2_B, LMA_DNEW);
  w2.nks = m->C_new / 2; w2.tout = 1;
  if (a) { a->pe_off = pe; a->we = we; a->w2 = w2; }
  for (int i = 0; i < m->n_layers; ++i) {
    const int s = F16_LMA_OFF_BLOCK0 + F16_LMA_BLOCK_SLOTS * i;
    LmaBlockOps B;
    B.ln1_w = put(s + F16_LMA_BLK_LN1_W, LMA_DNEW);
    B.ln1_b = put(s + F16_LMA_BLK_LN1_B, LMA_DNEW);
    q.w_off = put(s + F16_LMA_BLK_ATTN_W, 3 * nks_d * 64);
    q.b_off = put(s + F16_LMA_BLK_ATTN_B, 3 * LMA_DNEW);
    q.nks = nks_d; q.tout = 1;
    kv.w_off = q.w_off + nks_d * 64; kv.b_off = q.b_off + LMA_DNEW; kv.nks = nks_d; kv.tout = 2;
    proj.w_off = put(s + F16_LMA_BLK_PROJ_W, nks_d * 64);
    proj.b_off = put(s + F16_LMA_BLK_PROJ_B, LMA_DNEW);
    proj.nks = nks_d; proj.tout = 1;
    B.ln2_w = put(s + F16_LMA_BLK_LN2_W, LMA_DNEW);
    B.ln2_b = put(s + F16_LMA_BLK_LN2_B, LMA_DNEW);
    fc.w_off = put(s + F16_LMA_BLK_FC_W, tff * nks_d * 64);
    fc.b_off = put(s + F16_LMA_BLK_FC_B, m->ff_hidden);
    fc.nks = nks_d; fc.tout = tff;
    proj2.w_off = put(s + F16_LMA_BLK_PROJ2_W, (m->ff_hidden / 2) * 64);
    proj2.b_off = put(s + F16_LMA_BLK_PROJ2_B, LMA_DNEW);
    proj2.nks = m->ff_hidden / 2; proj2.tout = 1;
    B.q = q; B.kv = kv; B.proj = proj; B.fc = fc; B.proj2 = proj2;
    if (a) a->blk[i] = B;
  }
  return p;
}

// the stacking permutation: where channel c of y[t] lies in `flat` (heads of dk channels, frames within a head)
static int lma_flat_index(const f16_lma_desc* m, const int t, const int c) {
  const int dk = LMA_EMBED / m->heads_stacking;
  return ((c / dk) * m->K + t) * dk + c % dk;
}

// The block's LDS in floats (the header comment's budget): zs, kv, the value row, and per wave ln,
// ao and the widest phase of S (s_out)
static int64_t lma_lds_floats(const f16_policy_desc* d, const f16_lma_desc* m, int32_t* kv_out, int32_t* s_out) {
  const int max_w = policy_widths(d).max_w;
  int32_t s = LMA_XF + LMA_EMBED * POL_ROWS;
  if (m->n_layers > 0) s = m->ff_hidden * POL_ROWS > s ? m->ff_hidden * POL_ROWS : s;
  s = max_w * POL_ROWS > s ? max_w * POL_ROWS : s;
  const int32_t kv = m->n_layers > 0 ? 2 * m->L_new * LMA_IMG : 0;
  *kv_out = kv;
  *s_out = s;
  return (int64_t)m->L_new * LMA_IMG + kv + POL_ROWS + (int64_t)LMA_WAVES * (2 * LMA_IMG + s);
}

static int policy_lma_forward_impl(void* stream, const f16_policy_desc* desc, const f16_lma_desc* m, const float* blob,
                                   int64_t n, const float* obs, int64_t row_stride, int64_t frame_stride, uint64_t seed,
                                   uint64_t step, int64_t id_base, const float* eps, float* actions, float* values,
                                   float* log_probs, float* features_out, uint32_t flags) {
  if (const char* e = policy_desc_error(desc)) return set_err(-1, e);
  if (const char* e = lma_desc_error(desc, m)) return set_err(-1, e);
  if (int rc = policy_forward_check("f16env_policy_lma_forward", flags, n, blob, obs, row_stride, frame_stride, eps,
                                    actions, values, log_probs, features_out))
    return rc;
  const bool vonly = (flags & F16_POLICY_VALUE_ONLY) != 0;
  LmaArgs a{};
  int64_t off[F16_LMA_N_OFFSETS];
  const int64_t nf = lma_layout(desc, m, off, &a);
  if (nf > 0x7fffffffLL) return set_err(-1, "the blob is too large");
  const int64_t lds = lma_lds_floats(desc, m, &a.kv_floats, &a.s_floats) * 4;
  if (lds > POL_LDS_BYTES) return set_err(-1, "the LMA policy's images do not fit the LDS");
  for (int t = 0; t < m->K; ++t)
    for (int s = 0; s < LMA_EMBED / 2; ++s) {
      const int f = lma_flat_index(m, t, 2 * s);
      a.rmap[t * (LMA_EMBED / 2) + s] = (uint8_t)(f / m->C_new);
      a.cmap[t * (LMA_EMBED / 2) + s] = (uint8_t)(f % m->C_new / 2);
    }
  const void* fn = desc->D == 15 ? (const void*)f16_policy_lma_forward_kernel<15> : (const void*)f16_policy_lma_forward_kernel<17>;
  const int64_t blocks = (n + POL_ROWS - 1) / POL_ROWS;
  if (blocks > 0x7fffffffLL) return set_err(-1, "n too large");
  static uint64_t prepared[2];
  if (int rc = policy_prepare_instance(fn, &prepared[desc->D == 17 ? 1 : 0])) return rc;
  if (n == 0) return 0;
  a.blob = blob; a.obs = obs; a.eps = vonly ? nullptr : eps;
  a.actions = actions; a.values = values; a.log_probs = log_probs; a.features = features_out;
  a.n = n; a.row_stride = row_stride; a.frame_stride = frame_stride; a.id_base = id_base;
  a.seed = seed; a.step = step;
  a.K = m->K; a.L = m->L_new; a.n_layers = m->n_layers;
  a.n_pi = desc->n_pi; a.n_vf = desc->n_vf;
  a.relu = desc->activation == F16_POLICY_ACT_RELU ? 1 : 0;
  a.flags = (int32_t)flags;
  a.logstd_off = (int32_t)off[F16_POLICY_OFF_LOG_STD];
  void* kargs[] = {&a};
  HIPCHK(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(64 * LMA_WAVES), kargs, (size_t)lds, (hipStream_t)stream));
  return 0;
}

}  // namespace f16
