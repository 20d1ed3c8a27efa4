// aa_kernels.hip — MI355X (gfx950) kernels of the decode step behind k_lstm, and the C-ABI of the
// step and greedy decode ("Knowing When to Look"; reference: code_src/models/adaptive_attention.py,
// code_src/models/baseline_attention.py).  See DESIGN.md for the data layout and rooflines; the pack
// and encoder kernels are in aa_encoder.hip, k_lstm in aa_lstm.hpp / aa_lstm.hip.
//
// Kernels (all arithmetic that defines an output is fp32):
//   decode step t (x T)
//     k_lstm          (aa_lstm.hpp) gates = table[tok] + xg + h W_hh^T; LSTM cell; sentinel; the
//                     projection partials; from step 1 on, step t-1's rescoring in the same launch
//     k_atten5        W_g h, W_s s (the partials summed), 49+1 tanh scores, softmax, context, beta mix,
//                     u = c_hat + h     adaptive_attention.py:26-58, 132 (input of mlp)
//                     (k_atten: H = 256 / 768; k_atten5b: an image's beams together)
//     k_vscreen8      bf16 MFMA logits with a rigorous error bound -> per-granule candidate summary
//                     (k_vscreen2 / k_vscreen: the cross-check and the other shapes)
//     fused rescore   exact fp32 logits of the candidates (MFMA-order fma chain) + first-index argmax,
//                     in the next step's k_lstm<.., RS>; the last step's in k_vrescore
//                     adaptive_attention.py:132, 201
//   exact-vocab path (scores output / verification): k_vocab (aa_beam.hip, with the other exact vocab
//                     GEMM k_vexact: fp32 MFMA GEMM + fused argmax) + k_finalize
//   small: k_fill_tok, k_key_ids, k_split_rows, k_logits_at, k_synth_uniform
#include "aa_internal.hpp"
#include "aa_lstm.hpp"

namespace aa {

// Vocab-screen error bound.  For one logit, the fp32 path (k_vocab / k_vrescore) computes
// L = fl(sum_k u_k w_k) + b and the screen computes A = fl(sum_k bf16(u_k) bf16(w_k)) + b (the
// bf16 x bf16 products are exact in fp32).  With du = u - bf16(u), dw = w - bf16(w):
//   sum bf16(u) bf16(w) - sum u w = sum du_k bf16(w_k) + sum u_k dw_k
//   => |.| <= ||du||_2 ||bf16(w)||_2 + ||u||_2 ||dw||_2            (Cauchy-Schwarz, exact reals)
// and both fp32 accumulations add <= gamma_H sum|terms| each (MFMA: gamma_512 ~ 3.1e-5 times
// ||bf16(u)|| ||bf16(w)|| <= (1 + 2^-8)^2 ||u|| ||w||; the rescoring's 8 chains of 64: gamma_67 ~
// 4e-6 ||u|| ||w||).  ||du|| comes from the attention kernel that rounds u (the exact differences,
// Sterbenz), ||dw_n|| from the pack; ||bf16(w)|| <= (1 + 2^-8) ||w||.  The screen applies one bound
// per (row, 32-column granule g):
//   E = SC_BF (||du|| W_g + ||u|| D_g) + SC_ACC(H) ||u|| W_g + EPS_ABS (||u|| W_g + B_g),
//   W_g = max_{n in g} ||w_n||, D_g = max ||dw_n||, B_g = max |b_n|
// SC_BF = 1.005 >= (1 + 2^-8) with the fp32 norms' own rounding (norms inflated at the source);
// SC_ACC(512) = 5e-5 >= 3.1e-5 + 4e-6 with slack (sc_acc below); the EPS_ABS term bounds 2^-17 |A| >= the
// bias-addition roundings plus the < 32-ulp truncation of the screened values that carries the
// arg-max in their low bits (|A| <= ||u|| ||w_n|| (1 + 2^-7) + |b_n|).  The rounding errors are
// about 2^-10 relative on average against the worst case 2^-8 per operand, so E is ~2.5x below the
// Cauchy-Schwarz bound on the worst case used before (0.0085 ||u|| W_g): fewer candidates for the
// exact rescoring (tools/screen_candidates.py: mean 7.2 -> 2.5 per row, 32-column expansions 10x
// rarer).  A column n is a candidate iff A_n + E >= max_m (A_m - E): every column holding the
// exact-fp32 maximum passes, every rejected column is strictly below it.
// SC_ACC depends on H: the MFMA chain's gamma_H (1 + 2^-8)^2 plus the rescoring's
// gamma_{H/8 + 4} (8 chains of H/8, the 3-level tree, the bias) is <= 1.1 (H + H/8 + 8) 2^-24;
// 5e-5 is kept as the floor, so H <= 512 is unchanged (3.8e-5 at H = 512; 5.7e-5 at 768, 7.6e-5
// at 1024).
constexpr float SC_BF = 1.005f;
constexpr float sc_acc(int H) {
  const float g = 1.1f * (float)(H + H / 8 + 8) * 0x1p-24f;
  return g > 5e-5f ? g : 5e-5f;
}
constexpr float EPS_ABS = 1e-5f;
// un = (||u||, ||u - bf16(u)||) of the row, g = (W_g, B_g, D_g, -) of the granule, all inflated at
// their source over their own fp32 rounding
template <int H>
__device__ __forceinline__ float screen_bound(float2 un, float4 g) {
  constexpr float SC_ACC = sc_acc(H);
  const float uw = un.x * g.x;
  return SC_BF * (un.y * g.x + un.x * g.z) + SC_ACC * uw + EPS_ABS * (uw + g.y);
}

__global__ void k_fill_tok(int64_t* __restrict__ tok, int B, int64_t v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) tok[i] = v;
}
__global__ void k_key_ids(const uint64_t* __restrict__ keys, int B, int64_t* __restrict__ ids, int ld) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) ids[(int64_t)i * ld] = key_token(keys[i]);
}

// h [B][H] fp32 -> three bf16 planes in MFMA A-fragment order (see k_lstm); one thread per 8 values.
__global__ void k_split_rows(const float* __restrict__ h, int B, int H, bf16x8* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (m, kc, half)
  const int KC = H / 16;
  if (i >= (int64_t)B * KC * 2) return;
  const int hf = (int)(i & 1), kc = (int)((i >> 1) % KC), m = (int)((i >> 1) / KC);
  const float* src = h + (int64_t)m * H + 16 * kc + 8 * hf;
  bf16x8 p0, p1, p2;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    __bf16 x0, x1, x2;
    split3(src[e], x0, x1, x2);
    p0[e] = x0; p1[e] = x1; p2[e] = x2;
  }
  bf16x8* o = out + ((size_t)((m >> 5) * KC + kc) * 3) * 64 + (m & 31) + 32 * hf;
  o[0] = p0;
  o[64] = p1;
  o[128] = p2;
}

// ---------------------------------------------------------------------------------------------
// D2: adaptive attention, one row per workgroup (Atten.forward, adaptive_attention.py:26-58).
//   hg    = W_g h_t,  ss = W_s s_t  (sum of the LSTM tiles' partials)   (:35, :45)
//   z_k   = w_h . tanh(VWv[k] + hg),  k < 49;  z_s = w_h . tanh(ss + hg)  (:38, :47)
//   alpha = softmax_49(z); beta = softmax_50([z; z_s])[49]              (:39, :51-55)
//   c_t   = sum_k alpha_k V[k];  u = beta s + (1 - beta) c_t + h_t       (:42, :56, :132)
// Also emits bf16(u) and ||u||_2 for the vocab screen.
// ---------------------------------------------------------------------------------------------
// Latency structure: every load that does not depend on alpha is issued up front (this thread's V
// columns, VWv scores operands, h, s, the partial projections), so the kernel pays ~one memory
// latency instead of one per phase.  HPT = H / 256 columns per thread.
// kdiv: rows per image (beam search: the beams of image b are rows b*kdiv .. b*kdiv + kdiv-1 and
// share V / VWv of image b; 1 for the greedy path)
template <int HPT>
__global__ __launch_bounds__(256) void k_atten(int B, int NTL, int kdiv, const float* __restrict__ h_new,
                                               const float* __restrict__ s_new, const float* __restrict__ part,
                                               const float* __restrict__ Vf, const float* __restrict__ VWv,
                                               const float* __restrict__ wh, float* __restrict__ alpha_out,
                                               int64_t alpha_ld, float* __restrict__ beta_out, int64_t beta_ld,
                                               float* __restrict__ u_out, uint16_t* __restrict__ ub_out,
                                               float* __restrict__ unorm, bf16x8* __restrict__ ub3_out) {
  constexpr int H = 256 * HPT;
  __shared__ float proj[PART];
  __shared__ float zs[PP];
  __shared__ float sh_alpha[PP];
  __shared__ float sh_beta;
  __shared__ float sh_norm[8];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int b = blockIdx.x;
  // ---- loads independent of alpha, oldest first in the order they are consumed ------------------
  // (vmcnt retires in issue order: the partial sums wait only for the partials, the scores only
  //  for partials + VWv, while the 98 V values of this thread stay in flight.)  No branches
  //  around loads: out-of-range lanes read clamped addresses and their values are never used.
  constexpr int NT16 = H / 16;  // == NTL
  const int tp = part_col(t < 2 * P ? t : 2 * P - 1);
  float pv[NT16];
  {
    const float* pp = part + (int64_t)b * NT16 * PART + tp;
#pragma unroll
    for (int i = 0; i < NT16; ++i) pv[i] = pp[(int64_t)i * PART];
  }
  const int k = t >> 2, q = t & 3;
  const int kc = k < P ? k : P - 1;
  const int img = kdiv == 1 ? b : b / kdiv;
  const float* vw = VWv + ((int64_t)img * P + kc) * PP;
  float vwr[13], whr[13];
#pragma unroll
  for (int i = 0; i < 13; ++i) {
    const int j = q + 4 * i < P ? q + 4 * i : P - 1;
    vwr[i] = vw[j];
    whr[i] = q + 4 * i < P ? wh[j] : 0.f;  // w_h = 0 for the padding term: fma(0, tanh(.), z) == z
  }
  const float* vb = Vf + (int64_t)img * P * H;
  float vv[HPT][P];
#pragma unroll
  for (int i = 0; i < HPT; ++i)
#pragma unroll
    for (int kk = 0; kk < P; ++kk) vv[i][kk] = vb[(int64_t)kk * H + t + 256 * i];
  float hv[HPT], sv[HPT];
#pragma unroll
  for (int i = 0; i < HPT; ++i) {
    hv[i] = h_new[(int64_t)b * H + t + 256 * i];
    sv[i] = s_new[(int64_t)b * H + t + 256 * i];
  }
  // 1) projections: partials of the H/16 LSTM tiles added in fixed tile order
  {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < NT16; ++i) a += pv[i];
    if (t < 2 * P) proj[t] = a;
  }
  __syncthreads();
  // 2) scores: item k (0..49) by a quad of lanes, j = q + 4i, quad combined in fixed order
  {
    float z = 0.f;
#pragma unroll
    for (int i = 0; i < 13; ++i) {
      const int j = q + 4 * i < P ? q + 4 * i : P - 1;
      const float x = (k < P ? vwr[i] : proj[P + j]) + proj[j];
      z = __builtin_fmaf(whr[i], tanhf(x), z);
    }
    const float z1 = __shfl_xor(z, 1, 64);
    const float z2 = __shfl_xor(z, 2, 64);
    const float z3 = __shfl_xor(z, 3, 64);
    if (q == 0 && k <= P) zs[k] = (z + z1) + (z2 + z3);
  }
  __syncthreads();
  // 3) softmax (wave 0)
  if (w == 0) {
    const float z = lane < P ? zs[lane] : -INFINITY;
    const float zsn = zs[P];
    const float m = wave_max(z);
    const float e = lane < P ? expf(z - m) : 0.f;
    const float S = wave_sum(e);
    const float a = e / S;
    if (lane < P) {
      sh_alpha[lane] = a;
      if (alpha_out) alpha_out[(int64_t)b * alpha_ld + lane] = a;
    }
    const float m2 = fmaxf(m, zsn);
    const float e2 = lane < P ? expf(z - m2) : 0.f;
    const float es = expf(zsn - m2);
    const float S2 = wave_sum(e2) + es;
    if (lane == 0) {
      const float beta = es / S2;
      sh_beta = beta;
      if (beta_out) beta_out[(int64_t)b * beta_ld] = beta;
    }
  }
  __syncthreads();
  // 4) context + u
  const float beta = sh_beta;
  float nsq = 0.f, dsq = 0.f;  // ||u||^2 and ||u - bf16(u)||^2 (the screen's bound)
#pragma unroll
  for (int i = 0; i < HPT; ++i) {
    const int d = t + 256 * i;
    float c = 0.f;
#pragma unroll
    for (int kk = 0; kk < P; ++kk) c = __builtin_fmaf(sh_alpha[kk], vv[i][kk], c);
    const float chat = __builtin_fmaf(beta, sv[i], (1.f - beta) * c);
    const float u = chat + hv[i];
    nsq = __builtin_fmaf(u, u, nsq);
    u_out[(int64_t)b * H + d] = u;
    if (ub_out) {
      const uint16_t ubv = f2bf(u);
      ub_out[frag_off(b, d, H)] = ubv;
      const float du = u - __uint_as_float((uint32_t)ubv << 16);  // exact (Sterbenz)
      dsq = __builtin_fmaf(du, du, dsq);
    }
    if (ub3_out) {  // u as 3 bf16 planes in fragment order (beam search's bf16x3 vocab GEMM)
      __bf16 x0, x1, x2;
      split3(u, x0, x1, x2);
      __bf16* o = reinterpret_cast<__bf16*>(ub3_out + ((size_t)((b >> 5) * (H / 16) + (d >> 4)) * 3) * 64 +
                                            (b & 31) + 32 * ((d >> 3) & 1)) + (d & 7);
      o[0] = x0;
      o[64 * 8] = x1;
      o[128 * 8] = x2;
    }
  }
  if (unorm) {  // [2][B]: ||u||, ||u - bf16(u)||, each inflated over its fp32 rounding (gamma_H < 1e-4)
    nsq = wave_sum(nsq);
    dsq = wave_sum(dsq);
    if (lane == 0) sh_norm[w] = nsq, sh_norm[4 + w] = dsq;
    __syncthreads();
    if (t == 0) {
      unorm[b] = sqrtf((sh_norm[0] + sh_norm[1]) + (sh_norm[2] + sh_norm[3])) * 1.0001f;
      unorm[B + b] = sqrtf((sh_norm[4] + sh_norm[5]) + (sh_norm[6] + sh_norm[7])) * 1.0001f;
    }
  }
}

// The arithmetic of one attention row once its operands are in registers, shared by k_atten5's
// forms with and without the sentinel (the same operations in the same order).  Thread t
// (512 per row): projection group grp = t >> 7, output jp = t & 127 (pv: its H/64 tile partials, tiles
// grp, grp + 4, ...); score item k = t >> 3, lane q = t & 7 (vwr / whr: its 7 terms j = q + 8 i);
// context dimensions t + 512 i (hv, sv; V through vget(i, kk)).  The 32 projection partials are summed
// by the four groups, then (g0 + g1) + (g2 + g3); each of the 50 scores by 8 lanes, xor-butterfly.
struct AttSmem {
  float red[4][128];
  float proj[PART];
  float zs[PP];
  float alpha[PP];
  float norm[16];
  float beta;
};
// SENT = false (the baseline model, baseline_attention.py:78-96,126): only the 49 W_g projections are
// summed, 49 scores, one softmax, u = c_t + h; sv and beta_out are not touched.  alpha comes out of
// the same operations in the same order as with the sentinel (beta does not enter alpha).
template <int H, bool SENT = true, class VG>
__device__ __forceinline__ void atten_row_math(int B, int b, const float (&pv)[H / 64], const float (&vwr)[7],
                                               const float (&whr)[7], const float (&hv)[H / 512],
                                               const float (&sv)[H / 512], VG&& vget, AttSmem& sm,
                                               float* __restrict__ alpha_out, int64_t alpha_ld,
                                               float* __restrict__ beta_out, int64_t beta_ld, float* __restrict__ u_out,
                                               uint16_t* __restrict__ ub_out, float* __restrict__ unorm,
                                               bf16x8* __restrict__ ub3_out) {
  constexpr int DPT = H / 512, NG = H / 64;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int grp = t >> 7, jp = t & 127, k = t >> 3, q = t & 7;
  // 1) projections: tile partials in four fixed groups (tiles grp, grp + 4, ...), groups combined
  {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < NG; ++i) a += pv[i];
    sm.red[grp][jp] = a;
  }
  __syncthreads();
  AA_TS(1, 1);
  if (t < (SENT ? 2 : 1) * P) sm.proj[t] = (sm.red[0][t] + sm.red[1][t]) + (sm.red[2][t] + sm.red[3][t]);
  __syncthreads();
  // 2) scores: item k (0..49) by 8 lanes, j = q + 8i
  {
    float z = 0.f;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const int j = q + 8 * i < P ? q + 8 * i : P - 1;
      float x;
      if constexpr (SENT) x = (k < P ? vwr[i] : sm.proj[P + j]) + sm.proj[j];
      else x = vwr[i] + sm.proj[j];
      z = __builtin_fmaf(whr[i], tanhf(x), z);
    }
    z = z + __shfl_xor(z, 1, 64);
    z = z + __shfl_xor(z, 2, 64);
    z = z + __shfl_xor(z, 4, 64);
    if (q == 0 && k < P + (SENT ? 1 : 0)) sm.zs[k] = z;
  }
  __syncthreads();
  AA_TS(1, 2);
  // 3) softmax (wave 0)
  if (w == 0) {
    const float z = lane < P ? sm.zs[lane] : -INFINITY;
    const float zsn = SENT ? sm.zs[P] : 0.f;
    const float m = wave_max(z);
    const float e = lane < P ? expf(z - m) : 0.f;
    const float S = wave_sum(e);
    const float a = e / S;
    if (lane < P) {
      sm.alpha[lane] = a;
      if (alpha_out) alpha_out[(int64_t)b * alpha_ld + lane] = a;
    }
    if constexpr (SENT) {
      const float m2 = fmaxf(m, zsn);
      const float e2 = lane < P ? expf(z - m2) : 0.f;
      const float es = expf(zsn - m2);
      const float S2 = wave_sum(e2) + es;
      if (lane == 0) {
        const float beta = es / S2;
        sm.beta = beta;
        if (beta_out) beta_out[(int64_t)b * beta_ld] = beta;
      }
    }
  }
  __syncthreads();
  AA_TS(1, 3);
  // 4) context + u
  const float beta = SENT ? sm.beta : 0.f;
  float nsq = 0.f, dsq = 0.f;  // ||u||^2 and ||u - bf16(u)||^2 (the screen's bound)
#pragma unroll
  for (int i = 0; i < DPT; ++i) {
    const int d = t + 512 * i;
    float c = 0.f;
#pragma unroll
    for (int kk = 0; kk < P; ++kk) c = __builtin_fmaf(sm.alpha[kk], vget(i, kk), c);
    float chat = c;  // (no sentinel: c_hat = c_t, baseline_attention.py:122)
    if constexpr (SENT) chat = __builtin_fmaf(beta, sv[i], (1.f - beta) * c);
    const float u = chat + hv[i];
    nsq = __builtin_fmaf(u, u, nsq);
    u_out[(int64_t)b * H + d] = u;
    if (ub_out) {
      const uint16_t ubv = f2bf(u);
      ub_out[frag_off(b, d, H)] = ubv;  // (2-byte: plain)
      const float du = u - __uint_as_float((uint32_t)ubv << 16);  // exact (Sterbenz)
      dsq = __builtin_fmaf(du, du, dsq);
    }
    if (ub3_out) {
      __bf16 x0, x1, x2;
      split3(u, x0, x1, x2);
      __bf16* o = reinterpret_cast<__bf16*>(ub3_out + ((size_t)((b >> 5) * (H / 16) + (d >> 4)) * 3) * 64 +
                                            (b & 31) + 32 * ((d >> 3) & 1)) + (d & 7);
      o[0] = x0;
      o[64 * 8] = x1;
      o[128 * 8] = x2;
    }
  }
  if (unorm) {  // [2][B]: ||u||, ||u - bf16(u)||, each inflated over its fp32 rounding (gamma_H < 1e-4)
    nsq = wave_sum(nsq);
    dsq = wave_sum(dsq);
    if (lane == 0) sm.norm[w] = nsq, sm.norm[8 + w] = dsq;
    __syncthreads();
    if (t == 0) {
      const float* n = sm.norm;
      // (each address is formed before its value: the instruction order the kernel was measured with)
      float* const pu = &unorm[b];
      *pu = sqrtf(((n[0] + n[1]) + (n[2] + n[3])) + ((n[4] + n[5]) + (n[6] + n[7]))) * 1.0001f;
      float* const pd = &unorm[B + b];
      *pd = sqrtf(((n[8] + n[9]) + (n[10] + n[11])) + ((n[12] + n[13]) + (n[14] + n[15]))) * 1.0001f;
    }
  }
  AA_TS(1, 4);
}

// k_atten with two threads per output dimension's worth of parallelism: 512 threads per row, each
// owning H/512 dimensions of the context (half the V registers of k_atten<2>, twice the waves in
// flight per CU), the 32 projection partials summed by four groups of 128 threads (8 each, then
// (g0 + g1) + (g2 + g3)), and each of the 50 scores by 8 lanes (7 terms each, xor-butterfly
// combine).  Same outputs as k_atten; rounding of the projections / scores differs (fixed orders).
// SENT = false: the baseline model's row (atten_row_math<H, false>): the 49 W_g partial columns only,
// s_new and beta_out are not read / written.
template <int H, bool SENT = true>
__global__ __launch_bounds__(512) void k_atten5(int B, int kdiv, const float* __restrict__ h_new,
                                                const float* __restrict__ s_new, const float* __restrict__ part,
                                                const float* __restrict__ Vf, const float* __restrict__ VWv,
                                                const float* __restrict__ wh, float* __restrict__ alpha_out,
                                                int64_t alpha_ld, float* __restrict__ beta_out, int64_t beta_ld,
                                                float* __restrict__ u_out, uint16_t* __restrict__ ub_out,
                                                float* __restrict__ unorm, bf16x8* __restrict__ ub3_out) {
  constexpr int DPT = H / 512, NT16 = H / 16, NG = NT16 / 4;
  __shared__ AttSmem sm;
  AA_TS(1, 0);
  const int t = threadIdx.x;
  const int b = blockIdx.x;
  const int img = kdiv == 1 ? b : b / kdiv;
  // loads, oldest first in the order they are consumed; clamped addresses, no branches
  constexpr int NPJ = (SENT ? 2 : 1) * P;  // projection outputs in use
  const int grp = t >> 7, jp = t & 127, jpc = part_col(jp < NPJ ? jp : NPJ - 1);
  float pv[NG];
  {
    const float* pp = part + ((int64_t)b * NT16 + grp) * PART + jpc;
#pragma unroll
    for (int i = 0; i < NG; ++i) pv[i] = pp[(int64_t)4 * i * PART];
  }
  const int k = t >> 3, q = t & 7;
  const int kc = k < P ? k : P - 1;
  const float* vw = VWv + ((int64_t)img * P + kc) * PP;
  float vwr[7], whr[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int j = q + 8 * i < P ? q + 8 * i : P - 1;
    vwr[i] = vw[j];
    whr[i] = q + 8 * i < P ? wh[j] : 0.f;
  }
  const float* vb = Vf + (int64_t)img * P * H;
  float vv[DPT][P];
  // all of V is issued before the small operands above are waited for (holding part of it back until
  // they had landed measured no better)
#pragma unroll
  for (int i = 0; i < DPT; ++i)
#pragma unroll
    for (int kk = 0; kk < P; ++kk) vv[i][kk] = vb[(int64_t)kk * H + t + 512 * i];
  float hv[DPT], sv[DPT];
#pragma unroll
  for (int i = 0; i < DPT; ++i) {
    hv[i] = h_new[(int64_t)b * H + t + 512 * i];
    if constexpr (SENT) sv[i] = s_new[(int64_t)b * H + t + 512 * i];
    else sv[i] = 0.f;
  }
  atten_row_math<H, SENT>(B, b, pv, vwr, whr, hv, sv, [&](int i, int kk) { return vv[i][kk]; }, sm, alpha_out,
                          alpha_ld, beta_out, beta_ld, u_out, ub_out, unorm, ub3_out);
}

// k_atten5 for beam search: one workgroup per IMAGE runs the KB rows (beams) of that image, so the
// image's V (100 KB) and VWv rows are loaded once instead of once per beam (the rows of an image are
// adjacent: r = img KB + k).  Every row's arithmetic is k_atten5's, in the same order (bit-identical
// alpha, beta, u); the rows' small loads are all issued up front, their phases share the barriers.
template <int H, int KB>
__global__ __launch_bounds__(512) void k_atten5b(const float* __restrict__ h_new, const float* __restrict__ s_new,
                                                 const float* __restrict__ part, const float* __restrict__ Vf,
                                                 const float* __restrict__ VWv, const float* __restrict__ wh,
                                                 float* __restrict__ alpha_out, int64_t alpha_ld,
                                                 float* __restrict__ beta_out, int64_t beta_ld, float* __restrict__ u_out,
                                                 uint16_t* __restrict__ ub_out, float* __restrict__ unorm,
                                                 bf16x8* __restrict__ ub3_out) {
  constexpr int DPT = H / 512, NT16 = H / 16, NG = NT16 / 4;
  __shared__ float red[KB][4][128];
  __shared__ float proj[KB][PART];
  __shared__ float zs[KB][PP];
  __shared__ float sh_alpha[KB][PP];
  __shared__ float sh_beta[KB];
  __shared__ float sh_norm[KB][16];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int img = blockIdx.x, r0 = img * KB;
  const int grp = t >> 7, jp = t & 127, jpc = part_col(jp < 2 * P ? jp : 2 * P - 1);
  float pv[KB][NG];
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    const float* pp = part + ((int64_t)(r0 + r) * NT16 + grp) * PART + jpc;
#pragma unroll
    for (int i = 0; i < NG; ++i) pv[r][i] = pp[(int64_t)4 * i * PART];
  }
  const int k = t >> 3, q = t & 7;
  const int kc = k < P ? k : P - 1;
  const float* vw = VWv + ((int64_t)img * P + kc) * PP;
  float vwr[7], whr[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int j = q + 8 * i < P ? q + 8 * i : P - 1;
    vwr[i] = vw[j];
    whr[i] = q + 8 * i < P ? wh[j] : 0.f;
  }
  const float* vb = Vf + (int64_t)img * P * H;
  float vv[DPT][P];
#pragma unroll
  for (int i = 0; i < DPT; ++i)
#pragma unroll
    for (int kk = 0; kk < P; ++kk) vv[i][kk] = vb[(int64_t)kk * H + t + 512 * i];
  float hv[KB][DPT], sv[KB][DPT];
#pragma unroll
  for (int r = 0; r < KB; ++r)
#pragma unroll
    for (int i = 0; i < DPT; ++i) {
      hv[r][i] = h_new[(int64_t)(r0 + r) * H + t + 512 * i];
      sv[r][i] = s_new[(int64_t)(r0 + r) * H + t + 512 * i];
    }
  // 1) projections
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < NG; ++i) a += pv[r][i];
    red[r][grp][jp] = a;
  }
  __syncthreads();
  for (int e = t; e < KB * 2 * P; e += 512) {
    const int r = e / (2 * P), j = e - r * (2 * P);
    proj[r][j] = (red[r][0][j] + red[r][1][j]) + (red[r][2][j] + red[r][3][j]);
  }
  __syncthreads();
  // 2) scores
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    float z = 0.f;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const int j = q + 8 * i < P ? q + 8 * i : P - 1;
      const float x = (k < P ? vwr[i] : proj[r][P + j]) + proj[r][j];
      z = __builtin_fmaf(whr[i], tanhf(x), z);
    }
    z = z + __shfl_xor(z, 1, 64);
    z = z + __shfl_xor(z, 2, 64);
    z = z + __shfl_xor(z, 4, 64);
    if (q == 0 && k <= P) zs[r][k] = z;
  }
  __syncthreads();
  // 3) softmax: wave r for row r
  if (w < KB) {
    const int r = w, b = r0 + r;
    const float z = lane < P ? zs[r][lane] : -INFINITY;
    const float zsn = zs[r][P];
    const float m = wave_max(z);
    const float e = lane < P ? expf(z - m) : 0.f;
    const float S = wave_sum(e);
    const float a = e / S;
    if (lane < P) {
      sh_alpha[r][lane] = a;
      if (alpha_out) alpha_out[(int64_t)b * alpha_ld + lane] = a;
    }
    const float m2 = fmaxf(m, zsn);
    const float e2 = lane < P ? expf(z - m2) : 0.f;
    const float es = expf(zsn - m2);
    const float S2 = wave_sum(e2) + es;
    if (lane == 0) {
      const float beta = es / S2;
      sh_beta[r] = beta;
      if (beta_out) beta_out[(int64_t)b * beta_ld] = beta;
    }
  }
  __syncthreads();
  // 4) context + u
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    const int b = r0 + r;
    const float beta = sh_beta[r];
    float nsq = 0.f, dsq = 0.f;  // ||u||^2 and ||u - bf16(u)||^2, as k_atten5 (the screen's bound)
#pragma unroll
    for (int i = 0; i < DPT; ++i) {
      const int d = t + 512 * i;
      float c = 0.f;
#pragma unroll
      for (int kk = 0; kk < P; ++kk) c = __builtin_fmaf(sh_alpha[r][kk], vv[i][kk], c);
      const float chat = __builtin_fmaf(beta, sv[r][i], (1.f - beta) * c);
      const float u = chat + hv[r][i];
      nsq = __builtin_fmaf(u, u, nsq);
      u_out[(int64_t)b * H + d] = u;
      if (ub_out) {
        const uint16_t ubv = f2bf(u);
        ub_out[frag_off(b, d, H)] = ubv;
        const float du = u - __uint_as_float((uint32_t)ubv << 16);  // exact (Sterbenz)
        dsq = __builtin_fmaf(du, du, dsq);
      }
      if (ub3_out) {
        __bf16 x0, x1, x2;
        split3(u, x0, x1, x2);
        __bf16* o = reinterpret_cast<__bf16*>(ub3_out + ((size_t)((b >> 5) * (H / 16) + (d >> 4)) * 3) * 64 +
                                              (b & 31) + 32 * ((d >> 3) & 1)) + (d & 7);
        o[0] = x0;
        o[64 * 8] = x1;
        o[128 * 8] = x2;
      }
    }
    if (unorm) {
      nsq = wave_sum(nsq);
      dsq = wave_sum(dsq);
      if (lane == 0) sh_norm[r][w] = nsq, sh_norm[r][8 + w] = dsq;
    }
  }
  if (unorm) {  // [2][B] as k_atten5 writes it (B = the launch's rows: one workgroup per KB rows)
    __syncthreads();
    const int B = gridDim.x * KB;
    if (t < KB) {
      const float* n = sh_norm[t];
      unorm[r0 + t] = sqrtf(((n[0] + n[1]) + (n[2] + n[3])) + ((n[4] + n[5]) + (n[6] + n[7]))) * 1.0001f;
      unorm[B + r0 + t] = sqrtf(((n[8] + n[9]) + (n[10] + n[11])) + ((n[12] + n[13]) + (n[14] + n[15]))) * 1.0001f;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// D3a (greedy path): vocab screen.  bf16 MFMA logits A_n = bf16(u) . bf16(w_n) + b_n over a
// 128x128 tile, then per (row, 32-column granule g) with the granule's bound E (see screen_bound):
//   summ[row][g] = {max_n A_n - E, max_n A_n + E, second largest A_n + E, arg-max column}.
// ---------------------------------------------------------------------------------------------

// One transposing butterfly step: a lane carrying M rows keeps half of them (the upper half if
// bit M of its lane index is set) merged with its partner's copy of the same rows.  Merge: top-2
// of the keys.
template <int M>
__device__ __forceinline__ void screen_bfly(uint32_t (&k1)[16], uint32_t (&k2)[16], int li) {
  const bool hi = (li & M) != 0;
#pragma unroll
  for (int k = 0; k < M / 2; ++k) {
    const uint32_t s1 = hi ? k1[k] : k1[k + M / 2], s2 = hi ? k2[k] : k2[k + M / 2];
    const uint32_t m1 = hi ? k1[k + M / 2] : k1[k], m2 = hi ? k2[k + M / 2] : k2[k];
    const uint32_t r1 = partner<M>(s1), r2 = partner<M>(s2);
    k1[k] = m1 > r1 ? m1 : r1;
    const uint32_t lo = m1 > r1 ? r1 : m1, h2 = m2 > r2 ? m2 : r2;
    k2[k] = lo > h2 ? lo : h2;
  }
}

// Screen tile: 64 rows x 64 columns per 256-thread workgroup.  Both operands are bf16 in
// MFMA-fragment order (u written so by k_atten, W_m at pack time), so wave w loads every fragment
// of its quarter of K -- 2 x 2 blocks x H/64 chunks -- straight into VGPRs in one round trip,
// computes the whole 64x64 tile over that quarter, and the four partial tiles meet in LDS
// ((p0 + p2) + (p1 + p3)); then each wave takes one 32x32 block for the epilogue.  (The screen's
// error bound holds for any fp32 summation order.)
constexpr int SC_BM = 64, SC_BN = 64, SC_PT = 64 * 68;  // partial tile, pitch 68 floats
template <int H>
__global__ __launch_bounds__(256, 2) void k_vscreen(int B, int V, int Vp, const bf16x8* __restrict__ ua,
                                                    const float* __restrict__ unorm, const bf16x8* __restrict__ wf,
                                                    const float4* __restrict__ gs, const float* __restrict__ bias,
                                                    float4* __restrict__ summ) {
  constexpr int KC = H / 16, KW = KC / 4;  // k16 chunks per wave
  __shared__ __attribute__((aligned(16))) float Pt[2 * SC_PT];
  __shared__ float2 un_s[SC_BM];
  const int NTn = Vp / VS_TILE, NTs = Vp / SC_BN, MT = (B + SC_BM - 1) / SC_BM;
  const int L = xcd_remap(blockIdx.x, MT * NTs);
  const int nt = L / MT, mt = L % MT;  // m fastest: a W tile is shared inside an XCD
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int m0 = mt * SC_BM, n0 = nt * SC_BN;
  const bf16x8* a0 = ua + ((size_t)(m0 >> 5) * KC + wave * KW) * 64 + lane;
  const bf16x8* w0 = wf + ((size_t)(n0 >> 5) * KC + wave * KW) * 64 + lane;
  bf16x8 fa[KW][2], fw[KW][2];
#pragma unroll
  for (int c = 0; c < KW; ++c)
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      fa[c][x] = a0[((size_t)x * KC + c) * 64];
      fw[c][x] = w0[((size_t)x * KC + c) * 64];
    }
  // epilogue operands, loaded behind the fragments (their latency hides under the MFMAs)
  const int ur = m0 + (t & 63) < B ? m0 + (t & 63) : B - 1;
  const float2 unv = make_float2(unorm[ur], unorm[B + ur]);
  const int wm = wave >> 1, wn_ = wave & 1;
  const int col = n0 + wn_ * 32 + li;
  const float bv = bias[col];
  const float4 gsv = gs[(n0 + wn_ * 32) / VS_TILE];
  floatx16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;
#pragma unroll
  for (int c = 0; c < KW; ++c)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int x = 0; x < 2; ++x) acc[a][x] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[c][a], fw[c][x], acc[a][x], 0, 0, 0);
  // partial tiles meet in LDS as [col][row] (pitch 68): a lane's 4 consecutive rows are one
  // 16-B access.  Waves 2, 3 -> LDS; waves 0, 1 add them; wave 1 -> LDS; wave 0 adds -> slot 0.
  auto put = [&](float* dst) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
          *reinterpret_cast<float4*>(dst + (x * 32 + li) * 68 + a * 32 + 8 * r4 + 4 * lh) =
              make_float4(acc[a][x][4 * r4], acc[a][x][4 * r4 + 1], acc[a][x][4 * r4 + 2], acc[a][x][4 * r4 + 3]);
  };
  auto add = [&](const float* src) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const float4 v = *reinterpret_cast<const float4*>(src + (x * 32 + li) * 68 + a * 32 + 8 * r4 + 4 * lh);
          acc[a][x][4 * r4] += v.x; acc[a][x][4 * r4 + 1] += v.y;
          acc[a][x][4 * r4 + 2] += v.z; acc[a][x][4 * r4 + 3] += v.w;
        }
  };
  if (wave >= 2) put(Pt + (wave - 2) * SC_PT);
  if (t < SC_BM) un_s[t] = unv;
  __syncthreads();
  if (wave < 2) add(Pt + wave * SC_PT);  // p0 + p2, p1 + p3
  __syncthreads();
  if (wave == 1) put(Pt);
  __syncthreads();
  if (wave == 0) {
    add(Pt);                              // (p0 + p2) + (p1 + p3)
    put(Pt);
  }
  __syncthreads();
  // each wave: one 32x32 block (wm, wn_) of the summed tile, back in MFMA C layout
  floatx16 blk;
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4) {
    const float4 v = *reinterpret_cast<const float4*>(Pt + (wn_ * 32 + li) * 68 + wm * 32 + 8 * r4 + 4 * lh);
    blk[4 * r4] = v.x; blk[4 * r4 + 1] = v.y; blk[4 * r4 + 2] = v.z; blk[4 * r4 + 3] = v.w;
  }
  // epilogue: screened logits A = acc + b -> order-preserving u32 keys whose low 5 bits are replaced
  // by the column's position in its granule (truncation < 32 ulp, covered by EPS_ABS), then per
  // (row, 32-column granule) a transposing butterfly over the 32 lanes that hold the granule's
  // columns (levels 16, 8, 4, 2 each halve the rows a lane carries; level 1 completes): k1 = max
  // key (value and arg-max), k2 = second largest.  The bound E of the granule is applied last.
  const int G0 = (n0 + wn_ * 32) / VS_TILE;
  {
    const int c = 0, a = wm;
    const bool valid = col < V;
    {
      uint32_t k1[16], k2[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t key = order_key(blk[r] + bv);
        k1[r] = valid ? (key & ~31u) | (uint32_t)li : 0u;
        k2[r] = 0u;
      }
      screen_bfly<16>(k1, k2, li);
      screen_bfly<8>(k1, k2, li);
      screen_bfly<4>(k1, k2, li);
      screen_bfly<2>(k1, k2, li);
      const uint32_t r1 = partner<1>(k1[0]), r2 = partner<1>(k2[0]);
      const uint32_t m1 = k1[0] > r1 ? k1[0] : r1;
      const uint32_t lo = k1[0] > r1 ? r1 : k1[0], h2 = k2[0] > r2 ? k2[0] : r2;
      const uint32_t m2 = lo > h2 ? lo : h2;
      const int rr = (li >> 1) & 15;  // this lane pair now holds row acc_row(rr) of the block
      const int rl = a * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
      const int row = m0 + rl;
      if (!(li & 1) && row < B) {
        float4 o = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
        if (m1) {
          const float E = screen_bound<H>(un_s[rl], gsv);
          const float x1 = key_value(m1 & ~31u);
          const float x2 = m2 ? key_value(m2 & ~31u) : -INFINITY;
          o = make_float4(x1 - E, x1 + E, x2 + E, __int_as_float((G0 + c) * VS_TILE + (int)(m1 & 31u)));
        }
        summ[(int64_t)row * NTn + G0 + c] = o;
      }
    }
  }
}

// Screen, wide-tile form (k_vscreen2): one 256-thread workgroup per 128 rows x 160 columns (5
// granules), so at B = 512, V = 10,123 the grid is exactly 256 workgroups (4 row tiles x 64 column
// tiles) and each CU moves 128 + 160 rows x H bf16 = 288 KB from L2 instead of the 64 x 64 form's
// 5 x 128 KB: the 64 x 64 form is bound by those bytes per CU, not by the MFMAs.
//   wave w owns the tile's rows 32w .. 32w+31 and all 5 column blocks (5 accumulators, K not split):
//   its u fragments (its own 32 rows, all of K) go straight to VGPRs in one round trip; the W_m
//   fragments of the 5 column blocks are shared by the 4 waves through LDS, staged in SC2_KS-chunk
//   stages (register prefetch of stage s+1 under the MFMAs of stage s, two LDS buffers, one
//   barrier per stage).  The epilogue is the 64 x 64 form's, per 32 x 32 block.
constexpr int SC2_BM = 128, SC2_NB = 5, SC2_BN = 32 * SC2_NB, SC2_KS = 4;
constexpr int SC2_STAGE = SC2_NB * SC2_KS * 64;  // bf16x8 per LDS stage (20 KB)

// Per (row, granule) summaries of a wave's NB 32 x 32 blocks of screened logits in MFMA C layout (rows
// row0.., columns c0..): keys, transposing top-2 butterfly, bound E, one float4 per row and granule
// (see k_vscreen's epilogue).  Each butterfly level is issued for every block before the next level
// starts: with one wave per SIMD (k_vscreen2's grid is one workgroup per CU) the late levels of one
// block (1 or 2 independent merges) leave the SIMD waiting on DPP and VALU latency; NB blocks side by
// side give each level NB times the independent work.  The top-2 merge is max / med3: the second
// largest of {m1 >= m2, r1 >= r2} is med3(m1, r1, max(m2, r2)).  Same keys, same summaries as
// k_vscreen's epilogue gives per block.
// median of three (the compiler emits v_med3_u32 for this pattern)
__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  const uint32_t t = hi < c ? hi : c;
  return lo > t ? lo : t;
}

template <int M>
__device__ __forceinline__ void screen_bfly_m3(uint32_t (&k1)[16], uint32_t (&k2)[16], int li) {
  const bool hi = (li & M) != 0;
#pragma unroll
  for (int k = 0; k < M / 2; ++k) {
    const uint32_t s1 = hi ? k1[k] : k1[k + M / 2], s2 = hi ? k2[k] : k2[k + M / 2];
    const uint32_t m1 = hi ? k1[k + M / 2] : k1[k], m2 = hi ? k2[k + M / 2] : k2[k];
    const uint32_t r1 = partner<M>(s1), r2 = partner<M>(s2);
    const uint32_t h2 = m2 > r2 ? m2 : r2;
    k1[k] = m1 > r1 ? m1 : r1;
    k2[k] = umed3(m1, r1, h2);
  }
}

// First level (M = 16, every k2 still 0) by v_permlane16_swap (gfx950): swapping the odd 16-lane
// rows of k1[k] with the even rows of k1[k + 8] leaves each lane holding its own key and its
// partner's (lane ^ 16) for exactly the row it keeps (k on the low half, k + 8 on the high half),
// so the level needs no selects and no ds_swizzle; top-2 of two keys = max / min.
__device__ __forceinline__ void screen_bfly16_swap(uint32_t (&k1)[16], uint32_t (&k2)[16]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const auto r = __builtin_amdgcn_permlane16_swap(k1[k], k1[k + 8], false, false);
    k1[k] = r[0] > r[1] ? r[0] : r[1];
    k2[k] = r[0] > r[1] ? r[1] : r[0];
  }
}

template <int H, int NB>
__device__ __forceinline__ void screen_blocks_summ(const floatx16 (&acc)[NB], int row0, int G0, const float (&bv)[NB],
                                                   const float4* __restrict__ gsb, const float2* __restrict__ un_blk,
                                                   int c0, int V, int B, int NTn, float4* __restrict__ summ) {
  const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  uint32_t k1[NB][16], k2[NB][16];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const bool valid = c0 + 32 * b + li < V;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t key = order_key(acc[b][r] + bv[b]);
      k1[b][r] = valid ? (key & ~31u) | (uint32_t)li : 0u;
      k2[b][r] = 0u;
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) screen_bfly16_swap(k1[b], k2[b]);
#pragma unroll
  for (int b = 0; b < NB; ++b) screen_bfly_m3<8>(k1[b], k2[b], li);
#pragma unroll
  for (int b = 0; b < NB; ++b) screen_bfly_m3<4>(k1[b], k2[b], li);
#pragma unroll
  for (int b = 0; b < NB; ++b) screen_bfly_m3<2>(k1[b], k2[b], li);
  const int rr = (li >> 1) & 15;  // this lane pair now holds row acc_row(rr) of each block
  const int rl = (rr & 3) + 8 * (rr >> 2) + 4 * lh;
  const int row = row0 + rl;
  const float2 uw0 = un_blk[rl];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const uint32_t r1 = partner<1>(k1[b][0]), r2 = partner<1>(k2[b][0]);
    const uint32_t m1 = k1[b][0] > r1 ? k1[b][0] : r1;
    const uint32_t h2 = k2[b][0] > r2 ? k2[b][0] : r2;
    const uint32_t m2 = umed3(k1[b][0], r1, h2);
    if (!(li & 1) && row < B) {
      float4 o = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
      if (m1) {
        const float E = screen_bound<H>(uw0, gsb[b]);
        const float x1 = key_value(m1 & ~31u);
        const float x2 = m2 ? key_value(m2 & ~31u) : -INFINITY;
        o = make_float4(x1 - E, x1 + E, x2 + E, __int_as_float((G0 + b) * VS_TILE + (int)(m1 & 31u)));
      }
      summ[(int64_t)row * NTn + G0 + b] = o;
    }
  }
}

// Main loop of the wide screen on NT threads: the tile's screened products acc[b] = bf16(u) . bf16(w) of
// the wave's 32 rows (row block wave & 3) x column blocks b0 .. b0 + NBW - 1 (no bias), and, staged in
// LDS for the epilogue, un_s = ||u|| of the tile's 128 rows and gs_s = the 5 granules' bound factors
// (no global loads inside the epilogue, no registers held across the loop).
template <int H, int NT, int NBW, bool RING3>
__device__ __forceinline__ void screen_main(int B, int m0, int n0, int b0, const bf16x8* __restrict__ ua,
                                            const float* __restrict__ unorm, const bf16x8* __restrict__ wf,
                                            bf16x8 (*Ws)[SC2_STAGE], float2* un_s, floatx16 (&acc)[NBW],
                                            const float4* __restrict__ gs, float4* gs_s) {
  constexpr int KC = H / 16, NS = KC / SC2_KS, PER = (SC2_STAGE + NT - 1) / NT;  // bf16x8 per thread per stage
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // this wave's u fragments and the W stages arrive two stages ahead in register rings instead of all
  // KC chunks at once, so the kernel fits in 256 registers and 40 KB of LDS.  Two stages ahead hide
  // more of the L2 latency than one (k_vscreen2 16.4 -> 15.5 us in A/B); three cost more in registers
  // than they hide.
  const bf16x8* a0 = ua + (size_t)((m0 >> 5) + (wave & 3)) * KC * 64 + lane;
  // stages in flight ahead of the one multiplied: W in registers (RW slots), u fragments (RU slots)
  constexpr int AH = 2 < NS ? 2 : NS, RW = AH, RU = AH + 1;
  bf16x8 fa[RU][SC2_KS];
  auto uload = [&](int s, int slot) {
#pragma unroll
    for (int c = 0; c < SC2_KS; ++c) fa[slot][c] = a0[(size_t)(s * SC2_KS + c) * 64];
  };
  // W stage s: for column block b (0..4), chunks [s KS, (s+1) KS) are one contiguous 8 KB run of the
  // fragment-order W_m; thread t moves bf16x8 j = t + NT i of the stage (b = j / (KS*64)).
  const bf16x8* wbase = wf + (size_t)(n0 >> 5) * KC * 64;
  bf16x8 wr[RW][PER];
  auto gload = [&](int s, int slot) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int j = t + NT * i;
      if (PER * NT == SC2_STAGE || j < SC2_STAGE) {  // (wave-uniform)
        const int b = j / (SC2_KS * 64), r = j - b * (SC2_KS * 64);
        wr[slot][i] = wbase[((size_t)b * KC + s * SC2_KS) * 64 + r];
      }
    }
  };
  auto lstore = [&](int buf, int slot) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int j = t + NT * i;
      if (PER * NT == SC2_STAGE || j < SC2_STAGE) Ws[buf][j] = wr[slot][i];
    }
  };
#pragma unroll
  for (int s = 0; s < AH; ++s) uload(s, s);
#pragma unroll
  for (int b = 0; b < NBW; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
#pragma unroll
  for (int s = 0; s < AH; ++s) gload(s, s);
  // epilogue operands, loaded behind the first stages' fragments (storing them to LDS waits for
  // those stages, which the first MFMAs wait for anyway)
  if (t < SC2_BM) {
    const int r = m0 + t;
    un_s[t] = make_float2(unorm[r < B ? r : B - 1], unorm[B + (r < B ? r : B - 1)]);
  } else if (t < SC2_BM + SC2_NB) {
    gs_s[t - SC2_BM] = gs[n0 / VS_TILE + t - SC2_BM];
  }
  if constexpr (RING3) {
    // three LDS buffers: stage s + 1's W is stored in the middle of stage s's MFMAs (its
    // buffer was last read in stage s - 2, before this stage's barrier), so the store's latency is off
    // the barrier -> read -> MFMA path; one barrier per stage.  10.1 -> 9.7 us, sequential decode
    // +0.7 % (A/B, profiles/r06i_screen_ring3_ab.txt); four stages ahead of the W / u loads: no gain
    lstore(0, 0);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      __syncthreads();
      if (s + AH < NS) {
        gload(s + AH, (s + AH) % RW);
        uload(s + AH, (s + AH) % RU);
      }
      const bf16x8* ws = Ws[s % 3] + lane;
#pragma unroll
      for (int c = 0; c < SC2_KS; ++c) {
        if (c == SC2_KS / 2 && s + 1 < NS) lstore((s + 1) % 3, (s + 1) % RW);
#pragma unroll
        for (int b = 0; b < NBW; ++b) {
          const bf16x8 w = ws[((b0 + b) * SC2_KS + c) * 64];
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s % RU][c], w, acc[b], 0, 0, 0);
        }
      }
    }
  } else {
    // two LDS buffers: stage s's W is stored, then one barrier, then its MFMAs
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      lstore(s & 1, s % RW);
      if (s + AH < NS) {
        gload(s + AH, s % RW);
        uload(s + AH, (s + AH) % RU);
      }
      __syncthreads();
      const bf16x8* ws = Ws[s & 1] + lane;
#pragma unroll
      for (int c = 0; c < SC2_KS; ++c) {
#pragma unroll
        for (int b = 0; b < NBW; ++b) {
          const bf16x8 w = ws[((b0 + b) * SC2_KS + c) * 64];
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s % RU][c], w, acc[b], 0, 0, 0);
        }
      }
    }
  }
}

template <int H>
__global__ __launch_bounds__(256, 2) void k_vscreen2(int B, int V, int Vp, const bf16x8* __restrict__ ua,
                                                  const float* __restrict__ unorm, const bf16x8* __restrict__ wf,
                                                  const float4* __restrict__ gs, const float* __restrict__ bias,
                                                  float4* __restrict__ summ) {
  __shared__ __attribute__((aligned(16))) bf16x8 Ws[2][SC2_STAGE];
  __shared__ float2 un_s[SC2_BM];
  __shared__ float4 gs_s[SC2_NB];
  AA_TS(2, 0);
  const int NTn = Vp / VS_TILE, NT = Vp / SC2_BN, MT = (B + SC2_BM - 1) / SC2_BM;
  const int L = xcd_remap(blockIdx.x, MT * NT);
  const int nt = L / MT, mt = L % MT;  // m fastest: a W tile is shared inside an XCD
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31;
  const int m0 = mt * SC2_BM, n0 = nt * SC2_BN;
  float bvs[SC2_NB];
#pragma unroll
  for (int b = 0; b < SC2_NB; ++b) bvs[b] = bias[n0 + 32 * b + li];
  floatx16 acc[SC2_NB];
  screen_main<H, 256, SC2_NB, false>(B, m0, n0, 0, ua, unorm, wf, Ws, un_s, acc, gs, gs_s);
  AA_TS(2, 1);
  const int row0 = m0 + 32 * wave;
  screen_blocks_summ<H, SC2_NB>(acc, row0, n0 / VS_TILE, bvs, gs_s, un_s + 32 * wave, n0, V, B, NTn, summ);
  AA_TS(2, 2);
}

// The wide screen on 512 threads (k_vscreen8, the default): the same 128 x 160 tile, W stages and
// per-block products, but two waves per row block -- wave w < 4 takes column blocks 0..2 of rows
// 32 w.., wave w + 4 blocks 3..4 of the same rows -- so each SIMD holds two waves (one of each group)
// whose MFMA chains and LDS reads interleave, where k_vscreen2's single wave per SIMD waited on every
// LDS read (41 % of wave cycles waiting).  Every block accumulates its chunks in the
// same order, so the summaries are k_vscreen2's bit for bit.
constexpr int SC8_NT = 512, SC8_NA = 3, SC8_NBB = SC2_NB - SC8_NA;  // threads; blocks of group 0 / 1
template <int H, int NBW>
__device__ __forceinline__ void screen8_group(int B, int V, int m0, int n0, int b0, int NTn,
                                              const bf16x8* __restrict__ ua, const float* __restrict__ unorm,
                                              const bf16x8* __restrict__ wf, const float4* __restrict__ gs,
                                              const float* __restrict__ bias, float4* __restrict__ summ,
                                              bf16x8 (*Ws)[SC2_STAGE], float2* un_s, float4* gs_s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31;
  float bvs[NBW];
#pragma unroll
  for (int b = 0; b < NBW; ++b) bvs[b] = bias[n0 + 32 * (b0 + b) + li];
  floatx16 acc[NBW];
  screen_main<H, SC8_NT, NBW, true>(B, m0, n0, b0, ua, unorm, wf, Ws, un_s, acc, gs, gs_s);
  AA_TS(2, 1);
  const int row0 = m0 + 32 * (wave & 3);
  screen_blocks_summ<H, NBW>(acc, row0, n0 / VS_TILE + b0, bvs, gs_s + b0, un_s + 32 * (wave & 3), n0 + 32 * b0, V, B,
                             NTn, summ);
}
template <int H>
__global__ __launch_bounds__(SC8_NT) void k_vscreen8(int B, int V, int Vp, const bf16x8* __restrict__ ua,
                                                     const float* __restrict__ unorm, const bf16x8* __restrict__ wf,
                                                     const float4* __restrict__ gs, const float* __restrict__ bias,
                                                     float4* __restrict__ summ) {
  __shared__ __attribute__((aligned(16))) bf16x8 Ws[3][SC2_STAGE];
  __shared__ float2 un_s[SC2_BM];
  __shared__ float4 gs_s[SC2_NB];
  AA_TS(2, 0);
  const int NTn = Vp / VS_TILE, NT = Vp / SC2_BN, MT = (B + SC2_BM - 1) / SC2_BM;
  const int L = xcd_remap(blockIdx.x, MT * NT);
  const int nt = L / MT, mt = L % MT;  // m fastest: a W tile is shared inside an XCD
  const int m0 = mt * SC2_BM, n0 = nt * SC2_BN;
  // The two groups run different instantiations of the main loop and the epilogue, each with its own
  // __syncthreads() calls (the same number on both sides).  This relies on the hardware barrier
  // counting the workgroup's waves whichever code path each arrives from; AA_DECODE_SCREEN4's bitwise
  // test against k_vscreen2 is the guard.
  if (threadIdx.x < 256)  // (wave-uniform) column blocks 0..2
    screen8_group<H, SC8_NA>(B, V, m0, n0, 0, NTn, ua, unorm, wf, gs, bias, summ, Ws, un_s, gs_s);
  else                    // column blocks 3..4
    screen8_group<H, SC8_NBB>(B, V, m0, n0, SC8_NA, NTn, ua, unorm, wf, gs, bias, summ, Ws, un_s, gs_s);
  AA_TS(2, 2);
}

template <int H>
__global__ __launch_bounds__(RS_NT) void k_vrescore(int B, int V, int Vp, const float* __restrict__ u,
                                                  const float4* __restrict__ summ, const float* __restrict__ W,
                                                  const float* __restrict__ bias, uint64_t* __restrict__ keys,
                                                  int64_t* __restrict__ ids, int T, int t_step) {
  __shared__ __attribute__((aligned(16))) float scr[RsScratch<H>::FLOATS];
  AA_TS(3, 0);
  rescore_row<H, false>(blockIdx.x, true, threadIdx.x, V, Vp, u, summ, W, bias, keys, ids, T, t_step, scr);
  AA_TS(3, 3);
}

// ---------------------------------------------------------------------------------------------
// Exact fp32 logits of selected columns (cols [B][n], -1 = skip) -> out [B][n]; same arithmetic.
__global__ __launch_bounds__(256) void k_logits_at(int H, int V, const float* __restrict__ u, const int32_t* __restrict__ cols,
                                                   int n, const float* __restrict__ W, const float* __restrict__ bias,
                                                   float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float urow[MAX_H];
  const int b = blockIdx.x, t = threadIdx.x;
  for (int d = 4 * t; d < H; d += 1024) *reinterpret_cast<float4*>(&urow[d]) = *reinterpret_cast<const float4*>(u + (int64_t)b * H + d);
  __syncthreads();
  const int g = t >> 3, lane8 = t & 7;
  for (int i = g; i < n; i += 32) {
    const int c = cols[(int64_t)b * n + i];
    const bool ok = c >= 0 && c < V;
    const int col = ok ? c : 0;
    const float x = exact_logit8(urow, W + (int64_t)col * H, H, bias[col], lane8);
    if (lane8 == 0) out[(int64_t)b * n + i] = ok ? x : 0.f;
  }
}

// ids [B][T] from the argmax keys [T][ldk] (ldk = the whole batch when B is a lane's row block)
__global__ void k_finalize(const uint64_t* __restrict__ keys, int B, int T, int64_t* __restrict__ ids, int ldk) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T) return;
  const int b = (int)(i / T), t = (int)(i % T);
  ids[i] = key_token(keys[(int64_t)t * ldk + b]);
}

__global__ void k_synth_uniform(float* __restrict__ dst, int64_t n, uint64_t key, int64_t start, double lo, double span, int plain) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t z = splitmix(key + (uint64_t)(start + i + 1) * GOLDEN);
    const double u = (double)(z >> 40) * (1.0 / 16777216.0);
    dst[i] = plain ? (float)u : (float)__dadd_rn(lo, __dmul_rn(span, u));
  }
}

}  // namespace aa

// =============================================================================================
// C-ABI  (exported functions get C linkage and default visibility from adaptive_amd.h)
// =============================================================================================
using namespace aa;


int aa_abi_version(void) { return AA_ABI_VERSION; }
#ifdef AA_TS_ENABLE
namespace aa {
template <int H>
int ts_set_lstm(void* buf);  // aa_lstm.hip: each k_lstm object's copy of the pointer
}
extern "C" __attribute__((visibility("default"))) int aa_ts_setup(void* buf) {
  int rc = ts_set_local(buf);
  if (!rc) rc = ts_set_lstm<256>(buf);
  if (!rc) rc = ts_set_lstm<512>(buf);
  if (!rc) rc = ts_set_lstm<768>(buf);
  if (!rc) rc = ts_set_lstm<1024>(buf);
  return rc;
}
#endif

const char* aa_error_string(int code) {
  switch (code) {
    case AA_OK: return "ok";
    case AA_ERR_NULL: return "a required pointer is NULL";
    case AA_ERR_DIMS: return "unsupported model dimensions (need embed%32==0, hidden%256==0, hidden<=1024, vocab>=1, channels%64==0, spatial==49)";
    case AA_ERR_SHAPE: return "bad batch size or step count";
    case AA_ERR_BUFFER: return "packed-weight or workspace buffer too small";
    case AA_ERR_ALIGN: return "a device pointer is not 16-byte aligned";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
  }
}

int aa_check_dims(const aa_dims* d) {
  if (!d) return AA_ERR_NULL;
  if (d->embed <= 0 || d->embed % 32 || d->hidden <= 0 || d->hidden % 256 || d->hidden > MAX_H || d->vocab < 1 ||
      d->channels <= 0 || d->channels % 64 || d->spatial != P)
    return AA_ERR_DIMS;
  return AA_OK;
}

size_t aa_packed_bytes(const aa_dims* d) {
  if (aa_check_dims(d) != AA_OK) return 0;
  return make_layout(*d).total_floats * sizeof(float);
}



// (the one-step API's workspace is not made of EncWS / RowWS: V, v_g, h and c are the caller's, and
// it holds one split-h buffer)
struct StepWS {
  float *xg, *s, *u, *vwv, *part;
  bf16x8* hsp;
  uint64_t* keys;
  int64_t* tok0;
};
static StepWS carve_step(char* base, const Layout& L, int B, size_t* bytes) {
  Carver c{base};
  StepWS w;
  w.xg = c.take<float>((size_t)B * L.N5);
  w.s = c.take<float>((size_t)B * L.H);
  w.u = c.take<float>((size_t)B * L.H);
  w.vwv = c.take<float>((size_t)B * P * PP);
  w.part = c.take<float>((size_t)B * (L.H / 16) * PART);
  w.hsp = c.take<bf16x8>(hsp_frags(L, B));
  w.keys = c.take<uint64_t>((size_t)B);
  w.tok0 = c.take<int64_t>((size_t)B);
  *bytes = c.off;
  return w;
}

struct DecodeWS {
  EncWS e;
  RowWS r;
  float* unorm;
  uint16_t* ub;
  float4* summ;
  uint64_t* keys;
  int64_t* tok0;
};
static DecodeWS carve_decode(char* base, const Layout& L, int B, int T, size_t* bytes) {
  Carver c{base};
  DecodeWS w;
  w.e = carve_enc(c, L, B);
  w.r = carve_rows(c, L, B);
  w.unorm = c.take<float>((size_t)2 * B);  // ||u|| then ||u - bf16(u)|| per row
  w.ub = c.take<uint16_t>((size_t)((B + 127) / 128) * 128 * L.H);  // fragment order, 128-row tiles
  w.summ = c.take<float4>((size_t)B * (L.Vp / VS_TILE));
  w.keys = c.take<uint64_t>((size_t)T * B);
  w.tok0 = c.take<int64_t>((size_t)B);
  *bytes = c.off;
  return w;
}

size_t aa_step_workspace_bytes(const aa_dims* d, int32_t B) {
  if (aa_check_dims(d) != AA_OK || B < 0) return 0;
  size_t n;
  carve_step(nullptr, make_layout(*d), B, &n);
  return n;
}

size_t aa_decode_workspace_bytes(const aa_dims* d, int32_t B, int32_t T) {
  if (aa_check_dims(d) != AA_OK || B < 0 || T < 0) return 0;
  size_t n;
  carve_decode(nullptr, make_layout(*d), B, T, &n);
  return n;
}


namespace aa {

// LSTM step: the object of the model's hidden size launches its k_lstm form (aa_lstm.hip)
void lstm_launch(const Layout& L, const MP& p, const StepIO& io, hipStream_t s) {
  aa_for_hidden(L.H, [&](auto h) { lstm_launch_h<h.value>(L, p, io, s); });
}

// Attention for one step (io.kdiv rows per image: beam search; k_atten5b runs an image's rows together)
void atten_launch(const Layout& L, const MP& p, const StepIO& io, hipStream_t s) {
  const int H = L.H, B = io.B, kdiv = io.kdiv;
  const float *h = io.h_out, *sb = io.s, *pt = io.part;
  if (io.base) {  // the baseline model's row (H = 512, one row per image): s and beta are not touched
    AA_TLAUNCH(io.atten_ev, io.ei, (k_atten5<512, false>), dim3(B), dim3(512), 0, s, B, kdiv, h, sb, pt, io.V, io.vwv,
               p.wh, io.alpha, io.alpha_ld, (float*)nullptr, io.beta_ld, io.u, io.ub, io.unorm, io.ub3);
    return;
  }
#define AA_ATTEN_TAIL h, sb, pt, io.V, io.vwv, p.wh, io.alpha, io.alpha_ld, io.beta, io.beta_ld, io.u, io.ub, io.unorm, io.ub3
#define AA_ATTEN(HPT_) \
  AA_TLAUNCH(io.atten_ev, io.ei, k_atten<HPT_>, dim3(B), dim3(256), 0, s, B, H / 16, kdiv, AA_ATTEN_TAIL)
#define AA_ATTEN5(H_) AA_TLAUNCH(io.atten_ev, io.ei, k_atten5<H_>, dim3(B), dim3(512), 0, s, B, kdiv, AA_ATTEN_TAIL)
#define AA_ATTEN5B(KB_) \
  AA_TLAUNCH(io.atten_ev, io.ei, (k_atten5b<512, KB_>), dim3(B / KB_), dim3(512), 0, s, AA_ATTEN_TAIL)
  if (H == 512 && kdiv >= 2 && kdiv <= 5 && B % kdiv == 0) {  // beam: one workgroup per image
    switch (kdiv) {
      case 2: AA_ATTEN5B(2); break;
      case 3: AA_ATTEN5B(3); break;
      case 4: AA_ATTEN5B(4); break;
      default: AA_ATTEN5B(5); break;
    }
    return;
  }
  switch (H) {
    case 256: AA_ATTEN(1); break;
    case 512: AA_ATTEN5(512); break;
    case 768: AA_ATTEN(3); break;
    default: AA_ATTEN5(1024); break;
  }
#undef AA_ATTEN
#undef AA_ATTEN5
#undef AA_ATTEN5B
#undef AA_ATTEN_TAIL
}

// LSTM + attention for one step
void lstm_atten_launch(const Layout& L, const MP& p, const StepIO& io, hipStream_t s) {
  lstm_launch(L, p, io, s);
  atten_launch(L, p, io, s);
}

void split_rows_launch(const float* h, int B, int H, bf16x8* out, hipStream_t s) {
  hipLaunchKernelGGL(k_split_rows, dim3((unsigned)(((int64_t)B * (H / 8) + 255) / 256)), dim3(256), 0, s, h, B, H, out);
}
void fill_tok_launch(int64_t* tok, int B, int64_t v, hipStream_t s) {
  hipLaunchKernelGGL(k_fill_tok, dim3((B + 255) / 256), dim3(256), 0, s, tok, B, v);
}

}  // namespace aa

// The no-sentinel kernels exist for the reference's base_lstm_hidden_size only (k_atten5<512>'s path).
static bool baseline_ok(const Layout& L) { return L.H == 512; }

// aa_decode_step / aa_baseline_decode_step (base: the no-sentinel kernels, beta unused)
static int step_impl(const aa_model* m, int32_t B, const int64_t* tokens_in, const float* V, const float* VWv,
                     const float* v_g, const float* h_in, const float* c_in, float* h_out, float* c_out, float* scores,
                     int64_t* tokens_out, float* alpha, float* beta, void* workspace, size_t workspace_bytes,
                     aa_stream_t stream, bool base) {
  Layout L;
  int rc = check_model(m, &L);
  if (rc) return rc;
  if (base && !baseline_ok(L)) return AA_ERR_DIMS;
  if (B < 0) return AA_ERR_SHAPE;
  if (B == 0) return AA_OK;
  if (!V || !v_g || !h_in || !c_in || !h_out || !c_out || !tokens_out || !workspace) return AA_ERR_NULL;
  if (!al16(V) || !al16(VWv) || !al16(v_g) || !al16(h_in) || !al16(c_in) || !al16(h_out) || !al16(c_out) ||
      !al16(workspace))
    return AA_ERR_ALIGN;
  size_t need;
  StepWS w = carve_step(static_cast<char*>(workspace), L, B, &need);
  if (workspace_bytes < need) return AA_ERR_BUFFER;
  hipStream_t s = (hipStream_t)stream;
  const MP p = resolve(m, L);
  if (!VWv) {
    gemm_bias(V, L.H, B * P, p.wv, L.H, PP, L.H, nullptr, w.vwv, PP, s);
    VWv = w.vwv;
  }
  gemm_bias(v_g, L.E, B, p.wvg, L.E, L.N5, L.E, p.bias5, w.xg, L.N5, s);
  AA_TRY(hipMemsetAsync(w.keys, 0, (size_t)B * sizeof(uint64_t), s));
  split_rows_launch(h_in, B, L.H, w.hsp, s);
  const int64_t* tok = tokens_in;
  if (!tok) {
    fill_tok_launch(w.tok0, B, 1, s);  // <start>
    tok = w.tok0;
  }
  lstm_atten_launch(L, p,
                    {.B = B, .tok = tok, .V = V, .vwv = VWv, .xg = w.xg, .hsp_in = w.hsp, .c_in = c_in, .h_out = h_out,
                     .c_out = c_out, .s = w.s, .part = w.part, .u = w.u, .alpha = alpha, .beta = beta, .base = base},
                    s);
  vocab_launch(L, p, B, w.u, scores, L.V, w.keys, s);
  hipLaunchKernelGGL(k_finalize, dim3((B + 255) / 256), dim3(256), 0, s, w.keys, B, 1, tokens_out, B);
  return launch_status();
}

int aa_decode_step(const aa_model* m, int32_t B, const int64_t* tokens_in, const float* V, const float* VWv,
                   const float* v_g, const float* h_in, const float* c_in, float* h_out, float* c_out, float* scores,
                   int64_t* tokens_out, float* alpha, float* beta, void* workspace, size_t workspace_bytes,
                   aa_stream_t stream) {
  return step_impl(m, B, tokens_in, V, VWv, v_g, h_in, c_in, h_out, c_out, scores, tokens_out, alpha, beta, workspace,
                   workspace_bytes, stream, false);
}

int aa_baseline_decode_step(const aa_model* m, int32_t B, const int64_t* tokens_in, const float* V, const float* VWv,
                            const float* v_g, const float* h_in, const float* c_in, float* h_out, float* c_out,
                            float* scores, int64_t* tokens_out, float* alpha, void* workspace, size_t workspace_bytes,
                            aa_stream_t stream) {
  return step_impl(m, B, tokens_in, V, VWv, v_g, h_in, c_in, h_out, c_out, scores, tokens_out, alpha, nullptr,
                   workspace, workspace_bytes, stream, true);
}

// wide vocab-screen tiles (k_vscreen2) when the padded vocabulary is whole 160-column tiles
// (V = 10,123: 64 of them) and a wave's u fragments fit its registers; k_vscreen otherwise
static bool screen_wide(const Layout& L) { return L.Vp % SC2_BN == 0 && L.H <= 512; }

// The T-step loop over the B rows: k_lstm (GEMM + cell + attention projections), k_atten, then the
// vocab stage -- k_vscreen2 (bf16 screen, granule summaries) + k_vrescore (exact fp32 rescoring of
// the candidates), or with AA_DECODE_EXACT_VOCAB the exact fp32 GEMM k_vocab + k_key_ids.
static int decode_rows(const Layout& L, const MP& p, const DecodeWS& w, int B, int T, int32_t flags, int64_t* ids,
                       float* alpha, float* beta, const aa_trace* trace, hipStream_t s) {
  const bool exact = (flags & AA_DECODE_EXACT_VOCAB) != 0;
  const bool base = (flags & AA_DECODE_BASELINE) != 0;  // no-sentinel kernels; beta is not touched
  const int H = L.H;
  const RowWS& r = w.r;
  const bool wide = screen_wide(L);
  // the rescoring of step t-1 rides in step t's LSTM launch (k_lstm<.., RS>); the last step's has
  // its own launch
  const bool fused = !exact && (flags & AA_DECODE_SPLIT_RESCORE) == 0;
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    // token of step t-1: ids[:, t-1] (written by the previous step); t = 0: nullptr = <start> for every row
    const int64_t* tok = t ? ids + (t - 1) : nullptr;
    const int tok_ld = t ? T : 1;
    uint64_t* kt = w.keys + (size_t)t * B;
    float* alt = alpha ? alpha + (size_t)t * P : nullptr;
    float* blt = beta ? beta + t : nullptr;
    RsArgs ra{rup((B + 1) / 2, 8), L.Vp, T, t - 1, (flags & AA_DECODE_RS_SELF) ? 0 : RS_WAIT_TICKS, r.u, w.summ,
              p.mlp_w, p.mlp_b, kt - B, ids};
    lstm_atten_launch(L, p,
                      {.B = B, .tok = tok, .tok_ld = tok_ld, .V = w.e.V, .vwv = w.e.vwv, .xg = r.xg,
                       .hsp_in = r.hsp[cur], .c_in = r.c[cur], .h_out = r.h[nxt], .hsp_out = r.hsp[nxt],
                       .c_out = r.c[nxt], .s = r.s, .part = r.part, .u = r.u, .ub = exact ? nullptr : w.ub,
                       .unorm = exact ? nullptr : w.unorm, .alpha = alt, .alpha_ld = (int64_t)T * P, .beta = blt,
                       .beta_ld = T, .ra = fused && t > 0 ? &ra : nullptr, .base = base,
                       .lstm_ev = trace ? trace->lstm_events : nullptr,
                       .atten_ev = trace ? trace->atten_events : nullptr, .ei = 2 * t},
                      s);
    aa_event_t* sev = trace ? trace->screen_events : nullptr;
    aa_event_t* rev = trace ? trace->rescore_events : nullptr;
    if (exact) {
      vocab_launch(L, p, B, r.u, nullptr, L.V, kt, s, sev, 2 * t);
      hipLaunchKernelGGL(k_key_ids, dim3((B + 255) / 256), dim3(256), 0, s, kt, B, ids + t, T);
      continue;
    }
    const bf16x8* ubf = reinterpret_cast<const bf16x8*>(w.ub);
    const bf16x8* wbf = reinterpret_cast<const bf16x8*>(p.mlp_wb);
    const float* unorm = w.unorm;
    aa_for_hidden(H, [&](auto h) {
      constexpr int H_ = h.value;
      const dim3 g2(((B + SC2_BM - 1) / SC2_BM) * (L.Vp / SC2_BN));
      if constexpr (H_ <= 512) {  // screen_wide() admits no larger H: no k_vscreen8 / k_vscreen2 beyond it
        if (wide) {
          if (!(flags & AA_DECODE_SCREEN4))
            AA_TLAUNCH(sev, 2 * t, k_vscreen8<H_>, g2, dim3(SC8_NT), 0, s, B, L.V, L.Vp, ubf, unorm, wbf, p.mlp_gs,
                       p.mlp_b, w.summ);
          else
            AA_TLAUNCH(sev, 2 * t, k_vscreen2<H_>, g2, dim3(256), 0, s, B, L.V, L.Vp, ubf, unorm, wbf, p.mlp_gs,
                       p.mlp_b, w.summ);
          return;
        }
      }
      AA_TLAUNCH(sev, 2 * t, k_vscreen<H_>, dim3(((B + SC_BM - 1) / SC_BM) * (L.Vp / SC_BN)), dim3(256), 0, s, B, L.V,
                 L.Vp, ubf, unorm, wbf, p.mlp_gs, p.mlp_b, w.summ);
    });
    if (fused && t + 1 < T) continue;  // rescored by step t+1's k_lstm
    aa_for_hidden(H, [&](auto h) {
      AA_TLAUNCH(rev, 2 * t, k_vrescore<h.value>, dim3(B), dim3(RS_NT), 0, s, B, L.V, L.Vp, (const float*)r.u,
                 (const float4*)w.summ, p.mlp_w, p.mlp_b, kt, ids, T, t);
    });
  }
  return launch_status();
}

// aux: optional second stream for the encoder's a_g branch (heads -> x_g beside the VWv GEMM);
// `s` waits for it before the step loop.
static int greedy_impl(const aa_model* m, const float* feats, int32_t B, int32_t T, int64_t* ids, float* alpha,
                       float* beta, void* workspace, size_t workspace_bytes, const aa_trace* trace, int32_t flags,
                       hipStream_t s, hipStream_t aux = nullptr) {
  Layout L;
  int rc = check_model(m, &L);
  if (rc) return rc;
  if ((flags & AA_DECODE_BASELINE) && !baseline_ok(L)) return AA_ERR_DIMS;
  if (B < 0 || T < 0) return AA_ERR_SHAPE;
  if (B == 0 || T == 0) return AA_OK;
  if (!feats || !ids || !workspace) return AA_ERR_NULL;
  if (!al16(feats) || !al16(workspace)) return AA_ERR_ALIGN;
  size_t need;
  DecodeWS w = carve_decode(static_cast<char*>(workspace), L, B, T, &need);
  if (workspace_bytes < need) return AA_ERR_BUFFER;
  const MP p = resolve(m, L);
  // keys [T][B] cleared: the exact vocab stage accumulates into them by atomicMax (k_vocab); the
  // fused rescoring publishes them as readiness-tagged granules (a nonzero key = ready, k_lstm<.., RS>).
  // (The split default writes every key it produces; step 0's k_lstm takes <start> itself.)
  const bool clear = (flags & AA_DECODE_EXACT_VOCAB) || ((flags & AA_DECODE_SPLIT_RESCORE) == 0 && T > 1);
  const DecodeInit init{w.tok0, B, w.keys, T * B};
  rc = encoder_launch(L, p, feats, B, w.e.a_g, w.e.V, w.e.vg, w.r.h[0], w.r.c[0], w.e.vwv, w.r.xg,
                      trace ? trace->encoder_events : nullptr, flags, s, aux, w.r.hsp[0], clear ? &init : nullptr);
  if (rc) return rc;
  return decode_rows(L, p, w, B, T, flags, ids, alpha, beta, trace, s);
}

int aa_greedy_decode(const aa_model* m, const float* feats, int32_t B, int32_t T, int64_t* ids, float* alpha,
                     float* beta, void* workspace, size_t workspace_bytes, const aa_trace* trace, int32_t flags,
                     aa_stream_t stream) {
  return greedy_impl(m, feats, B, T, ids, alpha, beta, workspace, workspace_bytes, trace, flags, (hipStream_t)stream);
}

int aa_greedy_decode_aux(const aa_model* m, const float* feats, int32_t B, int32_t T, int64_t* ids, float* alpha,
                         float* beta, void* workspace, size_t workspace_bytes, const aa_trace* trace, int32_t flags,
                         aa_stream_t stream, aa_stream_t aux_stream) {
  return greedy_impl(m, feats, B, T, ids, alpha, beta, workspace, workspace_bytes, trace, flags, (hipStream_t)stream,
                     (hipStream_t)aux_stream);
}

// ---- decode plans: the whole greedy decode captured once into a hipGraph ------------------------
struct aa_decode_plan {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipStream_t cap = nullptr, aux = nullptr;
};

static void plan_free(aa_decode_plan* p) {
  if (!p) return;
  if (p->exec) (void)hipGraphExecDestroy(p->exec);
  if (p->graph) (void)hipGraphDestroy(p->graph);
  if (p->cap) (void)hipStreamDestroy(p->cap);
  if (p->aux) (void)hipStreamDestroy(p->aux);
  delete p;
}

int aa_decode_plan_create(const aa_model* m, const float* feats, int32_t B, int32_t T, int64_t* ids, float* alpha,
                          float* beta, void* workspace, size_t workspace_bytes, int32_t flags, aa_decode_plan** out) {
  if (!out) return AA_ERR_NULL;
  *out = nullptr;
  Layout L;
  int rc = check_model(m, &L);
  if (rc) return rc;
  if ((flags & AA_DECODE_BASELINE) && !baseline_ok(L)) return AA_ERR_DIMS;
  if (B <= 0 || T <= 0) return AA_ERR_SHAPE;
  if (!feats || !ids || !workspace) return AA_ERR_NULL;
  if (!al16(feats) || !al16(workspace)) return AA_ERR_ALIGN;
  size_t need;
  carve_decode(nullptr, L, B, T, &need);
  if (workspace_bytes < need) return AA_ERR_BUFFER;
  aa_decode_plan* p = new aa_decode_plan();
  hipError_t e = hipStreamCreateWithFlags(&p->cap, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->aux, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamBeginCapture(p->cap, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) {
    plan_free(p);
    return (int)e;
  }
  rc = greedy_impl(m, feats, B, T, ids, alpha, beta, workspace, workspace_bytes, nullptr, flags, p->cap,
                   (flags & AA_DECODE_ONE_STREAM) ? nullptr : p->aux);
  e = hipStreamEndCapture(p->cap, &p->graph);
  if (rc == 0 && e != hipSuccess) rc = (int)e;
  if (rc == 0) {
    e = hipGraphInstantiate(&p->exec, p->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) rc = (int)e;
  }
  if (rc) {
    plan_free(p);
    return rc;
  }
  // the capture streams are not needed to replay the graph: release them (and their hardware
  // queues -- HIP maps streams onto a few queues per process, and idle streams crowd them)
  (void)hipStreamDestroy(p->cap);
  (void)hipStreamDestroy(p->aux);
  p->cap = p->aux = nullptr;
  *out = p;
  return AA_OK;
}

int aa_decode_plan_launch(const aa_decode_plan* plan, aa_stream_t stream) {
  if (!plan || !plan->exec) return AA_ERR_NULL;
  return (int)hipGraphLaunch(plan->exec, (hipStream_t)stream);
}

int aa_decode_plan_destroy(aa_decode_plan* plan) {
  plan_free(plan);
  return AA_OK;
}

int aa_vocab_logits(const aa_model* m, int32_t B, const float* u, float* scores, aa_stream_t stream) {
  Layout L;
  int rc = check_model(m, &L);
  if (rc) return rc;
  if (B < 0) return AA_ERR_SHAPE;
  if (B == 0) return AA_OK;
  if (!u || !scores) return AA_ERR_NULL;
  if (!al16(u)) return AA_ERR_ALIGN;
  const MP p = resolve(m, L);
  vocab_launch(L, p, B, u, scores, L.V, nullptr, (hipStream_t)stream);
  return launch_status();
}

int aa_vocab_logits_at(const aa_model* m, int32_t B, const float* u, const int32_t* cols, int32_t n, float* out,
                       aa_stream_t stream) {
  Layout L;
  int rc = check_model(m, &L);
  if (rc) return rc;
  if (B < 0 || n < 0) return AA_ERR_SHAPE;
  if (B == 0 || n == 0) return AA_OK;
  if (!u || !cols || !out) return AA_ERR_NULL;
  if (!al16(u)) return AA_ERR_ALIGN;
  const MP p = resolve(m, L);
  hipLaunchKernelGGL(k_logits_at, dim3(B), dim3(256), 0, (hipStream_t)stream, L.H, L.V, u, cols, n, p.mlp_w, p.mlp_b, out);
  return launch_status();
}

int aa_synth_uniform(float* dst, int64_t n, uint64_t key, int64_t start, double lo, double hi, aa_stream_t stream) {
  if (n < 0 || start < 0) return AA_ERR_SHAPE;
  if (n == 0) return AA_OK;
  if (!dst) return AA_ERR_NULL;
  const int plain = (lo == 0.0 && hi == 1.0) ? 1 : 0;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_synth_uniform, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     (hipStream_t)stream, dst, n, key, start, lo, hi - lo, plain);
  return launch_status();
}

