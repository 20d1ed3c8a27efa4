// aa_kernels.hip — MI355X (gfx950) kernels and C-ABI for the adaptive-attention greedy decode
// ("Knowing When to Look"; reference: code_src/models/adaptive_attention.py,
// code_src/models/baseline_attention.py).  See DESIGN.md for the data layout and rooflines.
//
// Kernels (all arithmetic that defines an output is fp32):
//   pack time (once per weight set)
//     k_pack_lstm     W_hh / emb-part / v_g-part of W_ih and W_x re-laid in gate-interleaved tiles
//     k_gemm_bias     table[v] = embed[v] . [W_ih(emb part); W_x(emb part)]^T   (V x 5H)
//     k_pack_mlp      bf16 copy and row norms of W_m for the vocab screen
//   encoder tail (once per batch)
//     k_avgpool       a_g = AvgPool2d(7)(A)                           baseline_attention.py:46-47
//     k_enc_v         V = relu(A^T W_a^T + b_a)  [B*49, H]             :50-51
//     k_enc_heads     v_g | h0 | c0 = act(a_g [W_b;W_h0;W_c0]^T + b)   :53-60
//     k_gemm_bias     VWv = V W_v^T (step-invariant, hoisted)          adaptive_attention.py:34
//     k_gemm_bias     xg = v_g . [W_ih(v_g part); W_x(v_g part)]^T + b_ih + b_hh (step-invariant)
//   decode step t (x T)
//     k_lstm          gates = table[tok] + xg + h W_hh^T; LSTM cell; sentinel s = sigm(.) tanh(c')
//                     baseline_attention.py:151-172, adaptive_attention.py:79-83
//     k_atten         W_g h, W_s s, 49+1 tanh scores, softmax, context, beta mix, u = c_hat + h
//                     adaptive_attention.py:26-58, 132 (input of mlp)
//     k_vscreen       bf16 MFMA logits with a rigorous error bound -> per-tile candidate summary
//     k_vrescore      exact fp32 logits of the candidates (MFMA-order fma chain) + first-index argmax
//                     adaptive_attention.py:132, 201
//   exact-vocab path (scores output / verification): k_vocab (fp32 MFMA GEMM + fused argmax) + k_finalize
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <vector>

#include "aa_common.hpp"

namespace aa {

// Write-through stores (agent-scope relaxed atomic stores = `global_store_* sc1`): the line leaves
// for memory at once instead of sitting dirty in this XCD's L2 until the kernel-end writeback, which
// the next launch waits for (MI355X_MICROARCH.md, boundary: + dirty bytes / 6 TB/s).  k_lstm's
// outputs take them (the attention-projection partials, h / c / s / split-h); on k_atten5's u /
// bf16 u / norms, the screen's summaries and k_enc_v4's V they measured slower.
template <class T>
__device__ __forceinline__ void st_wt(T* p, const T& v) {
  if constexpr (sizeof(T) == 4) {
    __hip_atomic_store(reinterpret_cast<uint32_t*>(p), __builtin_bit_cast(uint32_t, v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  } else {
    static_assert(sizeof(T) == 8, "4- or 8-byte stores");
    __hip_atomic_store(reinterpret_cast<uint64_t*>(p), __builtin_bit_cast(uint64_t, v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
}

constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;

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
constexpr int VS_TILE = 32;     // screen summary granule: one (lbmax, top-2 ub) per row per 32 columns
constexpr int RS_CAP = 2048;    // candidate list capacity per row in k_vrescore (else full row)
// Exact fp32 logits (k_vocab and the rescoring) are NP_VOCAB independent fma chains over contiguous
// K ranges (in the MFMA k order), combined as ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)), then + bias.
constexpr int NP_VOCAB = 8;

// ---------------------------------------------------------------------------------------------
// Packed weight layout (float offsets into aa_model.packed), 64-float aligned regions.
// ---------------------------------------------------------------------------------------------
struct Layout {
  int E, H, V, C;
  int NH, NHp;   // heads rows E + 2H, padded to 64
  int Vp;        // vocab rows padded to 128
  int N5;        // 5H: 4 gates (packed tile order) + sentinel
  size_t enc_a_w, enc_a_b, enc_w3, whh3, heads_w, heads_b, wv, wg, ws, wh, whh, wemb, wvg, bias5, table, mlp_w, mlp_b, mlp_wb, mlp_wn, mlp_gs, wgs, mlp_w3, enc_w4, heads_w4, wvg4, wv4;
  size_t total_floats;
};

static inline size_t al64(size_t x) { return (x + 63) & ~size_t(63); }
static inline int rup(int x, int m) { return (x + m - 1) / m * m; }

static Layout make_layout(const aa_dims& d) {
  Layout L;
  L.E = d.embed; L.H = d.hidden; L.V = d.vocab; L.C = d.channels;
  L.NH = L.E + 2 * L.H; L.NHp = rup(L.NH, 64);
  L.Vp = rup(L.V, 128);
  L.N5 = 5 * L.H;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o = al64(o + n); return r; };
  L.enc_a_w = take((size_t)L.H * L.C);
  L.enc_a_b = take(L.H);
  L.enc_w3 = take((size_t)3 * L.H * L.C / 2);  // bf16 [H/32][C/16][3][64][8]
  L.heads_w = take((size_t)L.NHp * L.C);
  L.heads_b = take(L.NHp);
  L.wv = take((size_t)PP * L.H);
  L.wg = take((size_t)P * L.H);
  L.ws = take((size_t)P * L.H);
  L.wh = take(PP);
  L.whh = take((size_t)4 * L.H * L.H);
  L.whh3 = take((size_t)3 * 4 * L.H * L.H / 2);  // bf16 fragments [4H/32][H/16][3][64][8]
  L.wemb = take((size_t)L.N5 * L.E);
  L.wvg = take((size_t)L.N5 * L.E);
  L.bias5 = take(L.N5);
  L.table = take((size_t)L.V * L.N5);
  L.mlp_w = take((size_t)L.Vp * L.H);
  L.mlp_b = take(L.Vp);
  L.mlp_wb = take((size_t)L.Vp * L.H / 2);  // bf16
  L.mlp_wn = take((size_t)2 * L.Vp);  // ||w_n|| then ||w_n - bf16(w_n)|| (inflated)
  L.mlp_gs = take((size_t)4 * (L.Vp / VS_TILE));  // float4 per granule: (max ||w_n||, max |b_n|, max ||dw_n||, 0)
  L.wgs = take((size_t)(L.H / 16) * 2 * P * 16);  // [tile][98][16]: W_g rows then W_s rows, 16 units of the tile
  L.mlp_w3 = take((size_t)3 * L.Vp * L.H / 2);    // W_m as 3 bf16 planes, fragments [Vp/32][H/16][3][64][8] (beam)
  L.enc_w4 = take((size_t)3 * L.H * L.C / 2);     // W_a as 3 bf16 planes, 16x16x32 fragments [H/16][C/32][3][64][8]
  L.heads_w4 = take((size_t)3 * L.NHp * L.C / 2);  // heads as 3 bf16 planes, 16x16x32 fragments [NHp/16][C/32][3][64][8]
  L.wvg4 = take((size_t)3 * L.N5 * L.E / 2);       // W_vg (x_g GEMM) likewise [N5/16][E/32][3][64][8]
  L.wv4 = take((size_t)3 * PP * L.H / 2);          // W_v (VWv GEMM) likewise [PP/16][H/32][3][64][8]
  L.total_floats = o;
  return L;
}

struct MP {  // resolved device pointers of the packed weights
  const bf16x8 *enc_w3, *whh3, *mlp_w3, *enc_w4, *heads_w4, *wvg4, *wv4;
  const float *enc_a_w, *enc_a_b, *heads_w, *heads_b, *wv, *wg, *ws, *wh, *whh, *wemb, *wvg, *bias5, *table, *mlp_w,
      *mlp_b, *mlp_wn, *wgs;
  const float4* mlp_gs;
  const uint16_t* mlp_wb;
};

static MP resolve(const aa_model* m, const Layout& L) {
  const float* b = static_cast<const float*>(m->packed);
  MP p;
  p.enc_a_w = b + L.enc_a_w; p.enc_a_b = b + L.enc_a_b;
  p.enc_w3 = reinterpret_cast<const bf16x8*>(b + L.enc_w3);
  p.whh3 = reinterpret_cast<const bf16x8*>(b + L.whh3);
  p.mlp_w3 = reinterpret_cast<const bf16x8*>(b + L.mlp_w3);
  p.enc_w4 = reinterpret_cast<const bf16x8*>(b + L.enc_w4);
  p.heads_w4 = reinterpret_cast<const bf16x8*>(b + L.heads_w4);
  p.wvg4 = reinterpret_cast<const bf16x8*>(b + L.wvg4);
  p.wv4 = reinterpret_cast<const bf16x8*>(b + L.wv4);
  p.heads_w = b + L.heads_w; p.heads_b = b + L.heads_b;
  p.wv = b + L.wv; p.wg = b + L.wg; p.ws = b + L.ws; p.wh = b + L.wh;
  p.whh = b + L.whh; p.wemb = b + L.wemb; p.wvg = b + L.wvg; p.bias5 = b + L.bias5; p.table = b + L.table;
  p.mlp_w = b + L.mlp_w; p.mlp_b = b + L.mlp_b;
  p.mlp_wb = reinterpret_cast<const uint16_t*>(b + L.mlp_wb); p.mlp_wn = b + L.mlp_wn; p.wgs = b + L.wgs;
  p.mlp_gs = reinterpret_cast<const float4*>(b + L.mlp_gs);
  return p;
}

// ---------------------------------------------------------------------------------------------
// small math helpers (accurate libm: expf/tanhf from the device library, no fast-math)
// ---------------------------------------------------------------------------------------------

// Argmax key: larger logit wins; on equal logits the smaller vocab index wins (torch max(2)[1]
// returns the first maximal index, adaptive_attention.py:201).
__device__ __forceinline__ uint64_t argmax_key(float x, int n) {
  uint32_t u = __float_as_uint(x);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)n);
}
// order-preserving map of a (finite) float to u32: a < b  <=>  order_key(a) < order_key(b)
__device__ __forceinline__ uint32_t order_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ int64_t key_token(uint64_t k) { return (int64_t)(0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFu)); }

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  lo = __shfl_xor(lo, o, 64);
  hi = __shfl_xor(hi, o, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t x = shfl_xor_u64(k, o);
    k = x > k ? x : k;
  }
  return k;
}

// Element (row m, k) of a [rows][K] bf16 matrix stored in MFMA-fragment order (32-row blocks x
// 16-wide k chunks x 64 lanes x 8): lane l of a fragment holds row (l & 31), k = 8 (l >> 5) + e.
__device__ __forceinline__ int64_t frag_off(int m, int k, int K) {
  return (((int64_t)(m >> 5) * (K >> 4) + (k >> 4)) * 64 + (m & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7);
}

// fp32 -> bf16, round to nearest even (finite inputs)
__device__ __forceinline__ uint16_t f2bf(float x) {
  const uint32_t u = __float_as_uint(x);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// ---------------------------------------------------------------------------------------------
// E0: a_g[b, c] = (sum_p A[b, c, p]) / 49, sequential fp32 sum in p order (the order of ATen's
// cpu_avg_pool inner loop), one wave per 64 channels staged through LDS with 16-B loads.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_avgpool(const float* __restrict__ feats, int64_t nch, float* __restrict__ a_g) {
  __shared__ float buf[4][64 * P];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t ch0 = ((int64_t)blockIdx.x * 4 + w) * 64;
  const int nhere = ch0 < nch ? (int)(nch - ch0 < 64 ? nch - ch0 : 64) : 0;
  const int nf4 = nhere * P / 4;  // nhere is a multiple of 32 -> whole float4s
  const float4* src = reinterpret_cast<const float4*>(feats + ch0 * P);
  float4* dst = reinterpret_cast<float4*>(buf[w]);
  for (int q = lane; q < nf4; q += 64) dst[q] = src[q];
  __syncthreads();
  if (lane < nhere) {
    const float* row = buf[w] + lane * P;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += row[p];
    a_g[ch0 + lane] = s / 49.0f;
  }
}

// ---------------------------------------------------------------------------------------------
// E1: V = relu(A_rows W_a^T + b_a).  A row m = b*49 + p of the virtual [B*49, C] matrix is
// column p of image b's [C, 49] NCHW block: read straight from the feature map (no transpose
// pass), lanes over consecutive rows -> contiguous addresses.
// ---------------------------------------------------------------------------------------------
template <int BM>
struct ANCHW {
  // Per-thread row base pointer computed once (the thread's row is the same for every i and
  // K-step: q % BM == t % BM); a K-step only adds k * 49.
  const float* base;
  __device__ __forceinline__ void init(const float* F, int C, int m0, int M) {
    const int m = m0 + (int)(threadIdx.x % BM);
    const int mc = m < M ? m : M - 1;  // clamp, never zero (see ARowMajor)
    const int b = mc / P, p = mc - b * P;
    base = F + (int64_t)b * C * P + p;
  }
  __device__ __forceinline__ void map(int q, int& r, int& kq) const { r = q % BM; kq = q / BM; }
  __device__ __forceinline__ float4 load(int /*i*/, int q, int k0) const {
    const float* s = base + (k0 + 4 * (q / BM)) * P;
    return make_float4(s[0], s[P], s[2 * P], s[3 * P]);
  }
};

__global__ __launch_bounds__(256) void k_enc_v(const float* __restrict__ feats, int B, int C, int H,
                                               const float* __restrict__ W, const float* __restrict__ bias,
                                               float* __restrict__ V) {
  constexpr int BM = 64, BN = 64;
  __shared__ __attribute__((aligned(16))) float lds[Tile<BM, BN>::LDS_FLOATS];
  const int M = B * P, MT = (M + BM - 1) / BM, NTn = H / BN;
  const int L = xcd_remap(blockIdx.x, MT * NTn);
  const int mt = L / NTn, nt = L % NTn;  // n fastest: the A tile is shared inside an XCD
  ANCHW<BM> al;
  al.init(feats, C, mt * BM, M);
  WRowMajor wl{W, C, nt * BN};
  floatx16 acc[1][1];
  gemm_mainloop<BM, BN>(al, wl, C / BK, lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  const int col = nt * BN + wn * 32 + (lane & 31);
  const float bv = bias[col];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mt * BM + wm * 32 + acc_row(r, lane);
    if (row < M) V[(int64_t)row * H + col] = reluf_(acc[0][0][r] + bv);
  }
}

// ---------------------------------------------------------------------------------------------
// E1 (default): the same V on bf16 MFMA with 3-way split operands ("bf16x3"), fp32-accurate.
// Every fp32 operand x is split exactly as x = x0 + x1 + x2 + r with x_i bf16 (x0 = bf16(x),
// x1 = bf16(x - x0), x2 = bf16(x - x0 - x1); each difference is exact in fp32, |r| <= 2^-24 |x|).
// a.w is accumulated from the six partial products with i + j <= 2 (smallest first); the three
// dropped ones are <= 2^-24 |a w| each, so the result is as accurate as an fp32 GEMM (whose own
// accumulation error over K = 2048 dominates), at 6 bf16 MFMAs (6 x 32 cycles) per 32x32x16
// block instead of 8 fp32 MFMAs (8 x 64 cycles).
//   W: pre-split at pack time into MFMA-fragment order, enc_w3[nb][kc][q][lane][8] (1 KB per
//      fragment: lane l holds W[32 nb + (l & 31)][16 kc + 8 (l >> 5) + j]) and read straight into
//      VGPRs one stage ahead (each fragment is one coalesced 16-B-per-lane load).
//   A: read from the NCHW feature map (row m = b*49 + p, column = channel; lanes over consecutive
//      rows -> contiguous addresses), split in registers, staged in LDS as three bf16 planes
//      [row][k] with an 80-B pitch (conflict-free ds_read_b128 / ds_write_b128).
// Tile 128 x 128 per 256-thread workgroup; each wave owns 128 x 32 (4 blocks of 32 x 32: its own
// W columns, the A rows shared through LDS);
// K in stages of 32 (two k16 MFMA steps), A double-buffered in LDS, A and W prefetched a stage
// ahead in registers.
// ---------------------------------------------------------------------------------------------
constexpr int EV_BM = 128, EV_BN = 128, EV_BK = 32, EV_LD = 40;  // LDS pitch in bf16 (80 B)

__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)x;
  const float r1 = x - (float)h;
  m = (__bf16)r1;
  const float r2 = r1 - (float)m;
  l = (__bf16)r2;
}

__global__ __launch_bounds__(256, 2) void k_enc_v3(const float* __restrict__ feats, int B, int C, int H,
                                                   const bf16x8* __restrict__ W3, const float* __restrict__ bias,
                                                   float* __restrict__ V) {
  __shared__ __attribute__((aligned(16))) __bf16 As[2][3][EV_BM * EV_LD];
  const int M = B * P, MT = (M + EV_BM - 1) / EV_BM, NTn = H / EV_BN, KC = C / 16;
  const int L = xcd_remap(blockIdx.x, MT * NTn);
  const int mt = L / NTn, nt = L % NTn;  // n fastest: the A tile is shared inside an XCD
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  // A staging: thread -> row r (0..127), k-half kh: k = 16 kh + i, i < 16, of each 32-stage
  const int r = t & (EV_BM - 1), kh = t >> 7;
  int m = mt * EV_BM + r;
  m = m < M ? m : M - 1;  // clamp, never zero (rows >= M are not stored)
  const int bi = m / P, pi = m - bi * P;
  const float* arow = feats + (int64_t)bi * C * P + pi + (int64_t)(16 * kh) * P;
  // W fragments of this wave: its own 32-column block (no fragment is loaded by two waves)
  const int nb0 = (nt * EV_BN + wave * 32) / 32;
  const bf16x8* wf0 = W3 + (size_t)nb0 * KC * 3 * 64 + lane;
  float ra[16];
  bf16x8 wa[2][3], wb[2][3];  // [sub][q], two stages in flight
  floatx16 acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[a][i] = 0.f;

  auto gload_a = [&](int s) {
    const float* src = arow + (int64_t)(EV_BK * s) * P;
#pragma unroll
    for (int i = 0; i < 16; ++i) ra[i] = src[i * P];
  };
  auto gload_w = [&](int s, bf16x8 (&w)[2][3]) {
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int q = 0; q < 3; ++q) w[sub][q] = wf0[((size_t)(2 * s + sub) * 3 + q) * 64];
  };
  auto lstore_a = [&](int buf) {
    bf16x8 h[2], md[2], lo[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      __bf16 x0, x1, x2;
      split3(ra[i], x0, x1, x2);
      h[i >> 3][i & 7] = x0;
      md[i >> 3][i & 7] = x1;
      lo[i >> 3][i & 7] = x2;
    }
    const int o = r * EV_LD + 16 * kh;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<bf16x8*>(&As[buf][0][o + 8 * j]) = h[j];
      *reinterpret_cast<bf16x8*>(&As[buf][1][o + 8 * j]) = md[j];
      *reinterpret_cast<bf16x8*>(&As[buf][2][o + 8 * j]) = lo[j];
    }
  };
  auto compute = [&](int buf, const bf16x8 (&w)[2][3]) {
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        bf16x8 fa[3];
#pragma unroll
        for (int q = 0; q < 3; ++q)
          fa[q] = *reinterpret_cast<const bf16x8*>(&As[buf][q][(a * 32 + li) * EV_LD + 16 * sub + 8 * lh]);
        floatx16 x = acc[a];
        x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[2], w[sub][0], x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1], w[sub][1], x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], w[sub][2], x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1], w[sub][0], x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], w[sub][1], x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], w[sub][0], x, 0, 0, 0);
        acc[a] = x;
      }
    }
  };

  const int ns = C / EV_BK;  // even (C % 64 == 0 checked by the host)
  gload_a(0);
  gload_w(0, wa);
  lstore_a(0);
  gload_a(1);
  gload_w(1, wb);
  __syncthreads();
  // No branches around the prefetch loads (a branch makes the compiler's vmcnt bookkeeping assume
  // the worst at the join and drain the A prefetch inside the MFMA stream): past the end the
  // stage index is clamped and the extra loads / LDS stores are harmless.
  for (int s = 0; s < ns; s += 2) {
    const int s2 = s + 2 < ns ? s + 2 : ns - 1, s3 = s + 3 < ns ? s + 3 : ns - 1;
    // stage s: A in As[0], W in wa; A of s+1 in ra, W of s+1 in wb
    // (sched_barrier: keep the scheduler from hoisting the split of a just-issued A prefetch into
    //  the MFMA stream above it, which would wait for the load right away)
    lstore_a(1);
    gload_a(s2);
    __builtin_amdgcn_sched_barrier(0);
    compute(0, wa);
    gload_w(s2, wa);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    // stage s+1: A in As[1], W in wb (As[0] is free: its last reader passed the barrier)
    lstore_a(0);
    gload_a(s3);
    __builtin_amdgcn_sched_barrier(0);
    compute(1, wb);
    gload_w(s3, wb);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
  }
  const int col = nt * EV_BN + wave * 32 + li;
  const float bv = bias[col];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = mt * EV_BM + a * 32 + acc_row(i, lane);
      if (row < M) V[(int64_t)row * H + col] = reluf_(acc[a][i] + bv);
    }
}

// ---------------------------------------------------------------------------------------------
// E1 (default at H = 128 NCB): the same bf16x3 V, one workgroup per TWO IMAGES and all H columns,
// so the feature map is read from HBM exactly once and the grid is B/2 workgroups (256 at
// B = 512: one per CU).  k_enc_v3's 128 x 128 tiles re-read every A row block once per column
// tile (4x the A traffic through L2, 431 MB of HBM per launch against 260 MB algorithmic).
//   rows: the 98 rows m = 98 wg .. 98 wg + 97 (images 2 wg, 2 wg + 1), computed as 7 blocks of
//         16 rows of v_mfma_f32_16x16x32_bf16 (rows 98..111 of the tile are never stored);
//   columns: wave w owns NCB 16-column blocks [16 NCB w, 16 NCB (w + 1)), all 7 row blocks
//         (7 NCB accumulators of 4 floats);
//   A: 16 dword loads per thread per 32-channel stage (lanes over consecutive rows: contiguous
//      addresses), split in registers, three bf16 planes [row][k] in LDS with a 96-B pitch
//      (conflict-free 16x16x32 ds_read_b128 fragment reads), double-buffered, one stage ahead;
//   W: pre-split at pack time in 16x16x32 B-fragment order (enc_w4[nb][kc][q][lane][8], lane l
//      holds W[16 nb + (l & 15)][32 kc + 8 (l >> 4) + j]); each column pair's fragments of stage
//      s + 1 are loaded straight into VGPRs right after the pair's last MFMA of stage s.
// The six products per block run smallest first, as in k_enc_v3 (fp32-accurate).
// The avg-pool a_g (k_avgpool) is fused: the staging threads also put each stage's fp32 values in
// LDS as [image][channel][p], and one wave per stage (rotating) sums every channel of both images
// sequentially in p order and divides by 49 -- k_avgpool's arithmetic, bit-identical to ATen.
// ---------------------------------------------------------------------------------------------
// The feature map is read once per batch: non-temporal loads keep the 205 MB stream from
// evicting the step kernels' working set (V, W_m, the token table) of the batches in flight.
constexpr int E4_ROWS = 98, E4_RB = 7, E4_LD = 48;  // rows per workgroup, 16-row blocks, LDS pitch (bf16)
constexpr int E4_SP = 52, E4_MAXC = 2048;           // a_g staging pitch (floats), largest channel count
typedef float floatx4 __attribute__((ext_vector_type(4)));

// NW waves (8 or 16): each wave owns NCB 16-column blocks (H = 16 NCB NW); the A staging is done by
// the first 512 threads either way.  NW = 16 (four waves per SIMD instead of two, half the columns
// each; what H = 512 launches): k_enc_v4 247 -> 242 us, sequential decode +0.9 % (A/B, two rounds)
constexpr int ENC4_NW = 16;

template <int NCB, int NW = 8>
__global__ __launch_bounds__(64 * NW) void k_enc_v4(const float* __restrict__ feats, int B, int C,
                                                const bf16x8* __restrict__ W4, const float* __restrict__ bias,
                                                float* __restrict__ V, float* __restrict__ a_g) {
  static_assert(NCB % 2 == 0, "columns are processed in pairs of 16-column blocks");
  constexpr int H = 16 * NCB * NW, NPAIR = NCB / 2, PL = E4_RB * 16 * E4_LD;  // PL: one plane, bf16
  constexpr int NT = 64 * NW;
  const bool stager = NW == 8 || threadIdx.x < 512;
  __shared__ __attribute__((aligned(16))) __bf16 As[2][3][PL];
  __shared__ __attribute__((aligned(16))) float Sg[2][2 * 32 * E4_SP];  // fp32 stage copy for a_g
  __shared__ __attribute__((aligned(16))) float Ag[2 * E4_MAXC];        // a_g of the two images
  const int M = B * P, KC = C / 32;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.x * E4_ROWS;
  // staging: thread t < 392 -> row r = t % 98, channels 8 kg .. 8 kg + 7 of each 32-channel stage;
  // threads 392..511 fill garbage rows 98..105 (never stored) from a valid address.  (Each 8-lane
  // group of the ds_write_b128 then hits 4 distinct 16-B slots: 2-way store conflicts.  Remapping the
  // groups to 4 rows x 2 channel groups removes them but splits each wave's 256-B row-contiguous
  // feature loads into 128-B pieces: measured 246 -> 256 us, not kept.)
  const int sr = t < 4 * E4_ROWS ? t % E4_ROWS : E4_ROWS + (t & 7);
  const int kg = t < 4 * E4_ROWS ? t / E4_ROWS : (t >> 3) & 3;
  const bool stg = stager;
  int m = m0 + (t < 4 * E4_ROWS ? sr : 0);
  m = m < M ? m : M - 1;  // clamp, never zero (rows >= M are not stored)
  const int bi = m / P, pi = m - bi * P;
  const float* arow = feats + (int64_t)bi * C * P + pi + (int64_t)(8 * kg) * P;
  const int so = sr * E4_LD + 8 * kg;
  // fragment reads: lane l -> row 16 rb + (l & 15), k = 8 (l >> 4)
  const int fo = (lane & 15) * E4_LD + 8 * (lane >> 4);
  const bf16x8* wsrc = W4 + (size_t)(wave * NCB) * KC * 3 * 64 + lane;  // block nb = wave NCB + c
  float ra[8];
  bf16x8 wv[NCB][3];
  floatx4 acc[E4_RB][NCB];
#pragma unroll
  for (int rb = 0; rb < E4_RB; ++rb)
#pragma unroll
    for (int c = 0; c < NCB; ++c) acc[rb][c] = floatx4{0.f, 0.f, 0.f, 0.f};

  auto gload_a = [&](int s) {
    const float* src = arow + (int64_t)(32 * s) * P;
#pragma unroll
    for (int i = 0; i < 8; ++i) ra[i] = __builtin_nontemporal_load(src + i * P);
  };
  auto gload_w = [&](int s, int c) {
#pragma unroll
    for (int q = 0; q < 3; ++q) wv[c][q] = wsrc[((size_t)c * KC * 3 + (size_t)s * 3 + q) * 64];
  };
  auto lstore_a = [&](int buf) {
    bf16x8 x[3];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      __bf16 x0, x1, x2;
      split3(ra[i], x0, x1, x2);
      x[0][i] = x0; x[1][i] = x1; x[2][i] = x2;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) *reinterpret_cast<bf16x8*>(&As[buf][q][so]) = x[q];
    if (t < 4 * E4_ROWS) {  // sr = 49 image + p
      const int img = sr >= P, pp = sr - img * P;
      float* g = &Sg[buf][(img * 32 + 8 * kg) * E4_SP + pp];
#pragma unroll
      for (int i = 0; i < 8; ++i) g[i * E4_SP] = ra[i];
    }
  };

  const int ns = KC;
  if (stg) gload_a(0);
#pragma unroll
  for (int c = 0; c < NCB; ++c) gload_w(0, c);
  if (stg) lstore_a(0);
  if (stg) gload_a(ns > 1 ? 1 : 0);
  __syncthreads();
  for (int s = 0; s < ns; ++s) {
    const int buf = s & 1, s1 = s + 1 < ns ? s + 1 : ns - 1, s2 = s + 2 < ns ? s + 2 : ns - 1;
    // A of stage s+1 (in ra) into the other buffer: its last readers (stage s-1) passed the barrier
    if (stg) {
      lstore_a(buf ^ 1);
      gload_a(s2);
    }
    __builtin_amdgcn_sched_barrier(0);
    const __bf16* Ab = &As[buf][0][fo];
#pragma unroll
    for (int cp = 0; cp < NPAIR; ++cp) {
#pragma unroll
      for (int rb = 0; rb < E4_RB; ++rb) {
        bf16x8 fa[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) fa[q] = *reinterpret_cast<const bf16x8*>(Ab + q * PL + rb * 16 * E4_LD);
        // the pair's two accumulator chains interleaved (each chain's product order unchanged:
        // bit-identical), so no MFMA waits on its immediate predecessor
        {
          const int c0 = 2 * cp, c1 = c0 + 1;
          floatx4 x = acc[rb][c0], y = acc[rb][c1];
          x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[2], wv[c0][0], x, 0, 0, 0);
          y = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[2], wv[c1][0], y, 0, 0, 0);
          x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1], wv[c0][1], x, 0, 0, 0);
          y = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1], wv[c1][1], y, 0, 0, 0);
          x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0], wv[c0][2], x, 0, 0, 0);
          y = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0], wv[c1][2], y, 0, 0, 0);
          x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1], wv[c0][0], x, 0, 0, 0);
          y = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1], wv[c1][0], y, 0, 0, 0);
          x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0], wv[c0][1], x, 0, 0, 0);
          y = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0], wv[c1][1], y, 0, 0, 0);
          x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0], wv[c0][0], x, 0, 0, 0);
          y = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0], wv[c1][0], y, 0, 0, 0);
          acc[rb][c0] = x;
          acc[rb][c1] = y;
        }
      }
      gload_w(s1, 2 * cp);
      gload_w(s1, 2 * cp + 1);
      // re-read the A fragments for the next pair instead of keeping all 21 live (VGPR budget)
      asm volatile("" ::: "memory");
    }
    // one wave per stage (rotating over waves 0..7) sums the stage's channels for a_g (giving the turns
    // to waves 8..15, which do no A staging, measured 4 us slower at NW = 16)
    if (wave == (s & 7)) {  // lane -> (image lane / 32, channel lane % 32)
      const float* g = &Sg[buf][lane * E4_SP];
      float sum = 0.f;
#pragma unroll 4
      for (int pp = 0; pp < 48; pp += 4) {  // 16-B reads (E4_SP * 4 B = 13 x 16 B), summed in p order
        const float4 v = *reinterpret_cast<const float4*>(g + pp);
        sum += v.x; sum += v.y; sum += v.z; sum += v.w;
      }
      sum += g[48];
      Ag[(lane >> 5) * C + 32 * s + (lane & 31)] = sum / 49.0f;
    }
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
  }
  // a_g of the workgroup's images (the last workgroup of an odd batch holds one)
  for (int i = t; i < 2 * C; i += NT) {
    const int img = 2 * blockIdx.x + (i >= C);
    if (img < B) a_g[(int64_t)img * C + (i - (i >= C ? C : 0))] = Ag[i];
  }
  // epilogue: lane l holds column 16 nb + (l & 15), rows 16 rb + 4 (l >> 4) + i.  Stored straight
  // from the accumulators, every store instruction wrote 64-B row pieces (16 columns x 4 rows): 1.39x
  // the V bytes left L2 (r01 PMC).  Instead each 16-row block goes through LDS ([16][H + 4] floats,
  // aliasing the A stages) and leaves as whole rows: the workgroup's 98 rows are one contiguous
  // 98 H-float run of V, written by 16-B lanes, 1 KB per wave instruction.
  float* Vs = reinterpret_cast<float*>(&As[0][0][0]);
  constexpr int VSP = H + 4;  // pitch: rows 4 apart land 16 banks apart (conflict-free transposed writes)
  static_assert(16 * VSP * 4 <= sizeof(As), "V staging must fit in the A stages");
  float bvs[NCB];
#pragma unroll
  for (int c = 0; c < NCB; ++c) bvs[c] = bias[(wave * NCB + c) * 16 + (lane & 15)];
#pragma unroll
  for (int rb = 0; rb < E4_RB; ++rb) {
    __syncthreads();  // the previous block's rows were read out (rb = 0: the A stages are free)
#pragma unroll
    for (int c = 0; c < NCB; ++c) {
      const int col = (wave * NCB + c) * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) Vs[(4 * (lane >> 4) + i) * VSP + col] = reluf_(acc[rb][c][i] + bvs[c]);
    }
    __syncthreads();
    constexpr int F4 = 16 * H / 4;  // float4s of the block
#pragma unroll
    for (int q = t; q < F4; q += NT) {
      const int r = q / (H / 4), c4 = q % (H / 4), tr = rb * 16 + r, row = m0 + tr;
      if (tr < E4_ROWS && row < M)
        *reinterpret_cast<float4*>(V + (int64_t)row * H + 4 * c4) = *reinterpret_cast<const float4*>(Vs + r * VSP + 4 * c4);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// E2: heads.  [v_g | h0 | c0] = a_g · [W_b; W_h0; W_c0]^T + b, relu / tanh / tanh by column.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_enc_heads(const float* __restrict__ a_g, int B, int C, int E, int H, int NHp,
                                                   const float* __restrict__ W, const float* __restrict__ bias,
                                                   float* __restrict__ v_g, float* __restrict__ h0, float* __restrict__ c0) {
  constexpr int BM = 64, BN = 64;
  __shared__ __attribute__((aligned(16))) float lds[Tile<BM, BN>::LDS_FLOATS];
  const int MT = (B + BM - 1) / BM, NTn = NHp / BN;
  const int L = xcd_remap(blockIdx.x, MT * NTn);
  const int nt = L / MT, mt = L % MT;
  ARowMajor al{a_g, C, mt * BM, B};
  WRowMajor wl{W, C, nt * BN};
  floatx16 acc[1][1];
  gemm_mainloop<BM, BN>(al, wl, C / BK, lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  const int col = nt * BN + wn * 32 + (lane & 31);
  if (col >= E + 2 * H) return;
  const float bv = bias[col];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mt * BM + wm * 32 + acc_row(r, lane);
    if (row >= B) continue;
    const float x = acc[0][0][r] + bv;
    if (col < E) v_g[(int64_t)row * E + col] = reluf_(x);
    else if (col < E + H) h0[(int64_t)row * H + (col - E)] = tanhf(x);
    else c0[(int64_t)row * H + (col - E - H)] = tanhf(x);
  }
}

// ---------------------------------------------------------------------------------------------
// E2 (default): the encoder's small GEMMs on bf16 MFMA with 3-way split operands (fp32-accurate, as
// k_enc_v4): out[M x N] = A[M x K] W^T (+ bias), A fp32 row-major (lda K), W pre-split in 16x16x32
// B-fragment order (k_pack_w4).  A workgroup owns 32 rows x 16 NB columns; its NWV waves each run
// 1/NWV of K over the whole tile (v_mfma_f32_16x16x32_bf16, a fragments split in registers), and the
// NWV partial tiles are summed in LDS as a fixed pairwise tree before bias and epilogue.  These GEMMs
// are short (K = 256..2048, 32-row tiles): their time is the K loop's load latency, so K is spread
// over waves (k_enc_heads' 64 x 64 fp32-MFMA tiles ran all K = 2048 per workgroup: ≈66 µs).
//   MODE_HEADS: columns [0, E) -> v_g = relu, [E, E+H) -> h0 = tanh, [E+H, E+2H) -> c0 = tanh
//   MODE_PLAIN: out0[row * ldo + col] = acc + (bias ? bias[col] : 0), col < N  (x_g, VWv)
// ---------------------------------------------------------------------------------------------
enum { MODE_HEADS = 0, MODE_PLAIN = 1 };
template <int NB, int NWV, int MODE>
__global__ __launch_bounds__(64 * NWV) void k_gemm3(const float* __restrict__ A, int M, int K, int N,
                                                    const bf16x8* __restrict__ W4, const float* __restrict__ bias,
                                                    float* __restrict__ out0, int ldo, float* __restrict__ h0,
                                                    float* __restrict__ c0, int E, int H,
                                                    bf16x8* __restrict__ hsp = nullptr, int64_t* __restrict__ tok0 = nullptr,
                                                    int tok_n = 0, uint64_t* __restrict__ keys = nullptr, int key_n = 0) {
  constexpr int BN = 16 * NB, TP = BN + 4;  // tile columns, LDS row pitch of a partial tile (floats)
  if (MODE == MODE_HEADS && tok0) {  // k_decode_init's work (one-stream decode): <start> ids, cleared keys
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int i = i0; i < tok_n; i += stride) tok0[i] = 1;
    for (int i = i0; i < key_n; i += stride) __hip_atomic_store(keys + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __shared__ __attribute__((aligned(16))) float Pt[NWV][32 * TP];
  const int KC = K / 32, NTn = (N + BN - 1) / BN;
  const int mt = blockIdx.x / NTn, nt = blockIdx.x % NTn;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = mt * 32;
  const float* arow[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    int m = m0 + 16 * rb + (lane & 15);
    m = m < M ? m : M - 1;  // clamp, never zero (rows >= M are not stored)
    arow[rb] = A + (int64_t)m * K + 8 * (lane >> 4);
  }
  const bf16x8* wsrc = W4 + (size_t)(nt * NB) * KC * 3 * 64 + lane;
  floatx4 acc[2][NB];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int c = 0; c < NB; ++c) acc[rb][c] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int per = KC / NWV, kc0 = wave * per;  // K % (64 NWV) == 0 (checked by the host): per is even
  float4 av[2][2][2];   // [slot][row block][half]
  bf16x8 wv[2][NB][3];  // [slot][column block][plane]
  auto load = [&](int slot, int kc) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      av[slot][rb][0] = *reinterpret_cast<const float4*>(arow[rb] + 32 * kc);
      av[slot][rb][1] = *reinterpret_cast<const float4*>(arow[rb] + 32 * kc + 4);
    }
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
      for (int q = 0; q < 3; ++q) wv[slot][c][q] = wsrc[((size_t)c * KC * 3 + (size_t)kc * 3 + q) * 64];
  };
  auto step = [&](int slot) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      bf16x8 fa[3];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        __bf16 x0, x1, x2;
        split3(f4c(av[slot][rb][i >> 2], i & 3), x0, x1, x2);
        fa[0][i] = x0; fa[1][i] = x1; fa[2][i] = x2;
      }
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        floatx4 x = acc[rb][c];
        x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[2], wv[slot][c][0], x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1], wv[slot][c][1], x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0], wv[slot][c][2], x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1], wv[slot][c][0], x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0], wv[slot][c][1], x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0], wv[slot][c][0], x, 0, 0, 0);
        acc[rb][c] = x;
      }
    }
  };
  // two chunks in flight; `per` is even; past the end the chunk index is clamped (harmless reloads)
  const int last = kc0 + per - 1;
  load(0, kc0);
  load(1, kc0 + 1 < last ? kc0 + 1 : last);
  for (int kc = kc0; kc < kc0 + per; kc += 2) {
    step(0);
    load(0, kc + 2 < last ? kc + 2 : last);
    step(1);
    load(1, kc + 3 < last ? kc + 3 : last);
  }
  // partial tile of this wave -> LDS [row][col]: lane holds column 16 c + (l & 15), rows 16 rb + 4 (l >> 4) + i
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) Pt[wave][(16 * rb + 4 * (lane >> 4) + i) * TP + 16 * c + (lane & 15)] = acc[rb][c][i];
  __syncthreads();
  for (int e = t; e < 32 * BN; e += 64 * NWV) {
    const int r = e / BN, cl = e - r * BN, row = m0 + r, col = nt * BN + cl;
    if (row >= M || col >= N) continue;
    const int o = r * TP + cl;
    float ps[NWV];
#pragma unroll
    for (int w = 0; w < NWV; ++w) ps[w] = Pt[w][o];
#pragma unroll
    for (int st = 1; st < NWV; st *= 2)  // ((p0 + p1) + (p2 + p3)) + ...
#pragma unroll
      for (int w = 0; w + st < NWV; w += 2 * st) ps[w] += ps[w + st];
    if (MODE == MODE_PLAIN) {
      out0[(int64_t)row * ldo + col] = bias ? ps[0] + bias[col] : ps[0];
    } else {
      const float x = ps[0] + bias[col];
      if (col < E) out0[(int64_t)row * E + col] = reluf_(x);
      else if (col < E + H) {
        const float hv = tanhf(x);
        const int k = col - E;
        h0[(int64_t)row * H + k] = hv;
        if (hsp) {  // k_split_rows's fragments of h0 (the first step's GEMM operand), element by element
          __bf16 x0, x1, x2;
          split3(hv, x0, x1, x2);
          __bf16* o = reinterpret_cast<__bf16*>(hsp + ((size_t)((row >> 5) * (H / 16) + (k >> 4)) * 3) * 64 +
                                                (row & 31) + 32 * ((k >> 3) & 1)) + (k & 7);
          o[0] = x0;
          o[64 * 8] = x1;
          o[128 * 8] = x2;
        }
      } else {
        c0[(int64_t)row * H + (col - E - H)] = tanhf(x);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Generic C[M, N] = A[M, K] · W[N, K]^T (+ bias[N]) with a row-major store (ldc), N % 64 == 0.
// Used for VWv (encoder), xg (encoder) and the per-token table (pack time).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gemm_bias(const float* __restrict__ A, int lda, int M, const float* __restrict__ W,
                                                   int ldw, int N, int K, const float* __restrict__ bias,
                                                   float* __restrict__ Cm, int64_t ldc) {
  constexpr int BM = 64, BN = 64;
  __shared__ __attribute__((aligned(16))) float lds[Tile<BM, BN>::LDS_FLOATS];
  const int MT = (M + BM - 1) / BM, NTn = N / BN;
  const int L = xcd_remap(blockIdx.x, MT * NTn);
  const int nt = L / MT, mt = L % MT;
  ARowMajor al{A, lda, mt * BM, M};
  WRowMajor wl{W, ldw, nt * BN};
  floatx16 acc[1][1];
  gemm_mainloop<BM, BN>(al, wl, K / BK, lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  const int col = nt * BN + wn * 32 + (lane & 31);
  const float bv = bias ? bias[col] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mt * BM + wm * 32 + acc_row(r, lane);
    if (row < M) Cm[(int64_t)row * ldc + col] = bias ? acc[0][0][r] + bv : acc[0][0][r];
  }
}

// ---------------------------------------------------------------------------------------------
// D1: LSTM step + sentinel.  x_t = [embed[tok]; v_g] enters through two step-invariant terms:
//   table[tok] = embed[tok] . W_ih[:, :E]^T (pack time)   and   xg[b] = v_g[b] . W_ih[:, E:]^T + b_ih + b_hh
// (per batch), so the step's GEMM is only h_{t-1} W_hh^T (K = H).  Columns are packed per tile of
// 16 hidden units as (i, f, g, o) x 16; the epilogue exchanges the tile through LDS so one thread
// sees all four gates of a unit:
//   c' = s(f) c + s(i) tanh(g),  h' = s(o) tanh(c')            (torch LSTM cell, gate order i,f,g,o)
//   s  = sigmoid(x W_x^T + W_h . 0) * tanh(c')                  (Sentinel, h_{t-1} = 0 while sampling,
//                                                                adaptive_attention.py:116-122)
// with x W_x^T = table[tok][4H + j] + xg[b][4H + j].
// The tile then contributes its 16 units to the attention projections W_g h' and W_s s
// (Atten.affine_g / affine_s, adaptive_attention.py:35,45): part[b][tile][j] = sum_{u in tile}
// (j < 49 ? h'_u W_g[j][u] : s_u W_s[j-49][u]); k_atten adds the H/16 partials in tile order.
// ---------------------------------------------------------------------------------------------
constexpr int PART = 128;  // partial-projection row pitch (W_g h outputs at 0..48, W_s s at 64..112)
// Column of projection output j (0..97: W_g then W_s) in a partial row.  Each half
// starts on a 256-B boundary, so every store instruction of the tile's projection phase (a 32 x 32
// accumulator block: two rows x 32 columns) writes two whole 128-B lines (the write-through stores of
// partial lines otherwise cost the memory side a read-modify-write each).
__device__ __forceinline__ int part_col(int j) { return j < P ? j : 64 + (j - P); }

// The GEMM h_{t-1} W_hh^T runs on bf16 MFMA with 3-way split operands (see k_enc_v3): h arrives
// already split (hsp_in, written by the previous step's epilogue or k_split_rows) and W_hh is
// pre-split at pack time, both in MFMA-fragment order, so every operand is one coalesced 16-B
// load per lane straight into VGPRs -- no LDS staging.  Fragment index of (row block rb, k16
// chunk kc, plane q): ((rb * KC + kc) * 3 + q) * 64 + lane.
// 512 threads = 8 waves; wave w computes the whole 64x64 tile (2 x 2 blocks of 32x32) over K
// chunks [w KC/8, (w+1) KC/8), so no fragment is loaded twice in the workgroup; the eight partial
// tiles meet in LDS and are summed in a fixed tree ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)).
__device__ __forceinline__ void x3_step(floatx16& acc, const bf16x8 (&a)[3], const bf16x8 (&w)[3]) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], w[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], w[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], w[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[0], acc, 0, 0, 0);
}

// Two-accumulator form (the lean k_lstm / k_lstm_gemm GEMMs): the three small products (i + j = 2)
// go to one chain and the three large ones (i + j <= 1) to another, summed once at the end -- two
// independent MFMA chains per wave instead of one dependent chain of 6 per chunk (sequential decode
// +3 % in A/B; at least as accurate: the small terms no longer meet the large running sum chunk by
// chunk).
__device__ __forceinline__ void x3_step2(floatx16& sm, floatx16& bg, const bf16x8 (&a)[3], const bf16x8 (&w)[3]) {
  sm = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], w[0], sm, 0, 0, 0);
  bg = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], w[0], bg, 0, 0, 0);
  sm = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], w[1], sm, 0, 0, 0);
  bg = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[1], bg, 0, 0, 0);
  sm = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[2], sm, 0, 0, 0);
  bg = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[0], bg, 0, 0, 0);
}

constexpr int LS_CP = 68;  // k_lstm LDS tile pitch (floats): conflict-free cell reads

// Cell epilogue shared by k_lstm (GEMM + cell in one launch) and k_lstm_cell (cell of a GEMM done
// by k_lstm_gemm): thread -> row rr (0..63) of the tile, units u0, u0 + 1 of tile nt.
// gate[g][q] = (h W_hh^T)[gate g, unit u0 + q] + (table[tok] + xg) -- the pre-activations;
// sa + sb = x W_x^T of the sentinel; cprev = c_{t-1}; wsv = this thread's float4 of the tile's
// W_g / W_s slice.  Writes c', h', s, the next step's split-h fragments, and the tile's partial
// attention projections part[row][nt][j] = sum_{u in tile} (j < 49 ? h'_u W_g[j][u] : s_u W_s[j-49][u])
// (v_mfma_f32_32x32x2f32, units (i, 8 + i) per instruction, i = 0..7 in order).
constexpr int LS_HP = 68;    // pitch of the transposed h' / s tiles [unit][row]: conflict-free MFMA A reads
constexpr int LS_WSP = 100;  // 98 projection outputs padded to whole float4s
constexpr int LS_TAIL_FLOATS = 2 * 16 * LS_HP + 16 * LS_WSP;
// SENT = false (the baseline spatial-attention model, baseline_attention.py:78-128: no sentinel): no
// s (sa / sb are not read, the Ss tile and the s_out store are gone) and only the W_g half of the
// projections -- waves 0..3 (cb < 2), columns 0..63 of a part row; c', h', the split-h fragments and
// the W_g partials by the same arithmetic in the same order as with the sentinel.
template <int H, bool SENT = true>
__device__ __forceinline__ void lstm_cell_tail(int B, int m0, int nt, const float (&gate)[4][2], float2 sa, float2 sb,
                                               float2 cprev, float4 wsv, float* Hs, float* h_out,
                                               bf16x8* __restrict__ hsp_out, float* __restrict__ c_out,
                                               float* __restrict__ s_out, float* __restrict__ part) {
  constexpr int HP = LS_HP, WSP = LS_WSP, NTn = H / 16, KC = H / 16;
  float* Ss = Hs + 16 * HP;   // [16][HP] s of the tile, transposed
  float* Wsl = Ss + 16 * HP;  // [16][WSP] W_g / W_s rows (j < 49: W_g, else W_s) per unit
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int rr = t >> 3, u0 = (t & 7) * 2, m = m0 + rr, j = nt * 16 + u0;
  {  // transpose the W_g / W_s slice to [unit][j] (j = 98, 99 are zero)
    const int jj = t >> 2, uq = (t & 3) * 4;
    if (t < (SENT ? 2 : 1) * P * 4) {
      Wsl[(uq + 0) * WSP + jj] = wsv.x; Wsl[(uq + 1) * WSP + jj] = wsv.y;
      Wsl[(uq + 2) * WSP + jj] = wsv.z; Wsl[(uq + 3) * WSP + jj] = wsv.w;
    } else if (SENT && t < 2 * P * 4 + 32) {
      const int z = t - 2 * P * 4;  // 32 zeros: j = 98, 99 for 16 units
      Wsl[(z >> 1) * WSP + 2 * P + (z & 1)] = 0.f;
    }
  }
  {
    float hn[2], cn[2], sn[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float i_ = sigmoidf_(gate[0][q]), f_ = sigmoidf_(gate[1][q]), g_ = tanhf(gate[2][q]),
                  o_ = sigmoidf_(gate[3][q]);
      cn[q] = f_ * (&cprev.x)[q] + i_ * g_;
      const float tc = tanhf(cn[q]);
      hn[q] = o_ * tc;
      if constexpr (SENT) sn[q] = sigmoidf_((&sa.x)[q] + (&sb.x)[q]) * tc;
    }
    Hs[u0 * HP + rr] = hn[0];
    Hs[(u0 + 1) * HP + rr] = hn[1];
    if constexpr (SENT) {
      Ss[u0 * HP + rr] = sn[0];
      Ss[(u0 + 1) * HP + rr] = sn[1];
    }
    if (m < B) {
      st_wt(reinterpret_cast<float2*>(c_out + (int64_t)m * H + j), make_float2(cn[0], cn[1]));
      st_wt(reinterpret_cast<float2*>(h_out + (int64_t)m * H + j), make_float2(hn[0], hn[1]));
      if constexpr (SENT) st_wt(reinterpret_cast<float2*>(s_out + (int64_t)m * H + j), make_float2(sn[0], sn[1]));
      if (hsp_out) {
        // next step's A fragments: k = j.. in chunk nt, lane (m % 32) + 32 * (u0 / 8), elements u0 % 8..
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        bf16x2 p0, p1, p2;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          __bf16 x0, x1, x2;
          split3(hn[q], x0, x1, x2);
          p0[q] = x0; p1[q] = x1; p2[q] = x2;
        }
        bf16x8* o = hsp_out + ((size_t)((m >> 5) * KC + nt) * 3) * 64 + (m & 31) + 32 * (u0 >> 3);
        const int e = u0 & 7;
        st_wt(reinterpret_cast<bf16x2*>(reinterpret_cast<__bf16*>(o) + e), p0);
        st_wt(reinterpret_cast<bf16x2*>(reinterpret_cast<__bf16*>(o + 64) + e), p1);
        st_wt(reinterpret_cast<bf16x2*>(reinterpret_cast<__bf16*>(o + 128) + e), p2);
      }
    }
  }
  AA_TS(0, 3);
  __syncthreads();
  // Wave -> one 32x32 block: rows rb*32.., columns cb = 0, 1: W_g j = 0..63; cb = 2, 3: W_s j = 0..63.
  if (SENT || wave < 4) {
    const int rb = wave & 1, cb = wave >> 1, li = lane & 31, lh = lane >> 5;
    const float* X = cb < 2 ? Hs : Ss;
    const int jj = (cb & 1) * 32 + li, jg = (cb < 2 ? 0 : P) + jj, jgc = jg < WSP ? jg : WSP - 1;
    floatx16 pacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) pacc[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int u = i + 8 * lh;
      const float av = X[u * HP + rb * 32 + li];
      const float wv = jj < P ? Wsl[u * WSP + jgc] : 0.f;
      pacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wv, pacc, 0, 0, 0);
    }
    // (all 32 lanes store -- columns jj >= P hold zeros, their W values being 0 -- so the lines are whole)
    const int col = (cb < 2 ? 0 : 64) + jj;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int mr = m0 + rb * 32 + acc_row(r, lane);
      if (mr < B) st_wt(&part[((int64_t)mr * NTn + nt) * PART + col], pacc[r]);
    }
  }
}

// LDS-staged variant of the lean GEMM (the default): the same waves, blocks, K halves, chunk order
// and MFMA sequence (bit-identical accumulators), but every fragment reaches LDS ONCE per workgroup by
// LDS-DMA (global_load_lds, 1 KB per wave instruction) and the two waves that share it read it
// from there.  The register-staged lean GEMM loads each fragment twice (768 KB per workgroup where
// 384 KB are unique): its fragment stream was the GEMM phase's bound (tools/ktrace: loads alone 5.0
// of the 8.9 us).  A stage = chunk `it` of both K halves = 24 fragments (24 KB): fragment f = 12 kh
// + j, j < 6: A row block j / 3, plane j % 3; j >= 6: W column block (j - 6) / 3, plane (j - 6) % 3.
// Wave w issues fragments 3w .. 3w + 2 of every stage.  Three stages in a ring: stage it + 2 is in
// flight while stage it is multiplied (counted vmcnt, raw s_barrier: a __syncthreads() would drain
// the DMAs).  `pre` runs after the first three stages are issued: it may issue exactly LS_GATHERS
// ordinary loads (the cell's gathers), which the counted waits of the first two iterations account
// for.  Ends with the K halves summed into Pt [column][row] (Pt aliases the ring).
constexpr int LS_NB = 3;                      // ring stages (LS_NB - 1 in flight ahead of the one multiplied)
constexpr int LS_STAGE = 24 * 64;             // bf16x8 per stage
constexpr int LS_GATHERS = 12;                // ordinary loads issued by k_lstm's gathers (ISA-checked)
constexpr int LS_NPW = 3;                     // fragments each wave DMAs per ring stage

// s_waitcnt vmcnt(n) for an n that is a compile-time constant once the caller's loop is unrolled
template <int V>
__device__ __forceinline__ void vm_wait_c() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(V) : "memory"); }
template <int V = 0>
__device__ __forceinline__ void vm_wait(int n) {
  if constexpr (V < 63) {
    if (n == V) vm_wait_c<V>();
    else vm_wait<V + 1>(n);
  } else {
    vm_wait_c<63>();
  }
}

// Two more hooks for the fused-rescoring launch (k_lstm<.., RS>), both inside the ring at fixed
// iterations so every wait stays a compile-time count: at iteration JK (after that iteration's
// stage issue) `kdma` lets wave 0 issue ONE more LDS-DMA (the tile's published keys); at iteration JG
// >= JK + NB (by then that DMA has landed: it is older than the stage the iteration waits for)
// `mid` may read it from LDS and issue exactly NG2 ordinary loads per wave (the token-dependent
// table gathers), which land under the remaining iterations.  JK < 0: no hooks.
struct NoHook {
  __device__ void operator()() const {}
};
template <int H, int NG = LS_GATHERS, int JK = -1, int JG = -1, int NG2 = 0, class F, class FK = NoHook,
          class FM = NoHook>
__device__ __forceinline__ void lstm_gemm_lds(const bf16x8* af0, const bf16x8* af1, const bf16x8* wf0,
                                              const bf16x8* wf1, bf16x8* stg, float* Pt, F&& pre,
                                              FK&& kdma = FK{}, FM&& mid = FM{}) {
  constexpr int KC = H / 16, CP = LS_CP, N = KC / 2, NB = LS_NB < N ? LS_NB : N;
  constexpr int LS_GATHERS = NG;  // ordinary loads `pre` issues (0: none)
  static_assert(NB >= 3, "the ring needs at least three stages");
  static_assert(JK < 0 || (JK + NB < N - 1 && JG >= JK + NB && JG < N - 1), "hook iterations");
  // last stage issued before each hook's loads (they are younger than it, older than the next)
  constexpr int SK = JK + NB < N - 1 ? JK + NB : N - 1, SG = JG + NB < N - 1 ? JG + NB : N - 1;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int a = (wave >> 1) & 1, c = wave & 1, kh = wave >> 2;
  const bf16x8* src[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int f = 3 * wave + i, hf = f / 12, j = f % 12;
    const bf16x8* base = j < 6 ? (j < 3 ? af0 : af1) : (j < 9 ? wf0 : wf1);
    src[i] = base + (size_t)(hf * N * 3 + (j % 3)) * 64;  // + it * 3 * 64 per stage
  }
  auto issue = [&](int it) {
    bf16x8* dst = stg + (it % NB) * LS_STAGE + (3 * wave) * 64;
#pragma unroll
    for (int i = 0; i < LS_NPW; ++i)
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src[i] + (size_t)it * 3 * 64),
                                       (__attribute__((address_space(3))) void*)(dst + i * 64), 16, 0, 0);
  };
  bf16x8 fa[2][3], fw[2][3];
  auto lread = [&](int it, int set) {
    const bf16x8* sb = stg + (it % NB) * LS_STAGE + kh * 12 * 64 + lane;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      fa[set][q] = sb[(3 * a + q) * 64];
      fw[set][q] = sb[(6 + 3 * c + q) * 64];
    }
  };
  floatx16 acc, acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = acc2[r] = 0.f;
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int it = 0; it < NB; ++it) issue(it);
  __builtin_amdgcn_sched_barrier(0);
  pre();  // waits for its own older loads with vmcnt(3 NB); issues exactly LS_GATHERS loads
  __builtin_amdgcn_sched_barrier(0);
  // stage 0 landed (younger: stages 1 .. NB-1 and the gathers)
  vm_wait(LS_NPW * (NB - 1) + LS_GATHERS);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  lread(0, 0);
#pragma unroll
  for (int it = 0; it < N; ++it) {
    const int set = it & 1;
    if (it + 1 < N) {
      // stage it + 1 landed: younger are the stages issued after it (up to it + NB - 1) and, while
      // it + 1 <= NB - 1, the gathers (issued after stage NB - 1)
      const int last = it + NB - 1 < N - 1 ? it + NB - 1 : N - 1;
      int younger = LS_NPW * (last - (it + 1)) + (it + 1 <= NB - 1 ? LS_GATHERS : 0);
      if (JK >= 0 && it >= JG + 1 && it + 1 <= SG) younger += NG2;
      if (JK >= 0 && it >= JK + 1 && it + 1 <= SK && wave == 0) younger += 1;
      vm_wait(younger);
      // every wave's stage-it reads retired (lgkmcnt) before any wave refills that buffer
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (it + NB < N) issue(it + NB);
      if constexpr (JK >= 0) {
        if (it == JK) {
          __builtin_amdgcn_sched_barrier(0);
          kdma();
          __builtin_amdgcn_sched_barrier(0);
        }
        if (it == JG) {
          __builtin_amdgcn_sched_barrier(0);
          mid();
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      lread(it + 1, set ^ 1);
    }
    x3_step2(acc2, acc, fa[set], fw[set]);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] += acc2[r];  // large-product chain + small-product chain
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // ring free: Pt aliases it
  const int li = lane & 31, lh = lane >> 5;
  float* dst = Pt + (c * 32 + li) * CP + a * 32 + 4 * lh;
  if (kh) {
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4)
      *reinterpret_cast<float4*>(dst + 8 * r4) = make_float4(acc[4 * r4], acc[4 * r4 + 1], acc[4 * r4 + 2], acc[4 * r4 + 3]);
  }
  __syncthreads();
  if (!kh) {
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      float4* e = reinterpret_cast<float4*>(dst + 8 * r4);
      const float4 v = *e;
      *e = make_float4(acc[4 * r4] + v.x, acc[4 * r4 + 1] + v.y, acc[4 * r4 + 2] + v.z, acc[4 * r4 + 3] + v.w);
    }
  }
}

// G (beam search): row m continues the hypothesis of row par[m] of the previous step, so its h
// fragments and c are gathered from that row (the beams of an image are adjacent rows, so the
// gathered 16-B fragment loads stay within the same or the neighbouring 32-row block).
// The previous step's rescoring, run inside k_lstm<H, false, true> (greedy steps t >= 1): workgroups
// 0 .. NR-1 rescore rows 2 bid, 2 bid + 1 of step t - 1 (k_vrescore's body, two 256-thread groups)
// and publish each row's argmax key as one agent-scope 8-byte store into keys[t-1] (zeroed before
// the decode, so a nonzero key is the readiness tag); the GEMM workgroups run the token-independent
// h W_hh^T phase meanwhile and only then wait for their 64 rows' keys.  A GEMM workgroup never waits
// on a workgroup that might not be resident: past RS_WAIT_TICKS of polling it rescores the missing
// rows itself (the same function on the same inputs: the same key), so the launch cannot deadlock
// whatever the dispatch order or the co-resident work of other streams.
struct RsArgs {
  int NR, Vp, T, t_step;
  uint64_t wait;  // poll bound in ticks of the 100 MHz clock (RS_WAIT_TICKS; 0: AA_DECODE_RS_SELF)
  const float* u;
  const float4* summ;
  const float* W;
  const float* bias;
  uint64_t* keys;  // keys[t-1] (B entries)
  int64_t* ids;
};
template <int H>
struct RsScratch;
template <int H, bool PUB>
__device__ __forceinline__ uint64_t rescore_row(int b, bool write, int t, int V, int Vp, const float* __restrict__ u,
                                                const float4* __restrict__ summ, const float* __restrict__ W,
                                                const float* __restrict__ bias, uint64_t* __restrict__ keys,
                                                int64_t* __restrict__ ids, int T, int t_step, float* scr);
constexpr uint64_t RS_WAIT_TICKS = 5000;  // 50 us of the 100 MHz constant clock
// ring iterations (of H / 32) at which k_lstm<.., RS> DMAs the tile's keys and gathers the table rows
constexpr int LS_RS_JK = 10, LS_RS_JG = LS_RS_JK + 3;
// SENT = false: the baseline model's step -- the sentinel's x W_x^T gathers (sa, sb) are not issued,
// so the gathers are LS_GATHERS - 2 ordinary loads (the ring's counted waits are told so), and the
// cell tail is lstm_cell_tail<H, false>; s_out is not written.
template <int H, bool G = false, bool RS = false, bool SENT = true>
__global__ __launch_bounds__(512, 4) void k_lstm(int B, int V, const int64_t* __restrict__ tok, int tok_ld,
                                              const float* __restrict__ table,
                                              const float* __restrict__ xg, const bf16x8* __restrict__ hsp_in,
                                              const float* __restrict__ c_in, const int* __restrict__ par,
                                              const bf16x8* __restrict__ whh3,
                                              const float* __restrict__ wgs, float* __restrict__ h_out,
                                              bf16x8* __restrict__ hsp_out, float* __restrict__ c_out,
                                              float* __restrict__ s_out, float* __restrict__ part, RsArgs ra) {
  constexpr int BM = 64, CP = LS_CP, TS = 64 * LS_CP;
  AA_TS(0, 0);
  // the LDS-DMA ring of lstm_gemm_lds (72 KB; the summed tile and the cell tail alias it)
  constexpr int RING_FLOATS = (LS_NB < H / 32 ? LS_NB : H / 32) * LS_STAGE * 4;
  // + the tile's 64 tokens (+ RS: the missing-row mask and slow-path flag, the 64 keys' low words
  // DMA'd mid-ring)
  constexpr int LDS_FLOATS = RING_FLOATS + 64 + 4 + (RS ? 64 : 0);
  static_assert(TS + LS_TAIL_FLOATS <= LDS_FLOATS, "tile + tail must fit in the ring");
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  constexpr int NTn = H / 16, KC = H / 16;
  const int MT = (B + BM - 1) / BM;
  int bid = blockIdx.x;
  if constexpr (RS) {
    static_assert(!G, "the fused rescoring is the greedy path's");
    static_assert(TS + 2 * RsScratch<H>::FLOATS <= RING_FLOATS, "two rescoring scratch areas beside the tile");
    if (bid < ra.NR) {  // rescoring role (uniform per workgroup): rows 2 bid + (t >> 8)
      AA_TS(4, 0);
      const int row = 2 * bid + (int)(threadIdx.x >> 8);
      rescore_row<H, true>(row < B ? row : B - 1, row < B, threadIdx.x & 255, V, ra.Vp, ra.u, ra.summ, ra.W,
                           ra.bias, ra.keys, ra.ids, ra.T, ra.t_step, lds + (threadIdx.x >> 8) * RsScratch<H>::FLOATS);
      AA_TS(4, 1);
      return;
    }
    bid -= ra.NR;
  }
  const int L = xcd_remap(bid, MT * NTn);
  const int nt = L / MT, mt = L % MT;  // m fastest: a weight tile is shared inside an XCD
  const int t = threadIdx.x, lane = t & 63;
  const int m0 = mt * BM;
  float* Pt = lds;  // [4][64][CP] partial tiles
  const int rr = t >> 3, u0 = (t & 7) * 2, m = m0 + rr;
  const int mc = m < B ? m : B - 1;  // rows >= B compute on row B-1 and store nothing
  const int j = nt * 16 + u0;
  // (token first, then the GEMM's first loads, then the token-dependent gathers: in-order vmcnt
  //  then waits for the token alone; the asm barriers keep the compiler from reordering the loads)
  int64_t tk = 0;
  int* tok_lds = reinterpret_cast<int*>(lds + RING_FLOATS);
  // the tile's 64 tokens by ONE LDS-DMA of wave 0 (the low dword of each int64 token), so that no
  // ordinary load is outstanding beside the ring's DMAs: hipcc drains every DMA (vmcnt(0)) before
  // the first use of an ordinary load's result while a DMA is in flight
  // (tok == nullptr: the first step of a greedy decode, every row starts from <start> = 1: no load)
  if (t < 64 && tok) {
    const int r = m0 + t < B ? m0 + t : B - 1;
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(tok + (int64_t)r * tok_ld),
                                     (__attribute__((address_space(3))) void*)tok_lds, 4, 0, 0);
  }
  const bf16x8* af0;
  const bf16x8* af1;
  int pc = mc;  // source row of c (and of h, through the fragments)
  if constexpr (G) {
    const int ra0 = m0 + (lane & 31), ra1 = ra0 + 32;
    const int p0 = par[ra0 < B ? ra0 : B - 1], p1 = par[ra1 < B ? ra1 : B - 1];
    const int hl = 32 * (lane >> 5);
    af0 = hsp_in + (size_t)(p0 >> 5) * KC * 3 * 64 + (p0 & 31) + hl;
    af1 = hsp_in + (size_t)(p1 >> 5) * KC * 3 * 64 + (p1 & 31) + hl;
    pc = par[mc];
  } else {
    af0 = hsp_in + (size_t)(m0 / 32) * KC * 3 * 64 + lane;
    af1 = af0 + (size_t)KC * 3 * 64;
  }
  const bf16x8* wf0 = whh3 + (size_t)(nt * 2) * KC * 3 * 64 + lane;
  const bf16x8* wf1 = wf0 + (size_t)KC * 3 * 64;
  // epilogue gathers behind the first GEMM loads: token -> table row, x_g, c, W_g/W_s slice
  float2 ta[4], xa[4], sa, sb, cprev;
  if constexpr (!SENT) sa = sb = make_float2(0.f, 0.f);  // (not gathered, not read)
  constexpr int NGATH = SENT ? LS_GATHERS : LS_GATHERS - 2;  // ordinary loads of gathers()
  constexpr int NWS4 = (SENT ? 2 : 1) * P * 4;               // float4s of the tile's W_g (/ W_s) slice in use
  float4 wsv;
  const int N5 = 5 * H;
  // the token's table row (5 loads)
  auto gather_table = [&] {
    tk = tk < 0 ? 0 : (tk >= V ? V - 1 : tk);
    const float* trow = table + tk * N5;
#pragma unroll
    for (int g = 0; g < 4; ++g) ta[g] = *reinterpret_cast<const float2*>(trow + nt * 64 + g * 16 + u0);
    if constexpr (SENT) sa = *reinterpret_cast<const float2*>(trow + 4 * H + j);
  };
  // the token-independent operands: x_g, c, the W_g / W_s slice (7 loads)
  auto gather_x = [&] {
    const float* xrow = xg + (int64_t)mc * N5;
#pragma unroll
    for (int g = 0; g < 4; ++g) xa[g] = *reinterpret_cast<const float2*>(xrow + nt * 64 + g * 16 + u0);
    if constexpr (SENT) sb = *reinterpret_cast<const float2*>(xrow + 4 * H + j);
    cprev = *reinterpret_cast<const float2*>(c_in + (int64_t)pc * H + j);
    // W_g / W_s slice: wgs[tile] is [98][16] (j-major); thread t < 392 takes float4 t
    const float4* src = reinterpret_cast<const float4*>(wgs + (int64_t)nt * 2 * P * 16);
    wsv = src[t < NWS4 ? t : NWS4 - 1];
  };
  auto gathers = [&] {
    gather_table();
    gather_x();
  };
  // token first (oldest), then the ring's first three stages, then -- once the token is in --
  // the token-dependent gathers (exactly LS_GATHERS loads, counted by the ring's waits)
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (RS) {
    // The GEMM phase needs no token.  At ring iteration LS_RS_JK wave 0 DMAs the low words of the
    // tile's 64 keys into LDS (agent-coherent sc1 reads of the granules the rescoring workgroups
    // publish: a non-zero low word = published, it is 0xFFFFFFFF - token), and at iteration LS_RS_JG
    // -- that DMA landed -- every thread takes its row's token if published and issues all twelve
    // gathers (table row, x_g, c, W_g / W_s slice: issued there rather than with the first stages, so
    // they are not live across the whole ring), which land under the last iterations.  Rows not yet published then are polled / rescored after the ring, as before,
    // and only their table rows are gathered again.
    uint32_t* klo = reinterpret_cast<uint32_t*>(lds + RING_FLOATS + 64 + 4);
    // (hooks scaled to the ring's H / 32 iterations; rings under 12 iterations: gathers after the ring)
    constexpr int NI = H / 32, JK = NI >= 12 ? LS_RS_JK * NI / 16 : -1, JG = JK < 0 ? -1 : JK + (LS_RS_JG - LS_RS_JK);
    lstm_gemm_lds<H, 0, JK, JG, NGATH>(
        af0, af1, wf0, wf1, reinterpret_cast<bf16x8*>(lds), Pt, [] {},
        [&] {
          if (t < 64) {
            const int r = m0 + t < B ? m0 + t : B - 1;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(ra.keys + r),
                                             (__attribute__((address_space(3))) void*)klo, 4, 0, 16 /* sc1 */);
          }
        },
        [&] {
          const uint32_t kl = klo[rr];
          tk = kl != 0u ? (int64_t)(0xFFFFFFFFu - kl) : 0;  // not yet published: gathered again below
          gathers();
        });
    AA_TS(0, 5);
    __syncthreads();
    uint64_t* miss = reinterpret_cast<uint64_t*>(lds + RING_FLOATS + 64);
    if (t < 64) {
      const uint32_t kl = JK < 0 ? 0u : klo[t];
      if (__all(kl != 0u)) {  // wave-uniform: every row was published by iteration JK
        if (t == 0) miss[0] = 0, miss[1] = 0;
      } else {
        const int r = m0 + t < B ? m0 + t : B - 1;
        uint64_t k = __hip_atomic_load(ra.keys + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t t0 = wall_clock64();
        while (!__all(k != 0)) {  // wave-uniform: bounded poll of the 8-byte granules
          if (wall_clock64() - t0 > ra.wait) break;
          __builtin_amdgcn_s_sleep(1);
          if (k == 0) k = __hip_atomic_load(ra.keys + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        tok_lds[t] = (int)key_token(k);
        const uint64_t mb = __ballot(k == 0);
        if (t == 0) miss[0] = mb, miss[1] = 1;
      }
    }
    __syncthreads();
    if (miss[1]) {  // (workgroup-uniform) some key came after iteration JK: the slow path
      uint64_t mb = miss[0];
      // rows not yet published: rescored here, two at a time (the tile's Pt stays below the scratch)
      while (mb) {
        const int i0 = __builtin_ctzll(mb);
        mb &= mb - 1;
        const int i1 = mb ? __builtin_ctzll(mb) : i0;
        if (mb) mb &= mb - 1;
        const int i = (t >> 8) ? i1 : i0;
        const int r = m0 + i < B ? m0 + i : B - 1;
        const uint64_t k = rescore_row<H, true>(r, (t >> 8) == 0 || i1 != i0, t & 255, V, ra.Vp, ra.u, ra.summ, ra.W,
                                                ra.bias, ra.keys, ra.ids, ra.T, ra.t_step,
                                                lds + TS + (t >> 8) * RsScratch<H>::FLOATS);
        if ((t & 255) == 0) tok_lds[i] = (int)key_token(k);
        __syncthreads();
      }
      // every gather again (the mid-ring values are dead on this path, so they are not kept live
      // across the rescoring above)
      tk = tok_lds[rr];
      gathers();
    }
  } else {
    lstm_gemm_lds<H, NGATH>(af0, af1, wf0, wf1, reinterpret_cast<bf16x8*>(lds), Pt, [&] {
      // wave 0's token DMA is older than its ring DMAs: retire it, then every wave reads its row's
      if (t < 64) vm_wait(LS_NPW * (LS_NB < H / 32 ? LS_NB : H / 32));
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      tk = tok ? tok_lds[rr] : 1;
      gathers();
      asm volatile("" ::: "memory");
    });
  }
  AA_TS(0, 1);
  __syncthreads();
  float gate[4][2];
  {
    const float* cr = Pt + rr;  // column j of the summed tile at cr[j * CP]
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int q = 0; q < 2; ++q) gate[g][q] = cr[(16 * g + u0 + q) * CP] + ((&ta[g].x)[q] + (&xa[g].x)[q]);
  }
  AA_TS(0, 2);
  lstm_cell_tail<H, SENT>(B, m0, nt, gate, sa, sb, cprev, wsv, lds + TS, h_out, hsp_out, c_out, s_out, part);
  AA_TS(0, 4);
}

__global__ void k_fill_tok(int64_t* __restrict__ tok, int B, int64_t v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) tok[i] = v;
}
// Start of a greedy decode: <start> tokens, and (exact vocab stage) the [T][B] argmax keys that
// k_vocab accumulates by atomicMax cleared -- by memory-side stores, like the atomics that follow (a
// plain store's line would stay in this XCD's L2)
__global__ void k_decode_init(int64_t* __restrict__ tok, int B, int64_t v, uint64_t* __restrict__ keys, int n) {
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (int i = i0; i < B; i += stride) tok[i] = v;
  if (keys)
    for (int i = i0; i < n; i += stride) __hip_atomic_store(keys + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// The arithmetic of one attention row once its operands are in registers, shared by k_atten5 and
// the attention role of the fused launch k_lstm<.., AT> (so the two produce the same bits).  Thread t
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
// Partner exchange for the screen epilogue's butterfly over the 32 lanes of a column block: level
// M pairs each lane with one whose index differs in bit M and agrees in the bits above it --
// M = 16: ds_swizzle xor 16; 8: DPP row_mirror (i <-> 15 - i); 4: row_half_mirror (i <-> 7 - i);
// 2, 1: DPP quad_perm xor 2 / xor 1.  No LDS traffic except the one swizzle level.
template <int M>
__device__ __forceinline__ uint32_t partner(uint32_t v) {
  if constexpr (M == 16) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);
  else if constexpr (M == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);
  else if constexpr (M == 4) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);
  else if constexpr (M == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
  else return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
}

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

// Exact fp32 logit of one column, computed by a group of 8 lanes (lane8 = 0..7): lane8 j runs the
// fma chain of partial j (K-steps [j*per, (j+1)*per) of 32, in the MFMA k order: pairs (s, 16+s)),
// then the fixed tree ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)) over xor-1/2/4 shuffles, then + bias.
// Bit-identical to k_vocab (gemm_mainloop_np<.., NP_VOCAB>).  All 8 lanes return the logit.
// u is read from LDS (urow), w straight from memory (each lane 4*32*per contiguous bytes).
template <int HC = 0>  // HC > 0: H known at compile time (the K steps' loads issue together)
__device__ __forceinline__ float exact_logit8(const float* __restrict__ urow, const float* __restrict__ wrow, int H,
                                              float b, int lane8) {
  const int per = (HC > 0 ? HC : H) / (32 * NP_VOCAB);
  const int k0 = lane8 * per * 32;
  float acc = 0.f;
  constexpr int KU = HC > 0 ? HC / (32 * NP_VOCAB) : 1;
#pragma unroll KU
  for (int ks = 0; ks < per; ++ks) {
    float4 w[8], u[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      w[q] = *reinterpret_cast<const float4*>(wrow + k0 + 32 * ks + 4 * q);
      u[q] = *reinterpret_cast<const float4*>(urow + k0 + 32 * ks + 4 * q);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      acc = __builtin_fmaf(f4c(u[s >> 2], s & 3), f4c(w[s >> 2], s & 3), acc);
      acc = __builtin_fmaf(f4c(u[4 + (s >> 2)], s & 3), f4c(w[4 + (s >> 2)], s & 3), acc);
    }
  }
  acc = acc + __shfl_xor(acc, 1, 64);
  acc = acc + __shfl_xor(acc, 2, 64);
  acc = acc + __shfl_xor(acc, 4, 64);
  return acc + b;
}

// ---------------------------------------------------------------------------------------------
// D3b (greedy path): one workgroup (4 waves) per row.  M = max over granules of lbmax; candidates
// = idx1 of granules with ub1 >= M, plus every column of granules with ub2 >= M (two candidates in
// one granule).  32 candidates are scored per pass (8 lanes each, exact_logit8); first-index argmax
// -> keys[row], ids[row, t].  A list longer than RS_CAP falls back to every column (correct, slow).
// (Tried: re-screening a ub2 >= M granule's 32 columns in bf16 here, sequentially or 64 columns per
// round, and scoring only those within the bound: fewer exact logits, but slower overall.  Also
// tried: each wave reading the W row of its best granule's arg-max column before the barriers, as a
// cache warm-up for the likely winner: k_vrescore 9.95 -> 10.4 us by events in A/B.)
// ---------------------------------------------------------------------------------------------
constexpr int RS_NT = 256, RS_NW = RS_NT / 64;
// LDS scratch of one rescored row (floats): u row, candidate list, count, wave maxima, wave keys
template <int H>
struct RsScratch {
  static constexpr int URow = 0, Cand = H, NCand = H + RS_CAP, WMax = NCand + 4, WBest = WMax + RS_NW + 4,
                       FLOATS = WBest + 2 * RS_NW;
  static_assert(H % 4 == 0 && WBest % 2 == 0, "16-B u row, 8-B keys");
};
// The rescoring of one row by RS_NT threads (t = 0 .. RS_NT-1 of the calling group; every thread of
// the workgroup reaches the same three barriers): k_vrescore's body.  PUB: the key is stored by an
// agent-scope atomic store (a write-through granule that k_lstm<.., RS> polls within its launch);
// write = false computes without storing (a padding group that only keeps the barrier count).
// Returns the row's key in every thread.
template <int H, bool PUB>
__device__ __forceinline__ uint64_t rescore_row(int b, bool write, int t, int V, int Vp, const float* __restrict__ u,
                                                const float4* __restrict__ summ, const float* __restrict__ W,
                                                const float* __restrict__ bias, uint64_t* __restrict__ keys,
                                                int64_t* __restrict__ ids, int T, int t_step, float* scr) {
  typedef RsScratch<H> S;
  float* urow = scr + S::URow;
  int* cand = reinterpret_cast<int*>(scr + S::Cand);
  int& ncand = *reinterpret_cast<int*>(scr + S::NCand);
  float* wmax = scr + S::WMax;
  uint64_t* wbest = reinterpret_cast<uint64_t*>(scr + S::WBest);
  const int lane = t & 63, w = t >> 6;
  const int NTn = Vp / VS_TILE;
  for (int d = 4 * t; d < H; d += 4 * RS_NT) *reinterpret_cast<float4*>(&urow[d]) = *reinterpret_cast<const float4*>(u + (int64_t)b * H + d);
  if (t == 0) ncand = 0;
  const float4* sm = summ + (int64_t)b * NTn;
  // a thread's first two summaries stay in registers between the max and the selection (any
  // further ones are read again)
  float4 s0 = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f), s1 = s0;
  if (t < NTn) s0 = sm[t];
  if (t + RS_NT < NTn) s1 = sm[t + RS_NT];
  float mlb = fmaxf(s0.x, s1.x);
  for (int i = t + 2 * RS_NT; i < NTn; i += RS_NT) mlb = fmaxf(mlb, sm[i].x);
  mlb = wave_max(mlb);
  if (lane == 0) wmax[w] = mlb;
  __syncthreads();
  AA_TS(3, 1);
  mlb = wmax[0];
#pragma unroll
  for (int i = 1; i < RS_NW; ++i) mlb = fmaxf(mlb, wmax[i]);
  auto select = [&](const float4& s, int i) {
    if (s.z >= mlb) {  // >= 2 candidates in this granule: take all of its columns
      const int pos = atomicAdd(&ncand, VS_TILE);
      for (int c = 0; c < VS_TILE; ++c)
        if (pos + c < RS_CAP) cand[pos + c] = i * VS_TILE + c;
    } else if (s.y >= mlb) {
      const int pos = atomicAdd(&ncand, 1);
      if (pos < RS_CAP) cand[pos] = __float_as_int(s.w);
    }
  };
  if (t < NTn) select(s0, t);
  if (t + RS_NT < NTn) select(s1, t + RS_NT);
  for (int i = t + 2 * RS_NT; i < NTn; i += RS_NT) select(sm[i], i);
  __syncthreads();
  AA_TS(3, 2);
  // an empty list (summaries that are all NaN) or an overflowing one: every column; the key starts at
  // the lowest non-zero key, so a published key is never 0 (0 = "not yet published" for k_lstm<.., RS>)
  const bool all = ncand > RS_CAP || ncand == 0;
  const int n = all ? V : ncand;
  const int g = t >> 3, lane8 = t & 7;
  uint64_t best = argmax_key(-INFINITY, V - 1);
  for (int i = g; i < n; i += RS_NT / 8) {
    int col = all ? i : cand[i];
    const bool ok = col < V;
    col = ok ? col : V - 1;
    // (the K steps' loads one after the other: measured faster here than all issued together)
    const float x = exact_logit8(urow, W + (int64_t)col * H, H, bias[col], lane8);
    if (ok) {
      const uint64_t k = argmax_key(x, col);
      best = k > best ? k : best;
    }
  }
  best = wave_max_u64(best);
  if (lane == 0) wbest[w] = best;
  __syncthreads();
  uint64_t k = wbest[0];
#pragma unroll
  for (int i = 1; i < RS_NW; ++i) k = wbest[i] > k ? wbest[i] : k;
  if (t == 0 && write) {
    if (ids) ids[(int64_t)b * T + t_step] = key_token(k);
    if constexpr (PUB) __hip_atomic_store(keys + b, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else keys[b] = k;
  }
  return k;
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

// ---------------------------------------------------------------------------------------------
// D3 (exact path): logits = u W_m^T + b_m (AdaptiveBlock.mlp, adaptive_attention.py:132) with the
// argmax of sampler (:201) fused into the epilogue: per-row max over the tile's columns by 64-bit
// keys (lane shuffles, then LDS across the two column waves), one atomicMax per row per workgroup.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vocab(int B, int H, int V, int Vp, int ld, const float* __restrict__ u,
                                               const float* __restrict__ W, const float* __restrict__ bias,
                                               float* __restrict__ scores, uint64_t* __restrict__ keys) {
  constexpr int BM = 64, BN = 64;
  __shared__ __attribute__((aligned(16))) float lds[Tile<BM, BN>::LDS_FLOATS];
  const int MT = (B + BM - 1) / BM, NTn = Vp / BN;
  const int L = xcd_remap(blockIdx.x, MT * NTn);
  const int nt = L / MT, mt = L % MT;
  ARowMajor al{u, H, mt * BM, B};
  WRowMajor wl{W, H, nt * BN};
  floatx16 acc[NP_VOCAB][1][1];
  gemm_mainloop_np<BM, BN, NP_VOCAB>(al, wl, H / BK, lds, acc);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  const int col = nt * BN + wn * 32 + (lane & 31);
  const bool valid = col < V;
  const float bv = bias[col];
  uint64_t best[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float p01 = acc[0][0][0][r] + acc[1][0][0][r], p23 = acc[2][0][0][r] + acc[3][0][0][r];
    const float p45 = acc[4][0][0][r] + acc[5][0][0][r], p67 = acc[6][0][0][r] + acc[7][0][0][r];
    const float x = ((p01 + p23) + (p45 + p67)) + bv;
    const int row = mt * BM + wm * 32 + acc_row(r, lane);
    if (scores && valid && row < B) scores[(int64_t)row * ld + col] = x;
    uint64_t k = valid ? argmax_key(x, col) : 0ull;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const uint64_t y = shfl_xor_u64(k, o);
      k = y > k ? y : k;
    }
    best[r] = k;
  }
  uint64_t* red = reinterpret_cast<uint64_t*>(lds);  // [2 column waves][64 rows]
  if ((lane & 31) == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wn * 64 + wm * 32 + acc_row(r, lane)] = best[r];
  }
  __syncthreads();
  if (t < 64) {
    const uint64_t a = red[t], c = red[64 + t];
    const int row = mt * BM + t;
    if (row < B && keys) atomicMax(reinterpret_cast<unsigned long long*>(keys + row), (unsigned long long)(a > c ? a : c));
  }
}

// ids [B][T] from the argmax keys [T][ldk] (ldk = the whole batch when B is a lane's row block)
__global__ void k_finalize(const uint64_t* __restrict__ keys, int B, int T, int64_t* __restrict__ ids, int ldk) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T) return;
  const int b = (int)(i / T), t = (int)(i % T);
  ids[i] = key_token(keys[(int64_t)t * ldk + b]);
}

// ---------------------------------------------------------------------------------------------
// packing / synthetic data
// ---------------------------------------------------------------------------------------------
// Gate-interleaved LSTM tiles: packed row r = tile*64 + gate*16 + unit  <-  reference row
// gate*H + tile*16 + unit of W_ih / W_hh / biases (gate order i, f, g, o); rows 4H + j of the
// emb / v_g parts are W_x row j (sentinel).
__global__ void k_pack_lstm(const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                            const float* __restrict__ b_hh, const float* __restrict__ w_x, int E, int H,
                            float* __restrict__ whh, float* __restrict__ wemb, float* __restrict__ wvg, float* __restrict__ bias5) {
  const int r = blockIdx.x;  // 0 .. 5H-1
  const int KX = 2 * E;
  if (r < 4 * H) {
    const int tile = r / 64, g = (r % 64) / 16, un = r % 16;
    const int src = g * H + tile * 16 + un;
    for (int k = threadIdx.x; k < E; k += blockDim.x) {
      wemb[(int64_t)r * E + k] = w_ih[(int64_t)src * KX + k];
      wvg[(int64_t)r * E + k] = w_ih[(int64_t)src * KX + E + k];
    }
    for (int k = threadIdx.x; k < H; k += blockDim.x) whh[(int64_t)r * H + k] = w_hh[(int64_t)src * H + k];
    if (threadIdx.x == 0) bias5[r] = b_ih[src] + b_hh[src];
  } else if (w_x) {  // (a baseline model has no sentinel: its fifth block stays zero)
    const int j = r - 4 * H;
    for (int k = threadIdx.x; k < E; k += blockDim.x) {
      wemb[(int64_t)r * E + k] = w_x[(int64_t)j * KX + k];
      wvg[(int64_t)r * E + k] = w_x[(int64_t)j * KX + E + k];
    }
    if (threadIdx.x == 0) bias5[r] = 0.f;
  }
}

// wgs[tile][j][u] = (j < 49 ? W_g[j] : W_s[j - 49])[tile*16 + u]
// W_a split into three bf16 planes in MFMA-fragment order (see k_enc_v3): block = (nb, kc), lane l
// -> W[32 nb + (l & 31)][16 kc + 8 (l >> 5) + j], planes q = 0, 1, 2 at out[((nb KC + kc) 3 + q) 64 + l].
__global__ void k_pack_w3(const float* __restrict__ w, int C, bf16x8* __restrict__ out) {
  const int KC = C / 16, nb = blockIdx.x / KC, kc = blockIdx.x % KC, l = threadIdx.x;
  const float* src = w + (int64_t)(32 * nb + (l & 31)) * C + 16 * kc + 8 * (l >> 5);
  bf16x8 h, m, lo;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 a, b, c;
    split3(src[j], a, b, c);
    h[j] = a; m[j] = b; lo[j] = c;
  }
  bf16x8* o = out + ((size_t)blockIdx.x * 3) * 64 + l;
  o[0] = h;
  o[64] = m;
  o[128] = lo;
}

// W_a split into three bf16 planes in 16x16x32 B-fragment order (see k_enc_v4): block = (nb, kc),
// lane l -> W[16 nb + (l & 15)][32 kc + 8 (l >> 4) + j], planes at out[((nb KC + kc) 3 + q) 64 + l].
__global__ void k_pack_w4(const float* __restrict__ w, int C, bf16x8* __restrict__ out) {
  const int KC = C / 32, nb = blockIdx.x / KC, kc = blockIdx.x % KC, l = threadIdx.x;
  const float* src = w + (int64_t)(16 * nb + (l & 15)) * C + 32 * kc + 8 * (l >> 4);
  bf16x8 h, m, lo;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 a, b, c;
    split3(src[j], a, b, c);
    h[j] = a; m[j] = b; lo[j] = c;
  }
  bf16x8* o = out + ((size_t)blockIdx.x * 3) * 64 + l;
  o[0] = h;
  o[64] = m;
  o[128] = lo;
}

__global__ void k_pack_wgs(const float* __restrict__ wg, const float* __restrict__ ws, int H, float* __restrict__ out) {
  const int tile = blockIdx.x;
  // (ws == nullptr: a baseline model, the W_s half stays zero)
  for (int i = threadIdx.x; i < (ws ? 2 : 1) * P * 16; i += blockDim.x) {
    const int j = i / 16, u = i % 16;
    const float* src = j < P ? wg + (int64_t)j * H : ws + (int64_t)(j - P) * H;
    out[(int64_t)tile * 2 * P * 16 + i] = src[tile * 16 + u];
  }
}

// bf16 copy of W_m (zero rows beyond V) and, for the screen bound, the row norms ||w_n||_2 (wn[n])
// and ||w_n - bf16(w_n)||_2 (wn[Vp + n]), each inflated by 1e-4 over its fp32 rounding (a sum of
// H <= 1024 squares: relative error <= gamma_1024 ~ 6.1e-5, then the square root).
__global__ void k_pack_mlp(const float* __restrict__ w, int V, int H, int Vp, uint16_t* __restrict__ wb,
                           float* __restrict__ wn) {
  const int n = blockIdx.x, lane = threadIdx.x;  // 64 threads
  float s = 0.f, sd = 0.f;
  for (int k = lane; k < H; k += 64) {
    const float x = n < V ? w[(int64_t)n * H + k] : 0.f;
    const uint16_t xb = f2bf(x);
    wb[frag_off(n, k, H)] = xb;
    const float d = x - __uint_as_float((uint32_t)xb << 16);  // exact (Sterbenz)
    s = __builtin_fmaf(x, x, s);
    sd = __builtin_fmaf(d, d, sd);
  }
  s = wave_sum(s);
  sd = wave_sum(sd);
  if (lane == 0) {
    wn[n] = sqrtf(s) * 1.0001f;
    wn[Vp + n] = sqrtf(sd) * 1.0001f;
  }
}

// Per 32-column granule of the vocab: (max ||w_n||, max |b_n|, max ||w_n - bf16(w_n)||, 0) for the
// screen's bound.
__global__ void k_pack_gs(const float* __restrict__ wn, const float* __restrict__ b, int Vp, float4* __restrict__ gs) {
  const int g = blockIdx.x, l = threadIdx.x;  // 64 threads, lanes >= 32 mirror 0..31
  const int n = g * VS_TILE + (l & (VS_TILE - 1));
  const float mw = wave_max(wn[n]), mb = wave_max(fabsf(b[n])), md = wave_max(wn[Vp + n]);
  if (l == 0) gs[g] = make_float4(mw, mb, md, 0.f);
}

__device__ __forceinline__ uint64_t splitmix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
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

static int launch_status() { return aa_launch_status(); }
static bool al16(const void* p) { return aa_al16(p); }

static void gemm_bias(const float* A, int lda, int M, const float* W, int ldw, int N, int K, const float* bias, float* C,
                      int64_t ldc, hipStream_t s) {
  const int MT = (M + 63) / 64, NTn = N / 64;
  hipLaunchKernelGGL(k_gemm_bias, dim3(MT * NTn), dim3(256), 0, s, A, lda, M, W, ldw, N, K, bias, C, ldc);
}

int aa_abi_version(void) { return AA_ABI_VERSION; }
#ifdef AA_TS_ENABLE
extern "C" __attribute__((visibility("default"))) int aa_ts_setup(void* buf) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(aa_ts_buf), &buf, sizeof(buf));
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

static int check_model(const aa_model* m, Layout* L) {
  if (!m || !m->packed) return AA_ERR_NULL;
  int rc = aa_check_dims(&m->dims);
  if (rc) return rc;
  *L = make_layout(m->dims);
  if (m->packed_bytes < L->total_floats * sizeof(float)) return AA_ERR_BUFFER;
  if (((uintptr_t)m->packed & 255u) != 0) return AA_ERR_ALIGN;
  return AA_OK;
}

int aa_pack_weights(const aa_model* m, const aa_ref_weights* w, aa_stream_t stream) {
  Layout L;
  int rc = check_model(m, &L);
  if (rc) return rc;
  if (!w) return AA_ERR_NULL;
  const float* req[] = {w->enc_affine_a_w, w->enc_affine_a_b, w->enc_affine_b_w, w->enc_affine_b_b,
                        w->enc_affine_h0_w, w->enc_affine_h0_b, w->enc_affine_c0_w, w->enc_affine_c0_b,
                        w->embed_w, w->lstm_w_ih, w->lstm_w_hh, w->lstm_b_ih, w->lstm_b_hh,
                        w->att_affine_v_w, w->att_affine_g_w, w->att_affine_h_w, w->mlp_w, w->mlp_b};
  for (const float* p : req)
    if (!p) return AA_ERR_NULL;
  // both sentinel weights NULL: a baseline (no-sentinel) model, whose sentinel blocks stay zero; one
  // without the other is an error
  const bool baseline = !w->sent_affine_x_w && !w->att_affine_s_w;
  if (!baseline && (!w->sent_affine_x_w || !w->att_affine_s_w)) return AA_ERR_NULL;
  if (!al16(w->embed_w)) return AA_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  float* base = static_cast<float*>(m->packed);
  const int E = L.E, H = L.H, V = L.V, C = L.C;
  AA_TRY(hipMemsetAsync(base, 0, L.total_floats * sizeof(float), s));
  auto cp = [&](const float* src, size_t off, size_t n) {
    return hipMemcpyAsync(base + off, src, n * sizeof(float), hipMemcpyDeviceToDevice, s);
  };
  AA_TRY(cp(w->enc_affine_a_w, L.enc_a_w, (size_t)H * C));
  AA_TRY(cp(w->enc_affine_a_b, L.enc_a_b, H));
  AA_TRY(cp(w->enc_affine_b_w, L.heads_w, (size_t)E * C));
  AA_TRY(cp(w->enc_affine_h0_w, L.heads_w + (size_t)E * C, (size_t)H * C));
  AA_TRY(cp(w->enc_affine_c0_w, L.heads_w + (size_t)(E + H) * C, (size_t)H * C));
  AA_TRY(cp(w->enc_affine_b_b, L.heads_b, E));
  AA_TRY(cp(w->enc_affine_h0_b, L.heads_b + E, H));
  AA_TRY(cp(w->enc_affine_c0_b, L.heads_b + E + H, H));
  AA_TRY(cp(w->att_affine_v_w, L.wv, (size_t)P * H));  // rows 49..63 stay zero
  AA_TRY(cp(w->att_affine_g_w, L.wg, (size_t)P * H));
  if (!baseline) AA_TRY(cp(w->att_affine_s_w, L.ws, (size_t)P * H));
  AA_TRY(cp(w->att_affine_h_w, L.wh, P));
  AA_TRY(cp(w->mlp_w, L.mlp_w, (size_t)V * H));        // rows V..Vp-1 stay zero
  AA_TRY(cp(w->mlp_b, L.mlp_b, V));
  hipLaunchKernelGGL(k_pack_lstm, dim3(L.N5), dim3(256), 0, s, w->lstm_w_ih, w->lstm_w_hh, w->lstm_b_ih, w->lstm_b_hh,
                     w->sent_affine_x_w, E, H, base + L.whh, base + L.wemb, base + L.wvg, base + L.bias5);
  // table[v] = embed[v] . [W_ih(emb part) (packed gate order); W_x(emb part)]^T
  gemm_bias(w->embed_w, E, V, base + L.wemb, E, L.N5, E, nullptr, base + L.table, L.N5, s);
  hipLaunchKernelGGL(k_pack_mlp, dim3(L.Vp), dim3(64), 0, s, base + L.mlp_w, V, H, L.Vp,
                     reinterpret_cast<uint16_t*>(base + L.mlp_wb), base + L.mlp_wn);
  hipLaunchKernelGGL(k_pack_gs, dim3(L.Vp / VS_TILE), dim3(64), 0, s, base + L.mlp_wn, base + L.mlp_b, L.Vp,
                     reinterpret_cast<float4*>(base + L.mlp_gs));
  hipLaunchKernelGGL(k_pack_wgs, dim3(H / 16), dim3(256), 0, s, w->att_affine_g_w, w->att_affine_s_w, H, base + L.wgs);
  hipLaunchKernelGGL(k_pack_w3, dim3((H / 32) * (C / 16)), dim3(64), 0, s, w->enc_affine_a_w, C,
                     reinterpret_cast<bf16x8*>(base + L.enc_w3));
  hipLaunchKernelGGL(k_pack_w3, dim3((4 * H / 32) * (H / 16)), dim3(64), 0, s, base + L.whh, H,
                     reinterpret_cast<bf16x8*>(base + L.whh3));
  hipLaunchKernelGGL(k_pack_w3, dim3((L.Vp / 32) * (H / 16)), dim3(64), 0, s, base + L.mlp_w, H,
                     reinterpret_cast<bf16x8*>(base + L.mlp_w3));
  hipLaunchKernelGGL(k_pack_w4, dim3((H / 16) * (C / 32)), dim3(64), 0, s, w->enc_affine_a_w, C,
                     reinterpret_cast<bf16x8*>(base + L.enc_w4));
  hipLaunchKernelGGL(k_pack_w4, dim3((L.NHp / 16) * (C / 32)), dim3(64), 0, s, base + L.heads_w, C,
                     reinterpret_cast<bf16x8*>(base + L.heads_w4));
  if (E % 32 == 0)
    hipLaunchKernelGGL(k_pack_w4, dim3((L.N5 / 16) * (E / 32)), dim3(64), 0, s, base + L.wvg, E,
                       reinterpret_cast<bf16x8*>(base + L.wvg4));
  if (H % 32 == 0)
    hipLaunchKernelGGL(k_pack_w4, dim3((PP / 16) * (H / 32)), dim3(64), 0, s, base + L.wv, H,
                       reinterpret_cast<bf16x8*>(base + L.wv4));
  return launch_status();
}

static inline void rec(aa_event_t* arr, int i, hipStream_t s) {
  if (arr) (void)hipEventRecord((hipEvent_t)arr[i], s);
}
// Per-kernel timing hook (aa_trace): with an event array, the pair (I, I + 1) is handed to the launch
// itself (hipExtLaunchKernel's start / stop events), which stamps it with the dispatch's own begin /
// end timestamps -- the figures rocprofv3's kernel trace reads -- and no event packet sits between the
// timed launches.  (Round 4 recorded events around each launch: ~1.5-3 us per launch of skew, and a
// traced decode 1.46x slower than an untraced one.)  Kernel names with commas go in parentheses.
#define AA_TLAUNCH(EV, I, K, G, BL, SH, S, ...)                                                              \
  do {                                                                                                       \
    aa_event_t* ev_ = (EV);                                                                                  \
    if (ev_)                                                                                                 \
      hipExtLaunchKernelGGL(K, G, BL, SH, S, (hipEvent_t)ev_[(I)], (hipEvent_t)ev_[(I) + 1], 0u, __VA_ARGS__); \
    else                                                                                                     \
      hipLaunchKernelGGL(K, G, BL, SH, S, __VA_ARGS__);                                                      \
  } while (0)

// Encoder tail.  With an aux stream, the a_g branch (k_avgpool -> k_enc_heads -> x_g GEMM: HBM- and
// latency-bound) runs beside the V branch (k_enc_v3 -> VWv GEMM: MFMA-bound); both read only the
// features, and `s` waits for aux before returning.
// the encoder's V GEMM runs on k_enc_v4 (which also writes the compressed V when asked)
static bool enc_v4(const Layout& L, int32_t flags) {
  return !(flags & AA_DECODE_FP32_ENCODER) && (L.H == 512 || L.H == 256) && L.C <= E4_MAXC;
}
// x_g and VWv on k_gemm3 (bf16x3) unless an fp32-MFMA encoder was asked for; K % 256 == 0 (4 waves)
static bool gemm3_ok(int32_t flags, int K) {
  return !(flags & AA_DECODE_FP32_ENCODER) && K % 256 == 0;
}
// hsp0 != nullptr (greedy decode): h0 split into the 3-plane fragments k_lstm reads, on `s` after the
// VWv GEMM, waiting for the heads only (the aux stream's x_g GEMM is still running: off the critical path)
// init: the greedy decode's k_decode_init (the [T][B] key clear), launched on the aux stream beside
// k_enc_v4 when there is one (it is needed only from step 1 on), else first on `s`
struct DecodeInit {
  int64_t* tok0;
  int B;
  uint64_t* keys;
  int n;
};
static int encoder_launch(const Layout& L, const MP& p, const float* feats, int B, float* a_g, float* V, float* v_g,
                          float* h0, float* c0, float* VWv, float* xg, aa_event_t* ev, int32_t flags,
                          hipStream_t s, hipStream_t aux = nullptr, bf16x8* hsp0 = nullptr,
                          const DecodeInit* init = nullptr) {
  const int C = L.C, H = L.H, E = L.E;
  const int64_t nch = (int64_t)B * C;
  hipEvent_t fork = nullptr, join = nullptr, heads_done = nullptr;
  hipStream_t sa = s;
  if (aux && aux != s) {
    AA_TRY(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
    AA_TRY(hipEventCreateWithFlags(&join, hipEventDisableTiming));
    if (hsp0) AA_TRY(hipEventCreateWithFlags(&heads_done, hipEventDisableTiming));
    AA_TRY(hipEventRecord(fork, s));
    AA_TRY(hipStreamWaitEvent(aux, fork, 0));
    sa = aux;
  }
  // the heads kernel also writes h0's bf16x3 fragments for the first step (no k_split_rows launch)
  const bool heads_split = hsp0 && !(flags & AA_DECODE_FP32_ENCODER || C % 256) && (E + 2 * H) % 80 == 0 && C % 512 == 0;
  // on one stream the heads launch (k_gemm3<5, 8, MODE_HEADS>) also does k_decode_init's stores: one
  // launch fewer on the encoder phase's chain (the ids / keys are first read by step 0 / step 1)
  const bool init_in_heads = init && sa == s && !(flags & AA_DECODE_FP32_ENCODER || C % 256) &&
                             (E + 2 * H) % 80 == 0 && C % 512 == 0;
  if (init && !init_in_heads) {
    const int nblk = init->n / 256 + 1;
    hipLaunchKernelGGL(k_decode_init, dim3(nblk < 1024 ? nblk : 1024), dim3(256), 0, sa, init->tok0, init->B,
                       (int64_t)1, init->keys, init->n);
  }
  auto heads_xg = [&](hipStream_t st) {
    const int NH = E + 2 * H;
    if (flags & AA_DECODE_FP32_ENCODER || C % 256) {
      const int MT = (B + 63) / 64, NTn = L.NHp / 64;
      AA_TLAUNCH(ev, 4, k_enc_heads, dim3(MT * NTn), dim3(256), 0, st, a_g, B, C, E, H, L.NHp, p.heads_w, p.heads_b,
                 v_g, h0, c0);
    } else if (NH % 80 == 0 && C % 512 == 0) {
      AA_TLAUNCH(ev, 4, (k_gemm3<5, 8, MODE_HEADS>), dim3(((B + 31) / 32) * (NH / 80)), dim3(512), 0, st,
                 (const float*)a_g, B, C, NH, (const bf16x8*)p.heads_w4, (const float*)p.heads_b, v_g, 0, h0, c0, E, H,
                 heads_split ? hsp0 : (bf16x8*)nullptr, init_in_heads ? init->tok0 : (int64_t*)nullptr,
                 init_in_heads ? init->B : 0, init_in_heads ? init->keys : (uint64_t*)nullptr,
                 init_in_heads ? init->n : 0);
    } else {
      AA_TLAUNCH(ev, 4, (k_gemm3<4, 4, MODE_HEADS>), dim3(((B + 31) / 32) * ((NH + 63) / 64)), dim3(256), 0, st,
                 (const float*)a_g, B, C, NH, (const bf16x8*)p.heads_w4, (const float*)p.heads_b, v_g, 0, h0, c0, E, H,
                 (bf16x8*)nullptr, (int64_t*)nullptr, 0, (uint64_t*)nullptr, 0);
    }
    if (heads_done) (void)hipEventRecord(heads_done, st);
    if (xg && gemm3_ok(flags, E) && L.N5 % 80 == 0) {
      AA_TLAUNCH(ev, 8, (k_gemm3<5, 4, MODE_PLAIN>), dim3(((B + 31) / 32) * (L.N5 / 80)), dim3(256), 0, st,
                 (const float*)v_g, B, E, L.N5, (const bf16x8*)p.wvg4, (const float*)p.bias5, xg, L.N5, (float*)nullptr,
                 (float*)nullptr, 0, 0, (bf16x8*)nullptr, (int64_t*)nullptr, 0, (uint64_t*)nullptr, 0);
    } else if (xg) {
      rec(ev, 8, st);
      gemm_bias(v_g, E, B, p.wvg, E, L.N5, E, p.bias5, xg, L.N5, st);
      rec(ev, 9, st);
    }
  };
  const bool v4 = enc_v4(L, flags);
  if (v4) {
    // k_enc_v4 computes V and a_g in one pass over the feature map; the a_g branch (heads, x_g)
    // then runs on aux beside the VWv GEMM.  (Trace: the fused avg-pool is a zero-length pair.)
    const int nwg = (B * P + E4_ROWS - 1) / E4_ROWS;
    if (H == 512)
      AA_TLAUNCH(ev, 2, (k_enc_v4<32 / ENC4_NW, ENC4_NW>), dim3(nwg), dim3(64 * ENC4_NW), 0, s, feats, B, C,
                 (const bf16x8*)p.enc_w4, (const float*)p.enc_a_b, V, a_g);
    else
      AA_TLAUNCH(ev, 2, k_enc_v4<2>, dim3(nwg), dim3(512), 0, s, feats, B, C, (const bf16x8*)p.enc_w4,
                 (const float*)p.enc_a_b, V, a_g);
    if (sa != s) {  // aux waits for a_g
      hipEvent_t agr = nullptr;
      AA_TRY(hipEventCreateWithFlags(&agr, hipEventDisableTiming));
      AA_TRY(hipEventRecord(agr, s));
      AA_TRY(hipStreamWaitEvent(sa, agr, 0));
      AA_TRY(hipEventDestroy(agr));
    }
    heads_xg(sa);
  } else {
    AA_TLAUNCH(ev, 0, k_avgpool, dim3((unsigned)((nch + 255) / 256)), dim3(256), 0, sa, feats, nch, a_g);
    heads_xg(sa);
    if (flags & AA_DECODE_FP32_ENCODER) {
      const int M = B * P, MT = (M + 63) / 64, NTn = H / 64;
      AA_TLAUNCH(ev, 2, k_enc_v, dim3(MT * NTn), dim3(256), 0, s, feats, B, C, H, (const float*)p.enc_a_w,
                 (const float*)p.enc_a_b, V);
    } else {
      const int M = B * P, MT = (M + EV_BM - 1) / EV_BM, NTn = H / EV_BN;
      AA_TLAUNCH(ev, 2, k_enc_v3, dim3(MT * NTn), dim3(256), 0, s, feats, B, C, H, (const bf16x8*)p.enc_w3,
                 (const float*)p.enc_a_b, V);
    }
  }
  if (VWv && gemm3_ok(flags, H)) {
    AA_TLAUNCH(ev, 6, (k_gemm3<4, 4, MODE_PLAIN>), dim3((B * P + 31) / 32), dim3(256), 0, s, (const float*)V, B * P, H,
               PP, (const bf16x8*)p.wv4, (const float*)nullptr, VWv, PP, (float*)nullptr, (float*)nullptr, 0, 0,
               (bf16x8*)nullptr, (int64_t*)nullptr, 0, (uint64_t*)nullptr, 0);
  } else if (VWv) {
    rec(ev, 6, s);
    gemm_bias(V, H, B * P, p.wv, H, PP, H, nullptr, VWv, PP, s);
    rec(ev, 7, s);
  }
  if (hsp0 && !heads_split) {
    if (heads_done) AA_TRY(hipStreamWaitEvent(s, heads_done, 0));
    hipLaunchKernelGGL(k_split_rows, dim3((unsigned)(((int64_t)B * (H / 8) + 255) / 256)), dim3(256), 0, s, h0, B, H,
                       hsp0);
  }
  if (heads_done) AA_TRY(hipEventDestroy(heads_done));
  if (join) {
    AA_TRY(hipEventRecord(join, sa));
    AA_TRY(hipStreamWaitEvent(s, join, 0));
    AA_TRY(hipEventDestroy(join));
    AA_TRY(hipEventDestroy(fork));
  }
  return launch_status();
}

int aa_encoder_tail(const aa_model* m, const float* feats, int32_t B, float* a_g, float* V, float* v_g, float* h0,
                    float* c0, float* VWv, int32_t flags, aa_stream_t stream) {
  Layout L;
  int rc = check_model(m, &L);
  if (rc) return rc;
  if (B < 0) return AA_ERR_SHAPE;
  if (B == 0) return AA_OK;
  if (!feats || !a_g || !V || !v_g || !h0 || !c0) return AA_ERR_NULL;
  if (!al16(feats) || !al16(a_g) || !al16(V) || !al16(VWv) || !al16(v_g)) return AA_ERR_ALIGN;
  return encoder_launch(L, resolve(m, L), feats, B, a_g, V, v_g, h0, c0, VWv, nullptr, nullptr, flags,
                        (hipStream_t)stream);
}

// ---- workspace carving ----------------------------------------------------------------------
struct Carver {
  char* base;
  size_t off = 0;
  template <class T>
  T* take(size_t n) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off = (off + n * sizeof(T) + 255) & ~size_t(255);
    return p;
  }
};

struct StepWS {
  float *xg, *s, *u, *vwv, *part;
  bf16x8* hsp;
  uint64_t* keys;
  int64_t* tok0;
};
// split-h fragment buffer: rows padded to 32, 3 planes of bf16
// (rows padded to whole 64-row tiles: k_lstm reads its tile's two row blocks)
static size_t hsp_frags(const Layout& L, int B) { return (size_t)((B + 63) / 64) * 2 * (L.H / 16) * 3 * 64; }
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
  float *a_g, *V, *vwv, *vg, *xg, *h[2], *c[2], *s, *u, *unorm, *part;
  uint16_t* ub;
  bf16x8* hsp[2];
  float4* summ;
  uint64_t* keys;
  int64_t* tok0;
};
static DecodeWS carve_decode(char* base, const Layout& L, int B, int T, size_t* bytes) {
  Carver c{base};
  DecodeWS w;
  w.a_g = c.take<float>((size_t)B * L.C);
  w.V = c.take<float>((size_t)B * P * L.H);
  w.vwv = c.take<float>((size_t)B * P * PP);
  w.vg = c.take<float>((size_t)B * L.E);
  w.xg = c.take<float>((size_t)B * L.N5);
  for (int i = 0; i < 2; ++i) {
    w.h[i] = c.take<float>((size_t)B * L.H);
    w.c[i] = c.take<float>((size_t)B * L.H);
  }
  w.s = c.take<float>((size_t)B * L.H);
  w.u = c.take<float>((size_t)B * L.H);
  w.unorm = c.take<float>((size_t)2 * B);  // ||u|| then ||u - bf16(u)|| per row
  w.part = c.take<float>((size_t)B * (L.H / 16) * PART);
  w.ub = c.take<uint16_t>((size_t)((B + 127) / 128) * 128 * L.H);  // fragment order, 128-row tiles
  for (int i = 0; i < 2; ++i) w.hsp[i] = c.take<bf16x8>(hsp_frags(L, B));
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


// LSTM step (GEMM + cell in one launch), shared by the step API, the greedy loop and beam search.
// par != nullptr: beam search (rows continue rows par[] of the previous step)
// ra != nullptr: greedy step t >= 1 with step t-1's rescoring in the same launch (k_lstm<.., RS>); the
// tokens come from the published keys, `tok` is not read
static void lstm_launch(const Layout& L, const MP& p, int B, const int64_t* tok, int tok_ld, const float* xg,
                        const bf16x8* hsp_in, const float* c_in, float* h_out, bf16x8* hsp_out, float* c_out,
                        float* s_buf, float* part, hipStream_t s, const int* par = nullptr,
                        const RsArgs* ra = nullptr, aa_event_t* ev = nullptr, int ei = 0, bool base = false) {
  const int H = L.H, MT = (B + 63) / 64;
  const RsArgs none{};
  const int64_t* tnull = nullptr;
  if (base) {  // the baseline model's no-sentinel step (H = 512, greedy: baseline_ok()); s_buf is not written
    if (ra)
      AA_TLAUNCH(ev, ei, (k_lstm<512, false, true, false>), dim3(ra->NR + MT * (512 / 16)), dim3(512), 0, s, B, L.V,
                 tnull, 0, p.table, xg, hsp_in, c_in, par, p.whh3, p.wgs, h_out, hsp_out, c_out, s_buf, part,
                 *ra);
    else
      AA_TLAUNCH(ev, ei, (k_lstm<512, false, false, false>), dim3(MT * (512 / 16)), dim3(512), 0, s, B, L.V, tok,
                 tok_ld, p.table, xg, hsp_in, c_in, par, p.whh3, p.wgs, h_out, hsp_out, c_out, s_buf, part, none);
    return;
  }
  aa_for_hidden(H, [&](auto h) {
    constexpr int H_ = h.value;
    if (par)
      AA_TLAUNCH(ev, ei, (k_lstm<H_, true>), dim3(MT * (H_ / 16)), dim3(512), 0, s, B, L.V, tok, tok_ld,
                 p.table, xg, hsp_in, c_in, par, p.whh3, p.wgs, h_out, hsp_out, c_out, s_buf, part, none);
    else if (ra)
      AA_TLAUNCH(ev, ei, (k_lstm<H_, false, true>), dim3(ra->NR + MT * (H_ / 16)), dim3(512), 0, s, B, L.V,
                 tnull, 0, p.table, xg, hsp_in, c_in, par, p.whh3, p.wgs, h_out, hsp_out, c_out, s_buf, part,
                 *ra);
    else
      AA_TLAUNCH(ev, ei, (k_lstm<H_, false>), dim3(MT * (H_ / 16)), dim3(512), 0, s, B, L.V, tok, tok_ld,
                 p.table, xg, hsp_in, c_in, par, p.whh3, p.wgs, h_out, hsp_out, c_out, s_buf, part, none);
  });
}

// Attention for one step (kdiv rows per image: beam search; k_atten5b runs an image's rows together)
static void atten_launch(const Layout& L, const MP& p, int B, const float* V, const float* vwv, const float* h_out,
                         float* s_buf, float* part, float* u, uint16_t* ub, float* unorm, float* alpha,
                         int64_t alpha_ld, float* beta, int64_t beta_ld, hipStream_t s, int kdiv = 1,
                         bf16x8* ub3 = nullptr, aa_event_t* ev = nullptr, int ei = 0, bool base = false) {
  const int H = L.H;
  const float* sb = s_buf;
  const float* pt = part;
  if (base) {  // the baseline model's row (H = 512, one row per image): s_buf and beta are not touched
    AA_TLAUNCH(ev, ei, (k_atten5<512, false>), dim3(B), dim3(512), 0, s, B, kdiv, h_out, sb, pt, V, vwv, p.wh, alpha,
               alpha_ld, (float*)nullptr, beta_ld, u, ub, unorm, ub3);
    return;
  }
#define AA_ATTEN(HPT_)                                                                                     \
  AA_TLAUNCH(ev, ei, k_atten<HPT_>, dim3(B), dim3(256), 0, s, B, H / 16, kdiv, h_out, sb, pt, V, vwv, p.wh, alpha, \
             alpha_ld, beta, beta_ld, u, ub, unorm, ub3)
#define AA_ATTEN5(H_)                                                                                      \
  AA_TLAUNCH(ev, ei, k_atten5<H_>, dim3(B), dim3(512), 0, s, B, kdiv, h_out, sb, pt, V, vwv, p.wh, alpha, \
             alpha_ld, beta, beta_ld, u, ub, unorm, ub3)
#define AA_ATTEN5B(KB_)                                                                                    \
  AA_TLAUNCH(ev, ei, (k_atten5b<512, KB_>), dim3(B / KB_), dim3(512), 0, s, h_out, sb, pt, V, vwv, p.wh, alpha, \
             alpha_ld, beta, beta_ld, u, ub, unorm, ub3)
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
}

// LSTM + attention for one step (fused LSTM kernel)
static void lstm_atten_launch(const Layout& L, const MP& p, int B, const int64_t* tok, int tok_ld,
                              const float* V, const float* vwv, const float* xg, const bf16x8* hsp_in,
                              const float* c_in, float* h_out, bf16x8* hsp_out, float* c_out, float* s_buf, float* part, float* u, uint16_t* ub,
                              float* unorm, float* alpha, int64_t alpha_ld, float* beta, int64_t beta_ld,
                              const aa_trace* tr, int t, hipStream_t s, const int* par = nullptr, int kdiv = 1,
                              bf16x8* ub3 = nullptr, const RsArgs* ra = nullptr, bool base = false) {
  lstm_launch(L, p, B, tok, tok_ld, xg, hsp_in, c_in, h_out, hsp_out, c_out, s_buf, part, s, par, ra,
              tr ? tr->lstm_events : nullptr, 2 * t, base);
  atten_launch(L, p, B, V, vwv, h_out, s_buf, part, u, ub, unorm, alpha, alpha_ld, beta, beta_ld, s, kdiv, ub3,
               tr ? tr->atten_events : nullptr, 2 * t, base);
}

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
  hipLaunchKernelGGL(k_split_rows, dim3((unsigned)(((int64_t)B * (L.H / 8) + 255) / 256)), dim3(256), 0, s, h_in, B,
                     L.H, w.hsp);
  const int64_t* tok = tokens_in;
  if (!tok) {
    hipLaunchKernelGGL(k_fill_tok, dim3((B + 255) / 256), dim3(256), 0, s, w.tok0, B, (int64_t)1);  // <start>
    tok = w.tok0;
  }
  lstm_atten_launch(L, p, B, tok, 1, V, VWv, w.xg, w.hsp, c_in, h_out, nullptr, c_out, w.s, w.part, w.u,
                    nullptr, nullptr, alpha, P, beta, 1, nullptr, 0, s, nullptr, 1, nullptr, nullptr, base);
  hipLaunchKernelGGL(k_vocab, dim3(((B + 63) / 64) * (L.Vp / 64)), dim3(256), 0, s, B, L.H, L.V, L.Vp, L.V, w.u, p.mlp_w,
                     p.mlp_b, scores, w.keys);
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
  const int H = L.H, MT = (B + 63) / 64;
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
    RsArgs ra{rup((B + 1) / 2, 8), L.Vp, T, t - 1, (flags & AA_DECODE_RS_SELF) ? 0 : RS_WAIT_TICKS, w.u, w.summ,
              p.mlp_w, p.mlp_b, kt - B, ids};
    lstm_launch(L, p, B, tok, tok_ld, w.xg, w.hsp[cur], w.c[cur], w.h[nxt], w.hsp[nxt], w.c[nxt], w.s, w.part, s,
                nullptr, fused && t > 0 ? &ra : nullptr, trace ? trace->lstm_events : nullptr, 2 * t, base);
    atten_launch(L, p, B, w.V, w.vwv, w.h[nxt], w.s, w.part, w.u, exact ? nullptr : w.ub, exact ? nullptr : w.unorm,
                 alt, (int64_t)T * P, blt, T, s, 1, nullptr, trace ? trace->atten_events : nullptr, 2 * t, base);
    aa_event_t* sev = trace ? trace->screen_events : nullptr;
    aa_event_t* rev = trace ? trace->rescore_events : nullptr;
    if (exact) {
      AA_TLAUNCH(sev, 2 * t, k_vocab, dim3(MT * (L.Vp / 64)), dim3(256), 0, s, B, L.H, L.V, L.Vp, L.V,
                 (const float*)w.u, p.mlp_w, p.mlp_b, (float*)nullptr, kt);
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
      AA_TLAUNCH(rev, 2 * t, k_vrescore<h.value>, dim3(B), dim3(RS_NT), 0, s, B, L.V, L.Vp, (const float*)w.u,
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
  rc = encoder_launch(L, p, feats, B, w.a_g, w.V, w.vg, w.h[0], w.c[0], w.vwv, w.xg,
                      trace ? trace->encoder_events : nullptr, flags, s, aux, w.hsp[0], clear ? &init : nullptr);
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
  hipLaunchKernelGGL(k_vocab, dim3(((B + 63) / 64) * (L.Vp / 64)), dim3(256), 0, (hipStream_t)stream, B, L.H, L.V, L.Vp, L.V,
                     u, p.mlp_w, p.mlp_b, scores, nullptr);
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

// AA_DECODE_ONLY: A/B variant builds of the greedy path only (tools/build_variant.sh; the training
// and beam entry points are then absent and adaptive_amd._lib binds only what the library exports)
#ifndef AA_DECODE_ONLY
// teacher-forced training step (same translation unit: reuses the encoder kernels)
#include "aa_train.hip"
// beam-search decode (reuses k_lstm / k_atten / k_vocab and the encoder)
#include "aa_beam.hip"
// seeded temperature-sampling decode (the beam's step loop with one row per image)
#include "aa_sample.hip"
#endif
