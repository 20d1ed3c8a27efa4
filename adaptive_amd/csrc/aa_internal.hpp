// aa_internal.hpp — what the library's translation units share beyond aa_common.hpp: the packed
// weight layout (Layout, MP, make_layout, resolve, check_model), workspace carving (Carver and the two
// pieces every decode mode's workspace starts with), the timed-launch macro, the small device helpers
// several units use, the named arguments of one decode step (StepIO), and the declarations of the host
// functions one object calls in another.  Each kernel is compiled into exactly one object: a unit that
// needs a kernel defined elsewhere calls that unit's launch function.  The cross-object functions are
// in namespace aa and keep the build's hidden visibility (the library exports adaptive_amd.h only).
//   aa_encoder.hip    pack kernels, encoder tail (k_enc_v4 / k_gemm3 / ...), k_gemm_bias
//   aa_lstm.hip       k_lstm (aa_lstm.hpp), one object per hidden size
//   aa_kernels.hip    attention, vocab screen / rescoring, the step and greedy C ABI
//   aa_beam.hip       beam search and the exact fp32 vocab GEMMs (k_vocab, k_vexact)
//   aa_tgemm.hip      the training step's GEMM engine (aa_tgemm.hpp)
//   aa_sample.hip, aa_train.hip, aa_optim.hip
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

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
  size_t enc_a_w, enc_a_b, enc_w3, whh3, heads_w, heads_b, wv, wg, ws, wh, whh, wemb, wvg, bias5, table, mlp_w, mlp_b, mlp_wb, mlp_wn, mlp_gs, wgs, mlp_w3, enc_w4, heads_w4, wvg4, wv4, enc_w4h, enc_w4h_sc;
  size_t total_floats;
};

static inline size_t al64(size_t x) { return (x + 63) & ~size_t(63); }
static inline int rup(int x, int m) { return (x + m - 1) / m * m; }

inline Layout make_layout(const aa_dims& d) {
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
  L.enc_w4h = take((size_t)2 * L.H * L.C / 2);     // W_a 2^e as 2 fp16 planes (hi, lo), 16x16x32 fragments [H/16][C/32][2][64][8]
  L.enc_w4h_sc = take(2);                          // its un-scale 2^-(e + ENC_F16_A_EXP) and the exponent e (as a float)
  L.total_floats = o;
  return L;
}

struct MP {  // resolved device pointers of the packed weights
  const bf16x8 *enc_w3, *whh3, *mlp_w3, *enc_w4, *heads_w4, *wvg4, *wv4;
  const f16x8* enc_w4h;
  const float* enc_w4h_sc;
  const float *enc_a_w, *enc_a_b, *heads_w, *heads_b, *wv, *wg, *ws, *wh, *whh, *wemb, *wvg, *bias5, *table, *mlp_w,
      *mlp_b, *mlp_wn, *wgs;
  const float4* mlp_gs;
  const uint16_t* mlp_wb;
};

inline MP resolve(const aa_model* m, const Layout& L) {
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
  p.enc_w4h = reinterpret_cast<const f16x8*>(b + L.enc_w4h);
  p.enc_w4h_sc = b + L.enc_w4h_sc;
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

// exact 3-way bf16 split x = h + m + l + r, |r| <= 2^-24 |x| (see k_enc_v3)
__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)x;
  const float r1 = x - (float)h;
  m = (__bf16)r1;
  const float r2 = r1 - (float)m;
  l = (__bf16)r2;
}

// The encoder V GEMM's two-way fp16 split (k_enc_v4's fast path; the error argument is at the kernel).
// Features are scaled by 2^ENC_F16_A_EXP before the split; a feature that is not below ENC_F16_A_MAX
// in magnitude (or not finite) sends its workgroup through the bf16x3 body.  W_a is scaled at pack
// time by the power of two 2^e that puts max|W_a| 2^e in [2^ENC_F16_W_TOP, 2^(ENC_F16_W_TOP + 1)), e
// clamped to +-ENC_F16_W_ECLAMP (e = 0 for an all-zero or non-finite tensor).
// (tests/test_split_f16_emulation.py reads these four lines.)
constexpr int ENC_F16_A_EXP = 6;
constexpr float ENC_F16_A_MAX = 512.0f;
constexpr int ENC_F16_W_TOP = 13;
constexpr int ENC_F16_W_ECLAMP = 64;
// exact 2-way fp16 split of an already scaled x = h + l + r: the difference is exact in fp32 and, while
// l is a normal fp16 number, |r| <= 2^-22 |x| (2^-25 absolute once l is subnormal)
__device__ __forceinline__ void split2h(float x, _Float16& h, _Float16& l) {
  h = (_Float16)x;
  l = (_Float16)(x - (float)h);
}

// one k16 chunk of a bf16x3 GEMM: the six products with i + j <= 2, smallest first (see k_enc_v3)
__device__ __forceinline__ void x3_step(floatx16& acc, const bf16x8 (&a)[3], const bf16x8 (&w)[3]) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], w[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], w[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], w[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[0], acc, 0, 0, 0);
}

constexpr int PART = 128;  // partial-projection row pitch (W_g h outputs at 0..48, W_s s at 64..112)
// Column of projection output j (0..97: W_g then W_s) in a partial row.  Each half
// starts on a 256-B boundary, so every store instruction of the tile's projection phase (a 32 x 32
// accumulator block: two rows x 32 columns) writes two whole 128-B lines (the write-through stores of
// partial lines otherwise cost the memory side a read-modify-write each).
__device__ __forceinline__ int part_col(int j) { return j < P ? j : 64 + (j - P); }

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

// splitmix64 finaliser (the synthetic-data and sampling counters)
__device__ __forceinline__ uint64_t splitmix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

constexpr int BEAM_VPT = 64;  // logits held per thread in the beam / sampling selection: V <= 256 * 64

static inline int launch_status() { return aa_launch_status(); }
static inline bool al16(const void* p) { return aa_al16(p); }

inline int check_model(const aa_model* m, Layout* L) {
  if (!m || !m->packed) return AA_ERR_NULL;
  int rc = aa_check_dims(&m->dims);
  if (rc) return rc;
  *L = make_layout(m->dims);
  if (m->packed_bytes < L->total_floats * sizeof(float)) return AA_ERR_BUFFER;
  if (((uintptr_t)m->packed & 255u) != 0) return AA_ERR_ALIGN;
  return AA_OK;
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
// split-h fragment buffer: rows padded to 32, 3 planes of bf16
// (rows padded to whole 64-row tiles: k_lstm reads its tile's two row blocks)
inline size_t hsp_frags(const Layout& L, int B) { return (size_t)((B + 63) / 64) * 2 * (L.H / 16) * 3 * 64; }

// The two pieces every decode workspace is made of (a Carver rounds each take to 256 B, so a
// workspace's size does not depend on the order of its takes): the encoder tail's outputs for B images
struct EncWS {
  float *a_g, *V, *vwv, *vg;
};
inline EncWS carve_enc(Carver& c, const Layout& L, size_t B) {
  EncWS w;
  w.a_g = c.take<float>(B * L.C);
  w.V = c.take<float>(B * P * L.H);
  w.vwv = c.take<float>(B * P * PP);
  w.vg = c.take<float>(B * L.E);
  return w;
}
// ... and the recurrent state of R rows (R = B, beam search: B K): x_g, double-buffered h / c / split h,
// the sentinel s, u = c_hat + h, the attention-projection partials
struct RowWS {
  float *xg, *h[2], *c[2], *s, *u, *part;
  bf16x8* hsp[2];
};
inline RowWS carve_rows(Carver& c, const Layout& L, size_t R) {
  RowWS w;
  w.xg = c.take<float>(R * L.N5);
  for (int i = 0; i < 2; ++i) {
    w.h[i] = c.take<float>(R * L.H);
    w.c[i] = c.take<float>(R * L.H);
    w.hsp[i] = c.take<bf16x8>(hsp_frags(L, (int)R));
  }
  w.s = c.take<float>(R * L.H);
  w.u = c.take<float>(R * L.H);
  w.part = c.take<float>(R * (L.H / 16) * PART);
  return w;
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

// ---- one decode step: k_lstm then the attention kernel ------------------------------------------
// The operands of a step over B rows, filled by designated initialisers at the call sites.
struct RsArgs;  // aa_lstm.hpp
struct StepIO {
  int B;
  const int64_t* tok;  // token of row r at tok[r * tok_ld]; nullptr: <start> for every row
  int tok_ld = 1;
  const float *V, *vwv, *xg;  // encoder outputs (of image r / kdiv) and the rows' x_g
  const bf16x8* hsp_in;       // state in: split h and c (of row par[r] when par is set)
  const float* c_in;
  float* h_out;               // state out
  bf16x8* hsp_out = nullptr;  // (nullptr: the next step's split h is not written)
  float* c_out;
  float *s, *part, *u;        // sentinel, projection partials, u = c_hat + h
  uint16_t* ub = nullptr;     // bf16(u) in fragment order and (||u||, ||u - bf16(u)||): the vocab screen's
  float* unorm = nullptr;
  bf16x8* ub3 = nullptr;      // u as bf16x3 fragments (beam search's bf16x3 vocab GEMM)
  float* alpha = nullptr;     // attention weights / sentinel gate of row r at r * ld
  int64_t alpha_ld = P;
  float* beta = nullptr;
  int64_t beta_ld = 1;
  const int* par = nullptr;   // beam search: rows continue rows par[] of the previous step
  int kdiv = 1;               // rows per image (beam search: k_atten5b runs an image's rows together)
  const RsArgs* ra = nullptr; // greedy step t >= 1 with step t-1's rescoring in the LSTM launch
                              // (k_lstm<.., RS>); the tokens come from the published keys, tok is not read
  bool base = false;          // the baseline model's no-sentinel kernels (H = 512): s and beta are not touched
  aa_event_t* lstm_ev = nullptr;   // trace: event pairs (ei, ei + 1) handed to the two launches
  aa_event_t* atten_ev = nullptr;
  int ei = 0;
};
// aa_lstm.hip, one object per hidden size: the k_lstm form the step asks for (plain, beam gather,
// fused rescoring; H = 512 also the two no-sentinel forms)
template <int H>
void lstm_launch_h(const Layout& L, const MP& p, const StepIO& io, hipStream_t s);
// aa_kernels.hip
void lstm_launch(const Layout& L, const MP& p, const StepIO& io, hipStream_t s);
void atten_launch(const Layout& L, const MP& p, const StepIO& io, hipStream_t s);
void lstm_atten_launch(const Layout& L, const MP& p, const StepIO& io, hipStream_t s);
void split_rows_launch(const float* h, int B, int H, bf16x8* out, hipStream_t s);      // k_split_rows
void fill_tok_launch(int64_t* tok, int B, int64_t v, hipStream_t s);                    // k_fill_tok
// aa_beam.hip: k_expand_rows, dst[r][:] = src[r / K][:] for the B K rows (n floats per row, a multiple of 4)
void expand_rows_launch(const float* src, int B, int K, int n, float* dst, hipStream_t s);
// aa_beam.hip: the exact fp32 vocab GEMMs
// k_vocab: exact fp32 logits of R rows (scores, pitch ld; may be nullptr) and argmax keys (may be nullptr)
void vocab_launch(const Layout& L, const MP& p, int R, const float* u, float* scores, int ld, uint64_t* keys,
                  hipStream_t s, aa_event_t* ev = nullptr, int ei = 0);
// k_vexact: exact fp32 logits (pitch Vp) and their granule summaries
void vexact_launch(const Layout& L, const MP& p, int R, const float* u, float* logits, float2* gsum, hipStream_t s,
                   aa_event_t* ev = nullptr, int ei = 0);
// aa_encoder.hip
void gemm_bias(const float* A, int lda, int M, const float* W, int ldw, int N, int K, const float* bias, float* C,
               int64_t ldc, hipStream_t s);                                             // k_gemm_bias
void avgpool_launch(const float* feats, int64_t nch, float* a_g, hipStream_t s);        // k_avgpool
void enc_v_launch(const float* feats, int B, int C, int H, const float* w, const float* b, float* V,
                  hipStream_t s);                                                       // k_enc_v
struct DecodeInit {  // the greedy decode's k_decode_init: <start> tokens and the [T][B] key clear
  int64_t* tok0;
  int B;
  uint64_t* keys;
  int n;
};
int encoder_launch(const Layout& L, const MP& p, const float* feats, int B, float* a_g, float* V, float* v_g,
                   float* h0, float* c0, float* VWv, float* xg, aa_event_t* ev, int32_t flags, hipStream_t s,
                   hipStream_t aux = nullptr, bf16x8* hsp0 = nullptr, const DecodeInit* init = nullptr);

}  // namespace aa
