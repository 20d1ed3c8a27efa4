// aa_lstm.hpp — the decode step's LSTM kernel k_lstm and everything it is built from: the LDS-staged
// bf16x3 GEMM h W_hh^T (lstm_gemm_lds, x3_step2, vm_wait), the cell epilogue (lstm_cell_tail: c', h', the
// sentinel s, the next step's split h, the per-tile attention projections), and -- for the greedy
// path's fused launch k_lstm<.., RS> -- the exact rescoring of one row (rescore_row, exact_logit8,
// RsScratch, RsArgs), which k_vrescore (aa_kernels.hip) shares.  All arithmetic that defines an output
// is fp32.  aa_lstm.hip instantiates the kernel, one object per hidden size: 80 % of the library's
// device code is these instantiations, so no other unit launches k_lstm itself.
#pragma once
#include "aa_internal.hpp"

namespace aa {

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

// The GEMM h_{t-1} W_hh^T runs on bf16 MFMA with 3-way split operands (see k_enc_v3): h arrives
// already split (hsp_in, written by the previous step's epilogue or k_split_rows) and W_hh is
// pre-split at pack time, both in MFMA-fragment order, so every operand is one coalesced 16-B
// load per lane straight into VGPRs -- no LDS staging.  Fragment index of (row block rb, k16
// chunk kc, plane q): ((rb * KC + kc) * 3 + q) * 64 + lane.
// 512 threads = 8 waves; wave w computes the whole 64x64 tile (2 x 2 blocks of 32x32) over K
// chunks [w KC/8, (w+1) KC/8), so no fragment is loaded twice in the workgroup; the eight partial
// tiles meet in LDS and are summed in a fixed tree ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)).

// Two-accumulator form (k_lstm's GEMM, lstm_gemm_lds): the three small products (i + j = 2)
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

// Cell epilogue of k_lstm (GEMM + cell in one launch): thread -> row rr (0..63) of the tile, units
// u0, u0 + 1 of tile nt.
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

}  // namespace aa
