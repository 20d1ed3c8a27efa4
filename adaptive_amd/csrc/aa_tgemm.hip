// aa_tgemm.hip — the generic GEMM engine of the training step (aa_tgemm.hpp): k_tgemm on fp32 operands
// in any of the layouts the backward pass needs (bounds-checked, fixed accumulation order; bf16 MFMA
// with AA_TRAIN_BF16), k_bgemm on pre-packed bf16 operands, the deterministic split-K reduce, the
// bf16 operand packers and the column sums.  It knows nothing of the model: aa_train.hip is its caller.
#include <stdio.h>
#include <stdlib.h>

#include "aa_tgemm.hpp"

namespace aa {

// k_tgemm: 64x64 tiles, 256 threads (2 x 2 waves of 32x32), K steps of TStep::KS through double-buffered
// LDS (fp32 MFMA: lanes 0-31 take k = s, lanes 32-63 k = KS/2 + s of each step).
// K step of the training GEMM: 64 with bf16 operands (two 32-wide halves per thread, so a
// latency-bound GEMM -- the per-step recurrent ones, K = 128 per split -- pays half the global round
// trips), 32 with fp32 operands (a 64-deep fp32 tile pair would need 70 KB of LDS and halve the
// occupancy of the large GEMMs: measured slower).  Tiles [64 rows][pitch]: fp32 pitch KS + 4 floats,
// bf16 KS + 8 bf16 (conflict-free 16-B fragment reads either way).
template <bool BF>
struct TStep {
  static constexpr int KS = BF ? 64 : 32, HH = KS / 32, LDK = KS + 4, LDB = KS + 8;
  static constexpr int TILE_F = BF ? 64 * LDB / 2 : 64 * LDK;  // one operand tile, in floats
};

// BF: operands rounded to bf16 (RNE) as they are staged in LDS, products on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation (BASELINE config 5: bf16 compute, fp32 master
// weights); same tiles, loads and epilogue as the fp32 engine.
template <bool BF>
__global__ __launch_bounds__(256) void k_tgemm(TG g) {
  constexpr int TBK = TStep<BF>::KS, HH = TStep<BF>::HH, TLDK = TStep<BF>::LDK, TLDB = TStep<BF>::LDB;
  __shared__ __attribute__((aligned(16))) float lds[2][2][TStep<BF>::TILE_F];
  const int tilesN = (g.N + 63) / 64;
  const int split = blockIdx.x % g.splits, tile = blockIdx.x / g.splits;
  const int mt = tile / tilesN, nt = tile % tilesN;
  const int kbeg = split * g.kper, kend = g.splits > 1 ? (kbeg + g.kper < g.K ? kbeg + g.kper : g.K) : g.K;
  const int m0 = mt * 64, n0 = nt * 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wmv = wave >> 1, wnv = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  float ra[HH][8], rw[HH][8];  // [32-wide k half][8 consecutive elements]
  // operands are read 8 consecutive elements per thread along their contiguous dimension, as two
  // 16-B loads when the 8 are in bounds and aligned, else element by element with zero fill
  const bool a4 = ((g.lda & 3) == 0) && ((((uintptr_t)g.A) & 15) == 0);
  const bool w4 = ((g.ldw & 3) == 0) && ((((uintptr_t)g.W) & 15) == 0) && g.wm != W_NCHW;
  auto load8 = [&](float (&r)[8], const float* base) {
    const float4 x = *reinterpret_cast<const float4*>(base), y = *reinterpret_cast<const float4*>(base + 4);
    r[0] = x.x; r[1] = x.y; r[2] = x.z; r[3] = x.w; r[4] = y.x; r[5] = y.y; r[6] = y.z; r[7] = y.w;
  };
  auto gload = [&](int k0, float (&ra)[HH][8], float (&rw)[HH][8]) {
#pragma unroll
    for (int hh = 0; hh < HH; ++hh) {
      const int kh = k0 + 32 * hh;
      if (!g.at) {  // 4 threads per row, 8 consecutive k each
        const int r = t >> 2, kq = (t & 3) * 8, m = m0 + r;
        const int64_t base = (int64_t)(m < g.M ? (g.arow ? g.arow[m] : m) : 0) * g.lda;
        if (a4 && m < g.M && kh + kq + 8 <= kend) load8(ra[hh], g.A + base + kh + kq);
        else
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int k = kh + kq + i;
            ra[hh][i] = (m < g.M && k < kend) ? g.A[base + k] : 0.f;
          }
      } else {  // 8 threads per k, 8 consecutive m each
        const int k = kh + (t >> 3), mq = (t & 7) * 8;
        if (a4 && k < kend && m0 + mq + 8 <= g.M) load8(ra[hh], g.A + (int64_t)k * g.lda + m0 + mq);
        else
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int m = m0 + mq + i;
            ra[hh][i] = (m < g.M && k < kend) ? g.A[(int64_t)k * g.lda + m] : 0.f;
          }
      }
      if (g.wm == W_COLS) {
        const int k = kh + (t >> 3), nq = (t & 7) * 8;
        if (w4 && k < kend && n0 + nq + 8 <= g.N) load8(rw[hh], g.W + (int64_t)k * g.ldw + n0 + nq);
        else
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int n = n0 + nq + i;
            rw[hh][i] = (n < g.N && k < kend) ? g.W[(int64_t)k * g.ldw + n] : 0.f;
          }
      } else {
        const int r = t >> 2, kq = (t & 3) * 8, n = n0 + r;
        if (w4 && n < g.N && kh + kq + 8 <= kend) load8(rw[hh], g.W + (int64_t)n * g.ldw + kh + kq);
        else
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int k = kh + kq + i;
            float v = 0.f;
            if (n < g.N && k < kend) {
              if (g.wm == W_ROWS) v = g.W[(int64_t)n * g.ldw + k];
              else v = g.W[((int64_t)(k / P) * g.ldw + n) * P + (k % P)];
            }
            rw[hh][i] = v;
          }
      }
    }
  };
  auto lstore = [&](int buf, float (&ra)[HH][8], float (&rw)[HH][8]) {
#pragma unroll
    for (int hh = 0; hh < HH; ++hh) {
      const int ko = 32 * hh;
      if constexpr (BF) {
        __bf16* As = reinterpret_cast<__bf16*>(lds[buf][0]);
        __bf16* Ws = reinterpret_cast<__bf16*>(lds[buf][1]);
        if (!g.at) {
          const int r = t >> 2, kq = (t & 3) * 8;
          bf16x8 v;
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = (__bf16)ra[hh][i];
          *reinterpret_cast<bf16x8*>(As + r * TLDB + ko + kq) = v;
        } else {
          const int k = t >> 3, mq = (t & 7) * 8;
#pragma unroll
          for (int i = 0; i < 8; ++i) As[(mq + i) * TLDB + ko + k] = (__bf16)ra[hh][i];
        }
        if (g.wm == W_COLS) {
          const int k = t >> 3, nq = (t & 7) * 8;
#pragma unroll
          for (int i = 0; i < 8; ++i) Ws[(nq + i) * TLDB + ko + k] = (__bf16)rw[hh][i];
        } else {
          const int r = t >> 2, kq = (t & 3) * 8;
          bf16x8 v;
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = (__bf16)rw[hh][i];
          *reinterpret_cast<bf16x8*>(Ws + r * TLDB + ko + kq) = v;
        }
      } else {
        float* As = lds[buf][0];
        float* Ws = lds[buf][1];
        if (!g.at) {
          const int r = t >> 2, kq = (t & 3) * 8;
#pragma unroll
          for (int i = 0; i < 8; ++i) As[r * TLDK + ko + kq + i] = ra[hh][i];
        } else {
          const int k = t >> 3, mq = (t & 7) * 8;
#pragma unroll
          for (int i = 0; i < 8; ++i) As[(mq + i) * TLDK + ko + k] = ra[hh][i];
        }
        if (g.wm == W_COLS) {
          const int k = t >> 3, nq = (t & 7) * 8;
#pragma unroll
          for (int i = 0; i < 8; ++i) Ws[(nq + i) * TLDK + ko + k] = rw[hh][i];
        } else {
          const int r = t >> 2, kq = (t & 3) * 8;
#pragma unroll
          for (int i = 0; i < 8; ++i) Ws[r * TLDK + ko + kq + i] = rw[hh][i];
        }
      }
    }
  };
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int nk = (kend - kbeg + TBK - 1) / TBK;
  auto compute = [&](int buf) {
    if constexpr (BF) {
      const __bf16* As = reinterpret_cast<const __bf16*>(lds[buf][0]);
      const __bf16* Ws = reinterpret_cast<const __bf16*>(lds[buf][1]);
#pragma unroll
      for (int kb = 0; kb < TBK / 16; ++kb) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(As + (wmv * 32 + li) * TLDB + 16 * kb + 8 * lh);
        const bf16x8 w = *reinterpret_cast<const bf16x8*>(Ws + (wnv * 32 + li) * TLDB + 16 * kb + 8 * lh);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, w, acc, 0, 0, 0);
      }
    } else {
      const float* As = lds[buf][0];
      const float* Ws = lds[buf][1];
#pragma unroll
      for (int s8 = 0; s8 < TBK / 8; ++s8) {  // lane half lh: k = (TBK / 2) lh + 4 s8 + j
        const float4 a = *reinterpret_cast<const float4*>(As + (wmv * 32 + li) * TLDK + (TBK / 2) * lh + 4 * s8);
        const float4 w = *reinterpret_cast<const float4*>(Ws + (wnv * 32 + li) * TLDK + (TBK / 2) * lh + 4 * s8);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f4c(a, j), f4c(w, j), acc, 0, 0, 0);
      }
    }
  };
  // (loading two K steps ahead from two register sets -- 145 VGPRs, three waves per SIMD instead of
  // four -- was bit-identical and 1-2 % slower over the training step: profiles/r06z6_train_tgemm_pf2_ab.txt)
  gload(kbeg, ra, rw);
  lstore(0, ra, rw);
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    if (ks + 1 < nk) gload(kbeg + (ks + 1) * TBK, ra, rw);
    compute(ks & 1);
    if (ks + 1 < nk) lstore((ks & 1) ^ 1, ra, rw);
    __syncthreads();
  }
  const int col = n0 + wnv * 32 + li;
  if (g.splits > 1) {
    float* pt = g.part + (int64_t)split * g.M * g.N;
    if (col < g.N)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wmv * 32 + acc_row(r, lane);
        if (m < g.M) pt[(int64_t)m * g.N + col] = acc[r];
      }
    return;
  }
  if (col >= g.N) return;
  const float bv = (g.bias ? g.bias[col] : 0.f) + (g.bias2 ? g.bias2[col] : 0.f);
  // accumulate: the 16 old values are loaded together before any store (a load after a store to C
  // may alias it, so loads interleaved with the stores each waited a full round trip: 16 per thread)
  float* dst[16];
  float old[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wmv * 32 + acc_row(r, lane);
    const int mc = m < g.M ? m : g.M - 1;
    dst[r] = g.C + (int64_t)(g.crow ? g.crow[mc] : mc) * g.ldc + col;
  }
  if (g.accumulate) {
#pragma unroll
    for (int r = 0; r < 16; ++r) old[r] = m0 + wmv * 32 + acc_row(r, lane) < g.M ? *dst[r] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wmv * 32 + acc_row(r, lane);
    if (m >= g.M) continue;
    float v = acc[r] + bv;
    if (g.act == ACT_RELU) v = reluf_(v);
    else if (g.act == ACT_TANH) v = tanhf(v);
    *dst[r] = g.accumulate ? old[r] + v : v;
  }
}

// split-K epilogue: partials summed in split order, then bias / act / row map / accumulate
__global__ void k_tgemm_reduce(TG g) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)g.M * g.N) return;
  const int m = (int)(i / g.N), n = (int)(i % g.N);
  float v = sk_sum(g.part, g.splits, (int64_t)g.M * g.N, i);
  v += (g.bias ? g.bias[n] : 0.f) + (g.bias2 ? g.bias2[n] : 0.f);
  if (g.act == ACT_RELU) v = reluf_(v);
  else if (g.act == ACT_TANH) v = tanhf(v);
  float* dst = g.C + (int64_t)(g.crow ? g.crow[m] : m) * g.ldc + n;
  *dst = g.accumulate ? *dst + v : v;
}

// k_tgemm_reduce four columns per thread (16-B partial loads and stores; every element's arithmetic
// and order exactly k_tgemm_reduce's): for N % 4 == 0 with 16-B aligned C rows, bias and partials
// (reduce_launch checks).  The element-wise form's 4-B loads ran the largest reduce (dW_m's, 5.2 M
// elements) at ~2 TB/s.
__global__ void k_tgemm_reduce4(TG g) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, i = 4 * q;
  if (i >= (int64_t)g.M * g.N) return;
  const int m = (int)(i / g.N), n = (int)(i % g.N);
  const int64_t MN = (int64_t)g.M * g.N;
  float4 x[SK_MAX];
#pragma unroll
  for (int sp = 0; sp < SK_MAX; ++sp)
    x[sp] = sp < g.splits ? *reinterpret_cast<const float4*>(g.part + sp * MN + i) : make_float4(0.f, 0.f, 0.f, 0.f);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (g.splits == 1) {
    v[0] = x[0].x; v[1] = x[0].y; v[2] = x[0].z; v[3] = x[0].w;
  } else {
#pragma unroll
    for (int sp = 0; sp < SK_MAX; ++sp)
      if (sp < g.splits) {
        v[0] += x[sp].x; v[1] += x[sp].y; v[2] += x[sp].z; v[3] += x[sp].w;
      }
    for (int sp = SK_MAX; sp < g.splits; ++sp) {
      const float4 y = *reinterpret_cast<const float4*>(g.part + sp * MN + i);
      v[0] += y.x; v[1] += y.y; v[2] += y.z; v[3] += y.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] + 0.f;
  }
  float* dst = g.C + (int64_t)(g.crow ? g.crow[m] : m) * g.ldc + n;
  const float4 old = g.accumulate ? *reinterpret_cast<const float4*>(dst) : make_float4(0.f, 0.f, 0.f, 0.f);
  float r[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float t = v[e] + ((g.bias ? g.bias[n + e] : 0.f) + (g.bias2 ? g.bias2[n + e] : 0.f));
    if (g.act == ACT_RELU) t = reluf_(t);
    else if (g.act == ACT_TANH) t = tanhf(t);
    r[e] = g.accumulate ? (&old.x)[e] + t : t;
  }
  *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
}

// the split-K reduce of `g`: four columns per thread when the shapes and pointers allow
static void reduce_launch(const TG& g, hipStream_t s) {
  const auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (g.N % 4 == 0 && g.ldc % 4 == 0 && a16(g.C) && a16(g.part))
    hipLaunchKernelGGL(k_tgemm_reduce4, dim3((unsigned)(((int64_t)g.M * g.N / 4 + 255) / 256)), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL(k_tgemm_reduce, dim3((unsigned)(((int64_t)g.M * g.N + 255) / 256)), dim3(256), 0, s, g);
}

// k_tgemm's split-K bound (floats of partials): its split counts, and so its fp32 sums, as before
// the scratch grew for k_bgemm
constexpr size_t TG_SPLIT_CAP = (size_t)4 << 20;

int tgemm(const GemmCtx& gc, TG g, bool defer) {
  const int M = g.M, N = g.N, K = g.K;
  if (M <= 0 || N <= 0) return 0;
  const hipStream_t s = gc.s;
  static const bool tlog = [] {  // AA_TG_LOG=1: one stderr line per GEMM (shape attribution of a trace)
    const char* e = getenv("AA_TG_LOG");
    return e && atoi(e) == 1;
  }();
  if (tlog) fprintf(stderr, "tgemm M %d N %d K %d at %d wm %d acc %d stream %p\n", M, N, K, (int)g.at, (int)g.wm, g.accumulate, (void*)s);
  const int tiles = ((M + 63) / 64) * ((N + 63) / 64);
  int splits = 1;
  // few tiles: split to ~256 workgroups (>= 128 deep each); long K over < 512 tiles (the vocab-sized
  // backward GEMMs, the weight gradients over all T*B rows): split to ~1024 (>= 512 deep each)
  const bool small = tiles < 128 && K >= 256, deep = tiles < 512 && K >= 1024;
  // workgroups a deep split aims at (512 / 256 measured within one box's noise of 1024:
  // profiles/r06z3_train_bgemm_split_ab.txt)
  constexpr int deep_wg = 1024;
  if ((small || deep) && gc.split) {
    splits = small ? (256 + tiles - 1) / tiles : (deep_wg + tiles - 1) / tiles;
    const int kmax = K / (small ? 128 : 512);
    if (splits > kmax) splits = kmax;
    const size_t capsp = (gc.cap < TG_SPLIT_CAP ? gc.cap : TG_SPLIT_CAP) / ((size_t)M * N);
    if ((size_t)splits > capsp) splits = (int)capsp;
    if (splits < 2) splits = 1;
  }
  int kper = K;
  if (splits > 1) {
    const int ks = gc.bf16 ? TStep<true>::KS : TStep<false>::KS;
    kper = ((K + splits - 1) / splits + ks - 1) / ks * ks;
    splits = (K + kper - 1) / kper;
  }
  // split-K partials reduced by k_tgemm_reduce unless the consumer sums them itself (defer).  (An
  // in-launch combine by each tile's last-arriving split -- device-scope ticket, write-through
  // partials -- was bit-identical and measured slower in round 4: 597-602 vs 683-698 steps/s.)
  g.splits = splits;
  g.kper = kper;
  g.part = splits > 1 ? gc.split : nullptr;
  if (gc.bf16)
    hipLaunchKernelGGL(k_tgemm<true>, dim3(tiles * splits), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL(k_tgemm<false>, dim3(tiles * splits), dim3(256), 0, s, g);
  if (splits > 1 && !defer) reduce_launch(g, s);
  return splits;
}


// ---------------------------------------------------------------------------------------------
// The four large GEMMs of a bf16 step (vocab forward, dU = dS W_m, dW_m = dS^T U, dW_a = dV^T A) on
// pre-packed bf16 operands: k_tgemm converted fp32 operands while staging 64 x 64 tiles (16 FLOP
// per byte through the CU, 6-10 % of the bf16 peak on these shapes).  Here both operands are bf16,
// row-major and K-contiguous ("NT": C[m][n] = sum_k A[m][k] B[n][k]), K a multiple of 64 with
// zero padding, produced by the k_pk_* kernels below (RNE, the same rounding k_tgemm<true> applies
// while staging), and a workgroup computes a 128 x 128 tile (four waves of 64 x 64 = 2 x 2
// v_mfma_f32_32x32x16_bf16 blocks), 64-deep K steps double-buffered in LDS (144-B rows:
// conflict-free 16-B fragment reads and staging stores).  Split-K partials go through
// k_tgemm_reduce (fixed split order), so a step stays deterministic.
// ---------------------------------------------------------------------------------------------
constexpr int BG_T = 128, BG_KS = 64, BG_LD = BG_KS + 8;
__global__ __launch_bounds__(256, 2) void k_bgemm(BG g) {
  __shared__ __attribute__((aligned(16))) __bf16 lds[2][2][BG_T * BG_LD];
  const int tilesN = (g.N + BG_T - 1) / BG_T;
  const int split = blockIdx.x % g.splits, tile = blockIdx.x / g.splits;
  const int mt = tile / tilesN, nt = tile % tilesN;
  const int m0 = mt * BG_T, n0 = nt * BG_T;
  const int kbeg = split * g.kper, kend = kbeg + g.kper < g.K ? kbeg + g.kper : g.K;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  // staging: 128 rows x 64 k per operand and step = 1024 16-B pieces, four per thread: piece
  // q = t + 256 i -> row q >> 3, k 8 (q & 7) (8 lanes per 128-B row: coalesced loads, conflict-free
  // ds_write_b128); rows past M / N are clamped (never stored)
  const __bf16* pa[4];
  const __bf16* pb[4];
  int so[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = t + 256 * i, r = q >> 3, kq = (q & 7) * 8;
    const int m = m0 + r < g.M ? m0 + r : g.M - 1, n = n0 + r < g.N ? n0 + r : g.N - 1;
    pa[i] = g.A + (int64_t)m * g.lda + kq;
    pb[i] = g.B + (int64_t)n * g.ldb + kq;
    so[i] = r * BG_LD + kq;
  }
  bf16x8 ra[4], rb[4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const bf16x8*>(pa[i] + k0);
      rb[i] = *reinterpret_cast<const bf16x8*>(pb[i] + k0);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<bf16x8*>(&lds[buf][0][so[i]]) = ra[i];
      *reinterpret_cast<bf16x8*>(&lds[buf][1][so[i]]) = rb[i];
    }
  };
  floatx16 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;
  const int nk = (kend - kbeg) / BG_KS;
  gload(kbeg);
  lstore(0);
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    const int buf = ks & 1;
    if (ks + 1 < nk) gload(kbeg + (ks + 1) * BG_KS);
    const __bf16* As = lds[buf][0];
    const __bf16* Bs = lds[buf][1];
#pragma unroll
    for (int kb = 0; kb < BG_KS / 16; ++kb) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) a[x] = *reinterpret_cast<const bf16x8*>(As + (wm * 64 + x * 32 + li) * BG_LD + 16 * kb + 8 * lh);
#pragma unroll
      for (int y = 0; y < 2; ++y) b[y] = *reinterpret_cast<const bf16x8*>(Bs + (wn * 64 + y * 32 + li) * BG_LD + 16 * kb + 8 * lh);
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[x], b[y], acc[x][y], 0, 0, 0);
    }
    if (ks + 1 < nk) lstore(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int y = 0; y < 2; ++y) {
    const int col = n0 + wn * 64 + y * 32 + li;
    if (col >= g.N) continue;
    const float bv = g.bias ? g.bias[col] : 0.f;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 + x * 32 + acc_row(r, lane);
        if (m >= g.M) continue;
        if (g.splits > 1) {
          g.part[(int64_t)split * g.M * g.N + (int64_t)m * g.N + col] = acc[x][y][r];
        } else {
          float v = acc[x][y][r] + bv;
          if (g.act == ACT_RELU) v = reluf_(v);
          float* dst = g.C + (int64_t)(g.crow ? g.crow[m] : m) * g.ldc + col;
          *dst = g.accumulate ? *dst + v : v;
        }
      }
  }
}

// dst[r][k] = bf16(src[map ? map[r] : r][k]) for k < cols, 0 up to Kp (a multiple of 8): 8 per thread,
// as two 16-B loads when the source rows allow (vec: lds % 4 == 0, cols % 8 == 0, 16-B aligned base)
__global__ void k_pk_rows(const float* __restrict__ src, int64_t lds, const int* __restrict__ map, int rows, int cols,
                          __bf16* __restrict__ dst, int Kp, int vec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per = Kp / 8;
  if (i >= (int64_t)rows * per) return;
  const int r = (int)(i / per), k0 = (int)(i % per) * 8;
  const float* sr = src + (int64_t)(map ? map[r] : r) * lds;
  bf16x8 v;
  if (vec && k0 < cols) {
    const float4 x = *reinterpret_cast<const float4*>(sr + k0), y = *reinterpret_cast<const float4*>(sr + k0 + 4);
    v[0] = (__bf16)x.x; v[1] = (__bf16)x.y; v[2] = (__bf16)x.z; v[3] = (__bf16)x.w;
    v[4] = (__bf16)y.x; v[5] = (__bf16)y.y; v[6] = (__bf16)y.z; v[7] = (__bf16)y.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)(k0 + j < cols ? sr[k0 + j] : 0.f);
  }
  *reinterpret_cast<bf16x8*>(dst + (int64_t)r * Kp + k0) = v;
}

// transpose: dst[c][r] = bf16(src[r lds + c]) for r < rows, 0 for rows <= r < Kp; dst has cols rows
// of Kp.  64 x 64 tiles through LDS (reads along c, writes along r, both coalesced).  S: float or
// __bf16 (a bf16 source is already rounded: the same values)
template <class S>
__global__ __launch_bounds__(256) void k_pk_trans(const S* __restrict__ src, int64_t lds, int rows, int cols,
                                                  __bf16* __restrict__ dst, int Kp) {
  __shared__ float tile[64][65];
  const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64, t = threadIdx.x;
  for (int i = t; i < 64 * 64; i += 256) {
    const int rr = i / 64, cc = i % 64, r = r0 + rr, c = c0 + cc;
    tile[rr][cc] = (r < rows && c < cols) ? (float)src[(int64_t)r * lds + c] : 0.f;
  }
  __syncthreads();
  for (int i = t; i < 64 * 64; i += 256) {
    const int cc = i / 64, rr = i % 64, c = c0 + cc, r = r0 + rr;
    if (c < cols && r < Kp) dst[(int64_t)c * Kp + r] = (__bf16)tile[rr][cc];
  }
}

// the NCHW feature map as the bf16 row matrix of the encoder GEMM V = relu(A W_a^T + b): dst[b 49 + p][c]
// = feats[b][c][p]; a workgroup per (image, 64 channels) reads its 64 x 49 contiguous floats and writes
// 49 rows of 128 B
__global__ __launch_bounds__(256) void k_pk_featrows(const float* __restrict__ feats, int C, __bf16* __restrict__ dst) {
  __shared__ float tile[64 * P];
  const int b = blockIdx.y, c0 = blockIdx.x * 64, t = threadIdx.x;
  const float* src = feats + ((int64_t)b * C + c0) * P;
  for (int i = t; i < 64 * P; i += 256) tile[i] = src[i];  // [c][p]
  __syncthreads();
  for (int i = t; i < P * 8; i += 256) {  // row p, 8-channel piece j
    const int p = i >> 3, j = i & 7;
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (__bf16)tile[(8 * j + e) * P + p];
    *reinterpret_cast<bf16x8*>(dst + ((int64_t)b * P + p) * C + c0 + 8 * j) = v;
  }
}

// One pass over the NCHW feature map for a bf16 step: a workgroup per (image, 64 channels) reads its
// 64 x 49 contiguous floats once and writes (1) the rows of the encoder GEMM's operand, as
// k_pk_featrows; (2) the K-contiguous operand of the backward's dW_a = dV^T A, cols[c][b 49 + p] (as
// k_pk_feats, zero past row B 49 up to Kp: the last image's workgroups); (3) a_g[b][c] = the 49 values
// summed in p order / 49 -- k_avgpool's arithmetic, bit-identical.  Replaces k_avgpool +
// k_pk_featrows + the backward's k_pk_feats (three reads of the map, one now).
__global__ __launch_bounds__(256) void k_pk_feats3(const float* __restrict__ feats, int B, int C,
                                                   __bf16* __restrict__ rows, __bf16* __restrict__ cols, int Kp,
                                                   float* __restrict__ a_g) {
  __shared__ float tile[64 * P];
  const int b = blockIdx.y, c0 = blockIdx.x * 64, t = threadIdx.x;
  const float* src = feats + ((int64_t)b * C + c0) * P;
  for (int i = t; i < 64 * P; i += 256) tile[i] = src[i];  // [c][p]
  __syncthreads();
  for (int i = t; i < P * 8; i += 256) {  // row p, 8-channel piece j
    const int p = i >> 3, j = i & 7;
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (__bf16)tile[(8 * j + e) * P + p];
    *reinterpret_cast<bf16x8*>(rows + ((int64_t)b * P + p) * C + c0 + 8 * j) = v;
  }
  for (int i = t; i < 64 * P; i += 256) {
    const int c = i / P, p = i - c * P;
    cols[(int64_t)(c0 + c) * Kp + b * P + p] = (__bf16)tile[i];
  }
  if (b == B - 1)
    for (int i = t; i < 64 * (Kp - B * P); i += 256) {
      const int c = i / (Kp - B * P), r = B * P + i % (Kp - B * P);
      cols[(int64_t)(c0 + c) * Kp + r] = (__bf16)0.f;
    }
  if (t < 64) {
    const float* g = tile + t * P;
    float sum = 0.f;
    for (int p = 0; p < P; ++p) sum += g[p];
    a_g[(int64_t)b * C + c0 + t] = sum / 49.0f;
  }
}

// the NCHW feature map as the K-contiguous operand of dW_a = dV^T A: dst[c][b 49 + p] = feats[b][c][p],
// zero for rows >= B 49 up to Kp; 8 consecutive rows per thread (one 16-B store)
__global__ void k_pk_feats(const float* __restrict__ feats, int B, int C, __bf16* __restrict__ dst, int Kp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per = Kp / 8;
  if (i >= (int64_t)C * per) return;
  const int c = (int)(i / per), row0 = (int)(i % per) * 8;
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = row0 + j;
    float x = 0.f;
    if (row < B * P) {
      const int b = row / P, p = row - b * P;
      x = feats[((int64_t)b * C + c) * P + p];
    }
    v[j] = (__bf16)x;
  }
  *reinterpret_cast<bf16x8*>(dst + (int64_t)c * Kp + row0) = v;
}

// C[M,N] (+)= A B^T (+ bias) on k_bgemm; K a multiple of 64.  Fewer than 512 tiles: split K to
// ~256 workgroups (bounded by the split scratch), partials reduced by k_tgemm_reduce in split order.
void bgemm(const GemmCtx& gc, BG g) {
  const int M = g.M, N = g.N, K = g.K;
  if (M <= 0 || N <= 0 || K <= 0) return;
  const int tiles = ((M + BG_T - 1) / BG_T) * ((N + BG_T - 1) / BG_T), ksteps = K / BG_KS;
  // workgroups a split launch aims at: 64 / 128 / 192 / 512 / 1024 / 2048 measured no better (at 1024
  // dU's split writes 18 partial sets where 256 writes 5: profiles/r06z3_train_bgemm_split_ab.txt)
  constexpr int wg_target = 256;
  int splits = tiles >= 512 ? 1 : (wg_target + tiles - 1) / tiles;
  if (splits > ksteps) splits = ksteps;
  const size_t capsp = gc.split ? gc.cap / ((size_t)M * N) : 1;
  if ((size_t)splits > capsp) splits = (int)capsp;
  if (splits < 1) splits = 1;
  const int kper = (ksteps + splits - 1) / splits * BG_KS;
  splits = (K + kper - 1) / kper;
  g.splits = splits;
  g.kper = kper;
  g.part = splits > 1 ? gc.split : nullptr;
  hipLaunchKernelGGL(k_bgemm, dim3(tiles * splits), dim3(256), 0, gc.s, g);
  if (splits > 1) {
    TG r{};
    r.M = M; r.N = N; r.K = K; r.C = g.C; r.ldc = g.ldc; r.crow = g.crow; r.bias = g.bias; r.accumulate = g.accumulate;
    r.splits = splits; r.kper = kper; r.part = gc.split; r.act = g.act;
    reduce_launch(r, gc.s);
  }
}
void pk_rows(hipStream_t st, const float* src, int64_t lds, const int* map, int rows, int cols, __bf16* dst, int Kp) {
  const int64_t n = (int64_t)rows * (Kp / 8);
  const int vec = lds % 4 == 0 && cols % 8 == 0 && ((uintptr_t)src & 15) == 0;
  hipLaunchKernelGGL(k_pk_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, lds, map, rows, cols, dst, Kp,
                     vec);
}
template <class S>
void pk_trans(hipStream_t st, const S* src, int64_t lds, int rows, int cols, __bf16* dst, int Kp) {
  hipLaunchKernelGGL(k_pk_trans<S>, dim3((unsigned)(Kp / 64), (unsigned)((cols + 63) / 64)), dim3(256), 0, st, src, lds,
                     rows, cols, dst, Kp);
}
template void pk_trans<float>(hipStream_t, const float*, int64_t, int, int, __bf16*, int);
template void pk_trans<__bf16>(hipStream_t, const __bf16*, int64_t, int, int, __bf16*, int);
void pk_feats3(hipStream_t st, const float* feats, int B, int C, __bf16* rows, __bf16* cols, float* a_g) {
  hipLaunchKernelGGL(k_pk_feats3, dim3(C / 64, B), dim3(256), 0, st, feats, B, C, rows, cols, rup64(B * P), a_g);
}

// column sums: out[n] = sum_m X[m ldx + n], deterministic: rows split into CS_CH fixed chunks
// summed in order by k_colsum (one thread per (column, chunk)), the chunk sums added in chunk
// order by k_colsum_fin.
__global__ void k_colsum(const float* __restrict__ X, int M, int N, int64_t ldx, float* __restrict__ part) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x, ch = blockIdx.y;
  if (n >= N) return;
  const int per = (M + CS_CH - 1) / CS_CH, m0 = ch * per, m1 = m0 + per < M ? m0 + per : M;
  float s = 0.f;
  int m = m0;
  // eight loads in flight, then the eight adds in row order (the same sum, bit for bit, as one row
  // at a time; a chunk of 98 rows -- the dV bias gradient -- ran ~30 us one dependent load at a time)
  for (; m + 8 <= m1; m += 8) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = X[(int64_t)(m + j) * ldx + n];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += x[j];
  }
  for (; m < m1; ++m) s += X[(int64_t)m * ldx + n];
  part[(int64_t)ch * N + n] = s;
}
__global__ void k_colsum_fin(const float* __restrict__ part, int N, float* __restrict__ out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int ch = 0; ch < CS_CH; ++ch) s += part[(int64_t)ch * N + n];
  out[n] = s;
}
// k_colsum + k_colsum_fin in one launch for short columns (M <= CS1_MAXM: the encoder-head bias
// gradients over the B rows): a workgroup per 64 columns, wave g sums chunks [16 g, 16 g + 16) of
// its lane's column (k_colsum's chunks, rows in order from 0), the 64 chunk sums go through LDS and
// lane c of wave 0 adds them in chunk order from 0 -- k_colsum_fin's arithmetic: the same bits, one
// launch instead of two, every load of a thread in flight at once.
constexpr int CS1_MAXM = 512;
__global__ __launch_bounds__(256) void k_colsum1(const float* __restrict__ X, int M, int N, int64_t ldx,
                                                 float* __restrict__ out) {
  __shared__ float cs[CS_CH][65];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6, n = blockIdx.x * 64 + c;
  const int per = (M + CS_CH - 1) / CS_CH;
  const int nc = n < N ? n : N - 1;
  for (int j = 0; j < CS_CH / 4; ++j) {
    const int ch = 16 * g + j, m0 = ch * per, m1 = m0 + per < M ? m0 + per : M;
    float x[CS1_MAXM / CS_CH];
#pragma unroll
    for (int i = 0; i < CS1_MAXM / CS_CH; ++i) x[i] = m0 + i < m1 ? X[(int64_t)(m0 + i) * ldx + nc] : 0.f;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CS1_MAXM / CS_CH; ++i)
      if (m0 + i < m1) s += x[i];
    cs[ch][c] = s;
  }
  __syncthreads();
  if (g == 0 && n < N) {
    float s = 0.f;
    for (int ch = 0; ch < CS_CH; ++ch) s += cs[ch][c];
    out[n] = s;
  }
}
void colsum_fin(hipStream_t st, const float* part, int N, float* out) {
  hipLaunchKernelGGL(k_colsum_fin, dim3((N + 255) / 256), dim3(256), 0, st, part, N, out);
}
void colsum(hipStream_t st, const float* X, int M, int N, int64_t ldx, float* scratch, float* out) {
  if (M > 0 && M <= CS1_MAXM) {
    hipLaunchKernelGGL(k_colsum1, dim3((N + 63) / 64), dim3(256), 0, st, X, M, N, ldx, out);
    return;
  }
  hipLaunchKernelGGL(k_colsum, dim3((N + 255) / 256, CS_CH), dim3(256), 0, st, X, M, N, ldx, scratch);
  colsum_fin(st, scratch, N, out);
}

}  // namespace aa

