// aa_tgemm.hpp — the training step's generic GEMM engine (aa_tgemm.hip) as the training code
// (aa_train.hip) calls it: the two GEMMs with their operands named at the call site, the bf16 operand
// packers and the deterministic column sums.  Every kernel of the engine is compiled in aa_tgemm.o
// only; sk_sum is the one device function shared, because the LSTM cell kernels sum a deferred
// GEMM's split-K partials themselves.
#pragma once
#include "aa_internal.hpp"

namespace aa {

// ---------------------------------------------------------------------------------------------
// generic GEMM: C[M, N] (+)= act(sum_k A(m, k) W(n, k) + bias[n] + bias2[n])
//   A(m, k) = at == A_COLS ? A[k lda + m] : A[row(m) lda + k]        row(m) = arow ? arow[m] : m
//   W(n, k) = wm == W_ROWS : W[n ldw + k]
//             wm == W_COLS : W[k ldw + n]
//             wm == W_NCHW : NCHW feature map [B][C][49] read as the [B*49, C] row matrix transposed:
//                            W(n = c, k = b*49 + p) = W[b*ldw*49 + c*49 + p]   (ldw = C)
//   C row m -> crow ? crow[m] : m
// TG is both the kernels' argument (k_tgemm, k_tgemm_reduce*) and the named-argument list of tgemm():
// a call site fills the operands with designated initialisers, tgemm() fills the split-K fields.
// ---------------------------------------------------------------------------------------------
enum TgA : int { A_ROWS = 0, A_COLS = 1 };               // A[m][k] | A[k][m] (the product A^T W^T)
enum TgW : int { W_ROWS = 0, W_COLS = 1, W_NCHW = 2 };   // W[n][k] | W[k][n] | the feature map
enum TgAct : int { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2 };
struct TG {
  int M, N, K;
  const float* A;
  int64_t lda;
  const int* arow = nullptr;
  TgA at = A_ROWS;
  const float* W;
  int64_t ldw;
  TgW wm = W_ROWS;
  float* C;
  int64_t ldc;
  const int* crow = nullptr;
  const float* bias = nullptr;
  const float* bias2 = nullptr;
  int accumulate = false;  // C += ...
  TgAct act = ACT_NONE;
  // filled by tgemm() / bgemm()
  int splits = 1;  // split-K: > 1 -> raw partial tiles to part[split][M][N], reduced by k_tgemm_reduce
  int kper = 0;    // K per split (multiple of the K step)
  float* part = nullptr;
};

// value i of a split GEMM: its S partials summed in split order from 0 (+ 0, as the reduce adds absent
// biases), or src itself when it was not split.  Up to SK_MAX partials are loaded together before the
// ordered sum (a loop over a runtime count waits for each load in turn).
constexpr int SK_MAX = 16;
__device__ __forceinline__ float sk_sum(const float* __restrict__ src, int S, int64_t MN, int64_t i) {
  if (S == 1) return src[i];
  float x[SK_MAX];
#pragma unroll
  for (int sp = 0; sp < SK_MAX; ++sp) x[sp] = sp < S ? src[sp * MN + i] : 0.f;
  float v = 0.f;
#pragma unroll
  for (int sp = 0; sp < SK_MAX; ++sp)
    if (sp < S) v += x[sp];
  for (int sp = SK_MAX; sp < S; ++sp) v += src[sp * MN + i];
  return v + 0.f;
}

// launch context of a training call: stream + split-K scratch carved from its workspace
struct GemmCtx {
  hipStream_t s;
  float* split;
  size_t cap;  // floats
  bool bf16;   // AA_TRAIN_BF16: bf16 operands, fp32 accumulation
  bool sent_h0 = false;  // AA_TRAIN_SENTINEL_H0: the sentinel gate without its h_{t-1} W_h term
};

// The GEMM `g` on k_tgemm; too few output tiles to fill the chip: split along K, deterministically
// reduced.  Returns the split count (0: nothing to do, M or N empty).
// `defer` (the recurrent LSTM GEMMs): a split-K GEMM leaves its partial tiles in gc.split and the
// consumer (k_tr_cell_sk / k_tr_cell_bwd_sk) sums them in split order itself -- k_tgemm_reduce's
// arithmetic, one launch fewer per recurrent step; 1 = C written (no split; no bias / act /
// accumulate allowed with defer).
constexpr bool TG_DEFER = true;
int tgemm(const GemmCtx& gc, TG g, bool defer = false);

// C[M,N] (+)= act(A B^T + bias) on k_bgemm: both operands bf16, row-major and K-contiguous, K a
// multiple of 64 with zero padding (the k_pk_* packers below).  BG, like TG, is the kernel's argument
// and the call's named-argument list.
struct BG {
  int M, N, K;
  const __bf16* A;
  int64_t lda;
  const __bf16* B;
  int64_t ldb;
  float* C;
  int64_t ldc;
  const int* crow = nullptr;
  const float* bias = nullptr;
  int accumulate = false;
  // filled by bgemm()
  int splits = 1, kper = 0;
  float* part = nullptr;
  TgAct act = ACT_NONE;  // none or relu (after the bias)
};
void bgemm(const GemmCtx& gc, BG g);

// bf16 operand packers (RNE, the rounding k_tgemm<true> applies while staging)
static inline int rup64(int x) { return (x + 63) / 64 * 64; }
// dst[r][k] = bf16(src[map ? map[r] : r][k]) for k < cols, 0 up to Kp (a multiple of 8)
void pk_rows(hipStream_t st, const float* src, int64_t lds, const int* map, int rows, int cols, __bf16* dst, int Kp);
// dst[c][r] = bf16(src[r lds + c]) for r < rows, 0 up to Kp (a multiple of 64); S: float or __bf16
template <class S>
void pk_trans(hipStream_t st, const S* src, int64_t lds, int rows, int cols, __bf16* dst, int Kp);
// one pass over the NCHW feature map: rows[b 49 + p][c], cols[c][b 49 + p] (pitch rup64(B 49)) and a_g
void pk_feats3(hipStream_t st, const float* feats, int B, int C, __bf16* rows, __bf16* cols, float* a_g);

// column sums out[n] = sum_m X[m ldx + n] in a fixed order: CS_CH row chunks summed in order into
// scratch [CS_CH][N], the chunk sums added in chunk order (colsum_fin: that second half alone)
constexpr int CS_CH = 64;
void colsum(hipStream_t st, const float* X, int M, int N, int64_t ldx, float* scratch, float* out);
void colsum_fin(hipStream_t st, const float* part, int N, float* out);

}  // namespace aa
