// aa_metrics.hip — BLEU-1..4 and ROUGE-L of token-id captions against a corpus resident on the device.
//
// What is computed is the reference's coco/pycocoevalcap/bleu/bleu_scorer.py (as bleu/bleu.py calls it:
// option 'closest', n = 4) and rouge/rouge.py, on token ids instead of words; include/adaptive_amd.h states
// the expressions and tests/metrics_oracle.py restates them on the CPU.  A caption is the ids before the
// row's first end_id (all T without one); n-gram keys are aa_cider.hip's.
//
// k_metrics: one 256-thread workgroup per caption, T <= 64, laid out like k_cider.  Wave n - 1 owns order n
// and lane i the n-gram that starts at position i: keys go to LDS, lane i counts its key among its wave's
// and learns whether it is the first occurrence, first-occurrence lanes binary-search the image's
// clip-count range (one search per n-gram: the maximum over the references was taken on the host), and a
// wave butterfly sums min(count, clip) into correct_n.
// ROUGE-L: the hypothesis has at most 64 tokens, so the LCS against a reference of any length is the
// bit-parallel recurrence on one 64-bit word per wave (Crochemore et al. / Hyyro: V = ~0; per reference
// token U = V & M, V = (V + U) | (V - U); LCS = the zeros among V's low L bits).  The match mask M of a
// reference token is a wave64 ballot of hyp_tok == ref_tok over the lanes that hold the hypothesis, so no
// table of masks is built; a wave loads 64 reference tokens at a time (lane j token j) and broadcasts them
// one by one.  The four waves take the image's references in turn; the largest lcs (prec's numerator), the
// largest rec and the closest reference length meet in LDS.  The carries of V + U run upwards only, so
// the bits above L never reach the bits below it and are masked off at the popcount.
// All float arithmetic is float64 without contraction.  Every data-dependent loop is bounded (the search by
// 64 halvings, the LCS by the reference's stored length, the references by the corpus's count): a
// malformed corpus gives a wrong score, not a kernel that does not end.  A token outside [0, 65535) before
// the first end_id, or an image outside the corpus, makes the row's floats NaN and its statistics 0.
//
// k_bleu_corpus: one workgroup; int64 column totals of the rows' statistics, then the corpus expression.
#include <math.h>

#include "aa_internal.hpp"

namespace aa {

constexpr int MET_N = 4;
constexpr int MET_STATS = 10;  // correct_1..4, guess_1..4, testlen, reflen

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the entry of an ascending key range that holds `key`, or -1: at most 64 halvings
__device__ __forceinline__ int find_clip(const uint64_t* __restrict__ keys, int n, uint64_t key) {
  int lo = 0, hi = n;
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && keys[lo] == key ? lo : -1;
}

// bleu_1..4 of ten statistics (int64: a row's or the corpus totals), the reference's order of operations
__device__ __forceinline__ double bleu_of(const int64_t* correct, const int64_t* guess, int64_t testlen,
                                          int64_t reflen, int n) {
  double b = 1.0;
  for (int k = 0; k < n; ++k) b *= ((double)correct[k] + 1e-15) / ((double)guess[k] + 1e-9);
  double v = pow(b, 1.0 / (double)n);
  const double ratio = ((double)testlen + 1e-15) / ((double)reflen + 1e-9);
  if (ratio < 1.0) v *= exp(1.0 - 1.0 / ratio);
  return v;
}

__global__ __launch_bounds__(256) void k_metrics(aa_metrics_corpus C, const int64_t* __restrict__ ids, int T,
                                                 int64_t ids_ld, int64_t end_id, const int32_t* __restrict__ image,
                                                 int32_t* __restrict__ stats, double* __restrict__ bleu,
                                                 double* __restrict__ rouge) {
  __shared__ uint64_t skey[MET_N][64];
  __shared__ int scorrect[MET_N];
  __shared__ uint64_t sclose[MET_N];  // (|l - L| << 32) | l of the wave's closest reference
  __shared__ int slcs[MET_N];
  __shared__ double srec[MET_N];
  const int row = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = wv + 1;
  const int64_t img = image ? (int64_t)image[row] : (int64_t)row;
  const bool img_ok = img >= 0 && img < C.images;

  // tokens, L = the first end_id, the out-of-range flag
  const int64_t tok = lane < T ? ids[(int64_t)row * ids_ld + lane] : end_id;
  const uint64_t endm = __ballot(lane >= T || tok == end_id);
  const int L = endm ? __ffsll((unsigned long long)endm) - 1 : 64;  // no bit: T == 64 without an end_id
  const bool bad = __ballot(lane < L && (tok < 0 || tok >= 65535)) != 0;

  // lane i's n-gram: tokens i .. i + n - 1 (wave-uniform n: every lane runs the shuffles)
  const int nk = L - n + 1 > 0 ? L - n + 1 : 0;  // n-grams of this order: guess_n
  const uint32_t t1 = (uint32_t)(tok & 0xFFFF) + 1u;
  uint64_t key = 0;
#pragma unroll
  for (int j = 0; j < MET_N; ++j) {
    const uint32_t tj = __shfl(t1, (lane + j) & 63, 64);
    if (j < n) key |= (uint64_t)tj << (16 * j);
  }
  if (lane >= nk || bad) key = 0;
  skey[wv][lane] = key;
  __syncthreads();
  int cnt = 0;
  bool first = key != 0;
  for (int k = 0; k < nk; ++k) {
    const bool same = skey[wv][k] == key;
    cnt += same;
    first = first && !(same && k < lane);
  }

  // correct_n: the first occurrences against the image's clip counts
  int r0 = 0, r1 = 0, e0 = 0, ne = 0;
  if (img_ok) {
    r0 = C.img_ptr[img];
    r1 = C.img_ptr[img + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > C.refs ? C.refs : r1;
    e0 = C.clip_ptr[img];
    ne = C.clip_ptr[img + 1] - e0;
  }
  int term = 0;
  if (first) {
    const int at = find_clip(C.clip_keys + e0, ne, key);
    const int clip = at >= 0 ? C.clip_counts[e0 + at] : 0;
    term = cnt < clip ? cnt : clip;
  }
  const int correct = wave_sum_int(term);

  // this wave's references: the closest length, and the LCS on one 64-bit word
  const uint64_t maskL = L >= 64 ? ~0ull : (1ull << L) - 1ull;
  const bool holds = lane < L && !bad;
  const uint32_t htok = (uint32_t)tok;
  uint64_t closest = ~0ull;
  int lcs_max = 0;
  double rec_max = 0.0;
  for (int r = r0 + wv; r < r1; r += MET_N) {
    const int t0 = C.tok_ptr[r], have = C.tok_ptr[r + 1] - t0;
    int lr = C.ref_len[r];
    lr = lr > have ? have : lr;
    lr = lr < 0 ? 0 : lr;
    const uint64_t dist = (uint64_t)(lr > L ? lr - L : L - lr);
    const uint64_t ck = (dist << 32) | (uint64_t)(uint32_t)lr;
    closest = ck < closest ? ck : closest;
    uint64_t V = ~0ull;
    for (int base = 0; base < lr; base += 64) {
      const int m = lr - base < 64 ? lr - base : 64;
      const uint32_t rt = lane < m ? (uint32_t)C.ref_tok[(int64_t)t0 + base + lane] : 0xFFFFFFFFu;
      for (int j = 0; j < m; ++j) {
        const uint32_t y = __shfl(rt, j, 64);
        const uint64_t M = __ballot(holds && htok == y);
        const uint64_t U = V & M;
        V = (V + U) | (V - U);
      }
    }
    int lcs = __popcll((unsigned long long)(~V & maskL));
    if (L == 0 && lr == 0) lcs = 1;  // the reference's "".split(" "): one empty word on each side
    lcs_max = lcs > lcs_max ? lcs : lcs_max;
    const double rec = (double)lcs / (double)(lr > 0 ? lr : 1);
    rec_max = rec > rec_max ? rec : rec_max;
  }
  if (lane == 0) {
    scorrect[wv] = correct;
    sclose[wv] = closest;
    slcs[wv] = lcs_max;
    srec[wv] = rec_max;
  }
  __syncthreads();
  if (lane != 0) return;

  const bool nan_row = bad || !img_ok || r1 <= r0;
  uint64_t ck = sclose[0];
  for (int k = 1; k < MET_N; ++k) ck = sclose[k] < ck ? sclose[k] : ck;
  const int64_t reflen = (int64_t)(ck & 0xFFFFFFFFull);
  int64_t cor[MET_N], gue[MET_N];
  for (int k = 0; k < MET_N; ++k) {
    cor[k] = scorrect[k];
    gue[k] = L - k > 0 ? L - k : 0;
  }
  // lane 0 of wave n - 1 finishes bleu_n; wave 0's also the statistics and ROUGE-L
  bleu[(int64_t)row * MET_N + wv] = nan_row ? (double)NAN : bleu_of(cor, gue, L, reflen, n);
  if (wv != 0) return;
  int32_t* st = stats + (int64_t)row * MET_STATS;
  for (int k = 0; k < MET_N; ++k) {
    st[k] = nan_row ? 0 : (int32_t)cor[k];
    st[MET_N + k] = nan_row ? 0 : (int32_t)gue[k];
  }
  st[8] = nan_row ? 0 : L;
  st[9] = nan_row ? 0 : (int32_t)reflen;
  int lcs = slcs[0];
  double rc = srec[0];
  for (int k = 1; k < MET_N; ++k) {
    lcs = slcs[k] > lcs ? slcs[k] : lcs;
    rc = srec[k] > rc ? srec[k] : rc;
  }
  const double p = (double)lcs / (double)(L > 0 ? L : 1);
  const double beta2 = 1.2 * 1.2;
  double s = 0.0;
  if (p != 0.0 && rc != 0.0) s = ((1.0 + beta2) * p * rc) / (rc + beta2 * p);
  rouge[row] = nan_row ? (double)NAN : s;
}

__global__ __launch_bounds__(256) void k_bleu_corpus(const int32_t* __restrict__ stats, int R,
                                                     double* __restrict__ out) {
  __shared__ int64_t stot[4][MET_STATS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int64_t acc[MET_STATS];
#pragma unroll
  for (int c = 0; c < MET_STATS; ++c) acc[c] = 0;
  for (int r = threadIdx.x; r < R; r += 256) {
#pragma unroll
    for (int c = 0; c < MET_STATS; ++c) acc[c] += (int64_t)stats[(int64_t)r * MET_STATS + c];
  }
#pragma unroll
  for (int c = 0; c < MET_STATS; ++c) {
    uint64_t v = (uint64_t)acc[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
    if (lane == 0) stot[wv][c] = (int64_t)v;
  }
  __syncthreads();
  if (threadIdx.x >= MET_N) return;
  int64_t tot[MET_STATS];
  for (int c = 0; c < MET_STATS; ++c) tot[c] = ((stot[0][c] + stot[1][c]) + stot[2][c]) + stot[3][c];
  out[threadIdx.x] = bleu_of(tot, tot + MET_N, tot[8], tot[9], (int)threadIdx.x + 1);
}

}  // namespace aa

using namespace aa;

int aa_metrics_score(const aa_metrics_corpus* corpus, const int64_t* ids, int32_t R, int32_t T, int64_t ids_ld,
                     int32_t end_id, const int32_t* image, int32_t* stats, double* bleu, double* rouge,
                     aa_stream_t stream) {
  if (R < 0 || T < 0 || T > AA_CIDER_MAX_T || ids_ld < T) return AA_ERR_SHAPE;
  if (R == 0) return AA_OK;
  if (!corpus) return AA_ERR_NULL;
  const aa_metrics_corpus& c = *corpus;
  if (c.images < 1 || c.refs < 1) return AA_ERR_SHAPE;
  if (!c.img_ptr || !c.clip_ptr || !c.clip_keys || !c.clip_counts || !c.ref_len || !c.tok_ptr || !c.ref_tok)
    return AA_ERR_NULL;
  if ((!ids && T > 0) || !stats || !bleu || !rouge) return AA_ERR_NULL;
  hipLaunchKernelGGL(k_metrics, dim3(R), dim3(256), 0, (hipStream_t)stream, c, ids, T, ids_ld, (int64_t)end_id, image,
                     stats, bleu, rouge);
  return launch_status();
}

int aa_bleu_corpus(const int32_t* stats, int32_t R, double* out, aa_stream_t stream) {
  if (R < 0) return AA_ERR_SHAPE;
  if (R == 0) return AA_OK;
  if (!stats || !out) return AA_ERR_NULL;
  hipLaunchKernelGGL(k_bleu_corpus, dim3(1), dim3(256), 0, (hipStream_t)stream, stats, R, out);
  return launch_status();
}
