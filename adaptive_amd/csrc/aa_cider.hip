// aa_cider.hip — CIDEr-D of token-id captions against a corpus resident on the device.
//
// What is computed is the reference's coco/pycocoevalcap/cider/cider_scorer.py (count clipping and a
// Gaussian length penalty: CIDEr-D, whatever the file is called), on token ids instead of words; restated
// on the CPU by tests/cider_oracle.py.  A caption is the ids before the row's first end_id (all T without
// one).  For a caption w_0 .. w_{L-1}, orders n = 1..4:
//   c(g)      count of the contiguous n-gram g
//   w(g)      log M - log max(1, df(g)), df = the number of corpus images with g in any reference, M = the
//             corpus's images; computed on the host in float64 and looked up here (absent: w_unseen = log M)
//   vec(g)    c(g) w(g);   norm_n = sqrt(sum_{|g| = n} vec(g)^2)
//   length    the number of BIGRAMS, max(L - 1, 0): the reference adds the term frequencies of its
//             zero-based order index 1.  Reproduced, not corrected.
//   per reference r, order n:
//             val = sum_{g in hyp} min(vec_h(g), vec_r(g)) vec_r(g)             (vec_r = 0 when absent)
//             if norm_h,n != 0 and norm_r,n != 0: val /= norm_h,n norm_r,n
//             val *= exp(-(length_h - length_r)^2 / (2 sigma^2))
//   score     10 mean_n(sum_r val_n) / #refs
//
// n-gram key: sum_j (tok_j + 1) << 16 j, j < n -- exact and collision-free for tokens in [0, 65535); the
// order is the number of non-zero 16-bit fields and 0 is no key.  References are CSR (img_ptr -> ref_ptr ->
// keys ascending / counts) with their norms and lengths precomputed; w(g) sits in an open-addressing table
// (slot = splitmix64(key) & (size - 1), linear probing, 0 = empty).
//
// k_cider: one 256-thread workgroup per caption, T <= 64.  Wave n - 1 owns order n and lane i the n-gram
// that starts at position i, so every per-order sum is one wave64 butterfly and the waves meet only for the
// last line.  Each wave reads the row's tokens itself (one 512-byte line, four times) and finds L with a
// ballot; keys go to LDS, where lane i counts its key among its wave's and learns whether it is the first
// occurrence.  First-occurrence lanes probe the table, then for each reference of the row's image
// binary-search its key range in global memory (a reference is a few hundred bytes; copying it to LDS
// first, behind two barriers per reference, measured 7 % faster per launch -- 2 us of a step whose draw
// takes 8.8 ms -- and was not kept: DESIGN.md section 17).  All arithmetic is
// float64 without contraction.  Every data-dependent loop is bounded (the probe by tab_size, the search by
// 64 halvings, the references by the corpus's count): a malformed corpus gives a wrong score, not a kernel
// that does not end.  A token outside [0, 65535) before the first end_id, or an image outside the corpus,
// makes the row's score NaN (the cross-entropy kernel's policy for a bad target).
#include <math.h>

#include "aa_internal.hpp"

namespace aa {

constexpr int CIDER_N = 4;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the entry of an ascending key range that holds `key`, or -1: at most 64 halvings
__device__ __forceinline__ int find_key(const uint64_t* __restrict__ keys, int n, uint64_t key) {
  int lo = 0, hi = n;
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && keys[lo] == key ? lo : -1;
}

__global__ __launch_bounds__(256) void k_cider(aa_cider_corpus C, const int64_t* __restrict__ ids, int T,
                                               int64_t ids_ld, int64_t end_id, const int32_t* __restrict__ image,
                                               double* __restrict__ scores) {
  __shared__ uint64_t skey[CIDER_N][64];
  __shared__ double sacc[CIDER_N];
  const int row = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = wv + 1;
  const int64_t img = image ? (int64_t)image[row] : (int64_t)row;
  const bool img_ok = img >= 0 && img < C.images;

  // tokens, L = the first end_id, the out-of-range flag
  const int64_t tok = lane < T ? ids[(int64_t)row * ids_ld + lane] : end_id;
  const uint64_t endm = __ballot(lane >= T || tok == end_id);
  const int L = endm ? __ffsll((unsigned long long)endm) - 1 : 64;  // no bit: T == 64 without an end_id
  const bool bad = __ballot(lane < L && (tok < 0 || tok >= 65535)) != 0;

  // lane i's n-gram: tokens i .. i + n - 1 (wave-uniform n: every lane runs the shuffles)
  const int nk = L - n + 1 > 0 ? L - n + 1 : 0;  // n-grams of this order
  const uint32_t t1 = (uint32_t)(tok & 0xFFFF) + 1u;
  uint64_t key = 0;
#pragma unroll
  for (int j = 0; j < CIDER_N; ++j) {
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

  // w(g) of the first occurrences: at most tab_size probes
  double w = 0.0;
  if (first) {
    w = C.w_unseen;
    const uint64_t mask = (uint64_t)C.tab_size - 1;
    uint64_t slot = splitmix(key) & mask;
    for (int64_t step = 0; step < C.tab_size; ++step) {
      const uint64_t tk = C.tab_keys[slot];
      if (tk == key) {
        w = C.tab_w[slot];
        break;
      }
      if (tk == 0) break;
      slot = (slot + 1) & mask;
    }
  }
  const double vh = first ? (double)cnt * w : 0.0;
  const double nh = sqrt(wave_sum(vh * vh));
  const int len_h = L > 0 ? L - 1 : 0;

  // the row's references, in order
  int r0 = 0, r1 = 0;
  if (img_ok) {
    r0 = C.img_ptr[img];
    r1 = C.img_ptr[img + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > C.refs ? C.refs : r1;
  }
  const double inv2s2 = 2.0 * (C.sigma * C.sigma);
  double acc = 0.0;
  for (int r = r0; r < r1; ++r) {
    double term = 0.0;
    const int e0 = C.ref_ptr[r], ne = C.ref_ptr[r + 1] - e0;
    if (first) {
      const int at = find_key(C.keys + e0, ne, key);
      const double vr = at >= 0 ? (double)C.counts[e0 + at] * w : 0.0;  // absent: 0
      term = fmin(vh, vr) * vr;
    }
    double val = wave_sum(term);
    if (lane == 0) {
      const double nr = C.ref_norm[(int64_t)r * CIDER_N + wv];
      if (nh != 0.0 && nr != 0.0) val /= nh * nr;
      const double delta = (double)(len_h - C.ref_len[r]);
      val *= exp(-(delta * delta) / inv2s2);
      acc += val;
    }
  }
  if (lane == 0) sacc[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = (((sacc[0] + sacc[1]) + sacc[2]) + sacc[3]) / 4.0;  // the reference's mean, then / #refs, then * 10
    s = s / (double)(r1 - r0) * 10.0;
    scores[row] = (bad || !img_ok || r1 <= r0) ? (double)NAN : s;
  }
}

}  // namespace aa

using namespace aa;

int aa_cider_score(const aa_cider_corpus* corpus, const int64_t* ids, int32_t R, int32_t T, int64_t ids_ld,
                   int32_t end_id, const int32_t* image, double* scores, aa_stream_t stream) {
  if (R < 0 || T < 0 || T > AA_CIDER_MAX_T || ids_ld < T) return AA_ERR_SHAPE;
  if (R == 0) return AA_OK;
  if (!corpus) return AA_ERR_NULL;
  const aa_cider_corpus& c = *corpus;
  if (c.images < 1 || c.refs < 1 || c.tab_size < 1 || (c.tab_size & (c.tab_size - 1)) != 0) return AA_ERR_SHAPE;
  if (!(c.sigma > 0.0) || !(c.sigma <= 1.7976931348623157e308)) return AA_ERR_SHAPE;  // NaN fails the first
  if (!c.img_ptr || !c.ref_ptr || !c.keys || !c.counts || !c.ref_norm || !c.ref_len || !c.tab_keys || !c.tab_w)
    return AA_ERR_NULL;
  if ((!ids && T > 0) || !scores) return AA_ERR_NULL;
  hipLaunchKernelGGL(k_cider, dim3(R), dim3(256), 0, (hipStream_t)stream, c, ids, T, ids_ld, (int64_t)end_id, image,
                     scores);
  return launch_status();
}
