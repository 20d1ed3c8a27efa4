// aa_sample.hip — seeded temperature-sampling caption decode.  The reference has no sampling decode,
// so (as for beam search) its semantics are defined here and restated on the CPU by
// tests/sample_oracle.py SampleOracle:
//
//   step t, image b (global row row0 + b), exact fp32 logits x[v], v < V:
//     y[v]  = x[v] / tau                                               (fp32 division)
//     e     = ((row0 + b) T + t) V + v                                 (64-bit element counter)
//     u     = (2 (splitmix64(key + (e + 1) GOLDEN) >> 41) + 1) 2^-24   (exact in fp32, inside (0, 1))
//     g     = -log(-log(u))                                            (standard Gumbel noise)
//     token = argmax_v (y[v] + g)                                      (Gumbel-max: a draw from softmax(y));
//                                                                      ties to the smaller v
//     logp  = y[token] - (max y + log sum exp(y - max y))              (tempered log-probability)
//   the token feeds step t + 1; all T steps run (no <end> handling, as in the greedy sampler).
//
// The noise of an element depends only on (key, global row, T, t, v): a row-sharded batch samples
// what the whole batch would, and the same arguments give the same bits.
//
// Step loop: aa_beam_decode's with one row per image -- k_lstm + k_atten (lstm_atten_launch), the
// exact fp32 logits of k_vexact, then k_sample_select (one workgroup per row, one pass over the row).
//
// Truncation (aa_sample_decode_ex / aa_sample_select; restated by tests/sample_trunc_oracle.py).  With
// m = max y and e_v = exp(y_v - m), per row and step:
//   top-k   S_k = { v : #{ w : y_w > y_v } < k }: a token stays unless at least k tokens are strictly
//           better, so the ties at the k-th value all stay (|S_k| may exceed k); k == 0 or k >= V: off.
//   top-p   on the distribution renormalised over S_k: Z_k = sum_{S_k} e_v, G(v) = sum_{w in S_k, y_w > y_v} e_w
//           (the mass strictly above v), S = { v in S_k : G(v) < p Z_k }, p = top_p as fp32, 0 < p <= 1;
//           p == 1 is off by rule (not by computation: an e_v that underflows cannot drop a token).
//   so      S = { v : y_v >= theta } for one threshold theta = min_{v in S} y_v; tie groups are kept or
//           dropped whole, and the arg-max of y is always in S.
//   token = argmax_{v in S} (y_v + g_v), ties to the smaller v, with the g_v of the untruncated decode (same
//           element counter: the noise of a column does not depend on S);
//   logp  = y_token - (m + log sum_{v in S} e_v)      (log-probability under the truncated distribution)
//   kept  = |S| and theta are optional outputs.
// With both truncations off the untouched k_sample_select runs: bit-identical to the plain decode.
// top_k = 1 at tau = 1 gives the greedy (exact-vocab) ids with logp == 0 exactly (log 1) and kept == 1.
// -0 and +0 compare equal (y is taken as x / tau + 0).
//
// How G < p Z_k is evaluated (k_sample_trunc): on fixed-point masses q_v = floor(e_v 2^40), e_v =
// expf(y_v - m) in fp32, summed as 64-bit integers (V <= 2^14, so every sum is below 2^54 and exact
// whatever the order of the adds).  p = M 2^-s exactly (M the 24-bit significand), and for integers
// G < M Z / 2^s  <=>  G < ceil(M Z / 2^s): the row's threshold Tq = ceil(M Z_k / 2^s) is one 128-bit
// integer product, and a token stays iff the integer G(v) < Tq.  No floating-point comparison of masses.
//
// num_samples = N rows per image (aa_sample_decode_ex): the encoder tail runs once for the B images, h0 /
// c0 / x_g are expanded to the R = B N rows (row b N + n) and the step loop runs R rows with kdiv = N,
// exactly as beam search shares an image's V among its beams; the selection's row origin is row0 N.  The
// result equals, bit for bit, the decode of images.repeat_interleave(N) with row0 N.
#include "aa_internal.hpp"

namespace aa {

constexpr int SAMPLE_VPT = BEAM_VPT;  // V <= 256 * 64, as beam_check

// g = -log(-log(u)) of element counter e.  u = (2 k23 + 1) / 2^24 with k23 the top 23 bits: 24
// significant bits, so the int -> float conversion and the scaling are exact, and 2^-24 <= u <=
// 1 - 2^-24 keeps both logs finite (|g| < 17).  Accurate logf (device library, no fast-math).
__device__ __forceinline__ float gumbel_noise(uint64_t key, uint64_t e) {
  const uint64_t z = splitmix(key + (e + 1) * GOLDEN);
  const uint32_t k23 = (uint32_t)(z >> 41);
  const float u = (float)(2u * k23 + 1u) * (1.0f / 16777216.0f);
  return -logf(-logf(u));
}

__global__ void k_synth_gumbel(float* __restrict__ dst, int64_t n, uint64_t key, int64_t start) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = gumbel_noise(key, (uint64_t)(start + i));
}

// One workgroup (256 threads) per row: thread j takes columns j + 256 i < V (coalesced; columns of the
// padded pitch Vp beyond V take no part) and keeps three scalars -- the best perturbed key (argmax_key:
// value, then the smaller column) and an online (max, sum exp(y - max)) pair of the unperturbed y --
// then the workgroup reduces them in a fixed order (wave butterflies, then the four waves in order):
// deterministic, and independent of the other rows.  No per-thread arrays indexed at run time: the
// columns go SEL_U at a time through fully unrolled loops, so the SEL_U loads are in flight together and
// the SEL_U independent noise chains (splitmix64, two logf: ~70 dependent instructions each) interleave;
// one element at a time, each iteration waited for its own load and ran the chain alone (27 us per
// launch at B = 512, V = 10,123: DESIGN.md section 15).  The running pair is rescaled once per SEL_U
// columns: one expf per column plus one per batch.
constexpr int SEL_U = 8;
__global__ __launch_bounds__(256) void k_sample_select(int V, int Vp, int T, int t, float tau, uint64_t key,
                                                       int64_t row0, const float* __restrict__ logits,
                                                       int64_t* __restrict__ tok, int64_t* __restrict__ ids,
                                                       float* __restrict__ logp) {
  __shared__ float red_m[4], red_s[4];
  __shared__ uint64_t red_k[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (int64_t)b * Vp;
  const uint64_t e0 = ((uint64_t)(row0 + b) * (uint64_t)T + (uint64_t)t) * (uint64_t)V;
  uint64_t best = 0;  // below every key of a real column (argmax_key's high word is never 0 for a finite value)
  float m = -INFINITY, s = 0.f;
  for (int c0 = tid; c0 < V; c0 += 256 * SEL_U) {
    float y[SEL_U];
#pragma unroll
    for (int j = 0; j < SEL_U; ++j) {
      const int col = c0 + 256 * j;
      y[j] = col < V ? x[col] : -INFINITY;
    }
    float mb = -INFINITY;
#pragma unroll
    for (int j = 0; j < SEL_U; ++j) {
      const int col = c0 + 256 * j;
      y[j] = y[j] / tau;  // -inf stays -inf
      mb = fmaxf(mb, y[j]);
      const uint64_t k =
          col < V ? argmax_key((y[j] + gumbel_noise(key, e0 + (uint64_t)col)) + 0.0f, col) : 0ull;
      best = k > best ? k : best;
    }
    // column c0 is real, so mn is finite; m = -inf (first batch): s = 0 * 0; a column past V adds expf(-inf) = 0
    const float mn = fmaxf(m, mb);
    s *= expf(m - mn);
#pragma unroll
    for (int j = 0; j < SEL_U; ++j) s += expf(y[j] - mn);
    m = mn;
  }
  // wave reduction, then the four waves' (key, max, sum) through LDS, combined in wave order
  best = wave_max_u64(best);
  const float mw = wave_max(m);
  // a thread without columns (V < 256) holds (m, s) = (-inf, 0): its term is 0
  const float sw = wave_sum(m == -INFINITY ? 0.f : s * expf(m - mw));
  if ((tid & 63) == 0) {
    red_k[tid >> 6] = best;
    red_m[tid >> 6] = mw;
    red_s[tid >> 6] = sw;
  }
  __syncthreads();
  if (tid == 0) {
    uint64_t kb = red_k[0];
    float M = red_m[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      kb = red_k[w] > kb ? red_k[w] : kb;
      M = fmaxf(M, red_m[w]);
    }
    float S = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) S += red_m[w] == -INFINITY ? 0.f : red_s[w] * expf(red_m[w] - M);  // V < 193: empty waves
    const int64_t c = key_token(kb);
    const float yc = x[c] / tau;  // the same division as in the loop: the same bits
    tok[b] = c;
    ids[(int64_t)b * T + t] = c;
    logp[(int64_t)b * T + t] = yc - (M + logf(S));
  }
}

// ---- truncated selection (top-k / top-p; semantics and the mass comparison in the head comment) ----
// One workgroup (512 threads) per row, independent of the other rows.  y = x / tau goes to LDS once (loads
// SEL_U at a time behind one wait, as k_sample_select); every later pass reads LDS.  The threshold theta is
// found by a multi-level histogram select.  A level puts every candidate column (lo <= key <= hi) into one
// of TR_NB bins holding (u32 count, u64 fixed-point mass, min key, max key), filled with integer LDS atomics
// -- integer add / min / max commute, so a histogram is exact and the same whatever the arrival order -- and
// wave 0 scans the bins in order for the first one where the target is reached; that bin's (min, max) keys
// are the next level's candidates.
//   level 0 bins by value, floor((m - y) TR_NB / (m - min y)): fp32 subtraction, multiplication by a
//     positive scale and the conversion are monotone, so a bin holds a contiguous range of y and every
//     column of a lower bin is strictly better than every column of a higher one.  (Binning by the top bits of
//     the key instead would put a row of logits around 0 into a handful of bins: the atomics of a wave
//     would serialise on one address.)
//   levels 1..: bins (hi - key) >> sh of the order-preserving u32 key, sh = bits(hi - lo) - 9.
//   A level whose bin holds one key (min == max) ends the search: that key is theta, its columns the tie group
//   at the threshold, kept whole.  Each key level shrinks bits(hi - lo) by 9: at most four of them.
// top-k selects on the counts (the first bin where the count of strictly better columns plus its own
// reaches k), top-p on the masses of the columns with key >= theta_k (the first bin where the mass strictly
// above plus its own reaches Tq).  The final pass takes sum e_v over S per thread in column order, then the
// waves in order (fixed order: the same bits every run), and the Gumbel arg-max over S only: when S fits
// the list (u16 columns in the histograms' LDS, or in the 64 KiB of ys beyond the row: V = 10,123 leaves room for
// every column) the kept columns are compacted -- the list's order
// varies, but a maximum of (value, column) keys does not depend on it -- and the ~70-instruction noise chain
// runs for |S| columns, TR_U chains interleaved; a larger S takes the untruncated kernel's pass with a
// predicate.  512 threads: at B = 512 a CU holds two rows (74 KiB of LDS each), and every pass is a chain of
// LDS round trips, so the two rows' sixteen waves (four per SIMD) are what hides them.  No per-thread
// array is indexed at run time; every loop's bound is a constant or V.
constexpr int TR_NT = 512, TR_NW = TR_NT / 64;
constexpr int TR_LOGNB = 9, TR_NB = 1 << TR_LOGNB, TR_BPL = TR_NB / 64;  // bins, bins per lane of the scan
constexpr int TR_VMAX = 256 * SAMPLE_VPT;      // y of one row in LDS: 64 KiB
constexpr int TR_HB = TR_NB * 20;              // histogram bytes: u64 mass, u32 count, u32 min key, u32 max key
constexpr int TR_LIST = TR_HB / 2;             // u16 columns in the histograms' LDS
constexpr int TR_LEVELS = 5;                   // the value level, then at most four key levels (32 bits, 9 per level)
constexpr int TR_U = 4;

// bin -> LDS slot: lane l of the scan owns bins 8 l .. 8 l + 7 and reads them at [i * 64 + l] (no bank conflict)
__device__ __forceinline__ int hist_slot(int bin) { return ((bin & (TR_BPL - 1)) << 6) | (bin / TR_BPL); }
__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int o) {
  const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}
// q_v = floor(exp(y - m) 2^40): y <= m, so q <= 2^40; the scaling by a power of two is exact
__device__ __forceinline__ uint64_t mass_q(float y, float m) { return (uint64_t)(expf(y - m) * 1099511627776.0f); }
// Tq = ceil(p Z) for p = M 2^-s exactly (0 < p <= 1: 23 <= s <= 149), Z >= 2^40: an integer G < p Z  <=>  G < Tq
__device__ __forceinline__ uint64_t mass_threshold(float p, uint64_t Z) {
  const uint32_t u = __float_as_uint(p), E = u >> 23;
  const uint32_t M = E ? ((u & 0x7FFFFFu) | 0x800000u) : (u & 0x7FFFFFu);
  const int s = E ? 150 - (int)E : 149;
  if (s >= 100) return 1;  // M Z < 2^78: the quotient is in (0, 1)
  const unsigned __int128 one = 1;
  return (uint64_t)(((unsigned __int128)M * Z + ((one << s) - 1)) >> s);
}
__device__ __forceinline__ int value_bin(float y, float m, float scale) {
  return (int)fminf(fmaxf((m - y) * scale, 0.f), (float)(TR_NB - 1));  // (a NaN product goes to bin 0)
}

__global__ __launch_bounds__(TR_NT) void k_sample_trunc(int V, int Vp, int T, int t, float tau, uint64_t key,
                                                        int64_t row0, int top_k, float top_p,
                                                        const float* __restrict__ logits, int64_t* __restrict__ tok,
                                                        int64_t* __restrict__ ids, float* __restrict__ logp,
                                                        int32_t* __restrict__ kept_out, float* __restrict__ theta_out) {
  __shared__ float ys[TR_VMAX];
  __shared__ uint64_t hbuf[TR_HB / 8];
  __shared__ float red_f[2 * TR_NW];
  __shared__ uint64_t red_k[TR_NW];
  __shared__ uint32_t s_lo, s_hi, s_acnt, s_cin, s_n;
  __shared__ uint64_t s_amass;
  uint64_t* hm = hbuf;                                          // masses, counts, min keys, max keys
  uint32_t* hc = reinterpret_cast<uint32_t*>(hbuf + TR_NB);
  uint32_t* hlo = hc + TR_NB;
  uint32_t* hhi = hlo + TR_NB;
  // the final pass's kept columns: in the part of ys beyond the row when that holds more than the histograms' LDS
  const int V4 = (V + 3) & ~3, tail = (TR_VMAX - V4) * 2;
  uint16_t* list = tail > TR_LIST ? reinterpret_cast<uint16_t*>(ys + V4) : reinterpret_cast<uint16_t*>(hbuf);
  const uint32_t cap = tail > TR_LIST ? (uint32_t)tail : (uint32_t)TR_LIST;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* x = logits + (int64_t)b * Vp;

  // y to LDS, max and min
  float m = -INFINITY, mn = INFINITY;
  for (int c0 = tid; c0 < V; c0 += TR_NT * SEL_U) {
    float y[SEL_U];
#pragma unroll
    for (int j = 0; j < SEL_U; ++j) {
      const int col = c0 + TR_NT * j;
      y[j] = col < V ? x[col] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < SEL_U; ++j) {
      const int col = c0 + TR_NT * j;
      if (col < V) {
        const float v = y[j] / tau + 0.0f;  // the untruncated kernel's division; -0 becomes +0
        ys[col] = v;
        m = fmaxf(m, v);
        mn = fminf(mn, v);
      }
    }
  }
  m = wave_max(m);
  mn = -wave_max(-mn);
  if (lane == 0) {
    red_f[wv] = m;  // a wave without columns holds (-inf, +inf)
    red_f[TR_NW + wv] = mn;
  }
  __syncthreads();
  m = red_f[0];
  mn = red_f[TR_NW];
#pragma unroll
  for (int w = 1; w < TR_NW; ++w) {
    m = fmaxf(m, red_f[w]);
    mn = fminf(mn, red_f[TR_NW + w]);
  }
  const float span = m - mn;
  const float scale = span > 0.f ? fminf((float)TR_NB / span, 1e30f) : 0.f;  // all equal: one bin

  // The threshold among the columns with key >= floor_key: on counts (target = k) or on masses (target = Tq,
  // worked out from the level-0 histogram's total).  Every branch below is workgroup-uniform.
  auto select = [&](const bool mass, const uint32_t floor_key, uint64_t target, uint32_t& th, uint32_t& kept) {
    uint32_t lo = floor_key, hi = 0xFFFFFFFFu, acnt = 0;  // candidates: lo <= key <= hi; acnt / amass: strictly above hi
    uint64_t amass = 0;
    int sh = -1;  // -1: the value level
    for (int lvl = 0; lvl < TR_LEVELS; ++lvl) {
      for (int i = tid; i < TR_NB; i += TR_NT) {
        hm[i] = 0;
        hc[i] = 0;
        hlo[i] = 0xFFFFFFFFu;
        hhi[i] = 0;
      }
      __syncthreads();
#pragma unroll 4
      for (int col = tid; col < V; col += TR_NT) {
        const float y = ys[col];
        const uint32_t k = order_key(y);
        if (k >= lo && k <= hi) {
          const int bin = sh < 0 ? value_bin(y, m, scale) : (int)min((hi - k) >> sh, (uint32_t)(TR_NB - 1));
          const int sl = hist_slot(bin);
          atomicAdd(&hc[sl], 1u);
          atomicMin(&hlo[sl], k);
          atomicMax(&hhi[sl], k);
          if (mass) atomicAdd(reinterpret_cast<unsigned long long*>(&hm[sl]), (unsigned long long)mass_q(y, m));
        }
      }
      __syncthreads();
      if (wv == 0) {  // scan in bin order: the first bin whose inclusive count / mass reaches the target
        uint32_t c[TR_BPL], tc = 0;
        uint64_t q[TR_BPL], tq = 0;
#pragma unroll
        for (int i = 0; i < TR_BPL; ++i) {
          c[i] = hc[i * 64 + lane];
          q[i] = mass ? hm[i * 64 + lane] : 0ull;
          tc += c[i];
          tq += q[i];
        }
        uint32_t pc = tc;
        uint64_t pq = tq;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t xc = __shfl_up(pc, o, 64);
          const uint64_t xq = shfl_up_u64(pq, o);
          if (lane >= o) {
            pc += xc;
            pq += xq;
          }
        }
        if (mass && lvl == 0) target = mass_threshold(top_p, shfl_u64(pq, 63));  // Z_k: the candidates' whole mass
        uint32_t rc = acnt + (pc - tc), fa = 0, fc = 0;
        uint64_t rq = amass + (pq - tq), fq = 0;
        int fi = -1;
#pragma unroll
        for (int i = 0; i < TR_BPL; ++i) {
          const uint32_t nc = rc + c[i];
          const uint64_t nq = rq + q[i];
          const bool cross = mass ? nq >= target : (uint64_t)nc >= target;
          if (fi < 0 && cross) {
            fi = i;
            fa = rc;
            fq = rq;
            fc = c[i];
          }
          rc = nc;
          rq = nq;
        }
        const uint64_t bal = __ballot(fi >= 0);  // (a target within the candidates' total is always reached)
        const int win = bal ? __ffsll((unsigned long long)bal) - 1 : 63;
        if (lane == win) {
          const int sl = (fi >= 0 ? fi : TR_BPL - 1) * 64 + lane;
          s_lo = hlo[sl];  // the bin's own key range: the next level's candidates
          s_hi = hhi[sl];
          s_acnt = fa;
          s_amass = fq;
          s_cin = fc;
        }
      }
      __syncthreads();
      lo = s_lo;
      hi = s_hi;
      acnt = s_acnt;
      amass = s_amass;
      if (lo >= hi) {  // one key: the tie group at the threshold, kept whole (lo > hi: an empty bin, not reached)
        th = hi;
        kept = acnt + s_cin;
        return;
      }
      sh = max(32 - __clz((int)(hi - lo)) - TR_LOGNB, 0);
    }
    th = hi;  // not reached: the fourth key level has sh == 0, so its bins are single keys
    kept = acnt;
  };

  uint32_t th = 0, kept = (uint32_t)V;
  if (top_k > 0 && top_k < V) select(false, 0u, (uint64_t)top_k, th, kept);
  if (top_p < 1.0f) select(true, th, 0ull, th, kept);

  // S = { key >= th }: sum e_v in a fixed order, Gumbel arg-max over S
  const uint64_t e0 = ((uint64_t)(row0 + b) * (uint64_t)T + (uint64_t)t) * (uint64_t)V;
  uint64_t best = 0;
  float s = 0.f;
  if (kept <= cap) {
    if (tid == 0) s_n = 0;
    __syncthreads();  // (also: the last scan's reads of the histograms are done)
#pragma unroll 4
    for (int col = tid; col < V; col += TR_NT) {
      const float y = ys[col];
      if (order_key(y) >= th) {
        s += expf(y - m);
        const uint32_t i = atomicAdd(&s_n, 1u);
        if (i < cap) list[i] = (uint16_t)col;
      }
    }
    __syncthreads();
    const int n = (int)min(s_n, cap);
    for (int i0 = tid; i0 < n; i0 += TR_NT * TR_U) {
#pragma unroll
      for (int j = 0; j < TR_U; ++j) {
        const int i = i0 + TR_NT * j;
        const int col = i < n ? (int)list[i] : 0;
        const uint64_t k = argmax_key((ys[col] + gumbel_noise(key, e0 + (uint64_t)col)) + 0.0f, col);
        best = (i < n && k > best) ? k : best;
      }
    }
  } else {
    for (int c0 = tid; c0 < V; c0 += TR_NT * SEL_U) {
#pragma unroll
      for (int j = 0; j < SEL_U; ++j) {
        const int col = c0 + TR_NT * j;
        const float y = ys[col < V ? col : c0];
        const bool in = col < V && order_key(y) >= th;
        s += in ? expf(y - m) : 0.f;
        const uint64_t k = argmax_key((y + gumbel_noise(key, e0 + (uint64_t)col)) + 0.0f, col);
        best = (in && k > best) ? k : best;
      }
    }
  }
  best = wave_max_u64(best);
  s = wave_sum(s);
  __syncthreads();  // red_f's first use is long over; this keeps the rule one sync between uses
  if (lane == 0) {
    red_k[wv] = best;
    red_f[wv] = s;
  }
  __syncthreads();
  if (tid == 0) {
    uint64_t kb = red_k[0];
    float S = red_f[0];
#pragma unroll
    for (int w = 1; w < TR_NW; ++w) {
      kb = red_k[w] > kb ? red_k[w] : kb;
      S += red_f[w];
    }
    int64_t c = key_token(kb);
    c = c < V ? c : 0;  // (kb == 0: no column was kept -- only a row of NaNs gets here; stay inside ys)
    tok[b] = c;
    ids[(int64_t)b * T + t] = c;
    logp[(int64_t)b * T + t] = ys[c] - (m + logf(S));  // kept == 1: S == 1, logf(1) == 0, ys[c] == m: exactly 0
    if (kept_out) kept_out[(int64_t)b * T + t] = (int32_t)kept;
    if (theta_out) theta_out[(int64_t)b * T + t] = key_value(th);
  }
}

// kept / theta of an untruncated draw (S is the whole row): V and min y
__global__ __launch_bounds__(256) void k_sample_kept_all(int V, int Vp, int T, int t, float tau,
                                                         const float* __restrict__ logits,
                                                         int32_t* __restrict__ kept_out, float* __restrict__ theta_out) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (int64_t)b * Vp;
  float mn = INFINITY;
  for (int col = tid; col < V; col += 256) mn = fminf(mn, x[col] / tau + 0.0f);
  mn = -wave_max(-mn);
  if ((tid & 63) == 0) red[tid >> 6] = mn;
  __syncthreads();
  if (tid == 0) {
    if (kept_out) kept_out[(int64_t)b * T + t] = V;
    if (theta_out) theta_out[(int64_t)b * T + t] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  }
}

// one step's selection over R rows: the untouched k_sample_select when both truncations are off
static void select_launch(int R, int V, int Vp, int T, int t, float tau, uint64_t key, int64_t row_origin, int top_k,
                          float top_p, const float* logits, int64_t* tok, int64_t* ids, float* logp, int32_t* kept,
                          float* theta, aa_event_t* ev, hipStream_t s) {
  const bool trunc = (top_k > 0 && top_k < V) || top_p < 1.0f;
  if (trunc) {
    AA_TLAUNCH(ev, 2 * t, k_sample_trunc, dim3(R), dim3(TR_NT), 0, s, V, Vp, T, t, tau, key, row_origin, top_k, top_p,
               logits, tok, ids, logp, kept, theta);
    return;
  }
  AA_TLAUNCH(ev, 2 * t, k_sample_select, dim3(R), dim3(256), 0, s, V, Vp, T, t, tau, key, row_origin, logits, tok, ids,
             logp);
  if (kept || theta)
    hipLaunchKernelGGL(k_sample_kept_all, dim3(R), dim3(256), 0, s, V, Vp, T, t, tau, logits, kept, theta);
}

struct SampleWS {
  EncWS e;    // of the B images
  RowWS r;    // of the R = B N rows
  float* xg1; // N > 1: the images' x_g, expanded to the rows' r.xg
  float* logits;
  float2* gsum;
  int64_t *tok0, *tok;
};
static SampleWS carve_sample(char* base, const Layout& L, int B, int N, size_t* bytes) {
  Carver c{base};
  SampleWS w;
  const size_t R = (size_t)B * N;
  w.e = carve_enc(c, L, B);
  w.xg1 = N > 1 ? c.take<float>((size_t)B * L.N5) : nullptr;
  w.r = carve_rows(c, L, R);
  w.logits = c.take<float>(R * L.Vp);
  w.gsum = c.take<float2>(R * (L.Vp / 32));  // k_vexact's granule summaries (written, not read here)
  w.tok0 = c.take<int64_t>(R);
  w.tok = c.take<int64_t>(R);
  *bytes = c.off;
  return w;
}

static int sample_check(const aa_dims* d, int B, int T) {
  if (!d) return AA_ERR_NULL;
  if (aa_check_dims(d) != AA_OK) return AA_ERR_DIMS;
  if (d->vocab > 256 * SAMPLE_VPT) return AA_ERR_DIMS;
  if (B < 0 || T < 0 || B > (1 << 24)) return AA_ERR_SHAPE;
  return AA_OK;
}

}  // namespace aa

using namespace aa;

static bool opts_ok(int32_t top_k, float top_p, int32_t N) {
  return top_k >= 0 && top_p > 0.f && top_p <= 1.f && N >= 1;  // (a NaN top_p fails both comparisons)
}

size_t aa_sample_workspace_bytes(const aa_dims* d, int32_t B, int32_t T) {
  return aa_sample_workspace_bytes_ex(d, B, T, 1);
}

size_t aa_sample_workspace_bytes_ex(const aa_dims* d, int32_t B, int32_t T, int32_t N) {
  if (sample_check(d, B, T) != AA_OK) return 0;
  if (N < 1 || (int64_t)B * N > (int64_t)1 << 24) return 0;
  if (B == 0 || T == 0) return 0;
  size_t n;
  carve_sample(nullptr, make_layout(*d), B, N, &n);
  return n;
}

int aa_sample_decode(const aa_model* m, const float* feats, int32_t B, int32_t T, float temperature, uint64_t key,
                     int64_t row0, int64_t* ids, float* logp, float* alpha, float* beta, void* workspace,
                     size_t workspace_bytes, int32_t flags, aa_stream_t stream, aa_event_t* select_events) {
  return aa_sample_decode_ex(m, feats, B, T, temperature, key, row0, ids, logp, alpha, beta, workspace, workspace_bytes,
                             flags, stream, select_events, nullptr);
}

int aa_sample_decode_ex(const aa_model* m, const float* feats, int32_t B, int32_t T, float temperature, uint64_t key,
                        int64_t row0, int64_t* ids, float* logp, float* alpha, float* beta, void* workspace,
                        size_t workspace_bytes, int32_t flags, aa_stream_t stream, aa_event_t* select_events,
                        const aa_sample_opts* opts) {
  Layout L;
  int rc = check_model(m, &L);
  if (rc) return rc;
  rc = sample_check(&m->dims, B, T);
  if (rc) return rc;
  // !(tau > 0) also rejects NaN; the upper bound rejects +inf
  if (!(temperature > 0.f) || !(temperature <= 3.402823466e38f)) return AA_ERR_SHAPE;
  if (row0 < 0) return AA_ERR_SHAPE;
  if (flags & ~AA_DECODE_FP32_ENCODER) return AA_ERR_SHAPE;  // AA_DECODE_BASELINE too: no no-sentinel kernels here
  const int32_t top_k = opts ? opts->top_k : 0, N = opts ? opts->num_samples : 1;
  const float top_p = opts ? opts->top_p : 1.0f;
  if (!opts_ok(top_k, top_p, N)) return AA_ERR_SHAPE;
  if ((int64_t)B * N > (int64_t)1 << 24) return AA_ERR_SHAPE;
  if (B == 0 || T == 0) return AA_OK;
  // the element counters (row0 + B) N T V stay inside 62 bits: no wrap-around, and start + n fits int64
  // (two divisions: N T V itself may pass 64 bits)
  if ((uint64_t)row0 + (uint64_t)B > ((uint64_t)1 << 62) / ((uint64_t)T * (uint64_t)L.V) / (uint64_t)N)
    return AA_ERR_SHAPE;
  if (!feats || !ids || !logp || !workspace) return AA_ERR_NULL;
  if (!al16(feats) || !al16(workspace)) return AA_ERR_ALIGN;
  size_t need;
  SampleWS w = carve_sample(static_cast<char*>(workspace), L, B, N, &need);
  if (workspace_bytes < need) return AA_ERR_BUFFER;
  hipStream_t s = (hipStream_t)stream;
  const MP p = resolve(m, L);
  const EncWS& e = w.e;
  const RowWS& r = w.r;
  const int R = B * N;
  if (N == 1) {
    rc = encoder_launch(L, p, feats, B, e.a_g, e.V, e.vg, r.h[0], r.c[0], e.vwv, r.xg, nullptr, flags, s);
    if (rc) return rc;
  } else {  // the encoder tail once for the B images; h0 / c0 / x_g expanded to the R rows (as aa_beam_decode)
    rc = encoder_launch(L, p, feats, B, e.a_g, e.V, e.vg, r.h[1], r.c[1], e.vwv, w.xg1, nullptr, flags, s);
    if (rc) return rc;
    expand_rows_launch(r.h[1], B, N, L.H, r.h[0], s);
    expand_rows_launch(r.c[1], B, N, L.H, r.c[0], s);
    expand_rows_launch(w.xg1, B, N, L.N5, r.xg, s);
  }
  split_rows_launch(r.h[0], R, L.H, r.hsp[0], s);
  fill_tok_launch(w.tok0, R, 1, s);  // <start>
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    // alpha / beta straight to the outputs, with the greedy decode's leading dimensions; every row carries
    // its own state (no gather), an image's N rows share its V / VWv (kdiv)
    lstm_atten_launch(L, p,
                      {.B = R, .tok = t ? w.tok : w.tok0, .V = e.V, .vwv = e.vwv, .xg = r.xg, .hsp_in = r.hsp[cur],
                       .c_in = r.c[cur], .h_out = r.h[nxt], .hsp_out = r.hsp[nxt], .c_out = r.c[nxt], .s = r.s,
                       .part = r.part, .u = r.u, .alpha = alpha ? alpha + (size_t)t * P : nullptr,
                       .alpha_ld = (int64_t)T * P, .beta = beta ? beta + t : nullptr, .beta_ld = T, .kdiv = N,
                       .ei = 2 * t},
                      s);
    vexact_launch(L, p, R, r.u, w.logits, w.gsum, s);
    select_launch(R, L.V, L.Vp, T, t, temperature, key, row0 * N, top_k, top_p, w.logits, w.tok, ids, logp,
                  opts ? opts->kept : nullptr, opts ? opts->theta : nullptr, select_events, s);
  }
  return launch_status();
}

int aa_sample_select(const float* logits, int32_t R, int32_t V, int32_t Vp, int32_t T, int32_t t, float temperature,
                     uint64_t key, int64_t row0, int32_t top_k, float top_p, int64_t* tok, int64_t* ids, float* logp,
                     int32_t* kept, float* theta, aa_stream_t stream) {
  if (R < 0 || R > (1 << 24) || V < 1 || V > 256 * SAMPLE_VPT || Vp < V || T < 1 || t < 0 || t >= T) return AA_ERR_SHAPE;
  if (!(temperature > 0.f) || !(temperature <= 3.402823466e38f)) return AA_ERR_SHAPE;
  if (row0 < 0 || !opts_ok(top_k, top_p, 1)) return AA_ERR_SHAPE;
  if (R == 0) return AA_OK;
  if ((uint64_t)row0 + (uint64_t)R > ((uint64_t)1 << 62) / ((uint64_t)T * (uint64_t)V)) return AA_ERR_SHAPE;
  if (!logits || !tok || !ids || !logp) return AA_ERR_NULL;
  select_launch(R, V, Vp, T, t, temperature, key, row0, top_k, top_p, logits, tok, ids, logp, kept, theta, nullptr,
                (hipStream_t)stream);
  return launch_status();
}

int aa_synth_gumbel(float* dst, int64_t n, uint64_t key, int64_t start, aa_stream_t stream) {
  if (n < 0 || start < 0) return AA_ERR_SHAPE;
  if (n == 0) return AA_OK;
  if (!dst) return AA_ERR_NULL;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_synth_gumbel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     (hipStream_t)stream, dst, n, key, start);
  return launch_status();
}
