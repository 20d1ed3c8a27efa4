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

struct SampleWS {
  EncWS e;
  RowWS r;
  float* logits;
  float2* gsum;
  int64_t *tok0, *tok;
};
static SampleWS carve_sample(char* base, const Layout& L, int B, size_t* bytes) {
  Carver c{base};
  SampleWS w;
  const size_t R = (size_t)B;
  w.e = carve_enc(c, L, R);
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

size_t aa_sample_workspace_bytes(const aa_dims* d, int32_t B, int32_t T) {
  if (sample_check(d, B, T) != AA_OK) return 0;
  if (B == 0 || T == 0) return 0;
  size_t n;
  carve_sample(nullptr, make_layout(*d), B, &n);
  return n;
}

int aa_sample_decode(const aa_model* m, const float* feats, int32_t B, int32_t T, float temperature, uint64_t key,
                     int64_t row0, int64_t* ids, float* logp, float* alpha, float* beta, void* workspace,
                     size_t workspace_bytes, int32_t flags, aa_stream_t stream, aa_event_t* select_events) {
  Layout L;
  int rc = check_model(m, &L);
  if (rc) return rc;
  rc = sample_check(&m->dims, B, T);
  if (rc) return rc;
  // !(tau > 0) also rejects NaN; the upper bound rejects +inf
  if (!(temperature > 0.f) || !(temperature <= 3.402823466e38f)) return AA_ERR_SHAPE;
  if (row0 < 0) return AA_ERR_SHAPE;
  if (flags & ~AA_DECODE_FP32_ENCODER) return AA_ERR_SHAPE;  // AA_DECODE_BASELINE too: no no-sentinel kernels here
  if (B == 0 || T == 0) return AA_OK;
  // the element counters (row0 + B) T V stay inside 62 bits: no wrap-around, and start + n fits int64
  if ((uint64_t)row0 + (uint64_t)B > ((uint64_t)1 << 62) / ((uint64_t)T * (uint64_t)L.V)) return AA_ERR_SHAPE;
  if (!feats || !ids || !logp || !workspace) return AA_ERR_NULL;
  if (!al16(feats) || !al16(workspace)) return AA_ERR_ALIGN;
  size_t need;
  SampleWS w = carve_sample(static_cast<char*>(workspace), L, B, &need);
  if (workspace_bytes < need) return AA_ERR_BUFFER;
  hipStream_t s = (hipStream_t)stream;
  const MP p = resolve(m, L);
  const EncWS& e = w.e;
  const RowWS& r = w.r;
  rc = encoder_launch(L, p, feats, B, e.a_g, e.V, e.vg, r.h[0], r.c[0], e.vwv, r.xg, nullptr, flags, s);
  if (rc) return rc;
  split_rows_launch(r.h[0], B, L.H, r.hsp[0], s);
  fill_tok_launch(w.tok0, B, 1, s);  // <start>
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    // alpha / beta straight to the outputs, with the greedy decode's leading dimensions
    lstm_atten_launch(L, p,
                      {.B = B, .tok = t ? w.tok : w.tok0, .V = e.V, .vwv = e.vwv, .xg = r.xg, .hsp_in = r.hsp[cur],
                       .c_in = r.c[cur], .h_out = r.h[nxt], .hsp_out = r.hsp[nxt], .c_out = r.c[nxt], .s = r.s,
                       .part = r.part, .u = r.u, .alpha = alpha ? alpha + (size_t)t * P : nullptr,
                       .alpha_ld = (int64_t)T * P, .beta = beta ? beta + t : nullptr, .beta_ld = T, .ei = 2 * t},
                      s);
    vexact_launch(L, p, B, r.u, w.logits, w.gsum, s);
    AA_TLAUNCH(select_events, 2 * t, k_sample_select, dim3(B), dim3(256), 0, s, L.V, L.Vp, T, t, temperature, key, row0,
               (const float*)w.logits, w.tok, ids, logp);
  }
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
