// aa_optim.hip — the two pieces of train.py's closure that sit around the teacher-forced
// forward/backward (code_src/train.py:197-219): the CrossEntropyLoss on the packed scores and the
// Adam step over every parameter.  Both are HBM-bound elementwise passes, so each is ONE launch
// per call (Adam: every parameter tensor in one grid; cross entropy: one read of the scores
// forward, one read + one write backward) instead of PyTorch's per-op kernel chains.  Beside the
// cross entropy, its policy-gradient sibling for self-critical training (aa_policy_loss_*).
//
// Its own translation unit (linked into libadaptive_amd.so beside aa_kernels.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "adaptive_amd.h"

namespace aa_optim {

__global__ __launch_bounds__(256) void k_read_probe(const float4* __restrict__ src, int64_t n, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  float acc = 0.f;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 7 * stride < n; i += 8 * stride) {
    float4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = src[i + k * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += (v[k].x + v[k].y) + (v[k].z + v[k].w);
  }
  for (; i < n; i += stride) {
    const float4 v = src[i];
    acc += (v.x + v.y) + (v.z + v.w);
  }
  __shared__ float red[4];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- Adam (torch.optim.Adam, amsgrad=False, maximize=False; model_factory.py:71 builds it) -------------
// One workgroup = ADAM_CHUNK consecutive elements of one tensor.  The per-tensor table travels in
// the kernel arguments (no upload, no allocation).
constexpr int ADAM_THREADS = 256;
constexpr int ADAM_VEC = 4;                                  // float4 per thread per round
constexpr int ADAM_ROUNDS = 4;                               // rounds per workgroup
constexpr int ADAM_CHUNK = ADAM_THREADS * ADAM_VEC * ADAM_ROUNDS;  // 4096 elements

struct AdamArgs {
  int n;                                  // tensors in this launch (<= AA_ADAM_MAX_TENSORS)
  int aligned;                            // bit i: tensor i's four pointers are 16-byte aligned
  int64_t blk0[AA_ADAM_MAX_TENSORS + 1];  // first workgroup of tensor i (prefix sum)
  int64_t numel[AA_ADAM_MAX_TENSORS];
  float* p[AA_ADAM_MAX_TENSORS];
  const float* g[AA_ADAM_MAX_TENSORS];
  float* m[AA_ADAM_MAX_TENSORS];
  float* v[AA_ADAM_MAX_TENSORS];
  float w1;         // 1 - beta1 (lerp weight)
  float beta2;
  float omb2;       // 1 - beta2
  float bc2_sqrt;   // sqrt(1 - beta2^step)
  float step_size;  // -lr / (1 - beta1^step)
  float eps;
  float wd;         // L2 weight decay (added to the gradient, as torch's Adam does)
};

// torch's foreach Adam, element by element, in its op order (optim/adam.py _multi_tensor_adam):
// g' = g + wd p; m = lerp(m, g', 1-b1); v = v*b2; v = v + (1-b2)*(g'*g'); d = sqrt(v)/bc2s + eps;
// p = p + step_size*(m/d).  lerp as ATen's (Lerp.h): |w| < 0.5 ? a + w(b-a) : b - (b-a)(1-w).
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamArgs& a) {
  if (a.wd != 0.f) g = g + a.wd * p;
  m = (fabsf(a.w1) < 0.5f) ? m + a.w1 * (g - m) : g - (g - m) * (1.f - a.w1);
  v = v * a.beta2;
  v = v + a.omb2 * (g * g);
  const float d = sqrtf(v) / a.bc2_sqrt + a.eps;
  p = p + a.step_size * (m / d);
}

__global__ __launch_bounds__(ADAM_THREADS) void k_adam(AdamArgs a) {
  const int64_t blk = blockIdx.x;
  int t = 0;
  while (t + 1 < a.n && blk >= a.blk0[t + 1]) ++t;  // <= 24 scalar compares
  const int64_t base = (blk - a.blk0[t]) * ADAM_CHUNK;
  const int64_t n = a.numel[t];
  float* __restrict__ P = a.p[t];
  const float* __restrict__ G = a.g[t];
  float* __restrict__ M = a.m[t];
  float* __restrict__ Vv = a.v[t];
  if (((a.aligned >> t) & 1) && base + ADAM_CHUNK <= n) {
    // full chunk, vector path: every load of the chunk issued before the arithmetic
    float4 p4[ADAM_ROUNDS], g4[ADAM_ROUNDS], m4[ADAM_ROUNDS], v4[ADAM_ROUNDS];
#pragma unroll
    for (int r = 0; r < ADAM_ROUNDS; ++r) {
      const int64_t i = base + ((int64_t)r * ADAM_THREADS + threadIdx.x) * ADAM_VEC;
      p4[r] = *reinterpret_cast<const float4*>(P + i);
      g4[r] = *reinterpret_cast<const float4*>(G + i);
      m4[r] = *reinterpret_cast<const float4*>(M + i);
      v4[r] = *reinterpret_cast<const float4*>(Vv + i);
    }
#pragma unroll
    for (int r = 0; r < ADAM_ROUNDS; ++r) {
      adam_elem(p4[r].x, g4[r].x, m4[r].x, v4[r].x, a);
      adam_elem(p4[r].y, g4[r].y, m4[r].y, v4[r].y, a);
      adam_elem(p4[r].z, g4[r].z, m4[r].z, v4[r].z, a);
      adam_elem(p4[r].w, g4[r].w, m4[r].w, v4[r].w, a);
      const int64_t i = base + ((int64_t)r * ADAM_THREADS + threadIdx.x) * ADAM_VEC;
      *reinterpret_cast<float4*>(P + i) = p4[r];
      *reinterpret_cast<float4*>(M + i) = m4[r];
      *reinterpret_cast<float4*>(Vv + i) = v4[r];
    }
  } else {
    // tail chunk or unaligned tensor: scalar, coalesced
    const int64_t end = base + ADAM_CHUNK < n ? base + ADAM_CHUNK : n;
    for (int64_t i = base + threadIdx.x; i < end; i += ADAM_THREADS) {
      float p = P[i], m = M[i], v = Vv[i];
      adam_elem(p, G[i], m, v, a);
      P[i] = p;
      M[i] = m;
      Vv[i] = v;
    }
  }
}

// ---- cross entropy (nn.CrossEntropyLoss(), reduction mean; train.py:63,208) -------------------
// Forward: one workgroup per row: lse_i = log sum_j exp(x_ij) (one read of the row: in registers for
// rows up to 12288 scores, an online max / sum beyond), loss_i = lse_i - x_i[t_i] (0 for ignored rows); then one workgroup sums loss_i in a fixed
// order and divides by the number of counted rows.  Backward: dx_ij = (exp(x_ij - lse_i) - [j ==
// t_i]) * dloss / count (0 for ignored rows): one read and one write of the scores.
constexpr int CE_THREADS = 256;

__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  if (m2 > m) {
    s = s * expf(m - m2) + s2;
    m = m2;
  } else if (m2 != -INFINITY) {
    s = s + s2 * expf(m2 - m);
  }
}

__global__ __launch_bounds__(CE_THREADS) void k_ce_rows(const float* __restrict__ x, int64_t ldx, int V,
                                                        const int64_t* __restrict__ tgt, int64_t ignore,
                                                        float* __restrict__ lse_out, float* __restrict__ loss_out,
                                                        int* __restrict__ valid_out) {
  const int row = blockIdx.x;
  const float* __restrict__ xr = x + (int64_t)row * ldx;
  float m = -INFINITY, s = 0.f;
  int j = threadIdx.x;
  // eight independent loads in flight per lane, then the online update
  for (; j + 7 * CE_THREADS < V; j += 8 * CE_THREADS) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = xr[j + k * CE_THREADS];
#pragma unroll
    for (int k = 0; k < 8; ++k) lse_merge(m, s, v[k], 1.f);
  }
  for (; j < V; j += CE_THREADS) lse_merge(m, s, xr[j], 1.f);
  // wave butterfly, then across the four waves through LDS (fixed order: deterministic)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float m2 = __shfl_xor(m, off), s2 = __shfl_xor(s, off);
    lse_merge(m, s, m2, s2);
  }
  __shared__ float sm[CE_THREADS / 64], ss[CE_THREADS / 64];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[w] = m;
    ss[w] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0];
    for (int k = 1; k < CE_THREADS / 64; ++k) lse_merge(M, S, sm[k], ss[k]);
    const float lse = M + logf(S);
    const int64_t t = tgt[row];
    float loss;
    int valid = 1;
    if (t == ignore) {
      loss = 0.f;
      valid = 0;
    } else if (t < 0 || t >= V) {
      loss = NAN;  // out-of-range class index: poison the loss (torch raises a device assert)
    } else {
      loss = lse - xr[t];
    }
    lse_out[row] = lse;
    loss_out[row] = loss;
    valid_out[row] = valid;
  }
}

// Rows of up to CE_THREADS * CE_NPT scores: the row is held in registers (every load of the row in
// flight at once), then max and sum exp(x - max) as two fixed-order block reductions: one exp per
// score and no data-dependent branch (the online loop above pays a compare and branch per score).
constexpr int CE_NPT = 48;

__device__ __forceinline__ float block_reduce(float x, bool is_max, float* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float o = __shfl_xor(x, off);
    x = is_max ? fmaxf(x, o) : x + o;
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = x;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int k = 1; k < CE_THREADS / 64; ++k) r = is_max ? fmaxf(r, red[k]) : r + red[k];
  __syncthreads();  // red is reused by the next reduction
  return r;
}

__global__ __launch_bounds__(CE_THREADS) void k_ce_rows_reg(const float* __restrict__ x, int64_t ldx, int V,
                                                            const int64_t* __restrict__ tgt, int64_t ignore,
                                                            float* __restrict__ lse_out, float* __restrict__ loss_out,
                                                            int* __restrict__ valid_out) {
  const int row = blockIdx.x;
  const float* __restrict__ xr = x + (int64_t)row * ldx;
  __shared__ float red[CE_THREADS / 64];
  float v[CE_NPT];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < CE_NPT; ++k) {
    const int j = threadIdx.x + k * CE_THREADS;
    v[k] = j < V ? xr[j] : -INFINITY;
  }
#pragma unroll
  for (int k = 0; k < CE_NPT; ++k) m = fmaxf(m, v[k]);
  const float M = block_reduce(m, true, red);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < CE_NPT; ++k)
    if (threadIdx.x + k * CE_THREADS < V) s += expf(v[k] - M);
  const float S = block_reduce(s, false, red);
  if (threadIdx.x == 0) {
    const float lse = M + logf(S);
    const int64_t t = tgt[row];
    float loss;
    int valid = 1;
    if (t == ignore) {
      loss = 0.f;
      valid = 0;
    } else if (t < 0 || t >= V) {
      loss = NAN;
    } else {
      loss = lse - xr[t];
    }
    lse_out[row] = lse;
    loss_out[row] = loss;
    valid_out[row] = valid;
  }
}

__global__ __launch_bounds__(1024) void k_ce_reduce(const float* __restrict__ loss_rows,
                                                    const int* __restrict__ valid_rows, int N,
                                                    float* __restrict__ loss, float* __restrict__ count) {
  float s = 0.f;
  int c = 0;
  for (int i = threadIdx.x; i < N; i += 1024) {
    s += loss_rows[i];
    c += valid_rows[i];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_xor(s, off);
    c += __shfl_xor(c, off);
  }
  __shared__ float ws[16];
  __shared__ int wc[16];
  if ((threadIdx.x & 63) == 0) {
    ws[threadIdx.x >> 6] = s;
    wc[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float S = 0.f;
    int C = 0;
    for (int k = 0; k < 16; ++k) {
      S += ws[k];
      C += wc[k];
    }
    count[0] = (float)C;
    loss[0] = S / (float)C;
  }
}

// x and dx may alias (dlogits in place of logits, lddx == ldx): every element is read by the thread
// that writes it, before the write, so neither pointer is __restrict__
__global__ __launch_bounds__(CE_THREADS) void k_ce_bwd(const float* x, int64_t ldx, int V,
                                                       const int64_t* __restrict__ tgt, int64_t ignore,
                                                       const float* __restrict__ lse, const float* __restrict__ dloss,
                                                       const float* __restrict__ count, float* dx, int64_t lddx) {
  const int row = blockIdx.x;
  const float* xr = x + (int64_t)row * ldx;
  float* dr = dx + (int64_t)row * lddx;
  const int64_t t = tgt[row];
  const float scale = (t == ignore) ? 0.f : dloss[0] / count[0];
  const float L = lse[row];
  int j = threadIdx.x;
  for (; j + 7 * CE_THREADS < V; j += 8 * CE_THREADS) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = xr[j + k * CE_THREADS];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = j + k * CE_THREADS;
      dr[c] = (expf(v[k] - L) - (c == t ? 1.f : 0.f)) * scale;
    }
  }
  for (; j < V; j += CE_THREADS) dr[j] = (expf(xr[j] - L) - (j == t ? 1.f : 0.f)) * scale;
}

// ---- policy-gradient (self-critical) loss over full-length sampled captions -----------------------
// logits [T R][ldx], t-major (row t R + r = caption r at step t: the teacher-forced forward's packed
// scores when every length is T), ids [R][ids_ld], advantage [R].  One workgroup per row, as the cross
// entropy's.  live(r, t) = no end_id in ids[r][0 .. t-1], found by the workgroup itself.  Forward:
// y = x / tau, logp = y[id] - logsumexp(y), term = A_r logp; k_pg_reduce: loss = -(sum term) / #live in
// a fixed order.  Backward: dx = (exp(y - lse) - [v == id]) dloss A_r / (tau #live).  A dead row, or
// one whose caption has A_r == 0, is never read: its term is 0 and its gradient row is written as +0.
// An id outside [0, V) at a live position poisons the loss and that gradient row with NaN (whatever
// A_r is), as the cross entropy's bad target does.
__device__ __forceinline__ bool pg_live(const int64_t* __restrict__ idr, int t, int end_id) {
  if (end_id < 0) return true;
  int hit = 0;
  for (int i = threadIdx.x; i < t; i += CE_THREADS) hit |= idr[i] == (int64_t)end_id;
  return !__syncthreads_or(hit);
}

// the row's y_v = x_v / tau (x / 1 is x exactly: the division is skipped at tau == 1, same bits)
__device__ __forceinline__ float pg_y(float x, float tau, bool unit) { return unit ? x : x / tau; }

// thread 0, after the row's log-sum-exp: the row's outputs
__device__ __forceinline__ void pg_row_out(const float* __restrict__ xr, int V, int64_t id, float A, float tau,
                                           bool unit, float lse, int row, int64_t lp_at, float* __restrict__ lse_out,
                                           float* __restrict__ term_out, int* __restrict__ live_out,
                                           float* __restrict__ logp) {
  const bool bad = id < 0 || id >= V;
  const float lp = bad ? NAN : pg_y(xr[id], tau, unit) - lse;
  lse_out[row] = lse;
  term_out[row] = bad ? NAN : (A == 0.f ? 0.f : A * lp);
  live_out[row] = 1;
  if (logp) logp[lp_at] = lp;
}

template <bool REG>
__global__ __launch_bounds__(CE_THREADS) void k_pg_rows(const float* __restrict__ x, int64_t ldx, int R, int T, int V,
                                                        const int64_t* __restrict__ ids, int64_t ids_ld,
                                                        const float* __restrict__ adv, int end_id, float tau,
                                                        float* __restrict__ lse_out, float* __restrict__ term_out,
                                                        int* __restrict__ live_out, float* __restrict__ logp) {
  const int row = blockIdx.x;
  const int t = row / R, r = row - t * R;
  const int64_t* __restrict__ idr = ids + (int64_t)r * ids_ld;
  const int64_t lp_at = (int64_t)r * T + t;
  __shared__ float red[CE_THREADS / 64], red2[CE_THREADS / 64];
  const bool live = pg_live(idr, t, end_id);  // uniform over the workgroup
  const float A = adv[r];
  int64_t id = 0;
  bool skip = !live;
  if (live) {
    id = idr[t];
    // nothing of the row is wanted: A_r == 0 with a valid id and no logp output
    skip = A == 0.f && !logp && id >= 0 && id < V;
  }
  if (skip) {
    if (threadIdx.x == 0) {
      lse_out[row] = 0.f;
      term_out[row] = 0.f;
      live_out[row] = live ? 1 : 0;
      if (logp) logp[lp_at] = 0.f;  // (reached by dead rows only)
    }
    return;
  }
  const float* __restrict__ xr = x + (int64_t)row * ldx;
  const bool unit = tau == 1.f;
  float lse;
  if (REG) {
    float v[CE_NPT];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < CE_NPT; ++k) {
      const int j = threadIdx.x + k * CE_THREADS;
      v[k] = j < V ? xr[j] : -INFINITY;
    }
#pragma unroll
    for (int k = 0; k < CE_NPT; ++k) {
      v[k] = pg_y(v[k], tau, unit);
      m = fmaxf(m, v[k]);
    }
    const float M = block_reduce(m, true, red);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < CE_NPT; ++k)
      if (threadIdx.x + k * CE_THREADS < V) s += expf(v[k] - M);
    const float S = block_reduce(s, false, red);
    lse = M + logf(S);
  } else {
    float m = -INFINITY, s = 0.f;
    int j = threadIdx.x;
    for (; j + 7 * CE_THREADS < V; j += 8 * CE_THREADS) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = xr[j + k * CE_THREADS];
#pragma unroll
      for (int k = 0; k < 8; ++k) lse_merge(m, s, pg_y(v[k], tau, unit), 1.f);
    }
    for (; j < V; j += CE_THREADS) lse_merge(m, s, pg_y(xr[j], tau, unit), 1.f);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float m2 = __shfl_xor(m, off), s2 = __shfl_xor(s, off);
      lse_merge(m, s, m2, s2);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      red[w] = m;
      red2[w] = s;
    }
    __syncthreads();
    float M = red[0], S = red2[0];
    for (int k = 1; k < CE_THREADS / 64; ++k) lse_merge(M, S, red[k], red2[k]);
    lse = M + logf(S);
  }
  if (threadIdx.x == 0) pg_row_out(xr, V, id, A, tau, unit, lse, row, lp_at, lse_out, term_out, live_out, logp);
}

__global__ __launch_bounds__(1024) void k_pg_reduce(const float* __restrict__ term_rows,
                                                    const int* __restrict__ live_rows, int N,
                                                    float* __restrict__ loss, float* __restrict__ count) {
  float s = 0.f;
  int c = 0;
  for (int i = threadIdx.x; i < N; i += 1024) {
    s += term_rows[i];
    c += live_rows[i];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_xor(s, off);
    c += __shfl_xor(c, off);
  }
  __shared__ float ws[16];
  __shared__ int wc[16];
  if ((threadIdx.x & 63) == 0) {
    ws[threadIdx.x >> 6] = s;
    wc[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float S = 0.f;
    int C = 0;
    for (int k = 0; k < 16; ++k) {
      S += ws[k];
      C += wc[k];
    }
    count[0] = (float)C;  // >= R: step 0 of every caption is live
    loss[0] = -S / (float)C;
  }
}

// x and dx may alias (lddx == ldx), as in k_ce_bwd: an element is read by the thread that writes it
__global__ __launch_bounds__(CE_THREADS) void k_pg_bwd(const float* x, int64_t ldx, int R, int T, int V,
                                                       const int64_t* __restrict__ ids, int64_t ids_ld,
                                                       const float* __restrict__ adv, float tau,
                                                       const float* __restrict__ lse, const int* __restrict__ live_rows,
                                                       const float* __restrict__ dloss, const float* __restrict__ count,
                                                       float* dx, int64_t lddx) {
  const int row = blockIdx.x;
  const int t = row / R, r = row - t * R;
  float* dr = dx + (int64_t)row * lddx;
  const float A = adv[r];
  int64_t id = 0;
  bool bad = false;
  if (live_rows[row]) {
    id = ids[(int64_t)r * ids_ld + t];
    bad = id < 0 || id >= V;
  }
  if (!live_rows[row] || (A == 0.f && !bad)) {
    for (int j = threadIdx.x; j < V; j += CE_THREADS) dr[j] = 0.f;  // the logits are not read
    return;
  }
  const float* xr = x + (int64_t)row * ldx;
  const bool unit = tau == 1.f;
  const float scale = bad ? NAN : (dloss[0] * A) / (tau * count[0]);
  const float L = lse[row];
  int j = threadIdx.x;
  for (; j + 7 * CE_THREADS < V; j += 8 * CE_THREADS) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = xr[j + k * CE_THREADS];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = j + k * CE_THREADS;
      dr[c] = (expf(pg_y(v[k], tau, unit) - L) - (c == id ? 1.f : 0.f)) * scale;
    }
  }
  for (; j < V; j += CE_THREADS) dr[j] = (expf(pg_y(xr[j], tau, unit) - L) - (j == id ? 1.f : 0.f)) * scale;
}

// ---- clip_grad_norm_ (torch.nn.utils.clip_grad_norm_(params, max_norm), 2-norm; train.py:213-214) --------
// torch: norms = _foreach_norm(grads); total = vector_norm(stack(norms)); coef = max_norm / (total +
// 1e-6); grads *= clamp(coef, max=1).  Here: k_clip_sumsq writes one fp32 sum of squares per workgroup
// (CLIP_CHUNK elements of one tensor, a fixed order), k_clip_norm adds each tensor's partials in block
// order, takes the norm, combines the tensors' norms as torch does and writes the total (the caller's
// float) and the coefficient; k_clip_scale multiplies every gradient by the clamped coefficient (a
// multiply by exactly 1.0 when no clip is due, as torch's).  Three launches, one host call.
constexpr int CLIP_THREADS = 256, CLIP_VEC = 4, CLIP_ROUNDS = 8;
constexpr int CLIP_CHUNK = CLIP_THREADS * CLIP_VEC * CLIP_ROUNDS;  // 8192 elements per workgroup
struct ClipArgs {
  int n;
  int aligned;                            // bit i: tensor i is 16-byte aligned
  int64_t blk0[AA_CLIP_MAX_TENSORS + 1];  // first workgroup of tensor i (prefix sum)
  int64_t numel[AA_CLIP_MAX_TENSORS];
  float* g[AA_CLIP_MAX_TENSORS];
  float* part;      // [workgroups] sums of squares
  float* out;       // [2]: (unused), clamped coefficient
  float* total;     // the caller's total-norm float
  float max_norm;
};
__device__ __forceinline__ int clip_tensor(const ClipArgs& a, int64_t blk) {
  int t = 0;
  while (t + 1 < a.n && blk >= a.blk0[t + 1]) ++t;
  return t;
}
__global__ __launch_bounds__(CLIP_THREADS) void k_clip_sumsq(ClipArgs a) {
  const int64_t blk = blockIdx.x;
  const int t = clip_tensor(a, blk);
  const int64_t base = (blk - a.blk0[t]) * CLIP_CHUNK, n = a.numel[t];
  const float* __restrict__ G = a.g[t];
  float acc = 0.f;
  if (((a.aligned >> t) & 1) && base + CLIP_CHUNK <= n) {
    float4 g4[CLIP_ROUNDS];
#pragma unroll
    for (int r = 0; r < CLIP_ROUNDS; ++r)
      g4[r] = *reinterpret_cast<const float4*>(G + base + ((int64_t)r * CLIP_THREADS + threadIdx.x) * CLIP_VEC);
#pragma unroll
    for (int r = 0; r < CLIP_ROUNDS; ++r) {
      acc = fmaf(g4[r].x, g4[r].x, acc);
      acc = fmaf(g4[r].y, g4[r].y, acc);
      acc = fmaf(g4[r].z, g4[r].z, acc);
      acc = fmaf(g4[r].w, g4[r].w, acc);
    }
  } else {
    const int64_t end = base + CLIP_CHUNK < n ? base + CLIP_CHUNK : n;
    for (int64_t i = base + threadIdx.x; i < end; i += CLIP_THREADS) acc = fmaf(G[i], G[i], acc);
  }
  __shared__ float red[CLIP_THREADS / 64];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.part[blk] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(CLIP_THREADS) void k_clip_norm(ClipArgs a) {
  __shared__ float red[CLIP_THREADS / 64];
  __shared__ float norms[AA_CLIP_MAX_TENSORS];
  for (int t = 0; t < a.n; ++t) {
    float acc = 0.f;
    for (int64_t i = a.blk0[t] + threadIdx.x; i < a.blk0[t + 1]; i += CLIP_THREADS) acc += a.part[i];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) norms[t] = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int t = 0; t < a.n; ++t) s = fmaf(norms[t], norms[t], s);
    const float total = sqrtf(s);
    const float coef = a.max_norm / (total + 1e-6f);
    *a.total = total;
    a.out[1] = coef > 1.f ? 1.f : coef;  // clamp(max = 1) that keeps a NaN, as torch.clamp does
  }
}
__global__ __launch_bounds__(CLIP_THREADS) void k_clip_scale(ClipArgs a) {
  const int64_t blk = blockIdx.x;
  const int t = clip_tensor(a, blk);
  const int64_t base = (blk - a.blk0[t]) * CLIP_CHUNK, n = a.numel[t];
  float* __restrict__ G = a.g[t];
  const float c = a.out[1];
  if (((a.aligned >> t) & 1) && base + CLIP_CHUNK <= n) {
#pragma unroll
    for (int r = 0; r < CLIP_ROUNDS; ++r) {
      float4* q = reinterpret_cast<float4*>(G + base + ((int64_t)r * CLIP_THREADS + threadIdx.x) * CLIP_VEC);
      float4 v = *q;
      v.x *= c; v.y *= c; v.z *= c; v.w *= c;
      *q = v;
    }
  } else {
    const int64_t end = base + CLIP_CHUNK < n ? base + CLIP_CHUNK : n;
    for (int64_t i = base + threadIdx.x; i < end; i += CLIP_THREADS) G[i] *= c;
  }
}

}  // namespace aa_optim

using namespace aa_optim;

extern "C" {

int aa_adam_step(const aa_adam_tensor* tensors, int32_t n, double step, double lr, double beta1, double beta2,
                 double eps, double weight_decay, aa_stream_t stream) {
  if (n < 0) return AA_ERR_SHAPE;
  if (n > 0 && !tensors) return AA_ERR_NULL;
  if (!(step >= 1.0)) return AA_ERR_SHAPE;
  // step-invariant scalars exactly as torch computes them (Python doubles, cast to fp32 opmath)
  const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
  AdamArgs a;
  a.w1 = (float)(1.0 - beta1);
  a.beta2 = (float)beta2;
  a.omb2 = (float)(1.0 - beta2);
  a.bc2_sqrt = (float)sqrt(bc2);
  a.step_size = (float)((lr / bc1) * -1.0);
  a.eps = (float)eps;
  a.wd = (float)weight_decay;
  for (int i0 = 0; i0 < n; i0 += AA_ADAM_MAX_TENSORS) {  // one launch per AA_ADAM_MAX_TENSORS tensors
    a.n = 0;
    a.aligned = 0;
    int64_t blocks = 0;
    for (int i = i0; i < n && i < i0 + AA_ADAM_MAX_TENSORS; ++i) {
      const aa_adam_tensor& T = tensors[i];
      if (T.numel < 0) return AA_ERR_SHAPE;
      if (T.numel == 0) continue;
      if (!T.param || !T.grad || !T.exp_avg || !T.exp_avg_sq) return AA_ERR_NULL;
      const int k = a.n++;
      a.p[k] = (float*)T.param;
      a.g[k] = (const float*)T.grad;
      a.m[k] = (float*)T.exp_avg;
      a.v[k] = (float*)T.exp_avg_sq;
      a.numel[k] = T.numel;
      const uintptr_t orp = (uintptr_t)T.param | (uintptr_t)T.grad | (uintptr_t)T.exp_avg | (uintptr_t)T.exp_avg_sq;
      if ((orp & 15) == 0) a.aligned |= 1 << k;
      a.blk0[k] = blocks;
      blocks += (T.numel + ADAM_CHUNK - 1) / ADAM_CHUNK;
    }
    if (a.n == 0) continue;
    a.blk0[a.n] = blocks;
    if (blocks > 0x7fffffff) return AA_ERR_SHAPE;
    hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return AA_OK;
}

static bool clip_args(const aa_grad_tensor* t, int32_t n, ClipArgs* a, int64_t* blocks) {
  a->n = 0;
  a->aligned = 0;
  *blocks = 0;
  for (int i = 0; i < n; ++i) {
    if (t[i].numel < 0) return false;
    if (t[i].numel == 0) continue;
    const int k = a->n++;
    a->g[k] = t[i].grad;
    a->numel[k] = t[i].numel;
    if (((uintptr_t)t[i].grad & 15) == 0) a->aligned |= 1 << k;
    a->blk0[k] = *blocks;
    *blocks += (t[i].numel + CLIP_CHUNK - 1) / CLIP_CHUNK;
  }
  a->blk0[a->n] = *blocks;
  return true;
}

size_t aa_clip_grad_norm_workspace_bytes(const aa_grad_tensor* tensors, int32_t n) {
  if (n < 0 || n > AA_CLIP_MAX_TENSORS || (n > 0 && !tensors)) return 0;
  ClipArgs a;
  int64_t blocks;
  if (!clip_args(tensors, n, &a, &blocks)) return 0;
  return (size_t)(blocks + 2) * sizeof(float);
}

int aa_clip_grad_norm(const aa_grad_tensor* tensors, int32_t n, float max_norm, float* total_norm, void* workspace,
                      size_t workspace_bytes, aa_stream_t stream) {
  if (n < 0 || n > AA_CLIP_MAX_TENSORS) return AA_ERR_SHAPE;
  if ((n > 0 && !tensors) || !total_norm || !workspace) return AA_ERR_NULL;
  ClipArgs a;
  int64_t blocks;
  if (!clip_args(tensors, n, &a, &blocks)) return AA_ERR_SHAPE;
  for (int k = 0; k < a.n; ++k)
    if (!a.g[k]) return AA_ERR_NULL;
  if (workspace_bytes < (size_t)(blocks + 2) * sizeof(float)) return AA_ERR_BUFFER;
  if (blocks > 0x7fffffff) return AA_ERR_SHAPE;
  float* ws = (float*)workspace;
  a.out = ws;
  a.part = ws + 2;
  a.total = total_norm;
  a.max_norm = max_norm;
  hipStream_t st = (hipStream_t)stream;
  if (blocks > 0) hipLaunchKernelGGL(k_clip_sumsq, dim3((unsigned)blocks), dim3(CLIP_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_clip_norm, dim3(1), dim3(CLIP_THREADS), 0, st, a);
  if (blocks > 0) hipLaunchKernelGGL(k_clip_scale, dim3((unsigned)blocks), dim3(CLIP_THREADS), 0, st, a);
  return (int)hipGetLastError();
}

size_t aa_cross_entropy_workspace_bytes(int32_t N) {
  return N <= 0 ? 0 : (size_t)N * 3 * sizeof(float);
}

int aa_cross_entropy_forward(const float* logits, int32_t N, int32_t V, int64_t ldx, const int64_t* targets,
                             int64_t ignore_index, float* loss, float* count, void* workspace,
                             size_t workspace_bytes, aa_stream_t stream) {
  if (N <= 0 || V <= 0 || ldx < V) return AA_ERR_SHAPE;
  if (!logits || !targets || !loss || !count || !workspace) return AA_ERR_NULL;
  if (workspace_bytes < aa_cross_entropy_workspace_bytes(N)) return AA_ERR_BUFFER;
  float* lse = (float*)workspace;
  float* rows = lse + N;
  int* valid = (int*)(rows + N);
  hipStream_t st = (hipStream_t)stream;
  if (V <= CE_THREADS * CE_NPT)
    hipLaunchKernelGGL(k_ce_rows_reg, dim3(N), dim3(CE_THREADS), 0, st, logits, ldx, V, targets, ignore_index, lse,
                       rows, valid);
  else
    hipLaunchKernelGGL(k_ce_rows, dim3(N), dim3(CE_THREADS), 0, st, logits, ldx, V, targets, ignore_index, lse, rows,
                       valid);
  hipLaunchKernelGGL(k_ce_reduce, dim3(1), dim3(1024), 0, st, rows, valid, N, loss, count);
  return (int)hipGetLastError();
}

int aa_cross_entropy_backward(const float* logits, int32_t N, int32_t V, int64_t ldx, const int64_t* targets,
                              int64_t ignore_index, const float* dloss, const float* count, const void* workspace,
                              size_t workspace_bytes, float* dlogits, int64_t lddx, aa_stream_t stream) {
  if (N <= 0 || V <= 0 || ldx < V || lddx < V) return AA_ERR_SHAPE;
  if (!logits || !targets || !dloss || !count || !workspace || !dlogits) return AA_ERR_NULL;
  // the forward's per-row log-sum-exp: a workspace from a forward over fewer rows is refused
  if (workspace_bytes < aa_cross_entropy_workspace_bytes(N)) return AA_ERR_BUFFER;
  if (dlogits == logits && lddx != ldx) return AA_ERR_SHAPE;  // in place only with the same pitch
  hipLaunchKernelGGL(k_ce_bwd, dim3(N), dim3(CE_THREADS), 0, (hipStream_t)stream, logits, ldx, V, targets,
                     ignore_index, (const float*)workspace, dloss, count, dlogits, lddx);
  return (int)hipGetLastError();
}

// workspace: per row its log-sum-exp, its loss term A_r logp and its live flag
size_t aa_policy_loss_workspace_bytes(int32_t R, int32_t T) {
  if (R <= 0 || T <= 0 || (int64_t)R * T > 0x7fffffff) return 0;
  return (size_t)R * (size_t)T * 3 * sizeof(float);
}

static bool pg_shape_ok(int64_t ldx, int32_t R, int32_t T, int32_t V, int64_t ids_ld, float temperature) {
  return R > 0 && T > 0 && V > 0 && ldx >= V && ids_ld >= T && isfinite(temperature) && temperature > 0.f &&
         (int64_t)R * T <= 0x7fffffff;
}

int aa_policy_loss_forward(const float* logits, int64_t ldx, int32_t R, int32_t T, int32_t V, const int64_t* ids,
                           int64_t ids_ld, const float* advantage, int32_t end_id, float temperature, float* loss,
                           float* count, float* logp, void* workspace, size_t workspace_bytes, aa_stream_t stream) {
  if (!pg_shape_ok(ldx, R, T, V, ids_ld, temperature)) return AA_ERR_SHAPE;
  if (!logits || !ids || !advantage || !loss || !count || !workspace) return AA_ERR_NULL;  // logp may be NULL
  if (workspace_bytes < aa_policy_loss_workspace_bytes(R, T)) return AA_ERR_BUFFER;
  const int N = R * T;
  float* lse = (float*)workspace;
  float* term = lse + N;
  int* live = (int*)(term + N);
  hipStream_t st = (hipStream_t)stream;
  if (V <= CE_THREADS * CE_NPT)
    hipLaunchKernelGGL(k_pg_rows<true>, dim3(N), dim3(CE_THREADS), 0, st, logits, ldx, R, T, V, ids, ids_ld, advantage,
                       end_id, temperature, lse, term, live, logp);
  else
    hipLaunchKernelGGL(k_pg_rows<false>, dim3(N), dim3(CE_THREADS), 0, st, logits, ldx, R, T, V, ids, ids_ld,
                       advantage, end_id, temperature, lse, term, live, logp);
  hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(1024), 0, st, term, live, N, loss, count);
  return (int)hipGetLastError();
}

int aa_policy_loss_backward(const float* logits, int64_t ldx, int32_t R, int32_t T, int32_t V, const int64_t* ids,
                            int64_t ids_ld, const float* advantage, int32_t end_id, float temperature,
                            const float* dloss, const float* count, const void* workspace, size_t workspace_bytes,
                            float* dlogits, int64_t lddx, aa_stream_t stream) {
  (void)end_id;  // the live flags are the forward's, in the workspace
  if (!pg_shape_ok(ldx, R, T, V, ids_ld, temperature) || lddx < V) return AA_ERR_SHAPE;
  if (dlogits && dlogits == logits && lddx != ldx) return AA_ERR_SHAPE;  // in place only with the same pitch
  if (!logits || !ids || !advantage || !dloss || !count || !workspace || !dlogits) return AA_ERR_NULL;
  if (workspace_bytes < aa_policy_loss_workspace_bytes(R, T)) return AA_ERR_BUFFER;
  const int N = R * T;
  const float* lse = (const float*)workspace;
  const int* live = (const int*)(lse + 2 * (size_t)N);
  hipLaunchKernelGGL(k_pg_bwd, dim3(N), dim3(CE_THREADS), 0, (hipStream_t)stream, logits, ldx, R, T, V, ids, ids_ld,
                     advantage, temperature, lse, live, dloss, count, dlogits, lddx);
  return (int)hipGetLastError();
}

// Measurement helper (bench.py): one streaming read of [src, src + nbytes) by 16-B loads, grid-stride,
// 8 loads in flight per thread, each workgroup's sum written to out[blockIdx.x] (so the loads are not
// dead).  Read twice over a buffer that fits the 256 MiB Infinity Cache, the second pass measures the
// MALL-served read rate that k_atten's per-step re-read of V (51.4 MB at B = 512) runs against; over a
// buffer several times that size, the HBM read rate.
int aa_read_probe(const void* src, size_t nbytes, float* out, int32_t blocks, aa_stream_t stream) {
  if (!src || !out) return AA_ERR_NULL;
  if (blocks <= 0 || nbytes % 16 || ((uintptr_t)src & 15)) return AA_ERR_SHAPE;
  hipLaunchKernelGGL(aa_optim::k_read_probe, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const float4*>(src), (int64_t)(nbytes / 16), out);
  return (int)hipGetLastError();
}

}  // extern "C"
