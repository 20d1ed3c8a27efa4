// aa_encoder.hip — what runs once per weight set or once per batch, before the step loop
// (reference: code_src/models/baseline_attention.py, code_src/models/adaptive_attention.py).
//   pack time (once per weight set)
//     k_pack_lstm     W_hh / emb-part / v_g-part of W_ih and W_x re-laid in gate-interleaved tiles
//     k_gemm_bias     table[v] = embed[v] . [W_ih(emb part); W_x(emb part)]^T   (V x 5H)
//     k_pack_mlp      bf16 copy and row norms of W_m for the vocab screen (k_pack_gs: per granule)
//     k_pack_w3 / w4  bf16x3 MFMA-fragment copies of W_a, W_hh, W_m, the heads, W_vg, W_v
//     k_w4h_scale, k_pack_w4h  the scaled fp16x2 fragment copy of W_a (k_enc_v4's fast path)
//   encoder tail (once per batch), encoder_launch
//     k_enc_v4        V = relu(A^T W_a^T + b_a) [B*49, H] and a_g = AvgPool2d(7)(A) in one pass over the
//                     feature map (fp16x2 split, bf16x3 fallback)    baseline_attention.py:46-51
//     k_gemm3         v_g | h0 | c0 = act(a_g [W_b;W_h0;W_c0]^T + b) (MODE_HEADS)              :53-60
//                     VWv = V W_v^T (step-invariant, hoisted)         adaptive_attention.py:34
//                     xg = v_g . [W_ih(v_g part); W_x(v_g part)]^T + b_ih + b_hh (step-invariant)
//     k_avgpool, k_enc_v, k_enc_v3, k_enc_heads, k_gemm_bias: the fp32-MFMA encoder (AA_DECODE_FP32_ENCODER,
//                     the training forward) and the shapes k_enc_v4 / k_gemm3 do not take
//     k_decode_init   the greedy decode's <start> tokens and key clear (when the heads launch does not do it)
#include "aa_internal.hpp"

namespace aa {

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

// The fast path (default): the same GEMM from a TWO-way fp16 split, three products per block instead
// of six.  fp16 has an 11-bit significand, so x ~ hi + lo (hi = fp16(x), lo = fp16(x - hi), the
// difference exact in fp32) carries 22 bits: lo's own rounding leaves <= 2^-22 |x| while lo is a
// normal fp16 number.  hi.W_hi, hi.W_lo and lo.W_hi are exact in the fp32 accumulator (22-bit
// products); the dropped lo.W_lo is <= 2^-22 |a w|.  Per term that is <= 3 x 2^-22 |a w| in the worst
// case and ~2^-24 |a w| rms, so over K = 2048 terms of independent sign the result stays in the
// fp32-GEMM class (fp32 accumulation, the same in both paths, dominates).
// fp16's range is what needs care (bf16 has fp32's):
//   W_a is scaled at pack time by one power of two per tensor (k_pack_w4h: max|W_a| 2^e lands in
//   [2^13, 2^14), a factor >= 4 under fp16's 65504), so the lo part of every weight down to
//   2^-17 max|W_a| is a normal fp16 number;
//   the features are scaled by 2^ENC_F16_A_EXP = 64 as they are split.  A larger scale keeps the lo
//   parts of smaller features normal, a smaller one raises the overflow threshold; they multiply to
//   2^15.  Post-ReLU trunk features are O(1) with maxima of a few tens, so the threshold
//   ENC_F16_A_MAX = 512 sits an order of magnitude above them (hi <= 2^15, a factor 2 under 65504),
//   and a feature keeps a normal lo part down to 2^-3 / 64 = 2^-9.  Below that lo is subnormal: its
//   error is 2^-25 absolute (of the scaled value; MFMA reads fp16 subnormals as they are), i.e.
//   2^-31 per feature: 2^-22 of a 2^-9 feature, 2^-20 of the 2^-11 mean of features spread over
//   [1e-6, 1e-3].  A map whose features are ALL that small still meets the scheme's 2^-21 of
//   sum |a w|, because the errors are independent in sign over K = 2048 terms (emulation: 2^-24;
//   on the device, U[0,1) x 1e-4 features: 5.3e-7 against bf16x3's 1.6e-7, x 1 and x 100: 1.7e-7
//   against 2.4e-7, tests/test_gpu_encoder_f16.py) -- small features cost accuracy gradually, they
//   never trip anything.
//   Both scales are exact powers of two, removed by one exact multiply before bias and relu.
// Range guard: every staging thread notes a feature that is not finite or not below ENC_F16_A_MAX
// in magnitude; after the K loop a workgroup that saw one (an LDS flag: no global state, no second
// launch, no host sync) recomputes its two images with the bf16x3 body below, so such an image comes
// out bit for bit as the bf16x3 kernel computes it.  The bf16x3 body needs the larger register set,
// so carrying it costs the fast path nothing.  x3_only (AA_DECODE_ENC_BF16X3) sends every workgroup
// through the bf16x3 body only.  a_g is computed from the fp32 stage copy either way: bit-identical.
template <bool F>
struct BoolC {
  static constexpr bool value = F;
};
// (Tried on the fast path: stage s + 1's W fragments in a second register set, loaded at the start of
// stage s instead of after the pair's last MFMA -- 16 + 16 VGPRs of W.  128 VGPRs and 20 B/lane of
// scratch at 16 waves, k_enc_v4 175.7 / 178.9 -> 182.1 / 182.6 us in A/B: not kept.  The W loads'
// latency is not what the stage waits for.)
// (Also tried and not kept: 64-channel stages, and every thread staging four values per stage)

template <int NCB, int NW = 8>
__global__ __launch_bounds__(64 * NW) void k_enc_v4(const float* __restrict__ feats, int B, int C,
                                                const bf16x8* __restrict__ W4, const f16x8* __restrict__ W4h,
                                                const float* __restrict__ w4h_sc, const float* __restrict__ bias,
                                                float* __restrict__ V, float* __restrict__ a_g, int x3_only) {
  static_assert(NCB % 2 == 0, "columns are processed in pairs of 16-column blocks");
  constexpr int H = 16 * NCB * NW, NPAIR = NCB / 2, PL = E4_RB * 16 * E4_LD;  // PL: one plane, 16-bit elements
  constexpr int NT = 64 * NW;
  const bool stager = NW == 8 || threadIdx.x < 512;
  __shared__ __attribute__((aligned(16))) __bf16 As[2][3][PL];  // (the fp16 path: planes 0, 1 hold fp16 bits)
  __shared__ __attribute__((aligned(16))) float Sg[2][2 * 32 * E4_SP];  // fp32 stage copy for a_g
  __shared__ __attribute__((aligned(16))) float Ag[2 * E4_MAXC];        // a_g of the two images
  __shared__ int over_any;                                              // the range guard's flag
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
  floatx4 acc[E4_RB][NCB];

  // The K loop, as the fp16x2 fast path (F16) or the bf16x3 body: NPL planes of A in LDS and of W in
  // registers (16-byte fragments either way; the fp16 ones travel as bf16x8 bits).  Returns whether
  // this thread staged a feature outside the fast path's range (F16 only).
  auto kloop = [&](auto f16) -> bool {
    constexpr bool F16 = decltype(f16)::value;
    constexpr int NPL = F16 ? 2 : 3;
    const bf16x8* wsrc = (F16 ? reinterpret_cast<const bf16x8*>(W4h) : W4) + (size_t)(wave * NCB) * KC * NPL * 64 +
                         lane;  // block nb = wave NCB + c
    float ra[8];
    bf16x8 wv[NCB][NPL];
    bool over = false;
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
      for (int q = 0; q < NPL; ++q) wv[c][q] = wsrc[((size_t)c * KC * NPL + (size_t)s * NPL + q) * 64];
    };
    auto lstore_a = [&](int buf) {
      if constexpr (F16) {
        f16x8 x[2];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          _Float16 hi, lo;
          split2h(ra[i] * (float)(1 << ENC_F16_A_EXP), hi, lo);
          x[0][i] = hi; x[1][i] = lo;
          over |= !(__builtin_fabsf(ra[i]) < ENC_F16_A_MAX);  // also true for NaN
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) *reinterpret_cast<bf16x8*>(&As[buf][q][so]) = __builtin_bit_cast(bf16x8, x[q]);
      } else {
        bf16x8 x[3];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          __bf16 x0, x1, x2;
          split3(ra[i], x0, x1, x2);
          x[0][i] = x0; x[1][i] = x1; x[2][i] = x2;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<bf16x8*>(&As[buf][q][so]) = x[q];
      }
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
      if (stg) lstore_a(buf ^ 1);
      __builtin_amdgcn_sched_barrier(0);
      const __bf16* Ab = &As[buf][0][fo];
#pragma unroll
      for (int cp = 0; cp < NPAIR; ++cp) {
#pragma unroll
        for (int rb = 0; rb < E4_RB; ++rb) {
          bf16x8 fa[NPL];
#pragma unroll
          for (int q = 0; q < NPL; ++q) fa[q] = *reinterpret_cast<const bf16x8*>(Ab + q * PL + rb * 16 * E4_LD);
          // the pair's two accumulator chains interleaved (each chain's product order unchanged:
          // bit-identical), so no MFMA waits on its immediate predecessor
          const int c0 = 2 * cp, c1 = c0 + 1;
          floatx4 x = acc[rb][c0], y = acc[rb][c1];
          if constexpr (F16) {  // smallest first: lo.W_hi, hi.W_lo, hi.W_hi
            const f16x8 ah = __builtin_bit_cast(f16x8, fa[0]), al = __builtin_bit_cast(f16x8, fa[1]);
            const f16x8 w0h = __builtin_bit_cast(f16x8, wv[c0][0]), w0l = __builtin_bit_cast(f16x8, wv[c0][1]);
            const f16x8 w1h = __builtin_bit_cast(f16x8, wv[c1][0]), w1l = __builtin_bit_cast(f16x8, wv[c1][1]);
            x = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, w0h, x, 0, 0, 0);
            y = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, w1h, y, 0, 0, 0);
            x = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, w0l, x, 0, 0, 0);
            y = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, w1l, y, 0, 0, 0);
            x = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, w0h, x, 0, 0, 0);
            y = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, w1h, y, 0, 0, 0);
          } else {
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
          }
          acc[rb][c0] = x;
          acc[rb][c1] = y;
          // Stage s+2's features are asked for here, behind the first row block's MFMAs.  Issued at the
          // top of the stage (inside `if (stg)`, which the other waves skip) they were drained at once:
          // where the two paths join, the waits for the W fragments in front of the first MFMAs must hold
          // for both, vmcnt counts in order, and so `vmcnt(0)` also waited for the eight loads a staging
          // wave had just issued.  Here nothing waits for them before the next stage's lstore_a.
          if (cp == 0 && rb == 0) {
            __builtin_amdgcn_sched_barrier(0);
            if (stg) gload_a(s2);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        gload_w(s1, 2 * cp);
        gload_w(s1, 2 * cp + 1);
        // re-read the A fragments for the next pair instead of keeping them all live (VGPR budget)
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
    return over;
  };

  bool x3 = x3_only != 0;  // (workgroup-uniform)
  float unscale = 1.0f;
  if (!x3) {
    if (t == 0) over_any = 0;  // (ordered before the flag's writers by the K loop's barriers)
    if (kloop(BoolC<true>{})) over_any = 1;
    __syncthreads();
    x3 = over_any != 0;
    unscale = w4h_sc[0];
  }
  if (x3) {  // every LDS read of the fast path's last stage is behind its closing barrier
    kloop(BoolC<false>{});
    unscale = 1.0f;  // (x 1.0f is exact: the bf16x3 body's V is what it was without the fast path)
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
      for (int i = 0; i < 4; ++i)
        Vs[(4 * (lane >> 4) + i) * VSP + col] = reluf_(acc[rb][c][i] * unscale + bvs[c]);  // the exact un-scale first
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

// Start of a greedy decode: <start> tokens, and (exact vocab stage) the [T][B] argmax keys that
// k_vocab accumulates by atomicMax cleared -- by memory-side stores, like the atomics that follow (a
// plain store's line would stay in this XCD's L2)
__global__ void k_decode_init(int64_t* __restrict__ tok, int B, int64_t v, uint64_t* __restrict__ keys, int n) {
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (int i = i0; i < B; i += stride) tok[i] = v;
  if (keys)
    for (int i = i0; i < n; i += stride) __hip_atomic_store(keys + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// The fp16x2 copy of W_a (k_enc_v4's fast path).  k_w4h_scale (one workgroup): the tensor's power-of-two
// scale from max|W_a| (see ENC_F16_W_TOP), stored with the model as sc[0] = 2^-(e + ENC_F16_A_EXP), the
// kernel's un-scale, and sc[1] = e.  k_pack_w4h: W_a 2^e split in two fp16 planes (hi, lo) in k_pack_w4's
// fragment order, planes at out[((nb KC + kc) 2 + q) 64 + l].
__global__ __launch_bounds__(1024) void k_w4h_scale(const float* __restrict__ w, size_t n, float* __restrict__ sc) {
  __shared__ uint32_t part[16];
  uint32_t mx = 0;  // max |w| by its bit pattern (a NaN or inf ends up on top and gives e = 0)
  for (size_t i = threadIdx.x; i < n; i += 1024) {
    const uint32_t u = __float_as_uint(w[i]) & 0x7FFFFFFFu;
    mx = u > mx ? u : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t x = (uint32_t)__shfl_xor((int)mx, o, 64);
    mx = x > mx ? x : mx;
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 16; ++i) mx = part[i] > mx ? part[i] : mx;
    const int be = (int)(mx >> 23);  // biased exponent: 0 (zero / subnormal) and 255 (inf / NaN) take e = 0
    int e = be == 0 || be == 255 ? 0 : ENC_F16_W_TOP - (be - 127);
    e = e > ENC_F16_W_ECLAMP ? ENC_F16_W_ECLAMP : e < -ENC_F16_W_ECLAMP ? -ENC_F16_W_ECLAMP : e;
    sc[0] = ldexpf(1.0f, -(e + ENC_F16_A_EXP));
    sc[1] = (float)e;
  }
}
__global__ void k_pack_w4h(const float* __restrict__ w, int C, const float* __restrict__ sc, f16x8* __restrict__ out) {
  const int KC = C / 32, nb = blockIdx.x / KC, kc = blockIdx.x % KC, l = threadIdx.x;
  const float* src = w + (int64_t)(16 * nb + (l & 15)) * C + 32 * kc + 8 * (l >> 4);
  const float scale = ldexpf(1.0f, (int)sc[1]);
  f16x8 h, lo;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    _Float16 a, b;
    split2h(src[j] * scale, a, b);
    h[j] = a; lo[j] = b;
  }
  f16x8* o = out + ((size_t)blockIdx.x * 2) * 64 + l;
  o[0] = h;
  o[64] = lo;
}

// wgs[tile][j][u] = (j < 49 ? W_g[j] : W_s[j - 49])[tile*16 + u]
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

}  // namespace aa

using namespace aa;

namespace aa {

void gemm_bias(const float* A, int lda, int M, const float* W, int ldw, int N, int K, const float* bias, float* C,
                      int64_t ldc, hipStream_t s) {
  const int MT = (M + 63) / 64, NTn = N / 64;
  hipLaunchKernelGGL(k_gemm_bias, dim3(MT * NTn), dim3(256), 0, s, A, lda, M, W, ldw, N, K, bias, C, ldc);
}
// the training forward's fp32 encoder kernels
void avgpool_launch(const float* feats, int64_t nch, float* a_g, hipStream_t s) {
  hipLaunchKernelGGL(k_avgpool, dim3((unsigned)((nch + 255) / 256)), dim3(256), 0, s, feats, nch, a_g);
}
void enc_v_launch(const float* feats, int B, int C, int H, const float* w, const float* b, float* V, hipStream_t s) {
  const int M = B * P, MT = (M + 63) / 64, NTn = H / 64;
  hipLaunchKernelGGL(k_enc_v, dim3(MT * NTn), dim3(256), 0, s, feats, B, C, H, w, b, V);
}

}  // namespace aa

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
  hipLaunchKernelGGL(k_w4h_scale, dim3(1), dim3(1024), 0, s, w->enc_affine_a_w, (size_t)H * C, base + L.enc_w4h_sc);
  hipLaunchKernelGGL(k_pack_w4h, dim3((H / 16) * (C / 32)), dim3(64), 0, s, w->enc_affine_a_w, C,
                     (const float*)(base + L.enc_w4h_sc), reinterpret_cast<f16x8*>(base + L.enc_w4h));
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

// Encoder tail: k_enc_v4 (V and a_g in one pass over the features), then with an aux stream the a_g
// branch (k_gemm3 heads -> x_g GEMM: latency-bound) runs beside the VWv GEMM (k_gemm3: MFMA-bound), and
// `s` waits for aux before returning.  Shapes k_enc_v4 / k_gemm3 do not take, and AA_DECODE_FP32_ENCODER,
// go k_avgpool -> k_enc_heads -> x_g on the a_g branch beside k_enc_v3 / k_enc_v -> VWv.
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
int aa::encoder_launch(const Layout& L, const MP& p, const float* feats, int B, float* a_g, float* V, float* v_g,
                   float* h0, float* c0, float* VWv, float* xg, aa_event_t* ev, int32_t flags, hipStream_t s,
                   hipStream_t aux, bf16x8* hsp0, const DecodeInit* init) {
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
    const int x3_only = (flags & AA_DECODE_ENC_BF16X3) != 0;
    if (H == 512)
      AA_TLAUNCH(ev, 2, (k_enc_v4<32 / ENC4_NW, ENC4_NW>), dim3(nwg), dim3(64 * ENC4_NW), 0, s, feats, B, C,
                 (const bf16x8*)p.enc_w4, (const f16x8*)p.enc_w4h, (const float*)p.enc_w4h_sc, (const float*)p.enc_a_b,
                 V, a_g, x3_only);
    else
      AA_TLAUNCH(ev, 2, k_enc_v4<2>, dim3(nwg), dim3(512), 0, s, feats, B, C, (const bf16x8*)p.enc_w4,
                 (const f16x8*)p.enc_w4h, (const float*)p.enc_w4h_sc, (const float*)p.enc_a_b, V, a_g, x3_only);
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
    split_rows_launch(h0, B, H, hsp0, s);
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
