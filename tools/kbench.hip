// Kernel-level timing harness (tools only, not part of the product): includes the product kernels,
// re-launches one of them `reps` times on a workspace populated by a real aa_greedy_decode, and
// returns the mean time per launch (hidden size 512, the harness's model).  tools/kvariant.py adds
// copies of a kernel under study (the VARIANTS / VARIANT LAUNCH blocks) when a study needs them.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fPIC -shared -Iinclude \
//         -Wl,-z,defs tools/kbench.hip -o tools/_build/libkbench.so      (driven by tools/kbench.py)
// (the decode, encoder, beam and k_lstm units in one translation unit, so every launch function
// aa_kernels.hip calls is defined here -- vocab_launch is aa_beam.hip's -- and the library loads on its
// own; aa_lstm.hip without AA_LSTM_H holds every hidden size.  -Wl,-z,defs makes a missing one a link error.)
#include "../adaptive_amd/csrc/aa_kernels.hip"
#include "../adaptive_amd/csrc/aa_encoder.hip"
#include "../adaptive_amd/csrc/aa_beam.hip"
#include "../adaptive_amd/csrc/aa_lstm.hip"
#include <stdlib.h>
#include <string.h>

using namespace aa;

extern "C" int kb_time(const aa_model* m, const float* feats, void* ws, int B, int T, const char* which, int reps,
                       float* out_us) {
  Layout L;
  int rc = check_model(m, &L);
  if (rc) return rc;
  size_t need;
  DecodeWS w = carve_decode(static_cast<char*>(ws), L, B, T, &need);
  const MP p = resolve(m, L);
  hipStream_t s = nullptr;
  const int H = L.H, MT = (B + 63) / 64;
  const int t = 1;
  uint64_t* kt = w.keys + B;
  auto launch = [&]() -> bool {
    if (!strcmp(which, "lstm")) {
      hipLaunchKernelGGL(k_lstm<512>, dim3(MT * (H / 16)), dim3(512), 0, s, B, L.V, (const int64_t*)w.tok0, 1,
                         p.table, w.r.xg, w.r.hsp[0], w.r.c[0], (const int*)nullptr, p.whh3, p.wgs, w.r.h[1], w.r.hsp[1], w.r.c[1], w.r.s,
                         w.r.part,
                         RsArgs{});
    } else if (!strcmp(which, "atten5")) {
      hipLaunchKernelGGL(k_atten5<512>, dim3(B), dim3(512), 0, s, B, 1, w.r.h[1], w.r.s, w.r.part, w.e.V, w.e.vwv, p.wh,
                         (float*)nullptr, (int64_t)0, (float*)nullptr, (int64_t)0, w.r.u, w.ub, w.unorm, (bf16x8*)nullptr);
    } else if (!strcmp(which, "vscreen8")) {
      hipLaunchKernelGGL(k_vscreen8<512>, dim3(((B + SC2_BM - 1) / SC2_BM) * (L.Vp / SC2_BN)), dim3(SC8_NT), 0, s, B,
                         L.V, L.Vp, reinterpret_cast<const bf16x8*>(w.ub), w.unorm,
                         reinterpret_cast<const bf16x8*>(p.mlp_wb), p.mlp_gs, p.mlp_b, w.summ);
    } else if (!strcmp(which, "vscreen2")) {
      hipLaunchKernelGGL(k_vscreen2<512>, dim3(((B + SC2_BM - 1) / SC2_BM) * (L.Vp / SC2_BN)), dim3(256), 0, s, B,
                         L.V, L.Vp, reinterpret_cast<const bf16x8*>(w.ub), w.unorm,
                         reinterpret_cast<const bf16x8*>(p.mlp_wb), p.mlp_gs, p.mlp_b, w.summ);
    } else if (!strcmp(which, "vrescore")) {
      hipLaunchKernelGGL(k_vrescore<512>, dim3(B), dim3(RS_NT), 0, s, B, L.V, L.Vp, w.r.u, w.summ, p.mlp_w, p.mlp_b, kt,
                         (int64_t*)nullptr, T, t);
    } else if (!strcmp(which, "enc_v3")) {
      const int M = B * P;
      hipLaunchKernelGGL(k_enc_v3, dim3(((M + EV_BM - 1) / EV_BM) * (H / EV_BN)), dim3(256), 0, s, feats, B, L.C, H, p.enc_w3, p.enc_a_b, w.e.V);
    } else if (!strcmp(which, "enc_v4")) {
      hipLaunchKernelGGL((k_enc_v4<32 / ENC4_NW, ENC4_NW>), dim3((B * P + E4_ROWS - 1) / E4_ROWS), dim3(64 * ENC4_NW), 0,
                         s, feats, B, L.C, p.enc_w4, p.enc_w4h, p.enc_w4h_sc, p.enc_a_b, w.e.V, w.e.a_g, 0);
    } else if (!strcmp(which, "enc_v4_x3")) {  // the bf16x3 body in every workgroup
      hipLaunchKernelGGL((k_enc_v4<32 / ENC4_NW, ENC4_NW>), dim3((B * P + E4_ROWS - 1) / E4_ROWS), dim3(64 * ENC4_NW), 0,
                         s, feats, B, L.C, p.enc_w4, p.enc_w4h, p.enc_w4h_sc, p.enc_a_b, w.e.V, w.e.a_g, 1);
    } else {
      return false;
    }
    return true;
  };
  (void)t;
  if (!launch()) return -100;
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipEventRecord(e0, s);
  for (int i = 0; i < reps; ++i) launch();
  hipEventRecord(e1, s);
  hipEventSynchronize(e1);
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  *out_us = 1e3f * ms / reps;
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  return (int)hipGetLastError();
}
