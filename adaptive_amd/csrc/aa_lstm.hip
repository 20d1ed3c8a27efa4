// aa_lstm.hip — k_lstm's instantiations and their launch (aa_lstm.hpp has the kernel).  The Makefile
// compiles this file once per hidden size (-DAA_LSTM_H=256 / 512 / 768 / 1024), so the four objects
// build side by side and none is rebuilt for an edit elsewhere; without AA_LSTM_H (tools/kbench.hip,
// which includes the units into one) it holds all four sizes.
#include "aa_lstm.hpp"

namespace aa {

// In the single module all kernels once shared, exact_logit8 also had a caller with a run-time H
// (k_logits_at), so the compiler's interprocedural constant propagation left its H alone until it was
// inlined; here every caller passes this object's H, the propagation runs first, and k_lstm<.., RS> for
// H = 256 / 512 comes out with other instruction selection and more scratch.  This function, kept in
// the object but never called, is such a caller: with it the kernels compile to the same code as before.
__device__ __attribute__((used)) float exact_logit8_rt(const float* urow, const float* wrow, int H, float b, int lane8) {
  return exact_logit8(urow, wrow, H, b, lane8);
}

// LSTM step (GEMM + cell in one launch), shared by the step API, the greedy loop, beam search and
// sampling: io.par: beam search's gathering form; io.ra: step t-1's rescoring in the same launch;
// io.base: the baseline model's no-sentinel forms (H = 512, greedy: baseline_ok()); io.s is not written
template <int H>
void lstm_launch_h(const Layout& L, const MP& p, const StepIO& io, hipStream_t s) {
  const int B = io.B, MT = (B + 63) / 64;
  const RsArgs none{};
  const int64_t* tnull = nullptr;
#define AA_LSTM(G_, RS_, SENT_, GRID_, TOK_, LD_, RA_)                                                          \
  AA_TLAUNCH(io.lstm_ev, io.ei, (k_lstm<H, G_, RS_, SENT_>), dim3(GRID_), dim3(512), 0, s, B, L.V, TOK_, LD_, p.table, \
             io.xg, io.hsp_in, io.c_in, io.par, p.whh3, p.wgs, io.h_out, io.hsp_out, io.c_out, io.s, io.part, RA_)
  if constexpr (H == 512) {
    if (io.base) {
      if (io.ra) AA_LSTM(false, true, false, io.ra->NR + MT * (H / 16), tnull, 0, *io.ra);
      else AA_LSTM(false, false, false, MT * (H / 16), io.tok, io.tok_ld, none);
      return;
    }
  }
  if (io.par) AA_LSTM(true, false, true, MT * (H / 16), io.tok, io.tok_ld, none);
  else if (io.ra) AA_LSTM(false, true, true, io.ra->NR + MT * (H / 16), tnull, 0, *io.ra);
  else AA_LSTM(false, false, true, MT * (H / 16), io.tok, io.tok_ld, none);
#undef AA_LSTM
}

#ifdef AA_TS_ENABLE
template <int H>
int ts_set_lstm(void* buf) { return ts_set_local(buf); }
#define AA_LSTM_UNIT(H_) \
  template void lstm_launch_h<H_>(const Layout&, const MP&, const StepIO&, hipStream_t); \
  template int ts_set_lstm<H_>(void*);
#else
#define AA_LSTM_UNIT(H_) template void lstm_launch_h<H_>(const Layout&, const MP&, const StepIO&, hipStream_t);
#endif
#ifdef AA_LSTM_H
AA_LSTM_UNIT(AA_LSTM_H)
#else
AA_LSTM_UNIT(256) AA_LSTM_UNIT(512) AA_LSTM_UNIT(768) AA_LSTM_UNIT(1024)
#endif
#undef AA_LSTM_UNIT

}  // namespace aa
