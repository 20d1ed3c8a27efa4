/*
 * adaptive_amd.h — C-ABI of the MI355X-native adaptive-attention ("Knowing When to Look")
 * greedy-decode path.  Plain C: device pointers, sizes, opaque stream/event handles.
 *
 * The reference has no FFI: its boundary is the Python module API of
 *   code_src/models/adaptive_attention.py:159-216  (Encoder2Decoder, .sampler)
 *   code_src/models/baseline_attention.py:36-62    (AttentiveCNN.forward, the encoder tail)
 *   code_src/models/baseline_attention.py:148-194  (Decoder.forward, one step when T == 1)
 * Each entry point below names the reference interface it replaces.  The Python host layer
 * (adaptive_amd/adaptive_attention.py) binds them with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - All tensors are fp32 (ids int64), contiguous, row-major, caller-owned DEVICE memory.
 *  - No call allocates memory or synchronises the stream; scratch comes from a caller-provided
 *    workspace whose size is returned by the *_workspace_bytes queries.  Every launch goes to
 *    the given stream, so a caller may capture a call into a hipGraph.
 *  - Return value: 0 = success; negative = argument/shape error (see AA_ERR_*); positive = the
 *    hipError_t of a failed HIP call.  Nothing throws across the ABI.
 *  - Stateless and re-entrant: no hidden globals.
 *  - Load the library only after the process's HIP runtime is loaded (e.g. after `import torch`)
 *    so that one libamdhip64.so.7 serves both.
 */
#ifndef ADAPTIVE_AMD_H
#define ADAPTIVE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AA_ABI_VERSION 17
#define AA_API __attribute__((visibility("default")))

/* error codes (negative); positive codes are hipError_t values */
#define AA_OK 0
#define AA_ERR_NULL (-1)      /* a required pointer is NULL */
#define AA_ERR_DIMS (-2)      /* unsupported model dimensions */
#define AA_ERR_SHAPE (-3)     /* bad batch size / step count */
#define AA_ERR_BUFFER (-4)    /* packed-weight or workspace buffer too small */
#define AA_ERR_ALIGN (-5)     /* a pointer is not 16-byte aligned */

typedef void* aa_stream_t; /* hipStream_t (NULL = legacy default stream) */
typedef void* aa_event_t;  /* hipEvent_t */

/* Model dimensions: cf.adaptive_word_embed_size, cf.adaptive_lstm_hidden_size, cf.vocab_length
 * (code_src/config/cfg_wzn.py:115-116, code_src/train.py:40), ResNet channels and 7x7 locations.
 * Supported: embed % 32 == 0, hidden % 256 == 0 and <= 1024, vocab >= 1, channels % 32 == 0,
 * spatial == 49. */
typedef struct aa_dims {
  int32_t embed;    /* E = 256 */
  int32_t hidden;   /* H = 512 */
  int32_t vocab;    /* V = 10123 */
  int32_t channels; /* C = 2048 */
  int32_t spatial;  /* P = 49 */
} aa_dims;

/* Parameters in the reference state-dict layout (device pointers, fp32, contiguous).
 * Names follow Encoder2Decoder.state_dict() keys. */
typedef struct aa_ref_weights {
  const float* enc_affine_a_w;  /* encoder.affine_a.weight  [H, C] */
  const float* enc_affine_a_b;  /* encoder.affine_a.bias    [H]    */
  const float* enc_affine_b_w;  /* encoder.affine_b.weight  [E, C] */
  const float* enc_affine_b_b;  /* encoder.affine_b.bias    [E]    */
  const float* enc_affine_h0_w; /* encoder.affine_h0.weight [H, C] */
  const float* enc_affine_h0_b; /* encoder.affine_h0.bias   [H]    */
  const float* enc_affine_c0_w; /* encoder.affine_c0.weight [H, C] */
  const float* enc_affine_c0_b; /* encoder.affine_c0.bias   [H]    */
  const float* embed_w;         /* decoder.embed.weight     [V, E] */
  const float* lstm_w_ih;       /* decoder.LSTM.weight_ih_l0 [4H, 2E] (gates i,f,g,o) */
  const float* lstm_w_hh;       /* decoder.LSTM.weight_hh_l0 [4H, H]  */
  const float* lstm_b_ih;       /* decoder.LSTM.bias_ih_l0   [4H]     */
  const float* lstm_b_hh;       /* decoder.LSTM.bias_hh_l0   [4H]     */
  const float* sent_affine_x_w; /* decoder.adaptive.sentinel.affine_x.weight [H, 2E] */
  const float* sent_affine_h_w; /* decoder.adaptive.sentinel.affine_h.weight [H, H]
                                   (multiplies h_{t-1} = 0 while sampling; may be NULL) */
  const float* att_affine_v_w;  /* decoder.adaptive.atten.affine_v.weight [P, H] */
  const float* att_affine_g_w;  /* decoder.adaptive.atten.affine_g.weight [P, H] */
  const float* att_affine_s_w;  /* decoder.adaptive.atten.affine_s.weight [P, H] */
  const float* att_affine_h_w;  /* decoder.adaptive.atten.affine_h.weight [1, P] */
  const float* mlp_w;           /* decoder.adaptive.mlp.weight [V, H] */
  const float* mlp_b;           /* decoder.adaptive.mlp.bias   [V]    */
} aa_ref_weights;

/* Gradient outputs of aa_train_backward, same fields and shapes as aa_ref_weights. */
typedef struct aa_ref_grads {
  float* enc_affine_a_w;
  float* enc_affine_a_b;
  float* enc_affine_b_w;
  float* enc_affine_b_b;
  float* enc_affine_h0_w;
  float* enc_affine_h0_b;
  float* enc_affine_c0_w;
  float* enc_affine_c0_b;
  float* embed_w;
  float* lstm_w_ih;
  float* lstm_w_hh;
  float* lstm_b_ih;
  float* lstm_b_hh;
  float* sent_affine_x_w;
  float* sent_affine_h_w;
  float* att_affine_v_w;
  float* att_affine_g_w;
  float* att_affine_s_w;
  float* att_affine_h_w;
  float* mlp_w;
  float* mlp_b;
} aa_ref_grads;

/* A model = dims + a caller-owned device buffer holding the packed (kernel-layout) weights. */
typedef struct aa_model {
  aa_dims dims;
  void* packed;        /* device buffer, >= aa_packed_bytes(&dims) bytes, 256-B aligned */
  size_t packed_bytes;
} aa_model;

/* Optional per-kernel timing (hipEvent_t handles created by the caller), one array per kernel so
 * the figures line up with rocprofv3's per-kernel statistics.  For each non-NULL array, the pair
 * ([2i], [2i+1]) of the i-th launch of that kernel is handed to the launch itself
 * (hipExtLaunchKernel start / stop events): it carries the dispatch's own begin / end timestamps,
 * and no event packet sits between the traced launches:
 *   encoder_events: 2*AA_TRACE_ENCODER_KERNELS events, launches in the order
 *                   k_avgpool (not launched by k_enc_v4, which fuses it: pair 0 stays unrecorded),
 *                   k_enc_v, k_enc_heads, VWv GEMM, x_g GEMM;
 *   lstm/atten/screen/rescore_events: 2*T events, launch i = step i.  screen = k_vscreen2 /
 *                   k_vscreen (k_vocab under AA_DECODE_EXACT_VOCAB), rescore = k_vrescore (unused
 *                   under AA_DECODE_EXACT_VOCAB; by default only pair T-1 is recorded: the rescoring
 *                   of steps 0..T-2 runs inside the next step's LSTM launch); lstm = k_lstm (steps
 *                   >= 1 by default include the previous step's rescoring);
 *   gemm_events:    unused (kept for layout stability; may be NULL). */
#define AA_TRACE_ENCODER_KERNELS 5
typedef struct aa_trace {
  aa_event_t* encoder_events;
  aa_event_t* lstm_events;
  aa_event_t* atten_events;
  aa_event_t* screen_events;
  aa_event_t* rescore_events;
  aa_event_t* gemm_events;
} aa_trace;

AA_API int aa_abi_version(void);
AA_API const char* aa_error_string(int code);
AA_API int aa_check_dims(const aa_dims* dims);

/* Bytes of the packed weight buffer for these dims. */
AA_API size_t aa_packed_bytes(const aa_dims* dims);

/* Pack reference-layout weights into m->packed (device-side reorder; async on `stream`).
 * Replaces: the parameter set built by Encoder2Decoder.__init__ / load_state_dict
 * (adaptive_attention.py:159-165, model_factory.py:16).
 * Baseline model (baseline_attention.py:198-204, no visual sentinel): sent_affine_x_w and
 * att_affine_s_w both NULL (sent_affine_h_w too, it is never read).  The packed size and layout are
 * those of an adaptive model; the sentinel blocks stay zero.  One of the pair NULL without the other
 * is AA_ERR_NULL.  A model packed this way must be decoded with AA_DECODE_BASELINE /
 * aa_baseline_decode_step, an adaptive one without: nothing in the packed buffer records which it
 * is, and the wrong choice computes garbage silently. */
AA_API int aa_pack_weights(const aa_model* m, const aa_ref_weights* w, aa_stream_t stream);

/* Encoder tail: a_g = AvgPool2d(7)(A); V = relu(A^T W_a^T + b_a); v_g = relu(a_g W_b^T + b_b);
 * h0/c0 = tanh(a_g W^T + b); plus the step-invariant VWv = V W_v^T used by every decode step.
 * Replaces AttentiveCNN.forward after resnet_conv (baseline_attention.py:46-62).
 * feats: [B, C, 7, 7] NCHW post-trunk features.  Outputs: a_g [B,C], V [B,P,H], v_g [B,E],
 * h0 [B,H], c0 [B,H], VWv [B,P,64] (columns >= P are zero; may be NULL).  flags: 0 or
 * AA_DECODE_FP32_ENCODER or AA_DECODE_ENC_BF16X3. */
AA_API int aa_encoder_tail(const aa_model* m, const float* feats, int32_t B, float* a_g, float* V,
                           float* v_g, float* h0, float* c0, float* VWv, int32_t flags,
                           aa_stream_t stream);

/* Workspace for aa_decode_step at batch B. */
AA_API size_t aa_step_workspace_bytes(const aa_dims* dims, int32_t B);

/* One greedy decode step = Decoder.forward with T == 1 (baseline_attention.py:148-194) through
 * AdaptiveBlock (adaptive_attention.py:110-134) and the argmax of Encoder2Decoder.sampler (:201).
 * tokens_in [B] int64 (NULL = <start> = 1); VWv from aa_encoder_tail (may be NULL: recomputed);
 * h_in/c_in [B,H] -> h_out/c_out [B,H]; scores [B,V] (NULL = not written); tokens_out [B] int64
 * (first index on ties); alpha [B,P]; beta [B].  h_out/c_out must not alias h_in/c_in. */
AA_API int aa_decode_step(const aa_model* m, int32_t B, const int64_t* tokens_in, const float* V,
                          const float* VWv, const float* v_g, const float* h_in, const float* c_in,
                          float* h_out, float* c_out, float* scores, int64_t* tokens_out,
                          float* alpha, float* beta, void* workspace, size_t workspace_bytes,
                          aa_stream_t stream);

/* aa_decode_step for a baseline-packed model (see aa_pack_weights): Decoder.forward with T == 1
 * (baseline_attention.py:148-194) through the baseline AdaptiveBlock (:116-128) -- alpha = the
 * 49-way softmax, scores = mlp(c_t + h) -- and the argmax of its sampler (:267), on the no-sentinel
 * kernels.  Arguments as aa_decode_step without beta; workspace from aa_step_workspace_bytes.
 * hidden == 512 only (else AA_ERR_DIMS). */
AA_API int aa_baseline_decode_step(const aa_model* m, int32_t B, const int64_t* tokens_in,
                                   const float* V, const float* VWv, const float* v_g,
                                   const float* h_in, const float* c_in, float* h_out, float* c_out,
                                   float* scores, int64_t* tokens_out, float* alpha, void* workspace,
                                   size_t workspace_bytes, aa_stream_t stream);

/* Workspace for aa_greedy_decode at batch B and T steps. */
AA_API size_t aa_decode_workspace_bytes(const aa_dims* dims, int32_t B, int32_t T);

/* Decode flags */
#define AA_DECODE_EXACT_VOCAB 1 /* compute every fp32 logit (fp32 MFMA GEMM + fused argmax) instead of
                                   the bf16 screen + exact fp32 rescoring; both give the same ids */
#define AA_DECODE_FP32_ENCODER 2 /* V = relu(A W_a^T + b) on fp32 MFMA (v_mfma_f32_32x32x2f32) instead of
                                    the default fp32-accurate split-operand MFMA (k_enc_v4: 2-way fp16
                                    split, 3-way bf16 split for out-of-range features and in k_enc_v3) */
#define AA_DECODE_ONE_STREAM 512 /* decode plans: capture the whole decode on one stream (no side-stream
                                     branch for the encoder's a_g work); for several plans in flight */
#define AA_DECODE_SPLIT_RESCORE 1024 /* rescore each step in its own launch (k_vrescore) instead of inside
                                        the next step's LSTM launch; the same ids (cross-check path) */
#define AA_DECODE_RS_SELF 2048 /* test hook: the LSTM workgroups do not wait for the rescoring workgroups
                                  of their launch but rescore every row not yet published themselves
                                  (the fallback that keeps the fused launch deadlock-free); same ids */
#define AA_DECODE_SCREEN4 4096 /* the vocab screen on four waves per 128 x 160 tile (k_vscreen2) instead
                                  of eight (k_vscreen8); the same summaries bit for bit (cross-check) */
#define AA_DECODE_BASELINE 8192 /* the model is a baseline (no-sentinel) model, packed with
                                   sent_affine_x_w == att_affine_s_w == NULL: the decode is
                                   baseline_attention.py's sampler (:233-280) on the no-sentinel kernels;
                                   beta is neither read nor written (pass NULL); workspace size and layout
                                   unchanged; hidden == 512 only (else AA_ERR_DIMS); composes with every
                                   flag above.  The flag MUST match how the model was packed: a
                                   baseline-packed model decoded without it (or an adaptive one with it)
                                   computes garbage silently. */
#define AA_DECODE_ENC_BF16X3 16384 /* test hook: every k_enc_v4 workgroup computes V with the 3-way bf16
                                      split (six products) instead of the default 2-way fp16 split (three),
                                      i.e. the body a workgroup whose features leave the fp16 path's range
                                      falls back to; a_g is bit-identical, V agrees to fp32-GEMM accuracy */

/* Whole greedy decode = Encoder2Decoder.sampler(images, max_len=T) (adaptive_attention.py:168-216,
 * with the baseline's states transpose, baseline_attention.py:251-252).  feats [B,C,7,7];
 * ids [B,T] int64; alpha [B,T,P] and beta [B,T] may be NULL.  All T steps run (no early stop),
 * the first input token is <start> = 1.  trace may be NULL.
 * Vocab argmax (adaptive_attention.py:201): by default every logit is first bounded with a bf16
 * MFMA screen whose error is bounded rigorously (Cauchy-Schwarz on the rounding-error vectors of u
 * and w_n plus the fp32 accumulation terms, per 32-column granule);
 * only columns whose upper bound reaches the best lower bound are rescored in exact fp32 (the same
 * fma order as the fp32 GEMM), so the ids equal those of AA_DECODE_EXACT_VOCAB bit for bit. */
AA_API int aa_greedy_decode(const aa_model* m, const float* feats, int32_t B, int32_t T,
                            int64_t* ids, float* alpha, float* beta, void* workspace,
                            size_t workspace_bytes, const aa_trace* trace, int32_t flags,
                            aa_stream_t stream);

/* aa_greedy_decode with a second stream `aux_stream` for the encoder's a_g branch (heads, x_g GEMM)
 * beside the V branch's VWv GEMM.  Fork/join through events: the call is complete (and
 * graph-capturable) on `stream`.  aux_stream NULL or equal to `stream`: aa_greedy_decode.  The
 * results equal aa_greedy_decode's bit for bit. */
AA_API int aa_greedy_decode_aux(const aa_model* m, const float* feats, int32_t B, int32_t T,
                                int64_t* ids, float* alpha, float* beta, void* workspace,
                                size_t workspace_bytes, const aa_trace* trace, int32_t flags,
                                aa_stream_t stream, aa_stream_t aux_stream);

/* Decode plan: the complete greedy decode for fixed (B, T, flags) and fixed buffers, captured once
 * into a hipGraph (one graph launch replaces the ~4T+6 kernel launches).  Launch it as often as
 * needed on any stream; the buffers it was created with -- feats included -- are read/written at
 * every launch, so the caller owns them for the plan's lifetime (adaptive_amd.DecodePlan owns its
 * own input buffer and copies each batch into it).  Results equal aa_greedy_decode's bit for bit.
 * The plan captures aa_greedy_decode_aux's two-stream encoder unless flags &
 * AA_DECODE_ONE_STREAM.  It holds no device memory of its own besides the instantiated graph;
 * destroy it only after its last launch has completed. */
typedef struct aa_decode_plan aa_decode_plan;
AA_API int aa_decode_plan_create(const aa_model* m, const float* feats, int32_t B, int32_t T,
                                 int64_t* ids, float* alpha, float* beta, void* workspace,
                                 size_t workspace_bytes, int32_t flags, aa_decode_plan** plan);
AA_API int aa_decode_plan_launch(const aa_decode_plan* plan, aa_stream_t stream);
AA_API int aa_decode_plan_destroy(aa_decode_plan* plan);

/* ---- teacher-forced training step ----------------------------------------
 * Encoder2Decoder.forward(images, captions, lengths) (baseline_attention.py:206-230) and its
 * backward, fp32, deterministic.  feats [B,C,7,7]; tokens: captions [B][tok_ld] int64 (column t is
 * the input token of step t, <start> first); lengths: DEVICE int32 [B], sorted descending (as
 * pack_padded_sequence requires), T = lengths[0] steps, N = sum(lengths) packed rows.
 * aa_train_forward writes the packed scores [N][V] (pack_padded_sequence(scores, lengths).data:
 * rows t-major over the batch entries still running at step t) and keeps the activations in the
 * workspace; aa_train_backward takes dL/dscores [N][V] with the same arguments and workspace and
 * writes the gradient of every parameter (assigned, not accumulated), and, if dfeats is not NULL,
 * dL/dfeats [B,C,7,7] (the gradient into the ResNet trunk's output, for CNN fine-tuning).  The reference's loss
 * (train.py: CrossEntropyLoss on the packed scores) stays with the caller.  Token ids are not
 * validated on the device: the caller must keep them in [0, V) (the Python layer raises IndexError
 * as nn.Embedding does); an out-of-range id is clamped into [0, V) by the gather (no out-of-bounds
 * read) and then feeds the wrong embedding row. */
AA_API size_t aa_train_workspace_bytes(const aa_dims* dims, int32_t B, int32_t T);
#define AA_TRAIN_BF16 128 /* aa_train_forward / aa_train_backward flags: every GEMM on bf16 MFMA
                               (operands rounded to bf16, fp32 accumulation; BASELINE config 5's
                               "bf16 compute / fp32 master"); elementwise work and the encoder V GEMM
                               stay fp32.  0 = fp32 GEMMs (fp32 MFMA).  Pass the same flags to both. */
#define AA_TRAIN_SENTINEL_H0 64 /* the sentinel gate sigma(W_x x_t) without its h_{t-1} W_h term at every
                               step, as the one-token decode step computes it (the reference's sampler
                               calls Decoder.forward per token, which starts h_{t-1} from zeros each
                               time): the forward then reproduces the distribution aa_sample_decode /
                               aa_greedy_decode draw from; the gradient of sent_affine_h_w is written as
                               zeros.  Also accepted by aa_decoder_forward.  Pass the same flags to both. */
AA_API int aa_train_forward(const aa_ref_weights* w, const aa_dims* dims, const float* feats, int32_t B,
                            int32_t T, const int64_t* tokens, int32_t tok_ld, const int32_t* lengths,
                            float* scores, int32_t N, void* workspace, size_t workspace_bytes,
                            int32_t flags, aa_stream_t stream);
AA_API int aa_train_backward(const aa_ref_weights* w, const aa_dims* dims, const float* feats,
                             int32_t B, int32_t T, const int64_t* tokens, int32_t tok_ld,
                             const int32_t* lengths, const float* dscores, int32_t N,
                             const aa_ref_grads* grads, float* dfeats, void* workspace,
                             size_t workspace_bytes, int32_t flags, aa_stream_t stream);
/* The same two calls with a second stream `aux` (another stream of the same device, or NULL = one
 * stream): the work off the step's dependency chain -- the encoder's spatial V GEMM beside the LSTM
 * forward, the weight gradients beside the LSTM backward -- runs on aux, handed over by events.
 * Results are bit-identical to the one-stream calls (same kernels, same arithmetic order); both
 * calls end with `stream` waiting for everything they queued on aux, so the caller orders only
 * against `stream`.  aux must not be used by anything else during a call. */
AA_API int aa_train_forward_aux(const aa_ref_weights* w, const aa_dims* dims, const float* feats, int32_t B,
                                int32_t T, const int64_t* tokens, int32_t tok_ld, const int32_t* lengths,
                                float* scores, int32_t N, void* workspace, size_t workspace_bytes, int32_t flags,
                                aa_stream_t stream, aa_stream_t aux);
AA_API int aa_train_backward_aux(const aa_ref_weights* w, const aa_dims* dims, const float* feats, int32_t B,
                                 int32_t T, const int64_t* tokens, int32_t tok_ld, const int32_t* lengths,
                                 const float* dscores, int32_t N, const aa_ref_grads* grads, float* dfeats,
                                 void* workspace, size_t workspace_bytes, int32_t flags, aa_stream_t stream,
                                 aa_stream_t aux);

/* ---- Decoder.forward over T > 1 teacher-forced steps -------------------------------------------
 * decoder(V, v_g, captions, states) (baseline_attention.py:148-194 with the adaptive block,
 * adaptive_attention.py:110-134; called with whole captions from Encoder2Decoder.forward, :225):
 * V [B,P,H], v_g [B,E], h0 / c0 [B,H] (the states, any of the [1,B,H] / [B,1,H] views of one
 * contiguous buffer), tokens [B][tok_ld] int64 (column t feeds step t).  Every row runs all T steps
 * (no packing); the sentinel's h_{t-1} is 0 at t = 0 (init_hidden, :116-120).  Outputs (each may be
 * NULL): scores [B,T,V], alpha [B,T,P], beta [B,T], h_out / c_out [B,H] = the states after step
 * T-1.  Forward only (the training path with gradients is aa_train_forward/backward); flags:
 * AA_TRAIN_BF16 or 0 as for aa_train_forward.  Workspace: aa_decoder_workspace_bytes.  Token ids:
 * the caller keeps them in [0, V), as for aa_train_forward (out-of-range ids are clamped, not
 * reported). */
AA_API size_t aa_decoder_workspace_bytes(const aa_dims* dims, int32_t B, int32_t T);
AA_API int aa_decoder_forward(const aa_ref_weights* w, const aa_dims* dims, const float* V, const float* v_g,
                              const float* h0, const float* c0, int32_t B, int32_t T, const int64_t* tokens,
                              int32_t tok_ld, float* scores, float* alpha, float* beta, float* h_out,
                              float* c_out, void* workspace, size_t workspace_bytes, int32_t flags,
                              aa_stream_t stream);

/* ---- beam-search decode (BASELINE config 4) ------------------------------
 * Not in the reference (its for_wzn:3 lists beam search as a TODO): semantics defined here and in
 * oracle/adaptive_oracle.py BeamOracle.  K (1..AA_MAX_BEAM) hypotheses per image over the same
 * decoder step as aa_greedy_decode; at step 0 only beam 0 is live; a candidate's score is the
 * parent's cumulative score + log_softmax(logits) of the token; a beam that emitted end_id is
 * finished and carried unchanged (its only continuation is end_id at no cost; end_id < 0: none);
 * the K best candidates per image (score desc, ties to the smaller parent*V + token) survive.
 * All T steps run.  Outputs (each may be NULL): ids [B,T] int64, alpha [B,T,P], beta [B,T] of the
 * best final beam; seqs [B,K,T] int64 and scores [B,K] of all K final beams, best first.
 * Logits (default): exact fp32 -- the fma chains of aa_vocab_logits' fp32 MFMA GEMM, so the same
 * bits -- with per-32-column (max, sum exp(x - max)) summaries in a fixed butterfly order fused into
 * the GEMM epilogue (one launch per step); the selection builds each row's log-sum-exp from them.
 * flags & AA_DECODE_EXACT_VOCAB: the same values by two launches (the plain fp32 GEMM, then the
 * summaries) -- the cross-check path, bitwise equal to the default.  flags & AA_BEAM_FAST: the logits by bf16x3
 * MFMA (fp32-accurate but rounded differently) with the summaries fused into the GEMM epilogue --
 * about 2.3x faster, and the beams equal the exact ones except where two candidates are within the
 * logits' rounding difference of each other (measured: >= 98% of images at config 4).
 * Requires vocab <= 16384.  Replaces, for beam decoding, the greedy sampler's role in coco_eval
 * (code_src/tools/utils.py:171).  vocab_events (may be NULL): 2T hipEvent handles recorded on the
 * stream around each step's vocab stage (logits + summaries), for per-launch timing. */
#define AA_MAX_BEAM 8
#define AA_BEAM_FAST 256 /* aa_beam_decode: bf16x3 logits with fused summaries instead of exact fp32 */
AA_API size_t aa_beam_workspace_bytes(const aa_dims* dims, int32_t B, int32_t T, int32_t K);
AA_API int aa_beam_decode(const aa_model* m, const float* feats, int32_t B, int32_t T, int32_t K,
                          int32_t end_id, int64_t* ids, int64_t* seqs, float* scores, float* alpha,
                          float* beta, void* workspace, size_t workspace_bytes, int32_t flags,
                          aa_stream_t stream, aa_event_t* vocab_events);

/* ---- diverse beam groups and a length-normalised final ranking ----------------------------------
 * Additions to the beam decode; aa_beam_decode keeps its signature and behaviour (it is
 * aa_beam_decode_ex with opts == NULL).  Semantics defined here and in tests/beam_div_oracle.py.
 * groups = G divides K (Kg = K / G): group g owns the slots g Kg .. (g + 1) Kg - 1 of an image, and a
 * beam's parent is always in its own group.  Per step the raw candidates are aa_beam_decode's (the
 * same fp32 expression on the same logits; a finished beam's single carry-over end_id at its unchanged
 * score), except that at step 0 slot 0 of every group is live.  The groups select in order g = 0 ..
 * G - 1 over a per-image token count n[v] that starts at 0 every step (Hamming diversity, Vijayakumar
 * et al.): group g ranks its Kg V candidates by raw - diversity * n[v] in fp32 (a carry-over is never
 * penalised), descending, ties to the smaller q V + v with q the parent's slot in the image; the best
 * Kg survive into the group's slots in that order, each with its raw score as the new cumulative
 * score (the penalty steers the selection only); then n[v] += 1 for every survivor that newly emitted
 * v (carry-overs do not count).
 * Final ranking: len = the position of the beam's first end_id + 1, or T without one (always T when
 * end_id < 0); rank = cum / len^length_penalty in fp32; the K beams of an image come out by rank
 * descending, ties to the lower slot.  seqs and scores (the raw cum) are in that order, ids / alpha /
 * beta follow the first, and lengths / rank_scores / group ([B,K], each may be NULL) give every
 * beam's len, rank and group in the same order.
 * groups = 1, diversity = 0, length_penalty = 0 is aa_beam_decode's result, by other kernels.  With
 * diversity = 0 the beams of group g, in rank order, are those of a K / G-beam decode.
 * The vocabulary stages (default, AA_DECODE_EXACT_VOCAB, AA_BEAM_FAST) and the workspace
 * (aa_beam_workspace_bytes) are aa_beam_decode's.  Checks: as aa_beam_decode, and before the B == 0 /
 * T == 0 return AA_ERR_SHAPE for groups < 1, K % groups != 0, or a diversity or length_penalty that
 * is negative or not finite. */
typedef struct aa_beam_opts {
  int32_t groups;       /* >= 1, divides K */
  float diversity;      /* >= 0; 0: off */
  float length_penalty; /* >= 0; 0: rank by the raw score */
  int32_t* lengths;     /* [B, K] or NULL */
  float* rank_scores;   /* [B, K] or NULL */
  int32_t* group;       /* [B, K] or NULL */
} aa_beam_opts;
AA_API int aa_beam_decode_ex(const aa_model* m, const float* feats, int32_t B, int32_t T, int32_t K,
                             int32_t end_id, int64_t* ids, int64_t* seqs, float* scores, float* alpha,
                             float* beta, void* workspace, size_t workspace_bytes, int32_t flags,
                             aa_stream_t stream, aa_event_t* vocab_events, const aa_beam_opts* opts);

/* ---- constrained beam search: suppressed tokens, minimum length, no repeated n-grams ------------
 * Additions to the beam decode; aa_beam_decode and aa_beam_decode_ex keep their signatures and
 * behaviour.  Semantics defined here and in tests/beam_cons_oracle.py.  Take a live (unfinished)
 * hypothesis at step t with its own tokens y_0 .. y_{t-1} (traced through its parents; <start> is not
 * among them) and y_{-1} = 1 (<start>).  Candidate token v is forbidden iff
 *   1. v is in suppress_ids;
 *   2. v == end_id and t < min_length (a caption has min_length tokens before <end>; with
 *      min_length >= T no beam finishes);
 *   3. v == end_id and y_{t-1} is in no_end_after (no <end> right after "a", "the", "with", ...);
 *   4. n = no_repeat_ngram >= 1 and some j in [n-1, t-1] has (y_{j-n+1} .. y_{j-1}) ==
 *      (y_{t-n+1} .. y_{t-1}) and v == y_j: v would complete an n-gram the hypothesis already
 *      contains (n = 1: any token it emitted).  A live hypothesis holds no end_id, so rule 4 never
 *      forbids end_id.
 * A forbidden candidate takes no part in the selection.  Everything else is aa_beam_decode_ex's: a
 * finished beam keeps its single carried end_id at its unchanged score (no constraint applies to it);
 * step-0 liveness, the groups' order under raw - diversity * n[v], the tie order and the final
 * ranking are unchanged.  No renormalisation: a surviving candidate's score is the parent's score +
 * log_softmax over the full vocabulary -- the same fp32 expression on the same logits and the same
 * log-sum-exp from the same granule summaries -- so scores stay the model's log-probabilities, and a
 * call whose constraints never bind returns the unconstrained call's bits.  Sampling, the greedy
 * decode, renormalised and forced-word constraints are out of scope (constrained greedy is K = 1).
 * The id arrays are device memory, int32, with duplicates allowed.  cons == NULL, or all four off, is
 * aa_beam_decode_ex (opts == NULL as well: aa_beam_decode): the same kernels, the same bits.  The
 * workspace is aa_beam_workspace_bytes'.
 * Checks: as aa_beam_decode_ex, and before the B == 0 / T == 0 return AA_ERR_SHAPE for a list count
 * outside [0, AA_MAX_BEAM_SUPPRESS], min_length < 0, no_repeat_ngram < 0, min_length > 0 or a
 * non-empty no_end_after with end_id < 0, no_repeat_ngram > 0 with T > AA_MAX_BEAM_NGRAM_T (the rows'
 * histories are staged in LDS), and V - n_suppress - 1 - (no_repeat_ngram ? T : 0) < K (every live
 * row keeps K allowed candidates: the selection never runs dry).  A NULL list with a count > 0 is
 * AA_ERR_NULL, with the other pointers.  The ids themselves cannot be checked without reading
 * device memory: the caller keeps them inside [0, vocab) and end_id out of suppress_ids
 * (Encoder2Decoder.beam_search raises ValueError); the kernel ignores an id outside [0, vocab) and
 * an end_id among suppress_ids. */
#define AA_MAX_BEAM_SUPPRESS 64
#define AA_MAX_BEAM_NGRAM_T 256
typedef struct aa_beam_constraints {
  const int32_t* suppress_ids; /* [n_suppress], device memory */
  int32_t n_suppress;
  int32_t min_length;      /* 0: off */
  int32_t no_repeat_ngram; /* 0: off */
  const int32_t* no_end_after; /* [n_no_end_after], device memory */
  int32_t n_no_end_after;
} aa_beam_constraints;
AA_API int aa_beam_decode_cx(const aa_model* m, const float* feats, int32_t B, int32_t T, int32_t K,
                             int32_t end_id, int64_t* ids, int64_t* seqs, float* scores, float* alpha,
                             float* beta, void* workspace, size_t workspace_bytes, int32_t flags,
                             aa_stream_t stream, aa_event_t* vocab_events, const aa_beam_opts* opts,
                             const aa_beam_constraints* cons);

/* One step's selection on caller-supplied logits [R, Vp] fp32, R = B K rows (row b K + k is slot k of
 * image b; columns V .. Vp - 1 take no part): the selection apart from the model, as aa_sample_select
 * is for sampling.  The rows are at step t of a decode: cum [R] and fin [R] int32 are their scores and
 * finished flags, hist_tok / hist_par [t, R] int32 the tokens and parent slots (0 .. K - 1) of steps
 * 0 .. t - 1 as the decode keeps them (may be NULL when t == 0).  Computes the granule summaries
 * (k_gsumm), then runs the step's selection kernel once -- the one aa_beam_decode (opts == NULL),
 * aa_beam_decode_ex or, with a constraint set, aa_beam_decode_cx launches -- and writes tok [R] int64,
 * par [R] int32 (the parent's row b K + q), cum_out [R] and fin_out [R] (each may alias its input).
 * opts: groups and diversity are read.
 * Checks: AA_ERR_SHAPE for B < 0, K outside [1, AA_MAX_BEAM], B K > 2^24, V outside [1, 16384], K > V,
 * Vp < V, Vp % 32 != 0 or Vp > 16384, t outside [0, 2^20], end_id >= V, the options as aa_beam_decode_ex and the
 * constraints as aa_beam_decode_cx with t in place of T; B == 0 returns AA_OK; then NULL pointers,
 * AA_ERR_ALIGN unless logits and workspace are 16-byte aligned, AA_ERR_BUFFER below
 * aa_beam_select_step_workspace_bytes (0 for arguments the call refuses). */
AA_API size_t aa_beam_select_step_workspace_bytes(int32_t B, int32_t K, int32_t V, int32_t Vp, int32_t t);
AA_API int aa_beam_select_step(int32_t B, int32_t K, int32_t V, int32_t Vp, int32_t t, int32_t end_id,
                               const float* logits, const float* cum, const int32_t* fin,
                               const int32_t* hist_tok, const int32_t* hist_par, const aa_beam_opts* opts,
                               const aa_beam_constraints* cons, int64_t* tok, int32_t* par, float* cum_out,
                               int32_t* fin_out, void* workspace, size_t workspace_bytes, aa_stream_t stream);

/* ---- seeded temperature-sampling decode ---------------------------------------------------------
 * Not in the reference: semantics defined here and in tests/sample_oracle.py SampleOracle.  One
 * caption per image drawn from the model's own distribution by Gumbel-max over the exact fp32 logits
 * (aa_beam_decode's default logits), the same decoder step as aa_greedy_decode, from <start> = 1; all
 * T steps run (no <end> handling).  At step t, image b, with x[v] the logits (v < vocab):
 *   y[v]  = x[v] / temperature                                    (fp32)
 *   e     = ((row0 + b) * T + t) * vocab + v                      (64-bit element counter)
 *   u     = (2 * (splitmix64(key + (e + 1) * GOLDEN) >> 41) + 1) * 2^-24    (exact, inside (0, 1))
 *   g     = -log(-log(u))
 *   token = argmax_v (y[v] + g), ties to the smaller v; it is the input of step t + 1
 *   logp  = y[token] - (max y + log sum exp(y - max y))           (tempered log-probability)
 * key: the stream key (adaptive_amd.synth.stream_key(seed, "sample")); GOLDEN = 0x9E3779B97F4A7C15,
 * splitmix64 as in aa_synth_uniform.  The same (key, row0, T) gives the same output bit for bit, and
 * an image's draw depends only on its global row row0 + b: a batch sharded by rows (each shard with its
 * row0) samples what the whole batch would.
 * Outputs: ids [B,T] int64 and logp [B,T] (required); alpha [B,T,P] and beta [B,T] may be NULL.
 * Checks, in aa_beam_decode's order: model (NULL / dims / buffer / alignment), vocab <= 16384 (else
 * AA_ERR_DIMS), then AA_ERR_SHAPE for B < 0, T < 0, a temperature that is not finite and > 0, row0 < 0
 * or any flag other than AA_DECODE_FP32_ENCODER (AA_DECODE_BASELINE included: there are no no-sentinel
 * kernels on this path); then B == 0 or T == 0 returns AA_OK before any pointer is looked at; then
 * AA_ERR_SHAPE if (row0 + B) * T * vocab exceeds 2^62, NULL pointers, alignment, workspace size.
 * select_events (may be NULL): 2T hipEvent handles, pair t handed to step t's selection launch
 * (k_sample_select), for per-launch timing. */
AA_API size_t aa_sample_workspace_bytes(const aa_dims* dims, int32_t B, int32_t T);
AA_API int aa_sample_decode(const aa_model* m, const float* feats, int32_t B, int32_t T, float temperature,
                            uint64_t key, int64_t row0, int64_t* ids, float* logp, float* alpha,
                            float* beta, void* workspace, size_t workspace_bytes, int32_t flags,
                            aa_stream_t stream, aa_event_t* select_events);

/* ---- truncated sampling (top-k / nucleus) and N draws per image --------------------------------
 * Additions to the sampling decode; aa_sample_decode keeps its signature and behaviour (it is
 * aa_sample_decode_ex with opts == NULL).  Semantics defined here and in tests/sample_trunc_oracle.py.
 * Per row and step, with y[v] = x[v] / temperature (fp32, as above), m = max y, e_v = exp(y_v - m):
 *   top-k   S_k = { v : #{ w : y_w > y_v } < top_k }: a token stays unless at least top_k tokens are
 *           strictly better; the ties at the k-th value all stay, so |S_k| may exceed top_k.
 *           top_k == 0 or top_k >= vocab: off (S_k is every token).
 *   top-p   on the distribution renormalised over S_k: Z_k = sum_{S_k} e_v, G(v) = sum_{w in S_k,
 *           y_w > y_v} e_w (the mass strictly above v), S = { v in S_k : G(v) < p Z_k }, p = top_p as
 *           fp32, 0 < p <= 1.  p == 1 is off -- a rule, not a computation: an e_v that underflows
 *           cannot drop a token.  The comparison is made on integers: masses floor(e_v 2^40) with
 *           e_v = expf(y_v - m), summed in 64 bits, against ceil(p Z_k) (p taken as its exact binary
 *           fraction).
 *   hence   S = { v : y_v >= theta }, theta = min_{v in S} y_v: tie groups are kept or dropped
 *           whole, and the arg-max of y is always in S (-0 and +0 are one value).
 *   token = argmax_{v in S} (y_v + g_v), ties to the smaller v; g_v is the noise of the untruncated
 *           decode, from the same element counter: the noise of a column does not depend on S.
 *   logp  = y_token - (m + log sum_{v in S} e_v): the log-probability under the truncated,
 *           renormalised distribution.
 * With both truncations off the untruncated selection kernel runs unchanged: the same bits as
 * aa_sample_decode.  top_k = 1 at temperature 1 gives the ids of the exact-vocab greedy decode,
 * logp == 0 exactly and kept == 1.  Results are bit-reproducible and a row's depend on no other row.
 * num_samples = N: N rows per image over one encoder pass (the images' V is stored and read once
 * per image, as for the beams of aa_beam_decode).  Outputs have B N rows, image-major (row b N + n),
 * and equal bit for bit the decode of the images repeated N times each (repeat_interleave) with
 * row0 N in place of row0: row0 keeps counting images, so a shard of images 5..8 with row0 = 5
 * reproduces rows 5N .. 9N - 1 of the whole batch.
 * kept / theta (may be NULL): |S| as int32 and theta as fp32, [B N, T].
 * Checks: as aa_sample_decode, and before the B == 0 / T == 0 return AA_ERR_SHAPE for top_k < 0,
 * top_p not in (0, 1] (NaN included), num_samples < 1 or B N > 2^24; the counter bound is
 * (row0 + B) N T vocab <= 2^62.  The workspace is aa_sample_workspace_bytes_ex's (encoder outputs
 * for B images; row state, logits and tokens for B N rows; 0 for arguments the decode refuses). */
typedef struct aa_sample_opts {
  int32_t top_k;       /* 0: off */
  float top_p;         /* 1: off */
  int32_t num_samples; /* >= 1 */
  int32_t* kept;       /* [B N, T] or NULL */
  float* theta;        /* [B N, T] or NULL */
} aa_sample_opts;
AA_API size_t aa_sample_workspace_bytes_ex(const aa_dims* dims, int32_t B, int32_t T, int32_t num_samples);
AA_API int aa_sample_decode_ex(const aa_model* m, const float* feats, int32_t B, int32_t T, float temperature,
                               uint64_t key, int64_t row0, int64_t* ids, float* logp, float* alpha,
                               float* beta, void* workspace, size_t workspace_bytes, int32_t flags,
                               aa_stream_t stream, aa_event_t* select_events, const aa_sample_opts* opts);

/* One step's selection on caller-supplied logits [R, Vp] (columns V .. Vp - 1 take no part): what
 * aa_synth_gumbel is to the noise, the selection apart from the model.  Row r is global row row0 + r
 * of a T-step decode at step t (element counter ((row0 + r) T + t) V + v).  Writes tok[r] (int64
 * [R]) and column t of ids [R, T] int64, logp [R, T] and, when not NULL, kept [R, T] int32 and
 * theta [R, T].  With both truncations off it runs the untruncated selection kernel (kept = V,
 * theta = min y).  AA_ERR_SHAPE for R < 0 or > 2^24, V outside [1, 16384], Vp < V, T < 1, t outside
 * [0, T), a temperature that is not finite and > 0, row0 < 0, top_k < 0, top_p not in (0, 1], or
 * (row0 + R) T V > 2^62; R == 0 returns AA_OK; then NULL logits / tok / ids / logp. */
AA_API int aa_sample_select(const float* logits, int32_t R, int32_t V, int32_t Vp, int32_t T, int32_t t,
                            float temperature, uint64_t key, int64_t row0, int32_t top_k, float top_p,
                            int64_t* tok, int64_t* ids, float* logp, int32_t* kept, float* theta,
                            aa_stream_t stream);

/* The sampling decode's noise on its own (same values as adaptive_amd.synth.gumbel_f32 up to the
 * rounding of two logf): dst[i] = g of element counter start + i, i < n, as defined above. */
AA_API int aa_synth_gumbel(float* dst, int64_t n, uint64_t key, int64_t start, aa_stream_t stream);

/* Full fp32 vocab logits scores[B,V] = u W_m^T + b_m (AdaptiveBlock.mlp, adaptive_attention.py:132)
 * for given u = c_hat + h rows [B,H] (fp32 MFMA GEMM). */
AA_API int aa_vocab_logits(const aa_model* m, int32_t B, const float* u, float* scores,
                           aa_stream_t stream);

/* Exact fp32 vocab logits of selected columns: out[b][i] = u[b] . W_m[cols[b][i]] + b_m[cols[b][i]]
 * (AdaptiveBlock.mlp, adaptive_attention.py:132), computed in the fma order of the fp32 GEMM path,
 * i.e. bit-identical to the corresponding aa_decode_step scores.  u [B,H]; cols [B,n] int32
 * (entries outside [0, vocab) give 0); out [B,n].  Used to rescore candidate tokens. */
AA_API int aa_vocab_logits_at(const aa_model* m, int32_t B, const float* u, const int32_t* cols,
                              int32_t n, float* out, aa_stream_t stream);

/* ---- the rest of train.py's closure: CrossEntropyLoss and Adam ------------
 * aa_cross_entropy_forward: nn.CrossEntropyLoss()(logits, targets) (train.py:63,208; reduction
 * 'mean', ignore_index as torch's, default -100): logits [N][ldx] fp32 (V used columns), targets [N]
 * int64; writes loss[0] = mean over counted rows of (logsumexp(x_i) - x_i[t_i]) and count[0] = the
 * number of counted rows (as float), and keeps the per-row log-sum-exp in the workspace
 * (aa_cross_entropy_workspace_bytes(N)) for the backward.  A target outside [0, V) that is not
 * ignore_index makes the loss NaN (torch raises a device-side assert).  Deterministic (fixed-order
 * reductions).  aa_cross_entropy_backward: dlogits = (softmax(x_i) - onehot(t_i)) * dloss[0] /
 * count[0] (0 for ignored rows), dloss a DEVICE scalar (the incoming gradient of the loss), with the
 * forward's workspace (workspace_bytes >= aa_cross_entropy_workspace_bytes(N), else AA_ERR_BUFFER);
 * dlogits may alias logits (in place) only if lddx == ldx (else AA_ERR_SHAPE). */
AA_API size_t aa_cross_entropy_workspace_bytes(int32_t N);
AA_API int aa_cross_entropy_forward(const float* logits, int32_t N, int32_t V, int64_t ldx,
                                    const int64_t* targets, int64_t ignore_index, float* loss,
                                    float* count, void* workspace, size_t workspace_bytes,
                                    aa_stream_t stream);
AA_API int aa_cross_entropy_backward(const float* logits, int32_t N, int32_t V, int64_t ldx,
                                     const int64_t* targets, int64_t ignore_index, const float* dloss,
                                     const float* count, const void* workspace, size_t workspace_bytes,
                                     float* dlogits, int64_t lddx, aa_stream_t stream);

/* ---- the policy-gradient (self-critical) loss over sampled captions trained at the full length T ----
 * logits [T R][ldx] fp32, t-major: row t R + r is caption r at step t (the packed scores of
 * aa_train_forward when every length is T); ids [R][ids_ld] int64 the sampled tokens; advantage [R].
 *   live(r, t) = no end_id among ids[r][0 .. t-1] (the <end> token itself is trained; end_id < 0: every
 *                position is live); each workgroup finds it from the ids, no extra launch
 *   y          = x / temperature (fp32 division, as aa_sample_decode's)
 *   logp(r, t) = y[id] - (m + log sum_v exp(y_v - m)), m = max_v y_v; 0 at a dead position
 *   count      = #live;   loss = -(sum_live advantage[r] logp(r, t)) / count     (the token mean)
 *   dlogits(r, t, v) = dloss[0] advantage[r] (exp(y_v - lse) - [v == id]) / (temperature count)
 * A dead row, and a row of a caption with advantage[r] == 0, is not read: its loss term is 0 and its
 * row of dlogits is written as +0 (the forward still reads an advantage-0 row when logp is wanted).
 * An id outside [0, V) at a live position makes the loss NaN and that row of dlogits NaN, whatever the
 * advantage; ids at dead positions are only compared with end_id.  A non-finite advantage propagates.
 * Fixed-order reductions: bit-reproducible.  logp [R][T] may be NULL.  The forward's workspace
 * (aa_policy_loss_workspace_bytes(R, T); 0 for a refused shape) carries the per-row log-sum-exp and
 * live flags to the backward, which takes the same inputs; dlogits may alias logits only if lddx == ldx.
 * Checks, in this order: AA_ERR_SHAPE for R <= 0, T <= 0, V <= 0, ldx < V, lddx < V, ids_ld < T, a
 * temperature that is not finite and > 0, R T > 2^31 - 1, or in place with unequal pitches; AA_ERR_NULL;
 * AA_ERR_BUFFER for a workspace smaller than aa_policy_loss_workspace_bytes(R, T). */
AA_API size_t aa_policy_loss_workspace_bytes(int32_t R, int32_t T);
AA_API int aa_policy_loss_forward(const float* logits, int64_t ldx, int32_t R, int32_t T, int32_t V,
                                  const int64_t* ids, int64_t ids_ld, const float* advantage,
                                  int32_t end_id, float temperature, float* loss, float* count,
                                  float* logp, void* workspace, size_t workspace_bytes,
                                  aa_stream_t stream);
AA_API int aa_policy_loss_backward(const float* logits, int64_t ldx, int32_t R, int32_t T, int32_t V,
                                   const int64_t* ids, int64_t ids_ld, const float* advantage,
                                   int32_t end_id, float temperature, const float* dloss,
                                   const float* count, const void* workspace, size_t workspace_bytes,
                                   float* dlogits, int64_t lddx, aa_stream_t stream);

/* aa_adam_step: one torch.optim.Adam step (model_factory.py:71: Adam(params, lr, betas, weight_decay); amsgrad=False,
 * maximize=False, L2 weight_decay added to the gradient) over n fp32 tensors, every tensor in one
 * launch per AA_ADAM_MAX_TENSORS.  step = the step count AFTER this step's increment (1 on the first
 * step).  Element-wise in torch's foreach op order (optim/adam.py _multi_tensor_adam):
 * m = lerp(m, g, 1-b1); v = v*b2 + (1-b2)*g*g; p += (-lr/(1-b1^step)) * m / (sqrt(v)/sqrt(1-b2^step) + eps).
 * Tensors with numel 0 are skipped; the four pointers of a tensor must not overlap each other. */
#define AA_ADAM_MAX_TENSORS 24
typedef struct aa_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
} aa_adam_tensor;
AA_API int aa_adam_step(const aa_adam_tensor* tensors, int32_t n, double step, double lr, double beta1,
                        double beta2, double eps, double weight_decay, aa_stream_t stream);

/* aa_clip_grad_norm: torch.nn.utils.clip_grad_norm_(params, max_norm) with the 2-norm (train.py:213-214
 * clips the LSTM's gradients to 5): total = sqrt(sum_i ||g_i||^2) over the tensors' norms, coef =
 * max_norm / (total + 1e-6), every gradient multiplied in place by min(coef, 1) (NaN kept); the total
 * norm is written to total_norm (a device float).  Fixed reduction order: deterministic.  Up to
 * AA_CLIP_MAX_TENSORS tensors; workspace from aa_clip_grad_norm_workspace_bytes (0 = invalid input). */
#define AA_CLIP_MAX_TENSORS 24
typedef struct aa_grad_tensor {
  float* grad;
  int64_t numel;
} aa_grad_tensor;
AA_API size_t aa_clip_grad_norm_workspace_bytes(const aa_grad_tensor* tensors, int32_t n);
AA_API int aa_clip_grad_norm(const aa_grad_tensor* tensors, int32_t n, float max_norm, float* total_norm,
                             void* workspace, size_t workspace_bytes, aa_stream_t stream);

/* ---- CIDEr-D of token-id captions (the figure train.py selects models by; the sampling reward) ---
 * The reference's coco/pycocoevalcap/cider/cider_scorer.py (reached from coco_eval, tools/utils.py:
 * 234-250) on token ids in place of words; restated on the CPU by tests/cider_oracle.py.  Despite the
 * file's name it is CIDEr-D: clipped counts and a Gaussian length penalty.
 * A caption is the ids before the row's first end_id, or all T without one (captions.ids_to_sentences).
 * For a caption w_0 .. w_{L-1} and the orders n = 1..4:
 *   c(g)    = the count of the contiguous n-gram g
 *   df(g)   = the number of corpus images with g in any of their references; M = the corpus's images
 *   w(g)    = log M - log max(1, df(g))    (natural log, float64, computed on the host; an n-gram the
 *             corpus never saw has w = log M = w_unseen)
 *   vec(g)  = c(g) w(g);   norm_n = sqrt(sum_{|g| = n} vec(g)^2)
 *   length  = the number of BIGRAMS, max(L - 1, 0): the reference adds the term frequencies where its
 *             zero-based order index is 1, the bigram slot.  This is reproduced, not corrected: scores
 *             are the reference's.
 *   per reference r of the row's image and order n, in this order of operations:
 *     val_n  = sum_{g in hyp, |g| = n} min(vec_h(g), vec_r(g)) vec_r(g)      (vec_r(g) = 0 when absent)
 *     if norm_h,n != 0 and norm_r,n != 0:  val_n /= norm_h,n norm_r,n
 *     val_n *= exp(-(length_h - length_r)^2 / (2 sigma^2))                   (the reference: sigma = 6)
 *   score   = 10 mean_n(sum_r val_n) / #refs;  an empty caption scores 0.
 * All arithmetic is float64 without contraction; the sums are wave butterflies in a fixed order, so a
 * row's score is bit-reproducible and depends on no other row.
 * n-gram key: key(g) = sum_{j < n} (tok_j + 1) << 16 j, uint64: exact and collision-free for tokens in
 *   [0, 65535); the order is the number of non-zero 16-bit fields, 0 is no key.
 * aa_cider_corpus: a host struct of device pointers, built once per corpus (adaptive_amd.cider.CiderD).
 *   References are CSR: image i owns references img_ptr[i] .. img_ptr[i + 1] - 1, reference r the
 *   entries ref_ptr[r] .. ref_ptr[r + 1] - 1 of keys (ascending within a reference) and counts;
 *   ref_norm[r][n - 1] and ref_len[r] (its bigram count) are precomputed with the same w.
 *   w(g) is an open-addressing table of tab_size slots (a power of two, load factor <= 0.5): a key sits
 *   at slot splitmix64(key) & (tab_size - 1) or the next free one after it (linear probing, wrapping),
 *   tab_keys 0 = empty, tab_w its weight; splitmix64 as in aa_synth_uniform.  A miss is w_unseen.
 *   The document frequencies may come from another corpus than the references (a reward against the
 *   training set's statistics) or from the references themselves (the reference's compute_score).
 * aa_cider_score: scores[r] (float64 [R]) = the score of row r of ids [R, T] (int64, row pitch ids_ld)
 *   against image image[r] of the corpus (int32 [R]; NULL: row r against image r).  One launch, no
 *   workspace, no allocation, no synchronisation.  A token outside [0, 65535) before the row's first
 *   end_id, or an image outside [0, images), makes that row's score NaN (as a bad target does in
 *   aa_cross_entropy_forward); tokens after the first end_id are not looked at.  Every loop over the
 *   corpus's data is bounded, so a malformed table gives a wrong score and never a kernel that does
 *   not end; the CSR offsets themselves are trusted.
 * Checks: AA_ERR_SHAPE for R < 0, T outside [0, AA_CIDER_MAX_T] or ids_ld < T; R == 0 returns AA_OK
 *   before any pointer is looked at; then AA_ERR_NULL for a NULL corpus, AA_ERR_SHAPE for images < 1,
 *   refs < 1, a tab_size that is not a power of two, or a sigma that is not finite and > 0; then
 *   AA_ERR_NULL for a NULL corpus array, scores, or ids (ids may be NULL when T == 0). */
#define AA_CIDER_MAX_T 64
typedef struct aa_cider_corpus {
  const int32_t* img_ptr;   /* [images + 1] */
  const int32_t* ref_ptr;   /* [refs + 1] */
  const uint64_t* keys;     /* [ref_ptr[refs]], ascending within a reference */
  const int32_t* counts;    /* [ref_ptr[refs]] */
  const double* ref_norm;   /* [refs][4] */
  const int32_t* ref_len;   /* [refs]: bigram counts */
  const uint64_t* tab_keys; /* [tab_size], 0 = empty */
  const double* tab_w;      /* [tab_size] */
  int32_t images, refs;
  int64_t tab_size;         /* a power of two */
  double w_unseen;          /* log(images of the document-frequency corpus) */
  double sigma;
} aa_cider_corpus;
AA_API int aa_cider_score(const aa_cider_corpus* corpus, const int64_t* ids, int32_t R, int32_t T,
                          int64_t ids_ld, int32_t end_id, const int32_t* image, double* scores,
                          aa_stream_t stream);

/* ---- BLEU-1..4 and ROUGE-L of token-id captions (the rest of coco_eval's table that ids can give) ---
 * The reference's coco/pycocoevalcap/bleu/bleu_scorer.py as bleu/bleu.py calls it (option 'closest',
 * n = 4) and rouge/rouge.py, on token ids in place of words; restated on the CPU by
 * tests/metrics_oracle.py.  A caption is cut as for aa_cider_score.  For a hypothesis of L tokens
 * against the references of its image:
 *   testlen   = L;   guess_n = max(0, L - n + 1), n = 1..4
 *   correct_n = sum over the distinct n-grams g of order n of min(c_hyp(g), max_refs c_ref(g))
 *   reflen    = the reference length l with the smallest (|l - L|, l): a tie goes to the shorter
 *   sentence BLEU: b = 1; for n = 1..4: b *= (correct_n + 1e-15) / (guess_n + 1e-9),
 *               bleu_n = pow(b, 1 / n); ratio = (L + 1e-15) / (reflen + 1e-9); if ratio < 1 every
 *               bleu_n *= exp(1 - 1 / ratio)
 *   corpus BLEU: the same expression on the integer totals of the ten statistics over the rows
 *   ROUGE-L, beta = 1.2: per reference prec = lcs / max(L, 1), rec = lcs / max(Lr, 1), lcs the longest
 *               common subsequence -- 0 when exactly one side is empty and 1 WHEN BOTH ARE (the
 *               reference splits "" into one empty word; reproduced, not corrected); P = max prec,
 *               Rc = max rec, each over the references on its own;
 *               score = (1 + beta^2) P Rc / (Rc + beta^2 P) if both are non-zero, else 0
 * All float arithmetic is float64 without contraction; the statistics are integers, so a row's outputs
 * are bit-reproducible and depend on no other row.
 * aa_metrics_corpus: a host struct of device pointers, built once per corpus
 *   (adaptive_amd.metrics.CaptionMetrics).  Image i owns references img_ptr[i] .. img_ptr[i + 1] - 1 and
 *   the clip-count entries clip_ptr[i] .. clip_ptr[i + 1] - 1: clip_keys (aa_cider_score's n-gram keys,
 *   ascending within an image) and clip_counts (the largest count of the n-gram in one reference of
 *   the image).  Reference r has ref_len[r] tokens, ref_tok[tok_ptr[r] ..]; references may be empty
 *   and may be longer than AA_CIDER_MAX_T.
 * aa_metrics_score: row r of ids [R, T] (int64, row pitch ids_ld) against image image[r] (NULL: image
 *   r).  stats [R][10] int32 = correct_1..4, guess_1..4, testlen, reflen; bleu [R][4] and rouge [R]
 *   float64.  One launch, no workspace, no synchronisation.  A token outside [0, 65535) before the
 *   row's first end_id, or an image outside [0, images), makes that row's bleu and rouge NaN and its
 *   statistics 0 (so it adds nothing to a corpus total); no other row is affected.  Every loop over
 *   the corpus's data is bounded (the search by 64 halvings, the LCS by the reference's stored
 *   length, the references by the corpus's count); the CSR offsets themselves are trusted.
 * aa_bleu_corpus: out [4] float64 = corpus BLEU-1..4 of stats [R][10] (int64 column totals, then the
 *   expression above).  One launch of one workgroup.
 * Checks: aa_metrics_score as aa_cider_score -- AA_ERR_SHAPE for R < 0, T outside [0, AA_CIDER_MAX_T]
 *   or ids_ld < T; R == 0 returns AA_OK before any pointer is looked at; then AA_ERR_NULL for a NULL
 *   corpus, AA_ERR_SHAPE for images < 1 or refs < 1, AA_ERR_NULL for a NULL corpus array, output, or
 *   ids (ids may be NULL when T == 0).  aa_bleu_corpus: AA_ERR_SHAPE for R < 0; R == 0 returns AA_OK
 *   and writes nothing; AA_ERR_NULL for a NULL stats or out. */
typedef struct aa_metrics_corpus {
  const int32_t* img_ptr;      /* [images + 1] */
  const int32_t* clip_ptr;     /* [images + 1] */
  const uint64_t* clip_keys;   /* [clip_ptr[images]], ascending within an image */
  const int32_t* clip_counts;  /* [clip_ptr[images]] */
  const int32_t* ref_len;      /* [refs]: tokens */
  const int32_t* tok_ptr;      /* [refs + 1] */
  const uint16_t* ref_tok;     /* [tok_ptr[refs]] */
  int32_t images, refs;
} aa_metrics_corpus;
AA_API int aa_metrics_score(const aa_metrics_corpus* corpus, const int64_t* ids, int32_t R, int32_t T,
                            int64_t ids_ld, int32_t end_id, const int32_t* image, int32_t* stats, double* bleu,
                            double* rouge, aa_stream_t stream);
AA_API int aa_bleu_corpus(const int32_t* stats, int32_t R, double* out, aa_stream_t stream);

/* Measurement helper (bench.py's roofline block; not on the decode path): one streaming read of
 * nbytes (multiple of 16, 16-B aligned) from src by `blocks` workgroups, each writing its partial sum
 * to out[block].  Timed over a buffer resident in the 256 MiB Infinity Cache it gives the MALL-served
 * read ceiling that the attention's per-step re-read of V is priced against. */
AA_API int aa_read_probe(const void* src, size_t nbytes, float* out, int32_t blocks, aa_stream_t stream);

/* Counter-based synthetic data (same bits as adaptive_amd/synth.py):
 * dst[i] = fp32(lo + (hi - lo) * u(key, start + i)), u = (splitmix64(key + (start+i+1)*GOLDEN) >> 40) / 2^24.
 * For lo = 0, hi = 1 the value is u exactly. */
AA_API int aa_synth_uniform(float* dst, int64_t n, uint64_t key, int64_t start, double lo,
                            double hi, aa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADAPTIVE_AMD_H */
