/*
 * coattn.h -- C-ABI of the MI355X (gfx950) Hierarchical Co-Attention path (parallel and, from v0.11.0, alternating; v0.12.0: soft answer targets; v0.13.0: the optimiser step; v0.14.0: the frozen encoder's BatchNorm + ReLU + max-pool; v0.15.0: the same with the stock BatchNorm kernels' bits; v0.16.0: the encoder's first convolution and its BatchNorm statistics in one pass, the stock kernels' bits; v0.17.0: the sentence LSTM; v0.18.0: the word embedding and its dense gradient; v0.19.0: feature dropout with a counter RNG, the mask regenerated in the backward; v0.20.0: the gather of cached image features from a table; v0.21.0: attention overlays, the maps upsampled over the image and blended into it as uint8 pictures; v0.22.0: the first convolution computed twice and never stored).  This header is the 78 functions of 0.22.0; what later versions add -- v0.23.0: image preprocessing -- is declared in include/coattn_ext.h.
 *
 * Drop-in boundary.  The reference exposes no FFI: its boundary is the
 * Python nn.Module surface
 *     ParallelCoAttention.forward(x_img[B,N,d], 3 x x_ques[B,T,d]) -> (3 x v[B,d], 3 x q[B,d])
 *     (/root/reference/model.py:356-397, constructed model.py:167, called model.py:182)
 * with backward = autograd of model.py:372-392 (triggered at main.py:219-220).  This library
 * is what a ctypes binding behind that surface calls: coattn_forward replaces the forward
 * loop (model.py:372-395), coattn_backward replaces its autograd graph.  See INTEGRATION.md
 * for the reference-side stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (torch tensor.data_ptr()) unless marked "host";
 *   - the caller owns every buffer, including `saved` and `ws` (sizes: coattn_workspace_bytes);
 *   - calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream), re-entrant and thread-agnostic (backward runs on the autograd thread);
 *   - return 0 on success, < 0 on error (never throws); coattn_last_error() returns the
 *     calling thread's last message;
 *   - math is fp32 (dtype = COATTN_F32: fp32 storage and accumulation; products fp32-accurate by default, see
 *     "Widths of the fp32 mode" below), row-vector convention Linear(x) = x W^T + b.
 *
 * Layouts
 *   V      : the image features x_img[B,N,d] (model.py:215-217), given as a base pointer plus the element
 *            strides (v_sB, v_sN, v_sD) of that logical view -- no copy is ever made.  Two physical layouts
 *            run on the fused kernels:
 *              channel-major  [B][d][N]: (v_sB >= d*N, v_sN = 1, v_sD = N) -- the buffer behind the permuted
 *                             view the reference's NCHW encoder returns;
 *              location-major [B][N][d]: (v_sB >= N*d, v_sN = d, v_sD = 1) -- what a channels_last encoder
 *                             emits (x_img is then contiguous);
 *            any other strides take the general-shape kernels.  dV is described the same way.
 *            Alignment: the fused kernels read V in 16-byte units, so they also want every sample to start
 *            on a 16-byte boundary -- V itself, and v_sB a multiple of 4 floats.  A V that is not (a view
 *            that starts at an odd element, a sample pitch of N*d + 1) is a general-shape call under
 *            COATTN_IMPL_AUTO and is refused (-1, nothing launched) under COATTN_IMPL_FUSED, by the forward
 *            and the backward alike.  The general-shape kernels take any 4-byte aligned V.  Q[l] may sit at
 *            any 4-byte aligned address on either path.
 *   Q[l]   : [B, T, d]  contiguous, l = 0..L-1 (word, phrase, sentence; model.py:298).
 *   W_v,W_q: [d, d] (nn.Linear.weight, out x in); b_v,b_q: [d]; w_v,w_q: [d]; c_v,c_q: [1]
 *            (model.py:350-354).  W_b (model.py:347) is dead in the reference; it is read only under
 *            COATTN_FLAG_BILINEAR (below).
 *   v_out,q_out,gv,gq : [L, B, d].
 */
#ifndef COATTN_H
#define COATTN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COATTN_F32 0
#define COATTN_BF16 1   /* storage type of an INPUT where an entry point says so (coattn_features_native); the math stays fp32 */

/* impl selector (flags & 3): 0 = auto (fused kernels when the shape allows, else general),
 * 1 = general-shape kernels (MFMA GEMM composition), 2 = fused kernels (error if unsupported). */
#define COATTN_IMPL_AUTO 0
#define COATTN_IMPL_GENERAL 1
#define COATTN_IMPL_FUSED 2
/* flags bit 2: the reduced-precision mode that the reference reaches through apex AMP O1 (main.py:185).  The projections
 * P_v, P_q (model.py:380-384) and, in the backward, the d x d contractions that are their gradients (dQ += dP_q W_q,
 * dV += dP_v W_v, dW_v, dW_q) run on the bf16 MFMA (v_mfma_f32_32x32x16_bf16) with operands rounded to bf16 while staged,
 * ONE MFMA per product, fp32 accumulation and fp32 results (gemm_bf.hip at wide shapes, else the single-piece modes of
 * gemm_w.hip / gemm_tn.hip).  On the fused path with d % 512 == 0 the affinity / attention contractions of the fused
 * kernels do the same (single-product instantiations; other widths and the general-shape path keep those exact), and the
 * backward's workspace holds dP_v / dP_q as bf16 when only GEMMs consume them.  Inputs, `saved` and outputs are fp32 in
 * either mode.  Parity then holds to bf16 tolerance (~1e-2), not 1e-4.
 * The same bit selects the bf16 MFMA for the three contractions of coattn_phrase_forward/backward. */
#define COATTN_FLAG_BF16_PROJ 4
#define COATTN_FLAG_BF16_IN 8     /* coattn_linear_forward / coattn_linear_weight_grad, with COATTN_FLAG_BF16_PROJ: x (dy) is STORED as bf16 */
/* Widths of the fp32 mode (dtype COATTN_F32).  An fp32 product runs on the 16-bit MFMAs as partial products of 16-bit
 * PIECES of its operands.
 *   flags = 0 -- the DEFAULT, "exact": three bf16 pieces per operand (hi + mid + lo = the value exactly, six partial
 *     products down to relative order 2^-16, each exact in the fp32 accumulator): every contraction of coattn_forward /
 *     coattn_backward / coattn_phrase_* is fp32-accurate (one fp32 rounding per product) over fp32's whole range, as the
 *     reference's fp32 bmm / Linear (model.py:377-392).  inf / NaN inputs give inf / NaN outputs.
 *   COATTN_FLAG_FAST16 (flags bit 7) -- the "tolerance" mode a caller opts into (train.Trainer does): fewer partial
 *     products, inside the north star's 1e-4 contract on operands of ordinary magnitude:
 *       - forward-side contractions on two FP16 pieces (hi + lo: 22 significand bits, three partial products on
 *         v_mfma_f32_32x32x16_f16, ~2^-22 relative): the affinity A = Q V^T (model.py:377), the projections (model.py:380-384;
 *         the weight image holds 256 W, divided out), C^T P_q and C P_v.  RANGE: exact pieces for |x| <= 65,504 (values below
 *         2^-14 keep 2^-24 absolute; projection weights |W| <= 255); the conversions SATURATE (MODE.FP16_OVFL), so magnitudes
 *         up to 131,008 are still carried with fewer bits and larger ones -- +-inf included -- clamp there.  That event is not
 *         silent: the projection launch records the largest magnitude it converted, and coattn_status() reports it
 *         (-4 = an operand left the exact-piece range in the last coattn_forward on this `saved`);
 *       - gradient contractions of coattn_backward on two bf16 pieces (hi + mid: 16 significand bits, three partial products,
 *         ~2^-16 relative per product, random in sign, fp32's range) -- their operands are gradients of any magnitude.
 *     On the golden cases: v, q within 1e-6, attention maps within 4e-7, H_q within 2e-5, gradients within 1.5e-5 of max|.|
 *     (tests assert 5e-5; the contract is 1e-4); tests/test_split_emulation.py has the budget row by row.
 *     Shapes the hand-scheduled projection kernels do not take (the general-shape path; B N < 128 rows) stay exact.
 *   COATTN_FLAG_EXACT3 (flags bit 4) -- spells the default out (it wins over COATTN_FLAG_FAST16); kept from v0.5.x, where
 *     the tolerance mode was the default of flags = 0. */
#define COATTN_FLAG_EXACT3 16
/* flags bit 5 (coattn_linear_forward; `accumulate` of coattn_linear_weight_grad): the two-bf16-piece width for this product. */
#define COATTN_FLAG_SPLIT2 32
/* flags bit 6 (coattn_linear_forward): two FP16 pieces for this product (the form COATTN_FLAG_FAST16 runs the projections
 * in; no range report: that is coattn_forward's); the weight image written under this flag is read under this flag only. */
#define COATTN_FLAG_F16PAIR 64
#define COATTN_FLAG_FAST16 128
/* ---- bilinear affinity (v0.10.0) ---------------------------------------------------------------------------------
 * flags bit 8, on every co-attention entry point (coattn_forward, _infer, _attention_forward, _backward, their _len and
 * _maps forms, coattn_workspace_bytes): the affinity of the published model (Lu et al. 2016, eq. 3) in place of the
 * reference's C = tanh(Q V^T) (model.py:377).  Per sample and level, row-vector convention:
 *     K = Q W_b^T + b_b   [T,d]   (the module's own self.W_b(Q), model.py:347)
 *     A = K V^T,  C = tanh(A)     [T,N]
 * Everything else is unchanged: P_v, P_q, H_v, H_q, both softmaxes, v = a_v^T V and q = a_q^T Q (Q, not K).  Backward, with
 * dA = dC (.) (1 - C^2) as before:
 *     dK = dA V;  dQ = dP_q W_q + dK W_b + a_q (x) g_q;  dV = dP_v W_v + dA^T K + a_v (x) g_v;
 *     dW_b = sum_l sum_b dK^T Q;  db_b = sum_l sum_b sum_t dK[t]   (one W_b for all levels; `accumulate` as for the rest).
 * Unmasked, a pad row of Q (zeros) gives K = b_b: it holds weight in C and its dK is not zero (db_b sums every row).  Under
 * the length mask the rows t >= len_b of C are zero as before, so dK is zero there and the rule "the contents of pad rows do
 * not matter" holds unchanged.  The maps entry points take G_av / G_aq on top of this form as on the reference one.
 *   - coattn_params.W_b / b_b and coattn_param_grads.dW_b / db_b (the fields appended in v0.10.0) are read only under this
 *     flag; a caller built against 0.9 passes the 8-field structs and is not affected.  NULL W_b / b_b (any call) or NULL
 *     dW_b / db_b (a backward) under the flag: -1, nothing launched.
 *   - `saved` of a bilinear forward also holds K (coattn_workspace_bytes reports the larger buffers when given the flag);
 *     the backward and coattn_attention_forward read it there.  Same contract as above: same inputs, parameter values and
 *     flags.
 *   - Paths: the same as without the flag.  On fused shapes K is one more job on the pre-split-weight projection kernels, the
 *     fused forward streams K through phase 1 (BIL instantiations), and the backward forms dQ with ONE projection
 *     [dP_q | dK] [W_q; W_b] and dW_b on the hand-scheduled weight-gradient kernel (gemm_tn.hip); other shapes run the same math
 *     on the general-shape kernels.
 *   - COATTN_FLAG_FAST16: K replaces Q as phase 1's FP16-piece operand and the projection launch that stores it range-checks it,
 *     and W_b's image follows the |256 W| rule of W_q's: coattn_status / coattn_status_accumulate cover both (-4 when |K| >
 *     65,504 or |W_b| > 255.87).  Pad rows get K = b_b densely (the live-row bitmap serves P_q and dW_q only).
 *   - Refused (-1): the flag together with COATTN_FLAG_BF16_PROJ. */
#define COATTN_FLAG_BILINEAR 256
typedef struct coattn_params {
  const void* W_v; const void* b_v;   /* model.py:350 */
  const void* W_q; const void* b_q;   /* model.py:351 */
  const void* w_v; const void* c_v;   /* model.py:353 */
  const void* w_q; const void* c_q;   /* model.py:354 */
  const void* W_b; const void* b_b;   /* model.py:347; read only under COATTN_FLAG_BILINEAR (v0.10.0) */
} coattn_params;

typedef struct coattn_param_grads {
  void* dW_v; void* db_v; void* dW_q; void* db_q;
  void* dw_v; void* dc_v; void* dw_q; void* dc_q;
  void* dW_b; void* db_b;             /* written only under COATTN_FLAG_BILINEAR (v0.10.0) */
} coattn_param_grads;

/* library version: major*10000 + minor*100 + patch */
int coattn_version(void);

/* last error message of the calling thread ("" if none) */
const char* coattn_last_error(void);

/* Per-kernel timing of the calls this THREAD makes between the two (bench.py's per-kernel roofline legs; nothing a
 * training loop calls).  coattn_profile_begin records a HIP event on `stream`; every launch group of coattn_forward /
 * coattn_backward issued afterwards on this thread records one more behind it.  coattn_profile_end synchronises on the
 * last event and returns the number of marks n (<= max_marks), with us[i] = microseconds between mark i-1 and mark i and
 * `names` = the n mark names joined by '\n' (truncated to names_bytes).  Not for use under graph capture. */
int coattn_profile_begin(void* stream);
int coattn_profile_end(float* us, char* names, int names_bytes, int max_marks);

/* Image features as the encoder leaves them -> the layout the kernels run on (the boundary on the image side: what
 * HierarchicalCoAttentionNet does between image_encoder and co_attention, model.py:215-217 view + permute, under AMP
 * main.py:73, :185 with bf16 activations).
 *   x   : element (b, n, c) at x[b sB + n sN + c sD], x_dtype COATTN_F32 or COATTN_BF16, any non-negative strides -- e.g.
 *         the permuted NCHW view (sB >= d N, sN = 1, sD = N) at N = 49, whose 196-byte (98-byte) rows the kernels do not
 *         take in place;
 *   out : fp32 [B, N, d] contiguous (location-major), the V of coattn_forward / coattn_backward with strides (N d, d, 1).
 * One pass at the memory rate (read along n, written along c through an LDS tile).  Features that are already fp32 and
 * location-major, or channel-major with N % 4 == 0, need no call: coattn_forward takes them where they lie. */
int coattn_features_native(const void* x, int x_dtype, int64_t sB, int64_t sN, int64_t sD, void* out, int B, int N, int d,
                           void* stream);

/* 1 if a fused-kernel configuration exists for this shape (for channel-major or location-major V), else 0 */
int coattn_fused_supported(int B, int N, int T, int d, int L, int dtype);

/* Buffer sizes in bytes.  saved: forward -> backward state (P_v, P_q, C, a_v, a_q, H_q, W_q split into bf16
 * pieces for the backward's dQ projection, the status words of the tolerance mode, and the bitmap of the question rows that
 * are not all zeros: one bit per row and level, written by the exact forward, read by the backward's dW_q);
 * ws_fwd / ws_bwd: scratch, contents undefined after the call. */
int coattn_workspace_bytes(int B, int N, int T, int d, int L, int dtype, int flags,
                           size_t* saved, size_t* ws_fwd, size_t* ws_bwd);

/* Forward of model.py:372-395 for all L levels.
 *   Q      : host array of L device pointers.
 *   saved  : NULL for inference (nothing kept: the call is coattn_infer with no map buffers), else a buffer of `saved` bytes.
 *   v_out,q_out : [L,B,d].
 * Rows of Q_l that are all zeros -- the pad tokens of the reference's question hierarchy (model.py:263 padding_idx,
 * :292-296 pad_packed_sequence) -- project to the bias alone, and the exact mode (flags = 0) uses that: the launch that
 * splits the weights also reads every question row once, flags the rows that hold anything and writes (0 + b_q) into the
 * other rows of P_q; the projection GEMM then runs over the flagged rows only.  Data-driven (no length argument: the
 * reference's forward(x_img, x_ques_hierarchy) has none), and bit-identical to the dense product for every input: zero rows
 * anywhere, none at all, -0.0, NaN (tests/test_gpu_edges.py::test_zero_question_rows_take_the_bias_path_bit_for_bit).
 * coattn_backward uses the same bitmap (kept in `saved`): dW_q = sum dP_q^T Q contracts over the flagged rows only, and the
 * launch of the two weight gradients shares its split-K parts between dW_v and dW_q on the device (the count is not known on
 * the host).  Deterministic -- a function of the inputs --; the order of the additions differs from the all-rows plan, so dW_v /
 * dW_q agree with it to fp32 rounding, not bit for bit.  (One corner differs in kind: a non-finite dP_q element in a zero row
 * makes the reference's dW_q NaN through inf * 0; here that row is not contracted.  db_q, which sums every row, is non-finite in
 * both, so the step still shows.) */
int coattn_forward(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                   const coattn_params* p, void* v_out, void* q_out, void* saved, void* ws,
                   int B, int N, int T, int d, int L, int dtype, int flags, void* stream);

/* Inference (v0.7.0): the forward of coattn_forward with no `saved`, and the attention maps handed to the caller.
 *   av_out : [L,B,N] or NULL -- a_v, the softmax over the N image locations (model.py:387), per level;
 *   aq_out : [L,B,T] or NULL -- a_q, the softmax over the T question tokens (model.py:388).  UNMASKED, as the reference's:
 *            pad tokens hold weight too (their rows of Q are zeros, so they add nothing to q_out); coattn_infer_len (below)
 *            restricts it to the first len_b tokens;
 *   ws     : ws_fwd bytes of coattn_workspace_bytes (the state of the call lives there).
 * v_out / q_out are bit-identical to those of coattn_forward with a `saved` buffer, in every mode (flags 0, COATTN_FLAG_FAST16,
 * COATTN_FLAG_BF16_PROJ) and on both paths.  Forward only: the fused kernel forms C = tanh(Q V^T) for its own use but
 * stores neither C nor H_q (the backward's state; zero-byte buffer resources, the stores are dropped), and the projection
 * launch writes no image of W_q^T.  The maps are written where the kernels would write them into `saved` (the fused
 * kernel's softmax, or the general path's score kernels), with no extra pass; with NULL maps they go to `ws`.  P_v / P_q,
 * the row bitmap and the status words of the tolerance mode stay in `ws`: coattn_status / coattn_status_accumulate take
 * `ws` in place of `saved` after this call.  Nothing of it can feed coattn_backward. */
int coattn_infer(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q, const coattn_params* p,
                 void* v_out, void* q_out, void* av_out, void* aq_out, void* ws, int B, int N, int T, int d, int L,
                 int dtype, int flags, void* stream);

/* Second half of coattn_forward only: everything after the projections P_v, P_q (affinity +
 * tanh model.py:377, H_v/H_q :380-384, scores + row softmax :387-388, attended reductions
 * :391-392), reading P_v / P_q from a `saved` buffer that a previous coattn_forward on the same
 * inputs filled -- with the SAME flags (the fused and the general-shape kernels keep P_v / P_q in different scalings).
 * Exists so that tests and bench.py can time / check this kernel in isolation. */
int coattn_attention_forward(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                             const coattn_params* p, void* v_out, void* q_out, void* saved, void* ws,
                             int B, int N, int T, int d, int L, int dtype, int flags, void* stream);

/* ---- length-masked question attention (v0.8.0) ----------------------------------------------------------------
 * The forms above keep the reference's UNMASKED softmax over the T question positions (model.py:388): pad tokens take weight
 * in a_q.  The *_len forms take one more argument,
 *   q_len : DEVICE int32 [B], the length len_b of question b, shared by all L levels; NULL = unmasked (the call is then the
 *           one above, bit for bit).  Values outside [1, T] are CLAMPED into it on the device (0 acts as 1, T + 5 as T): the
 *           host cannot check device values without a synchronisation.
 * and compute, for every sample b, the reference's unmasked computation on Q_l[b, :len_b] alone (T = len_b):
 *   - a_q[l,b,t] = 0 exactly for t >= len_b, the softmax runs over t < len_b (q_out = sum_{t < len_b} a_q Q);
 *   - rows t >= len_b of C = tanh(Q V^T) are taken as ZERO (selected, not multiplied) in H_v = tanh(P_v + C^T P_q) and
 *     H_q = tanh(P_q + C P_v);
 *   - backward: dQ[l,b,t,:] = 0 for t >= len_b, and those rows contribute nothing to dV or to any parameter gradient.
 * The rows past len_b are not read for their values: outputs and gradients are the same whether they hold zeros or other
 * finite values (in the tolerance mode, values inside its operand range -- the projection launch still converts them).  In the
 * exact mode the bitmap of live question rows counts a row only if it is non-zero AND t < len_b.
 * coattn_backward_len MUST receive the same q_len (same values) as the coattn_forward_len that filled `saved`: nothing in
 * `saved` records it.  Same buffers, sizes (coattn_workspace_bytes), paths and modes as the unmasked forms. */
int coattn_forward_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q, const int32_t* q_len,
                       const coattn_params* p, void* v_out, void* q_out, void* saved, void* ws,
                       int B, int N, int T, int d, int L, int dtype, int flags, void* stream);
int coattn_infer_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q, const int32_t* q_len,
                     const coattn_params* p, void* v_out, void* q_out, void* av_out, void* aq_out, void* ws, int B, int N,
                     int T, int d, int L, int dtype, int flags, void* stream);
int coattn_attention_forward_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                                 const int32_t* q_len, const coattn_params* p, void* v_out, void* q_out, void* saved,
                                 void* ws, int B, int N, int T, int d, int L, int dtype, int flags, void* stream);
int coattn_backward_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q, const int32_t* q_len,
                        const coattn_params* p, const void* saved, const void* gv, const void* gq,
                        void* dV, int64_t dv_sB, int64_t dv_sN, int64_t dv_sD, void* const* dQ,
                        const coattn_param_grads* pg, int accumulate,
                        void* ws, int B, int N, int T, int d, int L, int dtype, int flags, void* stream);

/* Backward (autograd of model.py:372-392).
 *   gv,gq : [L,B,d] upstream gradients of v_out,q_out.
 *   dV    : gradient of x_img with its own strides (dv_sB, dv_sN, dv_sD) (overwritten), or NULL when the image
 *           features need no gradient (frozen encoder, model.py:239-241);
 *   dQ    : host array of L device pointers [B,T,d] (overwritten).
 *   pg    : parameter gradients; accumulate = 0 overwrites, 1 adds into them (grads of the
 *           three levels are always summed: one weight set is shared, model.py:167, :372).
 *   saved : of a coattn_forward call with the SAME inputs, parameter values and flags (it holds projections of
 *           them and an image of W_q; autograd's forward -> backward order guarantees this).  The same VALUES are enough:
 *           V, Q, the parameters and gradients may sit at other addresses (other alignments included) than in that
 *           forward, and `saved` may have held the state of an earlier forward.  What the forward keeps for the backward
 *           depends on the shape and mode alone (the image of W_q^T), or is tagged in `saved` by the forward that wrote it
 *           (the bitmap of the live question rows: without the tag the backward contracts over all rows)
 *           (tests/test_gpu_saved_state.py). */
int coattn_backward(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                    const coattn_params* p, const void* saved, const void* gv, const void* gq,
                    void* dV, int64_t dv_sB, int64_t dv_sN, int64_t dv_sD, void* const* dQ,
                    const coattn_param_grads* pg, int accumulate,
                    void* ws, int B, int N, int T, int d, int L, int dtype, int flags, void* stream);

/* ---- differentiable attention maps (v0.9.0) ----------------------------------------------------------------------
 * For a training loss ON the maps (attention supervision such as a KL term against human attention maps, an entropy penalty,
 * logging the maps of the batch being trained on).
 *   coattn_forward_maps(_len) : coattn_forward(_len) that also hands a_v [L,B,N] / a_q [L,B,T] to the caller.  `saved`, av_out
 *       and aq_out are REQUIRED (NULL: a negative code and coattn_last_error()).  v_out, q_out and `saved` are bit-identical to
 *       coattn_forward(_len)'s, the maps to coattn_infer(_len)'s: the kernels store each map twice from the same epilogue --
 *       into `saved`, where the backward reads it, and into the caller's buffer -- with no extra launch.
 *   coattn_backward_maps(_len) : coattn_backward(_len) with two more arguments right after gq,
 *       g_av : [L,B,N] upstream gradient of a_v, or NULL (= 0);
 *       g_aq : [L,B,T] upstream gradient of a_q, or NULL (= 0).
 *     Per sample b and level l only the two softmax backward steps change:
 *       da_v = V g_v + G_av,  ds_v = a_v (.) (da_v - sum_n a_v da_v)
 *       da_q = Q g_q + G_aq,  ds_q = a_q (.) (da_q - sum_t a_q da_q)
 *     and everything downstream of ds_v / ds_q (dZ, dP_v, dP_q, dC, dA, dV, dQ, every parameter gradient) is the backward of
 *     coattn_backward(_len).  With both NULL every output is bit-identical to coattn_backward(_len)'s, accumulate included.
 *     Under the length mask G_aq[l,b,t] for t >= len_b is READ AS 0: a NaN or inf a caller leaves in a pad slot changes no
 *     output bit.
 *   `saved` must come from a coattn_forward_maps(_len) or a coattn_forward(_len) with the same inputs, parameter values, flags
 *   (and q_len) -- both leave the same bits in it.  Same buffer sizes (coattn_workspace_bytes), paths and modes as the forms
 *   above. */
int coattn_forward_maps(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                        const coattn_params* p, void* v_out, void* q_out, void* av_out, void* aq_out, void* saved, void* ws,
                        int B, int N, int T, int d, int L, int dtype, int flags, void* stream);
int coattn_forward_maps_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                            const int32_t* q_len, const coattn_params* p, void* v_out, void* q_out, void* av_out,
                            void* aq_out, void* saved, void* ws, int B, int N, int T, int d, int L, int dtype, int flags,
                            void* stream);
int coattn_backward_maps(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                         const coattn_params* p, const void* saved, const void* gv, const void* gq, const void* g_av,
                         const void* g_aq, void* dV, int64_t dv_sB, int64_t dv_sN, int64_t dv_sD, void* const* dQ,
                         const coattn_param_grads* pg, int accumulate,
                         void* ws, int B, int N, int T, int d, int L, int dtype, int flags, void* stream);
int coattn_backward_maps_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                             const int32_t* q_len, const coattn_params* p, const void* saved, const void* gv, const void* gq,
                             const void* g_av, const void* g_aq, void* dV, int64_t dv_sB, int64_t dv_sN, int64_t dv_sD,
                             void* const* dQ, const coattn_param_grads* pg, int accumulate,
                             void* ws, int B, int N, int T, int d, int L, int dtype, int flags, void* stream);

/* ---- alternating co-attention (v0.11.0) --------------------------------------------------------------------------
 * The paper's second co-attention form (Lu et al. 2016, section 3.3, eq. 6): no T x N affinity, three chained guided-attention
 * steps.  Per sample b and level l, row-vector convention, one parameter set shared by the L levels, its own per step:
 *     guided(X, g):  H = tanh(X W_x^T + b_x + g)   [R,d]   (g broadcast over the R rows)
 *                    a = softmax_R(H w_h^T + c_h)  [R]
 *                    x^ = a^T X                    [d]
 *     step 1:  s^, a_s = guided(Q, 0)                            (W_x1, w_h1)      R = T
 *     step 2:  v^, a_v = guided(V, s^ W_g2^T + b_g2)             (W_x2, W_g2, w_h2) R = N
 *     step 3:  q^, a_q = guided(Q, v^ W_g3^T + b_g3)             (W_x3, W_g3, w_h3) R = T
 *     v_out = v^, q_out = q^  [L,B,d]   (the shapes and meaning of coattn_forward's outputs)
 * W_x*, W_g* are [d,d] (nn.Linear(d, d)), b_* [d]; w_h* [d] (nn.Linear(d, 1).weight), c_h* [1].
 *   q_len : DEVICE int32 [B] or NULL (unmasked: the softmaxes of steps 1 and 3 run over all T tokens).  With it, the semantics of
 *           v0.8.0: steps 1 and 3 run over the rows t < clamp(len_b, 1, T) alone; a_s, a_q are exactly 0 beyond, those rows of
 *           Q are not read for their values and dQ is 0 there.  The backward must receive the same q_len.
 * V, Q, strides, buffers, streams, errors: as coattn_forward (V by its three strides, Q a host array of L device pointers, the
 * caller owns every buffer, nothing is allocated, asynchronous on `stream`, no CPU fallback).  Limits: N, T <= 512, d <= 1024,
 * L <= 4.
 * EXACT MODE ONLY: flags must be 0 (COATTN_FLAG_FAST16, COATTN_FLAG_BF16_PROJ, COATTN_FLAG_BILINEAR, the impl selectors: -1).
 * Paths: [X1 | X3] = Q_l [W_x1; W_x3]^T + [b_x1; b_x3] for every level in ONE projection, X2 = V W_x2^T + b_x2 once per sample,
 * the guide vectors (M = L B) -- on the pre-split-weight kernels where they take the shape (gemm_w.hip), else on the general
 * GEMM; the weight gradients on the split-K weight-gradient kernel (gemm_tn.hip) with a fixed-order reduce.  The guided steps
 * run on their own kernels (coattn_alt.hip); step 2 takes the L levels of a sample in one workgroup.  No float atomics: two
 * runs are bitwise identical. */
typedef struct coattn_alt_params {
  const void* W_x1; const void* b_x1; const void* w_h1; const void* c_h1;
  const void* W_x2; const void* b_x2; const void* W_g2; const void* b_g2; const void* w_h2; const void* c_h2;
  const void* W_x3; const void* b_x3; const void* W_g3; const void* b_g3; const void* w_h3; const void* c_h3;
} coattn_alt_params;
typedef struct coattn_alt_param_grads {
  void* dW_x1; void* db_x1; void* dw_h1; void* dc_h1;
  void* dW_x2; void* db_x2; void* dW_g2; void* db_g2; void* dw_h2; void* dc_h2;
  void* dW_x3; void* db_x3; void* dW_g3; void* db_g3; void* dw_h3; void* dc_h3;
} coattn_alt_param_grads;
/* saved: forward -> backward state (X1 | X3, X2, both guide vectors, s^, v^, a_s, a_v, a_q); ws_fwd / ws_bwd: scratch.  H is not
 * stored: the backward recomputes it from X and g. */
int coattn_alt_workspace_bytes(int B, int N, int T, int d, int L, int dtype, int flags, size_t* saved, size_t* ws_fwd,
                               size_t* ws_bwd);
/* av_out [L,B,N] (a_v of step 2) and aq_out [L,B,T] (a_q of step 3) may each be NULL.  saved NULL: inference, nothing kept (the
 * state lives in ws), and v_out / q_out are bit-identical to a call with `saved`. */
int coattn_alt_forward(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q, const int32_t* q_len,
                       const coattn_alt_params* p, void* v_out, void* q_out, void* av_out, void* aq_out, void* saved, void* ws,
                       int B, int N, int T, int d, int L, int dtype, int flags, void* stream);
/* gv, gq [L,B,d]: upstream gradients of v_out, q_out.  g_av [L,B,N], g_aq [L,B,T]: upstream gradients of the maps, or NULL (= 0);
 * as in v0.9.0 they enter before the softmax backward (da = X g + G) and under the mask g_aq is read as 0 past the length.
 * dV (its own strides; overwritten) may be NULL for a frozen encoder; dQ: host array of L device pointers (overwritten).
 * pg: accumulate = 0 overwrites, 1 adds; the gradients of the L levels are summed.  Per step the backward forms, row by row,
 *     da_r = x_r . gx^ (+ G_a),  ds = a (.) (da - sum a da),  dH_r = ds_r w_h (.) (1 - H_r^2),  dg = sum_r dH_r,
 * and the gradient into v^ is gv + dg3 W_g3, into s^ dg2 W_g2.  `saved`: of a coattn_alt_forward with the same inputs, parameter
 * values, flags and q_len. */
int coattn_alt_backward(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q, const int32_t* q_len,
                        const coattn_alt_params* p, const void* saved, const void* gv, const void* gq, const void* g_av,
                        const void* g_aq, void* dV, int64_t dv_sB, int64_t dv_sN, int64_t dv_sD, void* const* dQ,
                        const coattn_alt_param_grads* pg, int accumulate, void* ws, int B, int N, int T, int d, int L,
                        int dtype, int flags, void* stream);

/* Range report of the tolerance mode (COATTN_FLAG_FAST16).  SYNCHRONISES `stream`, reads the status words the last
 * coattn_forward left in `saved` (or in `ws`, when that call was given saved = NULL) and returns
 *    0  every operand converted to FP16 pieces lay inside the exact-piece range (or the call did not use FP16 pieces:
 *       exact mode, reduced-precision mode, general-shape path);
 *   -4  some operand did not: an activation (image / question feature, stored projection) beyond 65,504 or a projection
 *       weight beyond 255.87 in magnitude, +-inf included -- its pieces were clamped (see COATTN_FLAG_FAST16) and the
 *       results of that call are not within tolerance of the reference; coattn_last_error() names the operand class and
 *       the magnitude.  Re-run with flags = 0 (exact), which computes the reference's value over fp32's whole range.
 * amax (host, may be NULL): [0] = largest |activation| beyond the range seen by the projection launch (0 if none),
 * [1] = largest |256 W| over both projection weights.  Call it where the host synchronises anyway (reading the loss). */
int coattn_status(const void* saved, int B, int N, int T, int d, int L, int dtype, void* stream, float* amax);
/* The same report made STICKY across calls without a synchronisation (v0.6.1): every coattn_forward rewrites the status words
 * of its `saved`, so a caller that reads them only now and then (a training loop that reads the loss every log_interval
 * steps) would miss the steps in between.  ASYNCHRONOUS on `stream`: folds the status words the last coattn_forward left in
 * `saved` into `acc`, two floats in DEVICE memory the caller owns and zeroes: acc[0] = max(acc[0], largest out-of-range
 * |activation| of that call), acc[1] = max(acc[1], largest |256 W|) -- maxima on the bit patterns, so a NaN wins.  A call
 * that used no FP16 pieces leaves acc alone.  The caller reads acc where it synchronises anyway: the tolerance mode held
 * for every folded call iff acc[0] <= 65504 and acc[1] <= 65504 (both 0 when nothing was out of range / no weights seen).
 * Steps run before the caller looks are NOT rolled back: a training loop that cannot afford that runs flags = 0. */
int coattn_status_accumulate(const void* saved, int B, int N, int T, int d, int L, int dtype, void* acc, void* stream);

/* ---- PhraseConvPool: the question hierarchy's phrase level ----------------
 * Replaces reference model.py:301-334 (`PhraseConvPool.forward`: 1/2/3-gram Conv1d + Tanh with
 * ConstantPad1d (0,0) / (1,0) / (1,1), concatenated along channels, then MaxPool2d((1,3)) over
 * groups of 3 CONSECUTIVE channels) and its autograd.  Weights in torch Conv1d layout
 * [E_out][E_in][k] (state_dict keys conv_unigram.1.*, conv_bigram.1.*, conv_trigram.1.*). */
typedef struct coattn_phrase_params {
  const void* W1; const void* b1;   /* [E,E,1], [E] */
  const void* W2; const void* b2;   /* [E,E,2], [E] */
  const void* W3; const void* b3;   /* [E,E,3], [E] */
} coattn_phrase_params;

typedef struct coattn_phrase_param_grads {
  void* dW1; void* db1; void* dW2; void* db2; void* dW3; void* db3;
} coattn_phrase_param_grads;

/* saved: forward -> backward state (argmax index per output element, then the status words of coattn_phrase_status);
 * ws_*: scratch.  flags: COATTN_FLAG_BF16_PROJ, COATTN_FLAG_FAST16 (see "Widths of the fp32 mode"); pass the same flags to the
 * forward and the backward of a step. */
int coattn_phrase_workspace_bytes(int B, int T, int E, int dtype, size_t* saved, size_t* ws_fwd, size_t* ws_bwd);

/* X [B,T,E] (rows past a question's length are zeros, as the embedding delivers them) -> out [B,T,E].
 * saved may be NULL for inference. */
int coattn_phrase_forward(const void* X, const coattn_phrase_params* p, void* out, void* saved, void* ws,
                          int B, int T, int E, int dtype, int flags, void* stream);

/* g_out [B,T,E] -> dX [B,T,E] (overwritten; NULL to skip) and the six parameter gradients
 * (accumulate = 0 overwrites, 1 adds).  `out` is the forward's output. */
int coattn_phrase_backward(const void* X, const coattn_phrase_params* p, const void* out, const void* saved,
                           const void* g_out, void* dX, const coattn_phrase_param_grads* pg, int accumulate,
                           void* ws, int B, int T, int E, int dtype, int flags, void* stream);

/* Range report of coattn_phrase_forward under COATTN_FLAG_FAST16 (its product Z = Xcat Wcat^T then runs on two FP16
 * pieces, like the co-attention's projections): as coattn_status -- synchronises, 0 / -4 -- on the status words behind the
 * argmax bytes of `saved` (saved must have been given to the forward call). */
int coattn_phrase_status(const void* saved, int B, int T, int E, void* stream, float* amax);
/* as coattn_status_accumulate, on the status words behind the phrase level's `saved` */
int coattn_phrase_status_accumulate(const void* saved, int B, int T, int E, void* acc, void* stream);

/* ---- cross entropy of the train step ------------------------------------------------
 * coattn_ce_forward replaces `nn.CrossEntropyLoss()(logits, label)` (main.py:94, :214; mean over the batch)
 * together with its gradient.  The MLPClassifier that produces the logits (model.py:400-434) stays on the stock
 * PyTorch-ROCm modules unless the fused head below is used (coattn_head_forward). */
/* Mean cross entropy over B rows of [B,K] logits with int64 labels in [0,K):
 * loss[0] = mean_i (logsumexp(z_i) - z_i[label_i]);  dlogits [B,K] = (softmax(z) - onehot) / B, or NULL to skip.
 * ws: coattn_ce_workspace_bytes.  A label outside [0,K) -- where nn.CrossEntropyLoss raises -- makes the loss NaN and
 * sets a status word in `ws`; the call itself stays asynchronous.  coattn_ce_status(ws, B, stream) SYNCHRONISES the
 * stream and returns -2 (coattn_last_error names the row) if the last coattn_ce_forward on this `ws` met such a label,
 * else 0: call it where the host synchronises anyway (reading the loss). */
int coattn_ce_workspace_bytes(int B, int K, int dtype, size_t* ws);
int coattn_ce_forward(const void* logits, const void* labels, void* loss, void* dlogits, void* ws, int B, int K,
                      int dtype, void* stream);
int coattn_ce_status(const void* ws, int B, void* stream);

/* ---- answer head: MLPClassifier + cross entropy and their backward ----------------------------
 * coattn_head_forward replaces `MLPClassifier.forward` (model.py:414-434, called at model.py:185 with the two lists
 * co-attention returns) and, when labels are given, `criterion(logits, label)` (main.py:214):
 *     h_w = tanh(W_w (q_w + v_w) + b_w); h_p = tanh(W_p [q_p + v_p | h_w] + b_p); h_s = tanh(W_s [q_s + v_s | h_p] + b_s);
 *     logits = W_h h_s + b_h;  loss = mean cross entropy.
 * coattn_head_backward replaces their autograd graph (main.py:219-220).  The adds, the concatenations, bias + tanh and
 * tanh' are folded into the operand addressing / epilogues of 32 x 32-tile products on the exact-fp32 MFMA (head.hip):
 * 4 launches + ONE for the loss (rows and their mean: the last workgroup's ticket, ce.hip) forward, 4 launches backward.
 *   v, q   : host arrays of 3 device pointers [B,d] each (word, phrase, sentence: the rows of co-attention's v_out /
 *            q_out, or any three tensors);  W_w [d,d], W_p [d,2d], W_s [mlp,2d], W_h [K,mlp] as nn.Linear stores them.
 *   labels : int64 [B] or NULL (then loss must be NULL too: logits only, e.g. validation's argmax).
 *   logits : [B,K] (written);  loss: [1] (written).  A label outside [0,K) makes the loss NaN and sets the status
 *            word coattn_head_status(saved, ...) reports (-2; it synchronises the stream, like coattn_ce_status).
 *            Every forward WITH a loss clears the word first, so `saved` may be reused call after call without a memset;
 *            a logits-only forward (labels NULL) leaves it alone: coattn_head_status then still reports the last
 *            forward on this `saved` that had a loss.
 *   saved  : forward -> backward state (h_w, h_p, h_s, d loss / d logits, row losses): coattn_head_workspace_bytes.
 * Backward: g_loss [1] (device) scales the saved d loss / d logits; g_logits [B,K] (may be NULL) is added to it -- the two
 * upstream gradients autograd can hand over; at least one must be given.  dv, dq: host arrays of 3 device pointers [B,d]
 * (overwritten; the gradient of q_l + v_l goes to both; dq may be NULL or equal dv: stored once; dv NULL: no input
 * gradients).  pg: the eight parameter gradients (accumulate = 0 overwrites, 1 adds).  ws: scratch of `ws_bwd` bytes. */
/* flags bit 0 of coattn_head_forward / coattn_head_backward: the layers of a direction as phases of ONE launch separated by
 * grid-wide barriers instead of one launch per layer (same tiles, same values; measured slower or equal: opt-in).  The
 * barriers' spins are bounded: should one time out (the grid not resident), the call's first output element -- logits[0][0],
 * and with it the loss; the first gradient element -- is NaN rather than silently stale. */
#define COATTN_HEAD_PERSISTENT 1
/* flags bit 2 (COATTN_FLAG_BF16_PROJ) of both: the reduced-precision mode -- the operands of the four products and of their
 * gradients rounded to bf16 while they are fed to the matrix pipe (ONE v_mfma_f32_32x32x16_bf16 where the exact head issues
 * eight v_mfma_f32_32x32x2_f32), fp32 accumulation, biases, tanh, cross entropy and bias gradients; bf16 tolerance.  Pass the
 * same flag to the forward and the backward of a step.  (The one-launch form is exact only: bits 0 and 2 together are an
 * argument error, -1.) */
typedef struct coattn_head_params {
  const void* W_w; const void* b_w;   /* model.py:409 */
  const void* W_p; const void* b_p;   /* model.py:410 */
  const void* W_s; const void* b_s;   /* model.py:411 */
  const void* W_h; const void* b_h;   /* model.py:412 */
} coattn_head_params;
typedef struct coattn_head_param_grads {
  void* dW_w; void* db_w; void* dW_p; void* db_p; void* dW_s; void* db_s; void* dW_h; void* db_h;
} coattn_head_param_grads;
int coattn_head_workspace_bytes(int B, int d, int mlp, int K, int dtype, size_t* saved, size_t* ws_bwd);
int coattn_head_forward(const void* const* v, const void* const* q, const coattn_head_params* p, const void* labels,
                        void* logits, void* loss, void* saved, int B, int d, int mlp, int K, int dtype, int flags,
                        void* stream);
int coattn_head_status(const void* saved, int B, int d, int mlp, int K, void* stream);
int coattn_head_backward(const void* const* v, const void* const* q, const coattn_head_params* p, const void* saved,
                         const void* g_loss, const void* g_logits, void* const* dv, void* const* dq,
                         const coattn_head_param_grads* pg, int accumulate, void* ws, int B, int d, int mlp, int K,
                         int dtype, int flags, void* stream);

/* ---- soft answer targets (v0.12.0): the VQA annotations' ten human answers instead of one majority label ----------
 * A VQA sample has up to A (answer, score) pairs; the task's own metric scores an answer min(1, humans who gave it / 3).
 * The targets are passed sparse, as the annotations are:
 *   ans_idx   : int32 [B,A], a class index in [0,K), or -1 for an empty slot;
 *   ans_score : fp32  [B,A], the slot's score; NOT READ for an empty slot (a NaN there changes no bit);
 *   1 <= A <= 16.
 * They stand for the dense target t[b][k] = sum over the slots a with ans_idx[b][a] == k of ans_score[b][a] (duplicate
 * indices in a row add; a row of empty slots is legal: t[b][:] = 0), which is never formed in memory.  An index >= K or
 * < -1 makes the loss NaN and raises the status word of the hard-label loss: coattn_ce_status / coattn_head_status
 * return -2 and name the row; the call stays asynchronous.
 * A LIVE slot's non-finite score propagates as it would through the dense target: a NaN score makes t[b][k] NaN -- the row's
 * loss (and with it the mean) NaN under both kinds, the row's whole gradient NaN under SOFT_CE (through S_b), the entry k alone
 * under BCE, the row's score NaN where k is the predicted class -- and a score of +inf is a target of +inf, which BCE and the
 * score clamp to 1.  min(t, 1) below means "1 where t > 1, else t", never a min that drops a NaN.  Other rows keep their bits.
 * Loss kinds, with S_b = sum_k t[b][k] and the mean taken over the B rows (loss = (1/B) sum_b row):
 *   COATTN_LOSS_SOFT_CE: row = S_b logsumexp(z_b) - sum_k t z           d loss / d z = (S_b softmax(z) - t) / B
 *                        (for a row whose only slot is (label, 1.0) this IS coattn_ce_forward's cross entropy, bit for bit;
 *                        the sum runs over the classes with t != 0, so a class WITHOUT a target may be masked with a logit
 *                        of -inf, as under coattn_ce_forward: finite loss, gradient +0 there; a +inf logit gives
 *                        logsumexp = +inf as torch.logsumexp does: gradient NaN at that class alone)
 *   COATTN_LOSS_BCE    : row = sum_k (softplus(z) - min(t, 1) z)        d loss / d z = (sigmoid(z) - min(t, 1)) / B
 *                        (binary cross entropy with logits summed over the classes; the target is clamped to 1, and
 *                        softplus is max(z, 0) + log1p(exp(-|z|)): finite for every finite logit)
 * One launch, no float atomics, bitwise repeatable -- as coattn_ce_forward. */
#define COATTN_LOSS_SOFT_CE 1
#define COATTN_LOSS_BCE 2
/* loss [1], dlogits [B,K] or NULL; ws: coattn_ce_workspace_bytes (its contents need no initialisation), read by
 * coattn_ce_status.  Argument errors (A outside 1..16, unknown kind, NULL pointers): -1 before anything is launched. */
int coattn_soft_loss_forward(const void* logits, const void* ans_idx, const void* ans_score, int A, int kind,
                             void* loss, void* dlogits, void* ws, int B, int K, int dtype, void* stream);
/* Evaluation: pred[b] = argmax_k z[b][k] (the lowest index among equal maxima), row_score[b] = min(1, t[b][pred[b]]) -- the
 * VQA accuracy of the predicted answer -- and score_sum[0] = their sum in a fixed order, in one launch.
 * argmax treats a NaN logit as numpy.argmax and torch.argmax do: it counts as the maximum, and the lowest index of a NaN wins,
 * also over a larger finite logit or +inf in the same row; a row of -inf alone predicts index 0.  pred[b] < K always.
 * pred: int32 [B]; row_score: fp32 [B], may be NULL; score_sum: fp32 [1]; ws as above (K <= 2^24). */
int coattn_vqa_score(const void* logits, const void* ans_idx, const void* ans_score, int A,
                     void* pred, void* row_score, void* score_sum,
                     void* ws, int B, int K, int dtype, void* stream);
/* coattn_head_forward with (ans_idx, ans_score, A, kind) in place of `labels` (loss must be given).  It writes the SAME
 * `saved` layout as coattn_head_forward, so coattn_head_backward and coattn_head_status serve both unchanged, and it
 * accepts the same flags (COATTN_HEAD_PERSISTENT, COATTN_FLAG_BF16_PROJ: the loss is fp32 in all of them).  The launch
 * count is coattn_head_forward's: four layers + ONE launch for the loss. */
int coattn_head_forward_soft(const void* const* v, const void* const* q, const coattn_head_params* p,
                             const void* ans_idx, const void* ans_score, int A, int kind,
                             void* logits, void* loss, void* saved, int B, int d, int mlp, int K, int dtype, int flags,
                             void* stream);

/* ---- the optimiser step (v0.13.0): Adam / AdamW with gradient clipping by global norm, fp32 ------------------------
 * The reference ends its step in torch.optim.Adam(...).step() (main.py:180, :222): eight or nine multi-tensor launches.  Here
 * one call updates a whole list of tensors in ONE launch (lists of more than 64 non-empty tensors: one launch per 64), with
 * torch.optim.Adam's arithmetic for the caller's step number `step` >= 1 (bc1 = 1 - beta1^step, bc2 = 1 - beta2^step):
 *     g' = g * clip                                        (max_grad_norm > 0 only)
 *     p  = p * (1 - lr * weight_decay)                     (weight_decay != 0 only: decoupled decay, torch.optim.AdamW)
 *     m  = beta1 m + (1 - beta1) g'       v = beta2 v + (1 - beta2) g'^2
 *     p  = p - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
 * p, m (exp_avg), v (exp_avg_sq) are updated in place, g is only read; each is n contiguous fp32 elements, 4-byte aligned
 * (16-byte accesses where all four pointers of a tensor are 16-byte aligned, dword accesses otherwise).  n = 0 entries are
 * skipped.  NaN / inf propagate as in the stock optimiser: nothing is skipped.
 * The hyper-parameters are doubles: 1 - beta, lr / bc1, sqrt(bc2) and 1 - lr * weight_decay are formed on the host in double
 * and rounded to fp32 once, as torch forms them from Python floats (1 - (float)0.999 is 1.3e-5 off 0.001).
 * max_grad_norm > 0: a launch ahead of the update (one per 64 tensors) sums g^2 over the whole list -- per-workgroup partials
 * in `ws`, added in a fixed order by the workgroup that takes the last integer ticket; accumulation in double, no float
 * atomics: bitwise repeatable -- and leaves norm = sqrt(sum) and clip = min(1, max_grad_norm / (norm + 1e-6))
 * (torch.nn.utils.clip_grad_norm_) in `ws`, where the update reads clip; the host never waits.  norm_out (device fp32 [1], may
 * be NULL) receives norm.  max_grad_norm <= 0: no clipping, no norm pass, `ws` and norm_out are not touched (ws may be NULL).
 * ws: coattn_adam_workspace_bytes(t, n_tensors) bytes (0 = bad list, see coattn_last_error), 8-byte aligned, contents need no
 * initialisation; t is a HOST array, read before the call returns.
 * Argument errors (n_tensors <= 0, a NULL pointer in an entry, n < 0, step < 1, a beta outside [0, 1), a clipped call whose
 * workspace is too small): -1 before anything is launched. */
typedef struct coattn_adam_tensor {
  void* p; const void* g; void* m; void* v; int64_t n;
} coattn_adam_tensor;
size_t coattn_adam_workspace_bytes(const coattn_adam_tensor* t, int n_tensors);
int coattn_adam_step(const coattn_adam_tensor* t, int n_tensors, int step, double lr, double beta1, double beta2,
                     double eps, double weight_decay, double max_grad_norm, void* norm_out, void* ws, size_t ws_bytes,
                     void* stream);

/* ---- the frozen image encoder's glue (v0.14.0): train-mode BatchNorm2d + ReLU + optional 2x2 max-pool, fp32, NHWC ----
 * The reference never puts its frozen VGG11-bn in eval mode (model.py:239-241): every step normalises each convolution's
 * output with fresh batch statistics.  The convolutions stay on MIOpen; this call replaces the memory-bound chain between
 * two of them -- BatchNorm2d (batch statistics, affine, running statistics with a momentum), ReLU and, with `pool`,
 * MaxPool2d(2, 2) (no padding, floor mode: Ho = H / 2, Wo = W / 2, an odd last row / column is dropped) -- by two passes
 * over x (csrc/encoder.hip): statistics accumulated in double, then normalise + pool + ReLU in one pass.  Forward only.
 *   x            : fp32, physically [B][H][W][C] with C contiguous (a channels_last [B,C,H,W] tensor), 16-byte aligned; read only
 *   gamma, beta  : fp32 [C], BatchNorm2d's weight and bias
 *   conv_bias    : fp32 [C] or NULL: a frozen bias of the convolution that the caller left out of x.  It cancels in the
 *                  normalised output and survives only in the running mean, where it is added here.
 *   running_mean, running_var : fp32 [C], updated in place: rm = (1 - momentum) rm + momentum (mean + conv_bias),
 *                  rv = (1 - momentum) rv + momentum var n / (n - 1) with n = B H W
 *   y            : fp32 [B][Ho][Wo][C] (pool) or [B][H][W][C], 16-byte aligned, not x
 *   stats_out    : fp32 [2][C] or NULL: the batch mean of x (without conv_bias) and the biased batch variance
 *   ws           : the workspace size call's bytes, 16-byte aligned, contents need no initialisation
 *   relu         : 0 leaves the ReLU out
 * y = relu(max over the window of ((x - mean) * gamma / sqrt(var + eps) + beta)); NaN propagates as in PyTorch; a constant
 * channel (var = 0) gives beta.  Results are bitwise repeatable (fixed-order reductions, no atomics).
 * The supported-shape query returns 1 only for dtype COATTN_F32, C a power of two in 16 .. 512, B H W >= 2, B H W C < 2^31
 * and, with pool, H >= 2 and W >= 2; it makes no GPU call.  The workspace size of an unsupported shape is 0.
 * Argument errors (an unsupported shape, a NULL or misaligned pointer, momentum outside [0, 1], eps <= 0): -1 before any
 * HIP call. */
int coattn_bn_supported(int B, int H, int W, int C, int pool, int dtype);
size_t coattn_bn_workspace_bytes(int B, int H, int W, int C);
int coattn_bn_relu_pool_forward(const void* x, const void* gamma, const void* beta, const void* conv_bias,
                                void* running_mean, void* running_var, double momentum, double eps, void* y,
                                void* stats_out, void* ws, int B, int H, int W, int C, int pool, int relu, int dtype,
                                void* stream);

/* The 2x2 / stride-2 / floor-mode max-pool and the ReLU alone, in one pass: y [B][H/2][W/2][C] = relu(max over each window of
 * x [B][H][W][C]) -- fp32, C contiguous, 16-byte aligned, y not x.  Maximum and ReLU are exact operations, so y has the values
 * of PyTorch's max_pool2d followed by relu bit for bit (NaN propagates the same way).  Shapes: those the supported-shape
 * query above accepts with pool = 1; anything else, or a NULL / misaligned pointer: -1 before any HIP call. */
int coattn_relu_pool_forward(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);

/* ---- the same chain with the STOCK kernels' bits (v0.15.0) ----
 * MIOpen's multi-kernel spatial forward-training BatchNorm (NHWC, fp32) is fp32 arithmetic in a fixed order: per thread a
 * sequential sum of x and fma(x, x, .) over the samples of one pixel position, one LDS halving tree per workgroup, a second
 * kernel that adds the workgroups' partials in a strided order, the same tree times 1 / (B H W), var = max(fma(-mean, mean,
 * E[x^2]), 0), invstd = rsq(var + eps); then y = fma(gamma, (x - mean) * invstd, beta).  This call sums in that order with that
 * formula, so mean, invstd, the running statistics and y are MIOpen's bit for bit -- in two passes over x instead of three,
 * with the 2x2 max-pool (floor mode) and the ReLU in the second.  Which order MIOpen uses depends on the geometry it compiles
 * for the shape; the geometry query reproduces it for the shapes it was read off for and answers 0 for every other one.
 *   coattn_bn_exact_geometry : 0 = not covered (dtype not COATTN_F32, C not 64 / 128 / 256 / 512, B > 1024, H W C in the
 *                  unobserved band 153601 .. 163839, H W = 1 modulo the workgroup's 8 or 16 pixels, more than 65535 pixel groups (the grid's
 *                  limit: H W > 1048560 at 16 pixels), B H W C >= 2^31); otherwise 10, the number of ints written to `out`
 *                  (may be NULL): vector width along C, workgroup shape g0 (channel groups) x g1 (pixels) x g2 (sample groups),
 *                  samples per thread, pixel groups, sample groups, the final kernel's workgroup shape f0 x f1 x f2.  No GPU call.
 *   x, y, gamma, beta, running_mean, running_var, B, H, W, C, pool, relu, dtype, stream : as for coattn_bn_relu_pool_forward
 *                  (the running statistics move as MIOpen moves them: there is no conv_bias here)
 *   save_mean, save_invstd : fp32 [C], written: the batch mean and 1 / sqrt(var + eps), MIOpen's saved statistics
 *   ws           : coattn_bn_exact_workspace_bytes, the per-workgroup partials; contents need no initialisation
 * Every pointer 16-byte aligned.  Argument errors (a shape that is not covered, a NULL or misaligned pointer, y == x, momentum
 * outside [0, 1], eps <= 0): -1 before any HIP call; the workspace size of a shape that is not covered is 0. */
int coattn_bn_exact_geometry(int B, int H, int W, int C, int dtype, int* out);
size_t coattn_bn_exact_workspace_bytes(int B, int H, int W, int C);
int coattn_bn_exact_forward(const void* x, const void* gamma, const void* beta, void* running_mean, void* running_var,
                            double momentum, double eps, void* y, void* save_mean, void* save_invstd, void* ws, int B, int H,
                            int W, int C, int pool, int relu, int dtype, void* stream);

/* ---- layer 1 of the frozen encoder: convolution, BatchNorm, ReLU and pool with the STOCK kernels' bits (v0.16.0) ----
 * conv2d(image, weight, padding 1) for 3 -> 64 channels and a 3x3 kernel, stride 1, no bias, in the arithmetic of the
 * Composable Kernel grouped convolution MIOpen runs this layer with: gemm-k = (ky, kx, c), c fastest, 27 terms padded with
 * zeros to 32; every output one chain from 0 of sixteen v_mfma_f32_32x32x2_f32, MFMA i adding the terms 16 (i / 8) + i % 8 and
 * that + 8 (lane half g holds the terms 8 g .. 8 g + 7 of each block of 16); a tap outside the image is a zero that is
 * multiplied all the same
 * (an infinite weight gives NaN along the border, as the stock kernel does).  One kernel writes x and adds it into the
 * statistics in the order of coattn_bn_exact_forward's first kernel (the wave that computes a pixel group's outputs owns its
 * sums); the second and third kernel of that call then run unchanged on x: the results are those of coattn_bn_exact_forward on x.
 *   coattn_conv1_bn_exact_supported : 1 only for dtype COATTN_F32, Cin = 3, Cout = 64 and a (B, H, W, 64) that
 *                  coattn_bn_exact_geometry covers (with pool: H, W >= 2); no GPU call
 *   image        : fp32, physically [B][H][W][3] (a channels_last [B,3,H,W] tensor), 4-byte aligned; read only
 *   weight       : fp32, physically [64][3][3][3] = [co][ky][kx][c] (a channels_last [64,3,3,3] tensor), 4-byte aligned; read only
 *   x_out        : fp32 [B][H][W][64], written: the convolution; or NULL: x is kept in ws (size it with with_x = 1)
 *   y, gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_invstd, pool, stream : as for
 *                  coattn_bn_exact_forward (the ReLU is always applied)
 *   ws           : coattn_conv1_bn_exact_workspace_bytes(B, H, W, with_x): the partials, then x if with_x; 16-byte aligned
 * Argument errors (a shape that is not covered, a NULL or misaligned pointer, aliased image / x_out / y, momentum outside
 * [0, 1], eps <= 0): -1 before any HIP call; the workspace size of a shape that is not covered is 0.
 * coattn_conv1_probe -- DEVELOPER ONLY, not part of the stable interface: the entry tools/probe_conv1_exact.py drives, kept so that
 * the arithmetic can be probed again when MIOpen changes its solver; nothing in the package calls it -- x alone, by a slow kernel of one thread per output whose chain is switchable
 * -- order 0 .. 5: (ky,kx,c) (ky,c,kx) (c,ky,kx) (kx,ky,c) (c,kx,ky) (kx,c,ky), last fastest, 28 terms; order 6 + 2 j + f:
 * (ky,kx,c) padded to 32 and taken in pairs (t, t + D) within blocks of 2 D, D = 8, 4, 2, 16 for j = 0 .. 3, f = 1 the upper
 * term first; step 0 fmaf, 1 multiply then add; halves 1, or 2: two chains over the halves of the terms, added; skip 1: zero
 * terms left out -- or, order -1 / -2, by the fast kernel with D = 8 (the one the forward call runs) / D = 4.  ws as above
 * with with_x = 0. */
int coattn_conv1_bn_exact_supported(int B, int H, int W, int Cin, int Cout, int pool, int dtype);
size_t coattn_conv1_bn_exact_workspace_bytes(int B, int H, int W, int with_x);
int coattn_conv1_bn_exact_forward(const void* image, const void* weight, const void* gamma, const void* beta, void* running_mean,
                                  void* running_var, double momentum, double eps, void* x_out, void* y, void* save_mean,
                                  void* save_invstd, void* ws, int B, int H, int W, int Cin, int Cout, int pool, int dtype,
                                  void* stream);
int coattn_conv1_probe(const void* image, const void* weight, void* x, void* ws, int B, int H, int W, int order, int step,
                       int halves, int skip, void* stream);

/* ---- layer 1 with the convolution computed twice and never stored (v0.22.0) ----
 * The results of coattn_conv1_bn_exact_forward bit for bit -- y, save_mean, save_invstd and the running statistics -- without
 * x: the first kernel is that call's with its stores left out (the statistics in the same order), the second is unchanged, the
 * third computes the same chain of MFMAs again and applies the normalise map, the 2x2 maximum and the ReLU of
 * coattn_bn_exact_forward's third kernel (the same device functions, the window's members in the same order) in registers.  y
 * is the only large tensor written; the image is read twice.
 *   coattn_conv1_bn_recompute_workspace_bytes : the partials alone (coattn_conv1_bn_exact_workspace_bytes with with_x = 0)
 *   every argument : as for coattn_conv1_bn_exact_forward, which has x_out in addition; the same shapes
 *                  (coattn_conv1_bn_exact_supported), pool 0 or 1, the ReLU always applied
 * The third kernel's workgroup takes COATTN_CONV1_RECOMPUTE_CHUNK consecutive samples of one tile (pooled: 2 image rows x 16
 * columns; not pooled: 32 consecutive pixels).
 * Argument errors (a shape that is not covered, a NULL or misaligned pointer, y == image, momentum outside [0, 1], eps <= 0):
 * -1 before any HIP call; the workspace size of a shape that is not covered is 0. */
#define COATTN_CONV1_RECOMPUTE_CHUNK 8
size_t coattn_conv1_bn_recompute_workspace_bytes(int B, int H, int W);
int coattn_conv1_bn_recompute_forward(const void* image, const void* weight, const void* gamma, const void* beta,
                                      void* running_mean, void* running_var, double momentum, double eps, void* y,
                                      void* save_mean, void* save_invstd, void* ws, int B, int H, int W, int Cin, int Cout, int pool,
                                      int dtype, void* stream);

/* ---- the sentence LSTM of the question hierarchy (v0.17.0; csrc/lstm.hip) ----
 * Reference model.py:286-296 -- pack_padded_sequence -> nn.LSTM (one layer, one direction, zero initial state) ->
 * pad_packed_sequence -- restated without packing, lengths read on the device:
 *   gates_t = X[:,t] W_ih^T + b_ih + h_{t-1} W_hh^T + b_hh          (gate order i, f, g, o: nn.LSTM's storage)
 *   c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g)      h_t = sigmoid(o) tanh(c_t)
 *   out[b,t,:]      = t < len_b ? h_t[b]   : 0         (selected, not multiplied: exact zeros)
 *   x_masked[b,t,:] = t < len_b ? X[b,t,:] : 0         (the phrase level as pad_packed_sequence returns it)
 * Exact fp32 only (the f32 MFMA and the three-piece projections): `flags` must be 0, any precision flag (COATTN_FLAG_FAST16,
 * COATTN_FLAG_BF16_PROJ, ...) is refused with -1.
 *   X            : fp32 [B][T][E], read only.  No output or gradient depends on the rows t >= len_b, for any values there of
 *                  magnitude up to 3.38e38 (bf16's largest finite value), the range of the projections' bf16 pieces that
 *                  live rows have too: dW_ih = dgates^T X multiplies those rows by the exact zeros of dgates, and a larger
 *                  value rounds to infinity in its leading piece (0 * inf = NaN in dW_ih).
 *   len          : int32 [B] on the device.  Values outside [1, T] are clamped on the device (0 acts as 1, T + 5 as T), as
 *                  in the *_len entry points; no order is required and nothing reads them on the host.  THE BACKWARD MUST BE
 *                  GIVEN THE SAME VALUES AS THE FORWARD that wrote `saved` (the saved state holds zeros past them).
 *   p            : W_ih [4H][E], W_hh [4H][H], b_ih [4H], b_hh [4H] as nn.LSTM stores weight_ih_l0 ... bias_hh_l0
 *   out          : fp32 [B][T][H], written
 *   x_masked     : fp32 [B][T][E], written; may be NULL
 *   saved        : `saved` bytes of the workspace size call, written for the backward: the activated gates [B][T][4H], the
 *                  cell state [B][T][H] and h_prev [B][T][H] (h_prev[b][t] = out[b][t-1], zeros at t = 0), zeros on the rows
 *                  past a length.  NULL: forward only (`out` has the same bits).
 *   ws           : ws_fwd / ws_bwd bytes, contents need no initialisation.  The backward reads nothing of the forward's.
 * Backward: g_out [B][T][H] and g_xmasked [B][T][E] (may be NULL) are the gradients at out and x_masked; their rows
 * t >= len_b are not read for their values.  dX [B][T][E] (may be NULL: the product is skipped, the parameter gradients keep
 * their bits) = the LSTM's gradient + g_xmasked on live rows, exact zeros on the others.  pg: dW_ih, dW_hh, db_ih, db_hh
 * (db_ih = db_hh = the column sums of the gate gradients); accumulate bit 0 adds onto the four.  The backward reads X, len, p,
 * saved and the two incoming gradients, nothing else.  `out` is NOT read -- h_{t-1} of every row is h_prev in `saved` -- and
 * is reserved: it may be NULL (it is only checked for alignment), and a caller need not keep the forward's out for this call.
 * One launch per time step in each direction, chained on the stream; every launch is deterministic (fixed-order sums, no
 * float atomics): same inputs, same bits.  A non-finite value in a live row of one sample reaches that sample's rows of out
 * and dX only (and the parameter gradients).
 * Supported (the query returns 1): dtype COATTN_F32, B >= 1, 1 <= T <= 64, E and H multiples of 32 in 32 .. 2048, and
 * B T 4 max(E, H) < 2^31 (32-bit element offsets of the GEMM layer).  Every buffer 16-byte aligned.
 * Argument errors (a NULL required pointer, a non-positive size, flags != 0, another dtype, an unsupported shape, a
 * misaligned buffer): -1 with a coattn_last_error message before any device work.  No allocation, no synchronisation. */
typedef struct coattn_lstm_params      { const void *w_ih, *w_hh, *b_ih, *b_hh; } coattn_lstm_params;
typedef struct coattn_lstm_param_grads { void *w_ih, *w_hh, *b_ih, *b_hh; } coattn_lstm_param_grads;
int coattn_lstm_supported(int B, int T, int E, int H, int dtype);
int coattn_lstm_workspace_bytes(int B, int T, int E, int H, int dtype, size_t* saved, size_t* ws_fwd, size_t* ws_bwd);
int coattn_lstm_forward(const void* X, const int32_t* len, const coattn_lstm_params* p, void* out, void* x_masked,
                        void* saved, void* ws, int B, int T, int E, int H, int dtype, int flags, void* stream);
int coattn_lstm_backward(const void* X, const int32_t* len, const coattn_lstm_params* p, const void* out, const void* saved,
                         const void* g_out, const void* g_xmasked, void* dX, const coattn_lstm_param_grads* pg,
                         int accumulate, void* ws, int B, int T, int E, int H, int dtype, int flags, void* stream);

/* ---- the word level of the question hierarchy: embedding gather and its dense gradient (v0.18.0; csrc/embedding.hip) ----
 * Reference model.py: nn.Embedding(V, E, padding_idx) over the question's token ids, in front of the phrase and sentence levels.
 *   ids          : n = B T token ids, contiguous, int32 (ids_dtype = COATTN_IDS_I32) or int64 (COATTN_IDS_I64, a LongTensor as
 *                  it is: all 64 bits are compared, no conversion launch); aligned to their element size; read on the device only
 *   W, dW        : fp32 [V][E];  out, g_out : fp32 [n][E];  all contiguous and 16-byte aligned
 *   padding_idx  : -1 = none, else in [0, V)
 *   bad_ids      : one int32 on the device, may be NULL; the forward ADDS to it (an integer atomic: the count is exact), the
 *                  caller zeroes it
 *   ws           : reserved, may be NULL: coattn_embedding_workspace_bytes reports ws_bwd = 0 (the row owners index the ids in
 *                  LDS; nothing the library keeps grows with V E, and nothing it would keep holds anything but integers)
 * Exact fp32 only: dtype must be COATTN_F32 and `flags` 0; any precision flag is refused with -1.
 * Forward (one launch, 16-byte accesses): out[i] = W[ids[i]] bit for bit -- row padding_idx too, as it is stored (what the stock
 * module does).  An id outside [0, V) -- negative, >= V, or an int64 whose low 32 bits alone would be a valid row -- gives a row
 * of exact +0 and adds 1 to *bad_ids; it is never used as an index, and no address outside W is formed.
 * Backward (ONE launch: no sort, no fill or memset of dW, no float atomics, no host read): dW[v] = sum of g_out[i] over the
 * positions i with ids[i] == v, for every v other than padding_idx.  Positions whose id is padding_idx or outside [0, V) are
 * left out by selection: their g_out rows are never loaded, so NaN or 1e30 there changes no bit.  Every element of dW is
 * written exactly once (the caller need not zero it); row padding_idx and every row without an occurrence are exact +0.
 * accumulate bit 0: dW[v] = dW[v] + sum (one rounding per element) on the rows with an occurrence, the other rows keep their
 * bits (they are not written).
 * SUMMATION ORDER, a pure function of ids (never of scheduling): let p_0 < p_1 < ... < p_{m-1} be the flat positions of token
 * v (padding and out-of-range positions excluded) and c = COATTN_EMBEDDING_CHUNK.  Chunk k holds the occurrences k c ..
 * min(m, (k+1) c) - 1 and is summed serially from its first element: s_k = ((g[p_kc] + g[p_kc+1]) + g[p_kc+2]) + ... .  The chunk
 * sums are combined left to right from the first: dW[v] = ((s_0 + s_1) + s_2) + ... .  One occurrence is therefore a copy (the
 * sign of a zero included); a token that fills a batch costs m / c + c dependent additions, not m.
 * A non-finite value in a live g_out row reaches exactly its token's row of dW.  Same inputs, same bits.
 * Supported (the query returns 1): dtype COATTN_F32, 1 <= n <= 65,536 (the positions are held as 16 bits in LDS), 1 <= V <=
 * 16,777,216 (2^24), E a multiple of 4 in 4 .. 2048.  Offsets into W, out, g_out and dW are 64-bit.
 * Argument errors (a NULL required pointer, a non-positive size, flags != 0, another dtype or ids_dtype, an unsupported shape,
 * padding_idx outside [-1, V), a misaligned buffer): -1 with a coattn_last_error message before any device work.  No
 * allocation, no synchronisation. */
#define COATTN_IDS_I32 0
#define COATTN_IDS_I64 1
#define COATTN_EMBEDDING_CHUNK 32
int coattn_embedding_supported(long long n, long long V, int E, int dtype);
int coattn_embedding_workspace_bytes(long long n, long long V, int E, int dtype, size_t* ws_bwd);
int coattn_embedding_forward(const void* ids, int ids_dtype, const void* W, void* out, int32_t* bad_ids, long long n, long long V,
                             int E, long long padding_idx, int dtype, int flags, void* stream);
int coattn_embedding_backward(const void* ids, int ids_dtype, const void* g_out, void* dW, void* ws, long long n, long long V,
                              int E, long long padding_idx, int accumulate, int dtype, int flags, void* stream);

/* ---- feature dropout: a counter RNG, the mask regenerated in the backward (v0.19.0; csrc/dropout.hip) ----
 * Lu et al. 2016 apply dropout 0.5 to every q_l + v_l in front of the recursive answer encoding.  Here it is one launch on the
 * attended features between the co-attention and the answer head (fp32, contiguous, n elements), and one launch on their
 * gradient.  No mask is stored, no float atomics are used, nothing is read on the host.
 * MASK DEFINITION (the contract; tests/_dropout.py restates it in numpy):
 *   - Element i of n has block j = i >> 2 and word w = i & 3.
 *   - r = Philox4x32-10(counter = (lo32(j), hi32(j), lo32(step), hi32(step)), key = (lo32(seed), hi32(seed)))[w].
 *   - The constants are the standard ones: multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85,
 *     ten rounds.
 *   - thr = (uint32) floor((double)p * 2^32).  An element is kept iff r >= thr.
 *   - scale = (float)(1.0 / (1.0 - (double)p)).
 *   - y[i] = x[i] * (keep ? scale : 0.0f).  This is a float multiply: NaN and inf propagate as in
 *     torch.nn.functional.dropout (a dropped inf or NaN is NaN), a dropped negative value gives -0.
 *   - With n <= 2^31 - 4, counter word 1 is always 0.  It is in the contract so that a later, larger limit does not change any
 *     mask.
 * p = 0 keeps every element and multiplies it by 1.0f.  The 16-byte and the per-element form of the kernel (chosen by the
 * alignment of the launch's pointers) give the same bits.
 * STATE: a 32-byte device buffer the caller owns, 4-byte aligned: u64 seed, u64 step (both little-endian word pairs), then 16
 * bytes for the library's own use (a ticket: 0 between calls; the caller zeroes them once).  `step` is the index of the mask
 * most recently drawn.  The caller may rewrite seed and step between calls, in stream order.
 *   coattn_dropout_forward   y0 = x0 * mask and, when x1 / y1 are given, y1 = x1 * mask with the SAME mask (x1 = y1 = NULL: one
 *                            pair).  advance = 1: draws mask step + 1 and leaves `step` incremented when the call has completed
 *                            on the stream (the workgroup that finishes last stores it; no second launch).  advance = 0: redraws
 *                            mask `step` and writes nothing to the state.  y may equal x (in place); any other overlap is the
 *                            caller's error.
 *   coattn_dropout_backward  dx = g * mask(step); in place allowed.  It never advances: any number of backwards after one
 *                            forward see that forward's mask.
 *   coattn_dropout_supported 1 for 1 <= n <= 2^31 - 4, else 0.
 * Refused with -1 and a coattn_last_error message, nothing launched: p < 0, p >= 1 or p NaN; n outside the supported range; a
 * NULL x0, y0, g, dx or state; exactly one of x1 / y1 given; a pointer not 4-byte aligned.
 * The calls are stream-ordered; no allocation, no synchronisation, no host read, no host-side state: they can be captured into
 * a HIP graph, and each replay of an advancing forward draws a fresh mask.  Two advancing forwards on one state must be ordered
 * (one stream, or an event between them). */
int coattn_dropout_supported(long long n);
int coattn_dropout_forward(const void* x0, void* y0, const void* x1, void* y1, long long n, float p, void* state, int advance,
                           void* stream);
int coattn_dropout_backward(const void* g, void* dx, long long n, float p, void* state, void* stream);

/* ---- cached image features: the rows of a batch gathered from a feature table (v0.20.0; csrc/features.hip) ----
 * The frozen image encoder is a fixed function of the image, so its features can be encoded once into a table and a training or
 * prediction step reads the rows of its batch instead of running the encoder (Lu et al. 2016 train from such features).
 *   table     : [S][N][d], contiguous and location-major (what coattn_features_native writes per image), fp32 (table_dtype =
 *               COATTN_F32) or bf16 (COATTN_BF16: the 16 stored bits); 16-byte aligned; read only
 *   idx       : B row indices, contiguous, int32 (idx_dtype = COATTN_IDS_I32) or int64 (COATTN_IDS_I64: all 64 bits are
 *               compared); aligned to their element size; read on the device only, never on the host
 *   out       : fp32 [B][N][d], contiguous, 16-byte aligned
 *   bad_idx   : one int32 on the device, may be NULL; the call ADDS to it (an integer atomic: the count is exact), the caller
 *               zeroes it
 * out[b] = table[idx[b]]: bit for bit from an fp32 table; from a bf16 table the exact up-cast -- the sixteen bits become the
 * high half of the fp32 word, so infinities, NaN payloads, denormals and the sign of a zero are kept.  An index outside [0, S)
 * -- negative, >= S, or an int64 whose low 32 bits alone would be a valid row -- gives a row of exact +0 and adds 1 to
 * *bad_idx; it is never used as an index, and no address outside `table` is formed.  Repeated indices are fine.
 * One launch of 16-byte loads and stores with 64-bit element offsets (S N d may pass 2^31 elements and 2^32 bytes).  No float
 * arithmetic, no atomics on floats: same inputs, same bits.  A row is cut into passes of COATTN_FEATURES_THREADS *
 * COATTN_FEATURES_LOADS 16-byte loads (4 fp32 or 8 bf16 elements each), one workgroup per (row, pass).
 * Supported (the query returns 1): table_dtype COATTN_F32 or COATTN_BF16, flags 0, S >= 1, B >= 1, 1 <= N <= 4096, 1 <= d <=
 * 2048, N d a multiple of 4 (fp32) or 8 (bf16), and B times the passes of a row at most 2^24 - 1 (B <= 8,191 for the largest
 * row there is; 16,777,215 for a row of one pass).
 * Argument errors (a NULL table, idx or out, a non-positive size, flags != 0, another table_dtype or idx_dtype, an unsupported
 * shape, a misaligned buffer): -1 with a coattn_last_error message before any device work.  No allocation, no synchronisation;
 * the call can be captured into a HIP graph. */
#define COATTN_FEATURES_THREADS 256
#define COATTN_FEATURES_LOADS 4
int coattn_features_gather_supported(long long S, long long B, int N, int d, int table_dtype, int flags);
int coattn_features_gather(const void* table, int table_dtype, const void* idx, int idx_dtype, void* out, int32_t* bad_idx,
                           long long S, long long B, int N, int d, int flags, void* stream);

/* ---- attention overlays: the maps drawn over the image they were computed from (v0.21.0; csrc/overlay.hip) ----
 * What coattn_infer returns, as pictures: each level's image attention upsampled to the image's size and blended into the
 * de-normalised image, and under it a strip of that level's question attention.  One launch, 64-bit output offsets, no
 * allocation, no synchronisation, nothing read on the host but `p`: the call can be captured into a HIP graph.
 *   image     : fp32 [B][3][H][W] at the element strides sB, sC, sH, sW (any: NCHW, channels-last, padded rows); normalised as
 *               (x - mean) / std per channel.  A contiguous image -- sW = 1 and sB, sC, sH multiples of 4 -- is read with 16-byte
 *               loads and must be 16-byte aligned; any other is read element by element (4-byte aligned)
 *   a_v       : fp32 [L][B][Gh*Gw], the row-major grid coattn_infer writes (av_out)
 *   a_q       : fp32 [L][B][T] (aq_out), or NULL (then strip_h must be 0); read only when strip_h > 0
 *   q_len     : B int32 question lengths on the device, or NULL (every row has T entries); a length is clamped to [1, T]
 *   p         : host structure, below; p->lut a device pointer to fp32 [256][3] in [0, 1], read by the heat mode only
 *   out       : uint8 [B][L+1][H+strip_h][W][3], interleaved RGB, 16-byte aligned.  Panel 0 is the de-normalised image (its
 *               strip rows are 0), panel 1+l is level l; every byte is written
 *   bad_maps  : one int32 on the device, may be NULL; the call ADDS to it (one integer atomic per bad map), the caller zeroes it
 * One workgroup of COATTN_OVERLAY_THREADS threads owns a band of COATTN_OVERLAY_ROWS output rows of one sample for all
 * panels: it reads the image band once and writes L+1 bands; the sample's L maps and their reciprocal maxima are found by the
 * workgroup itself in LDS.  A thread takes 4 pixels at a time and stores them as 12 bytes = 3 whole dwords (hence W % 4 == 0).
 *
 * THE ARITHMETIC IS THE CONTRACT.  Every line is one correctly rounded fp32 operation, in this order, none contracted into an
 * FMA; the same inputs give the same bytes on every run and in every layout of the image.
 *   Map normalisation, per (l, b):   mx = max a_v;   r = 1.0f / mx;   m[n] = a[n] * r.
 *     A map is BAD if an entry is NaN, +-inf or < 0, if mx == 0, or if r is not finite (a denormal maximum).  A bad map renders as
 *     m = 0 everywhere and adds exactly 1 to *bad_maps (by the workgroup of the sample's band 0 only).  a_q follows the same rule
 *     over its first len_b entries (all T where q_len is NULL), with its own r_q; a bad a_q row counts as well.
 *   Bilinear upsampling, half-pixel centres, edges clamped (F.interpolate(mode="bilinear", align_corners=False)):
 *     sy = (float)Gh / (float)H;   src = ((float)y + 0.5f) * sy - 0.5f;   src = max(src, 0);
 *     i0 = min((int)floor(src), Gh-1);   i1 = min(i0+1, Gh-1);   w1 = src - (float)i0;   w0 = 1 - w1;   the same in x (Gw, W);
 *     top = m[i0,j0]*wx0 + m[i0,j1]*wx1;   bot likewise on row i1;   u = top*wy0 + bot*wy1.     (H < Gh, downsampling, included)
 *   Pixel:   xh_c = clamp01(img * std_c + mean_c), clamp01(x) = x >= 0 ? (x <= 1 ? x : 1) : 0 -- a NaN pixel gives 0 and
 *     touches that pixel only;
 *     COATTN_OVERLAY_MASK (brightness follows attention):   g = floor + (1-floor)*u, 1-floor computed once;   o_c = xh_c * g;
 *     COATTN_OVERLAY_HEAT:   k = (int)(u*255 + 0.5f);   o_c = (1-alpha)*xh_c + alpha*lut[k][c], 1-alpha computed once;
 *     byte = (int)(clamp01(o_c)*255 + 0.5f);   panel 0: o_c = xh_c.
 *   Question strip, the rows y >= H of panels 1..L:   T cells, cell t = (x*T) / W in integers;   m_q = a_q[l][b][t] * r_q;
 *     heat: the colour lut[(int)(m_q*255 + 0.5f)], mask: the grey m_q, each through `byte`;   cells t >= len_b are 0.
 * Supported (the query returns 1): B >= 1, 1 <= L <= 8, 1 <= H, W <= 4096, W % 4 == 0, 1 <= Gh, Gw <= 64, 0 <= strip_h <= 4096,
 * strip_h == 0 or 1 <= T <= min(W, 4096), mode one of the two, and B times the bands of a sample below 2^31.
 * Argument errors -- an unsupported shape or mode, strip_h > 0 without a_q, a NULL image, a_v, p or out, the heat mode without
 * p->lut, alpha or floor outside [0, 1], a std that is not finite or is 0, a mean that is not finite, a misaligned buffer --: -1
 * with a coattn_last_error message before any device work. */
#define COATTN_OVERLAY_HEAT 0
#define COATTN_OVERLAY_MASK 1
#define COATTN_OVERLAY_ROWS 8
#define COATTN_OVERLAY_THREADS 256
typedef struct coattn_overlay_params {
  float mean[3];        /* the image's normalisation: pixel = img * std + mean */
  float std[3];
  float alpha;          /* heat mode: the weight of the colour */
  float floor;          /* mask mode: the brightness where the attention is 0 */
  const void* lut;      /* device fp32 [256][3] in [0, 1]; heat mode only (else may be NULL) */
} coattn_overlay_params;
int coattn_overlay_supported(int B, int L, int H, int W, int Gh, int Gw, int T, int strip_h, int mode);
int coattn_overlay_render(const void* image, int64_t sB, int64_t sC, int64_t sH, int64_t sW, const void* a_v, const void* a_q,
                          const int32_t* q_len, const coattn_overlay_params* p, void* out, int32_t* bad_maps, int B, int L, int H,
                          int W, int Gh, int Gw, int T, int strip_h, int mode, void* stream);

/* ---- building blocks (exported for the per-kernel parity tests) ------------------------ */

/* Strided, batched fp32 GEMM on the f32 MFMA:
 *   C[z](m,n) = act( out_scale * (sum_{i<inner} sum_k A[z,i](m,k) * B[z,i](k,n) + bias_n[n] + bias_m[m])
 *                    + beta * Cin[z](m,n) )
 * Row m of A / C / Cin lives at (m / mdiv) * sdiv + (m % mdiv) * sm (mdiv = 0: plain m * sm).
 * ksplit > 0: batch index z selects the k range [z*ksplit, min(K,(z+1)*ksplit)) instead.
 * inner_total > 0: z is a group of `inner` consecutive inner indices ig = z*inner + i < inner_total.
 * Pointer tables (level-merged launches; NULL entries = unused): a_ptrs/b_ptrs/c_ptrs/cin_ptrs[t]
 * replace A/B/C/Cin with t = z (ptr_by_inner = 0) or t = ig (ptr_by_inner = 1).
 * b_imod > 0: the inner stride of B wraps, B[ig] = B + (ig % b_imod) * b_si.
 * kband_n > 0 (multiple of 128, at most 3 bands): columns [j*kband_n, (j+1)*kband_n) contract only
 * over k in [kband_lo[j], kband_hi[j]) -- block-sparse B operands (n-gram taps of phrase.hip).  The bounds are
 * multiples of 4 inside [0, K]; lo == hi is an empty band (C = act(out_scale * biases + beta * Cin)); B is never
 * read outside its bands.
 * NaN and inf propagate: a non-finite element of A reaches exactly its row of C, one of B its column -- in the
 * bf16 modes too (the staging keeps every NaN pattern a NaN). */
typedef struct coattn_gemm_desc {
  const void* A; const void* B; const void* Cin; void* C;
  const void* bias_n; const void* bias_m;
  int M, N, K, batch, inner, inner_total, ksplit, act; /* act: 0 none, 1 tanh */
  float beta;
  int64_t a_sm, a_sk, a_sz, a_si, a_mdiv, a_sdiv;
  int64_t b_sk, b_sn, b_sz, b_si;
  int64_t c_sm, c_sn, c_sz, c_mdiv, c_sdiv;
  int64_t cin_sm, cin_sn, cin_sz, cin_mdiv, cin_sdiv;
  const void* a_ptrs[8]; const void* b_ptrs[8]; void* c_ptrs[8]; const void* cin_ptrs[8];
  int ptr_by_inner; int b_imod;
  int kband_n; int kband_lo[3]; int kband_hi[3];
  float out_scale;          /* 0 or 1: plain; else C = act(out_scale * (products + biases) + beta * Cin) */
} coattn_gemm_desc;

int coattn_gemm_f32(const coattn_gemm_desc* g, void* stream);

/* ---- nn.Linear against a pre-split weight ----------------------------------------------------------------
 * y[M][N] = out_scale * (x[M][K] W[N][K]^T + bias[N]) in fp32 accuracy (the W_v / W_q projections of
 * ParallelCoAttention.forward, model.py:380-384: x rows ld_x floats apart, W as nn.Linear stores it).
 * The weight is split once into its three bf16 pieces in MFMA-fragment order (`wimg`, device scratch of
 * coattn_linear_workspace_bytes(N, K) bytes) and the GEMM reads the fragments in place (gemm_w.hip) -- the
 * kernel pair coattn_forward uses for both projections.  flags bit 0: `wimg` already holds the image of this
 * W (skip the split) -- WRITTEN BY A CALL WITH THE SAME N, K, precision flags (bits 2, 3) AND ON THE SAME KERNEL: the image's
 * format belongs to the kernel that reads it (three-piece fragments for gemm_w.hip, hi-only 1 KB chunks for gemm_bf.hip), and
 * which kernel runs depends on M (>= 256 for gemm_bf.hip; a ragged last row tile is masked), ld_x and the alignment of x as well.  Reuse
 * an image only across calls of one shape class -- e.g. the steps of a loop over equal batches; a last partial batch with
 * another M must split again.  The library cannot check this (the image carries no tag).  flags bit 2 (COATTN_FLAG_BF16_PROJ): operands rounded to bf16, one MFMA per product.  K % 32 == 0, M >= 128, x 16-byte aligned with ld_x % 4 == 0; other shapes: error -1
 * (use coattn_gemm_f32).  bias may be NULL; out_scale 0 means 1.
 * flags bit 3 (COATTN_FLAG_BF16_IN, with bit 2): x holds bf16 elements (ld_x in elements, % 8 == 0) -- the activations of
 * an autocast encoder, or the fused backward's own bf16 gradients -- read as they are by the wide-shape kernel
 * (gemm_bf.hip: M >= 256, N % 256 == 0, K % 64 == 0; other shapes: error -1). */
size_t coattn_linear_workspace_bytes(int N, int K);
int coattn_linear_forward(const void* x, int64_t ld_x, const void* W, const void* bias, void* y, void* wimg,
                          int M, int N, int K, float out_scale, int flags, void* stream);

/* Weight gradient of the same layer: dW[n_out][n_in] (+)= dY[M][n_out]^T X[M][n_in] in fp32 accuracy
 * (autograd of the W_v / W_q projections, main.py:219-220): split-K parts on the hand-scheduled A^T B kernel
 * (gemm_tn.hip) + a deterministic reduce -- the kernel pair coattn_backward uses for dW_v and dW_q.
 * dY rows ld_dy floats apart, X rows ld_x; `ws`: device scratch of coattn_linear_wgrad_workspace_bytes bytes.
 * n_out, n_in multiples of 128, M >= 16, 16-byte aligned operands with ld % 4 == 0; other shapes: error -1.
 * accumulate: bit 0 adds onto dW; bit 2 (COATTN_FLAG_BF16_PROJ) selects the reduced-precision mode; bit 3
 * (COATTN_FLAG_BF16_IN, with bit 2): dy holds bf16 elements (ld_dy % 8 == 0; n_out, n_in % 256 == 0, M % 32 == 0). */
size_t coattn_linear_wgrad_workspace_bytes(int n_out, int n_in);
int coattn_linear_weight_grad(const void* dy, int64_t ld_dy, const void* x, int64_t ld_x, void* dW, void* ws, int M,
                              int n_out, int n_in, int accumulate, void* stream);

/* Same contract with the operands rounded to bf16 (round to nearest even) while they are staged and
 * contracted on v_mfma_f32_32x32x16_bf16 (fp32 accumulate / output): the arithmetic of
 * COATTN_FLAG_BF16_PROJ.  Every shape the aligned path of coattn_gemm_f32 takes runs in this mode with every
 * field of the descriptor.  Of the others (unaligned strides, M < 128), a plain product with B contiguous along
 * k -- A, B, C, bias_n, out_scale, an a_ptrs table by batch and the row splits of A and C, nothing else -- does
 * too; any further field (Cin or a cin_ptrs table, bias_m, act, inner > 1, an inner_total below batch, ksplit,
 * b_imod, kband_n, b_ptrs, c_ptrs, ptr_by_inner) or an unaligned A or B makes such a shape an exact fp32 product instead. */
int coattn_gemm_bf16(const coattn_gemm_desc* g, void* stream);

/* ---- one-shot gradient exchange over peer-mapped buckets (data-parallel training) -----------
 * The reference trains on one GPU (multi-GPU is a TODO: main.py:71, :102-106).  The co-attention model shards by QA
 * pair, so the only exchange is the gradient mean; on a fully connected xGMI node the pattern that fits is one shot:
 * every rank maps its peers' gradient buckets (HIP IPC, once) and two bandwidth kernels read peer memory directly.
 * peer_bufs[r] = rank r's bucket (world * shard_elems floats) as mapped in THIS process, peer_bufs[rank] its own.
 *   coattn_p2p_reduce_scatter  own bucket, shard `rank`  <-  scale * sum_r peer_bufs[r][shard `rank`], summed in rank
 *                              order (identical and repeatable on every rank);
 *   coattn_p2p_all_gather      own bucket, shard r  <-  peer_bufs[r][shard r] for every r != rank.
 * Both only ENQUEUE on `stream`; the caller orders the phases across ranks (every bucket packed before the first call,
 * every reduce done before the gather, every gather done before a bucket is packed again -- dist.py: a one-element
 * all-reduce on the stream under RCCL).  shard_elems % 4 == 0, 16-byte aligned buckets, world <= 8; else error -1. */
int coattn_p2p_enable_peer(int peer_device);   /* peer access from the current device to the device a mapped bucket lives on
                                                * (once per pair, before the first call below); -1 if they cannot reach each other */
int coattn_p2p_reduce_scatter(const void* const* peer_bufs, int world, int rank, int64_t shard_elems, float scale,
                              void* stream);
int coattn_p2p_all_gather(const void* const* peer_bufs, int world, int rank, int64_t shard_elems, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COATTN_H */
