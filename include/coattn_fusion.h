/*
 * coattn_fusion.h -- the fusion head of the baseline model, the entry points of libcoattn_hip.so after 0.25.0.  include/coattn.h
 * (the 78 functions of 0.22.0), include/coattn_ext.h (0.23.0, 0.24.0) and include/coattn_rnn.h (0.25.0: the four GRU functions)
 * stay as they are; the conventions are theirs: every pointer a DEVICE pointer unless marked "host", the caller owns every
 * buffer, calls asynchronous on `stream`, 0 on success and < 0 with a coattn_last_error message otherwise.  vqa_amd/_lib.py
 * tables these functions in FUSION_SIGNATURES.
 *
 * v0.26.0: the fusion head of the baseline model.
 */
#ifndef COATTN_FUSION_H
#define COATTN_FUSION_H

#include "coattn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the fusion head of the baseline model (v0.26.0; csrc/fusion.hip) ----
 * Reference model.py VQABaselineNet behind its two encoders: the tail of ImageBaselineEncoder.forward (F.normalize(p=2, dim=1) ->
 * Linear(Di, J) -> Tanh), QuestionBaselineEncoder.embedding_layer (Linear(H, J) -> Tanh), the elementwise product, mlp (Linear(J,
 * Mh) -> Dropout -> Tanh: the reference's order, dropout in FRONT of the tanh) and fc_final (Linear(Mh, K)).  f [B][Di] are the
 * image encoder's features (rows ld_f floats apart), h [B][H] the question GRU's last hidden state (rows ld_h floats apart).
 * Operation by operation in the order the kernels evaluate it (fp32; every product sum_k a[k] b[k] is one fma chain per wave on
 * v_mfma_f32_32x32x2_f32 -- wave w of eight takes the 32-wide k chunks w, w + 8, ... in increasing k -- and the eight partial
 * sums are added in wave order 0 .. 7 from a zero; the compiler may contract a product and the add behind it into one fma):
 *   ss_b    = sum_k f[b][k]^2             lane l of 64 adds k = 4 l + 256 t + e (t = 0, 1, ...; e = 0 .. 3) in increasing k as one
 *                                         fma chain from 0; the 64 lane sums meet in a fixed butterfly (lane distance 32, 16, 8,
 *                                         then i <-> i ^ 7, 2, 1)
 *   inv_b   = 1 / max(sqrtf(ss_b), 1e-12f)                     F.normalize's clamp: a zero row has ss = 0 and gives x^ = 0
 *   e_q     = tanh((h W_q^T) + b_q)                            [B][J]
 *   e_i     = tanh(inv_b * (f W_i^T) + b_i)                    [B][J]   THE NORMALISED FEATURES ARE NEVER FORMED: the row scale
 *                                                              is applied to the finished sum.  The reference normalises first
 *                                                              and multiplies then; the two orders differ by rounding only.
 *   pre     = ((e_i * e_q) W_m^T) + b_m                        [B][Mh]  (j = e_i * e_q is formed in the operand path, not stored)
 *   d       = p_drop > 0 ? pre * (keep ? scale : 0) : pre      keep, scale: exactly the mask of v0.19.0 (coattn.h, feature
 *                                                              dropout) over element index i = b Mh + n of the contiguous
 *                                                              [B][Mh] array, `drop_state` its 32-byte state
 *   m       = tanh(d)
 *   logits  = (m W_f^T) + b_f                                  [B][K] dense
 * Exact fp32 only: `flags` must be 0.
 *   p            : W_i [J][Di], b_i [J], W_q [J][H], b_q [J], W_m [Mh][J], b_m [Mh], W_f [K][Mh], b_f [K], dense, as nn.Linear
 *                  stores them
 *   saved        : `saved` bytes of the workspace size call, written by the TRAINING forward (saved != NULL), regions aligned to 64
 *                  floats: inv [B], e_i [B][J], e_q [B][J], m [B][Mh].  No mask and no j.  With p_drop > 0 the training forward
 *                  draws mask step + 1 and leaves the state's step incremented when it completes on the stream, as
 *                  coattn_dropout_forward(advance = 1) does (the last of its launches stores it: no extra launch); with p_drop == 0
 *                  the state is not read and may be NULL.
 *                  saved == NULL: inference.  p_drop must be 0, the logits have the bits of the saving forward at p_drop = 0 and
 *                  nothing but `logits` is written (the activations live in a stream-ordered allocation, hipMallocAsync /
 *                  hipFreeAsync on `stream`: no synchronisation).
 * Backward: g_logits [B][K] dense, REQUIRED, is the gradient at the logits.
 *   dm      = g W_f
 *   dpre    = dm * (1 - m * m) * (keep ? scale : 0)            mask `step` as the state holds it: regenerated, NEVER advanced --
 *                                                              two backwards after one forward give the same bits
 *   dj      = dpre W_m
 *   dp_i    = dj * e_q * (1 - e_i * e_i)          dp_q = dj * e_i * (1 - e_q * e_q)
 *   dW_i[n][k] = sum_b (dp_i[b][n] * inv_b) * f[b][k]          db_i[n] = sum_b dp_i[b][n]   (unscaled)
 *   dW_q    = dp_q^T h        db_q = sum_b dp_q        dh = dp_q W_q    [B][H] dense; may be NULL (the product is skipped, the
 *                                                                       parameter gradients keep their bits)
 *   dW_m    = dpre^T (e_i * e_q)   db_m = sum_b dpre   dW_f = g^T m   db_f = sum_b g
 * Every sum over b runs in increasing b, two rows per MFMA, as one fma chain (the bias sums: rows of even and of odd b as two
 * chains, added last).  accumulate bit 0 adds onto the eight parameter gradients.  THERE IS NO GRADIENT FOR f: the encoder in
 * front is frozen; a trainable image encoder is out of scope.  `ws`: ws_bwd bytes, contents need no initialisation.
 * Forward: 4 launches, backward: 3.  Every launch is deterministic (fixed-order sums, no float atomics): same inputs, same bits.
 * A non-finite value in row b of f or h reaches row b of logits and dh only (and the parameter gradients).
 * Supported (the query returns 1): dtype COATTN_F32, B >= 1, Di, H, J, Mh multiples of 4 in 4 .. 8192 (a row then starts on a
 * 16-byte boundary), K >= 2 (any K: the rows of logits and g_logits need no alignment), and every operand below 1 GB with the
 * tiles' overshoot: (B + 64) max(Di, H, J, Mh, K) < 2^28 and (K + 32) Mh < 2^28 (32-bit byte offsets below 2^30; B Mh <= 2^31 - 4
 * follows).  Per call: ld_f >= Di, ld_h >= H, both multiples of 4 with (B + 64) ld < 2^28; every buffer 16-byte aligned (the
 * dropout state: 4).
 * Argument errors (a NULL required pointer, p_drop outside [0, 1) or NaN, p_drop > 0 with a NULL state or with saved == NULL,
 * flags != 0, another dtype, an unsupported shape or leading dimension, a misaligned buffer): -1 with a coattn_last_error
 * message before any device work.  No allocation, no synchronisation. */
typedef struct coattn_fusion_params      { const void *W_i, *b_i, *W_q, *b_q, *W_m, *b_m, *W_f, *b_f; } coattn_fusion_params;   /* [J,Di] [J] [J,H] [J] [Mh,J] [Mh] [K,Mh] [K] */
typedef struct coattn_fusion_param_grads { void *W_i, *b_i, *W_q, *b_q, *W_m, *b_m, *W_f, *b_f; } coattn_fusion_param_grads;
int coattn_fusion_supported(int B, int Di, int H, int J, int Mh, int K, int dtype);
int coattn_fusion_workspace_bytes(int B, int Di, int H, int J, int Mh, int K, int dtype, size_t* saved, size_t* ws_bwd);
int coattn_fusion_forward(const void* f, int64_t ld_f, const void* h, int64_t ld_h, const coattn_fusion_params* p,
                          void* logits, void* saved, float p_drop, void* drop_state,
                          int B, int Di, int H, int J, int Mh, int K, int dtype, int flags, void* stream);
int coattn_fusion_backward(const void* f, int64_t ld_f, const void* h, int64_t ld_h, const coattn_fusion_params* p,
                           const void* saved, const void* g_logits, void* dh, const coattn_fusion_param_grads* pg,
                           int accumulate, float p_drop, void* drop_state, void* ws,
                           int B, int Di, int H, int J, int Mh, int K, int dtype, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
