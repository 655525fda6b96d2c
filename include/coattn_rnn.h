/*
 * coattn_rnn.h -- the recurrent entry points of libcoattn_hip.so after 0.24.0.  include/coattn.h (the 78 functions of 0.22.0) and
 * include/coattn_ext.h (0.23.0, 0.24.0) stay as they are; the conventions are theirs: every pointer a DEVICE pointer unless marked
 * "host", the caller owns every buffer, calls asynchronous on `stream`, 0 on success and < 0 with a coattn_last_error message
 * otherwise.  vqa_amd/_lib.py tables these functions in RNN_SIGNATURES.
 *
 * v0.25.0: the question GRU of the baseline model.
 */
#ifndef COATTN_RNN_H
#define COATTN_RNN_H

#include "coattn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the question GRU of the baseline model (v0.25.0; csrc/gru.hip) ----
 * Reference model.py QuestionBaselineEncoder -- pack_padded_sequence -> nn.GRU (one layer, one direction, zero initial state) ->
 * the hidden state after each question's last token -- restated without packing, lengths read on the device, in any order.
 * Gate order r, z, n (nn.GRU's storage).  One projection of all B T rows, then a live step (t < len_b) is, operation by operation
 * in the order the kernel evaluates it (fp32; the compiler may contract a product and the add behind it into one fma):
 *   Gx = X W_ih^T + b_ih                                                     all B T rows, one projection [B T][3H]
 *   hr = (h_{t-1} W_hr^T) + b_hr      hz = (h_{t-1} W_hz^T) + b_hz      hn = (h_{t-1} W_hn^T) + b_hn
 *   r  = sigmoid(Gx_r + hr)           z  = sigmoid(Gx_z + hz)           n  = tanh(Gx_n + r * hn)
 *   h_t = n + z * (h_{t-1} - n)                                              h_{-1} = 0; sigmoid(x) = 1 / (1 + expf(-x))
 *   seq_out[b,t,:] = t < len_b ? h_t[b] : 0          (selected, not multiplied: exact zeros)
 *   h_last[b,:]    = h_{len_b - 1}[b]                (written by the step kernel of step len_b - 1: no extra launch)
 * Exact fp32 only (the f32 MFMA and the three-piece projections): `flags` must be 0, any precision flag is refused with -1.
 *   X            : fp32 [B][T][E], read only.  No output or gradient depends on the rows t >= len_b, for any values there of
 *                  magnitude up to 3.38e38 (bf16's largest finite value): dW_ih = dGx^T X multiplies those rows by the exact
 *                  zeros of dGx, and a larger value rounds to infinity in the leading bf16 piece of the product's operand.
 *   len          : int32 [B] on the device.  Values outside [1, T] are clamped on the device (0 acts as 1, T + 5 as T); no order
 *                  is required and nothing reads them on the host.  THE BACKWARD MUST BE GIVEN THE SAME VALUES AS THE FORWARD
 *                  that wrote `saved` (the saved state holds zeros past them).
 *   p            : W_ih [3H][E], W_hh [3H][H], b_ih [3H], b_hh [3H] as nn.GRU stores weight_ih_l0 ... bias_hh_l0
 *   seq_out      : fp32 [B][T][H], written; REQUIRED: the recurrence reads h_{t-1} from it
 *   h_last       : fp32 [B][H], written; may be NULL
 *   saved        : `saved` bytes of the workspace size call, written for the backward, regions aligned to 64 floats: the activated
 *                  gates [B][T][3H] (r, z, n), hn [B][T][H] (the hidden-side pre-activation of n, b_hn included) and h_prev
 *                  [B][T][H] (h_prev[b][t] = seq_out[b][t-1], zeros at t = 0); zeros on the rows past a length.  NULL: forward
 *                  only (seq_out and h_last have the same bits).
 *   ws           : ws_fwd / ws_bwd bytes, contents need no initialisation.  The backward reads nothing of the forward's.
 * Backward: g_seq [B][T][H] and g_last [B][H] are the gradients at seq_out and h_last; each may be NULL (= zero), both NULL is
 * refused; the rows t >= len_b of g_seq are not read.  In reverse over the steps, for a live step:
 *   dh   = g_seq[b][t] + (t == len_b - 1 ? g_last[b] : 0) + (t + 1 < T ? dhc[b] + (dGh_{t+1} W_hh)[b] : 0)
 *   dnp  = dh * (1 - z) * (1 - n * n)        dzp = dh * (h_prev - n) * z * (1 - z)        drp = dnp * hn * r * (1 - r)
 *   dGx[b][t] = (drp, dzp, dnp)              dGh[b][t] = (drp, dzp, dnp * r)              dhc[b] = dh * z
 * and zeros in all three on a dead step.  TWO gradient arrays: the n gate multiplies the hidden-side product by r before the
 * tanh, so dGx feeds dW_ih = dGx^T X, db_ih and dX = dGx W_ih, and dGh feeds dW_hh = dGh^T h_prev, db_hh and the recurrent
 * product.  dX [B][T][E] may be NULL (the product is skipped, the parameter gradients keep their bits); its rows past a length
 * are exact zeros.  accumulate bit 0 adds onto the four parameter gradients.  The backward reads X, len, p, saved and the two
 * incoming gradients, nothing else.
 * One launch per time step in each direction, chained on the stream; every launch is deterministic (fixed-order sums, no float
 * atomics): same inputs, same bits.  A non-finite value in a live row of one sample reaches that sample's rows of seq_out,
 * h_last and dX only (and the parameter gradients).
 * Supported (the query returns 1): dtype COATTN_F32, B >= 1, 1 <= T <= 64, H a multiple of 32 in 32 .. 2048, E a multiple of 4 in
 * 4 .. 2048 (a row of X starts on a 16-byte boundary; the step kernels never read X, and the GEMM layer takes the widths that are
 * no multiple of 32 -- the baseline's 300 -- on its general kernels), and B T 3 max(E, H) < 2^31 (32-bit element offsets of the
 * GEMM layer).  Every buffer 16-byte aligned (len: 4).
 * Argument errors (a NULL required pointer, a non-positive size, flags != 0, another dtype, an unsupported shape, a misaligned
 * buffer, both gradients NULL): -1 with a coattn_last_error message before any device work.  No allocation, no synchronisation. */
typedef struct coattn_gru_params      { const void *w_ih, *w_hh, *b_ih, *b_hh; } coattn_gru_params;   /* [3H,E] [3H,H] [3H] [3H] */
typedef struct coattn_gru_param_grads { void *w_ih, *w_hh, *b_ih, *b_hh; } coattn_gru_param_grads;
int coattn_gru_supported(int B, int T, int E, int H, int dtype);
int coattn_gru_workspace_bytes(int B, int T, int E, int H, int dtype, size_t* saved, size_t* ws_fwd, size_t* ws_bwd);
int coattn_gru_forward(const void* X, const int32_t* len, const coattn_gru_params* p, void* seq_out, void* h_last, void* saved,
                       void* ws, int B, int T, int E, int H, int dtype, int flags, void* stream);
int coattn_gru_backward(const void* X, const int32_t* len, const coattn_gru_params* p, const void* saved, const void* g_seq,
                        const void* g_last, void* dX, const coattn_gru_param_grads* pg, int accumulate, void* ws,
                        int B, int T, int E, int H, int dtype, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
