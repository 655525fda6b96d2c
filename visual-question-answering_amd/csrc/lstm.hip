// Sentence LSTM of the question hierarchy (reference model.py:286-296: pack_padded_sequence -> nn.LSTM -> pad_packed_sequence),
// restated without packing: one layer, one direction, gate order i, f, g, o, zero initial state, per-sample lengths read on
// the device.  include/coattn.h "the sentence LSTM" holds the contract; DESIGN 3.13 the layout and the measurements.
//
//   forward   G_x = X W_ih^T + b_ih for all B T rows at once (gemm_w.hip, or gemm.hip for the shapes it refuses), then one
//             launch of lstm_fwd_step_kernel per time step; x_masked by lstm_mask_rows_kernel
//   backward  one launch of lstm_bwd_step_kernel per time step in reverse (dgates [B][T][4H], zeros on dead rows), then
//             dW_ih = dgates^T X and dW_hh = dgates^T h_prev on the split-K weight-gradient path (gemm_tn.hip, or gemm.hip's
//             split-K batches), db = column sums of dgates (fixed order), dX = dgates W_ih on gemm_w.hip (or gemm.hip) + lstm_mask_rows_kernel
//
// Both step kernels have the form of head.hip's tile products: a 32 x 32 output tile per workgroup, the contraction split
// over eight waves on the exact v_mfma_f32_32x32x2_f32, the waves' partial tiles summed through LDS in wave order, and
// the gate arithmetic in the epilogue.  Every row of a tile depends on its own sample alone (an MFMA row reads one row of A),
// so a NaN in one sample stays there, and rows past a sample's length are SELECTED to zero, never multiplied.  The tile
// product and the GEMM jobs around the recurrence are rnn_tile.h's, shared with gru.hip.
//
// `saved` (floats, regions aligned to 64): the activated gates [B][T][4H] (i, f, g, o), the cell state c [B][T][H] and
// h_prev [B][T][H] (h_prev[b][t] = out[b][t-1], zeros at t = 0: the B operand of dW_hh).  Rows past a length hold zeros.
#include "common.h"
#include "fused.h"
#include "rnn_tile.h"

namespace {

struct FwdStep {
  const float* Gx;                                   // [B T][4H]: X W_ih^T + b_ih
  const float* Whh; const float* bhh;
  const int* len;
  float* out;                                        // [B][T][H]
  float* gates;                                      // saved, or NULL
  float* cimg;                                       // [B][T][H]: saved, or the forward-only call's workspace
  float* hprev;                                      // saved, or NULL
  int B, T, H, t;
};

// grid (ceil(B / 32), H / 8): 32 samples x 8 hidden units; tile column j = gate (j >> 3) of unit u0 + (j & 7)
__global__ __launch_bounds__(kThreads) void lstm_fwd_step_kernel(const FwdStep p) {
  __shared__ float red[kWaves * 32 * kLdRed];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int b0 = blockIdx.x * 32, u0 = blockIdx.y * 8;
  const int B = p.B, T = p.T, H = p.H, t = p.t;
  const int br = b0 + r < B ? b0 + r : B - 1;       // (rows past the batch repeat the last sample: loaded, never stored)
  const bool any_live = __ballot(b0 + r < B && t < clamp_len(p.len[br], T)) != 0ull;   // the same answer in every wave
  const bool mm = any_live && t > 0;                 // step 0 has no recurrent product; a dead tile only writes its zeros
  if (mm) {
    const int nch = H / 8, lo = (w * nch) / kWaves, hi = ((w + 1) * nch) / kWaves;
    const float* a_row = p.out + ((long)br * T + (t - 1)) * H;               // h_{t-1}: the previous step's output row
    const float* b_row = p.Whh + ((long)(r >> 3) * H + u0 + (r & 7)) * H;
    const f32x16 acc = contract<true>(a_row, b_row, 0, lo, hi, h);
    store_partial(red + w * 32 * kLdRed, acc, r, h);
  }
  __syncthreads();
  if (tid >= 256) return;
  const int row = tid >> 3, u = u0 + (tid & 7), b = b0 + row;
  if (b >= B) return;
  const long bt = (long)b * T + t;
  const bool live = t < clamp_len(p.len[b], T);
  float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f, c = 0.f, hv = 0.f;
  if (live) {                                        // (a dead row's G_x may hold anything: it is not read)
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float rec = (mm ? sum_partials(red, row, 8 * g + (tid & 7)) : 0.f) + p.bhh[g * H + u];
      pre[g] = p.Gx[bt * 4 * H + g * H + u] + rec;
    }
    gi = sigmoid_f(pre[0]); gf = sigmoid_f(pre[1]); gg = tanhf(pre[2]); go = sigmoid_f(pre[3]);
    const float cp = t > 0 ? p.cimg[(bt - 1) * H + u] : 0.f;
    c = gf * cp + gi * gg;
    hv = go * tanhf(c);
  }
  p.out[bt * H + u] = hv;
  p.cimg[bt * H + u] = c;
  if (p.gates) {
    float* g = p.gates + bt * 4 * H + u;
    g[0] = gi; g[H] = gf; g[2 * H] = gg; g[3 * H] = go;
  }
  if (p.hprev) {
    if (t == 0) p.hprev[bt * H + u] = 0.f;
    if (t + 1 < T) p.hprev[(bt + 1) * H + u] = hv;
  }
}

struct BwdStep {
  const float* gout;                                 // [B][T][H]: the gradient at `out` (dead rows not read)
  const float* Whh;
  const int* len;
  const float* gates; const float* cimg;             // saved
  float* dgates;                                     // [B][T][4H]: pre-activation gate gradients, zeros on dead rows
  float* dc;                                         // [B][H]: the cell-state gradient carried to step t - 1
  int B, T, H, t;
};

// grid (ceil(B / 32), H / 32): dh_t = g_out[:, t] + dgates_{t+1} W_hh over 4H, then the gate gradients of step t
__global__ __launch_bounds__(kThreads) void lstm_bwd_step_kernel(const BwdStep p) {
  __shared__ float red[kWaves * 32 * kLdRed];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int b0 = blockIdx.x * 32, u0 = blockIdx.y * 32;
  const int B = p.B, T = p.T, H = p.H, t = p.t;
  const int br = b0 + r < B ? b0 + r : B - 1;
  const bool any_live = __ballot(b0 + r < B && t < clamp_len(p.len[br], T)) != 0ull;
  const bool mm = any_live && t + 1 < T;             // the last step has no successor
  if (mm) {
    const int nch = H / 2, lo = (w * nch) / kWaves, hi = ((w + 1) * nch) / kWaves;   // 4H / 8 chunks
    const float* a_row = p.dgates + ((long)br * T + (t + 1)) * 4 * H;
    const f32x16 acc = contract<false>(a_row, p.Whh + u0 + r, H, lo, hi, h);
    store_partial(red + w * 32 * kLdRed, acc, r, h);
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int row = (tid >> 5) + 16 * e, col = tid & 31, u = u0 + col, b = b0 + row;
    if (b >= B) continue;
    const long bt = (long)b * T + t;
    const bool live = t < clamp_len(p.len[b], T);
    float di = 0.f, df = 0.f, dg = 0.f, dout = 0.f, dcp = 0.f;
    if (live) {
      const float dh = p.gout[bt * H + u] + (mm ? sum_partials(red, row, col) : 0.f);
      const float* g = p.gates + bt * 4 * H + u;
      const float gi = g[0], gf = g[H], gg = g[2 * H], go = g[3 * H];
      const float c = p.cimg[bt * H + u], cp = t > 0 ? p.cimg[(bt - 1) * H + u] : 0.f;
      const float tc = tanhf(c);
      const float dct = (t + 1 < T ? p.dc[(long)b * H + u] : 0.f) + dh * go * (1.f - tc * tc);
      dout = dh * tc * (go * (1.f - go));
      di = dct * gg * (gi * (1.f - gi));
      df = dct * cp * (gf * (1.f - gf));
      dg = dct * gi * (1.f - gg * gg);
      dcp = dct * gf;
    }
    float* d = p.dgates + bt * 4 * H + u;
    d[0] = di; d[H] = df; d[2 * H] = dg; d[3 * H] = dout;
    p.dc[(long)b * H + u] = dcp;
  }
}

// y[b][t][:] = t < len_b ? x[b][t][:] (+ add[b][t][:]) : 0 over rows of W floats (W % 4 == 0); y may be x
__global__ __launch_bounds__(256) void lstm_mask_rows_kernel(const float* x, const float* __restrict__ add, float* y,
                                                             const int* __restrict__ len, long rows, int T, int W) {
  const int w4 = W / 4;
  const long n = rows * w4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long row = i / w4;
    f32x4 v = {};
    if ((int)(row % T) < clamp_len(len[row / T], T)) {
      v = reinterpret_cast<const f32x4*>(x)[i];
      if (add) v += reinterpret_cast<const f32x4*>(add)[i];
    }
    reinterpret_cast<f32x4*>(y)[i] = v;
  }
}

int launch_mask_rows4(const float* x, const float* add, float* y, const int* len, long rows, int T, int W, hipStream_t s) {
  const long n = rows * (W / 4);
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(lstm_mask_rows_kernel, dim3(blocks), dim3(256), 0, s, x, add, y, len, rows, T, W);
  CA_CHECK_LAUNCH("lstm mask rows");
  return 0;
}

// ---- plans ------------------------------------------------------------------------------------------------------------
bool shape_ok(int B, int T, int E, int H) {
  if (B < 1 || T < 1 || T > 64 || E < 32 || E > 2048 || H < 32 || H > 2048 || (E % 32) || (H % 32)) return false;
  // (the GEMM layer keeps 32-bit element offsets over [B T][4H] and [B T][E])
  return (long)B * T * 4 * (H > E ? H : E) < 2147483647L;
}

struct Saved { size_t gates, c, hprev, total; };
Saved saved_plan(int B, int T, int H) {
  Saved p;
  size_t o = 0;
  p.gates = o; o += al64((size_t)B * T * 4 * H);
  p.c = o;     o += al64((size_t)B * T * H);
  p.hprev = o; o += al64((size_t)B * T * H);
  p.total = o;
  return p;
}

struct FwdWs { size_t gx, c, wimg, bytes; };         // gx, c in floats; wimg, bytes in bytes
FwdWs fwd_plan(int B, int T, int E, int H) {
  FwdWs p;
  p.gx = 0;
  p.c = al64((size_t)B * T * 4 * H);
  p.wimg = (p.c + al64((size_t)B * T * H)) * sizeof(float);
  p.bytes = p.wimg + wsplit_bytes(4 * H, E);
  return p;
}

struct BwdWs { size_t dgates, dc, part, wimg, total; };    // floats
BwdWs bwd_plan(int B, int T, int E, int H) {
  BwdWs p;
  size_t o = 0;
  p.dgates = o; o += al64((size_t)B * T * 4 * H);
  p.dc = o;     o += al64((size_t)B * H);
  const size_t pi = (size_t)wgrad_parts(B * T, 4 * H, E) * 4 * H * E, ph = (size_t)wgrad_parts(B * T, 4 * H, H) * 4 * H * H;
  const size_t pb = (size_t)256 * 4 * H;            // grad_colsum: at most 256 chunks of rows
  size_t part = pi > ph ? pi : ph;
  part = part > pb ? part : pb;
  p.part = o; o += al64(part);
  p.wimg = o; o += al64(wsplit_bytes(E, 4 * H) / sizeof(float) + 1);
  p.total = o;
  return p;
}

int check_call(const char* what, int B, int T, int E, int H, int dtype, int flags) {
  CA_CHECK_ARG(dtype == COATTN_F32, "%s: unsupported dtype %d (only COATTN_F32)", what, dtype);
  CA_CHECK_ARG(B > 0 && T > 0 && E > 0 && H > 0, "%s: non-positive size B=%d T=%d E=%d H=%d", what, B, T, E, H);
  CA_CHECK_ARG(flags == 0, "%s: flags %d not supported: the recurrence is built in exact fp32 only (no COATTN_FLAG_FAST16, "
               "COATTN_FLAG_BF16_PROJ or other precision flag)", what, flags);
  CA_CHECK_ARG(shape_ok(B, T, E, H), "%s: shape B=%d T=%d E=%d H=%d not supported (T <= 64; E, H multiples of 32 up to 2048; "
               "B T 4 max(E, H) < 2^31: coattn_lstm_supported)", what, B, T, E, H);
  return 0;
}

}  // namespace

extern "C" int coattn_lstm_supported(int B, int T, int E, int H, int dtype) {
  return dtype == COATTN_F32 && shape_ok(B, T, E, H) ? 1 : 0;
}

extern "C" int coattn_lstm_workspace_bytes(int B, int T, int E, int H, int dtype, size_t* saved, size_t* ws_fwd, size_t* ws_bwd) {
  CA_TRY(check_call("lstm_workspace_bytes", B, T, E, H, dtype, 0));
  if (saved) *saved = saved_plan(B, T, H).total * sizeof(float);
  if (ws_fwd) *ws_fwd = fwd_plan(B, T, E, H).bytes;
  if (ws_bwd) *ws_bwd = bwd_plan(B, T, E, H).total * sizeof(float);
  return 0;
}

extern "C" int coattn_lstm_forward(const void* X, const int32_t* len, const coattn_lstm_params* p, void* out, void* x_masked,
                                   void* saved, void* ws, int B, int T, int E, int H, int dtype, int flags, void* stream) {
  CA_TRY(check_call("lstm_forward", B, T, E, H, dtype, flags));
  CA_CHECK_ARG(X && len && p && out && ws, "lstm_forward: null X, len, params, out or ws");
  CA_CHECK_ARG(p->w_ih && p->w_hh && p->b_ih && p->b_hh, "lstm_forward: null parameter");
  CA_CHECK_ARG(al16(X) && al16(out) && al16(x_masked) && al16(saved) && al16(ws) && al16(p->w_ih) && al16(p->w_hh) && al16(p->b_ih) &&
               al16(p->b_hh) && (((uintptr_t)len) & 3) == 0, "lstm_forward: every buffer must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const Saved sp = saved_plan(B, T, H);
  const FwdWs wp = fwd_plan(B, T, E, H);
  float* w = (float*)ws;
  float* sv = (float*)saved;
  float* Gx = w + wp.gx;
  void* wimg = (char*)ws + wp.wimg;
  // 1. G_x = X W_ih^T + b_ih: the exact pre-split-weight projection (coattn_linear_forward's kernels), gemm.hip otherwise
  CA_TRY(project((const float*)X, (const float*)p->w_ih, (const float*)p->b_ih, Gx, wimg, B, T, E, H, 4, s));
  prof_mark(s, "lstm_projection");
  // 2. x_masked: the phrase level as pad_packed_sequence returns it
  if (x_masked) CA_TRY(launch_mask_rows4((const float*)X, nullptr, (float*)x_masked, len, (long)B * T, T, E, s));
  // 3. the recurrence: one launch per step, chained on the stream
  FwdStep f = {};
  f.Gx = Gx; f.Whh = (const float*)p->w_hh; f.bhh = (const float*)p->b_hh; f.len = len; f.out = (float*)out;
  f.gates = sv ? sv + sp.gates : nullptr; f.cimg = sv ? sv + sp.c : w + wp.c; f.hprev = sv ? sv + sp.hprev : nullptr;
  f.B = B; f.T = T; f.H = H;
  const dim3 grid((B + 31) / 32, H / 8);
  for (int t = 0; t < T; ++t) {
    f.t = t;
    hipLaunchKernelGGL(lstm_fwd_step_kernel, grid, dim3(kThreads), 0, s, f);
  }
  CA_CHECK_LAUNCH("lstm_forward");
  prof_mark(s, "lstm_fwd_steps");
  return 0;
}

extern "C" int coattn_lstm_backward(const void* X, const int32_t* len, const coattn_lstm_params* p, const void* out,
                                    const void* saved, const void* g_out, const void* g_xmasked, void* dX,
                                    const coattn_lstm_param_grads* pg, int accumulate, void* ws, int B, int T, int E, int H,
                                    int dtype, int flags, void* stream) {
  CA_TRY(check_call("lstm_backward", B, T, E, H, dtype, flags));
  CA_CHECK_ARG(X && len && p && saved && g_out && pg && ws, "lstm_backward: null X, len, params, saved, g_out, grads or ws");
  CA_CHECK_ARG(p->w_ih && p->w_hh && p->b_ih && p->b_hh, "lstm_backward: null parameter");
  CA_CHECK_ARG(pg->w_ih && pg->w_hh && pg->b_ih && pg->b_hh, "lstm_backward: null parameter gradient");
  CA_CHECK_ARG(al16(X) && al16(out) && al16(saved) && al16(g_out) && al16(g_xmasked) && al16(dX) && al16(ws) && al16(p->w_ih) &&
               al16(p->w_hh) && al16(pg->w_ih) && al16(pg->w_hh) && al16(pg->b_ih) && al16(pg->b_hh) && (((uintptr_t)len) & 3) == 0,
               "lstm_backward: every buffer must be 16-byte aligned");
  (void)out;                                         // reserved, may be NULL: h_{t-1} of every row is kept in saved (h_prev)
  hipStream_t s = (hipStream_t)stream;
  const Saved sp = saved_plan(B, T, H);
  const BwdWs bp = bwd_plan(B, T, E, H);
  const float* sv = (const float*)saved;
  float* w = (float*)ws;
  float* dgates = w + bp.dgates;
  float* part = w + bp.part;
  const int acc = accumulate & 1, R = B * T;
  // 1. the recurrence in reverse
  BwdStep b = {};
  b.gout = (const float*)g_out; b.Whh = (const float*)p->w_hh; b.len = len; b.gates = sv + sp.gates; b.cimg = sv + sp.c;
  b.dgates = dgates; b.dc = w + bp.dc; b.B = B; b.T = T; b.H = H;
  const dim3 grid((B + 31) / 32, H / 32);
  for (int t = T - 1; t >= 0; --t) {
    b.t = t;
    hipLaunchKernelGGL(lstm_bwd_step_kernel, grid, dim3(kThreads), 0, s, b);
  }
  CA_CHECK_LAUNCH("lstm_backward");
  prof_mark(s, "lstm_bwd_steps");
  // 2. parameter gradients: dead rows of dgates are zeros, so they add nothing (dW_ih reads the raw X: 0 * x = 0 for every
  //    pad value whose bf16 pieces are finite, |x| <= 3.38e38 -- the header's range)
  CA_TRY(wgrad(dgates, (const float*)X, part, (float*)pg->w_ih, R, 4 * H, E, acc, s));
  CA_TRY(wgrad(dgates, sv + sp.hprev, part, (float*)pg->w_hh, R, 4 * H, H, acc, s));
  CA_TRY(grad_colsum(nullptr, dgates, R, 4 * H, part, (float*)pg->b_ih, acc, s));
  CA_TRY(grad_colsum(nullptr, dgates, R, 4 * H, part, (float*)pg->b_hh, acc, s));
  prof_mark(s, "lstm_param_grads");
  // 3. dX = dgates W_ih, plus the gradient that arrived at x_masked on live rows, exact zeros on dead rows
  if (dX) {
    CA_TRY(dx_product(dgates, (const float*)p->w_ih, (float*)dX, w + bp.wimg, B, T, E, H, 4, s));
    CA_TRY(launch_mask_rows4((const float*)dX, (const float*)g_xmasked, (float*)dX, len, (long)R, T, E, s));
    prof_mark(s, "lstm_dx");
  }
  return 0;
}
