// Question GRU of the baseline model (reference model.py QuestionBaselineEncoder: pack_padded_sequence -> nn.GRU -> the hidden
// state after each question's last token), restated without packing: one layer, one direction, gate order r, z, n, zero
// initial state, per-sample lengths read on the device.  include/coattn_rnn.h holds the contract; DESIGN 3.20 the layout and
// the measurements.
//
//   forward   G_x = X W_ih^T + b_ih for all B T rows at once (gemm_w.hip, or gemm.hip for the shapes it refuses: E = 300), then
//             one launch of gru_fwd_step_kernel per time step; the step len_b - 1 writes h_last[b]
//   backward  one launch of gru_bwd_step_kernel per time step in reverse, then dW_ih = dGx^T X and dW_hh = dGh^T h_prev on the
//             split-K weight-gradient path, db_ih / db_hh = the column sums of dGx / dGh (fixed order), dX = dGx W_ih
//
// The step kernels are lstm.hip's tile products (rnn_tile.h).  What differs from the LSTM:
//   * n = tanh(Gx_n + r * hn) multiplies the hidden-side product by r BEFORE the tanh, so the pre-activation gradient of n
//     reaches the input side as dnp and the hidden side as dnp * r: two gradient arrays, dGx (dW_ih, db_ih, dX) and dGh
//     (dW_hh, db_hh, the recurrent product);
//   * dh has a direct carry dh * z (dhc [B][H]) beside the matrix product;
//   * three gates fill 24 of the forward tile's 32 columns; columns 24 .. 31 load a clamped row of W_hh and are never read.
// Every row of a tile depends on its own sample alone, so a NaN in one sample stays there, and rows past a sample's length are
// SELECTED to zero, never multiplied.
//
// `saved` (floats, regions aligned to 64): the activated gates [B][T][3H] (r, z, n), hn [B][T][H] (h_{t-1} W_hn^T + b_hn) and
// h_prev [B][T][H] (h_prev[b][t] = seq_out[b][t-1], zeros at t = 0: the B operand of dW_hh).  Rows past a length hold zeros.
#include "common.h"
#include "fused.h"
#include "rnn_tile.h"
#include "../../include/coattn_rnn.h"

namespace {

struct FwdStep {
  const float* Gx;                                   // [B T][3H]: X W_ih^T + b_ih
  const float* Whh; const float* bhh;
  const int* len;
  float* out;                                        // seq_out [B][T][H]
  float* hlast;                                      // [B][H], or NULL
  float* gates; float* hn; float* hprev;             // saved, or all NULL
  int B, T, H, t;
};

// grid (ceil(B / 32), H / 8): 32 samples x 8 hidden units; tile column j < 24 = gate (j >> 3) of unit u0 + (j & 7)
__global__ __launch_bounds__(kThreads) void gru_fwd_step_kernel(const FwdStep p) {
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
    const int gate = (r >> 3) < 3 ? (r >> 3) : 2;    // (columns 24 .. 31 repeat gate n's rows, inside [3H][H]: loaded, never read)
    const float* b_row = p.Whh + ((long)gate * H + u0 + (r & 7)) * H;
    const f32x16 acc = contract<true>(a_row, b_row, 0, lo, hi, h);
    store_partial(red + w * 32 * kLdRed, acc, r, h);
  }
  __syncthreads();
  if (tid >= 256) return;
  const int row = tid >> 3, c = tid & 7, u = u0 + c, b = b0 + row;
  if (b >= B) return;
  const long bt = (long)b * T + t;
  const int len = clamp_len(p.len[b], T);
  const bool live = t < len;
  float gr = 0.f, gz = 0.f, gn = 0.f, hn = 0.f, hp = 0.f, hv = 0.f;
  if (live) {                                        // (a dead row's G_x may hold anything: it is not read)
    const float hr = (mm ? sum_partials(red, row, c) : 0.f) + p.bhh[u];
    const float hz = (mm ? sum_partials(red, row, 8 + c) : 0.f) + p.bhh[H + u];
    hn = (mm ? sum_partials(red, row, 16 + c) : 0.f) + p.bhh[2 * H + u];
    const float* gx = p.Gx + bt * 3 * H + u;
    gr = sigmoid_f(gx[0] + hr);
    gz = sigmoid_f(gx[H] + hz);
    gn = tanhf(gx[2 * H] + gr * hn);
    hp = t > 0 ? p.out[(bt - 1) * H + u] : 0.f;
    hv = gn + gz * (hp - gn);
    if (p.hlast && t == len - 1) p.hlast[(long)b * H + u] = hv;
  }
  p.out[bt * H + u] = hv;
  if (p.gates) {
    float* g = p.gates + bt * 3 * H + u;
    g[0] = gr; g[H] = gz; g[2 * H] = gn;
    p.hn[bt * H + u] = hn;
    p.hprev[bt * H + u] = hp;
  }
}

struct BwdStep {
  const float* gseq;                                 // [B][T][H] or NULL: the gradient at seq_out (dead rows not read)
  const float* glast;                                // [B][H] or NULL: the gradient at h_last
  const float* Whh;
  const int* len;
  const float* gates; const float* hn; const float* hprev;   // saved
  float* dGx; float* dGh;                            // [B][T][3H] each: the gate gradients of the input and the hidden side
  float* dhc;                                        // [B][H]: the direct carry dh * z to step t - 1
  int B, T, H, t;
};

// grid (ceil(B / 32), H / 32): dh_t = g_seq[:, t] + g_last (at len - 1) + dhc + dGh_{t+1} W_hh over 3H, then the gate gradients
__global__ __launch_bounds__(kThreads) void gru_bwd_step_kernel(const BwdStep p) {
  __shared__ float red[kWaves * 32 * kLdRed];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int b0 = blockIdx.x * 32, u0 = blockIdx.y * 32;
  const int B = p.B, T = p.T, H = p.H, t = p.t;
  const int br = b0 + r < B ? b0 + r : B - 1;
  const bool any_live = __ballot(b0 + r < B && t < clamp_len(p.len[br], T)) != 0ull;
  const bool mm = any_live && t + 1 < T;             // the last step has no successor
  if (mm) {
    const int nch = 3 * H / 8, lo = (w * nch) / kWaves, hi = ((w + 1) * nch) / kWaves;
    const float* a_row = p.dGh + ((long)br * T + (t + 1)) * 3 * H;
    const f32x16 acc = contract<false>(a_row, p.Whh + u0 + r, H, lo, hi, h);
    store_partial(red + w * 32 * kLdRed, acc, r, h);
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int row = (tid >> 5) + 16 * e, col = tid & 31, u = u0 + col, b = b0 + row;
    if (b >= B) continue;
    const long bt = (long)b * T + t;
    const int len = clamp_len(p.len[b], T);
    float drp = 0.f, dzp = 0.f, dnp = 0.f, dnr = 0.f, carry = 0.f;
    if (t < len) {
      float dh = p.gseq ? p.gseq[bt * H + u] : 0.f;
      if (p.glast && t == len - 1) dh += p.glast[(long)b * H + u];
      if (t + 1 < T) dh += p.dhc[(long)b * H + u] + (mm ? sum_partials(red, row, col) : 0.f);
      const float* g = p.gates + bt * 3 * H + u;
      const float gr = g[0], gz = g[H], gn = g[2 * H];
      const float hn = p.hn[bt * H + u], hp = p.hprev[bt * H + u];
      dnp = dh * (1.f - gz) * (1.f - gn * gn);
      dzp = dh * (hp - gn) * gz * (1.f - gz);
      drp = dnp * hn * gr * (1.f - gr);
      dnr = dnp * gr;
      carry = dh * gz;
    }
    float* dx = p.dGx + bt * 3 * H + u;
    float* dg = p.dGh + bt * 3 * H + u;
    dx[0] = drp; dx[H] = dzp; dx[2 * H] = dnp;
    dg[0] = drp; dg[H] = dzp; dg[2 * H] = dnr;
    p.dhc[(long)b * H + u] = carry;
  }
}

// ---- plans ------------------------------------------------------------------------------------------------------------
bool shape_ok(int B, int T, int E, int H) {
  if (B < 1 || T < 1 || T > 64 || E < 4 || E > 2048 || H < 32 || H > 2048 || (E % 4) || (H % 32)) return false;
  // (the GEMM layer keeps 32-bit element offsets over [B T][3H] and [B T][E])
  return (long)B * T * 3 * (H > E ? H : E) < 2147483647L;
}

struct Saved { size_t gates, hn, hprev, total; };
Saved saved_plan(int B, int T, int H) {
  Saved p;
  size_t o = 0;
  p.gates = o; o += al64((size_t)B * T * 3 * H);
  p.hn = o;    o += al64((size_t)B * T * H);
  p.hprev = o; o += al64((size_t)B * T * H);
  p.total = o;
  return p;
}

struct FwdWs { size_t gx, wimg, bytes; };            // gx in floats; wimg, bytes in bytes
FwdWs fwd_plan(int B, int T, int E, int H) {
  FwdWs p;
  p.gx = 0;
  p.wimg = al64((size_t)B * T * 3 * H) * sizeof(float);
  p.bytes = p.wimg + wsplit_bytes(3 * H, E);
  return p;
}

struct BwdWs { size_t dgx, dgh, dhc, part, wimg, total; };    // floats
BwdWs bwd_plan(int B, int T, int E, int H) {
  BwdWs p;
  size_t o = 0;
  p.dgx = o; o += al64((size_t)B * T * 3 * H);
  p.dgh = o; o += al64((size_t)B * T * 3 * H);
  p.dhc = o; o += al64((size_t)B * H);
  const size_t pi = (size_t)wgrad_parts(B * T, 3 * H, E) * 3 * H * E, ph = (size_t)wgrad_parts(B * T, 3 * H, H) * 3 * H * H;
  const size_t pb = (size_t)256 * 3 * H;            // grad_colsum: at most 256 chunks of rows
  size_t part = pi > ph ? pi : ph;
  part = part > pb ? part : pb;
  p.part = o; o += al64(part);
  p.wimg = o; o += al64(wsplit_bytes(E, 3 * H) / sizeof(float) + 1);
  p.total = o;
  return p;
}

int check_call(const char* what, int B, int T, int E, int H, int dtype, int flags) {
  CA_CHECK_ARG(dtype == COATTN_F32, "%s: unsupported dtype %d (only COATTN_F32)", what, dtype);
  CA_CHECK_ARG(B > 0 && T > 0 && E > 0 && H > 0, "%s: non-positive size B=%d T=%d E=%d H=%d", what, B, T, E, H);
  CA_CHECK_ARG(flags == 0, "%s: flags %d not supported: the recurrence is built in exact fp32 only (no COATTN_FLAG_FAST16, "
               "COATTN_FLAG_BF16_PROJ or other precision flag)", what, flags);
  CA_CHECK_ARG(shape_ok(B, T, E, H), "%s: shape B=%d T=%d E=%d H=%d not supported (T <= 64; E a multiple of 4 up to 2048; H a "
               "multiple of 32 up to 2048; B T 3 max(E, H) < 2^31: coattn_gru_supported)", what, B, T, E, H);
  return 0;
}

}  // namespace

extern "C" int coattn_gru_supported(int B, int T, int E, int H, int dtype) {
  return dtype == COATTN_F32 && shape_ok(B, T, E, H) ? 1 : 0;
}

extern "C" int coattn_gru_workspace_bytes(int B, int T, int E, int H, int dtype, size_t* saved, size_t* ws_fwd, size_t* ws_bwd) {
  CA_TRY(check_call("gru_workspace_bytes", B, T, E, H, dtype, 0));
  if (saved) *saved = saved_plan(B, T, H).total * sizeof(float);
  if (ws_fwd) *ws_fwd = fwd_plan(B, T, E, H).bytes;
  if (ws_bwd) *ws_bwd = bwd_plan(B, T, E, H).total * sizeof(float);
  return 0;
}

extern "C" int coattn_gru_forward(const void* X, const int32_t* len, const coattn_gru_params* p, void* seq_out, void* h_last,
                                  void* saved, void* ws, int B, int T, int E, int H, int dtype, int flags, void* stream) {
  CA_TRY(check_call("gru_forward", B, T, E, H, dtype, flags));
  CA_CHECK_ARG(X && len && p && seq_out && ws, "gru_forward: null X, len, params, seq_out or ws");
  CA_CHECK_ARG(p->w_ih && p->w_hh && p->b_ih && p->b_hh, "gru_forward: null parameter");
  CA_CHECK_ARG(al16(X) && al16(seq_out) && al16(h_last) && al16(saved) && al16(ws) && al16(p->w_ih) && al16(p->w_hh) && al16(p->b_ih) &&
               al16(p->b_hh) && (((uintptr_t)len) & 3) == 0, "gru_forward: every buffer must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const Saved sp = saved_plan(B, T, H);
  const FwdWs wp = fwd_plan(B, T, E, H);
  float* sv = (float*)saved;
  float* Gx = (float*)ws + wp.gx;
  // 1. G_x = X W_ih^T + b_ih: the exact pre-split-weight projection, gemm.hip otherwise
  CA_TRY(project((const float*)X, (const float*)p->w_ih, (const float*)p->b_ih, Gx, (char*)ws + wp.wimg, B, T, E, H, 3, s));
  prof_mark(s, "gru_projection");
  // 2. the recurrence: one launch per step, chained on the stream
  FwdStep f = {};
  f.Gx = Gx; f.Whh = (const float*)p->w_hh; f.bhh = (const float*)p->b_hh; f.len = len; f.out = (float*)seq_out;
  f.hlast = (float*)h_last;
  f.gates = sv ? sv + sp.gates : nullptr; f.hn = sv ? sv + sp.hn : nullptr; f.hprev = sv ? sv + sp.hprev : nullptr;
  f.B = B; f.T = T; f.H = H;
  const dim3 grid((B + 31) / 32, H / 8);
  for (int t = 0; t < T; ++t) {
    f.t = t;
    hipLaunchKernelGGL(gru_fwd_step_kernel, grid, dim3(kThreads), 0, s, f);
  }
  CA_CHECK_LAUNCH("gru_forward");
  prof_mark(s, "gru_fwd_steps");
  return 0;
}

extern "C" int coattn_gru_backward(const void* X, const int32_t* len, const coattn_gru_params* p, const void* saved,
                                   const void* g_seq, const void* g_last, void* dX, const coattn_gru_param_grads* pg,
                                   int accumulate, void* ws, int B, int T, int E, int H, int dtype, int flags, void* stream) {
  CA_TRY(check_call("gru_backward", B, T, E, H, dtype, flags));
  CA_CHECK_ARG(X && len && p && saved && pg && ws, "gru_backward: null X, len, params, saved, grads or ws");
  CA_CHECK_ARG(g_seq || g_last, "gru_backward: g_seq and g_last are both null: no gradient to propagate");
  CA_CHECK_ARG(p->w_ih && p->w_hh && p->b_ih && p->b_hh, "gru_backward: null parameter");
  CA_CHECK_ARG(pg->w_ih && pg->w_hh && pg->b_ih && pg->b_hh, "gru_backward: null parameter gradient");
  CA_CHECK_ARG(al16(X) && al16(saved) && al16(g_seq) && al16(g_last) && al16(dX) && al16(ws) && al16(p->w_ih) && al16(p->w_hh) &&
               al16(pg->w_ih) && al16(pg->w_hh) && al16(pg->b_ih) && al16(pg->b_hh) && (((uintptr_t)len) & 3) == 0,
               "gru_backward: every buffer must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const Saved sp = saved_plan(B, T, H);
  const BwdWs bp = bwd_plan(B, T, E, H);
  const float* sv = (const float*)saved;
  float* w = (float*)ws;
  float* dGx = w + bp.dgx;
  float* dGh = w + bp.dgh;
  float* part = w + bp.part;
  const int acc = accumulate & 1, R = B * T;
  // 1. the recurrence in reverse
  BwdStep b = {};
  b.gseq = (const float*)g_seq; b.glast = (const float*)g_last; b.Whh = (const float*)p->w_hh; b.len = len;
  b.gates = sv + sp.gates; b.hn = sv + sp.hn; b.hprev = sv + sp.hprev;
  b.dGx = dGx; b.dGh = dGh; b.dhc = w + bp.dhc; b.B = B; b.T = T; b.H = H;
  const dim3 grid((B + 31) / 32, H / 32);
  for (int t = T - 1; t >= 0; --t) {
    b.t = t;
    hipLaunchKernelGGL(gru_bwd_step_kernel, grid, dim3(kThreads), 0, s, b);
  }
  CA_CHECK_LAUNCH("gru_backward");
  prof_mark(s, "gru_bwd_steps");
  // 2. parameter gradients: dead rows of dGx and dGh are zeros, so they add nothing (dW_ih reads the raw X: 0 * x = 0 for
  //    every pad value whose bf16 pieces are finite -- the header's range)
  CA_TRY(wgrad(dGx, (const float*)X, part, (float*)pg->w_ih, R, 3 * H, E, acc, s));
  CA_TRY(wgrad(dGh, sv + sp.hprev, part, (float*)pg->w_hh, R, 3 * H, H, acc, s));
  CA_TRY(grad_colsum(nullptr, dGx, R, 3 * H, part, (float*)pg->b_ih, acc, s));
  CA_TRY(grad_colsum(nullptr, dGh, R, 3 * H, part, (float*)pg->b_hh, acc, s));
  prof_mark(s, "gru_param_grads");
  // 3. dX = dGx W_ih: the zero rows of dGx give exact zeros (sums of +-0 from a +0 accumulator)
  if (dX) {
    CA_TRY(dx_product(dGx, (const float*)p->w_ih, (float*)dX, w + bp.wimg, B, T, E, H, 3, s));
    prof_mark(s, "gru_dx");
  }
  return 0;
}
