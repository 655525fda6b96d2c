// C-ABI of the co-attention path (include/coattn.h): argument checking, workspace planning
// and kernel orchestration.  No torch types, no allocation, no synchronisation: every call
// only enqueues kernels on the caller's stream.
#include "common.h"
#include "fused.h"
#include "../../include/coattn_rnn.h"
#include "../../include/coattn_fusion.h"

#include <string.h>

// ---------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void coattn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" int coattn_version(void) { return 2600; }   // 0.26.0: the fusion head of the baseline model, row norm + two embeddings + product + Linear -> Philox dropout -> tanh + classifier, forward and backward (coattn_fusion_supported, coattn_fusion_workspace_bytes, coattn_fusion_forward, coattn_fusion_backward: fusion.hip; declared in include/coattn_fusion.h); 0.25.0: the question GRU of the baseline model, length-aware forward and backward (coattn_gru_supported, coattn_gru_workspace_bytes, coattn_gru_forward, coattn_gru_backward: gru.hip; declared in include/coattn_rnn.h); 0.24.0: the frozen encoder in eval mode, BatchNorm on running statistics + convolution bias + ReLU + pool in one launch, the first group from the image (coattn_bn_eval_supported, coattn_bn_eval_forward, coattn_conv1_bn_eval_supported, coattn_conv1_bn_eval_forward, the developer probe coattn_bn_eval_probe: encoder.hip); 0.23.0: image preprocessing, Pillow's 8-bit bilinear resize and the ToTensor + Normalize lookup for a batch of decoded images in one launch (coattn_preprocess_supported, coattn_preprocess_images: preprocess.hip; declared in include/coattn_ext.h, as every entry point after 0.22.0); 0.22.0: layer 1 of the frozen encoder with the convolution computed twice and never stored (coattn_conv1_bn_recompute_workspace_bytes, coattn_conv1_bn_recompute_forward: encoder.hip); 0.21.0: attention overlays (coattn_overlay_render: overlay.hip); 0.20.0: cached image features, the rows of a batch gathered from an fp32 or bf16 feature table in one launch (coattn_features_gather_supported, coattn_features_gather: features.hip); 0.19.0: feature dropout, a Philox4x32-10 mask regenerated in the backward from a device-side step counter (coattn_dropout_supported, coattn_dropout_forward, coattn_dropout_backward: dropout.hip); 0.18.0: the word embedding, gather and ordered dense gradient (coattn_embedding_supported, coattn_embedding_workspace_bytes, coattn_embedding_forward, coattn_embedding_backward: embedding.hip); 0.17.0: the sentence LSTM, length-aware forward and backward (coattn_lstm_supported, coattn_lstm_workspace_bytes, coattn_lstm_forward, coattn_lstm_backward: lstm.hip); 0.16.0: layer 1 of the frozen encoder, convolution and BatchNorm statistics in one pass with the stock kernels' bits (coattn_conv1_bn_exact_supported, coattn_conv1_bn_exact_workspace_bytes, coattn_conv1_bn_exact_forward, coattn_conv1_probe: encoder.hip); 0.15.0: the stock BatchNorm kernels' bits in two passes (coattn_bn_exact_geometry, coattn_bn_exact_workspace_bytes, coattn_bn_exact_forward: encoder.hip); 0.14.0: the frozen encoder's train-mode BatchNorm + ReLU + 2x2 max-pool (coattn_bn_supported, coattn_bn_workspace_bytes, coattn_bn_relu_pool_forward: encoder.hip); 0.13.0: the optimiser step (coattn_adam_workspace_bytes, coattn_adam_step: adam.hip); 0.12.0: soft answer targets (coattn_soft_loss_forward, coattn_vqa_score, coattn_head_forward_soft); 0.11.0: alternating co-attention (coattn_alt_workspace_bytes / _forward / _backward); 0.10.0: COATTN_FLAG_BILINEAR (the affinity tanh(Q W_b^T + b_b) V^T; W_b / b_b, dW_b / db_b appended to the parameter structs); 0.9.0: coattn_forward_maps(_len) / coattn_backward_maps(_len) (differentiable attention maps); 0.8.0: the length-masked forms coattn_forward_len / _infer_len / _attention_forward_len / _backward_len; 0.7.0: coattn_infer (forward only, attention maps to caller buffers); 0.6.1: coattn_status_accumulate / coattn_phrase_status_accumulate (sticky range report in a caller-owned accumulator); 0.6.0: flags = 0 is the exact mode, COATTN_FLAG_FAST16 the tolerance mode, coattn_status / coattn_phrase_status; 0.5.2: forward-side contractions on two FP16 pieces (COATTN_FLAG_F16PAIR); 0.5.1: coattn_features_native; 0.5.0: widths of the fp32 mode (COATTN_FLAG_EXACT3 / _SPLIT2), coattn_profile_*

// ---------------------------------------------------------------------------------------
// per-kernel timing (bench.py's backward roofline legs): HIP events recorded between the launches of the calls made
// on this thread between coattn_profile_begin and coattn_profile_end
// ---------------------------------------------------------------------------------------
namespace {
constexpr int kProfMax = 48;
struct Prof {
  bool on = false;
  int n = 0, created = 0;
  hipEvent_t ev[kProfMax + 1];
  const char* name[kProfMax];
};
thread_local Prof g_prof;
}  // namespace

void prof_mark(hipStream_t s, const char* name) {
  Prof& p = g_prof;
  if (!p.on || p.n >= kProfMax) return;
  if (hipEventRecord(p.ev[p.n + 1], s) != hipSuccess) { p.on = false; return; }
  p.name[p.n++] = name;
}

extern "C" int coattn_profile_begin(void* stream) {
  Prof& p = g_prof;
  while (p.created <= kProfMax) {
    if (hipEventCreate(&p.ev[p.created]) != hipSuccess) { coattn_set_error("profile: hipEventCreate failed"); return -3; }
    ++p.created;
  }
  p.n = 0;
  if (hipEventRecord(p.ev[0], (hipStream_t)stream) != hipSuccess) { coattn_set_error("profile: hipEventRecord failed"); return -3; }
  p.on = true;
  return 0;
}

extern "C" int coattn_profile_end(float* us, char* names, int names_bytes, int max_marks) {
  Prof& p = g_prof;
  CA_CHECK_ARG(p.on || p.n > 0, "profile: no coattn_profile_begin on this thread (or an event could not be recorded)");
  p.on = false;
  CA_CHECK_ARG(us && max_marks >= p.n, "profile: room for %d marks needed", p.n);
  if (p.n == 0) return 0;
  if (hipEventSynchronize(p.ev[p.n]) != hipSuccess) { coattn_set_error("profile: hipEventSynchronize failed"); return -3; }
  int o = 0;
  if (names && names_bytes > 0) names[0] = 0;
  for (int i = 0; i < p.n; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]) != hipSuccess) { coattn_set_error("profile: hipEventElapsedTime failed"); return -3; }
    us[i] = ms * 1000.f;
    if (names && o < names_bytes - 1) o += snprintf(names + o, (size_t)(names_bytes - o), "%s%s", i ? "\n" : "", p.name[i]);
  }
  const int n = p.n;
  p.n = 0;
  return n;
}
extern "C" const char* coattn_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------------------
// buffer plans (in floats, every region aligned to 64 floats = 256 B: common.h al64)
// ---------------------------------------------------------------------------------------
static const int kMaxSplits = 32;

struct BwdPlan {
  size_t Hv, dPv, dZq, dPq, dC, dav, dsv, daq, dsq, part, total;
};
static BwdPlan plan_bwd(int B, int N, int T, int d, int L) {
  BwdPlan p;
  size_t o = 0;
  p.Hv = o;  o += al64((size_t)B * N * d);
  p.dPv = o; o += al64((size_t)B * N * d);
  p.dZq = o; o += al64((size_t)B * T * d);
  p.dPq = o; o += al64((size_t)L * B * T * d);
  p.dC = o;  o += al64((size_t)L * B * T * N);
  p.dav = o; o += al64((size_t)L * B * N);
  p.dsv = o; o += al64((size_t)L * B * N);
  p.daq = o; o += al64((size_t)L * B * T);
  p.dsq = o; o += al64((size_t)L * B * T);
  size_t part = (size_t)kMaxSplits * d * d;
  size_t cs = (size_t)260 * d;
  p.part = o; o += al64(part > cs ? part : cs);
  p.total = o;
  return p;
}

// COATTN_FLAG_BILINEAR: behind the common layout of `saved` (at saved_off(..).total) lie K = Q W_b^T + b_b of all levels
// [L][B][T][d] and the range words of W_b's FP16 image (tolerance mode); behind the backward's workspace its BilBwd buffers
static bool bilinear(int flags) { return (flags & COATTN_FLAG_BILINEAR) != 0; }
static size_t wchunks(int d) { return (size_t)((d + 31) / 32) * ((d + 15) / 16); }
static size_t bil_floats(int B, int T, int d, int L, bool bil) {
  return bil ? al64((size_t)L * B * T * d) + al64(wchunks(d)) : 0;
}
static size_t saved_floats(int B, int N, int T, int d, int L, bool bil) {
  return saved_off(B, N, T, d, L).total + bil_floats(B, T, d, L, bil);
}
static size_t bil_bwd_floats(int B, int T, int d, int L) {
  const size_t k = al64((size_t)L * B * T * d);
  return 3 * k + al64((size_t)2 * d * d) + al64(wsplit_bytes(d, 2 * d) / sizeof(float) + 1) + al64((size_t)L * B * d);
}
static size_t fwd_ws_floats(int B, int N, int T, int d, int L, bool bil = false) {
  return saved_floats(B, N, T, d, L, bil) + al64((size_t)B * N * d);
}
static size_t bwd_ws_floats(int B, int N, int T, int d, int L, bool bil = false) {
  size_t bw = plan_bwd(B, N, T, d, L).total;
  if (fused_supported(B, N, T, d, L)) {
    const size_t fb = fused_bwd_ws_floats(B, N, T, d, L);
    if (fb > bw) bw = fb;
  }
  return bw + (bil ? bil_bwd_floats(B, T, d, L) : 0);
}

static int check_shape(int B, int N, int T, int d, int L, int dtype) {
  CA_CHECK_ARG(dtype == COATTN_F32, "unsupported dtype %d (only COATTN_F32)", dtype);
  CA_CHECK_ARG(B > 0 && B <= 65535, "bad batch size B=%d", B);
  CA_CHECK_ARG(N > 0 && N <= 4096 && T > 0 && T <= 4096, "bad N=%d / T=%d", N, T);
  CA_CHECK_ARG(d > 0 && d <= 8192, "bad hidden size d=%d", d);
  CA_CHECK_ARG(L > 0 && L <= 8, "bad number of levels L=%d", L);
  return 0;
}

extern "C" int coattn_fused_supported(int B, int N, int T, int d, int L, int dtype) {
  if (dtype != COATTN_F32) return 0;
  return fused_supported(B, N, T, d, L);
}

extern "C" int coattn_workspace_bytes(int B, int N, int T, int d, int L, int dtype, int flags, size_t* saved,
                                      size_t* ws_fwd, size_t* ws_bwd) {
  CA_TRY(check_shape(B, N, T, d, L, dtype));
  const bool bil = bilinear(flags);                   // (K in `saved`, dK in the backward's workspace)
  if (saved) *saved = saved_floats(B, N, T, d, L, bil) * sizeof(float);
  // the forward workspace ends with room for two pre-split weight images (gemm_w.hip)
  if (ws_fwd) *ws_fwd = fwd_ws_floats(B, N, T, d, L, bil) * sizeof(float) + (bil ? 3 : 2) * wsplit_bytes(d, d);   // (+ W_b's)
  if (ws_bwd) *ws_bwd = bwd_ws_floats(B, N, T, d, L, bil) * sizeof(float);
  return 0;
}

extern "C" int coattn_gemm_f32(const coattn_gemm_desc* g, void* stream) {
  CA_CHECK_ARG(g != nullptr, "gemm: null descriptor");
  return launch_gemm_f32(*g, (hipStream_t)stream);
}

extern "C" size_t coattn_linear_workspace_bytes(int N, int K) { return (N > 0 && K > 0) ? wsplit_bytes(N, K) : 0; }

extern "C" int coattn_linear_forward(const void* x, int64_t ld_x, const void* W, const void* bias, void* y, void* wimg,
                                     int M, int N, int K, float out_scale, int flags, void* stream) {
  CA_CHECK_ARG(x && W && y && wimg && M > 0 && N > 0 && K > 0 && ld_x >= K && ld_x < (1L << 24), "linear: bad argument");
  WGemm g = {};
  g.A = (const float*)x; g.a_sm = (int)ld_x; g.Wf = wimg; g.C = (float*)y; g.c_sm = N; g.bias_n = (const float*)bias;
  g.out_scale = out_scale; g.M = M; g.N = N; g.K = K; g.batch = 1;
  g.bf16 = (flags & COATTN_FLAG_BF16_PROJ) ? 1 : 0;
  g.np = (flags & COATTN_FLAG_SPLIT2) ? 2 : 3;
  if ((flags & COATTN_FLAG_F16PAIR) && !g.bf16) { g.np = 2; g.f16 = 1; }
  g.a_bf16 = (flags & COATTN_FLAG_BF16_IN) ? 1 : 0;
  CA_CHECK_ARG(!g.a_bf16 || g.bf16, "linear: COATTN_FLAG_BF16_IN needs COATTN_FLAG_BF16_PROJ");
  CA_CHECK_ARG(g.a_bf16 ? gemm_bf_supported(g) : gemm_w_supported(g), "linear: shape M=%d N=%d K=%d ld=%ld not supported (see coattn.h)", M, N, K, (long)ld_x);
  if (!(flags & 1)) {
    const WSplit job{(const float*)W, wimg, N, K, 0, K, wimg_pieces(g), nullptr};
    CA_TRY(launch_wsplit(&job, 1, (hipStream_t)stream));
  }
  return launch_gemm_wx(&g, 1, (hipStream_t)stream);
}

extern "C" size_t coattn_linear_wgrad_workspace_bytes(int n_out, int n_in) {
  return (n_out > 0 && n_in > 0) ? (size_t)32 * n_out * n_in * sizeof(float) : 0;
}

extern "C" int coattn_linear_weight_grad(const void* dy, int64_t ld_dy, const void* x, int64_t ld_x, void* dW, void* ws,
                                         int M, int n_out, int n_in, int accumulate, void* stream) {
  CA_CHECK_ARG(dy && x && dW && ws && M > 0 && n_out > 0 && n_in > 0 && ld_dy >= n_out && ld_x >= n_in &&
               ld_dy < (1L << 24) && ld_x < (1L << 24), "linear weight grad: bad argument");
  TnGemm g = {};
  g.A = (const float*)dy; g.a_ld = (int)ld_dy; g.B = (const float*)x; g.b_ld = (int)ld_x; g.C = (float*)ws;
  g.M = n_out; g.N = n_in; g.K = M; g.levels = 1;
  g.bf16 = (accumulate & COATTN_FLAG_BF16_PROJ) ? 1 : 0;
  g.np = (accumulate & COATTN_FLAG_SPLIT2) ? 2 : 3;
  g.a_bf16 = (accumulate & COATTN_FLAG_BF16_IN) ? 1 : 0;
  accumulate &= 1;
  CA_CHECK_ARG(!g.a_bf16 || g.bf16, "linear weight grad: COATTN_FLAG_BF16_IN needs COATTN_FLAG_BF16_PROJ");
  CA_CHECK_ARG(g.a_bf16 ? gemm_bf_tn_supported(g) : gemm_tn_supported(g), "linear weight grad: shape M=%d n_out=%d n_in=%d not supported (see coattn.h)", M, n_out, n_in);
  if (gemm_bf_tn_supported(g)) {                     // reduced-precision mode, wide shape: the single-product kernel (gemm_bf.hip)
    const int ntiles = (n_out / 256) * (n_in / 256);
    int want = (bf_tn_rounds() * 256 + ntiles - 1) / ntiles, spp, parts;
    want = want > 32 ? 32 : want;
    parts = gemm_bf_tn_plan(g, want, &spp);
    CA_TRY(launch_gemm_bf_tn(&g, &spp, &parts, 1, (hipStream_t)stream));
    return launch_reduce_partials((const float*)ws, (float*)dW, parts, (int64_t)n_out * n_in, accumulate, (hipStream_t)stream);
  }
  int ks, S;
  const int parts = gemm_tn_plan(g, 32, &ks, &S);
  CA_TRY(launch_gemm_tn(&g, &ks, &S, 1, (hipStream_t)stream));
  return launch_reduce_partials((const float*)ws, (float*)dW, parts, (int64_t)n_out * n_in, accumulate, (hipStream_t)stream);
}

extern "C" int coattn_gemm_bf16(const coattn_gemm_desc* g, void* stream) {
  CA_CHECK_ARG(g != nullptr, "gemm: null descriptor");
  return launch_gemm_bf16in(*g, (hipStream_t)stream);
}

// Range report of the tolerance mode (include/coattn.h): header + per-chunk weight maxima from the status words.
int read_status_words(const float* status, int n_words, hipStream_t s, float* amax, const char* what) {
  if (hipStreamSynchronize(s) != hipSuccess) { coattn_set_error("%s: hipStreamSynchronize failed", what); return -3; }
  float hdr[2] = {0.f, 0.f};
  if (hipMemcpy(hdr, status, sizeof(hdr), hipMemcpyDeviceToHost) != hipSuccess) { coattn_set_error("%s: reading the status words failed", what); return -3; }
  if (amax) amax[0] = amax[1] = 0.f;
  if (hdr[1] != 1.f) return 0;                       // the call converted nothing to FP16 pieces
  float wmax = 0.f;
  {
    const int n = n_words - kStatusHdr;
    float* w = (float*)malloc((size_t)n * sizeof(float));
    CA_CHECK_ARG(w != nullptr, "%s: out of host memory", what);
    const hipError_t e = hipMemcpy(w, status + kStatusHdr, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    for (int i = 0; e == hipSuccess && i < n; ++i) wmax = (w[i] > wmax || w[i] != w[i]) ? w[i] : wmax;
    free(w);
    if (e != hipSuccess) { coattn_set_error("%s: reading the status words failed", what); return -3; }
  }
  if (amax) { amax[0] = hdr[0]; amax[1] = wmax; }
  const bool act = !(hdr[0] <= kF16Exact), wgt = !(wmax <= kF16Exact);
  if (act || wgt) {
    coattn_set_error("%s: FP16-piece range exceeded in the last forward (COATTN_FLAG_FAST16): %s%s%s -- pieces were clamped; "
                     "re-run with flags = 0 (exact)", what,
                     act ? "an activation (feature or stored projection) of magnitude > 65504" : "", act && wgt ? " and " : "",
                     wgt ? "a projection weight of magnitude > 255.87" : "");
    return -4;
  }
  return 0;
}

// Folds a call's status words into a caller-owned accumulator (two floats, device): acc[0] = max over calls of the largest
// out-of-range activation, acc[1] = max over calls of the largest |256 W| -- bit-pattern maxima of non-negative values, so a
// NaN wins over everything.  One 256-thread workgroup, asynchronous.
__global__ __launch_bounds__(256) void status_fold_kernel(const float* __restrict__ status, int n_words, float* __restrict__ acc) {
  if (status[1] != 1.f) return;                       // the call converted nothing to FP16 pieces
  unsigned m = 0;
  for (int i = kStatusHdr + (int)threadIdx.x; i < n_words; i += 256) {
    const unsigned b = __builtin_bit_cast(unsigned, status[i]) & 0x7fffffffu;
    m = b > m ? b : m;
  }
  for (int o = 32; o > 0; o >>= 1) { const unsigned x = (unsigned)__shfl_xor((int)m, o, 64); m = x > m ? x : m; }
  if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned*>(acc) + 1, m);
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(acc), __builtin_bit_cast(unsigned, status[0]) & 0x7fffffffu);
}

int fold_status_words(const float* status, int n_words, float* acc, hipStream_t s, const char* what) {
  CA_CHECK_ARG(acc != nullptr, "%s: null accumulator", what);
  hipLaunchKernelGGL(status_fold_kernel, dim3(1), dim3(256), 0, s, status, n_words, acc);
  if (hipGetLastError() != hipSuccess) { coattn_set_error("%s: launch failed", what); return -3; }
  return 0;
}

extern "C" int coattn_status_accumulate(const void* saved, int B, int N, int T, int d, int L, int dtype, void* acc, void* stream) {
  CA_TRY(check_shape(B, N, T, d, L, dtype));
  CA_CHECK_ARG(saved != nullptr, "status_accumulate: null `saved`");
  const SavedOff sp = saved_off(B, N, T, d, L);
  return fold_status_words((const float*)saved + sp.status, (int)status_floats(d, d, 2), (float*)acc, (hipStream_t)stream,
                           "coattn_status_accumulate");
}

extern "C" int coattn_status(const void* saved, int B, int N, int T, int d, int L, int dtype, void* stream, float* amax) {
  CA_TRY(check_shape(B, N, T, d, L, dtype));
  CA_CHECK_ARG(saved != nullptr, "status: null `saved`");
  const SavedOff sp = saved_off(B, N, T, d, L);
  return read_status_words((const float*)saved + sp.status, (int)status_floats(d, d, 2), (hipStream_t)stream, amax, "coattn_status");
}

// ---------------------------------------------------------------------------------------
// general-shape implementation: MFMA GEMM composition
// ---------------------------------------------------------------------------------------
// COATTN_BF_TN_ROUNDS (developer switch): rounds of workgroups the split-K parts of gemm_bf.hip's weight-gradient kernel fill
int bf_tn_rounds() {
  static const int r = dev_env_int("COATTN_BF_TN_ROUNDS", 1);   // (measured: 1 round 101 us, 2: 128, 3: 152 -- the partial results' round trip)
  return r < 1 ? 1 : r;
}

// ---------------------------------------------------------------------------------------
// gradient jobs on the general GEMM (fused.h), shared by backward_general and the fallback branches of fused_backward
// ---------------------------------------------------------------------------------------
int grad_dw_splitk(const float* dY, const float* X, int K, int d, float* part, float* dW, int accumulate, bool bf16, hipStream_t s,
                   const float* const* Xl, int L, long dy_sl) {
  const SplitK k = splitk_plan(K);
  coattn_gemm_desc g = {};
  g.A = dY; g.a_sm = 1; g.a_sk = d;
  g.B = X; g.b_sk = d; g.b_sn = 1;
  if (!X) {                                          // levels as the inner loop (B from the pointer table)
    g.a_si = (int64_t)dy_sl; g.ptr_by_inner = 1; g.inner = L;
    for (int l = 0; l < L; ++l) g.b_ptrs[l] = Xl[l];
  }
  g.C = part; g.c_sz = (int64_t)d * d; g.c_sm = d; g.c_sn = 1;
  g.M = d; g.N = d; g.K = K; g.batch = k.S; g.ksplit = k.ks;
  CA_TRY(launch_gemm_mode(g, bf16, s));
  return launch_reduce_partials(part, dW, k.S, (int64_t)d * d, accumulate, s);
}

int grad_dw_sample_groups(const float* dPv, const float* V, const VLayout& vl, int B, int N, int d, float* part, float* dW,
                          int accumulate, bool bf16, hipStream_t s) {
  const int G = (B + 31) / 32;                       // inner index = sample, in <= 32 groups
  const int S = (B + G - 1) / G;
  coattn_gemm_desc g = {};
  g.A = dPv; g.a_sm = 1; g.a_sk = d; g.a_si = (int64_t)N * d; g.a_sz = (int64_t)G * N * d;
  g.B = V; g.b_sk = vl.sN; g.b_sn = vl.sD; g.b_si = vl.sB; g.b_sz = (int64_t)G * vl.sB;
  g.C = part; g.c_sz = (int64_t)d * d; g.c_sm = d; g.c_sn = 1;
  g.M = d; g.N = d; g.K = N; g.batch = S; g.inner = G; g.inner_total = B;
  CA_TRY(launch_gemm_mode(g, bf16, s));
  return launch_reduce_partials(part, dW, S, (int64_t)d * d, accumulate, s);
}

int grad_colsum(const float* w, const float* X, int R, int d, float* part, float* out, int accumulate, hipStream_t s) {
  const int rpc = (R + 255) / 256 > 32 ? (R + 255) / 256 : 32;
  int nch = 0;
  CA_TRY(launch_colsum_partial(w, X, part, R, d, rpc, &nch, s));
  return launch_reduce_partials(part, out, nch, d, accumulate, s);
}

int grad_dv_kt_da(const float* Kq, const float* dA, float* dV, const VLayout& dvl, int B, int N, int T, int d, hipStream_t s) {
  coattn_gemm_desc g = {};
  g.A = Kq; g.a_sz = (int64_t)T * d; g.a_sm = 1; g.a_sk = d;
  g.B = dA; g.b_sz = (int64_t)T * N; g.b_sk = N; g.b_sn = 1;
  g.Cin = dV; g.cin_sz = dvl.sB; g.cin_sm = dvl.sD; g.cin_sn = dvl.sN; g.beta = 1.f;
  g.C = dV; g.c_sz = dvl.sB; g.c_sm = dvl.sD; g.c_sn = dvl.sN;
  g.M = d; g.N = N; g.K = T; g.batch = B;
  return launch_gemm_f32(g, s);
}

int grad_dv_wv(const void* Wv, const float* dPv, float* dV, const VLayout& dvl, int B, int N, int d, bool bf16, hipStream_t s) {
  coattn_gemm_desc g = {};
  g.A = Wv; g.a_sm = 1; g.a_sk = d; g.a_sz = 0;
  g.B = dPv; g.b_sz = (int64_t)N * d; g.b_sk = 1; g.b_sn = d;
  g.Cin = dV; g.cin_sz = dvl.sB; g.cin_sm = dvl.sD; g.cin_sn = dvl.sN; g.beta = 1.f;
  g.C = dV; g.c_sz = dvl.sB; g.c_sm = dvl.sD; g.c_sn = dvl.sN;
  g.M = d; g.N = N; g.K = d; g.batch = B;
  return launch_gemm_mode(g, bf16, s);
}

int grad_bilinear_wb(const float* dK, const float* const* Q, int B, int T, int d, int L, float* part, float* dWb, float* dbb,
                     int accumulate, hipStream_t s) {
  for (int l = 0; l < L; ++l)
    CA_TRY(grad_dw_splitk(dK + (size_t)l * B * T * d, Q[l], B * T, d, part, dWb, (accumulate || l > 0) ? 1 : 0, false, s));
  return grad_colsum(nullptr, dK, L * B * T, d, part, dbb, accumulate, s);
}

namespace {

// P_v = V W_v^T + b_v   (model.py:380/384, evaluated once per sample)
int proj_v(const Ctx& c, const float* V, const float* Wv, const float* bv, float* Pv) {
  coattn_gemm_desc g = {};
  g.A = V; g.B = Wv; g.C = Pv; g.bias_n = bv; g.out_scale = c.pscale;
  g.M = c.B * c.N; g.N = c.d; g.K = c.d; g.batch = 1;
  g.a_sm = c.vl.sN; g.a_sk = c.vl.sD;            // row m = (b, n): split rows unless the samples abut
  if (c.vl.sB != (int64_t)c.N * c.vl.sN) { g.a_mdiv = c.N; g.a_sdiv = c.vl.sB; }
  g.b_sk = 1; g.b_sn = c.d;
  g.c_sm = c.d; g.c_sn = 1;
  return launch_gemm_mode(g, c.bf16_proj, c.s);
}
// K_l = Q_l W_b^T + b_b of all levels in one launch (batch z = level, A from the pointer table; COATTN_FLAG_BILINEAR)
int proj_k(const Ctx& c, const float* const* Q) {
  coattn_gemm_desc g = {};
  for (int l = 0; l < c.L; ++l) g.a_ptrs[l] = Q[l];
  g.B = c.Wb; g.C = c.K; g.c_sz = (int64_t)c.B * c.T * c.d; g.bias_n = c.bb;
  g.M = c.B * c.T; g.N = c.d; g.K = c.d; g.batch = c.L;
  g.a_sm = c.d; g.a_sk = 1;
  g.b_sk = 1; g.b_sn = c.d;
  g.c_sm = c.d; g.c_sn = 1;
  return launch_gemm_f32(g, c.s);
}
// C = tanh(Q V)   (model.py:377)
int affinity(const Ctx& c, const float* Q, const float* V, float* C) {
  coattn_gemm_desc g = {};
  g.A = Q; g.a_sz = (int64_t)c.T * c.d; g.a_sm = c.d; g.a_sk = 1;
  g.B = V; g.b_sz = c.vl.sB; g.b_sk = c.vl.sD; g.b_sn = c.vl.sN;
  g.C = C; g.c_sz = (int64_t)c.T * c.N; g.c_sm = c.N; g.c_sn = 1;
  g.M = c.T; g.N = c.N; g.K = c.d; g.batch = c.B; g.act = 1;
  return launch_gemm_f32(g, c.s);
}
// out = act(X + C^T Y): X,out [B,N,d], Y [B,T,d]   (H_v, model.py:380-381; dP_v in backward)
int ct_times(const Ctx& c, const float* C, const float* Y, const float* X, float* out, int act) {
  coattn_gemm_desc g = {};
  g.A = C; g.a_sz = (int64_t)c.T * c.N; g.a_sm = 1; g.a_sk = c.N;
  g.B = Y; g.b_sz = (int64_t)c.T * c.d; g.b_sk = c.d; g.b_sn = 1;
  g.Cin = X; g.cin_sz = (int64_t)c.N * c.d; g.cin_sm = c.d; g.cin_sn = 1; g.beta = 1.f;
  g.C = out; g.c_sz = (int64_t)c.N * c.d; g.c_sm = c.d; g.c_sn = 1;
  g.M = c.N; g.N = c.d; g.K = c.T; g.batch = c.B; g.act = act;
  return launch_gemm_f32(g, c.s);
}
// out = act(X + C Y): X,out [B,T,d], Y [B,N,d]   (H_q, model.py:383-384; dP_q in backward)
int c_times(const Ctx& c, const float* C, const float* Y, const float* X, float* out, int act) {
  coattn_gemm_desc g = {};
  g.A = C; g.a_sz = (int64_t)c.T * c.N; g.a_sm = c.N; g.a_sk = 1;
  g.B = Y; g.b_sz = (int64_t)c.N * c.d; g.b_sk = c.d; g.b_sn = 1;
  g.Cin = X; g.cin_sz = (int64_t)c.T * c.d; g.cin_sm = c.d; g.cin_sn = 1; g.beta = 1.f;
  g.C = out; g.c_sz = (int64_t)c.T * c.d; g.c_sm = c.d; g.c_sn = 1;
  g.M = c.T; g.N = c.d; g.K = c.N; g.batch = c.B; g.act = act;
  return launch_gemm_f32(g, c.s);
}

// out (+)= X W: X, out [B T][d], W [d][d]   (the projections backward: dQ_l += dP_q,l W_q, dK_l W_b)
int add_rows_times_w(const Ctx& c, const float* X, const float* W, float* out, bool bf16 = false) {
  coattn_gemm_desc g = {};
  g.A = X; g.a_sm = c.d; g.a_sk = 1;
  g.B = W; g.b_sk = c.d; g.b_sn = 1;
  g.Cin = out; g.cin_sm = c.d; g.cin_sn = 1; g.beta = 1.f;
  g.C = out; g.c_sm = c.d; g.c_sn = 1;
  g.M = c.B * c.T; g.N = c.d; g.K = c.d; g.batch = 1;
  return launch_gemm_mode(g, bf16, c.s);
}

// Width of the fp32 mode's contractions (fused.h, include/coattn.h "Widths of the fp32 mode").  flags = 0: every
// contraction on the exact three-piece split.  COATTN_FLAG_FAST16: the forward-side contractions on two FP16 pieces, the
// backward's on two bf16 pieces.  Developer switches (builds with -DCOATTN_DEV_SWITCHES only): COATTN_SPLIT=3 forces the exact
// split, COATTN_FWD_F16=0 / COATTN_FWD_F16_KERNEL=0 / COATTN_SPLIT_FWD=3 / COATTN_SPLIT_PQ=3 the bf16 widths of round 4's A/B runs.
static bool fast16(int flags) {
  static const int split = dev_env_int("COATTN_SPLIT", 2);
  return (flags & COATTN_FLAG_FAST16) && !(flags & COATTN_FLAG_EXACT3) && split != 3;
}
static int np_bwd(int flags) { return fast16(flags) ? 2 : 3; }
static int np_projq(int flags) {                    // P_q = Q W_q^T: its error reaches H_v summed over T <= 28 tokens only
  static const int pq = dev_env_int("COATTN_SPLIT_PQ", 2);
  return fast16(flags) ? (pq == 2 ? 2 : 3) : 3;
}
// The forward's projections P_v, P_q on two FP16 pieces (fused.h; tests/test_split_emulation.py: less error than the exact
// split of P_v next to two bf16 pieces of P_q, at half the MFMAs of the former).
static bool f16_fwd(int flags) {
  static const int on = dev_env_int("COATTN_FWD_F16", 1);
  return fast16(flags) && on != 0;
}
static int np_fwd(int flags, bool f16) {            // 4: both phases of the forward kernel on two FP16 pieces (coattn_fwd32.hip)
  static const int fwd = dev_env_int("COATTN_SPLIT_FWD", 2), hk = dev_env_int("COATTN_FWD_F16_KERNEL", 1);
  if (!fast16(flags)) return 3;
  if (f16) return (hk != 0 && fwd == 2) ? 4 : (fwd == 2 ? 2 : 3);
  return f16_fwd(flags) ? 3 : (fwd == 2 ? 2 : 3);   // FP16 pieces wanted but not available for this shape: exact
}

// COATTN_GEMM_W=0 (developer switch): the projections through gemm.hip instead of the pre-split-weight kernel
static bool gemm_w_enabled() {
  static const int on = dev_env_int("COATTN_GEMM_W", 1);
  return on != 0;
}

// The two projection jobs of a forward call on the pre-split-weight kernel (gemm_w.hip): P_v from the image features in
// either layout, P_q of all levels from the pointer table.  Returns through v_w / q_w which of them that kernel takes.
void projection_jobs(const Ctx& c, float* sv, char* wimg, WGemm& wv, WGemm& wq, bool& v_w, bool& q_w, bool want_f16) {
  const coattn_params* p = c.p;
  const SavedOff sp = saved_off(c.B, c.N, c.T, c.d, c.L);
  const size_t BTd = (size_t)c.B * c.T * c.d;
  wv = WGemm{}; wq = WGemm{};
  wv.A = c.V; wv.a_sm = (int)c.vl.sN; wv.Wf = wimg; wv.C = sv + sp.Pv; wv.c_sm = c.d;
  wv.bias_n = (const float*)p->b_v; wv.out_scale = c.pscale; wv.M = c.B * c.N; wv.N = c.d; wv.K = c.d; wv.batch = 1;
  for (int l = 0; l < c.L; ++l) wq.a_ptrs[l] = c.Q[l];
  wq.a_sm = c.d; wq.Wf = wimg + wsplit_bytes(c.d, c.d); wq.C = sv + sp.Pq; wq.c_sz = (long)BTd; wq.c_sm = c.d;
  wq.bias_n = (const float*)p->b_q; wq.out_scale = c.pscale; wq.M = c.B * c.T; wq.N = c.d; wq.K = c.d; wq.batch = c.L;
  wv.bf16 = wq.bf16 = c.bf16_proj ? 1 : 0;          // reduced precision: the same kernels, hi pieces only, one MFMA per product
  wv.np = 3; wq.np = c.np_pq;
  if (want_f16 && !c.bf16_proj) { wv.np = wq.np = 2; wv.f16 = wq.f16 = 1; }   // two FP16 pieces (any M runs on gemm_w then)
  const bool w_ok = gemm_w_enabled();
  v_w = false;
  if (w_ok && c.vl.sD == 1 && c.vl.sB == (long)c.N * c.vl.sN && c.vl.sN < (1L << 24)) {
    v_w = gemm_w_supported(wv) != 0;                 // location-major rows, samples abutting
  } else if (w_ok && c.vl.sN == 1 && c.vl.sD < (1L << 24)) {
    wv.a_sm = 0; wv.a_sk = (int)c.vl.sD; wv.a_mdiv = c.N; wv.a_sdiv = c.vl.sB;   // channel-major, read in place
    v_w = gemm_w_supported(wv) != 0;
  }
  q_w = w_ok && gemm_w_supported(wq);
}
// Tolerance mode: FP16 pieces are used only when BOTH projections run on the pre-split-weight kernel -- it is that launch
// which range-checks the image and question features and the stored projections for the fused kernel behind it
// (coattn_status); any other shape computes exactly.
bool f16_path(const Ctx& c, int flags, int fused) {
  if (!fused || c.bf16_proj || !f16_fwd(flags)) return false;
  WGemm wv, wq;
  bool v_w, q_w;
  projection_jobs(c, nullptr, nullptr, wv, wq, v_w, q_w, true);
  return v_w && q_w;
}

// Does the forward write the bitmap of the live question rows (and run P_q over them alone)?  A function of the call's shapes,
// pointers and mode.  The backward asks it of its own arguments (rowbits_in_saved) to learn whether it MAY use a bitmap; whether
// there is one it learns from the tag the forward left beside it (fused.h kRowTag).
static bool rowbits_predicate(const Ctx& c, const WGemm& wq, const float* sv, bool f16) {
  const coattn_params* p = c.p;
  static const int rows_env = dev_env_int("COATTN_SKIP_ZERO_ROWS", 1);   // developer switch
  const SavedOff sp = saved_off(c.B, c.N, c.T, c.d, c.L);
  return rows_env && !f16 && !c.bf16_proj && gemm_wx_kernel(wq) == 0 && wq.a_sk == 0 && p->b_q &&
         (wq.M + 31) / 32 <= kRowBitsMaxWords && c.d % 256 == 0 && c.d <= 1024 &&
         ((((uintptr_t)p->b_q) | ((uintptr_t)(sv + sp.Pq))) & 15) == 0;      // (16-byte accesses of the flag job)
}
bool rowbits_in_saved(const Ctx& c) {              // (the backward's Ctx: call_ctx answered f16_path for the same call)
  WGemm wv, wq;
  bool v_w, q_w;
  const bool f16 = c.f16_proj && !c.bf16_proj;
  projection_jobs(c, const_cast<float*>(c.saved), nullptr, wv, wq, v_w, q_w, f16);
  return q_w && rowbits_predicate(c, wq, c.saved, f16);
}

// wimg: room for two pre-split weight images (wsplit_bytes(d, d) each) at the end of the forward workspace
// c.keep: also split W_q the other way round into the saved state (sp.wqT) for the backward's dQ projection
int general_projections(const Ctx& c, char* wimg) {
  const coattn_params* p = c.p;
  float* sv = c.state;
  const SavedOff sp = saved_off(c.B, c.N, c.T, c.d, c.L);
  const size_t BTd = (size_t)c.B * c.T * c.d;
  // fp32 projections of row-major activations: the weight is split once, the GEMM reads it as MFMA fragments
  WGemm wv, wq;
  bool v_w, q_w;
  const bool f16 = c.f16_proj && !c.bf16_proj;        // (forward_impl: only when both projections run on gemm_w)
  projection_jobs(c, sv, wimg, wv, wq, v_w, q_w, f16);
  float* status = sv + sp.status;
  if (f16) wv.status = wq.status = status;            // both on two FP16 pieces, range-checked
  RowFlagJob rj = {};
  bool rows_in_gemm = false;
  // the image of W_q^T for the backward's dQ projection: whenever that job runs on the pre-split-weight kernels -- a question of
  // the shape and the mode alone, the backward asks the same one (fused.h dq_proj_job), whatever the alignment of Q here
  const WGemm wdq = dq_proj_job(c.B, c.T, c.d, c.L, c.bf16_proj ? 1 : 0, 3);
  const bool wqT = c.keep && gemm_w_enabled() && gemm_w_supported(wdq);
  unsigned* row_tag = reinterpret_cast<unsigned*>(sv + sp.rowcnt) + kRowTagWord;
  if (v_w || q_w || wqT) {
    WSplit jobs[3];
    int nj = 0;
    // (the image of W_q^T is read by the backward's dQ projection: a GEMM of P_q's shape with row-major A in the same
    //  precision mode, so it runs on the same kernel as P_q and wants the same image format)
    const int chunks = ((c.d + 31) / 32) * ((c.d + 15) / 16);
    if (v_w) jobs[nj++] = WSplit{(const float*)p->W_v, const_cast<void*>(wv.Wf), c.d, c.d, 0, c.d, wimg_pieces(wv), status + kStatusHdr};
    if (q_w) jobs[nj++] = WSplit{(const float*)p->W_q, const_cast<void*>(wq.Wf), c.d, c.d, 0, c.d, wimg_pieces(wq), status + kStatusHdr + chunks};
    if (wqT) jobs[nj++] = WSplit{(const float*)p->W_q, sv + sp.wqT, c.d, c.d, 1, c.d, wimg_pieces(wdq), nullptr};
    // Question rows of exact zeros -- the pad tokens (model.py:263, :292-296) -- project to the bias alone: the launch's extra
    // workgroups flag the rows of Q_l that hold anything, write (0 + b_q) * scale into the others' rows of P_q, and the exact
    // four-wave GEMM runs over the flagged rows only (same values bit for bit; 44 % fewer rows on BASELINE's synthetic
    // questions, lengths U{3..26} of 26).  Row-major A on gemm_w_kernel only: the other kernels compute every row.
    const bool skip_rows = q_w && rowbits_predicate(c, wq, sv, f16);
    if (skip_rows) {
      unsigned* bits = reinterpret_cast<unsigned*>(sv + sp.rowbits);        // (kept in `saved`: the backward's dW_q reads it)
      for (int l = 0; l < c.L; ++l) rj.a_ptrs[l] = c.Q[l];
      rj.a_sm = c.d; rj.C = sv + sp.Pq; rj.c_sz = (long)BTd; rj.c_sm = c.d;
      rj.bias_n = (const float*)p->b_q; rj.out_scale = c.pscale; rj.M = c.B * c.T; rj.N = c.d; rj.K = c.d; rj.batch = c.L;
      rj.rowbits = bits;
      rj.qlen = c.qlen; rj.T = c.T;                 // (length mask: rows past a question's length are not live)
      wq.rowbits = bits;
      // COATTN_FLAGS_IN_GEMM=1 (developer switch, DEV builds): the flag workgroups at the head of the PROJECTION launch instead,
      // its P_q tiles waiting on a counter the weight-split launch zeroes.  Measured and not adopted: the weight-split launch
      // gets its 6.6 us back, the projection launch loses 12.5 at N = 49 (392 flag workgroups hold the slots the first tiles
      // want) and 5 at N = 196 (LAB_NOTES A6.3)
      static const int in_gemm_env = dev_env_int("COATTN_FLAGS_IN_GEMM", 0);
      if (in_gemm_env) rj.rowcnt = reinterpret_cast<unsigned*>(sv + sp.rowcnt);
    }
    rows_in_gemm = skip_rows && rj.rowcnt != nullptr;
    CA_TRY(launch_wsplit(jobs, nj, c.s, status, f16 ? 1 : 0, (skip_rows && !rows_in_gemm) ? &rj : nullptr,
                         rows_in_gemm ? rj.rowcnt : nullptr, row_tag, skip_rows ? &rj : nullptr));
    // (also writes the header of the call's status words, and sets or clears the bitmap's tag)
    prof_mark(c.s, "wsplit");
  } else {                                            // no weight-split launch on this path: header = "no FP16 pieces", no bitmap
    if (hipMemsetAsync(status, 0, 2 * sizeof(float), c.s) != hipSuccess ||
        hipMemsetAsync(row_tag, 0, 3 * sizeof(unsigned), c.s) != hipSuccess) { coattn_set_error("forward: hipMemsetAsync failed"); return -3; }
  }
  if (v_w && q_w) {                                   // both projections in one launch
    const WGemm both[2] = {wv, wq};
    CA_TRY(launch_gemm_wx(both, 2, c.s, rows_in_gemm ? &rj : nullptr));
    prof_mark(c.s, "projections");
    return 0;
  }
  if (v_w) CA_TRY(launch_gemm_wx(&wv, 1, c.s));
  else CA_TRY(proj_v(c, c.V, (const float*)p->W_v, (const float*)p->b_v, sv + sp.Pv));
  if (q_w) return launch_gemm_wx(&wq, 1, c.s, rows_in_gemm ? &rj : nullptr);
  // P_q of all levels in one launch: batch z = level, A from the pointer table
  coattn_gemm_desc g = {};
  for (int l = 0; l < c.L; ++l) g.a_ptrs[l] = c.Q[l];
  g.B = p->W_q; g.C = sv + sp.Pq; g.c_sz = (int64_t)BTd; g.bias_n = p->b_q; g.out_scale = c.pscale;
  g.M = c.B * c.T; g.N = c.d; g.K = c.d; g.batch = c.L;
  g.a_sm = c.d; g.a_sk = 1;
  g.b_sk = 1; g.b_sn = c.d;
  g.c_sm = c.d; g.c_sn = 1;
  return launch_gemm_mode(g, c.bf16_proj, c.s);
}

// COATTN_FLAG_BILINEAR: K = Q W_b^T + b_b of all levels.  On the pre-split-weight kernels whenever P_q runs there -- the same
// kernel, width and FP16-piece mode as P_q (the tolerance mode range-checks the stored K: it is phase 1's FP16-piece operand), W_b
// split by a launch of its own into the third image of the forward workspace, whose |256 W| words are folded into W_q's (the
// range report covers both weights) -- else on the general GEMM.  Dense: pad rows take b_b, not the P_q bitmap's bias path.
int bilinear_projection(const Ctx& c, char* wimg_b) {
  float* sv = c.state;
  const SavedOff sp = saved_off(c.B, c.N, c.T, c.d, c.L);
  WGemm wv, wq;
  bool v_w, q_w;
  const bool f16 = c.f16_proj && !c.bf16_proj;
  projection_jobs(c, sv, nullptr, wv, wq, v_w, q_w, f16);
  if (!q_w) return proj_k(c, c.Q);
  WGemm wk = wq;
  wk.Wf = wimg_b; wk.C = c.K; wk.bias_n = c.bb; wk.out_scale = 1.f; wk.rowbits = nullptr;
  float* status = sv + sp.status;
  float* wb_words = c.K + al64((size_t)c.L * c.B * c.T * c.d);
  wk.status = f16 ? status : nullptr;
  const WSplit job{c.Wb, wimg_b, c.d, c.d, 0, c.d, wimg_pieces(wk), f16 ? wb_words : nullptr};
  CA_TRY(launch_wsplit(&job, 1, c.s));
  if (f16) CA_TRY(launch_max_words(status + kStatusHdr + wchunks(c.d), wb_words, (int)wchunks(c.d), c.s));
  CA_TRY(launch_gemm_wx(&wk, 1, c.s));
  prof_mark(c.s, "bilinear_projection");
  return 0;
}

// everything after the projections: affinity, H_v / H_q, scores, softmax, attended reductions
int general_attention(const Ctx& c) {
  const SavedOff sp = saved_off(c.B, c.N, c.T, c.d, c.L);
  const coattn_params* p = c.p;
  float* sv = c.state;
  float* Pv = sv + sp.Pv;
  float* Hv = c.tail;
  const size_t BTd = (size_t)c.B * c.T * c.d, BTN = (size_t)c.B * c.T * c.N;
  for (int l = 0; l < c.L; ++l) {
    float* Pq = sv + sp.Pq + l * BTd;
    float* C = sv + sp.C + l * BTN;
    float* Hq = sv + sp.Hq + l * BTd;
    const size_t lBN = (size_t)l * c.B * c.N, lBT = (size_t)l * c.B * c.T;
    const MapDst av = map_dst(c, sv + sp.av + lBN, c.av_out ? c.av_out + lBN : nullptr);
    const MapDst aq = map_dst(c, sv + sp.aq + lBT, c.aq_out ? c.aq_out + lBT : nullptr);
    CA_TRY(affinity(c, c.K ? c.K + l * BTd : c.Q[l], c.V, C));   // (bilinear: A = K V^T; q below stays a_q^T Q)
    if (c.qlen) CA_TRY(launch_mask_rows(C, c.qlen, c.B, c.T, c.N, c.s));   // length mask: C rows t >= len_b are zero
    CA_TRY(ct_times(c, C, Pq, Pv, Hv, 1));
    CA_TRY(c_times(c, C, Pv, Pq, Hq, 1));
    CA_TRY(launch_score_softmax(Hv, (const float*)p->w_v, (const float*)p->c_v, av.to, c.B, c.N, c.d, c.s, nullptr, av.copy));
    CA_TRY(launch_score_softmax(Hq, (const float*)p->w_q, (const float*)p->c_q, aq.to, c.B, c.T, c.d, c.s, c.qlen, aq.copy));
    // v = sum_n a_v[n] V[:,n]   (model.py:391);  q = sum_t a_q[t] Q[t,:]   (model.py:392)
    CA_TRY(launch_gemv(c.V, av.to, c.v_out + (size_t)l * c.B * c.d, c.B, c.d, c.N, c.vl.sB, c.vl.sD, c.vl.sN, c.N, c.d, c.s));
    CA_TRY(launch_gemv(c.Q[l], aq.to, c.q_out + (size_t)l * c.B * c.d, c.B, c.d, c.T, (int64_t)c.T * c.d, 1, c.d, c.T, c.d, c.s));
  }
  return 0;
}

int backward_general(const Ctx& c) {
  const SavedOff sp = saved_off(c.B, c.N, c.T, c.d, c.L);
  const BwdPlan bp = plan_bwd(c.B, c.N, c.T, c.d, c.L);
  const int B = c.B, N = c.N, T = c.T, d = c.d, L = c.L, accumulate = c.accumulate;
  const size_t BTd = (size_t)B * T * d, BTN = (size_t)B * T * N, BNd = (size_t)B * N * d, Bd = (size_t)B * d;
  const float* Pv = c.saved + sp.Pv;
  const float* wv = (const float*)c.p->w_v;
  const float* wq = (const float*)c.p->w_q;
  float* Hv = c.ws + bp.Hv;
  float* dPv = c.ws + bp.dPv;
  float* dZq = c.ws + bp.dZq;
  float* dC = c.ws + bp.dC;
  float* dav = c.ws + bp.dav;
  float* dsv = c.ws + bp.dsv;
  float* daq = c.ws + bp.daq;
  float* dsq = c.ws + bp.dsq;
  float* part = c.ws + bp.part;
  for (int l = 0; l < L; ++l) {
    const float* Pq = c.saved + sp.Pq + l * BTd;
    const float* C = c.saved + sp.C + l * BTN;
    const float* Hq = c.saved + sp.Hq + l * BTd;
    const float* av = c.saved + sp.av + (size_t)l * B * N;
    const float* aq = c.saved + sp.aq + (size_t)l * B * T;
    const float* gv = c.gv + l * Bd;
    const float* gq = c.gq + l * Bd;
    float* dPq = c.ws + bp.dPq + l * BTd;
    const int acc_l = (accumulate || l > 0) ? 1 : 0;
    // recompute H_v = tanh(P_v + C^T P_q)
    CA_TRY(ct_times(c, C, Pq, Pv, Hv, 1));
    // softmax backward of a_v, a_q
    CA_TRY(launch_gemv(c.V, gv, dav, B, N, d, c.vl.sB, c.vl.sN, c.vl.sD, d, N, c.s));
    // (coattn_backward_maps: da + G, the map's own upstream gradient -- G_aq read as 0 past a question's length)
    CA_TRY(launch_softmax_bwd(av, dav, dsv, B, N, c.s, c.g_av ? c.g_av + (size_t)l * B * N : nullptr));
    CA_TRY(launch_gemv(c.Q[l], gq, daq, B, T, d, (int64_t)T * d, d, 1, d, T, c.s));
    if (c.qlen) CA_TRY(launch_mask_rows(daq, c.qlen, B, T, 1, c.s));   // (a_q = 0 there: ds_q = 0 whatever the pad rows hold)
    CA_TRY(launch_softmax_bwd(aq, daq, dsq, B, T, c.s, c.g_aq ? c.g_aq + (size_t)l * B * T : nullptr, c.qlen));
    // dw_v += ds_v^T H_v ; dc_v += sum ds_v ; same for q
    CA_TRY(grad_colsum(dsv, Hv, B * N, d, part, (float*)c.pg->dw_v, acc_l, c.s));
    CA_TRY(launch_sum_all(dsv, (float*)c.pg->dc_v, (int64_t)B * N, acc_l, c.s));
    CA_TRY(grad_colsum(dsq, Hq, B * T, d, part, (float*)c.pg->dw_q, acc_l, c.s));
    CA_TRY(launch_sum_all(dsq, (float*)c.pg->dc_q, (int64_t)B * T, acc_l, c.s));
    // dZ_v (in place over H_v), dZ_q
    CA_TRY(launch_dz(dsv, wv, Hv, Hv, (int64_t)B * N, d, c.s));
    CA_TRY(launch_dz(dsq, wq, Hq, dZq, (int64_t)B * T, d, c.s));
    // dP_q = dZ_q + C dZ_v
    CA_TRY(c_times(c, C, Hv, dZq, dPq, 0));
    // dC = P_q dZ_v^T + dZ_q P_v^T ; dA = dC (1 - C^2)
    {
      coattn_gemm_desc g = {};
      g.A = Pq; g.a_sz = (int64_t)T * d; g.a_sm = d; g.a_sk = 1;
      g.B = Hv; g.b_sz = (int64_t)N * d; g.b_sk = 1; g.b_sn = d;
      g.C = dC; g.c_sz = (int64_t)T * N; g.c_sm = N; g.c_sn = 1;
      g.M = T; g.N = N; g.K = d; g.batch = B;
      CA_TRY(launch_gemm_f32(g, c.s));
      g.A = dZq; g.B = Pv; g.Cin = dC; g.cin_sz = g.c_sz; g.cin_sm = N; g.cin_sn = 1; g.beta = 1.f;
      CA_TRY(launch_gemm_f32(g, c.s));
    }
    CA_TRY(launch_dtanh(dC, C, dC, (int64_t)BTN, c.s));
    if (c.qlen) CA_TRY(launch_mask_rows(dC, c.qlen, B, T, N, c.s));     // length mask: dA rows t >= len_b are zero
    // dP_v(level) = dZ_v + C^T dZ_q   (in place), accumulate over levels
    CA_TRY(ct_times(c, C, dZq, Hv, Hv, 0));
    CA_TRY(launch_add_inplace(dPv, Hv, (int64_t)BNd, l > 0 ? 1 : 0, c.s));
    // dQ_l = a_q (x) gq + dA V^T   (+ dP_q W_q below);  bilinear: dK_l = dA V^T, dQ_l = a_q (x) gq + dK_l W_b (+ dP_q W_q)
    CA_TRY(launch_rank1(aq, gq, c.dQ[l], B, T, d, (int64_t)T * d, d, 1, 0, c.s));
    float* dKl = c.K ? c.dK + l * BTd : nullptr;
    {
      coattn_gemm_desc g = {};
      g.A = dC; g.a_sz = (int64_t)T * N; g.a_sm = N; g.a_sk = 1;
      g.B = c.V; g.b_sz = c.vl.sB; g.b_sk = c.vl.sN; g.b_sn = c.vl.sD;
      if (!dKl) { g.Cin = c.dQ[l]; g.cin_sz = (int64_t)T * d; g.cin_sm = d; g.cin_sn = 1; g.beta = 1.f; }
      g.C = dKl ? dKl : c.dQ[l]; g.c_sz = (int64_t)T * d; g.c_sm = d; g.c_sn = 1;
      g.M = T; g.N = d; g.K = N; g.batch = B;
      CA_TRY(launch_gemm_f32(g, c.s));
    }
    if (dKl) CA_TRY(add_rows_times_w(c, dKl, c.Wb, c.dQ[l]));
    // dV (+)= a_v (x) gv + Q^T dA   (bilinear: K^T dA)
    if (c.dV) CA_TRY(launch_rank1(av, gv, c.dV, B, N, d, c.dvl.sB, c.dvl.sN, c.dvl.sD, l > 0 ? 1 : 0, c.s));
    if (c.dV) CA_TRY(grad_dv_kt_da(c.K ? c.K + l * BTd : c.Q[l], dC, c.dV, c.dvl, B, N, T, d, c.s));
  }
  // projections backward
  for (int l = 0; l < L; ++l) CA_TRY(add_rows_times_w(c, c.ws + bp.dPq + l * BTd, (const float*)c.p->W_q, c.dQ[l], c.bf16_proj));
  if (c.dV) CA_TRY(grad_dv_wv(c.p->W_v, dPv, c.dV, c.dvl, B, N, d, c.bf16_proj, c.s));
  CA_TRY(grad_dw_sample_groups(dPv, c.V, c.vl, B, N, d, part, (float*)c.pg->dW_v, accumulate, c.bf16_proj, c.s));
  CA_TRY(grad_colsum(nullptr, dPv, B * N, d, part, (float*)c.pg->db_v, accumulate, c.s));
  // dW_q[j][k] += sum_m dP_q[m][j] Q_l[m][k],  m over (b,t): split-K, level by level
  for (int l = 0; l < L; ++l)
    CA_TRY(grad_dw_splitk(c.ws + bp.dPq + l * BTd, c.Q[l], B * T, d, part, (float*)c.pg->dW_q, (accumulate || l > 0) ? 1 : 0,
                          c.bf16_proj, c.s));
  CA_TRY(grad_colsum(nullptr, c.ws + bp.dPq, L * B * T, d, part, (float*)c.pg->db_q, accumulate, c.s));
  if (c.K) CA_TRY(grad_bilinear_wb(c.dK, c.Q, B, T, d, L, part, (float*)c.pg->dW_b, (float*)c.pg->db_b, accumulate, c.s));
  return 0;
}

// The fused forward reads V in 16-byte units (LDS-DMA in phase 1, the attended-feature passes of location-major features): every
// sample must start on a 16-byte boundary -- the base pointer, and v_sB a multiple of 4 floats (include/coattn.h "Layouts").
// Anything else is a general-shape call, in the forward and the backward alike: both ask here with the same V, so a state is
// always read by the path that wrote it.
int pick_impl(int flags, const void* V, int B, int N, int T, int d, int L, const VLayout& vl, int* fused) {
  const int sel = flags & 3;
  const bool aligned = (((uintptr_t)V) & 15) == 0 && (vl.sB & 3) == 0;
  const int ok = fused_supported(B, N, T, d, L) && fused_layout_ok(vl, N, d) && aligned;
  if (sel == COATTN_IMPL_FUSED) {
    CA_CHECK_ARG(ok, "fused kernels do not support B=%d N=%d T=%d d=%d L=%d with V strides (%ld, %ld, %ld)%s", B, N, T, d, L,
                 vl.sB, vl.sN, vl.sD, aligned ? "" : ": V and v_sB must be 16-byte aligned");
    *fused = 1;
  } else if (sel == COATTN_IMPL_GENERAL) {
    *fused = 0;
  } else {
    *fused = ok;
  }
  return 0;
}

}  // namespace

// The call descriptor (fused.h Ctx) of the arguments every entry point shares; the wrappers add their own.
static Ctx call_args(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q, const int32_t* q_len,
                     const coattn_params* p, int B, int N, int T, int d, int L, void* stream) {
  Ctx c{B, N, T, d, L, (hipStream_t)stream, VLayout{(long)v_sB, (long)v_sN, (long)v_sD}};
  c.V = (const float*)V; c.Q = (const float* const*)Q; c.p = p; c.qlen = q_len;
  return c;
}

// The modes of a call, derived alike by the forward and by the backward of its state: the backward re-asks the forward's
// questions about the same call (rowbits_in_saved), on the same Ctx.
static void call_modes(Ctx& c, int flags, int fused) {
  c.bf16_proj = (flags & COATTN_FLAG_BF16_PROJ) != 0;
  c.f16_proj = f16_path(c, flags, fused);
  // (the general-shape path stays exact throughout; a fused shape without the FP16 path too -- unless the developer switch
  //  COATTN_FWD_F16=0 asks for round 4's bf16 widths)
  c.np_pq = (fused && fast16(flags) && !f16_fwd(flags)) ? np_projq(flags) : 3;
  c.np_fwd = np_fwd(flags, c.f16_proj);
  c.np_bwd = np_bwd(flags);
  c.pscale = fused ? kPScale : 1.f;
  c.wgemm = gemm_w_enabled();
}

// COATTN_FLAG_BILINEAR: the refusals of include/coattn.h (pg: the backward's gradients, NULL in a forward)
static int check_bilinear(int flags, const coattn_params* p, const coattn_param_grads* pg) {
  if (!bilinear(flags)) return 0;
  CA_CHECK_ARG(!(flags & COATTN_FLAG_BF16_PROJ), "COATTN_FLAG_BILINEAR is not available in the reduced-precision mode (COATTN_FLAG_BF16_PROJ)");
  CA_CHECK_ARG(p->W_b && p->b_b, "COATTN_FLAG_BILINEAR: null W_b / b_b");
  CA_CHECK_ARG(!pg || (pg->dW_b && pg->db_b), "COATTN_FLAG_BILINEAR: null dW_b / db_b");
  return 0;
}

int check_vlayout(const VLayout& v, int N, int d, const char* what) {
  CA_CHECK_ARG(v.sN > 0 && v.sD > 0 && v.sB > 0, "%s: strides must be positive (sB=%ld sN=%ld sD=%ld)", what, v.sB, v.sN, v.sD);
  // the extent of one sample must not reach into the next one
  CA_CHECK_ARG((long)(N - 1) * v.sN + (long)(d - 1) * v.sD < v.sB, "%s: sample stride %ld is smaller than a sample's extent", what, v.sB);
  return 0;
}

// c: the call as its wrapper filled it -- c.state = `saved` (NULL: forward only -- the state lives in the workspace, and the
// fused kernel stores no C / H_q: nothing reads them), c.av_out / c.aq_out the caller's map buffers (may be NULL)
static int forward_impl(Ctx c, void* ws, int dtype, int flags, bool do_proj) {
  const int B = c.B, N = c.N, T = c.T, d = c.d, L = c.L;
  const coattn_params* p = c.p;
  CA_TRY(check_shape(B, N, T, d, L, dtype));
  CA_CHECK_ARG(c.V && c.Q && p && c.v_out && c.q_out && ws, "forward: null argument");
  CA_TRY(check_vlayout(c.vl, N, d, "forward: V"));
  for (int l = 0; l < L; ++l) CA_CHECK_ARG(c.Q[l] != nullptr, "forward: Q[%d] is null", l);
  CA_CHECK_ARG(p->W_v && p->b_v && p->W_q && p->b_q && p->w_v && p->c_v && p->w_q && p->c_q,
               "forward: null parameter pointer");
  const bool bil = bilinear(flags);
  CA_TRY(check_bilinear(flags, p, nullptr));
  int fused = 0;
  CA_TRY(pick_impl(flags, c.V, B, N, T, d, L, c.vl, &fused));
  c.keep = c.state != nullptr;
  if (!c.keep) c.state = (float*)ws;                  // inference: state lives in the workspace
  c.tail = (float*)ws + saved_floats(B, N, T, d, L, bil);
  call_modes(c, flags, fused);
  if (bil) { c.Wb = (const float*)p->W_b; c.bb = (const float*)p->b_b; c.K = c.state + saved_off(B, N, T, d, L).total; }
  if (do_proj) {
    char* wimg = (char*)ws + fwd_ws_floats(B, N, T, d, L, bil) * sizeof(float);
    CA_TRY(general_projections(c, wimg));
    if (bil) CA_TRY(bilinear_projection(c, wimg + 2 * wsplit_bytes(d, d)));
  }
  return fused ? fused_attention_forward(c) : general_attention(c);
}

extern "C" int coattn_forward_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                                  const int32_t* q_len, const coattn_params* p, void* v_out, void* q_out, void* saved, void* ws,
                                  int B, int N, int T, int d, int L, int dtype, int flags, void* stream) {
  Ctx c = call_args(V, v_sB, v_sN, v_sD, Q, q_len, p, B, N, T, d, L, stream);
  c.v_out = (float*)v_out; c.q_out = (float*)q_out; c.state = (float*)saved;
  return forward_impl(c, ws, dtype, flags, true);
}

extern "C" int coattn_forward(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                              const coattn_params* p, void* v_out, void* q_out, void* saved, void* ws, int B, int N,
                              int T, int d, int L, int dtype, int flags, void* stream) {
  return coattn_forward_len(V, v_sB, v_sN, v_sD, Q, nullptr, p, v_out, q_out, saved, ws, B, N, T, d, L, dtype, flags, stream);
}

extern "C" int coattn_forward_maps_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                                       const int32_t* q_len, const coattn_params* p, void* v_out, void* q_out, void* av_out,
                                       void* aq_out, void* saved, void* ws, int B, int N, int T, int d, int L, int dtype, int flags,
                                       void* stream) {
  CA_CHECK_ARG(saved != nullptr, "forward_maps: null `saved` (the backward state is required; coattn_infer keeps none)");
  CA_CHECK_ARG(av_out && aq_out, "forward_maps: null map buffer (av_out [L,B,N] and aq_out [L,B,T] are required)");
  Ctx c = call_args(V, v_sB, v_sN, v_sD, Q, q_len, p, B, N, T, d, L, stream);
  c.v_out = (float*)v_out; c.q_out = (float*)q_out; c.state = (float*)saved;
  c.av_out = (float*)av_out; c.aq_out = (float*)aq_out;
  return forward_impl(c, ws, dtype, flags, true);
}

extern "C" int coattn_forward_maps(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                                   const coattn_params* p, void* v_out, void* q_out, void* av_out, void* aq_out, void* saved,
                                   void* ws, int B, int N, int T, int d, int L, int dtype, int flags, void* stream) {
  return coattn_forward_maps_len(V, v_sB, v_sN, v_sD, Q, nullptr, p, v_out, q_out, av_out, aq_out, saved, ws, B, N, T, d, L,
                                 dtype, flags, stream);
}

extern "C" int coattn_infer_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                                const int32_t* q_len, const coattn_params* p, void* v_out, void* q_out, void* av_out,
                                void* aq_out, void* ws, int B, int N, int T, int d, int L, int dtype, int flags, void* stream) {
  Ctx c = call_args(V, v_sB, v_sN, v_sD, Q, q_len, p, B, N, T, d, L, stream);
  c.v_out = (float*)v_out; c.q_out = (float*)q_out;
  c.av_out = (float*)av_out; c.aq_out = (float*)aq_out;
  return forward_impl(c, ws, dtype, flags, true);
}

extern "C" int coattn_infer(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                            const coattn_params* p, void* v_out, void* q_out, void* av_out, void* aq_out, void* ws, int B,
                            int N, int T, int d, int L, int dtype, int flags, void* stream) {
  return coattn_infer_len(V, v_sB, v_sN, v_sD, Q, nullptr, p, v_out, q_out, av_out, aq_out, ws, B, N, T, d, L, dtype, flags,
                          stream);
}

extern "C" int coattn_attention_forward_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                                            const int32_t* q_len, const coattn_params* p, void* v_out, void* q_out, void* saved,
                                            void* ws, int B, int N, int T, int d, int L, int dtype, int flags, void* stream) {
  CA_CHECK_ARG(saved != nullptr, "attention_forward: needs the saved buffer of a previous coattn_forward");
  Ctx c = call_args(V, v_sB, v_sN, v_sD, Q, q_len, p, B, N, T, d, L, stream);
  c.v_out = (float*)v_out; c.q_out = (float*)q_out; c.state = (float*)saved;
  return forward_impl(c, ws, dtype, flags, false);
}

extern "C" int coattn_attention_forward(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                                        const coattn_params* p, void* v_out, void* q_out, void* saved, void* ws,
                                        int B, int N, int T, int d, int L, int dtype, int flags, void* stream) {
  return coattn_attention_forward_len(V, v_sB, v_sN, v_sD, Q, nullptr, p, v_out, q_out, saved, ws, B, N, T, d, L, dtype,
                                      flags, stream);
}

// c: the call as coattn_backward_maps_len filled it (c.g_av / c.g_aq may be NULL = 0, c.dV may be NULL)
static int backward_impl(Ctx c, int dtype, int flags) {
  const int B = c.B, N = c.N, T = c.T, d = c.d, L = c.L;
  const coattn_params* p = c.p;
  const coattn_param_grads* pg = c.pg;
  CA_TRY(check_shape(B, N, T, d, L, dtype));
  CA_CHECK_ARG(c.V && c.Q && p && c.saved && c.gv && c.gq && c.dQ && pg && c.ws, "backward: null argument");  // dV may be NULL
  CA_TRY(check_vlayout(c.vl, N, d, "backward: V"));
  if (c.dV) CA_TRY(check_vlayout(c.dvl, N, d, "backward: dV"));
  else c.dvl = c.vl;
  for (int l = 0; l < L; ++l) CA_CHECK_ARG(c.Q[l] && c.dQ[l], "backward: Q[%d]/dQ[%d] is null", l, l);
  CA_CHECK_ARG(pg->dW_v && pg->db_v && pg->dW_q && pg->db_q && pg->dw_v && pg->dc_v && pg->dw_q && pg->dc_q,
               "backward: null parameter-gradient pointer");
  CA_TRY(check_bilinear(flags, p, pg));
  int fused = 0;
  CA_TRY(pick_impl(flags, c.V, B, N, T, d, L, c.vl, &fused));
  call_modes(c, flags, fused);
  BilBwd bb = {};
  if (bilinear(flags)) {                              // K from the forward's `saved`, dK into the workspace
    c.Wb = (const float*)p->W_b; c.bb = (const float*)p->b_b;
    c.K = const_cast<float*>(c.saved) + saved_off(B, N, T, d, L).total;
    c.dK = c.ws + bwd_ws_floats(B, N, T, d, L, false);
    const size_t k = al64((size_t)L * B * T * d);
    bb.Wb = c.Wb; bb.K = c.K; bb.dK = c.dK; bb.dpk = c.dK + k; bb.wstack = c.dK + 3 * k;
    bb.wimg = c.dK + 3 * k + al64((size_t)2 * d * d);
    bb.zeros = (float*)bb.wimg + al64(wsplit_bytes(d, 2 * d) / sizeof(float) + 1);
    bb.dWb = (float*)pg->dW_b; bb.dbb = (float*)pg->db_b;
    c.bil = &bb;
  }
  // (`saved` of the fused forward holds P_v, P_q scaled by kPScale: only the fused backward may read it)
  CA_CHECK_ARG(!fused || fused_backward_supported(B, N, T, d, L), "backward: the fused forward's saved state has no fused backward for this shape");
  if (!fused) return backward_general(c);
  c.live_rows = rowbits_in_saved(c);
  return fused_backward(c);
}

extern "C" int coattn_backward_maps_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                                        const int32_t* q_len, const coattn_params* p, const void* saved, const void* gv,
                                        const void* gq, const void* g_av, const void* g_aq, void* dV, int64_t dv_sB,
                                        int64_t dv_sN, int64_t dv_sD, void* const* dQ, const coattn_param_grads* pg,
                                        int accumulate, void* ws, int B, int N, int T, int d, int L, int dtype, int flags,
                                        void* stream) {
  Ctx c = call_args(V, v_sB, v_sN, v_sD, Q, q_len, p, B, N, T, d, L, stream);
  c.saved = (const float*)saved; c.gv = (const float*)gv; c.gq = (const float*)gq;
  c.g_av = (const float*)g_av; c.g_aq = (const float*)g_aq;
  c.dV = (float*)dV; c.dvl = VLayout{(long)dv_sB, (long)dv_sN, (long)dv_sD}; c.dQ = (float* const*)dQ;
  c.pg = pg; c.accumulate = accumulate; c.ws = (float*)ws;
  return backward_impl(c, dtype, flags);
}

extern "C" int coattn_backward_len(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                                   const int32_t* q_len, const coattn_params* p, const void* saved, const void* gv,
                                   const void* gq, void* dV, int64_t dv_sB, int64_t dv_sN, int64_t dv_sD, void* const* dQ,
                                   const coattn_param_grads* pg, int accumulate, void* ws, int B, int N, int T, int d,
                                   int L, int dtype, int flags, void* stream) {
  return coattn_backward_maps_len(V, v_sB, v_sN, v_sD, Q, q_len, p, saved, gv, gq, nullptr, nullptr, dV, dv_sB, dv_sN, dv_sD, dQ,
                                  pg, accumulate, ws, B, N, T, d, L, dtype, flags, stream);
}

extern "C" int coattn_backward_maps(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                                    const coattn_params* p, const void* saved, const void* gv, const void* gq, const void* g_av,
                                    const void* g_aq, void* dV, int64_t dv_sB, int64_t dv_sN, int64_t dv_sD, void* const* dQ,
                                    const coattn_param_grads* pg, int accumulate, void* ws, int B, int N, int T, int d, int L,
                                    int dtype, int flags, void* stream) {
  return coattn_backward_maps_len(V, v_sB, v_sN, v_sD, Q, nullptr, p, saved, gv, gq, g_av, g_aq, dV, dv_sB, dv_sN, dv_sD, dQ, pg,
                                  accumulate, ws, B, N, T, d, L, dtype, flags, stream);
}

extern "C" int coattn_backward(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q,
                               const coattn_params* p, const void* saved, const void* gv, const void* gq, void* dV,
                               int64_t dv_sB, int64_t dv_sN, int64_t dv_sD, void* const* dQ,
                               const coattn_param_grads* pg, int accumulate, void* ws, int B, int N, int T, int d,
                               int L, int dtype, int flags, void* stream) {
  return coattn_backward_len(V, v_sB, v_sN, v_sD, Q, nullptr, p, saved, gv, gq, dV, dv_sB, dv_sN, dv_sD, dQ, pg, accumulate,
                             ws, B, N, T, d, L, dtype, flags, stream);
}
