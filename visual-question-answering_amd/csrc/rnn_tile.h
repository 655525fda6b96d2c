// What the recurrent layers share (lstm.hip, gru.hip): the 32 x 32 tile product of their step kernels -- the contraction split
// over eight waves on the exact v_mfma_f32_32x32x2_f32, the waves' partial tiles summed through LDS in wave order -- and the
// GEMM jobs around the recurrence: the projection of all B T rows, the two weight gradients, dX.  G is the layer's number of
// gates (4 for the LSTM, 3 for the GRU): the projections are [B T][G H].  Everything sits in an anonymous namespace: each
// file that includes this header gets its own copies, as it would of its own helpers.
#pragma once
#include "common.h"
#include "fused.h"

namespace {

constexpr int kWaves = 8, kThreads = 64 * kWaves;
constexpr int kLdRed = 33;                           // row stride of a wave's partial tile in LDS (conflict-free both ways)

__device__ __forceinline__ int clamp_len(int v, int T) { return v < 1 ? 1 : (v > T ? T : v); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// acc += A[32 x K] B[K x 32] over this wave's share of the 8-wide k chunks [lo, hi): lane (r, h) holds four consecutive k
// of row r of A starting at 8 c + 4 h, MFMA j contracts k = 8 c + j (h = 0) and 8 c + 4 + j (h = 1) -- one fixed order.
// BT: B is stored [column][k] (a_row-like, 16-byte loads); else [k][column] with row stride ldb (one dword per k).
template <bool BT>
__device__ __forceinline__ void load_chunk(const float* __restrict__ a_row, const float* __restrict__ b_ptr, long ldb, int k, f32x4& a,
                                           f32x4& b) {
  a = *reinterpret_cast<const f32x4*>(a_row + k);
  if (BT) {
    b = *reinterpret_cast<const f32x4*>(b_ptr + k);
  } else {
    b[0] = b_ptr[(long)k * ldb]; b[1] = b_ptr[(long)(k + 1) * ldb];
    b[2] = b_ptr[(long)(k + 2) * ldb]; b[3] = b_ptr[(long)(k + 3) * ldb];
  }
}
// (measured and not adopted: issuing the loads of eight chunks ahead of their MFMAs by hand -- the LSTM's backward step went from
//  21 to 35 us at cfg 2's shape, the forward from 12.7 to 12.1; the compiler's own schedule of this plain loop stays)
template <bool BT>
__device__ __forceinline__ f32x16 contract(const float* __restrict__ a_row, const float* __restrict__ b_ptr, long ldb, int lo, int hi,
                                           int h) {
  f32x16 acc = {};
  for (int c = lo; c < hi; ++c) {
    f32x4 a, b;
    load_chunk<BT>(a_row, b_ptr, ldb, 8 * c + 4 * h, a, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
  }
  return acc;
}

// the wave's tile into red[w]: register i of lane (r, h) is element (row (i & 3) + 8 (i >> 2) + 4 h, column r)
__device__ __forceinline__ void store_partial(float* red_w, const f32x16& acc, int r, int h) {
#pragma unroll
  for (int i = 0; i < 16; ++i) red_w[((i & 3) + 8 * (i >> 2) + 4 * h) * kLdRed + r] = acc[i];
}
__device__ __forceinline__ float sum_partials(const float* red, int row, int col) {
  float s = red[row * kLdRed + col];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) s += red[w * 32 * kLdRed + row * kLdRed + col];   // wave order: one fixed order
  return s;
}

// ---- the GEMM jobs ------------------------------------------------------------------------------------------------------
// G_x [B T][G H] = X W_ih^T + b_ih
WGemm proj_job(const float* X, const float* bih, float* Gx, const void* wimg, int B, int T, int E, int H, int G) {
  WGemm g = {};
  g.A = X; g.a_sm = E; g.Wf = wimg; g.C = Gx; g.c_sm = G * H; g.bias_n = bih; g.out_scale = 1.f;
  g.M = B * T; g.N = G * H; g.K = E; g.batch = 1; g.np = 3;
  return g;
}
// the exact pre-split-weight projection (coattn_linear_forward's kernels; wimg: wsplit_bytes(G H, E)), gemm.hip for the shapes
// it refuses
int project(const float* X, const float* Wih, const float* bih, float* Gx, void* wimg, int B, int T, int E, int H, int G, hipStream_t s) {
  const WGemm g = proj_job(X, bih, Gx, wimg, B, T, E, H, G);
  if (gemm_w_supported(g)) {
    const WSplit job{Wih, wimg, G * H, E, 0, E, wimg_pieces(g), nullptr};
    CA_TRY(launch_wsplit(&job, 1, s));
    return launch_gemm_wx(&g, 1, s);
  }
  coattn_gemm_desc d = {};
  d.A = X; d.a_sm = E; d.a_sk = 1;
  d.B = Wih; d.b_sk = 1; d.b_sn = E;
  d.C = Gx; d.c_sm = G * H; d.c_sn = 1; d.bias_n = bih;
  d.M = B * T; d.N = G * H; d.K = E; d.batch = 1;
  return launch_gemm_f32(d, s);
}

// dW [n_out][n_in] (+)= dY^T X over R rows: split-K parts on gemm_tn.hip, or as split-K batches of gemm.hip for the shapes
// that kernel refuses (n_out, n_in no multiples of 128, R < 16); then the deterministic reduce.  Returns the parts.
TnGemm wgrad_job(const float* dY, const float* X, float* part, int R, int n_out, int n_in) {
  TnGemm g = {};
  g.A = dY; g.a_ld = n_out; g.B = X; g.b_ld = n_in; g.C = part; g.M = n_out; g.N = n_in; g.K = R; g.levels = 1; g.np = 3;
  return g;
}
int wgrad_parts(int R, int n_out, int n_in) {
  const TnGemm g = wgrad_job(nullptr, nullptr, nullptr, R, n_out, n_in);
  int ks, S;
  return gemm_tn_supported(g) ? gemm_tn_plan(g, 32, &ks, &S) : splitk_plan(R).S;
}
int wgrad(const float* dY, const float* X, float* part, float* dW, int R, int n_out, int n_in, int accumulate, hipStream_t s) {
  const TnGemm g = wgrad_job(dY, X, part, R, n_out, n_in);
  int parts;
  if (gemm_tn_supported(g)) {
    int ks, S;
    parts = gemm_tn_plan(g, 32, &ks, &S);
    CA_TRY(launch_gemm_tn(&g, &ks, &S, 1, s));
  } else {
    const SplitK k = splitk_plan(R);
    coattn_gemm_desc d = {};
    d.A = dY; d.a_sm = 1; d.a_sk = n_out;
    d.B = X; d.b_sk = n_in; d.b_sn = 1;
    d.C = part; d.c_sz = (int64_t)n_out * n_in; d.c_sm = n_in; d.c_sn = 1;
    d.M = n_out; d.N = n_in; d.K = R; d.batch = k.S; d.ksplit = k.ks;
    CA_TRY(launch_gemm_f32(d, s));
    parts = k.S;
  }
  return launch_reduce_partials(part, dW, parts, (int64_t)n_out * n_in, accumulate, s);
}

// dX [B T][E] = dG W_ih over the G H gate gradients: the exact pre-split-weight projection against the image of W_ih^T
// (wimg: wsplit_bytes(E, G H)), gemm.hip for the shapes it refuses
WGemm dx_job(const float* dG, float* dX, const void* wimg, int B, int T, int E, int H, int G) {
  WGemm g = {};
  g.A = dG; g.a_sm = G * H; g.Wf = wimg; g.C = dX; g.c_sm = E; g.out_scale = 1.f;
  g.M = B * T; g.N = E; g.K = G * H; g.batch = 1; g.np = 3;
  return g;
}
int dx_product(const float* dG, const float* Wih, float* dX, void* wimg, int B, int T, int E, int H, int G, hipStream_t s) {
  const WGemm g = dx_job(dG, dX, wimg, B, T, E, H, G);
  if (gemm_w_supported(g)) {
    const WSplit job{Wih, wimg, E, G * H, 1, E, wimg_pieces(g), nullptr};
    CA_TRY(launch_wsplit(&job, 1, s));
    return launch_gemm_wx(&g, 1, s);
  }
  coattn_gemm_desc d = {};
  d.A = dG; d.a_sm = G * H; d.a_sk = 1;
  d.B = Wih; d.b_sk = E; d.b_sn = 1;
  d.C = dX; d.c_sm = E; d.c_sn = 1;
  d.M = B * T; d.N = E; d.K = G * H; d.batch = 1;
  return launch_gemm_f32(d, s);
}

}  // namespace
