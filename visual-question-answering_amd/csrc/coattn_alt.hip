// Alternating co-attention (Lu et al. 2016, section 3.3; include/coattn.h v0.11.0): three chained guided-attention steps
//     guided(X, g):  H = tanh(X W_x^T + b_x + g),  a = softmax_R(H w_h^T + c_h),  x^ = a^T X
//     step 1: s^ = guided(Q, 0)           step 2: v^ = guided(V, s^ W_g2^T + b_g2)      step 3: q^ = guided(Q, v^ W_g3^T + b_g3)
// The contractions run on the existing exact three-piece kernels (the pre-split-weight projection kernels gemm_w.hip, the
// weight-gradient kernel gemm_tn.hip; other shapes on the general GEMM, gemm.hip).  What is new is the guided-attention step
// itself, forward and backward (guided_fwd_kernel / guided_bwd_kernel below): per sample and level it reads the projected rows
// X W_x^T + b_x once for the scores (forward) or for dH (backward), and the rows of X once for x^ (forward) or for da
// (backward).  Step 2 takes the L levels of a sample in one workgroup: the image rows V and X2 = V W_x2^T + b_x2 do not depend
// on the level, so they are read once per sample.  No float atomics: every sum runs in a fixed order (bitwise repeatable).
#include "common.h"
#include "fused.h"
#include <initializer_list>

namespace {

constexpr int kAltMaxL = 4;            // levels per call (the question hierarchy has 3)
constexpr int kAltMaxR = 512;          // rows per step: T and N
constexpr int kAltMaxD = 1024;         // hidden size
// threads per workgroup: 512 for steps 1 and 3 (one workgroup per sample and level), 1024 for step 2 (one per sample: B of them,
// fewer than the CUs at B = 160, so each takes all the waves it can)
template <int NLV> constexpr int alt_threads() { return NLV == 1 ? 512 : 1024; }

// One guided-attention step for a workgroup: sample b = blockIdx.x, levels [l0, l0 + nl) with l0 = blockIdx.y (NLV = 1: one
// level, steps 1 and 3) or l0 = 0, nl = L (NLV = kAltMaxL: step 2, the levels share X and P).
//   X(l, r, j) = x[l][b x_sB + r x_sR + j x_sD]       the attended rows (Q_l or V)
//   P(l, r, j) = p + l p_sL + (b R + r) p_ld + j      their projection X W_x^T + b_x (p_sL = 0: shared by the levels)
//   g(l, j)    = g[(l B + b) d + j]                   the guide vector (NULL: 0)
struct GuidedArgs {
  const float* x[kAltMaxL]; long x_sB, x_sR, x_sD;
  const float* p; long p_sL; int p_ld;
  const float* g;
  const float* w; const float* c;      // w_h [d], c_h [1]
  const int* len;                      // [B] or NULL (the softmax over r < clamp(len_b, 1, R))
  int B, R, d, L;
  // forward
  float* a; float* a2; float* xhat;    // a [L][B][R] (a2: a copy, may be NULL), xhat [L][B][d]
  // backward
  const float* a_in;                   // the forward's a [L][B][R]
  const float* gx; const float* gx2;   // upstream gradient of x^ [L][B][d] (gx2 may be NULL: added to gx)
  const float* ga;                     // upstream gradient of a [L][B][R] or NULL
  float* gx_tot;                       // (may be NULL) gx + gx2, stored [L][B][d]
  float* dh; long dh_sL; int dh_ld;    // dH rows (NLV > 1: the sum over the levels), at dh + l dh_sL + (b R + r) dh_ld
  float* dg;                           // [L][B][d] sum_r dH_r, or NULL
  float* dw_part;                      // [(l B + b) or b][d + 1]: sum_r ds_r H_r, then sum_r ds_r
};

__device__ __forceinline__ int alt_rows(const GuidedArgs& a, int b) {
  if (!a.len) return a.R;
  const int n = a.len[b];
  return n < 1 ? 1 : (n > a.R ? a.R : n);
}

// sum over the workgroup of NW waves in a fixed order; every thread gets the result
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) t += red[i];
  return t;
}
template <int NW>
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) t = fmaxf(t, red[i]);
  return t;
}

template <int NLV>
__global__ __launch_bounds__(alt_threads<NLV>()) void guided_fwd_kernel(const GuidedArgs a) {
  constexpr int kAltThreads = alt_threads<NLV>(), kAltWaves = kAltThreads / 64, kAltMaxCols = kAltMaxD / kAltThreads;
  __shared__ float gs[NLV][kAltMaxD];
  __shared__ float ws[kAltMaxD];
  __shared__ float sc[NLV][kAltMaxR];
  __shared__ float red[16];
  const int b = blockIdx.x, l0 = NLV == 1 ? (int)blockIdx.y : 0, nl = NLV == 1 ? 1 : a.L;
  const int d = a.d, R = a.R, Re = alt_rows(a, b), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < d; j += kAltThreads) {
    ws[j] = a.w[j];
#pragma unroll
    for (int v = 0; v < NLV; ++v)
      if (v < nl) gs[v][j] = a.g ? a.g[((long)(l0 + v) * a.B + b) * d + j] : 0.f;
  }
  __syncthreads();
  const float c = a.c[0];
  // scores h_r = w_h . tanh(P_r + g) + c_h over the live rows: one wave per row
  const float* prow0 = a.p + (long)l0 * a.p_sL + (long)b * R * a.p_ld;
  for (int r = wave; r < Re; r += kAltWaves) {
    const float* pr = prow0 + (long)r * a.p_ld;
    float s[NLV];
#pragma unroll
    for (int v = 0; v < NLV; ++v) s[v] = 0.f;
    for (int j = lane; j < d; j += 64) {
      const float x = pr[j], w = ws[j];
#pragma unroll
      for (int v = 0; v < NLV; ++v)
        if (v < nl) s[v] += w * tanh_fast(x + gs[v][j]);
    }
#pragma unroll
    for (int v = 0; v < NLV; ++v) {
      const float t = wave_sum(s[v]);
      if (v < nl && lane == 0) sc[v][r] = t + c;
    }
  }
  __syncthreads();
  // softmax over r < Re; a = 0 beyond
#pragma unroll
  for (int v = 0; v < NLV; ++v) {
    if (v >= nl) break;
    float m = -INFINITY;
    for (int r = tid; r < Re; r += kAltThreads) m = fmaxf(m, sc[v][r]);
    m = block_max<kAltWaves>(m, red);
    float e = 0.f;
    for (int r = tid; r < Re; r += kAltThreads) e += expf(sc[v][r] - m);
    const float inv = 1.f / block_sum<kAltWaves>(e, red);
    __syncthreads();
    const long ao = ((long)(l0 + v) * a.B + b) * R;
    for (int r = tid; r < R; r += kAltThreads) {
      const float av = r < Re ? expf(sc[v][r] - m) * inv : 0.f;
      a.a[ao + r] = av;
      if (a.a2) a.a2[ao + r] = av;
      if (r < Re) sc[v][r] = av;
    }
  }
  __syncthreads();
  // x^ = sum_r a_r X_r: one thread per column, the rows in order
  const float* xb = a.x[l0] + (long)b * a.x_sB;
#pragma unroll
  for (int k = 0; k < kAltMaxCols; ++k) {
    const int j = tid + k * kAltThreads;
    if (j >= d) break;
    float acc[NLV];
#pragma unroll
    for (int v = 0; v < NLV; ++v) acc[v] = 0.f;
    const float* xj = xb + (long)j * a.x_sD;
#pragma unroll 4
    for (int r = 0; r < Re; ++r) {
      const float x = xj[(long)r * a.x_sR];
#pragma unroll
      for (int v = 0; v < NLV; ++v) acc[v] += sc[v][r] * x;
    }
#pragma unroll
    for (int v = 0; v < NLV; ++v)
      if (v < nl) a.xhat[((long)(l0 + v) * a.B + b) * d + j] = acc[v];
  }
}

template <int NLV>
__global__ __launch_bounds__(alt_threads<NLV>()) void guided_bwd_kernel(const GuidedArgs a) {
  constexpr int kAltThreads = alt_threads<NLV>(), kAltWaves = kAltThreads / 64, kAltMaxCols = kAltMaxD / kAltThreads;
  __shared__ float gs[NLV][kAltMaxD];
  __shared__ float gxs[NLV][kAltMaxD];
  __shared__ float ws[kAltMaxD];
  __shared__ float as[NLV][kAltMaxR];
  __shared__ float dss[NLV][kAltMaxR];
  __shared__ float red[16];
  const int b = blockIdx.x, l0 = NLV == 1 ? (int)blockIdx.y : 0, nl = NLV == 1 ? 1 : a.L;
  const int d = a.d, R = a.R, Re = alt_rows(a, b), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < d; j += kAltThreads) {
    ws[j] = a.w[j];
#pragma unroll
    for (int v = 0; v < NLV; ++v)
      if (v < nl) {
        const long o = ((long)(l0 + v) * a.B + b) * d + j;
        gs[v][j] = a.g ? a.g[o] : 0.f;
        const float t = a.gx2 ? a.gx[o] + a.gx2[o] : a.gx[o];
        gxs[v][j] = t;
        if (a.gx_tot) a.gx_tot[o] = t;
      }
  }
#pragma unroll
  for (int v = 0; v < NLV; ++v)
    if (v < nl)
      for (int r = tid; r < Re; r += kAltThreads) as[v][r] = a.a_in[((long)(l0 + v) * a.B + b) * R + r];
  __syncthreads();
  // da_r = X_r . gx^ (+ G_a): one wave per live row
  const float* xb = a.x[l0] + (long)b * a.x_sB;
  for (int r = wave; r < Re; r += kAltWaves) {
    const float* xr = xb + (long)r * a.x_sR;
    float s[NLV];
#pragma unroll
    for (int v = 0; v < NLV; ++v) s[v] = 0.f;
    for (int j = lane; j < d; j += 64) {
      const float x = xr[(long)j * a.x_sD];
#pragma unroll
      for (int v = 0; v < NLV; ++v) s[v] += x * gxs[v][j];
    }
#pragma unroll
    for (int v = 0; v < NLV; ++v) {
      const float t = wave_sum(s[v]);
      if (v < nl && lane == 0) dss[v][r] = t + (a.ga ? a.ga[((long)(l0 + v) * a.B + b) * R + r] : 0.f);
    }
  }
  __syncthreads();
  // ds = a (.) (da - sum_r a da); dc_h part = sum_r ds
  float dcs = 0.f;
#pragma unroll
  for (int v = 0; v < NLV; ++v) {
    if (v >= nl) break;
    // ds_r = a_r (da_r - sum a da) in two passes: S = sum a da in fp32 is off by about eps |da|, which the plain formula
    // leaves in sum_r ds_r (it should be 0) -- as large as ds itself when the da of the live rows are close to each other.
    // The second pass measures what is left, S2 = sum a (da - S), and takes it out: sum_r ds_r is then 0 to the rounding of
    // ds, and the rounding of da moves all ds_r of a sample by one common factor (without it: 6.3e-5 on dW_x3 at d = 1,
    // LAB_NOTES.md section 11)
    float t = 0.f;
    for (int r = tid; r < Re; r += kAltThreads) t += as[v][r] * dss[v][r];
    const float S = block_sum<kAltWaves>(t, red);
    float t2 = 0.f;
    for (int r = tid; r < Re; r += kAltThreads) t2 += as[v][r] * (dss[v][r] - S);
    const float S2 = block_sum<kAltWaves>(t2, red);
    float u = 0.f;
    for (int r = tid; r < Re; r += kAltThreads) {
      const float ds = as[v][r] * ((dss[v][r] - S) - S2);
      dss[v][r] = ds;
      u += ds;
    }
    dcs += block_sum<kAltWaves>(u, red);
  }
  __syncthreads();
  // dH_r = ds_r w_h (.) (1 - H_r^2) with H recomputed from P and g: one thread per column, the rows in order
  const float* pb = a.p + (long)l0 * a.p_sL + (long)b * R * a.p_ld;
  float* dhb = a.dh + (long)l0 * a.dh_sL + (long)b * R * a.dh_ld;
  float* wp = a.dw_part + (long)(NLV == 1 ? l0 * a.B + b : b) * (d + 1);
#pragma unroll
  for (int k = 0; k < kAltMaxCols; ++k) {
    const int j = tid + k * kAltThreads;
    if (j >= d) break;
    const float w = ws[j];
    float dg[NLV], gj[NLV];
#pragma unroll
    for (int v = 0; v < NLV; ++v) { dg[v] = 0.f; gj[v] = gs[v][j]; }
    float dw = 0.f;
#pragma unroll 2
    for (int r = 0; r < Re; ++r) {
      const float pr = pb[(long)r * a.p_ld + j];
      float sum = 0.f;
#pragma unroll
      for (int v = 0; v < NLV; ++v) {
        if (v < nl) {
          const float H = tanh_fast(pr + gj[v]), ds = dss[v][r];
          const float dh = ds * w * (1.f - H * H);
          dg[v] += dh;
          dw += ds * H;
          sum += dh;
        }
      }
      dhb[(long)r * a.dh_ld + j] = sum;
    }
    for (int r = Re; r < R; ++r) dhb[(long)r * a.dh_ld + j] = 0.f;   // (masked steps 1 / 3: the pad rows of dH)
    wp[j] = dw;
    if (a.dg) {
#pragma unroll
      for (int v = 0; v < NLV; ++v)
        if (v < nl) a.dg[((long)(l0 + v) * a.B + b) * d + j] = dg[v];
    }
  }
  if (tid == 0) wp[d] = dcs;
}

// dQ_l[b][t][:] += a_s[l][b][t] ds^[l][b][:] + a_q[l][b][t] gq[l][b][:]   (the rank-1 terms of x^ = a^T X, steps 1 and 3)
struct DqRank1 { float* dq[kAltMaxL]; const float* as; const float* gs; const float* aq; const float* gq; int B, T, d; };
__global__ __launch_bounds__(256) void alt_dq_rank1_kernel(const DqRank1 k) {
  const int l = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x, n = (long)k.B * k.T * k.d;
  if (i >= n) return;
  const long bt = i / k.d, b = bt / k.T;
  const int j = (int)(i - bt * k.d);
  const long lbt = (long)l * k.B * k.T + bt, lb = ((long)l * k.B + b) * k.d + j;
  k.dq[l][i] += k.as[lbt] * k.gs[lb] + k.aq[lbt] * k.gq[lb];
}

// dV[b][n][:] += sum_l a_v[l][b][n] gv^[l][b][:]   (strided dV)
struct DvRank1 { float* dv; long sB, sN, sD; const float* av; const float* gv; int B, N, d, L; };
__global__ __launch_bounds__(256) void alt_dv_rank1_kernel(const DvRank1 k) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, n = (long)k.B * k.N * k.d;
  if (i >= n) return;
  long b, r, j;
  if (k.sN == 1) { r = i % k.N; const long bj = i / k.N; j = bj % k.d; b = bj / k.d; }       // channel-major: along n
  else { j = i % k.d; const long br = i / k.d; r = br % k.N; b = br / k.N; }
  float t = 0.f;
  for (int l = 0; l < k.L; ++l) t += k.av[((long)l * k.B + b) * k.N + r] * k.gv[((long)l * k.B + b) * k.d + j];
  float* o = k.dv + b * k.sB + r * k.sN + j * k.sD;
  *o += t;
}

// up to 12 reductions dst[i][j] (+)= sum_p src[i][p ld_i + j], j < n_i, in a fixed order (partials of the weight / bias gradients)
struct AltReduce { const float* src[12]; float* dst[12]; long n[12], ld[12]; int nparts[12]; int njobs, accumulate; };
__global__ __launch_bounds__(256) void alt_reduce_kernel(const AltReduce r) {
  __shared__ float red[4][64];
  const int job = blockIdx.y, col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const long j = (long)blockIdx.x * 64 + col, n = r.n[job], ld = r.ld[job];
  if ((long)blockIdx.x * 64 >= n) return;
  const float* src = r.src[job];
  float acc = 0.f;
  if (j < n) {
    const int np = r.nparts[job];
    int p = grp;
    for (; p + 28 < np; p += 32) {                   // eight loads in flight per thread, added in order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(long)(p + 4 * u) * ld + j];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; p < np; p += 4) acc += src[(long)p * ld + j];
  }
  red[grp][col] = acc;
  __syncthreads();
  if (grp == 0 && j < n) {
    const float t = (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
    float* o = r.dst[job] + j;
    *o = r.accumulate ? *o + t : t;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------

struct AltSaved {                      // offsets in floats (forward -> backward state; in `ws` when saved is NULL)
  size_t x13, x2, g2, g3, sh, vh, as, av, aq, total;
};
AltSaved alt_saved(int B, int N, int T, int d, int L) {
  AltSaved s;
  size_t o = 0;
  s.x13 = o; o += al64((size_t)L * B * T * 2 * d);   // [X1 | X3] = Q_l [W_x1; W_x3]^T + [b_x1; b_x3]
  s.x2 = o;  o += al64((size_t)B * N * d);           // X2 = V W_x2^T + b_x2
  s.g2 = o;  o += al64((size_t)L * B * d);           // s^ W_g2^T + b_g2
  s.g3 = o;  o += al64((size_t)L * B * d);           // v^ W_g3^T + b_g3
  s.sh = o;  o += al64((size_t)L * B * d);           // s^
  s.vh = o;  o += al64((size_t)L * B * d);           // v^
  s.as = o;  o += al64((size_t)L * B * T);
  s.av = o;  o += al64((size_t)L * B * N);
  s.aq = o;  o += al64((size_t)L * B * T);
  s.total = o;
  return s;
}
// floats of the weight image a linear job writes for W [N][K] (AltLinear::img), the size of every img* slot of both plans
size_t alt_img_floats(int N, int K) { return al64(wsplit_bytes(N, K) / sizeof(float) + 1); }
struct AltFwdWs { size_t wcat, bcat, img13, img2, imgg2, imgg3, total; };    // floats, after the saved-sized block
AltFwdWs alt_fwd_ws(int d) {
  AltFwdWs w;
  size_t o = 0;
  w.wcat = o; o += al64((size_t)2 * d * d);
  w.bcat = o; o += al64((size_t)2 * d);
  w.img13 = o; o += alt_img_floats(2 * d, d);
  w.img2 = o; o += alt_img_floats(d, d);
  w.imgg2 = o; o += alt_img_floats(d, d);
  w.imgg3 = o; o += alt_img_floats(d, d);
  w.total = o;
  return w;
}
struct AltBwdWs { size_t dh13, dx2, dg1, dg2, dg3, dvt, dsh, wp1, wp2, wp3, part, wcat, img13, img2, imgg2, imgg3, total; };
constexpr int kAltMaxParts = 32;
AltBwdWs alt_bwd_ws(int B, int N, int T, int d, int L) {
  AltBwdWs w;
  size_t o = 0;
  w.dh13 = o; o += al64((size_t)L * B * T * 2 * d);
  w.dx2 = o;  o += al64((size_t)B * N * d);
  w.dg1 = o;  o += al64((size_t)L * B * d);
  w.dg2 = o;  o += al64((size_t)L * B * d);
  w.dg3 = o;  o += al64((size_t)L * B * d);
  w.dvt = o;  o += al64((size_t)L * B * d);
  w.dsh = o;  o += al64((size_t)L * B * d);
  w.wp1 = o;  o += al64((size_t)L * B * (d + 1));
  w.wp2 = o;  o += al64((size_t)B * (d + 1));
  w.wp3 = o;  o += al64((size_t)L * B * (d + 1));
  w.part = o; o += al64((size_t)kAltMaxParts * 2 * d * d);   // split-K parts of the weight gradients
  w.wcat = o; o += al64((size_t)2 * d * d);
  w.img13 = o; o += alt_img_floats(d, 2 * d);
  w.img2 = o; o += alt_img_floats(d, d);
  w.imgg2 = o; o += alt_img_floats(d, d);
  w.imgg3 = o; o += alt_img_floats(d, d);
  w.total = o;
  return w;
}

int alt_check(int B, int N, int T, int d, int L, int dtype, int flags) {
  CA_CHECK_ARG(dtype == COATTN_F32, "alternating co-attention: unsupported dtype %d (only COATTN_F32)", dtype);
  CA_CHECK_ARG(flags == 0, "alternating co-attention: flags must be 0 (exact mode only; COATTN_FLAG_FAST16, COATTN_FLAG_BF16_PROJ, "
               "COATTN_FLAG_BILINEAR and the impl selectors are not supported), got %d", flags);
  CA_CHECK_ARG(B > 0 && B <= 65535, "alternating co-attention: bad batch size B=%d", B);
  CA_CHECK_ARG(N > 0 && N <= kAltMaxR && T > 0 && T <= kAltMaxR, "alternating co-attention: N=%d / T=%d outside [1, %d]", N, T, kAltMaxR);
  CA_CHECK_ARG(d > 0 && d <= kAltMaxD, "alternating co-attention: hidden size d=%d outside [1, %d]", d, kAltMaxD);
  CA_CHECK_ARG(L > 0 && L <= kAltMaxL, "alternating co-attention: L=%d outside [1, %d]", L, kAltMaxL);
  return 0;
}

// One alternating call as its C-ABI wrapper fills it once alt_check has passed; every step of the forward and the backward
// reads its operands, offsets and base pointers from here.
struct AltCall {
  int B, N, T, d, L;
  hipStream_t s;
  const float* V; VLayout vl;            // x_img[B,N,d] by its element strides
  const float* const* Q;                 // [L] levels [B][T][d]
  const int* qlen;                       // [B] or NULL
  const coattn_alt_params* p;
  AltSaved so;                           // offsets of the state ...
  const float* sv;                       // ... in the caller's `saved`, or (forward, saved NULL) at the head of the workspace
  float* ws;                             // the workspace (forward: behind the state when it holds it), offsets fo / wo
  // forward
  float* st;                             // sv, to write
  bool keep;                             // the caller gave `saved`
  float* v_out; float* q_out; float* av_out; float* aq_out;   // [L][B][d] x 2; [L][B][N], [L][B][T], each may be NULL
  AltFwdWs fo;
  // backward
  const float* gv; const float* gq;      // [L][B][d] upstream gradients of v, q
  const float* g_av; const float* g_aq;  // upstream gradients of the maps, NULL = 0
  float* dV; VLayout dvl;                // NULL: the image features need no gradient
  float* const* dQ;
  const coattn_alt_param_grads* pg;      // NULL in a forward
  int accumulate;
  AltBwdWs wo;
};
AltCall alt_call(const void* V, VLayout vl, const void* const* Q, const int32_t* q_len, const coattn_alt_params* p, int B, int N,
                 int T, int d, int L, void* stream) {
  AltCall c = {};
  c.B = B; c.N = N; c.T = T; c.d = d; c.L = L; c.s = (hipStream_t)stream;
  c.V = (const float*)V; c.vl = vl; c.Q = (const float* const*)Q; c.qlen = q_len; c.p = p;
  c.so = alt_saved(B, N, T, d, L);
  return c;
}

// The pointers a call cannot do without: `req` by name, then every level of Q and the 16 parameters (backward: with dQ's
// levels and the 16 gradients)
struct AltReq { const void* ptr; const char* name; };
int alt_check_ptrs(const AltCall& c, const char* fn, std::initializer_list<AltReq> req) {
  for (const AltReq& a : req) CA_CHECK_ARG(a.ptr, "%s: %s is NULL", fn, a.name);
  const void* const* pp = (const void* const*)c.p;
  void* const* gp = (void* const*)c.pg;
  for (int l = 0; l < c.L; ++l) {
    if (gp) { CA_CHECK_ARG(c.Q[l] && c.dQ[l], "%s: Q[%d] / dQ[%d] is NULL", fn, l, l); }
    else { CA_CHECK_ARG(c.Q[l], "%s: Q[%d] is NULL", fn, l); }
  }
  for (int i = 0; i < 16; ++i) {
    if (gp) { CA_CHECK_ARG(pp[i] && gp[i], "%s: parameter or gradient %d is NULL", fn, i); }
    else { CA_CHECK_ARG(pp[i], "%s: parameter %d is NULL", fn, i); }
  }
  return 0;
}

// How the general GEMM walks the M rows of an operand: row-major rows `ld` apart (v NULL), or the [B, n, cols] view `v`, whose
// rows split by sample (mdiv / sdiv) only when the samples do not abut.  rows: the view is plain row-major rows as well
struct AltRows { long sm, sk; int mdiv; long sdiv; bool rows; };
AltRows alt_rows_of(const VLayout* v, int ld, int n, int cols) {
  if (!v) return AltRows{ld, 1, 0, 0, true};
  const bool abut = v->sB == (long)n * v->sN;
  return AltRows{v->sN, v->sD, abut ? 0 : n, abut ? 0 : v->sB, v->sD == 1 && v->sN == cols && v->sB == (long)n * cols};
}

// The linear job: y[z][m][:] = x[z][m][:] W^T + bias (W [N][K], the forward's projections) or x[z][m][:] W (w_kn: W [K][N], the
// back-projections dx = dy W), M rows per batch entry -- on the pre-split-weight kernel when it takes the shape (the weight
// image `img` is written here), else on the general GEMM
struct AltLinear {
  const float* x; const float* const* x_tab; long x_sz; int ld_x;    // x_z: table entry z, or x + z x_sz; rows ld_x apart ...
  const VLayout* x_view;                                             // ... or (not NULL) x as a [M / n, n, K] view by its strides
  const float* W; bool w_kn; const float* bias;                      // bias [N] or NULL
  float* y; float* const* y_tab; long y_sz; int ld_y;                // the same for y
  const VLayout* y_view;                                             // [M / n, n, N]
  int M, N, K, batch, n;                                             // n: rows per sample of a view
  void* img;                                                         // the job's weight-image slot (alt_img_floats(N, K) floats)
};
// one batch entry of plain rows, x rows K and y rows N apart
AltLinear alt_rows_job(const float* x, const float* W, bool w_kn, const float* bias, float* y, int M, int N, int K, void* img) {
  AltLinear l = {};
  l.x = x; l.ld_x = K; l.W = W; l.w_kn = w_kn; l.bias = bias; l.y = y; l.ld_y = N; l.M = M; l.N = N; l.K = K; l.batch = 1; l.img = img;
  return l;
}
int alt_linear(const AltLinear& l, hipStream_t s) {
  const AltRows a = alt_rows_of(l.x_view, l.ld_x, l.n, l.K), c = alt_rows_of(l.y_view, l.ld_y, l.n, l.N);
  WGemm g = {};
  g.A = l.x; g.Wf = l.img; g.C = l.y; g.c_sz = l.y_sz; g.c_sm = (int)c.sm; g.bias_n = l.bias; g.out_scale = 1.f;
  g.M = l.M; g.N = l.N; g.K = l.K; g.batch = l.batch; g.np = 3;
  if (a.rows) {
    g.a_sm = (int)a.sm;
    g.a_sz = l.x_tab || l.batch > 1 ? l.x_sz : 0;      // (0 for a single unbatched operand)
  } else {                                             // channel-major x: A contiguous along m (the kernel's a_sk form)
    g.a_sk = (int)a.sk; g.a_mdiv = l.n; g.a_sdiv = l.x_view->sB;
  }
  coattn_gemm_desc e = {};
  e.A = l.x; e.a_sz = l.x_sz; e.a_sm = a.sm; e.a_sk = a.sk; e.a_mdiv = a.mdiv; e.a_sdiv = a.sdiv;
  e.B = l.W; e.b_sk = l.w_kn ? l.N : 1; e.b_sn = l.w_kn ? 1 : l.K;
  e.C = l.y; e.c_sz = l.y_sz; e.c_sm = c.sm; e.c_sn = c.sk; e.c_mdiv = c.mdiv; e.c_sdiv = c.sdiv; e.bias_n = l.bias;
  e.M = l.M; e.N = l.N; e.K = l.K; e.batch = l.batch;
  for (int t = 0; t < l.batch; ++t) {
    if (l.x_tab) { g.a_ptrs[t] = l.x_tab[t]; e.a_ptrs[t] = l.x_tab[t]; }
    if (l.y_tab) { g.c_ptrs[t] = l.y_tab[t]; e.c_ptrs[t] = l.y_tab[t]; }
  }
  // The kernel stores rows only (a strided y: the general GEMM) and takes a view of x only along m, within the offsets its
  // a_sk form keeps (a_sk is an int).  Its 16-byte stores need no test of their own: ld_y is d or 2d and K, a multiple of
  // 32 here, is d or 2d, so ld_y % 4 == 0
  const bool view_ok = a.rows || (l.x_view->sN == 1 && l.x_view->sD < (1L << 30) && l.x_view->sB < (1L << 40));
  if (c.rows && view_ok && gemm_w_supported(g) && !gemm_bf_supported(g)) {
    const WSplit job{l.W, l.img, l.N, l.K, l.w_kn ? 1 : 0, l.w_kn ? l.N : l.K, wimg_pieces(g), nullptr};
    CA_TRY(launch_wsplit(&job, 1, s));
    return launch_gemm_wx(&g, 1, s);
  }
  return launch_gemm_f32(e, s);
}

// the next job of a reduce launch: dst[j] (+)= sum over p < nparts of src[p ld + j], j < n
void alt_reduce_job(AltReduce& r, const float* src, void* dst, long n, long ld, int nparts) {
  const int k = r.njobs++;
  r.src[k] = src; r.dst[k] = (float*)dst; r.n[k] = n; r.ld[k] = ld; r.nparts[k] = nparts;
}
int launch_alt_reduce(const AltReduce& r, hipStream_t s) {
  long nmax = 0;
  for (int i = 0; i < r.njobs; ++i) nmax = r.n[i] > nmax ? r.n[i] : nmax;
  hipLaunchKernelGGL(alt_reduce_kernel, dim3((unsigned)((nmax + 63) / 64), r.njobs), dim3(256), 0, s, r);
  CA_CHECK_LAUNCH("alt_reduce");
  return 0;
}

// The weight-gradient job: dW (+)= sum over rows of dY^T X, dY rows [rows][n_out] (ld_dy) per level, X rows [rows][n_in] (ld_x)
// per level (x_tab) or once (x); the [n_out][n_in] result may be split by rows into dW0 (rows < split) and dW1.  Parts in the
// call's workspace + a fixed-order reduce.  The parts come from gemm_tn when it takes the shape, else from the general GEMM's
// split-K level by level; X = the image features in another layout than rows (x_view): from the general GEMM over groups of
// G = ceil(B / kAltMaxParts) samples,  dW[j][k] = sum_b sum_n dY[b][n][j] V[b][n][k]
struct AltWgrad {
  const float* dy; int ld_dy; long dy_sl;
  const float* x; const float* const* x_tab; int ld_x;
  const VLayout* x_view;                 // (not NULL) x as the [B, N, n_in] view of the call's image features
  int rows, levels, n_out, n_in;
  float* dW0; float* dW1; int split;
};
int alt_wgrad(const AltWgrad& w, const AltCall& c) {
  float* part = c.ws + c.wo.part;
  const long mn = (long)w.n_out * w.n_in;
  // parts [batch] = dY_z^T X_z on the general GEMM; the caller adds how X and the contraction are walked
  auto part_job = [&](const float* dy, const float* x, float* out, int K, int batch) {
    coattn_gemm_desc g = {};
    g.A = dy; g.a_sm = 1; g.a_sk = w.ld_dy; g.B = x; g.C = out; g.c_sz = mn; g.c_sm = w.n_in; g.c_sn = 1;
    g.M = w.n_out; g.N = w.n_in; g.K = K; g.batch = batch;
    return g;
  };
  int parts;
  if (!alt_rows_of(w.x_view, w.ld_x, c.N, w.n_in).rows) {
    const int G = (c.B + kAltMaxParts - 1) / kAltMaxParts;
    parts = (c.B + G - 1) / G;
    coattn_gemm_desc g = part_job(w.dy, w.x, part, c.N, parts);
    g.a_si = (int64_t)c.N * w.ld_dy; g.a_sz = G * g.a_si;
    g.b_sk = w.x_view->sN; g.b_sn = w.x_view->sD; g.b_si = w.x_view->sB; g.b_sz = G * g.b_si;
    g.inner = G; g.inner_total = c.B;
    CA_TRY(launch_gemm_f32(g, c.s));
  } else {
    TnGemm t = {};
    t.A = w.dy; t.a_ld = w.ld_dy; t.a_sl = w.dy_sl;
    t.B = w.x; t.b_ld = w.ld_x;
    if (w.x_tab) for (int l = 0; l < w.levels; ++l) t.b_ptrs[l] = w.x_tab[l];
    t.C = part; t.M = w.n_out; t.N = w.n_in; t.K = w.rows; t.levels = w.levels; t.np = 3;
    if (gemm_tn_supported(t)) {
      int ks, S;
      parts = gemm_tn_plan(t, kAltMaxParts, &ks, &S);
      CA_TRY(launch_gemm_tn(&t, &ks, &S, 1, c.s));
    } else {
      const int per = (kAltMaxParts / w.levels) > 0 ? kAltMaxParts / w.levels : 1;
      int ks = (w.rows + per - 1) / per;
      ks = (ks + 15) / 16 * 16;
      const int S = (w.rows + ks - 1) / ks;
      for (int l = 0; l < w.levels; ++l) {
        coattn_gemm_desc g = part_job(w.dy + (long)l * w.dy_sl, w.x_tab ? w.x_tab[l] : w.x, part + (size_t)l * S * mn, w.rows, S);
        g.b_sk = w.ld_x; g.b_sn = 1; g.ksplit = ks;
        CA_TRY(launch_gemm_f32(g, c.s));
      }
      parts = w.levels * S;
    }
  }
  AltReduce r = {};
  r.accumulate = c.accumulate;
  alt_reduce_job(r, part, w.dW0, (long)w.split * w.n_in, mn, parts);
  if (w.dW1) alt_reduce_job(r, part + (size_t)w.split * w.n_in, w.dW1, (long)(w.n_out - w.split) * w.n_in, mn, parts);
  return launch_alt_reduce(r, c.s);
}
// a weight gradient of one level without a split: dW [n][n] (+)= dY^T X, both [rows][n] row-major (x_view NULL) or X the features
int alt_wgrad_square(const AltCall& c, const float* dy, const float* x, const VLayout* x_view, int rows, void* dW) {
  const AltWgrad w = {dy, c.d, 0, x, nullptr, c.d, x_view, rows, 1, c.d, c.d, (float*)dW, nullptr, c.d};
  return alt_wgrad(w, c);
}

template <int NLV>
int launch_guided(bool fwd, const GuidedArgs& a, hipStream_t s) {
  // every buffer the kernel writes or reads unconditionally must be there (a missing one is an argument error, not a fault)
  bool ok = a.x[0] && a.p && a.w && (NLV == 1 || a.L <= NLV);
  for (int l = 0; l < (NLV == 1 ? a.L : 1); ++l) ok = ok && a.x[l];
  ok = ok && (fwd ? (a.c && a.a && a.xhat) : (a.a_in && a.gx && a.dh && a.dw_part));
  CA_CHECK_ARG(ok, "alternating co-attention: internal error, a %s buffer of the guided step is missing", fwd ? "forward" : "backward");
  const dim3 grid(a.B, NLV == 1 ? a.L : 1);
  if (fwd) hipLaunchKernelGGL(guided_fwd_kernel<NLV>, grid, dim3(alt_threads<NLV>()), 0, s, a);
  else hipLaunchKernelGGL(guided_bwd_kernel<NLV>, grid, dim3(alt_threads<NLV>()), 0, s, a);
  CA_CHECK_LAUNCH(fwd ? "guided_fwd" : "guided_bwd");
  return 0;
}

// What the guided steps of a call share, forward and backward: steps 1 and 3 attend the question levels, their projections
// the halves of [X1 | X3] ...
GuidedArgs alt_q_side(const AltCall& c) {
  GuidedArgs q = {};
  for (int i = 0; i < c.L; ++i) q.x[i] = c.Q[i];
  q.x_sB = (long)c.T * c.d; q.x_sR = c.d; q.x_sD = 1;
  q.p_sL = (long)c.B * c.T * 2 * c.d; q.p_ld = 2 * c.d; q.len = c.qlen; q.B = c.B; q.R = c.T; q.d = c.d; q.L = c.L;
  return q;
}
// ... and step 2 the image features by their strides under the guide g2, every level of a sample against the same V and X2
GuidedArgs alt_v_side(const AltCall& c) {
  GuidedArgs a = {};
  for (int i = 0; i < kAltMaxL; ++i) a.x[i] = c.V;
  a.x_sB = c.vl.sB; a.x_sR = c.vl.sN; a.x_sD = c.vl.sD;
  a.p = c.sv + c.so.x2; a.p_sL = 0; a.p_ld = c.d; a.g = c.sv + c.so.g2; a.w = (const float*)c.p->w_h2;
  a.B = c.B; a.R = c.N; a.d = c.d; a.L = c.L;
  return a;
}

// ---- the forward's steps
int alt_fwd_projections(const AltCall& c) {
  const coattn_alt_params* p = c.p;
  const int d = c.d;
  float* wf = c.ws;
  // [X1 | X3] of every level: ONE projection against the stacked [W_x1; W_x3]
  CA_TRY(launch_concat_cols((const float*)p->W_x1, d * d, (const float*)p->W_x3, d * d, wf + c.fo.wcat, 1, c.s));
  CA_TRY(launch_concat_cols((const float*)p->b_x1, d, (const float*)p->b_x3, d, wf + c.fo.bcat, 1, c.s));
  AltLinear x13 = alt_rows_job(nullptr, wf + c.fo.wcat, false, wf + c.fo.bcat, c.st + c.so.x13, c.B * c.T, 2 * d, d, wf + c.fo.img13);
  x13.x_tab = c.Q; x13.y_sz = (long)c.B * c.T * 2 * d; x13.batch = c.L;
  CA_TRY(alt_linear(x13, c.s));
  // X2 = V W_x2^T + b_x2, once per sample (not per level)
  AltLinear x2 = alt_rows_job(c.V, (const float*)p->W_x2, false, (const float*)p->b_x2, c.st + c.so.x2, c.B * c.N, d, d, wf + c.fo.img2);
  x2.x_view = &c.vl; x2.n = c.N;
  return alt_linear(x2, c.s);
}
int alt_fwd_guided(const AltCall& c) {
  const coattn_alt_params* p = c.p;
  const int d = c.d, LB = c.L * c.B;
  float* sv = c.st;
  const AltSaved& so = c.so;
  // step 1: s^ = guided(Q, 0)
  GuidedArgs a1 = alt_q_side(c);
  a1.p = sv + so.x13; a1.w = (const float*)p->w_h1; a1.c = (const float*)p->c_h1; a1.a = sv + so.as; a1.xhat = sv + so.sh;
  CA_TRY(launch_guided<1>(true, a1, c.s));
  // step 2: v^ = guided(V, s^ W_g2^T + b_g2), the levels of a sample in one workgroup
  CA_TRY(alt_linear(alt_rows_job(sv + so.sh, (const float*)p->W_g2, false, (const float*)p->b_g2, sv + so.g2, LB, d, d,
                                 c.ws + c.fo.imgg2), c.s));
  GuidedArgs a2 = alt_v_side(c);
  a2.c = (const float*)p->c_h2;
  a2.a = c.av_out && !c.keep ? c.av_out : sv + so.av; a2.a2 = c.av_out && c.keep ? c.av_out : nullptr;
  a2.xhat = c.keep ? sv + so.vh : c.v_out;
  CA_TRY(launch_guided<kAltMaxL>(true, a2, c.s));
  const float* vh = a2.xhat;
  // step 3: q^ = guided(Q, v^ W_g3^T + b_g3)
  CA_TRY(alt_linear(alt_rows_job(vh, (const float*)p->W_g3, false, (const float*)p->b_g3, sv + so.g3, LB, d, d,
                                 c.ws + c.fo.imgg3), c.s));
  GuidedArgs a3 = alt_q_side(c);
  a3.p = sv + so.x13 + d; a3.g = sv + so.g3; a3.w = (const float*)p->w_h3; a3.c = (const float*)p->c_h3;
  a3.a = c.aq_out && !c.keep ? c.aq_out : sv + so.aq; a3.a2 = c.aq_out && c.keep ? c.aq_out : nullptr;
  a3.xhat = c.q_out;
  CA_TRY(launch_guided<1>(true, a3, c.s));
  if (c.keep && hipMemcpyAsync(c.v_out, vh, (size_t)LB * d * sizeof(float), hipMemcpyDeviceToDevice, c.s) != hipSuccess) {
    coattn_set_error("coattn_alt_forward: hipMemcpyAsync failed");
    return -3;
  }
  return 0;
}

// ---- the backward's steps
int alt_bwd_guided(const AltCall& c) {
  const coattn_alt_params* p = c.p;
  const int d = c.d, LB = c.L * c.B;
  const float* sv = c.sv;
  float* w = c.ws;
  const AltSaved& so = c.so;
  const AltBwdWs& wo = c.wo;
  GuidedArgs q = alt_q_side(c);
  q.dh_sL = q.p_sL; q.dh_ld = 2 * d;                    // [dH1 | dH3], laid out as [X1 | X3]
  // step 3: dH3 (into the right half of [dH1 | dH3]), dg3 = sum_t dH3
  GuidedArgs a3 = q;
  a3.p = sv + so.x13 + d; a3.g = sv + so.g3; a3.w = (const float*)p->w_h3; a3.a_in = sv + so.aq;
  a3.gx = c.gq; a3.ga = c.g_aq; a3.dh = w + wo.dh13 + d; a3.dg = w + wo.dg3; a3.dw_part = w + wo.wp3;
  CA_TRY(launch_guided<1>(false, a3, c.s));
  // gradient into v^: gv + dg3 W_g3 (the sum is formed by step 2's kernel)
  CA_TRY(alt_linear(alt_rows_job(w + wo.dg3, (const float*)p->W_g3, true, nullptr, w + wo.dvt, LB, d, d, w + wo.imgg3), c.s));
  // step 2: sum_l dH2_l into dX2, dg2 = sum_n dH2
  GuidedArgs a2 = alt_v_side(c);
  a2.a_in = sv + so.av; a2.gx = c.gv; a2.gx2 = w + wo.dvt; a2.gx_tot = w + wo.dvt; a2.ga = c.g_av;
  a2.dh = w + wo.dx2; a2.dh_ld = d; a2.dg = w + wo.dg2; a2.dw_part = w + wo.wp2;
  CA_TRY(launch_guided<kAltMaxL>(false, a2, c.s));
  // gradient into s^: dg2 W_g2
  CA_TRY(alt_linear(alt_rows_job(w + wo.dg2, (const float*)p->W_g2, true, nullptr, w + wo.dsh, LB, d, d, w + wo.imgg2), c.s));
  // step 1: dH1 (into the left half)
  GuidedArgs a1 = q;
  a1.p = sv + so.x13; a1.w = (const float*)p->w_h1; a1.a_in = sv + so.as;
  a1.gx = w + wo.dsh; a1.dh = w + wo.dh13; a1.dg = w + wo.dg1; a1.dw_part = w + wo.wp1;
  return launch_guided<1>(false, a1, c.s);
}
int alt_bwd_input_grads(const AltCall& c) {
  const coattn_alt_params* p = c.p;
  const int B = c.B, N = c.N, d = c.d, L = c.L;
  const long BT = (long)B * c.T;
  const float* sv = c.sv;
  float* w = c.ws;
  const AltBwdWs& wo = c.wo;
  // dQ_l = [dH1 | dH3]_l [W_x1; W_x3] (K = 2d) + the rank-1 terms of steps 1 and 3
  CA_TRY(launch_concat_cols((const float*)p->W_x1, d * d, (const float*)p->W_x3, d * d, w + wo.wcat, 1, c.s));
  AltLinear dq = alt_rows_job(w + wo.dh13, w + wo.wcat, true, nullptr, nullptr, (int)BT, d, 2 * d, w + wo.img13);
  dq.x_sz = BT * 2 * d; dq.y_tab = c.dQ; dq.batch = L;
  CA_TRY(alt_linear(dq, c.s));
  DqRank1 k = {};
  for (int l = 0; l < L; ++l) k.dq[l] = c.dQ[l];
  k.as = sv + c.so.as; k.gs = w + wo.dsh; k.aq = sv + c.so.aq; k.gq = c.gq; k.B = B; k.T = c.T; k.d = d;
  hipLaunchKernelGGL(alt_dq_rank1_kernel, dim3((unsigned)((BT * d + 255) / 256), L), dim3(256), 0, c.s, k);
  CA_CHECK_LAUNCH("alt_dq_rank1");
  if (!c.dV) return 0;
  // dV = dX2 W_x2 + sum_l a_v,l (x) gv^_l
  AltLinear dv = alt_rows_job(w + wo.dx2, (const float*)p->W_x2, true, nullptr, c.dV, B * N, d, d, w + wo.img2);
  dv.y_view = &c.dvl; dv.n = N;
  CA_TRY(alt_linear(dv, c.s));
  const DvRank1 r = {c.dV, c.dvl.sB, c.dvl.sN, c.dvl.sD, sv + c.so.av, w + wo.dvt, B, N, d, L};
  hipLaunchKernelGGL(alt_dv_rank1_kernel, dim3((unsigned)(((long)B * N * d + 255) / 256)), dim3(256), 0, c.s, r);
  CA_CHECK_LAUNCH("alt_dv_rank1");
  return 0;
}
int alt_bwd_param_grads(const AltCall& c) {
  const coattn_alt_param_grads* pg = c.pg;
  const int B = c.B, d = c.d, LB = c.L * c.B;
  float* w = c.ws;
  const AltBwdWs& wo = c.wo;
  const AltWgrad w13 = {w + wo.dh13, 2 * d, (long)B * c.T * 2 * d, nullptr, c.Q, d, nullptr, B * c.T, c.L, 2 * d, d,
                        (float*)pg->dW_x1, (float*)pg->dW_x3, d};
  CA_TRY(alt_wgrad(w13, c));
  CA_TRY(alt_wgrad_square(c, w + wo.dx2, c.V, &c.vl, B * c.N, pg->dW_x2));
  CA_TRY(alt_wgrad_square(c, w + wo.dg2, c.sv + c.so.sh, nullptr, LB, pg->dW_g2));
  CA_TRY(alt_wgrad_square(c, w + wo.dg3, c.sv + c.so.vh, nullptr, LB, pg->dW_g3));
  // w_h / c_h of the three steps (the per-workgroup partials [d + 1]) and the biases: b_x1 from the rows of dg1 = sum_t dH1;
  // b_x2, b_g2 both from the rows of dg2 = sum_n dH2, and b_x3, b_g3 from those of dg3 (each pair adds into the same
  // pre-activation, so their gradients are the same sum: no column-sum pass over dH)
  AltReduce r = {};
  r.accumulate = c.accumulate;
  const float* wp[3] = {w + wo.wp1, w + wo.wp2, w + wo.wp3};
  void* const dw[3] = {pg->dw_h1, pg->dw_h2, pg->dw_h3}, * const dc[3] = {pg->dc_h1, pg->dc_h2, pg->dc_h3};
  const int np[3] = {LB, B, LB};
  for (int i = 0; i < 3; ++i) {
    alt_reduce_job(r, wp[i], dw[i], d, d + 1, np[i]);
    alt_reduce_job(r, wp[i] + d, dc[i], 1, d + 1, np[i]);
  }
  alt_reduce_job(r, w + wo.dg2, pg->db_g2, d, d, LB);
  alt_reduce_job(r, w + wo.dg3, pg->db_g3, d, d, LB);
  alt_reduce_job(r, w + wo.dg1, pg->db_x1, d, d, LB);
  alt_reduce_job(r, w + wo.dg2, pg->db_x2, d, d, LB);
  alt_reduce_job(r, w + wo.dg3, pg->db_x3, d, d, LB);
  return launch_alt_reduce(r, c.s);
}

}  // namespace

extern "C" int coattn_alt_workspace_bytes(int B, int N, int T, int d, int L, int dtype, int flags, size_t* saved, size_t* ws_fwd,
                                          size_t* ws_bwd) {
  CA_TRY(alt_check(B, N, T, d, L, dtype, flags));
  const size_t sv = alt_saved(B, N, T, d, L).total;
  if (saved) *saved = sv * sizeof(float);
  if (ws_fwd) *ws_fwd = (sv + alt_fwd_ws(d).total) * sizeof(float);   // (room for the state itself when saved is NULL)
  if (ws_bwd) *ws_bwd = alt_bwd_ws(B, N, T, d, L).total * sizeof(float);
  return 0;
}

extern "C" int coattn_alt_forward(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q, const int32_t* q_len,
                                  const coattn_alt_params* p, void* v_out, void* q_out, void* av_out, void* aq_out, void* saved,
                                  void* ws, int B, int N, int T, int d, int L, int dtype, int flags, void* stream) {
  CA_TRY(alt_check(B, N, T, d, L, dtype, flags));
  AltCall c = alt_call(V, VLayout{v_sB, v_sN, v_sD}, Q, q_len, p, B, N, T, d, L, stream);
  CA_TRY(check_vlayout(c.vl, N, d, "coattn_alt_forward: V"));
  CA_TRY(alt_check_ptrs(c, "coattn_alt_forward", {{V, "V"}, {Q, "Q"}, {p, "p"}, {v_out, "v_out"}, {q_out, "q_out"}, {ws, "ws"}}));
  c.keep = saved != nullptr;
  c.st = (float*)(saved ? saved : ws); c.sv = c.st;
  c.ws = (float*)ws + (saved ? 0 : c.so.total);
  c.fo = alt_fwd_ws(d);
  c.v_out = (float*)v_out; c.q_out = (float*)q_out; c.av_out = (float*)av_out; c.aq_out = (float*)aq_out;
  CA_TRY(alt_fwd_projections(c));
  prof_mark(c.s, "alt_projections");
  CA_TRY(alt_fwd_guided(c));
  prof_mark(c.s, "alt_guided");
  return 0;
}

extern "C" int coattn_alt_backward(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q, const int32_t* q_len,
                                   const coattn_alt_params* p, const void* saved, const void* gv, const void* gq, const void* g_av,
                                   const void* g_aq, void* dV, int64_t dv_sB, int64_t dv_sN, int64_t dv_sD, void* const* dQ,
                                   const coattn_alt_param_grads* pg, int accumulate, void* ws, int B, int N, int T, int d, int L,
                                   int dtype, int flags, void* stream) {
  CA_TRY(alt_check(B, N, T, d, L, dtype, flags));
  AltCall c = alt_call(V, VLayout{v_sB, v_sN, v_sD}, Q, q_len, p, B, N, T, d, L, stream);
  c.dV = (float*)dV; c.dvl = VLayout{dv_sB, dv_sN, dv_sD}; c.dQ = (float* const*)dQ; c.pg = pg; c.accumulate = accumulate;
  CA_TRY(check_vlayout(c.vl, N, d, "coattn_alt_backward: V"));
  if (dV) CA_TRY(check_vlayout(c.dvl, N, d, "coattn_alt_backward: dV"));
  CA_TRY(alt_check_ptrs(c, "coattn_alt_backward", {{V, "V"}, {Q, "Q"}, {p, "p"}, {pg, "pg"}, {saved, "saved"}, {gv, "gv"}, {gq, "gq"},
                                                   {dQ, "dQ"}, {ws, "ws"}}));
  CA_CHECK_ARG(accumulate == 0 || accumulate == 1, "coattn_alt_backward: accumulate must be 0 or 1");
  c.sv = (const float*)saved; c.ws = (float*)ws; c.wo = alt_bwd_ws(B, N, T, d, L);
  c.gv = (const float*)gv; c.gq = (const float*)gq; c.g_av = (const float*)g_av; c.g_aq = (const float*)g_aq;
  CA_TRY(alt_bwd_guided(c));
  prof_mark(c.s, "alt_guided_bwd");
  CA_TRY(alt_bwd_input_grads(c));
  prof_mark(c.s, "alt_input_grads");
  CA_TRY(alt_bwd_param_grads(c));
  prof_mark(c.s, "alt_param_grads");
  return 0;
}
