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

namespace {

constexpr int kAltMaxL = 4;            // levels per call (the question hierarchy has 3)
constexpr int kAltMaxR = 512;          // rows per step: T and N
constexpr int kAltMaxD = 1024;         // hidden size
// threads per workgroup: 512 for steps 1 and 3 (one workgroup per sample and level), 1024 for step 2 (one per sample: B of them,
// fewer than the CUs at B = 160, so each takes all the waves it can)
template <int NLV> constexpr int alt_threads() { return NLV == 1 ? 512 : 1024; }

inline size_t al64(size_t n) { return (n + 63) & ~(size_t)63; }

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
struct AltFwdWs { size_t wcat, bcat, img13, img2, imgg2, imgg3, total; };    // floats, after the saved-sized block
AltFwdWs alt_fwd_ws(int d) {
  AltFwdWs w;
  size_t o = 0;
  const size_t img = al64(wsplit_bytes(d, d) / sizeof(float) + 1), img2d = al64(wsplit_bytes(2 * d, d) / sizeof(float) + 1);
  w.wcat = o; o += al64((size_t)2 * d * d);
  w.bcat = o; o += al64((size_t)2 * d);
  w.img13 = o; o += img2d;
  w.img2 = o; o += img;
  w.imgg2 = o; o += img;
  w.imgg3 = o; o += img;
  w.total = o;
  return w;
}
struct AltBwdWs { size_t dh13, dx2, dg1, dg2, dg3, dvt, dsh, wp1, wp2, wp3, part, wcat, img13, img2, imgg2, imgg3, total; };
constexpr int kAltMaxParts = 32;
AltBwdWs alt_bwd_ws(int B, int N, int T, int d, int L) {
  AltBwdWs w;
  size_t o = 0;
  const size_t img = al64(wsplit_bytes(d, d) / sizeof(float) + 1), img2d = al64(wsplit_bytes(d, 2 * d) / sizeof(float) + 1);
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
  w.img13 = o; o += img2d;
  w.img2 = o; o += img;
  w.imgg2 = o; o += img;
  w.imgg3 = o; o += img;
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
int alt_check_v(int64_t sB, int64_t sN, int64_t sD, int N, int d, const char* what) {
  CA_CHECK_ARG(sN > 0 && sD > 0 && sB > 0, "%s: strides must be positive (sB=%ld sN=%ld sD=%ld)", what, (long)sB, (long)sN, (long)sD);
  CA_CHECK_ARG((long)(N - 1) * sN + (long)(d - 1) * sD < sB, "%s: sample stride %ld is smaller than a sample's extent", what, (long)sB);
  return 0;
}

// y[z][m][:] = x[z][m][:] W^T + bias (M rows, x rows ld_x apart or the a_ptrs table) on the pre-split-weight kernel when it takes
// the shape (the weight image `img` written here), else on the general GEMM
struct Lin {
  const float* x; const float* x_ptrs[kAltMaxL]; long x_sz; int ld_x;
  const float* W; const float* bias; float* y; long y_sz; int ld_y;
  int M, N, K, batch;
};
int alt_linear(const Lin& l, void* img, hipStream_t s) {
  WGemm g = {};
  g.A = l.x; g.a_sz = l.x_sz; g.a_sm = l.ld_x;
  for (int t = 0; t < kAltMaxL; ++t) g.a_ptrs[t] = l.x_ptrs[t];
  g.Wf = img; g.C = l.y; g.c_sz = l.y_sz; g.c_sm = l.ld_y; g.bias_n = l.bias; g.out_scale = 1.f;
  g.M = l.M; g.N = l.N; g.K = l.K; g.batch = l.batch; g.np = 3;
  if (!l.x_ptrs[0] && l.batch == 1) g.a_sz = 0;
  if (gemm_w_supported(g) && (l.ld_y & 3) == 0 && !gemm_bf_supported(g)) {
    const WSplit job{l.W, img, l.N, l.K, 0, l.K, wimg_pieces(g), nullptr};
    CA_TRY(launch_wsplit(&job, 1, s));
    return launch_gemm_wx(&g, 1, s);
  }
  coattn_gemm_desc d = {};
  d.A = l.x; d.a_sz = l.x_sz; d.a_sm = l.ld_x; d.a_sk = 1;
  for (int t = 0; t < kAltMaxL; ++t) d.a_ptrs[t] = l.x_ptrs[t];
  d.B = l.W; d.b_sk = 1; d.b_sn = l.K;
  d.C = l.y; d.c_sz = l.y_sz; d.c_sm = l.ld_y; d.c_sn = 1; d.bias_n = l.bias;
  d.M = l.M; d.N = l.N; d.K = l.K; d.batch = l.batch;
  return launch_gemm_f32(d, s);
}

// y[m][:] = x[m][:] W (W [K][N] row-major: dx = dy W) -- the back-projections -- same dispatch
int alt_linear_t(const float* x, int ld_x, long x_sz, const float* W, float* const* y_ptrs, float* y, long y_sz, int M, int N, int K,
                 int batch, void* img, hipStream_t s) {
  WGemm g = {};
  g.A = x; g.a_sz = batch > 1 ? x_sz : 0; g.a_sm = ld_x;
  g.Wf = img; g.C = y; g.c_sz = y_sz; g.c_sm = N; g.out_scale = 1.f;
  if (y_ptrs) for (int t = 0; t < batch; ++t) g.c_ptrs[t] = y_ptrs[t];
  g.M = M; g.N = N; g.K = K; g.batch = batch; g.np = 3;
  if (gemm_w_supported(g) && !gemm_bf_supported(g)) {
    const WSplit job{W, img, N, K, 1, N, wimg_pieces(g), nullptr};
    CA_TRY(launch_wsplit(&job, 1, s));
    return launch_gemm_wx(&g, 1, s);
  }
  coattn_gemm_desc d = {};
  d.A = x; d.a_sz = x_sz; d.a_sm = ld_x; d.a_sk = 1;
  d.B = W; d.b_sk = N; d.b_sn = 1;
  d.C = y; d.c_sz = y_sz; d.c_sm = N; d.c_sn = 1;
  if (y_ptrs) for (int t = 0; t < batch; ++t) d.c_ptrs[t] = y_ptrs[t];
  d.M = M; d.N = N; d.K = K; d.batch = batch;
  return launch_gemm_f32(d, s);
}

int launch_alt_reduce(const AltReduce& r, hipStream_t s) {
  long nmax = 0;
  for (int i = 0; i < r.njobs; ++i) nmax = r.n[i] > nmax ? r.n[i] : nmax;
  hipLaunchKernelGGL(alt_reduce_kernel, dim3((unsigned)((nmax + 63) / 64), r.njobs), dim3(256), 0, s, r);
  CA_CHECK_LAUNCH("alt_reduce");
  return 0;
}

// dW (+)= sum over rows of dY^T X, dY rows [rows][n_out] (ld_dy), X rows [rows][n_in] (ld_x) per level (x_ptrs) or once;
// the [n_out][n_in] result may be split by rows into dW0 (rows < split) and dW1.  Split-K parts + a fixed-order reduce.
int alt_wgrad(const float* dy, int ld_dy, long dy_sl, const float* const* x_ptrs, const float* x, int ld_x, int rows, int levels,
              int n_out, int n_in, float* dW0, float* dW1, int split, int accumulate, float* part, hipStream_t s) {
  TnGemm t = {};
  t.A = dy; t.a_ld = ld_dy; t.a_sl = dy_sl;
  t.B = x; t.b_ld = ld_x;
  if (x_ptrs) for (int l = 0; l < levels; ++l) t.b_ptrs[l] = x_ptrs[l];
  t.C = part; t.M = n_out; t.N = n_in; t.K = rows; t.levels = levels; t.np = 3;
  int parts;
  if (gemm_tn_supported(t)) {
    int ks, S;
    parts = gemm_tn_plan(t, kAltMaxParts, &ks, &S);
    CA_TRY(launch_gemm_tn(&t, &ks, &S, 1, s));
  } else {
    const int per = (kAltMaxParts / levels) > 0 ? kAltMaxParts / levels : 1;
    int ks = (rows + per - 1) / per;
    ks = (ks + 15) / 16 * 16;
    const int S = (rows + ks - 1) / ks;
    for (int l = 0; l < levels; ++l) {
      coattn_gemm_desc g = {};
      g.A = dy + (long)l * dy_sl; g.a_sm = 1; g.a_sk = ld_dy;
      g.B = x_ptrs ? x_ptrs[l] : x; g.b_sk = ld_x; g.b_sn = 1;
      g.C = part + (size_t)l * S * n_out * n_in; g.c_sz = (int64_t)n_out * n_in; g.c_sm = n_in; g.c_sn = 1;
      g.M = n_out; g.N = n_in; g.K = rows; g.batch = S; g.ksplit = ks;
      CA_TRY(launch_gemm_f32(g, s));
    }
    parts = levels * S;
  }
  AltReduce r = {};
  r.accumulate = accumulate;
  r.src[0] = part; r.dst[0] = dW0; r.n[0] = (long)split * n_in; r.ld[0] = (long)n_out * n_in; r.nparts[0] = parts;
  r.njobs = 1;
  if (dW1) {
    r.src[1] = part + (size_t)split * n_in; r.dst[1] = dW1; r.n[1] = (long)(n_out - split) * n_in; r.ld[1] = r.ld[0];
    r.nparts[1] = parts; r.njobs = 2;
  }
  return launch_alt_reduce(r, s);
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
  CA_TRY(alt_check_v(v_sB, v_sN, v_sD, N, d, "coattn_alt_forward: V"));
  {
    const struct { const void* ptr; const char* name; } req[] = {{V, "V"}, {Q, "Q"}, {p, "p"}, {v_out, "v_out"}, {q_out, "q_out"}, {ws, "ws"}};
    for (const auto& a : req) CA_CHECK_ARG(a.ptr, "coattn_alt_forward: %s is NULL", a.name);
  }
  for (int l = 0; l < L; ++l) CA_CHECK_ARG(Q[l], "coattn_alt_forward: Q[%d] is NULL", l);
  const void* const* pp = (const void* const*)p;
  for (int i = 0; i < 16; ++i) CA_CHECK_ARG(pp[i], "coattn_alt_forward: parameter %d is NULL", i);
  hipStream_t s = (hipStream_t)stream;
  const AltSaved so = alt_saved(B, N, T, d, L);
  float* sv = saved ? (float*)saved : (float*)ws;
  float* wf = (float*)ws + (saved ? 0 : so.total);
  const AltFwdWs fo = alt_fwd_ws(d);
  const float* const* Qf = (const float* const*)Q;
  const long BT = (long)B * T, Bd = (long)B * d;
  // [X1 | X3] of every level: ONE projection against the stacked [W_x1; W_x3]
  CA_TRY(launch_concat_cols((const float*)p->W_x1, d * d, (const float*)p->W_x3, d * d, wf + fo.wcat, 1, s));
  CA_TRY(launch_concat_cols((const float*)p->b_x1, d, (const float*)p->b_x3, d, wf + fo.bcat, 1, s));
  {
    Lin l = {};
    for (int i = 0; i < L; ++i) l.x_ptrs[i] = Qf[i];
    l.ld_x = d; l.W = wf + fo.wcat; l.bias = wf + fo.bcat; l.y = sv + so.x13; l.y_sz = BT * 2 * d; l.ld_y = 2 * d;
    l.M = (int)BT; l.N = 2 * d; l.K = d; l.batch = L;
    CA_TRY(alt_linear(l, wf + fo.img13, s));
  }
  // X2 = V W_x2^T + b_x2, once per sample (not per level)
  const bool v_rows = v_sD == 1 && v_sN == d && v_sB == (int64_t)N * d;
  if (v_rows) {
    Lin l = {};
    l.x = (const float*)V; l.ld_x = d; l.W = (const float*)p->W_x2; l.bias = (const float*)p->b_x2; l.y = sv + so.x2; l.ld_y = d;
    l.M = B * N; l.N = d; l.K = d; l.batch = 1;
    CA_TRY(alt_linear(l, wf + fo.img2, s));
  } else {
    WGemm g = {};               // channel-major V: A contiguous along m (the pre-split-weight kernel's a_sk form)
    g.A = (const float*)V; g.a_sk = (int)v_sD; g.a_mdiv = N; g.a_sdiv = v_sB; g.Wf = wf + fo.img2; g.C = sv + so.x2; g.c_sm = d;
    g.bias_n = (const float*)p->b_x2; g.out_scale = 1.f; g.M = B * N; g.N = d; g.K = d; g.batch = 1; g.np = 3;
    if (v_sN == 1 && v_sD < (1L << 30) && v_sB < (1L << 40) && gemm_w_supported(g) && !gemm_bf_supported(g)) {
      const WSplit job{(const float*)p->W_x2, wf + fo.img2, d, d, 0, d, wimg_pieces(g), nullptr};
      CA_TRY(launch_wsplit(&job, 1, s));
      CA_TRY(launch_gemm_wx(&g, 1, s));
    } else {
      coattn_gemm_desc c = {};
      c.A = (const float*)V; c.a_sm = v_sN; c.a_sk = v_sD;
      if (v_sB != (int64_t)N * v_sN) { c.a_mdiv = N; c.a_sdiv = v_sB; }
      c.B = (const float*)p->W_x2; c.b_sk = 1; c.b_sn = d; c.C = sv + so.x2; c.c_sm = d; c.c_sn = 1; c.bias_n = (const float*)p->b_x2;
      c.M = B * N; c.N = d; c.K = d; c.batch = 1;
      CA_TRY(launch_gemm_f32(c, s));
    }
  }
  prof_mark(s, "alt_projections");
  GuidedArgs q = {};
  for (int i = 0; i < L; ++i) q.x[i] = Qf[i];
  q.x_sB = (long)T * d; q.x_sR = d; q.x_sD = 1;
  q.p_sL = BT * 2 * d; q.p_ld = 2 * d; q.len = q_len; q.B = B; q.R = T; q.d = d; q.L = L;
  // step 1: s^ = guided(Q, 0)
  GuidedArgs a1 = q;
  a1.p = sv + so.x13; a1.w = (const float*)p->w_h1; a1.c = (const float*)p->c_h1; a1.a = sv + so.as; a1.xhat = sv + so.sh;
  CA_TRY(launch_guided<1>(true, a1, s));
  // step 2: v^ = guided(V, s^ W_g2^T + b_g2), the levels of a sample in one workgroup
  {
    Lin l = {};
    l.x = sv + so.sh; l.ld_x = d; l.W = (const float*)p->W_g2; l.bias = (const float*)p->b_g2; l.y = sv + so.g2; l.ld_y = d;
    l.M = L * B; l.N = d; l.K = d; l.batch = 1;
    CA_TRY(alt_linear(l, wf + fo.imgg2, s));
  }
  GuidedArgs a2 = {};
  for (int i = 0; i < kAltMaxL; ++i) a2.x[i] = (const float*)V;
  a2.x_sB = v_sB; a2.x_sR = v_sN; a2.x_sD = v_sD;
  a2.p = sv + so.x2; a2.p_sL = 0; a2.p_ld = d; a2.g = sv + so.g2; a2.w = (const float*)p->w_h2; a2.c = (const float*)p->c_h2;
  a2.B = B; a2.R = N; a2.d = d; a2.L = L;
  a2.a = av_out && !saved ? (float*)av_out : sv + so.av; a2.a2 = av_out && saved ? (float*)av_out : nullptr;
  a2.xhat = saved ? sv + so.vh : (float*)v_out;
  CA_TRY(launch_guided<kAltMaxL>(true, a2, s));
  const float* vh = a2.xhat;
  // step 3: q^ = guided(Q, v^ W_g3^T + b_g3)
  {
    Lin l = {};
    l.x = vh; l.ld_x = d; l.W = (const float*)p->W_g3; l.bias = (const float*)p->b_g3; l.y = sv + so.g3; l.ld_y = d;
    l.M = L * B; l.N = d; l.K = d; l.batch = 1;
    CA_TRY(alt_linear(l, wf + fo.imgg3, s));
  }
  GuidedArgs a3 = q;
  a3.p = sv + so.x13 + d; a3.g = sv + so.g3; a3.w = (const float*)p->w_h3; a3.c = (const float*)p->c_h3;
  a3.a = aq_out && !saved ? (float*)aq_out : sv + so.aq; a3.a2 = aq_out && saved ? (float*)aq_out : nullptr;
  a3.xhat = (float*)q_out;
  CA_TRY(launch_guided<1>(true, a3, s));
  if (saved && hipMemcpyAsync(v_out, vh, (size_t)L * Bd * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
    coattn_set_error("coattn_alt_forward: hipMemcpyAsync failed");
    return -3;
  }
  prof_mark(s, "alt_guided");
  return 0;
}

extern "C" int coattn_alt_backward(const void* V, int64_t v_sB, int64_t v_sN, int64_t v_sD, const void* const* Q, const int32_t* q_len,
                                   const coattn_alt_params* p, const void* saved, const void* gv, const void* gq, const void* g_av,
                                   const void* g_aq, void* dV, int64_t dv_sB, int64_t dv_sN, int64_t dv_sD, void* const* dQ,
                                   const coattn_alt_param_grads* pg, int accumulate, void* ws, int B, int N, int T, int d, int L,
                                   int dtype, int flags, void* stream) {
  CA_TRY(alt_check(B, N, T, d, L, dtype, flags));
  CA_TRY(alt_check_v(v_sB, v_sN, v_sD, N, d, "coattn_alt_backward: V"));
  if (dV) CA_TRY(alt_check_v(dv_sB, dv_sN, dv_sD, N, d, "coattn_alt_backward: dV"));
  {
    const struct { const void* ptr; const char* name; } req[] = {{V, "V"}, {Q, "Q"}, {p, "p"}, {pg, "pg"}, {saved, "saved"}, {gv, "gv"},
                                                                 {gq, "gq"}, {dQ, "dQ"}, {ws, "ws"}};
    for (const auto& a : req) CA_CHECK_ARG(a.ptr, "coattn_alt_backward: %s is NULL", a.name);
  }
  for (int l = 0; l < L; ++l) CA_CHECK_ARG(Q[l] && dQ[l], "coattn_alt_backward: Q[%d] / dQ[%d] is NULL", l, l);
  const void* const* pp = (const void* const*)p;
  void* const* gp = (void* const*)pg;
  for (int i = 0; i < 16; ++i) CA_CHECK_ARG(pp[i] && gp[i], "coattn_alt_backward: parameter or gradient %d is NULL", i);
  CA_CHECK_ARG(accumulate == 0 || accumulate == 1, "coattn_alt_backward: accumulate must be 0 or 1");
  hipStream_t s = (hipStream_t)stream;
  const AltSaved so = alt_saved(B, N, T, d, L);
  const AltBwdWs wo = alt_bwd_ws(B, N, T, d, L);
  const float* sv = (const float*)saved;
  float* w = (float*)ws;
  const float* const* Qf = (const float* const*)Q;
  const long BT = (long)B * T;
  GuidedArgs q = {};
  for (int i = 0; i < L; ++i) q.x[i] = Qf[i];
  q.x_sB = (long)T * d; q.x_sR = d; q.x_sD = 1;
  q.p_sL = BT * 2 * d; q.p_ld = 2 * d; q.len = q_len; q.B = B; q.R = T; q.d = d; q.L = L;
  q.dh_sL = BT * 2 * d; q.dh_ld = 2 * d;
  // step 3: dH3 (into the right half of [dH1 | dH3]), dg3 = sum_t dH3
  GuidedArgs a3 = q;
  a3.p = sv + so.x13 + d; a3.g = sv + so.g3; a3.w = (const float*)p->w_h3; a3.a_in = sv + so.aq;
  a3.gx = (const float*)gq; a3.ga = (const float*)g_aq; a3.dh = w + wo.dh13 + d; a3.dg = w + wo.dg3; a3.dw_part = w + wo.wp3;
  CA_TRY(launch_guided<1>(false, a3, s));
  // gradient into v^: gv + dg3 W_g3 (the sum is formed by step 2's kernel)
  CA_TRY(alt_linear_t(w + wo.dg3, d, 0, (const float*)p->W_g3, nullptr, w + wo.dvt, 0, L * B, d, d, 1, w + wo.imgg3, s));
  // step 2: sum_l dH2_l into dX2, dg2 = sum_n dH2
  GuidedArgs a2 = {};
  for (int i = 0; i < kAltMaxL; ++i) a2.x[i] = (const float*)V;
  a2.x_sB = v_sB; a2.x_sR = v_sN; a2.x_sD = v_sD;
  a2.p = sv + so.x2; a2.p_ld = d; a2.g = sv + so.g2; a2.w = (const float*)p->w_h2; a2.a_in = sv + so.av;
  a2.B = B; a2.R = N; a2.d = d; a2.L = L;
  a2.gx = (const float*)gv; a2.gx2 = w + wo.dvt; a2.gx_tot = w + wo.dvt; a2.ga = (const float*)g_av;
  a2.dh = w + wo.dx2; a2.dh_ld = d; a2.dg = w + wo.dg2; a2.dw_part = w + wo.wp2;
  CA_TRY(launch_guided<kAltMaxL>(false, a2, s));
  // gradient into s^: dg2 W_g2
  CA_TRY(alt_linear_t(w + wo.dg2, d, 0, (const float*)p->W_g2, nullptr, w + wo.dsh, 0, L * B, d, d, 1, w + wo.imgg2, s));
  // step 1: dH1 (into the left half)
  GuidedArgs a1 = q;
  a1.p = sv + so.x13; a1.w = (const float*)p->w_h1; a1.a_in = sv + so.as;
  a1.gx = w + wo.dsh; a1.dh = w + wo.dh13; a1.dg = w + wo.dg1; a1.dw_part = w + wo.wp1;
  CA_TRY(launch_guided<1>(false, a1, s));
  prof_mark(s, "alt_guided_bwd");
  // dQ_l = [dH1 | dH3]_l [W_x1; W_x3] (K = 2d) + the rank-1 terms of steps 1 and 3
  CA_TRY(launch_concat_cols((const float*)p->W_x1, d * d, (const float*)p->W_x3, d * d, w + wo.wcat, 1, s));
  {
    float* yp[kAltMaxL] = {};
    for (int l = 0; l < L; ++l) yp[l] = (float*)dQ[l];
    CA_TRY(alt_linear_t(w + wo.dh13, 2 * d, BT * 2 * d, w + wo.wcat, yp, nullptr, 0, (int)BT, d, 2 * d, L, w + wo.img13, s));
    DqRank1 k = {};
    for (int l = 0; l < L; ++l) k.dq[l] = (float*)dQ[l];
    k.as = sv + so.as; k.gs = w + wo.dsh; k.aq = sv + so.aq; k.gq = (const float*)gq; k.B = B; k.T = T; k.d = d;
    hipLaunchKernelGGL(alt_dq_rank1_kernel, dim3((unsigned)((BT * d + 255) / 256), L), dim3(256), 0, s, k);
    CA_CHECK_LAUNCH("alt_dq_rank1");
  }
  // dV = dX2 W_x2 + sum_l a_v,l (x) gv^_l
  if (dV) {
    const bool lm = dv_sD == 1 && dv_sN == d && dv_sB == (int64_t)N * d;
    if (lm) {
      CA_TRY(alt_linear_t(w + wo.dx2, d, 0, (const float*)p->W_x2, nullptr, (float*)dV, 0, B * N, d, d, 1, w + wo.img2, s));
    } else {
      coattn_gemm_desc g = {};
      g.A = w + wo.dx2; g.a_sm = d; g.a_sk = 1;
      g.B = (const float*)p->W_x2; g.b_sk = d; g.b_sn = 1;
      g.C = (float*)dV; g.c_sm = dv_sN; g.c_sn = dv_sD;
      if (dv_sB != (int64_t)N * dv_sN) { g.c_mdiv = N; g.c_sdiv = dv_sB; }
      g.M = B * N; g.N = d; g.K = d; g.batch = 1;
      CA_TRY(launch_gemm_f32(g, s));
    }
    DvRank1 k = {(float*)dV, (long)dv_sB, (long)dv_sN, (long)dv_sD, sv + so.av, w + wo.dvt, B, N, d, L};
    hipLaunchKernelGGL(alt_dv_rank1_kernel, dim3((unsigned)(((long)B * N * d + 255) / 256)), dim3(256), 0, s, k);
    CA_CHECK_LAUNCH("alt_dv_rank1");
  }
  prof_mark(s, "alt_input_grads");
  // parameter gradients
  float* part = w + wo.part;
  CA_TRY(alt_wgrad(w + wo.dh13, 2 * d, BT * 2 * d, Qf, nullptr, d, (int)BT, L, 2 * d, d, (float*)pg->dW_x1, (float*)pg->dW_x3, d,
                   accumulate, part, s));
  const bool v_rows = v_sD == 1 && v_sN == d && v_sB == (int64_t)N * d;
  if (v_rows) {
    CA_TRY(alt_wgrad(w + wo.dx2, d, 0, nullptr, (const float*)V, d, B * N, 1, d, d, (float*)pg->dW_x2, nullptr, d, accumulate, part, s));
  } else {
    // dW_x2[j][k] = sum_b sum_n dX2[b][n][j] V[b][n][k] over groups of samples (strided V)
    const int G = (B + kAltMaxParts - 1) / kAltMaxParts, S = (B + G - 1) / G;
    coattn_gemm_desc g = {};
    g.A = w + wo.dx2; g.a_sm = 1; g.a_sk = d; g.a_si = (int64_t)N * d; g.a_sz = (int64_t)G * N * d;
    g.B = (const float*)V; g.b_sk = v_sN; g.b_sn = v_sD; g.b_si = v_sB; g.b_sz = (int64_t)G * v_sB;
    g.C = part; g.c_sz = (int64_t)d * d; g.c_sm = d; g.c_sn = 1;
    g.M = d; g.N = d; g.K = N; g.batch = S; g.inner = G; g.inner_total = B;
    CA_TRY(launch_gemm_f32(g, s));
    AltReduce r = {};
    r.src[0] = part; r.dst[0] = (float*)pg->dW_x2; r.n[0] = (long)d * d; r.ld[0] = (long)d * d; r.nparts[0] = S; r.njobs = 1;
    r.accumulate = accumulate;
    CA_TRY(launch_alt_reduce(r, s));
  }
  CA_TRY(alt_wgrad(w + wo.dg2, d, 0, nullptr, sv + so.sh, d, L * B, 1, d, d, (float*)pg->dW_g2, nullptr, d, accumulate, part, s));
  CA_TRY(alt_wgrad(w + wo.dg3, d, 0, nullptr, sv + so.vh, d, L * B, 1, d, d, (float*)pg->dW_g3, nullptr, d, accumulate, part, s));
  {
    // w_h / c_h of the three steps (the per-workgroup partials [d + 1]) and the biases: b_x1 from the rows of dg1 = sum_t dH1;
    // b_x2, b_g2 both from the rows of dg2 = sum_n dH2, and b_x3, b_g3 from those of dg3 (each pair adds into the same
    // pre-activation, so their gradients are the same sum: no column-sum pass over dH)
    AltReduce r = {};
    r.accumulate = accumulate;
    const float* wp[3] = {w + wo.wp1, w + wo.wp2, w + wo.wp3};
    float* dw[3] = {(float*)pg->dw_h1, (float*)pg->dw_h2, (float*)pg->dw_h3};
    float* dc[3] = {(float*)pg->dc_h1, (float*)pg->dc_h2, (float*)pg->dc_h3};
    const int np[3] = {L * B, B, L * B};
    for (int i = 0; i < 3; ++i) {
      r.src[2 * i] = wp[i]; r.dst[2 * i] = dw[i]; r.n[2 * i] = d; r.ld[2 * i] = d + 1; r.nparts[2 * i] = np[i];
      r.src[2 * i + 1] = wp[i] + d; r.dst[2 * i + 1] = dc[i]; r.n[2 * i + 1] = 1; r.ld[2 * i + 1] = d + 1; r.nparts[2 * i + 1] = np[i];
    }
    r.src[6] = w + wo.dg2; r.dst[6] = (float*)pg->db_g2; r.n[6] = d; r.ld[6] = d; r.nparts[6] = L * B;
    r.src[7] = w + wo.dg3; r.dst[7] = (float*)pg->db_g3; r.n[7] = d; r.ld[7] = d; r.nparts[7] = L * B;
    const float* dgs[3] = {w + wo.dg1, w + wo.dg2, w + wo.dg3};
    float* dbx[3] = {(float*)pg->db_x1, (float*)pg->db_x2, (float*)pg->db_x3};
    for (int i = 0; i < 3; ++i) {
      r.src[8 + i] = dgs[i]; r.dst[8 + i] = dbx[i]; r.n[8 + i] = d; r.ld[8 + i] = d; r.nparts[8 + i] = L * B;
    }
    r.njobs = 11;
    CA_TRY(launch_alt_reduce(r, s));
  }
  prof_mark(s, "alt_param_grads");
  return 0;
}
