// The memory-bound glue between the convolutions of the frozen VGG encoder on gfx950 (reference model.py:239-241: the
// encoder is frozen but never put in eval mode, so every step normalises with fresh BATCH statistics): train-mode
// BatchNorm2d + ReLU + an optional 2x2 / stride-2 MaxPool2d, fp32, channels_last, forward only.  The stock chain reads the
// convolution output three to four times (mean/variance, normalise, pool, ReLU); here it is read twice and the pooled
// (or unpooled) result written once.  Three launches per layer on the caller's stream, no atomics, no grid barriers:
//
//   bn_stats_partial_kernel   a flat stream of 16-byte loads over x.  Physically x is [B][H][W][C], so an element's channel is
//                             its index mod C, and a thread whose stride through the tensor is a multiple of C / 4 keeps
//                             its four channels: workgroups of 256 threads do for every supported C (C / 4 divides 256).
//                             Sum and sum of squares are accumulated in DOUBLE (the pass is HBM-bound; the conversions and
//                             adds hide behind eight loads in flight per thread): no E[x^2] - mean^2 cancellation and no
//                             8-million-term fp32 sum.  One LDS tree per workgroup in a fixed order, one [C][2] double
//                             partial per workgroup.
//   bn_finalize_kernel        one workgroup per four channels adds the partials in a fixed order (64 interleaved lanes, then an
//                             LDS tree), leaves mean (as an fp32 pair hi + lo), scale = gamma / sqrt(var + eps) and the
//                             biased variance in the workspace and updates the running statistics; a frozen convolution
//                             bias the caller left out of x is added to the running mean here (it cancels everywhere else).
//   bn_relu_pool_kernel<POOL> t = ((x - mean_hi) - mean_lo) * scale + beta per element -- the subtract-mean form: the
//                             rounding error is proportional to the result, not to mean * scale --, the maximum of the four
//                             t of a 2x2 window (gamma may be negative: the affine map goes first), then ReLU.  NaN
//                             propagates as in PyTorch.  Floor mode: Ho = H / 2, Wo = W / 2, an odd last row / column is
//                             never read.  16-byte accesses along C, 64-bit offsets.
//
// Traffic per layer of S bytes: S (statistics) + S (normalise) + S/4 or S written, plus the partials (32 bytes per channel
// and statistics workgroup, held below ~2 % of S by the grid size).
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxStatBlocks = 2048;
// a statistics workgroup writes 16 B per channel and the finalize pass reads them back; a pixel is 4 B per channel: one
// workgroup per >= 400 pixels keeps the partials at <= 2 % of the layer
constexpr int kPixelsPerStatBlock = 400;
constexpr int kMaxNormBlocks = 4096;
constexpr int kStatLoads = 8;           // 16-byte loads in flight per thread of the statistics pass

typedef double f64x2 __attribute__((ext_vector_type(2)));

inline int stat_blocks(int64_t pixels) {
  const int64_t g = pixels / kPixelsPerStatBlock;
  return g < 1 ? 1 : g > kMaxStatBlocks ? kMaxStatBlocks : (int)g;
}

// workspace: [G][C] double pairs (sum, sum of squares), then fp32 mean_hi[C], mean_lo[C], scale[C], var_biased[C]
inline size_t partial_bytes(int G, int C) { return (size_t)G * C * sizeof(f64x2); }

// `c4` = C / 4 (a power of two, 4 .. 128).  partial[(block * C + c)] = (sum, sum of squares) of channel c over this block's share.
__global__ __launch_bounds__(kThreads) void bn_stats_partial_kernel(const f32x4* __restrict__ x, f64x2* __restrict__ partial,
                                                                    int64_t total4, int c4) {
  __shared__ double sh[8][kThreads];
  const int tid = threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kThreads;            // a multiple of c4: the thread keeps its channels
  int64_t i = (int64_t)blockIdx.x * kThreads + tid;
  double acc[8];                                                    // acc[2 e] = sum, acc[2 e + 1] = sum of squares of channel e
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.0;
  for (; i + (kStatLoads - 1) * stride < total4; i += kStatLoads * stride) {
    f32x4 v[kStatLoads];
#pragma unroll
    for (int u = 0; u < kStatLoads; ++u) v[u] = x[i + u * stride];
#pragma unroll
    for (int u = 0; u < kStatLoads; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double d = (double)v[u][e];
        acc[2 * e] += d;
        acc[2 * e + 1] = fma(d, d, acc[2 * e + 1]);
      }
  }
  for (; i < total4; i += stride) {
    const f32x4 v = x[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d = (double)v[e];
      acc[2 * e] += d;
      acc[2 * e + 1] = fma(d, d, acc[2 * e + 1]);
    }
  }
  // threads tid, tid + c4, tid + 2 c4, ... hold the same channels: halve down to c4 threads, always (t) + (t + w)
#pragma unroll
  for (int k = 0; k < 8; ++k) sh[k][tid] = acc[k];
  for (int w = kThreads / 2; w >= c4; w >>= 1) {
    __syncthreads();
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        acc[k] += sh[k][tid + w];
        sh[k][tid] = acc[k];
      }
    }
  }
  if (tid < c4) {
    f64x2* out = partial + ((int64_t)blockIdx.x * c4 + tid) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = f64x2{acc[2 * e], acc[2 * e + 1]};
  }
}

// One workgroup per four channels: thread t takes channel 4 blockIdx.x + (t & 3) and the partials (t >> 2) + 64 j.
__global__ __launch_bounds__(kThreads) void bn_finalize_kernel(const f64x2* __restrict__ partial, int G, int C, double count,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ conv_bias, float* running_mean,
                                                               float* running_var, double momentum, double eps,
                                                               float* __restrict__ ws_f, float* __restrict__ stats_out) {
  __shared__ double sh[2][kThreads];
  const int tid = threadIdx.x;
  const int c = 4 * blockIdx.x + (tid & 3);
  double s = 0.0, q = 0.0;
#pragma unroll 4
  for (int g = tid >> 2; g < G; g += kThreads / 4) {
    const f64x2 p = partial[(int64_t)g * C + c];
    s += p.x;
    q += p.y;
  }
  sh[0][tid] = s;
  sh[1][tid] = q;
  for (int w = kThreads / 2; w >= 4; w >>= 1) {
    __syncthreads();
    if (tid < w) {
      s += sh[0][tid + w];
      q += sh[1][tid + w];
      sh[0][tid] = s;
      sh[1][tid] = q;
    }
  }
  if (tid >= 4) return;
  const double mean = s / count;
  double var = q / count - mean * mean;
  var = var < 0.0 ? 0.0 : var;                          // (a NaN stays a NaN; a constant channel gives 0: scale = gamma / sqrt(eps))
  const float mean_hi = (float)mean;
  ws_f[c] = mean_hi;
  ws_f[C + c] = (float)(mean - (double)mean_hi);
  ws_f[2 * C + c] = (float)((double)gamma[c] / sqrt(var + eps));
  ws_f[3 * C + c] = (float)var;
  const double bias = conv_bias ? (double)conv_bias[c] : 0.0;
  running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * (mean + bias));
  running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var * (count / (count - 1.0))));
  if (stats_out) {
    stats_out[c] = mean_hi;
    stats_out[C + c] = (float)var;
  }
}

struct Affine {
  float mean[4], lo[4], scale[4], beta[4];
};

__device__ __forceinline__ f32x4 affine(const f32x4 v, const Affine& a) {
  f32x4 t;
#pragma unroll
  for (int e = 0; e < 4; ++e) t[e] = fmaf((v[e] - a.mean[e]) - a.lo[e], a.scale[e], a.beta[e]);
  return t;
}
// PyTorch's maximum: a NaN wins
__device__ __forceinline__ f32x4 max_nan(const f32x4 a, const f32x4 b) {
  f32x4 m;
#pragma unroll
  for (int e = 0; e < 4; ++e) m[e] = (a[e] > b[e] || a[e] != a[e]) ? a[e] : b[e];
  return m;
}
__device__ __forceinline__ f32x4 relu_nan(const f32x4 a) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = a[e] < 0.f ? 0.f : a[e];       // (a NaN is not < 0: it stays)
  return r;
}

// One thread per 16 bytes of output: o = output pixel * c4 + channel group.  total4 = output pixels * c4; H, W: the INPUT's.
// AFFINE = false: the 2x2 maximum and the ReLU alone (ws_f, beta not read): max and ReLU are exact, so the result has the bits of
// max_pool2d followed by relu.
template <bool POOL, bool AFFINE = true>
__global__ __launch_bounds__(kThreads) void bn_relu_pool_kernel(const f32x4* __restrict__ x, const float* __restrict__ ws_f,
                                                                const float* __restrict__ beta, f32x4* __restrict__ y,
                                                                int H, int W, int C, int c4_shift, int64_t total4, int relu) {
  const int tid = threadIdx.x;
  const int c4 = C >> 2;
  const int cg = tid & (c4 - 1);                                    // (block starts and the grid stride are multiples of c4)
  Affine a;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a.mean[e] = AFFINE ? ws_f[4 * cg + e] : 0.f;
    a.lo[e] = AFFINE ? ws_f[C + 4 * cg + e] : 0.f;
    a.scale[e] = AFFINE ? ws_f[2 * C + 4 * cg + e] : 1.f;
    a.beta[e] = AFFINE ? beta[4 * cg + e] : 0.f;
  }
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  int64_t o = (int64_t)blockIdx.x * kThreads + tid;
  if (!POOL) {
    for (; o < total4; o += 4 * stride) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (o + u * stride < total4) v[u] = x[o + u * stride];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (o + u * stride < total4) {
          const f32x4 t = affine(v[u], a);
          y[o + u * stride] = relu ? relu_nan(t) : t;
        }
    }
    return;
  }
  const uint32_t Ho = (uint32_t)H >> 1, Wo = (uint32_t)W >> 1;
  const int64_t row4 = (int64_t)W * c4;                             // one input row in 16-byte units
  for (; o < total4; o += 2 * stride) {
    f32x4 v[2][4];
    bool live[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t ou = o + u * stride;
      live[u] = ou < total4;
      if (live[u]) {
        const uint32_t pix = (uint32_t)(ou >> c4_shift);            // output pixel < 2^29
        const uint32_t wo = pix % Wo, r = pix / Wo, ho = r % Ho, b = r / Ho;
        const int64_t in4 = (((int64_t)b * H + 2 * ho) * W + 2 * wo) * c4 + cg;
        v[u][0] = x[in4];
        v[u][1] = x[in4 + c4];
        v[u][2] = x[in4 + row4];
        v[u][3] = x[in4 + row4 + c4];
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (live[u]) {
        const f32x4 t = AFFINE ? max_nan(max_nan(affine(v[u][0], a), affine(v[u][1], a)),
                                         max_nan(affine(v[u][2], a), affine(v[u][3], a)))
                               : max_nan(max_nan(v[u][0], v[u][1]), max_nan(v[u][2], v[u][3]));
        y[o + u * stride] = relu ? relu_nan(t) : t;
      }
  }
}

inline int log2_exact(int v) {
  int s = 0;
  while ((1 << s) < v) ++s;
  return s;
}

}  // namespace

extern "C" int coattn_bn_supported(int B, int H, int W, int C, int pool, int dtype) {
  if (dtype != COATTN_F32 || B < 1 || H < 1 || W < 1) return 0;
  if (C < 16 || C > 512 || (C & (C - 1)) != 0) return 0;           // C / 4 must divide the workgroup's 256 threads
  const int64_t limit = (int64_t)1 << 31;
  const int64_t bh = (int64_t)B * H;
  if (bh >= limit) return 0;
  const int64_t pixels = bh * W;
  if (pixels < 2 || pixels >= limit || pixels * C >= limit) return 0;
  if (pool && (H < 2 || W < 2)) return 0;
  return 1;
}

extern "C" size_t coattn_bn_workspace_bytes(int B, int H, int W, int C) {
  if (!coattn_bn_supported(B, H, W, C, 0, COATTN_F32)) {
    coattn_set_error("bn_workspace_bytes: B=%d H=%d W=%d C=%d is not a supported shape (coattn_bn_supported)", B, H, W, C);
    return 0;
  }
  return partial_bytes(stat_blocks((int64_t)B * H * W), C) + (size_t)4 * C * sizeof(float);
}

extern "C" int coattn_bn_relu_pool_forward(const void* x, const void* gamma, const void* beta, const void* conv_bias,
                                           void* running_mean, void* running_var, double momentum, double eps, void* y,
                                           void* stats_out, void* ws, int B, int H, int W, int C, int pool, int relu,
                                           int dtype, void* stream) {
  CA_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1, "bn_relu_pool_forward: B=%d H=%d W=%d C=%d (all must be >= 1)", B, H, W,
               C);
  CA_CHECK_ARG(coattn_bn_supported(B, H, W, C, pool, dtype),
               "bn_relu_pool_forward: B=%d H=%d W=%d C=%d pool=%d dtype=%d is not supported (coattn_bn_supported)", B, H, W, C,
               pool, dtype);
  CA_CHECK_ARG(x && gamma && beta && running_mean && running_var && y && ws,
               "bn_relu_pool_forward: a null x / gamma / beta / running_mean / running_var / y / ws");
  CA_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0,
               "bn_relu_pool_forward: x, y and ws must be 16-byte aligned");
  CA_CHECK_ARG(x != y, "bn_relu_pool_forward: y must not be x");
  CA_CHECK_ARG(momentum >= 0.0 && momentum <= 1.0, "bn_relu_pool_forward: momentum %g outside [0, 1]", momentum);
  CA_CHECK_ARG(eps > 0.0, "bn_relu_pool_forward: eps %g (must be > 0)", eps);
  hipStream_t s = (hipStream_t)stream;
  const int c4 = C / 4;
  const int64_t pixels = (int64_t)B * H * W;
  const int G = stat_blocks(pixels);
  f64x2* partial = (f64x2*)ws;
  float* ws_f = (float*)((char*)ws + partial_bytes(G, C));
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(G), dim3(kThreads), 0, s, (const f32x4*)x, partial, pixels * c4, c4);
  CA_CHECK_LAUNCH("bn_stats_partial");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(c4), dim3(kThreads), 0, s, (const f64x2*)partial, G, C, (double)pixels,
                     (const float*)gamma, (const float*)conv_bias, (float*)running_mean, (float*)running_var, momentum, eps,
                     ws_f, (float*)stats_out);
  CA_CHECK_LAUNCH("bn_finalize");
  const int64_t out_pixels = pool ? (int64_t)B * (H / 2) * (W / 2) : pixels;
  const int64_t total4 = out_pixels * c4;
  const int per_thread = pool ? 2 : 4;
  int64_t blocks = (total4 + (int64_t)kThreads * per_thread - 1) / ((int64_t)kThreads * per_thread);
  if (blocks > kMaxNormBlocks) blocks = kMaxNormBlocks;
  if (pool)
    hipLaunchKernelGGL(bn_relu_pool_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, s, (const f32x4*)x, ws_f,
                       (const float*)beta, (f32x4*)y, H, W, C, log2_exact(c4), total4, relu);
  else
    hipLaunchKernelGGL(bn_relu_pool_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, s, (const f32x4*)x, ws_f,
                       (const float*)beta, (f32x4*)y, H, W, C, log2_exact(c4), total4, relu);
  CA_CHECK_LAUNCH("bn_relu_pool");
  prof_mark(s, "bn_relu_pool");
  return 0;
}

extern "C" int coattn_relu_pool_forward(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream) {
  CA_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1, "relu_pool_forward: B=%d H=%d W=%d C=%d (all must be >= 1)", B, H, W, C);
  CA_CHECK_ARG(coattn_bn_supported(B, H, W, C, 1, dtype),
               "relu_pool_forward: B=%d H=%d W=%d C=%d dtype=%d is not supported (coattn_bn_supported with pool)", B, H, W, C,
               dtype);
  CA_CHECK_ARG(x && y, "relu_pool_forward: a null x / y");
  CA_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0,
               "relu_pool_forward: x and y must be 16-byte aligned");
  CA_CHECK_ARG(x != y, "relu_pool_forward: y must not be x");
  hipStream_t s = (hipStream_t)stream;
  const int c4 = C / 4;
  const int64_t total4 = (int64_t)B * (H / 2) * (W / 2) * c4;
  int64_t blocks = (total4 + (int64_t)kThreads * 2 - 1) / ((int64_t)kThreads * 2);
  if (blocks > kMaxNormBlocks) blocks = kMaxNormBlocks;
  hipLaunchKernelGGL((bn_relu_pool_kernel<true, false>), dim3((unsigned)blocks), dim3(kThreads), 0, s, (const f32x4*)x,
                     (const float*)nullptr, (const float*)nullptr, (f32x4*)y, H, W, C, log2_exact(c4), total4, 1);
  CA_CHECK_LAUNCH("relu_pool");
  prof_mark(s, "relu_pool");
  return 0;
}
