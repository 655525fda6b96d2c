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
//
// The same two passes with the STOCK kernels' bits (coattn_bn_exact_forward, C-ABI 0.15.0; the default route of encoder.py once a
// shape is verified): MIOpen's multi-kernel spatial BatchNorm is plain fp32 arithmetic in a fixed order, so summing in that order
// gives its mean, invstd, running statistics and y bit for bit (DESIGN 3.12 "The stock kernels' bits"):
//
//   bn_stats_miopen_kernel     workgroup g0 x g1 (channel groups of four x pixels): a thread owns one pixel position and four
//                              channels and adds its B samples in order, sum += x and sq = fma(x, x, sq) in fp32; one halving
//                              tree over the g1 pixels in LDS; one [C][2] fp32 partial per workgroup.
//   bn_finalize_miopen_kernel  workgroup 2 x f1: thread (., t) adds the partials t, t + f1, ... in order, the same tree, times
//                              1 / (B H W); var = max(fma(-mean, mean, E[x^2]), 0), invstd = rsq(var + eps), the running statistics.
//   bn_relu_pool_kernel<POOL, true, true>   t = fma(gamma, (x - mean) * invstd, beta) per element, then the maximum, then ReLU.
//
// Layer 1 (coattn_conv1_bn_exact_forward, C-ABI 0.16.0): conv1_stats_miopen_kernel computes the 3 -> 64 channel convolution in the
// stock convolution's arithmetic and, in the same pass, the partials bn_stats_miopen_kernel would have left; the two kernels
// above follow unchanged.  coattn_conv1_bn_recompute_forward (C-ABI 0.22.0) gives the same results without ever storing the
// convolution output: conv1_stats_miopen_kernel<D, false> sums the statistics alone, conv1_norm_pool_kernel computes the
// convolution again and normalises, pools and writes y.
#include <math.h>

#include <initializer_list>
#include <type_traits>

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

// ---- MIOpen's summation order (the multi-kernel form of its spatial forward-training BatchNorm, NHWC, fp32, vector width 4) ----
// The geometry MIOpen compiles per shape, as bn_exact_geometry() reproduces it; each field under the name of coattn.h.
struct BnGeom {
  int vec, g0, g1, g2, nel, ngrps, ngrps2, f0, f1, f2;
};
constexpr int kGeomInts = 10;
constexpr int kExactLoads = 8;  // 16-byte loads in flight per thread; the adds stay in sample order

__device__ __forceinline__ void acc_miopen(f32x4& sum, f32x4& sq, const f32x4 v) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sum[e] += v[e];
    sq[e] = __builtin_fmaf(v[e], v[e], sq[e]);
  }
}

// The stock kernels' LDS tree: element (xl, yl) at 2 (xl + yl * xs), pairs (sum, sq); `size` rows are halved down to row 0 --
// always row r += row r + red -- and every thread reads row 0 of its column back, times `scale`.
__device__ __forceinline__ void tree_miopen(f32x4& sum, f32x4& sq, float scale, f32x4* lds, int xs, int xl, int yl, int size) {
  const int o1 = 2 * (xl + yl * xs);
  lds[o1] = sum;
  lds[o1 + 1] = sq;
  __syncthreads();
  for (int red = size >> 1; red > 0; red >>= 1) {
    if (yl < red) {
      const int o2 = o1 + red * xs * 2;
      sum += lds[o2];
      sq += lds[o2 + 1];
      lds[o1] = sum;
      lds[o1 + 1] = sq;
    }
    __syncthreads();
  }
  sum = lds[2 * xl] * scale;
  sq = lds[2 * xl + 1] * scale;
}

// grid (c4 / g0, ngrps, ngrps2), block (g0, g1, g2), LDS 32 g0 g1 g2 bytes.  Thread (x, y, z) owns pixel y of the samples
// z nel .. z nel + nel - 1, channels 4 x .. 4 x + 3.  partial[((bz * ngrps + by) * c4 + x) * 2 + {0, 1}] = (sum, sum of squares).
__global__ __launch_bounds__(1024) void bn_stats_miopen_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ partial, BnGeom g,
                                                               int B, int HW, int c4) {
  extern __shared__ f32x4 lds_stats[];
  const int xl = threadIdx.x, yl = threadIdx.y + threadIdx.z * g.g1;
  const int xg = blockIdx.x * g.g0 + xl, yg = blockIdx.y * g.g1 + threadIdx.y, zg = blockIdx.z * g.g2 + threadIdx.z;
  f32x4 sum = {0.f, 0.f, 0.f, 0.f}, sq = {0.f, 0.f, 0.f, 0.f};
  const int n0 = zg * g.nel;
  if (yg < HW && n0 < B) {
    const int64_t sample4 = (int64_t)HW * c4;                      // one sample in 16-byte units
    const f32x4* p = x + ((int64_t)n0 * sample4 + (int64_t)yg * c4 + xg);
    const int nel = B - n0 < g.nel ? B - n0 : g.nel;
    int n = 0;
    for (; n + kExactLoads <= nel; n += kExactLoads) {
      f32x4 v[kExactLoads];
#pragma unroll
      for (int u = 0; u < kExactLoads; ++u) v[u] = p[(n + u) * sample4];
#pragma unroll
      for (int u = 0; u < kExactLoads; ++u) acc_miopen(sum, sq, v[u]);
    }
    for (; n < nel; ++n) acc_miopen(sum, sq, p[n * sample4]);
  }
  tree_miopen(sum, sq, 1.f, lds_stats, g.g0, xl, yl, g.g1 * g.g2);
  if (yl == 0) {
    f32x4* out = partial + (((int64_t)blockIdx.z * g.ngrps + blockIdx.y) * c4 + xg) * 2;
    out[0] = sum;
    out[1] = sq;
  }
}

// grid c4 / f0, block (f0, f1, f2), LDS 32 f0 f1 f2 bytes.  `inhw` = float(1.0 / (B H W)), `unbias` = n / (n - 1) in fp32 with
// n = float(B H W) -- the constants the stock kernel is compiled with; `factor` = float(momentum), `eps` = float(eps).
__global__ __launch_bounds__(1024) void bn_finalize_miopen_kernel(const f32x4* __restrict__ partial, BnGeom g, int c4, float inhw,
                                                                  float unbias, float factor, float eps, f32x4* running_mean,
                                                                  f32x4* running_var, f32x4* __restrict__ save_mean,
                                                                  f32x4* __restrict__ save_invstd) {
  extern __shared__ f32x4 lds_final[];
  const int xl = threadIdx.x, yl = threadIdx.y + threadIdx.z * g.f1;
  const int xg = blockIdx.x * g.f0 + xl;
  f32x4 mean = {0.f, 0.f, 0.f, 0.f}, var = {0.f, 0.f, 0.f, 0.f};
  for (int z = threadIdx.z; z < g.ngrps2; z += g.f2)
    for (int y = threadIdx.y; y < g.ngrps; y += g.f1) {
      const f32x4* p = partial + (((int64_t)z * g.ngrps + y) * c4 + xg) * 2;
      mean += p[0];
      var += p[1];
    }
  tree_miopen(mean, var, inhw, lds_final, g.f0, xl, yl, g.f1 * g.f2);
  f32x4 invstd;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    var[e] = __builtin_fmaxf(__builtin_fmaf(-mean[e], mean[e], var[e]), 0.f);   // (OpenCL's max: a NaN variance becomes 0)
    invstd[e] = __builtin_amdgcn_rsqf(var[e] + eps);
  }
  if (yl != 0) return;
  const f32x4 rm = running_mean[xg], rv = running_var[xg];
  f32x4 nm, nv;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    nm[e] = __builtin_fmaf(mean[e], factor, __builtin_fmaf(-factor, rm[e], rm[e]));
    const float adjust = var[e] * unbias;
    nv[e] = __builtin_fmaf(1.f - factor, rv[e], factor * adjust);
  }
  running_mean[xg] = nm;
  running_var[xg] = nv;
  save_mean[xg] = mean;
  save_invstd[xg] = invstd;
}

// ---- layer 1 (3 -> 64 channels, 3x3, padding 1): the convolution in the stock kernel's arithmetic, statistics riding along ----
// MIOpen runs this layer on Composable Kernel's grouped forward convolution (GridwiseGemmMultipleD_xdl_cshuffle, fp32, one wave
// per 64 x 64 tile, KPerBlock 16, K1 4, 32x32 XDL): gemm-k = (ky, kx, c), c fastest, 27 terms padded with zeros to 32; the wave
// tile is v_mfma_f32_32x32x2_f32, whose two k come from the two lane halves, and the blockwise GEMM gives lane half g the terms
// 8 g .. 8 g + 7 of each block of 16.  So every output is ONE chain from 0 of sixteen MFMAs, MFMA i adding the terms
// (16 (i / 8) + i % 8, the same + 8): 0, 8, 1, 9, .. 7, 15, 16, 24, .. 23, 31.  A tap outside the image is a zero that is still
// multiplied.  The same instruction on the same pairs gives its bits (DESIGN 3.12 "Layer 1").
constexpr int kConv1Terms = 32;
constexpr int kConv1Mfmas = kConv1Terms / 2;
constexpr int kConv1Pixels = 32;   // the 32 columns of the MFMA: the pixels of one wave

// the term MFMA i takes from lane half g when half g holds D consecutive terms of each block of 2 D
template <int D>
__device__ __forceinline__ constexpr int conv1_term(int i, int g) { return (i / D) * 2 * D + g * D + i % D; }

// grid ceil(H W / 32), block 128 (two waves), LDS 16 KB.  The workgroup owns the pixels 32 blockIdx.x .. + 31, wave hh of it
// the output channels 32 hh .. 32 hh + 31; lane l = (g = l >> 5, p = l & 31).
//   A operand: lane (g, p) holds the terms of half g of pixel p (sixteen 4-byte loads per sample).
//   B operand: lane (g, p) holds the weights of output channel 32 hh + p for the terms of half g, loaded once;
//              weight is [64][3][3][3] = [co][ky][kx][c].
//   D: register v = 4 b + r of lane (g, p) is pixel 8 b + 4 g + r, channel 32 hh + p: a store of one register writes two
//      whole 128-byte lines (32 consecutive channels of two pixels).  Whole lines are what the 2 GB write needs: with the
//      operands the other way round (a lane holding four channels of one pixel, 16-byte stores) every store instruction
//      wrote 32 bytes into each of 32 lines and the kernel ran at the stock convolution's 2.3 TB/s.
// The wave walks the B samples in order; each (pixel, channel) is added into its own (sum, sq) exactly as the element of
// thread (channel group, pixel) of bn_stats_miopen_kernel is: sum += x, sq = fma(x, x, sq).  The tree then halves the g1 pixels of each pixel group (g1 = 16: two groups per workgroup; g1 = 8:
// four) in the stock order and writes the same [C][2] partials.
// The operands of lane half g for the pixel (h, w) and the output channel ch: wt[i] the weight and off[i] the image offset of the
// term MFMA i takes (0 where the term is a zero: the load is made and dropped); bit i of the result: term i is a tap inside the
// image.  `live` = false: a masked pixel, every term a zero.
template <int D>
__device__ __forceinline__ unsigned conv1_operands(const float* __restrict__ weight, int ch, int g, int h, int w, bool live, int H,
                                                   int W, float (&wt)[kConv1Mfmas], int (&off)[kConv1Mfmas]) {
  unsigned real = 0;
#pragma unroll
  for (int i = 0; i < kConv1Mfmas; ++i) {
    const int k = conv1_term<D>(i, g);
    const int tap = k / 3, c = k - 3 * tap, ky = tap / 3, kx = tap - 3 * ky;
    const int ih = h + ky - 1, iw = w + kx - 1;
    const bool in = live && k < 27 && ih >= 0 && ih < H && iw >= 0 && iw < W;
    off[i] = in ? (ih * W + iw) * 3 + c : 0;
    real |= in ? 1u << i : 0u;
    const float wk = weight[ch * 27 + (k < 27 ? k : 26)];
    wt[i] = k < 27 ? wk : 0.f;
  }
  return real;
}

// a term of the sample at `base` (uniform over the wave).  An unsigned BYTE offset keeps the load in its scalar-base form, one
// VGPR of address per term instead of a 64-bit pair computed per load; the kernel that stores x keeps the element offsets it
// was tuned with.
__device__ __forceinline__ float conv1_load(const float* __restrict__ base, int off) { return base[off]; }
__device__ __forceinline__ float conv1_load(const float* __restrict__ base, unsigned boff) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + boff);
}

// One output chain: sixteen MFMAs from 0 over `terms`; a term's register is reloaded from `ahead` as soon as its MFMA has read it.
template <typename Off>
__device__ __forceinline__ f32x16 conv1_chain(float (&terms)[kConv1Mfmas], const float (&wt)[kConv1Mfmas],
                                              const Off (&off)[kConv1Mfmas], unsigned real, const float* __restrict__ ahead) {
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
  for (int i = 0; i < kConv1Mfmas; ++i) {
    const float t = (real >> i) & 1u ? terms[i] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(t, wt[i], acc, 0, 0, 0);
    terms[i] = conv1_load(ahead, off[i]);
  }
  return acc;
}

// The same for both channel halves at once: two chains over one set of terms, the MFMAs of the two interleaved (each chain's order
// is its own: the bits are conv1_chain's).  One wave then loads a pixel's terms once for all 64 channels.
template <typename Off>
__device__ __forceinline__ void conv1_chain2(float (&terms)[kConv1Mfmas], const float (&wt0)[kConv1Mfmas],
                                             const float (&wt1)[kConv1Mfmas], const Off (&off)[kConv1Mfmas], unsigned real,
                                             const float* __restrict__ ahead, f32x16& acc0, f32x16& acc1) {
#pragma unroll
  for (int e = 0; e < 16; ++e) acc0[e] = acc1[e] = 0.f;
#pragma unroll
  for (int i = 0; i < kConv1Mfmas; ++i) {
    const float t = (real >> i) & 1u ? terms[i] : 0.f;
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(t, wt0[i], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(t, wt1[i], acc1, 0, 0, 0);
    terms[i] = conv1_load(ahead, off[i]);
  }
}

// STORE = false (pass A of coattn_conv1_bn_recompute_forward): the statistics alone, x is never written and `x` is not read;
// without the store addresses three waves per SIMD fit without scratch (four do not), which the occupancy hint asks for --
// a minimum of 1 is the default: the storing kernel is compiled as before.
template <int D, bool STORE = true>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(STORE ? 1 : 3))) void conv1_stats_miopen_kernel(
    const float* __restrict__ image, const float* __restrict__ weight, float* __restrict__ x, float* __restrict__ partial, int B,
    int H, int W, int g1, int ngrps) {
  __shared__ float lds[kConv1Pixels * 64 * 2];                      // [pixel][channel]{sum, sq}
  const int hh = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 5, p = lane & 31;
  const int HW = H * W;
  const int pbase = blockIdx.x * kConv1Pixels, pix = pbase + p;
  const bool live = pix < HW;                                       // (of the pixel whose terms this lane loads)
  const bool full = pbase + kConv1Pixels <= HW;                     // (of the workgroup: no masked pixel)
  const int h = pix / W, w = pix - h * W;
  const int ch = 32 * hh + p;
  float wt[kConv1Mfmas];
  int off[kConv1Mfmas];
  const unsigned real = conv1_operands<D>(weight, ch, g, h, w, live, H, W, wt, off);
  typename std::conditional<STORE, int, unsigned>::type toff[kConv1Mfmas];
#pragma unroll
  for (int i = 0; i < kConv1Mfmas; ++i) toff[i] = STORE ? off[i] : (unsigned)off[i] * 4u;   // (H W 12 < 2^29 for a covered shape)
  const int64_t sample = (int64_t)HW * 3;
  // two buffers of terms, for the samples n and n + 1; a term's register is reloaded for sample n + 2 as soon as its MFMA has
  // read it.  Two samples ahead, not one: a wait for a load also waits for every store issued before it, and these loads
  // are issued before the stores of the samples n and n + 1, so the chain of sample n + 2 waits for stores two samples old.
  float even[kConv1Mfmas], odd[kConv1Mfmas];
  const float* image1 = image + (B > 1 ? sample : 0);
#pragma unroll
  for (int i = 0; i < kConv1Mfmas; ++i) even[i] = conv1_load(image, toff[i]);
#pragma unroll
  for (int i = 0; i < kConv1Mfmas; ++i) odd[i] = conv1_load(image1, toff[i]);
  float sum[16], sq[16];                                            // [v]: pixel 8 (v >> 2) + 4 g + (v & 3), channel ch
#pragma unroll
  for (int v = 0; v < 16; ++v) sum[v] = sq[v] = 0.f;
  float* xo = STORE ? x + ((int64_t)(pbase + 4 * g) * 64 + ch) : nullptr;   // register v goes (8 (v >> 2) + (v & 3)) pixels further
  const int64_t xstep = (int64_t)HW * 64;
  auto one_sample = [&](float (&terms)[kConv1Mfmas], int n) {
    const float* ahead = image + (int64_t)(n + 2 < B ? n + 2 : B - 1) * sample;      // (the last two reload the last sample)
    const f32x16 acc = conv1_chain(terms, wt, toff, real, ahead);
    if (full) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        if constexpr (STORE) xo[(8 * (v >> 2) + (v & 3)) * 64] = acc[v];
        sum[v] += acc[v];
        sq[v] = __builtin_fmaf(acc[v], acc[v], sq[v]);
      }
    } else {
#pragma unroll
      for (int v = 0; v < 16; ++v)
        if (pbase + 8 * (v >> 2) + 4 * g + (v & 3) < HW) {
          if constexpr (STORE) xo[(8 * (v >> 2) + (v & 3)) * 64] = acc[v];
          sum[v] += acc[v];
          sq[v] = __builtin_fmaf(acc[v], acc[v], sq[v]);
        }
    }
    if constexpr (STORE) xo += xstep;
  };
  for (int n = 0; n < B; n += 2) {
    one_sample(even, n);
    if (n + 1 < B) one_sample(odd, n + 1);
  }
  // the stock tree over the g1 pixel rows of a pixel group: row r += row r + red, red = g1 / 2 .. 1
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int o = ((8 * (v >> 2) + 4 * g + (v & 3)) * 64 + ch) * 2;
    lds[o] = sum[v];
    lds[o + 1] = sq[v];
  }
  __syncthreads();
  for (int red = g1 >> 1; red > 0; red >>= 1) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int q = 8 * (v >> 2) + 4 * g + (v & 3);
      if ((q & (g1 - 1)) < red) {
        const int o = (q * 64 + ch) * 2, o2 = o + red * 128;
        sum[v] += lds[o2];
        sq[v] += lds[o2 + 1];
        lds[o] = sum[v];
        lds[o + 1] = sq[v];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int q = 8 * (v >> 2) + 4 * g + (v & 3), grp = (pbase + q) / g1;
    if ((q & (g1 - 1)) == 0 && grp < ngrps) {
      float* out = partial + (((int64_t)grp * 16 + (ch >> 2)) * 2) * 4 + (ch & 3);
      out[0] = sum[v];
      out[4] = sq[v];
    }
  }
}

// The slow probe of tools/probe_conv1_exact.py: one thread per output, the chain's order and step switchable.
//   order : 0 (ky, kx, c)  1 (ky, c, kx)  2 (c, ky, kx)  3 (kx, ky, c)  4 (c, kx, ky)  5 (kx, c, ky), last fastest, 28 terms;
//           6 + 2 j + f: (ky, kx, c) padded to 32 terms and taken in pairs (t, t + D) within blocks of 2 D, D = 8, 4, 2, 16 for
//           j = 0 .. 3 -- the order a k-reducing MFMA gives when each lane half holds D consecutive terms --, f = 1: the upper
//           term of a pair first
//   step  : 0 fmaf   1 multiply, then add (two roundings)
//   halves: 1 one chain   2 two chains over the first and the second half of the terms, added
//   skip  : 1 leaves the taps outside the image and the padding terms out instead of multiplying zeros
__global__ __launch_bounds__(256) void conv1_probe_kernel(const float* __restrict__ image, const float* __restrict__ weight,
                                                          float* __restrict__ x, int64_t total, int H, int W, int order, int step,
                                                          int halves, int skip) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int co = (int)(i & 63);
  const int64_t pixel = i >> 6;
  const int w = (int)(pixel % W), h = (int)((pixel / W) % H);
  const int64_t n = pixel / ((int64_t)W * H);
  const int terms = order < 6 ? 28 : 32;
  const int pair = order - 6, dist = pair < 0 ? 1 : (pair >> 1) == 0 ? 8 : (pair >> 1) == 1 ? 4 : (pair >> 1) == 2 ? 2 : 16;
  float acc[2] = {0.f, 0.f};
  for (int s = 0; s < terms; ++s) {
    int t = s;
    if (pair >= 0) {
      const int r = s % (2 * dist), gsel = (r & 1) ^ (pair & 1);
      t = (s / (2 * dist)) * 2 * dist + gsel * dist + (r >> 1);
    }
    float a = 0.f, v = 0.f;
    bool real = false;
    if (t < 27) {
      const int i0 = t / 9, i1 = (t / 3) % 3, i2 = t % 3;         // slowest .. fastest
      int ky, kx, c;
      switch (order) {
        case 1: ky = i0, c = i1, kx = i2; break;
        case 2: c = i0, ky = i1, kx = i2; break;
        case 3: kx = i0, ky = i1, c = i2; break;
        case 4: c = i0, kx = i1, ky = i2; break;
        case 5: kx = i0, c = i1, ky = i2; break;
        default: ky = i0, kx = i1, c = i2; break;
      }
      a = weight[co * 27 + (ky * 3 + kx) * 3 + c];
      const int hh = h + ky - 1, ww = w + kx - 1;
      if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
        v = image[((n * H + hh) * W + ww) * 3 + c];
        real = true;
      }
    }
    if (skip && !real) continue;
    float& sacc = acc[halves == 2 && s >= terms / 2 ? 1 : 0];
    if (step == 0) {
      sacc = __builtin_fmaf(a, v, sacc);
    } else {
      const float prod = __fmul_rn(a, v);
      sacc = __fadd_rn(prod, sacc);
    }
  }
  x[i] = halves == 2 ? __fadd_rn(acc[0], acc[1]) : acc[0];
}

struct Affine {
  float mean[4], lo[4], scale[4], beta[4], gamma[4];
};

// STOCK: MIOpen's normalise kernel, t = mad(gamma, (x - mean) * invstd, beta) with `scale` = invstd
// The per-element and per-window functions of the normalise pass, shared by bn_relu_pool_kernel and conv1_norm_pool_kernel: the
// two must give the same bits, -0 / +0 and NaN included.
template <bool STOCK>
__device__ __forceinline__ float affine1(float v, float mean, float lo, float scale, float gamma, float beta) {
  return STOCK ? __builtin_fmaf(gamma, (v - mean) * scale, beta) : fmaf((v - mean) - lo, scale, beta);
}
// PyTorch's maximum: a NaN wins
__device__ __forceinline__ float max_nan1(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float relu_nan1(float a) { return a < 0.f ? 0.f : a; }   // (a NaN is not < 0: it stays)
// the members of a 2x2 window in the order (0, 0), (0, 1), (1, 0), (1, 1) = (dy, dx)
__device__ __forceinline__ float window_max1(float t00, float t01, float t10, float t11) {
  return max_nan1(max_nan1(t00, t01), max_nan1(t10, t11));
}

// The eval forms (v0.24.0): MIOpen's spatial inference kernel computes, per channel, invVariance = rsqrt(fabs(variance + (float)
// epsilon)) and, per element, mad(scale, (x - mean) * invVariance, bias) -- affine1<true> with the running statistics.  A
// convolution bias the caller left out of x is one fp32 add in front (the stock convolution's separate add).
// The reciprocal square root is the candidate tools/probe_encoder_eval.py found equal to the stock kernel's on every operand
// (DESIGN 3.19): 1, the device library's rsqrt.  0 the bare v_rsq_f32 (differs where var + eps is subnormal), 2 1 / sqrt, each
// correctly rounded (differs in the last bit), 3 v_rsq_f32 of an operand scaled out of the subnormal range (equal on all of them).
template <int V>
__device__ __forceinline__ float eval_rsqrt(float a) {
  if (V == 0) return __builtin_amdgcn_rsqf(a);
  if (V == 1) return rsqrtf(a);
  if (V == 2) return __fdiv_rn(1.f, __fsqrt_rn(a));
  const bool small = a < 0x1p-100f;
  return __builtin_amdgcn_rsqf(small ? a * 0x1p+100f : a) * (small ? 0x1p+50f : 1.f);
}
constexpr int kEvalRsqrt = 1;
__device__ __forceinline__ float eval_invstd(float var, float eps) { return eval_rsqrt<kEvalRsqrt>(__builtin_fabsf(var + eps)); }
// EVAL: 0 the batch statistics of the train forms, 1 running statistics, 2 running statistics and a convolution bias
template <int EVAL>
__device__ __forceinline__ float add_bias1(float v, float bias) { return EVAL == 2 ? __fadd_rn(v, bias) : v; }

template <bool STOCK>
__device__ __forceinline__ f32x4 affine(const f32x4 v, const Affine& a) {
  f32x4 t;
#pragma unroll
  for (int e = 0; e < 4; ++e) t[e] = affine1<STOCK>(v[e], a.mean[e], a.lo[e], a.scale[e], a.gamma[e], a.beta[e]);
  return t;
}
__device__ __forceinline__ f32x4 window_max(const f32x4 t00, const f32x4 t01, const f32x4 t10, const f32x4 t11) {
  f32x4 m;
#pragma unroll
  for (int e = 0; e < 4; ++e) m[e] = window_max1(t00[e], t01[e], t10[e], t11[e]);
  return m;
}
__device__ __forceinline__ f32x4 relu_nan(const f32x4 a) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = relu_nan1(a[e]);
  return r;
}

// One thread per 16 bytes of output: o = output pixel * c4 + channel group.  total4 = output pixels * c4; H, W: the INPUT's.
// AFFINE = false: the 2x2 maximum and the ReLU alone (ws_f, beta not read): max and ReLU are exact, so the result has the bits of
// max_pool2d followed by relu.  STOCK: ws_f = save_mean, ws_f + 2 C = save_invstd (the caller passes `scale` itself) and
// `gamma` is read: the stock normalise kernel's map.  EVAL (with STOCK; coattn_bn_eval_forward): ws_f = running_mean, `scale` =
// running_var, from which the prologue computes invstd as the stock inference kernel does; EVAL == 2: `conv_bias` is added to x first.
template <bool POOL, bool AFFINE = true, bool STOCK = false, int EVAL = 0>
__global__ __launch_bounds__(kThreads) void bn_relu_pool_kernel(const f32x4* __restrict__ x, const float* __restrict__ ws_f,
                                                                const float* __restrict__ scale, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, f32x4* __restrict__ y,
                                                                int H, int W, int C, int c4_shift, int64_t total4, int relu,
                                                                const float* __restrict__ conv_bias = nullptr, float eps = 0.f) {
  const int tid = threadIdx.x;
  const int c4 = C >> 2;
  const int cg = tid & (c4 - 1);                                    // (block starts and the grid stride are multiples of c4)
  Affine a;
  f32x4 cb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a.mean[e] = AFFINE ? ws_f[4 * cg + e] : 0.f;
    a.lo[e] = AFFINE && !STOCK ? ws_f[C + 4 * cg + e] : 0.f;
    a.scale[e] = AFFINE ? scale[4 * cg + e] : 1.f;
    if (EVAL) a.scale[e] = eval_invstd(a.scale[e], eps);
    a.gamma[e] = STOCK ? gamma[4 * cg + e] : 1.f;
    a.beta[e] = AFFINE ? beta[4 * cg + e] : 0.f;
    if (EVAL == 2) cb[e] = conv_bias[4 * cg + e];
  }
  auto biased = [&](f32x4 v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = add_bias1<EVAL>(v[e], cb[e]);
    return v;
  };
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
          const f32x4 t = affine<STOCK>(biased(v[u]), a);
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
        const f32x4 t = AFFINE ? window_max(affine<STOCK>(biased(v[u][0]), a), affine<STOCK>(biased(v[u][1]), a),
                                            affine<STOCK>(biased(v[u][2]), a), affine<STOCK>(biased(v[u][3]), a))
                               : window_max(v[u][0], v[u][1], v[u][2], v[u][3]);
        y[o + u * stride] = relu ? relu_nan(t) : t;
      }
  }
}

// ---- layer 1 without x (pass B of coattn_conv1_bn_recompute_forward): the convolution again, normalised, pooled, ReLU, y alone ----
// The chain is conv1_stats_miopen_kernel's (conv1_operands, conv1_chain): an output's bits depend on the term order only, not on
// the MFMA row its pixel sits in, so the rows are free to be the pixels of whole pooling windows.  No state crosses samples: the
// grid is (tile, chunk of kConv1NormChunk samples).  A workgroup is ONE wave that runs both channel halves (chain hh: channels
// 32 hh .. 32 hh + 31) over one set of terms (conv1_chain2): with a wave per half, as above, the two waves issue the same
// sixteen scattered 4-byte loads per sample, and the pass took 428 us against 388 us this way at the benchmark's shape.  The
// weights are loaded once per workgroup, the terms of the samples n + 1 and n + 2 are in flight as above (y's stores are older
// than the loads behind them).
//   POOL : the tile is 2 image rows x 16 columns, tile t = (pooled row ho = t / cbs, column block cb = t % cbs), cbs = ceil(Wo / 8).
//          MFMA row slot q = 8 b + 4 g + r is member r (dy = r >> 1, dx = r & 1: bn_relu_pool_kernel's order) of the window
//          q >> 2 = 2 b + g, the pooled column 8 cb + 2 b + g.  Register v = 4 b + r of chain hh in lane (g, p) holds member r of
//          that window for channel 32 hh + p: the four registers of a b are one window, normalised, reduced and stored in-lane -- one store per
//          b, two whole 128-byte lines.  Windows past Wo are masked (their lanes load offset 0 and multiply zeros); floor mode:
//          the tile never reaches an odd last row or column.
//   !POOL: the tile is 32 consecutive pixels, stored as conv1_stats_miopen_kernel stores x.
// 163 VGPRs (both accumulators included), no LDS, no scratch: three waves per SIMD, which the occupancy hint asks for.
constexpr int kConv1NormChunk = COATTN_CONV1_RECOMPUTE_CHUNK;

// EVAL (coattn_conv1_bn_eval_forward: the whole group in this one launch): save_mean = running_mean, save_invstd = running_var,
// turned into invstd here as the stock inference kernel does; EVAL == 2: `conv_bias` is added to every convolution output first.
template <int D, bool POOL, int EVAL = 0>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void conv1_norm_pool_kernel(
    const float* __restrict__ image, const float* __restrict__ weight, const float* __restrict__ save_mean,
    const float* __restrict__ save_invstd, const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y,
    int B, int H, int W, int cbs, const float* __restrict__ conv_bias = nullptr, float eps = 0.f) {
  const int lane = threadIdx.x, g = lane >> 5, p = lane & 31;
  const int HW = H * W, Ho = H >> 1, Wo = W >> 1;
  const int n0 = blockIdx.y * kConv1NormChunk, n1 = n0 + kConv1NormChunk < B ? n0 + kConv1NormChunk : B;
  // the pixel whose terms this lane loads: slot p of the tile
  const int ho = POOL ? blockIdx.x / cbs : 0, cb = POOL ? blockIdx.x - ho * cbs : 0;
  const int pbase = blockIdx.x * kConv1Pixels;
  const int pix = pbase + p;
  const bool live = POOL ? 8 * cb + (p >> 2) < Wo : pix < HW;
  const int h = POOL ? 2 * ho + ((p >> 1) & 1) : pix / W;
  const int w = POOL ? 2 * (8 * cb + (p >> 2)) + (p & 1) : pix - h * W;
  float wt0[kConv1Mfmas], wt1[kConv1Mfmas];                         // channel p and channel 32 + p
  int off[kConv1Mfmas];
  const unsigned real = conv1_operands<D>(weight, p, g, h, w, live, H, W, wt0, off);
  conv1_operands<D>(weight, 32 + p, g, h, w, live, H, W, wt1, off);
  unsigned boff[kConv1Mfmas];
#pragma unroll
  for (int i = 0; i < kConv1Mfmas; ++i) boff[i] = (unsigned)off[i] * 4u;
  const float mean[2] = {save_mean[p], save_mean[32 + p]};
  float invstd[2] = {save_invstd[p], save_invstd[32 + p]};
  if (EVAL) invstd[0] = eval_invstd(invstd[0], eps), invstd[1] = eval_invstd(invstd[1], eps);
  const float cbias[2] = {EVAL == 2 ? conv_bias[p] : 0.f, EVAL == 2 ? conv_bias[32 + p] : 0.f};
  const float gm[2] = {gamma[p], gamma[32 + p]}, bt[2] = {beta[p], beta[32 + p]};
  const int64_t sample = (int64_t)HW * 3;
  float even[kConv1Mfmas], odd[kConv1Mfmas];
  const float* image0 = image + (int64_t)n0 * sample;
  const float* image1 = image + (int64_t)(n0 + 1 < n1 ? n0 + 1 : n0) * sample;
#pragma unroll
  for (int i = 0; i < kConv1Mfmas; ++i) even[i] = conv1_load(image0, boff[i]);
#pragma unroll
  for (int i = 0; i < kConv1Mfmas; ++i) odd[i] = conv1_load(image1, boff[i]);
  // POOL: register group b goes 2 b pooled pixels further; !POOL: register v goes (8 (v >> 2) + (v & 3)) pixels further;
  // the second chain's channel is 32 floats further
  const int wo = 8 * cb + g;
  float* yo = POOL ? y + ((((int64_t)n0 * Ho + ho) * Wo + wo) * 64 + p) : y + (((int64_t)n0 * HW + pbase + 4 * g) * 64 + p);
  const int64_t ystep = POOL ? (int64_t)Ho * Wo * 64 : (int64_t)HW * 64;
  const bool full = POOL ? 8 * cb + 8 <= Wo : pbase + kConv1Pixels <= HW;   // (of the workgroup: nothing masked)
  auto one_sample = [&](float (&terms)[kConv1Mfmas], int n) {
    const float* ahead = image + (int64_t)(n + 2 < n1 ? n + 2 : n1 - 1) * sample;    // (the last two reload the last sample)
    f32x16 acc[2];
    conv1_chain2(terms, wt0, wt1, boff, real, ahead, acc[0], acc[1]);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      if (POOL) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          auto t = [&](int r) {
            return affine1<true>(add_bias1<EVAL>(acc[hh][4 * b + r], cbias[hh]), mean[hh], 0.f, invstd[hh], gm[hh], bt[hh]);
          };
          const float m = window_max1(t(0), t(1), t(2), t(3));
          if (full || wo + 2 * b < Wo) yo[2 * b * 64 + 32 * hh] = relu_nan1(m);
        }
      } else {
#pragma unroll
        for (int v = 0; v < 16; ++v)
          if (full || pbase + 8 * (v >> 2) + 4 * g + (v & 3) < HW)
            yo[(8 * (v >> 2) + (v & 3)) * 64 + 32 * hh] =
                relu_nan1(affine1<true>(add_bias1<EVAL>(acc[hh][v], cbias[hh]), mean[hh], 0.f, invstd[hh], gm[hh], bt[hh]));
      }
    }
    yo += ystep;
  };
  for (int n = n0; n < n1; n += 2) {
    one_sample(even, n);
    if (n + 1 < n1) one_sample(odd, n + 1);
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
                       ws_f + 2 * C, (const float*)nullptr, (const float*)beta, (f32x4*)y, H, W, C, log2_exact(c4), total4, relu);
  else
    hipLaunchKernelGGL(bn_relu_pool_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, s, (const f32x4*)x, ws_f,
                       ws_f + 2 * C, (const float*)nullptr, (const float*)beta, (f32x4*)y, H, W, C, log2_exact(c4), total4, relu);
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
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (f32x4*)y, H, W,
                     C, log2_exact(c4), total4, 1);
  CA_CHECK_LAUNCH("relu_pool");
  prof_mark(s, "relu_pool");
  return 0;
}

// ---- the stock kernels' bits (v0.15.0) ------------------------------------------------------------------------------------
namespace {

// The geometry MIOpen gives its multi-kernel NHWC fp32 form, as read off its kernel builds (the table of
// observed values): vector width 4 along C, workgroups of 16 channel groups x g1 pixels, every thread adds all B samples
// (one sample group), the final kernel runs 2 channel groups x 8 g1 partial lanes.  g1 is 8 up to H W C = 153600 and 16 from
// 163840 on (every observed shape, C = 64 .. 512; B, 1 .. 1024, does not enter); between the two nothing was observed and
// nothing is covered.
constexpr int64_t kSmallMaxHWC = 153600, kLargeMinHWC = 163840;
constexpr int kExactMaxB = 1024;

bool bn_exact_geometry(int B, int H, int W, int C, int dtype, BnGeom* g) {
  if (dtype != COATTN_F32 || !coattn_bn_supported(B, H, W, C, 0, dtype)) return false;
  if (C < 64 || B > kExactMaxB) return false;                     // C / 4 a multiple of the 16 channel groups of a workgroup
  const int64_t hw = (int64_t)H * W, hwc = hw * C;
  if (hwc > kSmallMaxHWC && hwc < kLargeMinHWC) return false;
  g->vec = 4;
  g->g0 = 16;
  g->g1 = hwc <= kSmallMaxHWC ? 8 : 16;
  g->g2 = 1;
  g->nel = B;
  g->ngrps = (int)((hw + g->g1 - 1) / g->g1);
  g->ngrps2 = 1;
  g->f0 = 2;
  g->f1 = g->g0 * g->g1 / 2;
  g->f2 = 1;
  // MIOpen keeps its partials in two pixel rows of y per workgroup; where the last workgroup has one pixel only
  // (H W = 1 mod g1) it stores them another way and, with few samples, sums differently: observed, not reproduced
  if (hw % g->g1 == 1) return false;
  return g->ngrps <= 65535;                                         // (grid.y)
}

inline size_t exact_partial_bytes(const BnGeom& g, int C) { return (size_t)g.ngrps * g.ngrps2 * C * 2 * sizeof(float); }

// bn_finalize_miopen_kernel and the normalise (+ pool) + ReLU pass over x, behind a statistics kernel that left `partial`
int exact_tail(const void* x, const void* gamma, const void* beta, void* running_mean, void* running_var, double momentum,
               double eps, void* y, void* save_mean, void* save_invstd, const f32x4* partial, const BnGeom& g, int B, int H, int W,
               int C, int pool, int relu, hipStream_t s) {
  const int c4 = C / 4;
  const int64_t pixels = (int64_t)B * H * W;
  // the constants of the stock build: INHW = float(1.0 / n) as a kernel argument, n / (n - 1) folded in fp32
  const float n_f = (float)pixels;
  const float inhw = (float)(1.0 / (double)pixels), unbias = pixels == 1 ? 1.f : n_f / (n_f - 1.f);
  hipLaunchKernelGGL(bn_finalize_miopen_kernel, dim3(c4 / g.f0), dim3(g.f0, g.f1, g.f2),
                     (size_t)2 * g.f0 * g.f1 * g.f2 * sizeof(f32x4), s, (const f32x4*)partial, g, c4, inhw, unbias,
                     (float)momentum, (float)eps, (f32x4*)running_mean, (f32x4*)running_var, (f32x4*)save_mean,
                     (f32x4*)save_invstd);
  CA_CHECK_LAUNCH("bn_finalize_miopen");
  const int64_t out_pixels = pool ? (int64_t)B * (H / 2) * (W / 2) : pixels;
  const int64_t total4 = out_pixels * c4;
  const int per_thread = pool ? 2 : 4;
  int64_t blocks = (total4 + (int64_t)kThreads * per_thread - 1) / ((int64_t)kThreads * per_thread);
  if (blocks > kMaxNormBlocks) blocks = kMaxNormBlocks;
  if (pool)
    hipLaunchKernelGGL((bn_relu_pool_kernel<true, true, true>), dim3((unsigned)blocks), dim3(kThreads), 0, s, (const f32x4*)x,
                       (const float*)save_mean, (const float*)save_invstd, (const float*)gamma, (const float*)beta, (f32x4*)y, H,
                       W, C, log2_exact(c4), total4, relu);
  else
    hipLaunchKernelGGL((bn_relu_pool_kernel<false, true, true>), dim3((unsigned)blocks), dim3(kThreads), 0, s, (const f32x4*)x,
                       (const float*)save_mean, (const float*)save_invstd, (const float*)gamma, (const float*)beta, (f32x4*)y, H,
                       W, C, log2_exact(c4), total4, relu);
  CA_CHECK_LAUNCH("bn_relu_pool_exact");
  return 0;
}

}  // namespace

extern "C" int coattn_bn_exact_geometry(int B, int H, int W, int C, int dtype, int* out) {
  BnGeom g;
  if (!bn_exact_geometry(B, H, W, C, dtype, &g)) return 0;
  if (out) {
    const int v[kGeomInts] = {g.vec, g.g0, g.g1, g.g2, g.nel, g.ngrps, g.ngrps2, g.f0, g.f1, g.f2};
    for (int i = 0; i < kGeomInts; ++i) out[i] = v[i];
  }
  return kGeomInts;
}

extern "C" size_t coattn_bn_exact_workspace_bytes(int B, int H, int W, int C) {
  BnGeom g;
  if (!bn_exact_geometry(B, H, W, C, COATTN_F32, &g)) {
    coattn_set_error("bn_exact_workspace_bytes: B=%d H=%d W=%d C=%d is not a covered shape (coattn_bn_exact_geometry)", B, H, W, C);
    return 0;
  }
  return exact_partial_bytes(g, C);
}

extern "C" int coattn_bn_exact_forward(const void* x, const void* gamma, const void* beta, void* running_mean, void* running_var,
                                       double momentum, double eps, void* y, void* save_mean, void* save_invstd, void* ws, int B,
                                       int H, int W, int C, int pool, int relu, int dtype, void* stream) {
  CA_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1, "bn_exact_forward: B=%d H=%d W=%d C=%d (all must be >= 1)", B, H, W, C);
  BnGeom g;
  CA_CHECK_ARG(bn_exact_geometry(B, H, W, C, dtype, &g) && coattn_bn_supported(B, H, W, C, pool, dtype),
               "bn_exact_forward: B=%d H=%d W=%d C=%d pool=%d dtype=%d is not a covered shape (coattn_bn_exact_geometry)", B, H,
               W, C, pool, dtype);
  CA_CHECK_ARG(x && gamma && beta && running_mean && running_var && y && save_mean && save_invstd && ws,
               "bn_exact_forward: a null x / gamma / beta / running_mean / running_var / y / save_mean / save_invstd / ws");
  CA_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(ws) |
                 reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta) | reinterpret_cast<uintptr_t>(running_mean) |
                 reinterpret_cast<uintptr_t>(running_var) | reinterpret_cast<uintptr_t>(save_mean) |
                 reinterpret_cast<uintptr_t>(save_invstd)) & 15) == 0,
               "bn_exact_forward: every pointer must be 16-byte aligned");
  CA_CHECK_ARG(x != y, "bn_exact_forward: y must not be x");
  CA_CHECK_ARG(momentum >= 0.0 && momentum <= 1.0, "bn_exact_forward: momentum %g outside [0, 1]", momentum);
  CA_CHECK_ARG(eps > 0.0, "bn_exact_forward: eps %g (must be > 0)", eps);
  hipStream_t s = (hipStream_t)stream;
  const int c4 = C / 4, hw = H * W;
  f32x4* partial = (f32x4*)ws;
  hipLaunchKernelGGL(bn_stats_miopen_kernel, dim3(c4 / g.g0, g.ngrps, g.ngrps2), dim3(g.g0, g.g1, g.g2),
                     (size_t)2 * g.g0 * g.g1 * g.g2 * sizeof(f32x4), s, (const f32x4*)x, partial, g, B, hw, c4);
  CA_CHECK_LAUNCH("bn_stats_miopen");
  if (exact_tail(x, gamma, beta, running_mean, running_var, momentum, eps, y, save_mean, save_invstd, partial, g, B, H, W, C, pool,
                 relu, s))
    return -1;
  prof_mark(s, "bn_exact");
  return 0;
}

// ---- layer 1: convolution + statistics in one pass, the stock kernels' bits (v0.16.0) -----------------------------------------
namespace {

constexpr int kConv1PairDistance = 8;   // terms per lane half and block: KPerBlock / 2 of the stock kernel

inline size_t conv1_partial_bytes(const BnGeom& g) { return (exact_partial_bytes(g, 64) + 255) & ~(size_t)255; }

// x = NULL: the statistics alone (STORE = false)
void launch_conv1(int dist, const void* image, const void* weight, void* x, void* partial, const BnGeom& g, int B, int H, int W,
                  hipStream_t s) {
  const int blocks = (H * W + kConv1Pixels - 1) / kConv1Pixels;
  if (!x)
    hipLaunchKernelGGL((conv1_stats_miopen_kernel<kConv1PairDistance, false>), dim3(blocks), dim3(128), 0, s, (const float*)image,
                       (const float*)weight, (float*)nullptr, (float*)partial, B, H, W, g.g1, g.ngrps);
  else if (dist == 8)
    hipLaunchKernelGGL(conv1_stats_miopen_kernel<8>, dim3(blocks), dim3(128), 0, s, (const float*)image, (const float*)weight,
                       (float*)x, (float*)partial, B, H, W, g.g1, g.ngrps);
  else
    hipLaunchKernelGGL(conv1_stats_miopen_kernel<4>, dim3(blocks), dim3(128), 0, s, (const float*)image, (const float*)weight,
                       (float*)x, (float*)partial, B, H, W, g.g1, g.ngrps);
}

}  // namespace

extern "C" int coattn_conv1_bn_exact_supported(int B, int H, int W, int Cin, int Cout, int pool, int dtype) {
  BnGeom g;
  if (Cin != 3 || Cout != 64) return 0;
  return bn_exact_geometry(B, H, W, Cout, dtype, &g) && coattn_bn_supported(B, H, W, Cout, pool, dtype) ? 1 : 0;
}

extern "C" size_t coattn_conv1_bn_exact_workspace_bytes(int B, int H, int W, int with_x) {
  BnGeom g;
  if (!bn_exact_geometry(B, H, W, 64, COATTN_F32, &g)) {
    coattn_set_error("conv1_bn_exact_workspace_bytes: B=%d H=%d W=%d is not a covered shape (coattn_conv1_bn_exact_supported)", B, H, W);
    return 0;
  }
  return conv1_partial_bytes(g) + (with_x ? (size_t)B * H * W * 64 * sizeof(float) : 0);
}

extern "C" int coattn_conv1_bn_exact_forward(const void* image, const void* weight, const void* gamma, const void* beta,
                                             void* running_mean, void* running_var, double momentum, double eps, void* x_out,
                                             void* y, void* save_mean, void* save_invstd, void* ws, int B, int H, int W, int Cin,
                                             int Cout, int pool, int dtype, void* stream) {
  CA_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "conv1_bn_exact_forward: B=%d H=%d W=%d Cin=%d Cout=%d (all must be >= 1)",
               B, H, W, Cin, Cout);
  BnGeom g;
  CA_CHECK_ARG(coattn_conv1_bn_exact_supported(B, H, W, Cin, Cout, pool, dtype) && bn_exact_geometry(B, H, W, Cout, dtype, &g),
               "conv1_bn_exact_forward: B=%d H=%d W=%d Cin=%d Cout=%d pool=%d dtype=%d is not a covered shape "
               "(coattn_conv1_bn_exact_supported)", B, H, W, Cin, Cout, pool, dtype);
  CA_CHECK_ARG(image && weight && gamma && beta && running_mean && running_var && y && save_mean && save_invstd && ws,
               "conv1_bn_exact_forward: a null image / weight / gamma / beta / running_mean / running_var / y / save_mean / "
               "save_invstd / ws");
  CA_CHECK_ARG(((reinterpret_cast<uintptr_t>(x_out) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(ws) |
                 reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta) | reinterpret_cast<uintptr_t>(running_mean) |
                 reinterpret_cast<uintptr_t>(running_var) | reinterpret_cast<uintptr_t>(save_mean) |
                 reinterpret_cast<uintptr_t>(save_invstd)) & 15) == 0 &&
                   ((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(weight)) & 3) == 0,
               "conv1_bn_exact_forward: x_out, y, ws, the BatchNorm vectors must be 16-byte aligned, image and weight 4-byte aligned");
  CA_CHECK_ARG(momentum >= 0.0 && momentum <= 1.0, "conv1_bn_exact_forward: momentum %g outside [0, 1]", momentum);
  CA_CHECK_ARG(eps > 0.0, "conv1_bn_exact_forward: eps %g (must be > 0)", eps);
  void* x = x_out ? x_out : (void*)((char*)ws + conv1_partial_bytes(g));
  CA_CHECK_ARG(x != y && x != image && y != image, "conv1_bn_exact_forward: image, x_out and y must be three buffers");
  hipStream_t s = (hipStream_t)stream;
  launch_conv1(kConv1PairDistance, image, weight, x, ws, g, B, H, W, s);
  CA_CHECK_LAUNCH("conv1_stats_miopen");
  if (exact_tail(x, gamma, beta, running_mean, running_var, momentum, eps, y, save_mean, save_invstd, (const f32x4*)ws, g, B, H, W,
                 Cout, pool, 1, s))
    return -1;
  prof_mark(s, "conv1_bn_exact");
  return 0;
}

// ---- layer 1, the convolution computed twice and never stored (v0.22.0) ---------------------------------------------------------
extern "C" size_t coattn_conv1_bn_recompute_workspace_bytes(int B, int H, int W) {
  BnGeom g;
  if (!bn_exact_geometry(B, H, W, 64, COATTN_F32, &g)) {
    coattn_set_error("conv1_bn_recompute_workspace_bytes: B=%d H=%d W=%d is not a covered shape (coattn_conv1_bn_exact_supported)", B, H, W);
    return 0;
  }
  return conv1_partial_bytes(g);
}

extern "C" int coattn_conv1_bn_recompute_forward(const void* image, const void* weight, const void* gamma, const void* beta,
                                                 void* running_mean, void* running_var, double momentum, double eps, void* y,
                                                 void* save_mean, void* save_invstd, void* ws, int B, int H, int W, int Cin,
                                                 int Cout, int pool, int dtype, void* stream) {
  CA_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "conv1_bn_recompute_forward: B=%d H=%d W=%d Cin=%d Cout=%d (all must be >= 1)",
               B, H, W, Cin, Cout);
  BnGeom g;
  CA_CHECK_ARG(coattn_conv1_bn_exact_supported(B, H, W, Cin, Cout, pool, dtype) && bn_exact_geometry(B, H, W, Cout, dtype, &g),
               "conv1_bn_recompute_forward: B=%d H=%d W=%d Cin=%d Cout=%d pool=%d dtype=%d is not a covered shape "
               "(coattn_conv1_bn_exact_supported)", B, H, W, Cin, Cout, pool, dtype);
  CA_CHECK_ARG(image && weight && gamma && beta && running_mean && running_var && y && save_mean && save_invstd && ws,
               "conv1_bn_recompute_forward: a null image / weight / gamma / beta / running_mean / running_var / y / save_mean / "
               "save_invstd / ws");
  CA_CHECK_ARG(((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(gamma) |
                 reinterpret_cast<uintptr_t>(beta) | reinterpret_cast<uintptr_t>(running_mean) |
                 reinterpret_cast<uintptr_t>(running_var) | reinterpret_cast<uintptr_t>(save_mean) |
                 reinterpret_cast<uintptr_t>(save_invstd)) & 15) == 0 &&
                   ((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(weight)) & 3) == 0,
               "conv1_bn_recompute_forward: y, ws, the BatchNorm vectors must be 16-byte aligned, image and weight 4-byte aligned");
  CA_CHECK_ARG(momentum >= 0.0 && momentum <= 1.0, "conv1_bn_recompute_forward: momentum %g outside [0, 1]", momentum);
  CA_CHECK_ARG(eps > 0.0, "conv1_bn_recompute_forward: eps %g (must be > 0)", eps);
  CA_CHECK_ARG(y != image, "conv1_bn_recompute_forward: image and y must be two buffers");
  hipStream_t s = (hipStream_t)stream;
  // pass A: the statistics of the convolution, which is not stored
  launch_conv1(kConv1PairDistance, image, weight, nullptr, ws, g, B, H, W, s);
  CA_CHECK_LAUNCH("conv1_stats_miopen");
  prof_mark(s, "conv1_stats");
  const int64_t pixels = (int64_t)B * H * W;
  const float n_f = (float)pixels;
  const float inhw = (float)(1.0 / (double)pixels), unbias = pixels == 1 ? 1.f : n_f / (n_f - 1.f);   // (as exact_tail)
  const int c4 = Cout / 4;
  hipLaunchKernelGGL(bn_finalize_miopen_kernel, dim3(c4 / g.f0), dim3(g.f0, g.f1, g.f2),
                     (size_t)2 * g.f0 * g.f1 * g.f2 * sizeof(f32x4), s, (const f32x4*)ws, g, c4, inhw, unbias, (float)momentum,
                     (float)eps, (f32x4*)running_mean, (f32x4*)running_var, (f32x4*)save_mean, (f32x4*)save_invstd);
  CA_CHECK_LAUNCH("bn_finalize_miopen");
  prof_mark(s, "conv1_finalize");
  // pass B: the convolution again, normalised (+ pooled) + ReLU
  const int chunks = (B + kConv1NormChunk - 1) / kConv1NormChunk;
  if (pool) {
    const int cbs = (W / 2 + 7) / 8;
    hipLaunchKernelGGL((conv1_norm_pool_kernel<kConv1PairDistance, true>), dim3((unsigned)((H / 2) * cbs), chunks), dim3(64), 0, s,
                       (const float*)image, (const float*)weight, (const float*)save_mean, (const float*)save_invstd,
                       (const float*)gamma, (const float*)beta, (float*)y, B, H, W, cbs);
  } else {
    hipLaunchKernelGGL((conv1_norm_pool_kernel<kConv1PairDistance, false>), dim3((H * W + kConv1Pixels - 1) / kConv1Pixels, chunks),
                       dim3(64), 0, s, (const float*)image, (const float*)weight, (const float*)save_mean,
                       (const float*)save_invstd, (const float*)gamma, (const float*)beta, (float*)y, B, H, W, 0);
  }
  CA_CHECK_LAUNCH("conv1_norm_pool");
  prof_mark(s, "conv1_norm_pool");
  return 0;
}

extern "C" int coattn_conv1_probe(const void* image, const void* weight, void* x, void* ws, int B, int H, int W, int order, int step,
                                  int halves, int skip, void* stream) {
  BnGeom g;
  CA_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && bn_exact_geometry(B, H, W, 64, COATTN_F32, &g),
               "conv1_probe: B=%d H=%d W=%d is not a covered shape (coattn_conv1_bn_exact_supported)", B, H, W);
  CA_CHECK_ARG(image && weight && x && ws && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
               "conv1_probe: a null or misaligned image / weight / x / ws");
  CA_CHECK_ARG(order >= -2 && order <= 13 && (step == 0 || step == 1) && (halves == 1 || halves == 2) && (skip == 0 || skip == 1),
               "conv1_probe: order=%d step=%d halves=%d skip=%d", order, step, halves, skip);
  hipStream_t s = (hipStream_t)stream;
  if (order < 0) {
    launch_conv1(order == -1 ? 8 : 4, image, weight, x, ws, g, B, H, W, s);
  } else {
    const int64_t total = (int64_t)B * H * W * 64;
    hipLaunchKernelGGL(conv1_probe_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)image,
                       (const float*)weight, (float*)x, total, H, W, order, step, halves, skip);
  }
  CA_CHECK_LAUNCH("conv1_probe");
  return 0;
}

// ---- eval mode: running statistics, the whole map in one launch (v0.24.0; include/coattn_ext.h) --------------------------------
namespace {

// The slow probe of tools/probe_encoder_eval.py: one thread per element of x, no pool, every choice of the candidate space switchable.
//   rsqrt   : eval_rsqrt's candidates 0 .. 3
//   step    : 0 fma(gamma, (x - mean) * invstd, beta)   1 the same with a rounded product and a separate add
//   eps_mode: 0 var + (float)eps in fp32   1 (float)((double)var + eps)
__device__ __noinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
  const float prod = a * b;
  return prod + c;
}
__global__ __launch_bounds__(256) void bn_eval_probe_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ running_mean,
                                                            const float* __restrict__ running_var, double eps, float* __restrict__ y,
                                                            int64_t total, int C, int rsqrt, int step, int eps_mode) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const float a = __builtin_fabsf(eps_mode ? (float)((double)running_var[c] + eps) : running_var[c] + (float)eps);
  const float inv = rsqrt == 0 ? eval_rsqrt<0>(a) : rsqrt == 1 ? eval_rsqrt<1>(a) : rsqrt == 2 ? eval_rsqrt<2>(a) : eval_rsqrt<3>(a);
  const float xhat = __fmul_rn(__fsub_rn(x[i], running_mean[c]), inv);
  y[i] = step == 0 ? __builtin_fmaf(gamma[c], xhat, beta[c]) : mul_then_add(gamma[c], xhat, beta[c]);
}

inline bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15) == 0;
}

template <bool POOL>
void launch_bn_eval(const void* x, const void* conv_bias, const void* gamma, const void* beta, const void* running_mean,
                    const void* running_var, float eps, void* y, int H, int W, int C, int64_t total4, int relu, unsigned blocks,
                    hipStream_t s) {
  const int shift = log2_exact(C / 4);
  if (conv_bias)
    hipLaunchKernelGGL((bn_relu_pool_kernel<POOL, true, true, 2>), dim3(blocks), dim3(kThreads), 0, s, (const f32x4*)x,
                       (const float*)running_mean, (const float*)running_var, (const float*)gamma, (const float*)beta, (f32x4*)y, H,
                       W, C, shift, total4, relu, (const float*)conv_bias, eps);
  else
    hipLaunchKernelGGL((bn_relu_pool_kernel<POOL, true, true, 1>), dim3(blocks), dim3(kThreads), 0, s, (const f32x4*)x,
                       (const float*)running_mean, (const float*)running_var, (const float*)gamma, (const float*)beta, (f32x4*)y, H,
                       W, C, shift, total4, relu, (const float*)nullptr, eps);
}

template <bool POOL>
void launch_conv1_eval(const void* image, const void* weight, const void* conv_bias, const void* gamma, const void* beta,
                       const void* running_mean, const void* running_var, float eps, void* y, int B, int H, int W, dim3 grid, int cbs,
                       hipStream_t s) {
  if (conv_bias)
    hipLaunchKernelGGL((conv1_norm_pool_kernel<kConv1PairDistance, POOL, 2>), grid, dim3(64), 0, s, (const float*)image,
                       (const float*)weight, (const float*)running_mean, (const float*)running_var, (const float*)gamma,
                       (const float*)beta, (float*)y, B, H, W, cbs, (const float*)conv_bias, eps);
  else
    hipLaunchKernelGGL((conv1_norm_pool_kernel<kConv1PairDistance, POOL, 1>), grid, dim3(64), 0, s, (const float*)image,
                       (const float*)weight, (const float*)running_mean, (const float*)running_var, (const float*)gamma,
                       (const float*)beta, (float*)y, B, H, W, cbs, (const float*)nullptr, eps);
}

}  // namespace

extern "C" int coattn_bn_eval_supported(int B, int H, int W, int C, int pool, int dtype) {
  return coattn_bn_supported(B, H, W, C, pool, dtype);
}

extern "C" int coattn_bn_eval_forward(const void* x, const void* conv_bias, const void* gamma, const void* beta,
                                      const void* running_mean, const void* running_var, double eps, void* y, int B, int H, int W,
                                      int C, int pool, int relu, int dtype, void* stream) {
  CA_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1 && coattn_bn_eval_supported(B, H, W, C, pool, dtype),
               "bn_eval_forward: B=%d H=%d W=%d C=%d pool=%d dtype=%d is not supported (coattn_bn_eval_supported)", B, H, W, C, pool,
               dtype);
  CA_CHECK_ARG(x && gamma && beta && running_mean && running_var && y,
               "bn_eval_forward: a null x / gamma / beta / running_mean / running_var / y");
  CA_CHECK_ARG(aligned16({x, conv_bias, gamma, beta, running_mean, running_var, y}),
               "bn_eval_forward: every pointer must be 16-byte aligned");
  CA_CHECK_ARG(x != y, "bn_eval_forward: y must not be x");
  CA_CHECK_ARG(eps > 0.0, "bn_eval_forward: eps %g (must be > 0)", eps);
  hipStream_t s = (hipStream_t)stream;
  const int64_t out_pixels = pool ? (int64_t)B * (H / 2) * (W / 2) : (int64_t)B * H * W;
  const int64_t total4 = out_pixels * (C / 4);
  const int per_thread = pool ? 2 : 4;
  int64_t blocks = (total4 + (int64_t)kThreads * per_thread - 1) / ((int64_t)kThreads * per_thread);
  if (blocks > kMaxNormBlocks) blocks = kMaxNormBlocks;
  if (pool)
    launch_bn_eval<true>(x, conv_bias, gamma, beta, running_mean, running_var, (float)eps, y, H, W, C, total4, relu, (unsigned)blocks, s);
  else
    launch_bn_eval<false>(x, conv_bias, gamma, beta, running_mean, running_var, (float)eps, y, H, W, C, total4, relu, (unsigned)blocks, s);
  CA_CHECK_LAUNCH("bn_eval");
  prof_mark(s, "bn_eval");
  return 0;
}

extern "C" int coattn_conv1_bn_eval_supported(int B, int H, int W, int Cin, int Cout, int pool, int dtype) {
  if (Cin != 3 || Cout != 64 || !coattn_bn_eval_supported(B, H, W, Cout, pool, dtype)) return 0;
  // the kernel's 32-bit indices: byte offsets into one image sample, and a grid row of sample chunks
  return (int64_t)H * W * 12 < ((int64_t)1 << 29) && (B + kConv1NormChunk - 1) / kConv1NormChunk <= 65535 ? 1 : 0;
}

extern "C" int coattn_conv1_bn_eval_forward(const void* image, const void* weight, const void* conv_bias, const void* gamma,
                                            const void* beta, const void* running_mean, const void* running_var, double eps, void* y,
                                            int B, int H, int W, int Cin, int Cout, int pool, int dtype, void* stream) {
  CA_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && coattn_conv1_bn_eval_supported(B, H, W, Cin, Cout, pool, dtype),
               "conv1_bn_eval_forward: B=%d H=%d W=%d Cin=%d Cout=%d pool=%d dtype=%d is not supported "
               "(coattn_conv1_bn_eval_supported)", B, H, W, Cin, Cout, pool, dtype);
  CA_CHECK_ARG(image && weight && gamma && beta && running_mean && running_var && y,
               "conv1_bn_eval_forward: a null image / weight / gamma / beta / running_mean / running_var / y");
  CA_CHECK_ARG(aligned16({y, conv_bias, gamma, beta, running_mean, running_var}) &&
                   ((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(weight)) & 3) == 0,
               "conv1_bn_eval_forward: y, conv_bias and the BatchNorm vectors must be 16-byte aligned, image and weight 4-byte aligned");
  CA_CHECK_ARG(y != image, "conv1_bn_eval_forward: image and y must be two buffers");
  CA_CHECK_ARG(eps > 0.0, "conv1_bn_eval_forward: eps %g (must be > 0)", eps);
  hipStream_t s = (hipStream_t)stream;
  const int chunks = (B + kConv1NormChunk - 1) / kConv1NormChunk;
  if (pool) {
    const int cbs = (W / 2 + 7) / 8;
    launch_conv1_eval<true>(image, weight, conv_bias, gamma, beta, running_mean, running_var, (float)eps, y, B, H, W,
                            dim3((unsigned)((H / 2) * cbs), chunks), cbs, s);
  } else {
    launch_conv1_eval<false>(image, weight, conv_bias, gamma, beta, running_mean, running_var, (float)eps, y, B, H, W,
                             dim3((unsigned)((H * W + kConv1Pixels - 1) / kConv1Pixels), chunks), 0, s);
  }
  CA_CHECK_LAUNCH("conv1_bn_eval");
  prof_mark(s, "conv1_bn_eval");
  return 0;
}

extern "C" int coattn_bn_eval_probe(const void* x, const void* gamma, const void* beta, const void* running_mean,
                                    const void* running_var, double eps, void* y, int B, int H, int W, int C, int rsqrt, int step,
                                    int eps_mode, void* stream) {
  CA_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1 && (int64_t)B * H * W * C < ((int64_t)1 << 31), "bn_eval_probe: B=%d H=%d W=%d C=%d",
               B, H, W, C);
  CA_CHECK_ARG(x && gamma && beta && running_mean && running_var && y && x != y, "bn_eval_probe: a null pointer, or y is x");
  CA_CHECK_ARG(rsqrt >= 0 && rsqrt <= 3 && (step == 0 || step == 1) && (eps_mode == 0 || eps_mode == 1),
               "bn_eval_probe: rsqrt=%d step=%d eps_mode=%d", rsqrt, step, eps_mode);
  const int64_t total = (int64_t)B * H * W * C;
  hipLaunchKernelGGL(bn_eval_probe_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                     (const float*)gamma, (const float*)beta, (const float*)running_mean, (const float*)running_var, eps, (float*)y,
                     total, C, rsqrt, step, eps_mode);
  CA_CHECK_LAUNCH("bn_eval_probe");
  return 0;
}
