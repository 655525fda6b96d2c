// Attention overlays (include/coattn.h v0.21.0): the maps coattn_infer writes, upsampled over the image they were computed from and
// blended into it, as uint8 pictures [B][L+1][H+strip_h][W][3] -- panel 0 the de-normalised image, panel 1+l level l, under each
// level's panel a strip of the question attention.
//
// One launch.  Workgroup (b, band) -- a flat grid, b = blockIdx.x / bands -- owns COATTN_OVERLAY_ROWS output rows of sample b for
// every panel: it reads its band of the image once and writes L+1 bands.  It first loads the sample's L maps into LDS, finds
// their maxima (and those of the a_q rows, when its band reaches into the strip) and scales the maps in place; a bad map becomes
// zeros there and is counted by the band-0 workgroup.  A thread then takes 4 neighbouring pixels of a row at a time: one
// 16-byte load per channel of a contiguous image (scalar loads at any other strides), 12 bytes = 3 whole dwords per panel out.
//
// The arithmetic is the header's, operation by operation: every product, sum and the one division are separate correctly
// rounded fp32 operations, so nothing in this file may contract into an FMA.
#pragma clang fp contract(off)
#include "common.h"

#include <float.h>

namespace {

constexpr int kThreads = COATTN_OVERLAY_THREADS, kRows = COATTN_OVERLAY_ROWS;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxL = 8, kMaxG = 64, kMaxHW = 4096, kMaxStrip = 4096;
constexpr size_t kLdsMax = (size_t)kMaxL * kMaxG * kMaxG * sizeof(float);      // the maps of one sample at the largest shape

typedef unsigned int u32x3 __attribute__((ext_vector_type(3), aligned(4)));

struct Args {
  const float* image;
  long long sB, sC, sH, sW;
  const float* a_v;
  const float* a_q;
  const int* q_len;
  const float* lut;
  unsigned char* out;
  int* bad;
  float mean[3], std[3], alpha, floor;
  int B, L, H, W, Gh, Gw, T, strip_h;
};

__device__ __forceinline__ float clamp01(float x) { return x >= 0.0f ? (x <= 1.0f ? x : 1.0f) : 0.0f; }      // NaN -> 0

__device__ __forceinline__ unsigned to_byte(float o) { return (unsigned)(int)(clamp01(o) * 255.0f + 0.5f); }

// source cell pair and weights of output coordinate `y` along an axis of G cells scaled by s = (float)G / (float)extent
__device__ __forceinline__ void axis(int y, float s, int G, int& i0, int& i1, float& w0, float& w1) {
  float src = ((float)y + 0.5f) * s - 0.5f;
  src = src > 0.0f ? src : 0.0f;
  const int f = (int)src;                                    // src >= 0: the truncation is the floor
  i0 = f < G - 1 ? f : G - 1;
  i1 = i0 + 1 < G - 1 ? i0 + 1 : G - 1;
  w1 = src - (float)i0;
  w0 = 1.0f - w1;
}

__device__ __forceinline__ void store12(unsigned char* o, const unsigned (&c)[12]) {
  u32x3 v;
  v.x = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
  v.y = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
  v.z = c[8] | (c[9] << 8) | (c[10] << 16) | (c[11] << 24);
  *reinterpret_cast<u32x3*>(o) = v;
}

// the largest of this thread's entries of a[0..n) (0 when it has none) and whether one of them is NaN, infinite or negative,
// reduced over the wave
__device__ __forceinline__ void wave_max(float mx, int bad, float& wmx, int& wbad) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float other = __shfl_xor(mx, o);
    mx = other > mx ? other : mx;
  }
  wmx = mx;
  wbad = __any(bad);
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(kThreads) void overlay_kernel(const Args a) {
  extern __shared__ float s_map[];                           // [L][Gh*Gw]: raw, then scaled by the reciprocal maximum
  __shared__ float s_lut[MODE == COATTN_OVERLAY_HEAT ? 768 : 1];
  __shared__ float s_wmx[2 * kMaxL][kWaves];
  __shared__ int s_wbad[2 * kMaxL][kWaves];
  __shared__ float s_r[2 * kMaxL];                           // [l]: a_v's reciprocal maximum, [kMaxL + l]: a_q's
  __shared__ int s_bad[2 * kMaxL];

  const int L = a.L, H = a.H, W = a.W, Gh = a.Gh, Gw = a.Gw, T = a.T;
  const int G = Gh * Gw, rows_all = H + a.strip_h;
  const int bands = (rows_all + kRows - 1) / kRows;
  const int b = blockIdx.x / bands, band = blockIdx.x - b * bands;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int y0 = band * kRows;
  const int rows = rows_all - y0 < kRows ? rows_all - y0 : kRows;
  const bool want_v = y0 < H;                                // (band 0 always does)
  const bool want_q = a.strip_h > 0 && (band == 0 || y0 + rows > H);
  int len = T;
  if (want_q && a.q_len) {
    len = a.q_len[b];
    len = len < 1 ? 1 : (len > T ? T : len);
  }

  if (MODE == COATTN_OVERLAY_HEAT)
    for (int i = tid; i < 768; i += kThreads) s_lut[i] = a.lut[i];
  for (int l = 0; l < L; ++l) {
    if (want_v) {
      const float* __restrict__ src = a.a_v + ((size_t)l * a.B + b) * G;
      float mx = 0.0f;
      int bad = 0;
      for (int n = tid; n < G; n += kThreads) {
        const float v = src[n];
        s_map[l * G + n] = v;
        bad |= !(v >= 0.0f && v <= FLT_MAX);
        mx = v > mx ? v : mx;
      }
      float wmx;
      int wbad;
      wave_max(mx, bad, wmx, wbad);
      if ((tid & 63) == 0) s_wmx[l][wave] = wmx, s_wbad[l][wave] = wbad;
    }
    if (want_q) {
      const float* __restrict__ src = a.a_q + ((size_t)l * a.B + b) * T;
      float mx = 0.0f;
      int bad = 0;
      for (int t = tid; t < len; t += kThreads) {
        const float v = src[t];
        bad |= !(v >= 0.0f && v <= FLT_MAX);
        mx = v > mx ? v : mx;
      }
      float wmx;
      int wbad;
      wave_max(mx, bad, wmx, wbad);
      if ((tid & 63) == 0) s_wmx[kMaxL + l][wave] = wmx, s_wbad[kMaxL + l][wave] = wbad;
    }
  }
  __syncthreads();
  if (tid < 2 * kMaxL) {
    const int l = tid & (kMaxL - 1);
    const bool mine = l < L && (tid < kMaxL ? want_v : want_q);
    if (mine) {
      float mx = s_wmx[tid][0];
      int bad = s_wbad[tid][0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        mx = s_wmx[tid][w] > mx ? s_wmx[tid][w] : mx;
        bad |= s_wbad[tid][w];
      }
      const float r = 1.0f / mx;                             // (correctly rounded; a denormal maximum may overflow it)
      bad |= mx == 0.0f || !(r <= FLT_MAX);
      s_r[tid] = bad ? 0.0f : r;
      s_bad[tid] = bad;
      if (bad && band == 0 && a.bad) atomicAdd(a.bad, 1);
    }
  }
  __syncthreads();
  if (want_v) {
    for (int l = 0; l < L; ++l) {
      const float r = s_r[l];
      const int bad = s_bad[l];
      for (int n = tid; n < G; n += kThreads) s_map[l * G + n] = bad ? 0.0f : s_map[l * G + n] * r;
    }
  }
  __syncthreads();

  const int W4 = W >> 2, units = rows * W4;
  const size_t panel = (size_t)rows_all * W * 3;             // bytes of one panel
  const float sy = (float)Gh / (float)H, sx = (float)Gw / (float)W;
  const float omf = 1.0f - a.floor, oma = 1.0f - a.alpha;
  for (int u = tid; u < units; u += kThreads) {
    const int ry = u / W4, x = (u - ry * W4) << 2, y = y0 + ry;
    unsigned char* o = a.out + (size_t)b * (L + 1) * panel + ((size_t)y * W + x) * 3;
    unsigned c12[12];
    if (y < H) {
      float xh[3][4];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* p = a.image + b * a.sB + c * a.sC + y * a.sH;
        float px[4];
        if (VEC) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(p + x);
          px[0] = v.x, px[1] = v.y, px[2] = v.z, px[3] = v.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) px[i] = p[(x + i) * a.sW];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) xh[c][i] = clamp01(px[i] * a.std[c] + a.mean[c]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) c12[i * 3 + c] = to_byte(xh[c][i]);
      store12(o, c12);
      int i0, i1, j0[4], j1[4];
      float wy0, wy1, wx0[4], wx1[4];
      axis(y, sy, Gh, i0, i1, wy0, wy1);
#pragma unroll
      for (int i = 0; i < 4; ++i) axis(x + i, sx, Gw, j0[i], j1[i], wx0[i], wx1[i]);
      for (int l = 0; l < L; ++l) {
        const float* __restrict__ m0 = s_map + l * G + i0 * Gw;
        const float* __restrict__ m1 = s_map + l * G + i1 * Gw;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float top = m0[j0[i]] * wx0[i] + m0[j1[i]] * wx1[i];
          const float bot = m1[j0[i]] * wx0[i] + m1[j1[i]] * wx1[i];
          const float up = top * wy0 + bot * wy1;
          if (MODE == COATTN_OVERLAY_MASK) {
            const float g = a.floor + omf * up;
#pragma unroll
            for (int c = 0; c < 3; ++c) c12[i * 3 + c] = to_byte(xh[c][i] * g);
          } else {
            const int k = (int)(up * 255.0f + 0.5f);
#pragma unroll
            for (int c = 0; c < 3; ++c) c12[i * 3 + c] = to_byte(oma * xh[c][i] + a.alpha * s_lut[k * 3 + c]);
          }
        }
        store12(o + (size_t)(1 + l) * panel, c12);
      }
    } else {                                                 // the strip: zeros under the image, T cells under a level
#pragma unroll
      for (int i = 0; i < 12; ++i) c12[i] = 0u;
      store12(o, c12);
      for (int l = 0; l < L; ++l) {
        const float* __restrict__ q = a.a_q + ((size_t)l * a.B + b) * T;
        const float r = s_r[kMaxL + l];
        const int bad = s_bad[kMaxL + l];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = (int)(((unsigned)(x + i) * (unsigned)T) / (unsigned)W);
          if (t < len) {
            const float mq = bad ? 0.0f : q[t] * r;
            if (MODE == COATTN_OVERLAY_MASK) {
              const unsigned g = to_byte(mq);
              c12[i * 3] = c12[i * 3 + 1] = c12[i * 3 + 2] = g;
            } else {
              const int k = (int)(mq * 255.0f + 0.5f);
#pragma unroll
              for (int c = 0; c < 3; ++c) c12[i * 3 + c] = to_byte(s_lut[k * 3 + c]);
            }
          } else {
            c12[i * 3] = c12[i * 3 + 1] = c12[i * 3 + 2] = 0u;
          }
        }
        store12(o + (size_t)(1 + l) * panel, c12);
      }
    }
  }
}

bool mode_ok(int mode) { return mode == COATTN_OVERLAY_HEAT || mode == COATTN_OVERLAY_MASK; }

long long band_count(int H, int strip_h) { return ((long long)H + strip_h + kRows - 1) / kRows; }

bool shape_ok(int B, int L, int H, int W, int Gh, int Gw, int T, int strip_h, int mode) {
  if (!mode_ok(mode) || B < 1 || L < 1 || L > kMaxL || H < 1 || H > kMaxHW || W < 1 || W > kMaxHW || (W & 3)) return false;
  if (Gh < 1 || Gh > kMaxG || Gw < 1 || Gw > kMaxG || strip_h < 0 || strip_h > kMaxStrip) return false;
  if (strip_h > 0 && (T < 1 || T > W)) return false;         // (W <= 4096 already)
  return (long long)B * band_count(H, strip_h) <= 0x7fffffffll;
}

bool al(const void* p, uintptr_t n) { return (((uintptr_t)p) & (n - 1)) == 0; }

template <int MODE, bool VEC>
int launch(const Args& a, size_t lds, hipStream_t s, const char* what) {
  static DeviceOnce once;
  if (lds > 48 * 1024)                                       // (the runtime's default limit on dynamic LDS lies above this)
    CA_TRY(once.run([&] {
      return hipFuncSetAttribute(reinterpret_cast<const void*>(overlay_kernel<MODE, VEC>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
    }, what));
  const dim3 grid((unsigned)((long long)a.B * band_count(a.H, a.strip_h))), block(kThreads);
  hipLaunchKernelGGL((overlay_kernel<MODE, VEC>), grid, block, lds, s, a);
  return 0;
}

}  // namespace

extern "C" int coattn_overlay_supported(int B, int L, int H, int W, int Gh, int Gw, int T, int strip_h, int mode) {
  return shape_ok(B, L, H, W, Gh, Gw, T, strip_h, mode) ? 1 : 0;
}

extern "C" int coattn_overlay_render(const void* image, int64_t sB, int64_t sC, int64_t sH, int64_t sW, const void* a_v,
                                     const void* a_q, const int32_t* q_len, const coattn_overlay_params* p, void* out,
                                     int32_t* bad_maps, int B, int L, int H, int W, int Gh, int Gw, int T, int strip_h, int mode,
                                     void* stream) {
  const char* what = "overlay_render";
  CA_CHECK_ARG(mode_ok(mode), "%s: unsupported mode %d (COATTN_OVERLAY_HEAT or COATTN_OVERLAY_MASK)", what, mode);
  CA_CHECK_ARG(B > 0 && L > 0 && H > 0 && W > 0 && Gh > 0 && Gw > 0, "%s: non-positive size B=%d L=%d H=%d W=%d Gh=%d Gw=%d", what,
               B, L, H, W, Gh, Gw);
  CA_CHECK_ARG(strip_h >= 0, "%s: negative strip_h %d", what, strip_h);
  CA_CHECK_ARG(strip_h == 0 || a_q, "%s: strip_h=%d needs a_q (a NULL a_q takes strip_h = 0)", what, strip_h);
  CA_CHECK_ARG(shape_ok(B, L, H, W, Gh, Gw, T, strip_h, mode), "%s: shape B=%d L=%d H=%d W=%d Gh=%d Gw=%d T=%d strip_h=%d not "
               "supported (L <= 8, H, W, strip_h <= 4096, W a multiple of 4, Gh, Gw <= 64, 1 <= T <= W under a strip, B * bands < "
               "2^31: coattn_overlay_supported)", what, B, L, H, W, Gh, Gw, T, strip_h);
  CA_CHECK_ARG(image && a_v && p && out, "%s: null image, a_v, params or out", what);
  CA_CHECK_ARG(p->alpha >= 0.0f && p->alpha <= 1.0f && p->floor >= 0.0f && p->floor <= 1.0f, "%s: alpha %g and floor %g must lie "
               "in [0, 1]", what, (double)p->alpha, (double)p->floor);
  for (int c = 0; c < 3; ++c) {
    CA_CHECK_ARG(p->std[c] - p->std[c] == 0.0f && p->std[c] != 0.0f, "%s: std[%d] = %g must be finite and non-zero", what, c,
                 (double)p->std[c]);
    CA_CHECK_ARG(p->mean[c] - p->mean[c] == 0.0f, "%s: mean[%d] = %g must be finite", what, c, (double)p->mean[c]);
  }
  CA_CHECK_ARG(mode != COATTN_OVERLAY_HEAT || p->lut, "%s: the heat mode needs params.lut (fp32 [256][3] on the device)", what);
  const bool vec = sW == 1 && !((sB | sC | sH) & 3);         // a contiguous image: 16-byte loads
  CA_CHECK_ARG(al(out, 16) && (vec ? al(image, 16) : al(image, 4)), "%s: out and a contiguous image (sW = 1, the other strides "
               "multiples of 4) must be 16-byte aligned, an image of other strides 4-byte aligned", what);
  CA_CHECK_ARG(al(a_v, 4) && al(a_q, 4) && al(q_len, 4) && al(bad_maps, 4) && al(p->lut, 4), "%s: a_v, a_q, q_len, bad_maps and "
               "params.lut must be 4-byte aligned", what);
  Args a;
  a.image = (const float*)image, a.sB = sB, a.sC = sC, a.sH = sH, a.sW = sW;
  a.a_v = (const float*)a_v, a.a_q = strip_h ? (const float*)a_q : nullptr, a.q_len = (const int*)q_len;
  a.lut = (const float*)p->lut, a.out = (unsigned char*)out, a.bad = (int*)bad_maps;
  for (int c = 0; c < 3; ++c) a.mean[c] = p->mean[c], a.std[c] = p->std[c];
  a.alpha = p->alpha, a.floor = p->floor;
  a.B = B, a.L = L, a.H = H, a.W = W, a.Gh = Gh, a.Gw = Gw, a.T = strip_h ? T : 1, a.strip_h = strip_h;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)L * Gh * Gw * sizeof(float);
  if (mode == COATTN_OVERLAY_HEAT) {
    if (vec) CA_TRY((launch<COATTN_OVERLAY_HEAT, true>(a, lds, s, what)));
    else CA_TRY((launch<COATTN_OVERLAY_HEAT, false>(a, lds, s, what)));
  } else {
    if (vec) CA_TRY((launch<COATTN_OVERLAY_MASK, true>(a, lds, s, what)));
    else CA_TRY((launch<COATTN_OVERLAY_MASK, false>(a, lds, s, what)));
  }
  CA_CHECK_LAUNCH(what);
  prof_mark(s, what);
  return 0;
}
