// Image preprocessing (include/coattn_ext.h v0.23.0): a batch of decoded uint8 RGB images of different sizes -> the network's
// fp32 [B][3][S][S] input, Pillow's 8-bit bilinear resize bit for bit and a table lookup for ToTensor + Normalize.
//
// One launch.  Workgroup (b, band) -- a flat grid, b = blockIdx.x / bands -- owns COATTN_PREPROCESS_ROWS output rows of image b.
// It reads the image's descriptor and judges it (every workgroup of an image comes to the same verdict; band 0 counts a bad one),
// takes its window of source rows [win_lo, win_hi) from the vertical table, runs the horizontal pass of those rows into LDS as
// uint8 [rows][S][3] -- one thread per (row, x), three channels, every pixel byte a one-byte load: rows are 3 w bytes, aligned to
// nothing -- and then the vertical pass plus lookup out of LDS, one thread per output element, consecutive lanes on consecutive
// addresses of the output (x fastest for planar outputs, the channel fastest where sC == 1).  The intermediate never reaches memory;
// adjacent bands recompute the source rows their windows share.
//
// Integer arithmetic only: the header's sums in int32, an arithmetic shift, a clip.  No float operation, so nothing to contract.
#include "common.h"

#include "../../include/coattn_ext.h"

#include <limits.h>

namespace {

constexpr int kThreads = COATTN_PREPROCESS_THREADS, kBand = COATTN_PREPROCESS_ROWS;
constexpr int kMaxS = COATTN_PREPROCESS_MAX_S, kMaxIn = COATTN_PREPROCESS_MAX_IN, kMaxTaps = COATTN_PREPROCESS_MAX_TAPS;
constexpr int kLutBytes = 3 * 256 * (int)sizeof(float);      // the lookup table leads the dynamic region: a multiple of 16
constexpr size_t kLdsMax = 160 * 1024;
constexpr int kHalf = 1 << 21, kShift = 22;

struct Args {
  const unsigned char* pixels;
  long long pixel_bytes;
  const coattn_preprocess_desc* desc;
  const int* coef;
  long long coef_count;
  const float* lut;
  float* out;
  long long sB, sC, sH, sW;
  int* bad;
  int B, S, max_h, max_w, lds_rows;
};

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// lo and the tap count of one table row, clamped into [0, in): lo + n <= in, n <= taps (a well-formed table is left as it is)
__device__ __forceinline__ void span(const int* __restrict__ row, int taps, int in, int& lo, int& n) {
  lo = row[0];
  n = row[1];
  lo = lo < 0 ? 0 : (lo > in - 1 ? in - 1 : lo);
  const int room = in - lo < taps ? in - lo : taps;
  n = n < 0 ? 0 : (n > room ? room : n);
}

__device__ __forceinline__ bool table_ok(int tab, int taps, int S, long long coef_count) {
  return taps >= 1 && taps <= kMaxTaps && tab >= 0 && (long long)tab + (long long)S * (2 + taps) <= coef_count;
}

__device__ __forceinline__ void zero_band(const Args& a, int b, int y0, int ny) {
  const int S = a.S, units = ny * S * 3;
  for (int u = threadIdx.x; u < units; u += kThreads) {
    const int x = u % S, rest = u / S, c = rest % 3, y = y0 + rest / 3;
    a.out[b * a.sB + c * a.sC + y * a.sH + x * a.sW] = 0.0f;
  }
}

__global__ __launch_bounds__(kThreads) void preprocess_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* s_lut = reinterpret_cast<float*>(smem);             // [3][256]
  unsigned char* s_t = smem + kLutBytes;                     // [win_n][S][3]: the horizontal pass of the band's source rows

  const int S = a.S, bands = (S + kBand - 1) / kBand;
  const int b = blockIdx.x / bands, band = blockIdx.x - b * bands;
  const int tid = threadIdx.x;
  const int y0 = band * kBand;
  const int ny = S - y0 < kBand ? S - y0 : kBand;

  const coattn_preprocess_desc d = a.desc[b];
  const int h = d.h, w = d.w;
  bool ok = h >= 1 && h <= a.max_h && w >= 1 && w <= a.max_w && d.offset >= 0;
  if (ok) {
    const long long bytes = 3ll * h * w;                     // (h, w <= 8192: no overflow)
    ok = bytes <= a.pixel_bytes && d.offset <= a.pixel_bytes - bytes;
  }
  ok = ok && table_ok(d.tab_x, d.taps_x, S, a.coef_count) && table_ok(d.tab_y, d.taps_y, S, a.coef_count);
  if (!ok) {
    zero_band(a, b, y0, ny);
    if (band == 0 && tid == 0 && a.bad) atomicAdd(a.bad, 1);
    return;
  }

  const int* __restrict__ tx = a.coef + d.tab_x;
  const int* __restrict__ ty = a.coef + d.tab_y;
  const int rx = 2 + d.taps_x, ry = 2 + d.taps_y;
  int win_lo = INT_MAX, win_hi = 0;
  for (int i = 0; i < ny; ++i) {                             // (uniform: every thread reads the same <= 16 rows)
    int lo, n;
    span(ty + (y0 + i) * ry, d.taps_y, h, lo, n);
    win_lo = lo < win_lo ? lo : win_lo;
    win_hi = lo + n > win_hi ? lo + n : win_hi;
  }
  const int win_n = win_hi - win_lo;
  if (win_n > a.lds_rows) {                                  // a table that is not the header's for (h, S): nothing is staged
    zero_band(a, b, y0, ny);
    if (tid == 0 && a.bad) atomicAdd(a.bad, 1);
    return;
  }

  for (int i = tid; i < 768; i += kThreads) s_lut[i] = a.lut[i];

  // horizontal pass: source rows win_lo .. win_hi - 1, every output column
  const unsigned char* __restrict__ src = a.pixels + d.offset;
  const int units_h = win_n > 0 ? win_n * S : 0;
  for (int u = tid; u < units_h; u += kThreads) {
    const int r = u / S, x = u - r * S;
    const int* __restrict__ row = tx + x * rx;
    int lo, n;
    span(row, d.taps_x, w, lo, n);
    const unsigned char* __restrict__ p = src + ((size_t)(win_lo + r) * w + lo) * 3;
    int s0 = kHalf, s1 = kHalf, s2 = kHalf;
    for (int j = 0; j < n; ++j) {
      const int k = row[2 + j];
      s0 += k * (int)p[3 * j];
      s1 += k * (int)p[3 * j + 1];
      s2 += k * (int)p[3 * j + 2];
    }
    unsigned char* t = s_t + (size_t)u * 3;
    t[0] = (unsigned char)clip8(s0 >> kShift);
    t[1] = (unsigned char)clip8(s1 >> kShift);
    t[2] = (unsigned char)clip8(s2 >> kShift);
  }
  __syncthreads();

  // vertical pass and lookup: the band's ny rows
  const bool channel_fast = a.sC == 1;
  const int units_v = ny * S * 3, pitch = S * 3;
  for (int u = tid; u < units_v; u += kThreads) {
    int x, c, i;
    if (channel_fast) {
      c = u % 3;
      const int rest = u / 3;
      i = rest / S;
      x = rest - i * S;
    } else {
      const int rest = u / S;
      x = u - rest * S;
      i = rest / 3;
      c = rest - i * 3;
    }
    const int y = y0 + i;
    const int* __restrict__ row = ty + y * ry;
    int lo, n;
    span(row, d.taps_y, h, lo, n);
    const unsigned char* __restrict__ t = s_t + (size_t)(lo - win_lo) * pitch + x * 3 + c;
    int s = kHalf;
    for (int j = 0; j < n; ++j) s += row[2 + j] * (int)t[(size_t)j * pitch];
    a.out[b * a.sB + c * a.sC + y * a.sH + x * a.sW] = s_lut[c * 256 + clip8(s >> kShift)];
  }
}

long long band_count(int S) { return (S + kBand - 1) / kBand; }

// the tallest window of source rows a band can have for any h <= max_h (include/coattn_ext.h): lo > center - support - 0.5 and
// hi <= center + support + 0.5, so hi(y0 + ROWS - 1) - lo(y0) < (ROWS - 1) s + 2 max(s, 1) + 1, which grows with h
int window_rows(int S, int max_h) {
  const double s = (double)max_h / (double)S, fs = s > 1.0 ? s : 1.0;
  const long long rows = (long long)((kBand - 1) * s + 2.0 * fs + 1.0) + 1;
  return (int)(rows < max_h ? rows : max_h);
}

size_t lds_bytes(int S, int rows) { return (size_t)kLutBytes + (((size_t)rows * S * 3 + 15) & ~(size_t)15); }

bool shape_ok(int B, int S, int max_h, int max_w) {
  if (B < 1 || S < 1 || S > kMaxS || max_h < 1 || max_h > kMaxIn || max_w < 1 || max_w > kMaxIn) return false;
  if (lds_bytes(S, window_rows(S, max_h)) > kLdsMax) return false;
  return (long long)B * band_count(S) <= 0x7fffffffll;
}

bool al(const void* p, uintptr_t n) { return (((uintptr_t)p) & (n - 1)) == 0; }

}  // namespace

extern "C" int coattn_preprocess_supported(int B, int S, int max_h, int max_w) { return shape_ok(B, S, max_h, max_w) ? 1 : 0; }

extern "C" int coattn_preprocess_images(const void* pixels, long long pixel_bytes, const void* desc, const void* coef,
                                        long long coef_count, const void* lut, void* out, int64_t sB, int64_t sC, int64_t sH,
                                        int64_t sW, int32_t* bad_images, int B, int S, int max_h, int max_w, void* stream) {
  const char* what = "preprocess_images";
  CA_CHECK_ARG(shape_ok(B, S, max_h, max_w), "%s: shape B=%d S=%d max_h=%d max_w=%d not supported (B >= 1, 1 <= S <= %d, 1 <= "
               "max_h, max_w <= %d, the band's window of source rows within the 160 KiB of LDS: coattn_preprocess_supported)", what,
               B, S, max_h, max_w, kMaxS, kMaxIn);
  CA_CHECK_ARG(pixels && desc && coef && lut && out, "%s: null pixels, desc, coef, lut or out", what);
  CA_CHECK_ARG(pixel_bytes >= 1 && coef_count >= 1, "%s: pixel_bytes %lld and coef_count %lld must be positive", what, pixel_bytes,
               coef_count);
  CA_CHECK_ARG(al(desc, 8) && al(coef, 4) && al(lut, 4) && al(out, 4) && al(bad_images, 4), "%s: desc must be 8-byte aligned, coef, "
               "lut, out and bad_images 4-byte aligned", what);
  Args a;
  a.pixels = (const unsigned char*)pixels, a.pixel_bytes = pixel_bytes;
  a.desc = (const coattn_preprocess_desc*)desc, a.coef = (const int*)coef, a.coef_count = coef_count;
  a.lut = (const float*)lut, a.out = (float*)out, a.sB = sB, a.sC = sC, a.sH = sH, a.sW = sW, a.bad = (int*)bad_images;
  a.B = B, a.S = S, a.max_h = max_h, a.max_w = max_w, a.lds_rows = window_rows(S, max_h);
  const size_t lds = lds_bytes(S, a.lds_rows);
  static DeviceOnce once;
  if (lds > 48 * 1024)                                       // (the runtime's default limit on dynamic LDS lies above this)
    CA_TRY(once.run([&] {
      return hipFuncSetAttribute(reinterpret_cast<const void*>(preprocess_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)kLdsMax);
    }, what));
  const dim3 grid((unsigned)((long long)B * band_count(S))), block(kThreads);
  hipLaunchKernelGGL(preprocess_kernel, grid, block, lds, (hipStream_t)stream, a);
  CA_CHECK_LAUNCH(what);
  prof_mark((hipStream_t)stream, what);
  return 0;
}
