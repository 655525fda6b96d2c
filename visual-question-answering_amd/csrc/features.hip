// The cached image features' device-side data path (include/coattn.h v0.20.0): out[b] = table[idx[b]] as fp32, the rows of a
// batch gathered from a location-major [S][N][d] table of fp32 or bf16 features that the frozen encoder wrote once.
//
// One launch, no float arithmetic, no atomics on floats.  A row is cut into passes of COATTN_FEATURES_THREADS *
// COATTN_FEATURES_LOADS 16-byte loads; workgroup (b, c) -- a flat grid, b = blockIdx.x / passes -- copies pass c of row idx[b]:
// every thread has its COATTN_FEATURES_LOADS loads in flight before its first store, consecutive lanes take consecutive
// 16-byte vectors.  A bf16 vector holds eight elements and becomes two 16-byte stores: the sixteen bits are the high half of
// the fp32 word, every NaN payload and infinity as stored.  The index is read once per workgroup and compared over all 64
// bits; one outside [0, S) stores zeros, loads nothing and is counted by the workgroup of the row's first pass.
#include "common.h"

namespace {

constexpr int kThreads = COATTN_FEATURES_THREADS, kLoads = COATTN_FEATURES_LOADS;
constexpr int kMaxD = 2048, kMaxN = 4096;
constexpr long long kMaxGrid = (1ll << 24) - 1;              // workgroups of one launch: B * passes per row

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <typename IdT, bool BF16>
__global__ __launch_bounds__(kThreads) void features_gather_kernel(const u32x4* __restrict__ table, const IdT* __restrict__ idx,
                                                                   u32x4* __restrict__ out, int* bad, long long S,
                                                                   unsigned row16, unsigned passes) {
  const unsigned b = blockIdx.x / passes, c = blockIdx.x - b * passes;
  const long long id = idx[b];
  const bool ok = (unsigned long long)id < (unsigned long long)S;      // (all 64 bits of an int64 index; a negative one is huge)
  const unsigned j0 = c * (kThreads * kLoads) + threadIdx.x;           // this thread's first 16-byte vector of the row
  u32x4 v[kLoads];
#pragma unroll
  for (int u = 0; u < kLoads; ++u) v[u] = u32x4{0u, 0u, 0u, 0u};
  if (ok) {
    const u32x4* __restrict__ src = table + (size_t)id * row16;
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const unsigned j = j0 + u * kThreads;
      if (j < row16) v[u] = src[j];
    }
  } else if (c == 0 && threadIdx.x == 0 && bad) {
    atomicAdd(bad, 1);
  }
  u32x4* __restrict__ dst = out + (size_t)b * row16 * (BF16 ? 2 : 1);
#pragma unroll
  for (int u = 0; u < kLoads; ++u) {
    const unsigned j = j0 + u * kThreads;
    if (j >= row16) continue;
    if (BF16) {                                                        // element 2k is the low half of word k
      dst[(size_t)j * 2] = u32x4{v[u].x << 16, v[u].x & 0xffff0000u, v[u].y << 16, v[u].y & 0xffff0000u};
      dst[(size_t)j * 2 + 1] = u32x4{v[u].z << 16, v[u].z & 0xffff0000u, v[u].w << 16, v[u].w & 0xffff0000u};
    } else {
      dst[j] = v[u];
    }
  }
}

bool dtype_ok(int table_dtype) { return table_dtype == COATTN_F32 || table_dtype == COATTN_BF16; }

// 16-byte vectors of one table row, and the passes (workgroups) a row takes
long long row_vectors(long long N, long long d, int table_dtype) { return N * d / (table_dtype == COATTN_BF16 ? 8 : 4); }
long long row_passes(long long row16) { return (row16 + kThreads * kLoads - 1) / (kThreads * kLoads); }

bool shape_ok(long long S, long long B, int N, int d, int table_dtype) {
  if (!dtype_ok(table_dtype) || S < 1 || B < 1 || N < 1 || N > kMaxN || d < 1 || d > kMaxD) return false;
  if (((long long)N * d) % (table_dtype == COATTN_BF16 ? 8 : 4)) return false;
  if (B > kMaxGrid) return false;
  return B * row_passes(row_vectors(N, d, table_dtype)) <= kMaxGrid;
}

}  // namespace

extern "C" int coattn_features_gather_supported(long long S, long long B, int N, int d, int table_dtype, int flags) {
  return flags == 0 && shape_ok(S, B, N, d, table_dtype) ? 1 : 0;
}

extern "C" int coattn_features_gather(const void* table, int table_dtype, const void* idx, int idx_dtype, void* out,
                                      int32_t* bad_idx, long long S, long long B, int N, int d, int flags, void* stream) {
  const char* what = "features_gather";
  CA_CHECK_ARG(dtype_ok(table_dtype), "%s: unsupported table dtype %d (COATTN_F32 or COATTN_BF16)", what, table_dtype);
  CA_CHECK_ARG(idx_dtype == COATTN_IDS_I32 || idx_dtype == COATTN_IDS_I64, "%s: unsupported idx_dtype %d (COATTN_IDS_I32 or "
               "COATTN_IDS_I64)", what, idx_dtype);
  CA_CHECK_ARG(S > 0 && B > 0 && N > 0 && d > 0, "%s: non-positive size S=%lld B=%lld N=%d d=%d", what, S, B, N, d);
  CA_CHECK_ARG(flags == 0, "%s: flags %d not supported: the gather is an exact copy (no precision flag)", what, flags);
  CA_CHECK_ARG(shape_ok(S, B, N, d, table_dtype), "%s: shape S=%lld B=%lld N=%d d=%d not supported (N <= 4096, d <= 2048, N*d a "
               "multiple of %d for this table dtype, B * passes per row < 2^24: coattn_features_gather_supported)", what, S, B, N,
               d, table_dtype == COATTN_BF16 ? 8 : 4);
  CA_CHECK_ARG(table && idx && out, "%s: null table, idx or out", what);
  CA_CHECK_ARG(al16(table) && al16(out), "%s: table and out must be 16-byte aligned", what);
  CA_CHECK_ARG((((uintptr_t)idx) & (idx_dtype == COATTN_IDS_I64 ? 7 : 3)) == 0 && (((uintptr_t)bad_idx) & 3) == 0,
               "%s: idx must be aligned to its element size, bad_idx to 4 bytes", what);
  hipStream_t s = (hipStream_t)stream;
  const unsigned row16 = (unsigned)row_vectors(N, d, table_dtype);     // <= 2^21
  const unsigned passes = (unsigned)row_passes(row16);
  const dim3 grid((unsigned)(B * passes)), block(kThreads);
  const u32x4* t = (const u32x4*)table;
  u32x4* o = (u32x4*)out;
  const bool bf = table_dtype == COATTN_BF16;
  if (idx_dtype == COATTN_IDS_I64) {
    if (bf) hipLaunchKernelGGL((features_gather_kernel<long long, true>), grid, block, 0, s, t, (const long long*)idx, o,
                               (int*)bad_idx, S, row16, passes);
    else hipLaunchKernelGGL((features_gather_kernel<long long, false>), grid, block, 0, s, t, (const long long*)idx, o,
                            (int*)bad_idx, S, row16, passes);
  } else {
    if (bf) hipLaunchKernelGGL((features_gather_kernel<int, true>), grid, block, 0, s, t, (const int*)idx, o, (int*)bad_idx, S,
                               row16, passes);
    else hipLaunchKernelGGL((features_gather_kernel<int, false>), grid, block, 0, s, t, (const int*)idx, o, (int*)bad_idx, S,
                            row16, passes);
  }
  CA_CHECK_LAUNCH(what);
  prof_mark(s, what);
  return 0;
}
