// The word level of the question hierarchy (reference model.py: nn.Embedding in front of the phrase and sentence levels):
// the gather and its dense gradient, include/coattn.h v0.18.0.
//
// Forward: one launch, one 16-byte copy per thread; an id outside [0, V) selects a zero row and is counted.
// Backward: ONE launch, no sort, no fill, no float atomics, no workspace.  Workgroup (x, y) owns the kRows vocabulary rows
// from x * kRows and the LANES 16-byte columns from y * LANES of dW, and writes every element of them once:
//   1. each of its four waves counts, over its own contiguous quarter of the positions, the ids that fall on an owned row
//      (integer LDS atomics: the counts do not depend on their order);
//   2. a scan over (row, wave) turns the counts into cursors, and a second pass over the same quarters places the positions
//      (16-bit: n <= 65,536) into one LDS list grouped by row, ascending inside a row: a wave places the matches of a
//      64-position window row by row with a ballot, so the slot of a position is a function of the ids alone;
//   3. groups of LANES threads sum chunks of kChunk consecutive occurrences serially, chunk sums are combined left to
//      right (the order the header states).  A row of at most one chunk is done by one group; a hot row spreads its chunks
//      over all groups of the workgroup, and over the E / (4 LANES) workgroups that own its other columns.
#include "common.h"

namespace {

constexpr int kThreads = 256, kWaves = 4, kRows = 256, kBatch = 8, kChunk = COATTN_EMBEDDING_CHUNK;
constexpr long long kMaxN = 65536, kMaxV = 1ll << 24;
constexpr int kMaxE = 2048;
constexpr int kListMax = (int)kMaxN * 2;                     // bytes of the position list at n = kMaxN

template <typename IdT>
__global__ __launch_bounds__(kThreads) void embedding_fwd_kernel(const IdT* __restrict__ ids, const f32x4* __restrict__ W,
                                                                 f32x4* __restrict__ out, int* bad, unsigned total4,
                                                                 long long V, unsigned E4) {
  const unsigned idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total4) return;
  const unsigned i = idx / E4, c4 = idx - i * E4;
  const long long id = ids[i];
  const bool ok = (unsigned long long)id < (unsigned long long)V;     // (all 64 bits of an int64 id; a negative one is huge)
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (ok) v = W[(size_t)id * E4 + c4];
  else if (c4 == 0 && bad) atomicAdd(bad, 1);
  out[idx] = v;
}

// the owned row (0 .. v1 - v0 - 1) of position i, or -1: past the end, another workgroup's row, the padding id, outside the table
template <typename IdT>
__device__ __forceinline__ int owned_row(const IdT* __restrict__ ids, int i, int hi, long long v0, long long v1, long long pad) {
  if (i >= hi) return -1;
  const long long id = ids[i];
  return id >= v0 && id < v1 && id != pad ? (int)(id - v0) : -1;
}

// one chunk: ((g[p0] + g[p1]) + g[p2]) + ... over m >= 1 positions; eight loads in flight, the adds in order
__device__ __forceinline__ f32x4 chunk_sum(const f32x4* __restrict__ g4, const unsigned short* p, int m, unsigned E4, unsigned col4) {
  f32x4 s = g4[(size_t)p[0] * E4 + col4];
  for (int j = 1; j < m; j += 8) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (j + u < m) v[u] = g4[(size_t)p[j + u] * E4 + col4];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (j + u < m) s += v[u];
  }
  return s;
}

struct EmbBwd {
  const void* ids;
  const float* g;
  float* dW;
  int n, E, accumulate;
  long long V, pad;
};

template <typename IdT, int LANES>
__global__ __launch_bounds__(kThreads) void embedding_bwd_kernel(EmbBwd a) {
  constexpr int G = kThreads / LANES;
  extern __shared__ __align__(16) unsigned short list[];     // [n]: the positions on owned rows, by row, ascending
  __shared__ int cnt[kWaves][kRows];                         // counts per (wave, row), then the waves' write cursors
  __shared__ int rstart[kRows], rcount[kRows];
  __shared__ f32x4 csum[kThreads];                           // [G][LANES] chunk sums of a hot row
  __shared__ int wsum[kWaves], nhot;
  __shared__ unsigned short hot[kRows];                      // the owned rows of more than one chunk
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long v0 = (long long)blockIdx.x * kRows;
  const int R = a.V - v0 < kRows ? (int)(a.V - v0) : kRows;
  const long long v1 = v0 + R;
  const IdT* __restrict__ ids = (const IdT*)a.ids;
  const int n = a.n;

  for (int i = tid; i < kWaves * kRows; i += kThreads) (&cnt[0][0])[i] = 0;
  if (tid == 0) nhot = 0;
  __syncthreads();
  const int per = (n + kWaves * 64 - 1) / (kWaves * 64) * 64;
  const int lo = wave * per < n ? wave * per : n, hi = lo + per < n ? lo + per : n;
  // 1. counts (kBatch windows of 64 positions per round: their loads are in flight together)
  for (int base = lo; base < hi; base += 64 * kBatch) {
    int r[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) r[u] = owned_row<IdT>(ids, base + u * 64 + lane, hi, v0, v1, a.pad);
#pragma unroll
    for (int u = 0; u < kBatch; ++u)
      if (r[u] >= 0) atomicAdd(&cnt[wave][r[u]], 1);
  }
  __syncthreads();
  {
    // the rows' starts: an exclusive scan of the counts, one row per thread (in the wave by lane shifts, then over the waves);
    // rows of more than one chunk are noted for step 3 (in any order: a row's sum does not depend on when it is made)
    static_assert(kRows == kThreads, "one thread per owned row");
    int c = 0;
    for (int w = 0; w < kWaves; ++w) c += cnt[w][tid];
    rcount[tid] = c;
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    if (c > kChunk) hot[atomicAdd(&nhot, 1)] = (unsigned short)tid;
    __syncthreads();
    int run = incl - c;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    rstart[tid] = run;
    for (int w = 0; w < kWaves; ++w) {
      const int t = cnt[w][tid];
      cnt[w][tid] = run;
      run += t;
    }
  }
  __syncthreads();
  // 2. placement: window by window, row by row
  for (int base = lo; base < hi; base += 64 * kBatch) {
    int r[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) r[u] = owned_row<IdT>(ids, base + u * 64 + lane, hi, v0, v1, a.pad);
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const bool in = r[u] >= 0;
      unsigned long long todo = __ballot(in);
      while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int rr = __builtin_amdgcn_readlane(r[u], leader);
        const bool mine = r[u] == rr;                        // (rr >= 0: the leader is in)
        const unsigned long long m = __ballot(mine);
        const int cur = cnt[wave][rr];
        if (mine) list[cur + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)(base + u * 64 + lane);
        cnt[wave][rr] = cur + __popcll(m);                   // (every lane, the same value: read again by the next round)
        todo &= ~m;
      }
    }
  }
  __syncthreads();
  // 3. sums
  const int g = tid / LANES, l = tid % LANES;
  const unsigned E4 = a.E >> 2, col4 = blockIdx.y * LANES + l;
  const bool act = col4 < E4;
  const f32x4* __restrict__ g4 = (const f32x4*)a.g;
  f32x4* dW4 = (f32x4*)a.dW;
  const bool acc = a.accumulate & 1;
  if (act) {
    for (int r = g; r < R; r += G) {                         // rows of at most one chunk: one group each
      const int c = rcount[r];
      if (c > kChunk) continue;
      f32x4* dst = dW4 + (size_t)(v0 + r) * E4 + col4;
      if (c == 0) {
        if (!acc) *dst = f32x4{0.f, 0.f, 0.f, 0.f};
        continue;
      }
      const f32x4 s = chunk_sum(g4, list + rstart[r], c, E4, col4);
      *dst = acc ? *dst + s : s;
    }
  }
  const int hots = nhot;
  for (int h = 0; h < hots; ++h) {                           // hot rows: the whole workgroup, G chunks at a time
    const int r = hot[h], c = rcount[r];
    const int nch = (c + kChunk - 1) / kChunk;
    const unsigned short* p = list + rstart[r];
    f32x4 total = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < nch; k0 += G) {
      const int k = k0 + g;
      if (act && k < nch) csum[tid] = chunk_sum(g4, p + k * kChunk, c - k * kChunk < kChunk ? c - k * kChunk : kChunk, E4, col4);
      __syncthreads();
      if (act && g == 0) {
        const int m = nch - k0 < G ? nch - k0 : G;
        for (int j = 0; j < m; ++j) {
          const f32x4 s = csum[j * LANES + l];
          total = (k0 + j == 0) ? s : total + s;
        }
      }
      __syncthreads();
    }
    if (act && g == 0) {
      f32x4* dst = dW4 + (size_t)(v0 + r) * E4 + col4;
      *dst = acc ? *dst + total : total;
    }
  }
}

bool shape_ok(long long n, long long V, int E) {
  return n >= 1 && n <= kMaxN && V >= 1 && V <= kMaxV && E >= 4 && E <= kMaxE && E % 4 == 0;
}

int check_call(const char* what, long long n, long long V, int E, long long padding_idx, int dtype, int flags) {
  CA_CHECK_ARG(dtype == COATTN_F32, "%s: unsupported dtype %d (only COATTN_F32)", what, dtype);
  CA_CHECK_ARG(n > 0 && V > 0 && E > 0, "%s: non-positive size n=%lld V=%lld E=%d", what, n, V, E);
  CA_CHECK_ARG(flags == 0, "%s: flags %d not supported: the gather and its gradient are exact fp32 only (no precision flag)",
               what, flags);
  CA_CHECK_ARG(shape_ok(n, V, E), "%s: shape n=%lld V=%lld E=%d not supported (n <= 65536, V <= 2^24, E a multiple of 4 up to "
               "2048: coattn_embedding_supported)", what, n, V, E);
  CA_CHECK_ARG(padding_idx >= -1 && padding_idx < V, "%s: padding_idx %lld outside [-1, V = %lld)", what, padding_idx, V);
  return 0;
}

int check_ids(const char* what, const void* ids, int ids_dtype) {
  CA_CHECK_ARG(ids_dtype == COATTN_IDS_I32 || ids_dtype == COATTN_IDS_I64, "%s: unsupported ids_dtype %d (COATTN_IDS_I32 or "
               "COATTN_IDS_I64)", what, ids_dtype);
  CA_CHECK_ARG(ids, "%s: null ids", what);
  CA_CHECK_ARG((((uintptr_t)ids) & (ids_dtype == COATTN_IDS_I64 ? 7 : 3)) == 0, "%s: ids not aligned to their element size", what);
  return 0;
}

template <typename IdT, int LANES>
hipError_t allow_lds() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(embedding_bwd_kernel<IdT, LANES>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, kListMax);
}

DeviceOnce g_once;

}  // namespace

extern "C" int coattn_embedding_supported(long long n, long long V, int E, int dtype) {
  return dtype == COATTN_F32 && shape_ok(n, V, E) ? 1 : 0;
}

extern "C" int coattn_embedding_workspace_bytes(long long n, long long V, int E, int dtype, size_t* ws_bwd) {
  CA_TRY(check_call("embedding_workspace_bytes", n, V, E, -1, dtype, 0));
  if (ws_bwd) *ws_bwd = 0;                                   // the row owners index the ids in LDS: no pre-pass at these sizes
  return 0;
}

extern "C" int coattn_embedding_forward(const void* ids, int ids_dtype, const void* W, void* out, int32_t* bad_ids, long long n,
                                        long long V, int E, long long padding_idx, int dtype, int flags, void* stream) {
  CA_TRY(check_call("embedding_forward", n, V, E, padding_idx, dtype, flags));
  CA_TRY(check_ids("embedding_forward", ids, ids_dtype));
  CA_CHECK_ARG(W && out, "embedding_forward: null W or out");
  CA_CHECK_ARG(al16(W) && al16(out) && (((uintptr_t)bad_ids) & 3) == 0, "embedding_forward: W and out must be 16-byte aligned, "
               "bad_ids 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const unsigned E4 = (unsigned)E / 4, total4 = (unsigned)n * E4;      // <= 2^25
  const dim3 grid((total4 + kThreads - 1) / kThreads);
  if (ids_dtype == COATTN_IDS_I64)
    hipLaunchKernelGGL(embedding_fwd_kernel<long long>, grid, dim3(kThreads), 0, s, (const long long*)ids, (const f32x4*)W,
                       (f32x4*)out, (int*)bad_ids, total4, V, E4);
  else
    hipLaunchKernelGGL(embedding_fwd_kernel<int>, grid, dim3(kThreads), 0, s, (const int*)ids, (const f32x4*)W, (f32x4*)out,
                       (int*)bad_ids, total4, V, E4);
  CA_CHECK_LAUNCH("embedding_forward");
  prof_mark(s, "embedding_forward");
  return 0;
}

extern "C" int coattn_embedding_backward(const void* ids, int ids_dtype, const void* g_out, void* dW, void* ws, long long n,
                                         long long V, int E, long long padding_idx, int accumulate, int dtype, int flags,
                                         void* stream) {
  (void)ws;                                                  // reserved: coattn_embedding_workspace_bytes reports 0
  CA_TRY(check_call("embedding_backward", n, V, E, padding_idx, dtype, flags));
  CA_TRY(check_ids("embedding_backward", ids, ids_dtype));
  CA_CHECK_ARG(g_out && dW, "embedding_backward: null g_out or dW");
  CA_CHECK_ARG(al16(g_out) && al16(dW), "embedding_backward: g_out and dW must be 16-byte aligned");
  CA_TRY(g_once.run([] {
    hipError_t e = allow_lds<int, 8>();
    if (e == hipSuccess) e = allow_lds<int, 16>();
    if (e == hipSuccess) e = allow_lds<long long, 8>();
    if (e == hipSuccess) e = allow_lds<long long, 16>();
    return e;
  }, "embedding_backward"));
  hipStream_t s = (hipStream_t)stream;
  EmbBwd a = {};
  a.ids = ids; a.g = (const float*)g_out; a.dW = (float*)dW;
  a.n = (int)n; a.E = E; a.accumulate = accumulate; a.V = V; a.pad = padding_idx;
  const int E4 = E / 4, lanes = E > 512 ? 16 : 8;            // wide rows: 256-byte column slices, else 128-byte ones
  const dim3 grid((unsigned)((V + kRows - 1) / kRows), (unsigned)((E4 + lanes - 1) / lanes));
  const size_t lds = ((size_t)n * 2 + 15) & ~(size_t)15;
  const bool i64 = ids_dtype == COATTN_IDS_I64;
  if (lanes == 16) {
    if (i64) hipLaunchKernelGGL((embedding_bwd_kernel<long long, 16>), grid, dim3(kThreads), lds, s, a);
    else hipLaunchKernelGGL((embedding_bwd_kernel<int, 16>), grid, dim3(kThreads), lds, s, a);
  } else {
    if (i64) hipLaunchKernelGGL((embedding_bwd_kernel<long long, 8>), grid, dim3(kThreads), lds, s, a);
    else hipLaunchKernelGGL((embedding_bwd_kernel<int, 8>), grid, dim3(kThreads), lds, s, a);
  }
  CA_CHECK_LAUNCH("embedding_backward");
  prof_mark(s, "embedding_backward");
  return 0;
}
