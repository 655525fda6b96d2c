// The optimiser step of the train loop on gfx950 (reference main.py:180 / :222: torch.optim.Adam(model.parameters(), lr) and
// optimizer.step()), fp32: ONE launch updates a whole list of tensors, and -- what the reference lacks -- decoupled weight
// decay (AdamW) and gradient clipping by global norm (torch.nn.utils.clip_grad_norm_) ride along.
//
// Mapping.  A workgroup of 256 threads owns one chunk of kChunk = 4096 elements of one tensor.  The launch carries a block of
// up to kBlockTensors {p, g, m, v, n} entries and the prefix sums of their chunk counts as kernel arguments; a workgroup finds
// its (tensor, chunk) by a binary search over the prefix sums (uniform: scalar loads from the argument segment).  A longer
// list goes out as further launches of the same call.
//
// Traffic.  The update reads p, g, m, v and writes p, m, v: 28 B per element, in 16-byte accesses where the four pointers
// of the chunk are 16-byte aligned (every chunk of a tensor starts kChunk elements = 16 KB behind its base, so the base
// decides), dword accesses otherwise and on the last < 4 elements.  All of a thread's loads are issued before the first use.
// The norm pass reads g once more: 4 B per element.
//
// Arithmetic: torch.optim.Adam's single-tensor form (torch/optim/adam.py), one rounding each where it has one:
//     g' = g * clip                                   (clipped calls only; clip from the workspace, written by grad_norm_kernel)
//     p  = p * (1 - lr wd)                            (wd != 0 only)
//     m  = beta1 m + (1 - beta1) g'      v = beta2 v + (1 - beta2) g' g'
//     p  = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
// IEEE division and square root (hipcc's default for HIP: correctly rounded), fma for the two moment updates and the last line.
// The scalars (1 - beta, lr / bc1, sqrt(bc2), 1 - lr wd) are formed on the host in double and rounded once.
#include <math.h>

#include "common.h"

namespace {

constexpr int kChunk = 4096;            // elements per workgroup: 16 per thread, four 16-byte accesses per array
constexpr int kThreads = 256;
constexpr int kBlockTensors = 64;       // entries per launch (the attention model has 29 trainable tensors)
constexpr int64_t kMaxElems = (int64_t)1 << 40;

// workspace: a 64-byte header, then room for one double per chunk of the whole call (grad_norm_kernel's partials)
struct Header {
  unsigned ticket;                      // workgroups of grad_norm_kernel that have stored their partial (0 between calls)
  unsigned pad;
  float norm;                           // sqrt(sum of g^2) over every tensor of the call
  float clip;                           // min(1, max_norm / (norm + 1e-6))
};
constexpr size_t kHeaderBytes = 64;

struct TensorBlock {
  float* p[kBlockTensors];
  const float* g[kBlockTensors];
  float* m[kBlockTensors];
  float* v[kBlockTensors];
  long long n[kBlockTensors];
  int first[kBlockTensors + 1];         // first[t] = chunks of the entries before t; first[count] = workgroups of the launch
  int count;
};

struct Hyper {
  float beta1, omb1, beta2, omb2;       // omb = 1 - beta
  float step;                           // lr / bc1
  float bc2_sqrt;
  float eps;
  float decay;                          // 1 - lr wd
  int decoupled;                        // wd != 0
};

// the entry t with first[t] <= b < first[t + 1]  (entries of zero chunks never match: the call drops them before)
__device__ __forceinline__ int find_tensor(const TensorBlock& tb, int b) {
  int lo = 0, hi = tb.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tb.first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const Hyper& h, float clip, bool clipped) {
  if (clipped) g *= clip;
  if (h.decoupled) p *= h.decay;
  m = fmaf(h.beta1, m, h.omb1 * g);
  v = fmaf(h.beta2, v, h.omb2 * (g * g));
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p = fmaf(-h.step, m / denom, p);
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

__global__ __launch_bounds__(kThreads) void adam_step_kernel(const TensorBlock tb, const Hyper h, const float* __restrict__ clip_ptr) {
  const int b = blockIdx.x;
  const int t = find_tensor(tb, b);
  const long long off = (long long)(b - tb.first[t]) * kChunk;
  const long long left = tb.n[t] - off;
  const int cnt = left < kChunk ? (int)left : kChunk;
  float* p = tb.p[t] + off;
  const float* g = tb.g[t] + off;
  float* m = tb.m[t] + off;
  float* v = tb.v[t] + off;
  const bool clipped = clip_ptr != nullptr;
  const float clip = clipped ? clip_ptr[0] : 1.f;
  const int tid = threadIdx.x;
  if (aligned16(p, g, m, v)) {
    const int quads = cnt >> 2;
    f32x4 P[4], G[4], M[4], V[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = u * kThreads + tid;
      if (q < quads) {
        P[u] = reinterpret_cast<const f32x4*>(p)[q];
        G[u] = reinterpret_cast<const f32x4*>(g)[q];
        M[u] = reinterpret_cast<const f32x4*>(m)[q];
        V[u] = reinterpret_cast<const f32x4*>(v)[q];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = u * kThreads + tid;
      if (q < quads) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pp = P[u][e], mm = M[u][e], vv = V[u][e];
          adam_one(pp, G[u][e], mm, vv, h, clip, clipped);
          P[u][e] = pp; M[u][e] = mm; V[u][e] = vv;
        }
        reinterpret_cast<f32x4*>(p)[q] = P[u];
        reinterpret_cast<f32x4*>(m)[q] = M[u];
        reinterpret_cast<f32x4*>(v)[q] = V[u];
      }
    }
    const int i = (quads << 2) + tid;                   // the last cnt % 4 elements
    if (tid < 3 && i < cnt) {
      float pp = p[i], mm = m[i], vv = v[i];
      adam_one(pp, g[i], mm, vv, h, clip, clipped);
      p[i] = pp; m[i] = mm; v[i] = vv;
    }
    return;
  }
  for (int base = 0; base < cnt; base += 4 * kThreads) {
    float P[4], G[4], M[4], V[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = base + u * kThreads + tid;
      if (i < cnt) { P[u] = p[i]; G[u] = g[i]; M[u] = m[i]; V[u] = v[i]; }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = base + u * kThreads + tid;
      if (i < cnt) {
        adam_one(P[u], G[u], M[u], V[u], h, clip, clipped);
        p[i] = P[u]; m[i] = M[u]; v[i] = V[u];
      }
    }
  }
}

__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
  return x;
}
// every thread's value summed in one fixed order: the wave butterflies, then (0 + 1) + (2 + 3); valid in thread 0
__device__ __forceinline__ double block_sum_f64(double x, double* sh) {
  x = wave_sum_f64(x);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// partial[block_base + b] = sum of g^2 over kNormChunks consecutive chunks of the launch, accumulated in double (the pass reads
// 4 B per element: the conversions and double fmas hide behind the loads, and the norm then carries ONE fp32 rounding whatever
// the list's size).  A norm workgroup takes several chunks because each workgroup ends in a device-scope ticket on one word,
// and one word serves ~90 tickets per microsecond: one per chunk would cost more than reading the gradients does.
// The workgroup that draws the call's last ticket (total - 1, counted over every launch of the call: the launches run in stream
// order, so it sits in the last one) adds all partials -- strided over its threads, then block_sum_f64's order: the same bits
// whichever workgroup it is --, stores norm and clip and leaves the ticket at 0.  Partials go out and come back as agent-scope
// atomic accesses around the integer ticket, as ce.hip's row losses do.  No float atomics.
constexpr int kNormChunks = 4;

__global__ __launch_bounds__(kThreads) void grad_norm_kernel(const TensorBlock tb, double* partial, int block_base, int total,
                                                             Header* hdr, float max_norm, float* __restrict__ norm_out) {
  __shared__ double sh[4];
  __shared__ unsigned ticket;
  const int tid = threadIdx.x;
  const int nchunks = tb.first[tb.count];
  const int c0 = blockIdx.x * kNormChunks, c1 = c0 + kNormChunks < nchunks ? c0 + kNormChunks : nchunks;
  double acc = 0.0;
  for (int c = c0; c < c1; ++c) {
    const int t = find_tensor(tb, c);
    const long long off = (long long)(c - tb.first[t]) * kChunk;
    const long long left = tb.n[t] - off;
    const int cnt = left < kChunk ? (int)left : kChunk;
    const float* g = tb.g[t] + off;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
      const int quads = cnt >> 2;
      f32x4 G[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = u * kThreads + tid;
        G[u] = q < quads ? reinterpret_cast<const f32x4*>(g)[q] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fma((double)G[u][e], (double)G[u][e], acc);
      const int i = (quads << 2) + tid;
      if (tid < 3 && i < cnt) acc = fma((double)g[i], (double)g[i], acc);
    } else {
      for (int base = 0; base < cnt; base += 4 * kThreads) {
        float G[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = base + u * kThreads + tid;
          G[u] = i < cnt ? g[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fma((double)G[u], (double)G[u], acc);
      }
    }
  }
  acc = block_sum_f64(acc, sh);
  if (tid == 0) {
    __hip_atomic_store(&partial[block_base + blockIdx.x], acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();                                  // the partial is visible device-wide before the ticket is taken
    ticket = atomicAdd(&hdr->ticket, 1u);
  }
  __syncthreads();
  if (ticket != (unsigned)(total - 1)) return;
  __threadfence();
  double sum = 0.0;
  for (int r = tid; r < total; r += kThreads) sum += __hip_atomic_load(&partial[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();                                    // (sh is still being read by thread 0's first block_sum_f64)
  sum = block_sum_f64(sum, sh);
  if (tid == 0) {
    const float norm = (float)sqrt(sum);
    const float c = max_norm / (norm + 1e-6f);        // clip_grad_norm_'s coefficient; a NaN norm stays NaN, as its clamp leaves it
    hdr->norm = norm;
    hdr->clip = c > 1.f ? 1.f : c;
    if (norm_out) norm_out[0] = norm;
    hdr->ticket = 0u;
  }
}

inline int chunks_of(int64_t n) { return (int)((n + kChunk - 1) / kChunk); }

int check_list(const char* what, const coattn_adam_tensor* t, int n_tensors, int64_t* total_chunks) {
  CA_CHECK_ARG(t && n_tensors > 0, "%s: n_tensors=%d (a list of at least one tensor is needed)", what, n_tensors);
  int64_t total = 0;
  for (int i = 0; i < n_tensors; ++i) {
    CA_CHECK_ARG(t[i].n >= 0, "%s: tensor %d has n=%lld < 0", what, i, (long long)t[i].n);
    CA_CHECK_ARG(t[i].n <= kMaxElems, "%s: tensor %d has n=%lld elements (at most 2^40)", what, i, (long long)t[i].n);
    CA_CHECK_ARG(t[i].p && t[i].g && t[i].m && t[i].v, "%s: tensor %d has a null p / g / m / v", what, i);
    total += chunks_of(t[i].n);
  }
  CA_CHECK_ARG(total <= (int64_t)1 << 30, "%s: %lld chunks of %d elements in one call (at most 2^30)", what, (long long)total,
               kChunk);
  *total_chunks = total;
  return 0;
}

// Walks the list in launches of at most kBlockTensors non-empty entries; f(block, chunk_base) launches one.
template <typename F>
int for_each_block(const coattn_adam_tensor* t, int n_tensors, F f) {
  TensorBlock tb;
  tb.count = 0;
  tb.first[0] = 0;
  int chunk_base = 0;
  for (int i = 0; i <= n_tensors; ++i) {
    if (i < n_tensors && t[i].n > 0) {
      const int k = tb.count++;
      tb.p[k] = (float*)t[i].p;
      tb.g[k] = (const float*)t[i].g;
      tb.m[k] = (float*)t[i].m;
      tb.v[k] = (float*)t[i].v;
      tb.n[k] = t[i].n;
      tb.first[k + 1] = tb.first[k] + chunks_of(t[i].n);
    }
    if (tb.count == kBlockTensors || (i == n_tensors && tb.count > 0)) {
      CA_TRY(f(tb, chunk_base));
      chunk_base += tb.first[tb.count];
      tb.count = 0;
    }
  }
  return 0;
}

}  // namespace

extern "C" size_t coattn_adam_workspace_bytes(const coattn_adam_tensor* t, int n_tensors) {
  int64_t total = 0;
  if (check_list("adam_workspace_bytes", t, n_tensors, &total) != 0) return 0;
  return kHeaderBytes + (size_t)total * sizeof(double);
}

extern "C" int coattn_adam_step(const coattn_adam_tensor* t, int n_tensors, int step, double lr, double beta1, double beta2,
                                double eps, double weight_decay, double max_grad_norm, void* norm_out, void* ws,
                                size_t ws_bytes, void* stream) {
  int64_t total = 0;
  CA_TRY(check_list("adam_step", t, n_tensors, &total));
  CA_CHECK_ARG(step >= 1, "adam_step: step=%d (the first step is 1)", step);
  CA_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_step: betas (%g, %g) outside [0, 1)", beta1,
               beta2);
  const bool clip = max_grad_norm > 0.0;
  if (clip) {
    const size_t need = kHeaderBytes + (size_t)total * sizeof(double);
    CA_CHECK_ARG(ws && ws_bytes >= need, "adam_step: workspace of %zu bytes, %zu needed (coattn_adam_workspace_bytes)",
                 ws ? ws_bytes : (size_t)0, need);
    CA_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "adam_step: the workspace must be 8-byte aligned");
  }
  hipStream_t s = (hipStream_t)stream;
  Header* hdr = (Header*)ws;
  if (clip) {
    // the ticket starts at 0 whatever the workspace held
    if (hipMemsetAsync(hdr, 0, 16, s) != hipSuccess) {
      coattn_set_error("adam_step: clearing the workspace header failed");
      return -3;
    }
    if (total == 0) {
      if (norm_out && hipMemsetAsync(norm_out, 0, sizeof(float), s) != hipSuccess) {
        coattn_set_error("adam_step: clearing norm_out failed");
        return -3;
      }
      return 0;
    }
    double* partial = (double*)((char*)ws + kHeaderBytes);     // one per norm workgroup (the workspace has one per chunk: enough)
    const auto norm_blocks = [](const TensorBlock& tb) { return (tb.first[tb.count] + kNormChunks - 1) / kNormChunks; };
    int blocks = 0, block_base = 0;
    CA_TRY(for_each_block(t, n_tensors, [&](const TensorBlock& tb, int) { blocks += norm_blocks(tb); return 0; }));
    CA_TRY(for_each_block(t, n_tensors, [&](const TensorBlock& tb, int) {
      hipLaunchKernelGGL(grad_norm_kernel, dim3(norm_blocks(tb)), dim3(kThreads), 0, s, tb, partial, block_base, blocks, hdr,
                         (float)max_grad_norm, (float*)norm_out);
      CA_CHECK_LAUNCH("grad_norm");
      block_base += norm_blocks(tb);
      return 0;
    }));
    prof_mark(s, "grad_norm");
  }
  if (total == 0) return 0;
  Hyper h;
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  h.beta1 = (float)beta1;
  h.omb1 = (float)(1.0 - beta1);
  h.beta2 = (float)beta2;
  h.omb2 = (float)(1.0 - beta2);
  h.step = (float)(lr / bc1);
  h.bc2_sqrt = (float)sqrt(bc2);
  h.eps = (float)eps;
  h.decay = (float)(1.0 - lr * weight_decay);
  h.decoupled = weight_decay != 0.0;
  const float* clip_ptr = clip ? &hdr->clip : nullptr;
  CA_TRY(for_each_block(t, n_tensors, [&](const TensorBlock& tb, int) {
    hipLaunchKernelGGL(adam_step_kernel, dim3(tb.first[tb.count]), dim3(kThreads), 0, s, tb, h, clip_ptr);
    CA_CHECK_LAUNCH("adam_step");
    return 0;
  }));
  prof_mark(s, "adam_step");
  return 0;
}
