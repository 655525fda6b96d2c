// Feature dropout on the six attended features between the co-attention and the answer head (Lu et al. 2016: dropout 0.5 on
// every q_l + v_l), include/coattn.h v0.19.0.
//
// A stateless counter RNG: element i belongs to Philox block j = i >> 2, word w = i & 3, and the block is a pure function of
// (j, step, seed).  Nothing is stored: the backward regenerates the mask of the forward from the same three numbers.  One
// thread draws one block and covers its four consecutive elements -- one 16-byte access per pointer when every pointer of the
// launch is 16-byte aligned, four 4-byte accesses otherwise; both forms use the same words for the same elements.
//
// `step` lives on the device (state word 2, 3) and is advanced by the launch that draws the new mask: every workgroup reads it
// before it takes a ticket from state word 4, and the workgroup that draws the last ticket -- after every other one has read
// the step -- stores step + 1 and leaves the ticket at 0 (the pattern of ce.hip's mean).  No launch in front, no host state:
// the call can be captured, and every replay draws a fresh mask.
#include "philox.h"   // the counter RNG and the mask's arithmetic: shared with fusion.hip

namespace {

constexpr int kThreads = 256;
constexpr long long kMaxN = 2147483644ll;                    // 2^31 - 4: element indices fit 32 bits with the block's last word

struct DropArgs {
  const float* x0; float* y0;
  const float* x1; float* y1;                                // NULL: one pair
  unsigned n, thr;
  float scale;
  unsigned* state;                                           // seed lo, hi, step lo, hi, ticket
  int advance;
};

// (no __restrict__: y may be x)
template <bool VEC>
__global__ __launch_bounds__(kThreads) void dropout_kernel(DropArgs a) {
  const unsigned long long j = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const Drop d = drop_load(a.state, a.thr, a.scale, a.advance);
  const unsigned i0 = (unsigned)(j << 2);                    // (j < 2^29 for every thread with an element)
  if (j < (((unsigned long long)a.n + 3) >> 2)) {
    const u32x4 r = drop_block(d, j);
    const float m0 = drop_word(d, r.x), m1 = drop_word(d, r.y), m2 = drop_word(d, r.z), m3 = drop_word(d, r.w);
    const unsigned left = a.n - i0;                          // >= 1
    if (VEC && left >= 4) {
      const f32x4 m = {m0, m1, m2, m3};
      const f32x4 v0 = *(const f32x4*)(a.x0 + i0);
      *(f32x4*)(a.y0 + i0) = v0 * m;
      if (a.x1) {
        const f32x4 v1 = *(const f32x4*)(a.x1 + i0);
        *(f32x4*)(a.y1 + i0) = v1 * m;
      }
    } else {
      const float m[4] = {m0, m1, m2, m3};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if ((unsigned)w < left) {
          a.y0[(size_t)i0 + w] = a.x0[(size_t)i0 + w] * m[w];
          if (a.x1) a.y1[(size_t)i0 + w] = a.x1[(size_t)i0 + w] * m[w];
        }
      }
    }
  }
  if (!a.advance) return;
  // every thread of this workgroup has read the step (the values above depend on it) before its ticket is taken
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned ticket = atomicAdd(a.state + 4, 1u);
    if (ticket == gridDim.x - 1) {                           // every other workgroup has read the step as well
      a.state[2] = d.s0;
      a.state[3] = d.s1;
      a.state[4] = 0u;
    }
  }
}

bool al(const void* p, unsigned mask) { return (((uintptr_t)p) & mask) == 0; }

int launch(const char* what, const void* x0, void* y0, const void* x1, void* y1, long long n, float p, void* state, int advance,
           void* stream) {
  CA_CHECK_ARG(p >= 0.0f && p < 1.0f, "%s: p = %g outside [0, 1) (NaN included)", what, (double)p);
  CA_CHECK_ARG(n >= 1 && n <= kMaxN, "%s: n = %lld not supported (1 <= n <= 2^31 - 4: coattn_dropout_supported)", what, n);
  CA_CHECK_ARG(x0 && y0 && state, "%s: null input, output or state", what);
  CA_CHECK_ARG((x1 == nullptr) == (y1 == nullptr), "%s: x1 and y1 go together (both, or both NULL)", what);
  CA_CHECK_ARG(al(x0, 3) && al(y0, 3) && al(x1, 3) && al(y1, 3) && al(state, 3), "%s: every pointer must be 4-byte aligned", what);
  DropArgs a = {};
  a.x0 = (const float*)x0; a.y0 = (float*)y0; a.x1 = (const float*)x1; a.y1 = (float*)y1;
  a.n = (unsigned)n;
  const DropHost dh = drop_host(p);
  a.thr = dh.thr;
  a.scale = dh.scale;
  a.state = (unsigned*)state;
  a.advance = advance ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks4 = (unsigned)((n + 3) >> 2);
  const dim3 grid((blocks4 + kThreads - 1) / kThreads);
  if (al(x0, 15) && al(y0, 15) && al(x1, 15) && al(y1, 15)) hipLaunchKernelGGL(dropout_kernel<true>, grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(dropout_kernel<false>, grid, dim3(kThreads), 0, s, a);
  CA_CHECK_LAUNCH(what);
  prof_mark(s, what);
  return 0;
}

}  // namespace

extern "C" int coattn_dropout_supported(long long n) { return n >= 1 && n <= kMaxN ? 1 : 0; }

extern "C" int coattn_dropout_forward(const void* x0, void* y0, const void* x1, void* y1, long long n, float p, void* state,
                                      int advance, void* stream) {
  return launch("dropout_forward", x0, y0, x1, y1, n, p, state, advance, stream);
}

extern "C" int coattn_dropout_backward(const void* g, void* dx, long long n, float p, void* state, void* stream) {
  return launch("dropout_backward", g, dx, nullptr, nullptr, n, p, state, 0, stream);
}
