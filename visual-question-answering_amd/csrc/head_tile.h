// What the two heads share (head.hip: MLPClassifier of the attention model; fusion.hip: the fusion head of the baseline model):
// the pieces of a 32 x 32 output tile whose contraction is split over the eight waves of a 512-thread workgroup -- raw buffer
// loads through descriptors, the staging of a [32 rows][KC] block that is contiguous along the contraction index into a
// per-wave LDS image, the MFMAs on a staged chunk -- and the loops around these pieces: the pipelined forward and dX tiles
// (next chunk's loads in flight behind this chunk's MFMAs) and the cross-wave sum in wave order.  What stays with the file
// that owns it: the operand forms (sums, concatenations, products, row scales) as policy objects of the loops, with their
// descriptors; every epilogue as a functor epi(m, n, sum); and the weight-gradient tiles whole -- their loads and products ARE
// their operand forms (three column modes and a deferred scale in head.hip, a row scale or a second factor in fusion.hip),
// and what the two have in common is an eight-line loop over M and the twelve-line store of dW and db: a template over both
// would be more text than it removes.  Everything sits in an anonymous namespace: each file that includes this header gets
// its own copies, as it would of its own helpers.
#pragma once
#include "common.h"
#include "fused.h"

namespace {

constexpr int kWaves = 8, kThreads = 64 * kWaves;
constexpr int KC = 32;            // contraction chunk per wave step: 16 MFMAs of 32x32x2
constexpr int LDR = KC + 4;       // padded LDS row (floats): 16-byte aligned, rows 4 banks apart

__device__ __forceinline__ f32x16 mfma2(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ constexpr int crow32(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

// ---- operands through buffer descriptors -------------------------------------------------------------------------------
// Every load is a raw buffer load: the descriptor covers [rows x ld] floats, so a row past the end is out of range and
// reads 0 (the hardware's range check includes the scalar offset: checked on gfx950), a column past the end gets the
// out-of-range vector offset kOut -- no per-lane condition ever guards a load (hipcc branches around a guarded load and
// waits for it alone: dozens of dependent round trips per chunk, 44 us per backward launch instead of 9), and no load
// needs a 64-bit address register: lane part in voffset, the wave-uniform row / chunk part in the scalar offset.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr int kOut = (int)0xC0000000u;      // beyond every descriptor; scalar offsets stay below 1 GB, so no wrap-around
__device__ __forceinline__ rsrc_t mk_rsrc(const void* p, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, p ? (unsigned)bytes : 0u, 0x00020000);
}
// (the scalar offsets are wave-uniform by construction; under SGPR pressure hipcc moves such arithmetic to the VALU and
//  then wraps every load in a waterfall loop -- the readfirstlane keeps the load a single instruction)
// AUX: the load's cache-policy bits.  kSC1 (gfx940+: bit 4) = coherent at agent scope -- what an atomic monotonic load at that
// scope compiles to: the one-launch forms read what ANOTHER workgroup of the same launch stored (with agent-scope stores)
// through it, past this XCD's L2.
constexpr int kSC1 = 16;
template <int AUX = 0>
__device__ __forceinline__ float bl1(rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, __builtin_amdgcn_readfirstlane(soff), AUX));
}
template <int AUX = 0>
__device__ __forceinline__ f32x4 bl4(rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, __builtin_amdgcn_readfirstlane(soff), AUX));
}

// ---- staging of a [32 rows][KC] block, contiguous along k, into the wave's LDS image ---------------------------------
// VEC: whole 128-byte lines, lane (r = lane >> 3, c = lane & 7) of instruction t fetches 16 bytes of row 8 t + r.
// Otherwise (any shape / alignment): two rows per instruction, a lane per k.
struct Stage {
  f32x4 v[4];                     // 16 floats per lane either way: 32 rows x KC / 64 lanes
};
// the lane's share of the block of a plain [rows x ld] matrix starting at (row0, k0); columns >= Klim read 0
template <bool VEC, int AUX = 0>
__device__ __forceinline__ void stage_lin(Stage& s, rsrc_t r, int ld, int Klim, int lane, int row0, int k0) {
  if constexpr (VEC) {
    const int rr = lane >> 3, kk = 4 * (lane & 7);
    const int voff = k0 + kk < Klim ? (rr * ld + kk) * 4 : kOut;
#pragma unroll
    for (int t = 0; t < 4; ++t) s.v[t] = bl4<AUX>(r, voff, ((row0 + 8 * t) * ld + k0) * 4);
  } else {
    const int kk = lane & 31, half = lane >> 5;
    const int voff = k0 + kk < Klim ? (half * ld + kk) * 4 : kOut;
#pragma unroll
    for (int t = 0; t < 16; ++t) s.v[t >> 2][t & 3] = bl1<AUX>(r, voff, ((row0 + 2 * t) * ld + k0) * 4);
  }
}
template <bool VEC>
__device__ __forceinline__ void stage_store(const Stage& s, float* img, int lane) {
  if constexpr (VEC) {
    const int r = lane >> 3, c = lane & 7;
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(img + (8 * t + r) * LDR + 4 * c) = s.v[t];
  } else {
    const int kk = lane & 31, half = lane >> 5;
#pragma unroll
    for (int t = 0; t < 16; ++t) img[(2 * t + half) * LDR + kk] = s.v[t >> 2][t & 3];
  }
}

// eight consecutive floats -> one bf16 MFMA operand (round to nearest even)
__device__ __forceinline__ bf16x8 pack8(const f32x4& a, const f32x4& b) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 v = {cvt_pk_bf16(a[0], a[1]), cvt_pk_bf16(a[2], a[3]), cvt_pk_bf16(b[0], b[1]), cvt_pk_bf16(b[2], b[3])};
  return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ bf16x8 pack8(const float* x) {
  return pack8(f32x4{x[0], x[1], x[2], x[3]}, f32x4{x[4], x[5], x[6], x[7]});
}
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
// the staged A fragment of 16-k step ks: lane (li, lh) takes k = 16 ks + 8 lh .. + 7 of its row
__device__ __forceinline__ bf16x8 frag16(const float* img, int li, int lh, int ks) {
  const float* p = img + li * LDR + 16 * ks + 8 * lh;
  return pack8(*reinterpret_cast<const f32x4*>(p), *reinterpret_cast<const f32x4*>(p + 4));
}

// the MFMAs on the staged chunk.  Exact: 16 of 32x32x2, lane (li, lh) of MFMA (u, e) takes k = 8 u + 4 lh + e of its row;
// BF: 2 of 32x32x16 on rounded operands
template <bool BF>
__device__ __forceinline__ void mfma_chunk(f32x16& acc, const float* imgA, const float* imgB, int li, int lh) {
  if constexpr (BF) {
#pragma unroll
    for (int ks = 0; ks < KC / 16; ++ks) acc = mfma16(frag16(imgA, li, lh, ks), frag16(imgB, li, lh, ks), acc);
  } else {
#pragma unroll
    for (int u = 0; u < KC / 8; ++u) {
      const f32x4 fa = *reinterpret_cast<const f32x4*>(imgA + li * LDR + 8 * u + 4 * lh);
      const f32x4 fb = *reinterpret_cast<const f32x4*>(imgB + li * LDR + 8 * u + 4 * lh);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = mfma2(fa[e], fb[e], acc);
    }
  }
}

// cross-wave sum of the eight partial 32 x 32 accumulators in wave order; epi(m, n, sum) for every element inside the matrix
template <class Epi>
__device__ __forceinline__ void reduce_epi(const f32x16& acc, float* red, int m0, int n0, int M, int N, int w, Epi epi) {
  const int lane = threadIdx.x & 63;
  __syncthreads();                                   // every wave is done with its staging images
#pragma unroll
  for (int g = 0; g < 16; ++g) red[(w * 16 + g) * 64 + lane] = acc[g];
  __syncthreads();
#pragma unroll
  for (int gg = 0; gg < 2; ++gg) {
    const int g = w + 8 * gg;
    float s = 0.f;
#pragma unroll
    for (int ww = 0; ww < kWaves; ++ww) s += red[(ww * 16 + g) * 64 + lane];
    const int m = m0 + crow32(g, lane >> 5), n = n0 + (lane & 31);
    if (m < M && n < N) epi(m, n, s);
  }
}

// ---- the tile loops ------------------------------------------------------------------------------------------------------
// The operand that is staged (A of the forward, dY of dX) is a policy object of the including file: load(lane, row0, k0) issues
// the loads of the block at (row0, k0) into registers the object keeps, store(img, lane) writes them -- combined, where the
// operand is a sum or a product: only then do the loads have to be back -- into the wave's LDS image.  The object owns its
// descriptors, as the caller owns W's: the extents differ between the two heads.  It is taken BY VALUE and built in the call
// (a prvalue: nothing is copied), and the epilogue functor holds a copy of its record: in this form every kernel of the two
// heads compiles to the register counts it had with loops of its own (profiles/head_tile_regs.txt), head.hip's per-element
// backward kernels included, which a first shared dX loop took from 148 to 116 VGPRs -- one of the two prefetch sets.

// forward tile: epi(m, n, sum_k A(m, k) W[n][k])
template <bool VEC, bool BF, class Op, class Epi>
__device__ __forceinline__ void fwd_tile(Op A, rsrc_t wr, int ldw, int M, int N, int K, int m0, int n0, float* smem, Epi epi) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, lh = lane >> 5;
  float* imgA = smem + w * (2 * 32 * LDR);
  float* imgB = imgA + 32 * LDR;
  f32x16 acc = {};
  const int nchunks = (K + KC - 1) / KC;
  Stage sb;
  int c = w;                                         // chunks interleaved over the waves: neighbouring lines together
  if (c < nchunks) {
    A.load(lane, m0, c * KC);
    stage_lin<VEC>(sb, wr, ldw, K, lane, n0, c * KC);
  }
  for (; c < nchunks; c += kWaves) {
    A.store(imgA, lane);
    stage_store<VEC>(sb, imgB, lane);
    if (c + kWaves < nchunks) {                      // next chunk's lines in flight behind this chunk's MFMAs
      A.load(lane, m0, (c + kWaves) * KC);
      stage_lin<VEC>(sb, wr, ldw, K, lane, n0, (c + kWaves) * KC);
    }
    __builtin_amdgcn_wave_barrier();
    mfma_chunk<BF>(acc, imgA, imgB, li, lh);
    __builtin_amdgcn_wave_barrier();
  }
  reduce_epi(acc, smem, m0, n0, M, N, w, epi);
}

// dX tile: epi(m, k', sum_n Y(m, n) W[n][k']), W [Nc][ldw] straight to registers
template <bool BF, class Op, class Epi>
__device__ __forceinline__ void dx_tile(Op Y, rsrc_t wr, int ldw, int M, int Nc /* contraction */, int Kout, int m0, int k0,
                                        float* smem, Epi epi) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, lh = lane >> 5;
  float* imgA = smem + w * (2 * 32 * LDR);
  f32x16 acc = {};
  const int nchunks = (Nc + KC - 1) / KC;
  // a lane per output column: 128-byte row segments of W; the lane half takes 4 (BF: 8) consecutive contraction rows
  const int bvoff = k0 + li < Kout ? ((BF ? 8 : 4) * lh * ldw + k0 + li) * 4 : kOut;
  float fb0[16], fb1[16];
  // contraction rows nc + 8 u + 4 lh + e (BF: nc + 16 ks + 8 lh + i); rows >= Nc read 0
  auto loadB = [&](float (&fb)[16], int nc) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = nc + (BF ? 16 * (j >> 3) + (j & 7) : 8 * (j >> 2) + (j & 3));
      fb[j] = bl1(wr, bvoff, row * ldw * 4);
    }
  };
  auto compute = [&](const float (&fb)[16]) {
    __builtin_amdgcn_wave_barrier();
    if constexpr (BF) {
#pragma unroll
      for (int ks = 0; ks < KC / 16; ++ks) acc = mfma16(frag16(imgA, li, lh, ks), pack8(&fb[8 * ks]), acc);
    } else {
#pragma unroll
      for (int u = 0; u < KC / 8; ++u) {
        const f32x4 fa = *reinterpret_cast<const f32x4*>(imgA + li * LDR + 8 * u + 4 * lh);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = mfma2(fa[e], fb[4 * u + e], acc);
      }
    }
    __builtin_amdgcn_wave_barrier();
  };
  int c = w;
  if (c < nchunks) {
    Y.load(lane, m0, c * KC);
    loadB(fb0, c * KC);
  }
  while (c < nchunks) {                                      // two chunks per trip: the register sets alternate
    Y.store(imgA, lane);
    int cn = c + kWaves;
    if (cn < nchunks) {
      Y.load(lane, m0, cn * KC);
      loadB(fb1, cn * KC);
    }
    compute(fb0);
    c = cn;
    if (c >= nchunks) break;
    Y.store(imgA, lane);
    cn = c + kWaves;
    if (cn < nchunks) {
      Y.load(lane, m0, cn * KC);
      loadB(fb0, cn * KC);
    }
    compute(fb1);
    c = cn;
  }
  reduce_epi(acc, smem, m0, k0, M, Kout, w, epi);
}

}  // namespace
