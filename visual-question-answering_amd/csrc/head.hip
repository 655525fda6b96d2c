// Answer head of the attention model on gfx950: MLPClassifier (reference model.py:400-434) + nn.CrossEntropyLoss
// (main.py:94, :214) + their backward, behind the C-ABI coattn_head_forward / coattn_head_backward.
//
//   h_w = tanh(W_w (q_w + v_w) + b_w)                        [B, d]         model.py:428
//   h_p = tanh(W_p [q_p + v_p | h_w] + b_p)                  [B, d]         model.py:429
//   h_s = tanh(W_s [q_s + v_s | h_p] + b_s)                  [B, mlp]       model.py:430
//   logits = W_h h_s + b_h                                   [B, K]         model.py:433
//   loss = mean_i (logsumexp(logits_i) - logits_i[label_i])                main.py:214
//
// The batch is ONE short M dimension (B = 160 rows), so every product is a small GEMM that a single 128 x 128-tile
// launch cannot spread over the chip (round 1's composition of the general GEMM: thirty launches, 0.53 ms).  Here a
// product is cut into 32 x 32 output tiles, one 512-thread workgroup each, with the CONTRACTION split over the eight
// waves (cross-wave sum in a fixed order through LDS): 80-160 tiles per layer.  The q_l + v_l adds and the concatenations
// are folded into the A-operand addressing, bias + tanh into the epilogue, tanh' of the backward into the epilogue of the
// product that yields d h; every backward launch carries the dX tiles of a layer (the dependent chain) AND the tiles of
// that layer's weight gradient dW = dY^T X (+ the bias gradient), which depend on nothing the launch itself produces and
// fill the CUs the chain leaves idle.  Forward: 4 launches + cross entropy (1: ce.hip); backward: 4 launches.
//
// Arithmetic: exact fp32 on v_mfma_f32_32x32x2_f32 (one rounding per product, as an fmaf chain).  The products are too
// small for the bf16 3-way split of the big GEMMs to pay: every operand element is used by one 32 x 32 tile only, so the
// 11 VALU operations per split pair would cost more than the 64-cycle f32 MFMAs they replace.
// Reduced-precision mode (flags bit 2, COATTN_FLAG_BF16_PROJ -- the apex-O1 analogue, BASELINE config 4: d = 2048, K = 3000,
// where the exact head is bound by the f32 matrix pipe: 25 GFLOP forward + backward at 76 TFLOP/s): the same tiles, loads
// and staging, with eight operand values per lane rounded to bf16 (v_cvt_pk_bf16_f32) in front of ONE
// v_mfma_f32_32x32x16_bf16 where the exact path issues eight v_mfma_f32_32x32x2_f32; fp32 accumulation, bias, tanh,
// cross entropy and bias gradients as before.
// Operands that are contiguous along the contraction index (activations and nn.Linear weights in the forward, dY in dX)
// are fetched as whole 128-byte lines (8 rows per wave instruction), staged in a per-wave LDS image with padded rows and
// read back as fragments (ds_read_b128, conflict-free); operands contiguous along the tile index (the weight in dX, both
// operands of dW) go straight to registers (a lane per column: 128-byte row segments).  Deterministic: no atomics.
#include "head_tile.h"   // the buffer loads, the staging, the MFMAs on a block, the forward / dX tile loops: with fusion.hip
#include <type_traits>

namespace {

// activation operand with the reference's adds and concatenation folded in (model.py:428-430):
//   X(m, k) = k < ksplit ? x0[m][k] + x1[m][k] : h[m][k - ksplit]            (x1 may be NULL; rows ld0 / ldh apart)
struct Comp {
  const float* x0; const float* x1; const float* h;
  int ksplit, ld0, ldh;
};
// upstream gradient operand: dY(m, n) = p[m][n] * (scale ? scale[0] : 1) + (add ? add[m][n] : 0)
struct DY {
  const float* p; const float* scale; const float* add; int ld, ld_add;    // rows of p / of add this many floats apart
};
struct CompR {                    // Comp with descriptors over M rows, K columns in all
  rsrc_t x0, x1, h; int ksplit, ld0, ldh, K; bool two;
};
__device__ __forceinline__ CompR comp_rsrc(const Comp& c, int M, int K) {
  CompR r;
  r.x0 = mk_rsrc(c.x0, (long)M * c.ld0 * 4); r.x1 = mk_rsrc(c.x1, (long)M * c.ld0 * 4); r.h = mk_rsrc(c.h, (long)M * c.ldh * 4);
  r.ksplit = c.ksplit; r.ld0 = c.ld0; r.ldh = c.ldh; r.K = K; r.two = c.x1 != nullptr;
  return r;
}
struct DYR { rsrc_t p, add; int ld, ld_add, N; bool has_add; float sc; };
__device__ __forceinline__ DYR dy_rsrc(const DY& d, int M, int N) {
  DYR r;
  r.p = mk_rsrc(d.p, (long)M * d.ld * 4); r.add = mk_rsrc(d.add, (long)M * d.ld_add * 4);
  r.ld = d.ld; r.ld_add = d.ld_add; r.N = N; r.has_add = d.add != nullptr; r.sc = d.scale ? d.scale[0] : 1.f;
  return r;
}

// an operand that is the sum of two arrays keeps both register sets until the block is written to LDS: the addition
// would otherwise wait for both loads right where they are issued, in front of the other operand's loads
struct Stage2 {
  Stage a, b; bool two; float sc;   // value = a * sc + (two ? b : 0)
};
// COH (the one-launch forms): the hidden part `h` was stored by another workgroup of this launch -- agent-coherent loads
template <bool VEC, bool COH>
__device__ __forceinline__ void stage2(Stage2& s, const CompR& c, int lane, int m0, int k0) {
  constexpr int HA = COH ? kSC1 : 0;
  s.sc = 1.f;
  s.two = false;
  if (k0 + KC <= c.ksplit) {                                 // (wave-uniform branches: scalar control flow)
    stage_lin<VEC>(s.a, c.x0, c.ld0, c.K, lane, m0, k0);
    s.two = c.two;
    if (c.two) stage_lin<VEC>(s.b, c.x1, c.ld0, c.K, lane, m0, k0);
  } else if (k0 >= c.ksplit) {
    stage_lin<VEC, HA>(s.a, c.h, c.ldh, c.K - c.ksplit, lane, m0, k0 - c.ksplit);
  } else {                                                   // the chunk straddles the concatenation (d % 32 != 0): never VEC
    const int kk = lane & 31, half = lane >> 5, k = k0 + kk;
    const int v0 = k < c.ksplit ? (half * c.ld0 + kk) * 4 : kOut;
    const int vh = (k >= c.ksplit && k < c.K) ? (half * c.ldh + k - c.ksplit) * 4 : kOut;   // (scalar offsets stay >= 0)
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int s0 = ((m0 + 2 * t) * c.ld0 + k0) * 4, sh = (m0 + 2 * t) * c.ldh * 4;
      s.a.v[t >> 2][t & 3] = bl1(c.x0, v0, s0) + bl1(c.x1, v0, s0) + bl1<HA>(c.h, vh, sh);
    }
  }
}
template <bool VEC, bool COH>
__device__ __forceinline__ void stage2(Stage2& s, const DYR& y, int lane, int m0, int n0) {
  s.sc = y.sc;
  s.two = y.has_add;
  stage_lin<VEC, COH ? kSC1 : 0>(s.a, y.p, y.ld, y.N, lane, m0, n0);
  if (y.has_add) stage_lin<VEC>(s.b, y.add, y.ld_add, y.N, lane, m0, n0);
}
// either of the two (R: CompR, DYR) as the staged operand of head_tile.h's loops
template <bool VEC, bool COH, class R>
struct Op2 {
  R r; Stage2 s;
  __device__ __forceinline__ explicit Op2(const R& r_) : r(r_) {}
  __device__ __forceinline__ void load(int lane, int m0, int k0) { stage2<VEC, COH>(s, r, lane, m0, k0); }
  __device__ __forceinline__ void store(float* img, int lane) const {
    Stage t;
#pragma unroll
    for (int i = 0; i < 4; ++i) t.v[i] = s.two ? s.a.v[i] * s.sc + s.b.v[i] : s.a.v[i] * s.sc;
    stage_store<VEC>(t, img, lane);
  }
};
struct TileOut {
  float* C; int ldc;              // plain output rows
  const float* bias;              // [n] or NULL
  int act;                        // 1: tanh
  // dX epilogue: columns >= hsplit are gradients of a hidden activation: multiplied by 1 - hid^2 and stored to Ch
  int hsplit; const float* hid; int ldhid; float* Ch; int ldch;
  float* C2;                      // second copy of the plain columns (dq beside dv), may be NULL
};
// the epilogue of a forward or dX tile, on the cross-wave sum of element (m, n)
// COH (the one-launch forms): the outputs another workgroup of the launch reads next go out as agent-scope stores
template <bool COH>
struct TileEpi {
  const TileOut o;                // (a copy, as the operand objects are: head_tile.h says why)
  __device__ __forceinline__ void operator()(int m, int n, float s) const {
    if (o.bias) s += o.bias[n];
    if (o.act) s = tanhf(s);
    auto put = [](float* p, float v) {
      if constexpr (COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else *p = v;
    };
    if (n >= o.hsplit) {
      const float hv = o.hid[(long)m * o.ldhid + (n - o.hsplit)];
      put(&o.Ch[(long)m * o.ldch + (n - o.hsplit)], s * (1.f - hv * hv));
    } else {
      if (o.C) put(&o.C[(long)m * o.ldc + n], s);
      if (o.C2) o.C2[(long)m * o.ldc + n] = s;
    }
  }
};

// ---- forward tile: C[m][n] = act(sum_k X(m, k) W[n][k] + bias[n]);  dX tile: dX[m][k'] = sum_n dY(m, n) W[n][k'] ----
// (the loops: head_tile.h; every descriptor covers rows x ld floats)
template <bool VEC, bool BF, bool COH = false>
__device__ __forceinline__ void head_fwd_tile(const Comp& A, const float* __restrict__ W, int ldw, const TileOut& o, int M, int N,
                                              int K, int m0, int n0, float* smem) {
  fwd_tile<VEC, BF>(Op2<VEC, COH, CompR>(comp_rsrc(A, M, K)), mk_rsrc(W, (long)N * ldw * 4), ldw, M, N, K, m0, n0, smem,
                    TileEpi<COH>{o});
}
template <bool VEC, bool BF, bool COH = false>
__device__ __forceinline__ void head_dx_tile(const DY& Y, const float* __restrict__ W, int ldw, const TileOut& o, int M,
                                             int Nc /* contraction */, int Kout, int m0, int k0, float* smem) {
  dx_tile<BF>(Op2<VEC, COH, DYR>(dy_rsrc(Y, M, Nc)), mk_rsrc(W, (long)Nc * ldw * 4), ldw, M, Nc, Kout, m0, k0, smem,
              TileEpi<COH>{o});
}

// ---- dW tile (one WAVE): dW[n][k'] (+)= sum_m dY(m, n) X(m, k');  db[n] (+)= sum_m dY(m, n) for the tiles with k0 = 0 ----
template <bool BF, bool COH = false>
__device__ __forceinline__ void dw_tile(const DY& Y, const Comp& X, float* __restrict__ dW, int ldw, float* __restrict__ db, int M, int N, int Kin,
                                        int n0, int k0, int accumulate) {
  const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const DYR yr = dy_rsrc(Y, M, N);
  const CompR xr = comp_rsrc(X, M, Kin);
  const bool a_ok = n0 + li < N;
  // a lane per tile column, two batch rows per instruction (the lane halves: rows m + lh; BF: rows m + 8 lh, eight
  // consecutive rows per lane and MFMA); rows >= M are out of range and read 0
  constexpr int HR = BF ? 8 : 1;
  const int avoff = a_ok ? (HR * lh * yr.ld + n0 + li) * 4 : kOut, avoff_add = a_ok ? (HR * lh * yr.ld_add + n0 + li) * 4 : kOut;
  const int k = k0 + li;
  const int v0 = k < xr.ksplit ? (HR * lh * xr.ld0 + k) * 4 : kOut;
  const int vh = (k >= xr.ksplit && k < Kin) ? (HR * lh * xr.ldh + k - xr.ksplit) * 4 : kOut;
  f32x16 acc = {};
  float colsum = 0.f;
  // the loop is specialised ONCE per tile on the arrays its columns touch (a branch per load, even a wave-uniform one,
  // ends the basic block and hipcc waits for every load where it stands): 0 = q_l + v_l part, 1 = hidden part,
  // 2 = everything (a tile across the concatenation, or an added upstream gradient)
  auto run = [&](auto mode) {
    constexpr int MODE = decltype(mode)::value;
    float a0[16], b0[16], a1[16], b1[16];
    auto load = [&](float (&fa)[16], float (&fb)[16], int mc) {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int m = mc + (BF ? 16 * (s >> 3) + (s & 7) : 2 * s);
        fa[s] = bl1<COH ? kSC1 : 0>(yr.p, avoff, m * yr.ld * 4);
        if constexpr (MODE == 2) fa[s] = fa[s] * yr.sc + bl1(yr.add, avoff_add, m * yr.ld_add * 4);
        if constexpr (MODE == 0) fb[s] = bl1(xr.x0, v0, m * xr.ld0 * 4) + bl1(xr.x1, v0, m * xr.ld0 * 4);
        if constexpr (MODE == 1) fb[s] = bl1(xr.h, vh, m * xr.ldh * 4);
        if constexpr (MODE == 2) fb[s] = bl1(xr.x0, v0, m * xr.ld0 * 4) + bl1(xr.x1, v0, m * xr.ld0 * 4) + bl1(xr.h, vh, m * xr.ldh * 4);
      }
    };
    auto compute = [&](const float (&fa)[16], const float (&fb)[16]) {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        if constexpr (!BF) acc = mfma2(fa[s], fb[s], acc);
        colsum += fa[s];
      }
      if constexpr (BF) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) acc = mfma16(pack8(&fa[8 * ks]), pack8(&fb[8 * ks]), acc);
      }
    };
    load(a0, b0, 0);
    for (int mc = 0; mc < M; mc += 64) {                      // two chunks per trip: the register sets alternate
      if (mc + 32 < M) load(a1, b1, mc + 32);
      compute(a0, b0);
      if (mc + 32 >= M) break;
      if (mc + 64 < M) load(a0, b0, mc + 64);
      compute(a1, b1);
    }
  };
  if (yr.has_add || (k0 < xr.ksplit && k0 + 32 > xr.ksplit)) run(std::integral_constant<int, 2>());
  else if (k0 < xr.ksplit) run(std::integral_constant<int, 0>());
  else run(std::integral_constant<int, 1>());
  if (!yr.has_add) {                                          // modes 0, 1 leave the scale to the end: the products are linear in it
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] *= yr.sc;
    colsum *= yr.sc;
  }
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int n = n0 + crow32(g, lh);
    if (n < N && k < Kin) {
      float* p = dW + (long)n * ldw + k;
      *p = accumulate ? *p + acc[g] : acc[g];
    }
  }
  if (db && k0 == 0) {
    colsum = half_sum(colsum);
    if (lh == 0 && a_ok) db[n0 + li] = accumulate ? db[n0 + li] + colsum : colsum;
  }
}

struct FwdLayer {
  Comp A; const float* W; const float* bias; float* C; int ldc, act;
  int M, N, K;
  int* zero2;                     // two words workgroup 0 clears (the cross entropy's status word and ticket: ce.hip), or NULL
};

template <bool VEC, bool BF>
__global__ __launch_bounds__(kThreads) void head_fwd_kernel(const FwdLayer L) {
  __shared__ __attribute__((aligned(16))) float smem[kWaves * 2 * 32 * LDR];
  const int ntn = (L.N + 31) / 32;
  const int mt = blockIdx.x / ntn, nt = blockIdx.x % ntn;
  TileOut o = {};
  o.C = L.C; o.ldc = L.ldc; o.bias = L.bias; o.act = L.act; o.hsplit = 0x7fffffff;
  if (L.zero2 && blockIdx.x == 0 && threadIdx.x == 0) { L.zero2[0] = 0; L.zero2[1] = 0; }
  head_fwd_tile<VEC, BF>(L.A, L.W, L.K, o, L.M, L.N, L.K, 32 * mt, 32 * nt, smem);
}

struct BwdLayer {
  DY Y;                           // dY [M][N] of this layer (pre-activation gradient)
  const float* W;                 // [N][Kin]
  Comp X;                         // the layer's input [M][Kin] (composed)
  TileOut o;                      // where dX goes
  float* dW; float* db;
  int M, N, Kin, accumulate;
  int nx;                         // number of dX workgroups (0: the layer's input needs no gradient)
};

template <bool VEC, bool BF>
__global__ __launch_bounds__(kThreads) void head_bwd_kernel(const BwdLayer L) {
  __shared__ __attribute__((aligned(16))) float smem[kWaves * 2 * 32 * LDR];
  if ((int)blockIdx.x < L.nx) {
    const int ntk = (L.Kin + 31) / 32;
    const int mt = blockIdx.x / ntk, kt = blockIdx.x % ntk;
    head_dx_tile<VEC, BF>(L.Y, L.W, L.Kin, L.o, L.M, L.N, L.Kin, 32 * mt, 32 * kt, smem);
    return;
  }
  const int ntk = (L.Kin + 31) / 32, ntn = (L.N + 31) / 32;
  const int tile = ((int)blockIdx.x - L.nx) * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (tile >= ntk * ntn) return;
  dw_tile<BF>(L.Y, L.X, L.dW, L.Kin, L.db, L.M, L.N, L.Kin, 32 * (tile / ntk), 32 * (tile % ntk), L.accumulate);
}

// ---- the same tiles inside ONE launch per direction (COATTN_HEAD_PERSISTENT, opt-in) ---------------------------------
// The layers of a direction are phases of one kernel, separated by a grid-wide barrier instead of a kernel boundary
// (VERDICT r2 asked for this form first).  Rounds 2-5 built the barrier on device fences (every wave drains its stores, one
// lane's agent-scope RELEASE, an arrival counter, polling, one agent-scope ACQUIRE): on a multi-XCD part a release writes an
// XCD's whole L2 back and an acquire invalidates it -- 186 us for the two directions against 100 us of per-layer launches.
// Round 6: NO fence (186 -> 145 us), and a two-level barrier (145 -> 128 us) -- still behind the per-layer launches, which stay
// the default (LAB_NOTES A6.7).  Everything one phase hands to the next (h_w, h_p, h_s; dz_s, dz_p, dz_w) is STORED with agent-scope
// stores (write-through: acknowledged when visible device-wide) and LOADED with agent-coherent loads (cache-policy bit sc1:
// what an atomic monotonic load at agent scope compiles to) -- the tiles' COH instantiations; every wave waits for its own
// stores (s_waitcnt vmcnt(0)), workgroup barrier, one lane's relaxed agent-scope arrival, relaxed polling with s_sleep,
// workgroup barrier.  Weights, inputs and the previous launch's saved activations stay ordinary cached loads.  The
// grid is at most one workgroup per CU, so every workgroup is resident; the spin is bounded: a time-out raises bar[1], every
// workgroup then leaves its barriers with stale data, and workgroup 0 -- which owns element [0][0] of the last phase's
// output -- writes NaN over it when the kernel ends (nobody read bar[1] before): the forward's logits[0][0]
// turns the loss of that call into NaN, the backward's first gradient element is NaN.  Not combined with the
// reduced-precision flag (the one-launch kernels exist for the exact tiles only).
// Two levels, so that no word sees more than ~32 arrivals or ~32 pollers: workgroups are grouped by blockIdx.x & 7 (the XCD the
// round-robin dispatch puts them on; any grouping is correct).  A workgroup arrives at its group's counter; the group's last
// arriver of the phase arrives at the grid's counter, waits for all groups there and then publishes the phase number in the
// group's release word, which the others of the group poll.  Words 64 bytes apart: bar[0] grid counter, bar[1] time-out flag,
// bar[16 g + 16] group g's counter, bar[16 g + 24] its release word; all zeroed in front of the launch.
constexpr int kBarWords = 16 * 9;
__device__ __forceinline__ void grid_barrier(unsigned* bar, unsigned phase) {   // phase = 1, 2, 3: the barrier behind layer phase - 1
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // every storing wave: its agent-scope stores are acknowledged
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned grid = gridDim.x, g = blockIdx.x & 7u, ngroups = grid < 8u ? grid : 8u;
    const unsigned n_g = (grid - g + 7u) / 8u;                 // workgroups of this group
    unsigned* cnt = bar + 16 * g + 16;
    unsigned* rel = bar + 16 * g + 24;
    auto load = [](unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    unsigned spins = 0;
    auto timed_out = [&]() {
      if (++spins > (1u << 22)) { __hip_atomic_store(bar + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return true; }
      return load(bar + 1) != 0u && (spins & 1023u) == 0u;
    };
    const unsigned t = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t + 1u == phase * n_g) {                               // the group's last arriver of this phase
      __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      while (load(bar) < phase * ngroups) { __builtin_amdgcn_s_sleep(2); if (timed_out()) break; }
      __hip_atomic_store(rel, phase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      while (load(rel) < phase) { __builtin_amdgcn_s_sleep(2); if (timed_out()) break; }
    }
  }
  __syncthreads();
}

struct FwdAll { FwdLayer L[4]; unsigned* bar; float* poison; };
// after the last phase: make a barrier time-out visible in the values (see above)
__device__ __forceinline__ void poison_on_timeout(unsigned* bar, float* poison) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this workgroup's own stores of the last phase are out
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0 && __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)
    *poison = __builtin_nanf("");
}
template <bool VEC>
__global__ __launch_bounds__(kThreads) void head_fwd_persistent_kernel(const FwdAll a) {
  __shared__ __attribute__((aligned(16))) float smem[kWaves * 2 * 32 * LDR];
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const FwdLayer& L = a.L[l];
    const int ntn = (L.N + 31) / 32, ntiles = ((L.M + 31) / 32) * ntn;
    TileOut o = {};
    o.C = L.C; o.ldc = L.ldc; o.bias = L.bias; o.act = L.act; o.hsplit = 0x7fffffff;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
      head_fwd_tile<VEC, false, true>(L.A, L.W, L.K, o, L.M, L.N, L.K, 32 * (t / ntn), 32 * (t % ntn), smem);
      __syncthreads();                                        // the reduction slots become staging images again
    }
    if (l < 3) grid_barrier(a.bar, (unsigned)(l + 1));
  }
  poison_on_timeout(a.bar, a.poison);
}

struct BwdAll { BwdLayer L[4]; unsigned* bar; float* poison; bool vec0; };
template <bool VEC>
__global__ __launch_bounds__(kThreads) void head_bwd_persistent_kernel(const BwdAll a) {
  __shared__ __attribute__((aligned(16))) float smem[kWaves * 2 * 32 * LDR];
  for (int l = 0; l < 4; ++l) {
    const BwdLayer& L = a.L[l];
    const int ntk = (L.Kin + 31) / 32, ntn = (L.N + 31) / 32, ngroups = (ntk * ntn + kWaves - 1) / kWaves;
    for (int wk = blockIdx.x; wk < L.nx + ngroups; wk += gridDim.x) {
      if (wk < L.nx) {
        // (the last layer's dY rows are K floats: whole-line staging only when the host found them aligned)
        const int m0 = 32 * (wk / ntk), k0 = 32 * (wk % ntk);
        if (VEC && (l > 0 || a.vec0)) head_dx_tile<true, false, true>(L.Y, L.W, L.Kin, L.o, L.M, L.N, L.Kin, m0, k0, smem);
        else head_dx_tile<false, false, true>(L.Y, L.W, L.Kin, L.o, L.M, L.N, L.Kin, m0, k0, smem);
        __syncthreads();
      } else {
        const int tile = (wk - L.nx) * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if (tile < ntk * ntn) dw_tile<false, true>(L.Y, L.X, L.dW, L.Kin, L.db, L.M, L.N, L.Kin, 32 * (tile / ntk), 32 * (tile % ntk), L.accumulate);
      }
    }
    if (l < 3) grid_barrier(a.bar, (unsigned)(l + 1));
  }
  poison_on_timeout(a.bar, a.poison);
}

inline int kpad(int K) { return (K + 3) & ~3; }   // row stride of the saved d loss / d logits: whole-line staging in the backward
struct HeadSaved { size_t hw, hp, hs, dl, rl, st, total; };
inline HeadSaved head_saved(int B, int d, int mlp, int K) {
  HeadSaved s;
  size_t o = 0;
  s.hw = o; o += al64((size_t)B * d);
  s.hp = o; o += al64((size_t)B * d);
  s.hs = o; o += al64((size_t)B * mlp);
  s.dl = o; o += al64((size_t)B * kpad(K)); // d loss / d logits (written by the forward when labels are given), rows padded to 16 bytes
  s.rl = o; o += al64((size_t)B);          // row losses
  s.st = o; o += 64 + 192;                 // status word of the cross entropy (label out of range); + the one-launch form's barrier words
  s.total = o;
  return s;
}
struct HeadBwd { size_t dzs, dzp, dzw, total; };
inline HeadBwd head_bwd(int B, int d, int mlp) {
  HeadBwd s;
  size_t o = 0;
  s.dzs = o; o += al64((size_t)B * mlp);
  s.dzp = o; o += al64((size_t)B * d);
  s.dzw = o; o += al64((size_t)B * d);
  s.total = o;
  return s;
}

int check_dims(int B, int d, int mlp, int K, int dtype) {
  CA_CHECK_ARG(dtype == COATTN_F32, "head: unsupported dtype %d (only COATTN_F32)", dtype);
  CA_CHECK_ARG(B > 0 && B <= (1 << 20) && d > 0 && d <= 16384 && mlp > 0 && mlp <= 16384 && K > 0 && K <= (1 << 20),
               "head: bad B=%d d=%d mlp=%d K=%d", B, d, mlp, K);
  const long widest = 2L * d > mlp ? (2L * d > K ? 2L * d : K) : (mlp > K ? mlp : K);
  // every operand is addressed through a buffer descriptor with 32-bit byte offsets below 1 GB
  CA_CHECK_ARG((long)B * widest < (1L << 28) && (long)mlp * 2 * d < (1L << 28) && (long)K * mlp < (1L << 28),
               "head: B=%d d=%d mlp=%d K=%d is beyond the 1 GB per operand this kernel addresses", B, d, mlp, K);
  return 0;
}

int launch_fwd(const FwdLayer& L, bool vec, bool bf, hipStream_t s) {
  const dim3 grid((unsigned)(((L.M + 31) / 32) * ((L.N + 31) / 32))), block(kThreads);
  if (vec && bf) hipLaunchKernelGGL((head_fwd_kernel<true, true>), grid, block, 0, s, L);
  else if (vec) hipLaunchKernelGGL((head_fwd_kernel<true, false>), grid, block, 0, s, L);
  else if (bf) hipLaunchKernelGGL((head_fwd_kernel<false, true>), grid, block, 0, s, L);
  else hipLaunchKernelGGL((head_fwd_kernel<false, false>), grid, block, 0, s, L);
  CA_CHECK_LAUNCH("head_fwd");
  return 0;
}
int launch_bwd(BwdLayer& L, bool want_dx, bool vec, bool bf, hipStream_t s) {
  const int ntk = (L.Kin + 31) / 32, ntn = (L.N + 31) / 32;
  L.nx = want_dx ? ((L.M + 31) / 32) * ntk : 0;
  const dim3 grid((unsigned)(L.nx + (ntk * ntn + kWaves - 1) / kWaves)), block(kThreads);
  if (vec && bf) hipLaunchKernelGGL((head_bwd_kernel<true, true>), grid, block, 0, s, L);
  else if (vec) hipLaunchKernelGGL((head_bwd_kernel<true, false>), grid, block, 0, s, L);
  else if (bf) hipLaunchKernelGGL((head_bwd_kernel<false, true>), grid, block, 0, s, L);
  else hipLaunchKernelGGL((head_bwd_kernel<false, false>), grid, block, 0, s, L);
  CA_CHECK_LAUNCH("head_bwd");
  return 0;
}

}  // namespace

// cross entropy rows + mean (ce.hip)
int launch_ce_rows(const float* logits, const void* labels, float* row_loss, float* dlogits, float* loss, int B, int K, int* status, hipStream_t s, int ldd, bool zeroed);
int launch_soft_rows(const float* logits, const void* ans_idx, const void* ans_score, int A, int kind, float* row_loss, float* dlogits, float* loss, int B, int K, int* status, hipStream_t s, int ldd, bool zeroed);
int check_soft_targets(const char* what, const void* ans_idx, const void* ans_score, int A, int kind);
int head_status_check(const int* status_dev, void* stream);

namespace {
// what the loss behind the logits is computed against: int64 labels (kind 0), soft answer targets (COATTN_LOSS_*), or nothing
struct HeadTarget { const void* labels; const void* ans_idx; const void* ans_score; int A, kind; };
}  // namespace

extern "C" int coattn_head_workspace_bytes(int B, int d, int mlp, int K, int dtype, size_t* saved, size_t* ws_bwd) {
  CA_TRY(check_dims(B, d, mlp, K, dtype));
  if (saved) *saved = head_saved(B, d, mlp, K).total * sizeof(float);
  if (ws_bwd) *ws_bwd = (head_bwd(B, d, mlp).total + 192) * sizeof(float);      // + the barrier words of the one-launch form (kBarWords)
  return 0;
}

static int head_forward(const void* const* v, const void* const* q, const coattn_head_params* p, const HeadTarget& tg,
                        void* logits, void* loss, void* saved, int B, int d, int mlp, int K, int dtype, int flags,
                        void* stream) {
  const void* labels = tg.kind ? tg.ans_idx : tg.labels;     // (non-NULL: a loss follows the logits)
  CA_TRY(check_dims(B, d, mlp, K, dtype));
  CA_CHECK_ARG(v && q && p && logits && saved, "head_forward: null argument");
  for (int l = 0; l < 3; ++l) CA_CHECK_ARG(v[l] && q[l], "head_forward: v[%d] / q[%d] is null", l, l);
  CA_CHECK_ARG(p->W_w && p->b_w && p->W_p && p->b_p && p->W_s && p->b_s && p->W_h && p->b_h, "head_forward: null parameter pointer");
  CA_CHECK_ARG((labels != nullptr) == (loss != nullptr), "head_forward: labels and loss go together");
  hipStream_t s = (hipStream_t)stream;
  float* sv = (float*)saved;
  const HeadSaved hs = head_saved(B, d, mlp, K);
  bool vec = (d % 32) == 0 && (mlp % 32) == 0 && al16(sv);
  for (int l = 0; l < 3; ++l) vec = vec && al16(v[l]) && al16(q[l]);
  vec = vec && al16(p->W_w) && al16(p->W_p) && al16(p->W_s) && al16(p->W_h);
  FwdLayer Ls[4] = {};
  // h_w = tanh(W_w (q_w + v_w) + b_w)
  Ls[0].A = Comp{(const float*)q[0], (const float*)v[0], nullptr, d, d, 0};
  Ls[0].W = (const float*)p->W_w; Ls[0].bias = (const float*)p->b_w; Ls[0].C = sv + hs.hw; Ls[0].ldc = d; Ls[0].act = 1; Ls[0].N = d; Ls[0].K = d;
  // h_p = tanh(W_p [q_p + v_p | h_w] + b_p)
  Ls[1].A = Comp{(const float*)q[1], (const float*)v[1], sv + hs.hw, d, d, d};
  Ls[1].W = (const float*)p->W_p; Ls[1].bias = (const float*)p->b_p; Ls[1].C = sv + hs.hp; Ls[1].ldc = d; Ls[1].act = 1; Ls[1].N = d; Ls[1].K = 2 * d;
  // h_s = tanh(W_s [q_s + v_s | h_p] + b_s)
  Ls[2].A = Comp{(const float*)q[2], (const float*)v[2], sv + hs.hp, d, d, d};
  Ls[2].W = (const float*)p->W_s; Ls[2].bias = (const float*)p->b_s; Ls[2].C = sv + hs.hs; Ls[2].ldc = mlp; Ls[2].act = 1; Ls[2].N = mlp; Ls[2].K = 2 * d;
  // logits = W_h h_s + b_h
  Ls[3].A = Comp{nullptr, nullptr, sv + hs.hs, 0, 0, mlp};
  Ls[3].W = (const float*)p->W_h; Ls[3].bias = (const float*)p->b_h; Ls[3].C = (float*)logits; Ls[3].ldc = K; Ls[3].act = 0; Ls[3].N = K; Ls[3].K = mlp;
  for (int l = 0; l < 4; ++l) Ls[l].M = B;
  CA_CHECK_ARG(!((flags & COATTN_HEAD_PERSISTENT) && (flags & COATTN_FLAG_BF16_PROJ)),
               "head_forward: COATTN_HEAD_PERSISTENT has no reduced-precision form (drop one of the two flags)");
  bool ce_zeroed = false;
  if (flags & COATTN_HEAD_PERSISTENT) {
    FwdAll all = {};
    all.poison = (float*)logits;
    int most = 0;
    for (int l = 0; l < 4; ++l) { all.L[l] = Ls[l]; const int t = ((B + 31) / 32) * ((Ls[l].N + 31) / 32); most = t > most ? t : most; }
    all.bar = reinterpret_cast<unsigned*>(sv + hs.st) + 64;         // (behind the cross entropy's status words)
    CA_CHECK_ARG(hipMemsetAsync(all.bar, 0, kBarWords * 4, s) == hipSuccess, "head_forward: clearing the barrier words failed");
    const unsigned grid = (unsigned)(most < 256 ? most : 256);      // at most one workgroup per CU: all resident
    if (vec) hipLaunchKernelGGL(head_fwd_persistent_kernel<true>, dim3(grid), dim3(kThreads), 0, s, all);
    else hipLaunchKernelGGL(head_fwd_persistent_kernel<false>, dim3(grid), dim3(kThreads), 0, s, all);
    CA_CHECK_LAUNCH("head_fwd_persistent");
  } else {
    const bool bf = (flags & COATTN_FLAG_BF16_PROJ) != 0;
    if (labels) { Ls[3].zero2 = reinterpret_cast<int*>(sv + hs.st); ce_zeroed = true; }   // (the logits layer clears the loss's two words)
    for (int l = 0; l < 4; ++l) CA_TRY(launch_fwd(Ls[l], vec, bf, s));
  }
  if (tg.kind) CA_TRY(launch_soft_rows((const float*)logits, tg.ans_idx, tg.ans_score, tg.A, tg.kind, sv + hs.rl, sv + hs.dl, (float*)loss, B, K, reinterpret_cast<int*>(sv + hs.st), s, kpad(K), ce_zeroed));
  else if (labels) CA_TRY(launch_ce_rows((const float*)logits, labels, sv + hs.rl, sv + hs.dl, (float*)loss, B, K, reinterpret_cast<int*>(sv + hs.st), s, kpad(K), ce_zeroed));
  return 0;
}

extern "C" int coattn_head_forward(const void* const* v, const void* const* q, const coattn_head_params* p, const void* labels,
                                   void* logits, void* loss, void* saved, int B, int d, int mlp, int K, int dtype, int flags,
                                   void* stream) {
  return head_forward(v, q, p, HeadTarget{labels, nullptr, nullptr, 0, 0}, logits, loss, saved, B, d, mlp, K, dtype, flags, stream);
}

// as coattn_head_forward with soft answer targets: the same four layers, the same `saved` layout (d loss / d logits with padded
// rows, row losses, status word), the soft-target rows kernel (ce.hip) as the one launch behind the logits
extern "C" int coattn_head_forward_soft(const void* const* v, const void* const* q, const coattn_head_params* p,
                                        const void* ans_idx, const void* ans_score, int A, int kind, void* logits, void* loss,
                                        void* saved, int B, int d, int mlp, int K, int dtype, int flags, void* stream) {
  CA_TRY(check_soft_targets("head_forward_soft", ans_idx, ans_score, A, kind));
  CA_CHECK_ARG(loss, "head_forward_soft: null loss");
  return head_forward(v, q, p, HeadTarget{nullptr, ans_idx, ans_score, A, kind}, logits, loss, saved, B, d, mlp, K, dtype, flags, stream);
}

extern "C" int coattn_head_status(const void* saved, int B, int d, int mlp, int K, void* stream) {
  CA_TRY(check_dims(B, d, mlp, K, COATTN_F32));
  CA_CHECK_ARG(saved, "head_status: null argument");
  return head_status_check(reinterpret_cast<const int*>((const float*)saved + head_saved(B, d, mlp, K).st), stream);
}

extern "C" int coattn_head_backward(const void* const* v, const void* const* q, const coattn_head_params* p, const void* saved,
                                    const void* g_loss, const void* g_logits, void* const* dv, void* const* dq,
                                    const coattn_head_param_grads* pg, int accumulate, void* ws, int B, int d, int mlp, int K,
                                    int dtype, int flags, void* stream) {
  CA_TRY(check_dims(B, d, mlp, K, dtype));
  CA_CHECK_ARG(v && q && p && saved && pg && ws, "head_backward: null argument");
  CA_CHECK_ARG(g_loss || g_logits, "head_backward: neither g_loss nor g_logits given");
  for (int l = 0; l < 3; ++l) CA_CHECK_ARG(v[l] && q[l], "head_backward: v[%d] / q[%d] is null", l, l);
  if (dv) for (int l = 0; l < 3; ++l) CA_CHECK_ARG(dv[l], "head_backward: dv[%d] is null", l);
  CA_CHECK_ARG(!dq || dv, "head_backward: dq without dv");
  CA_CHECK_ARG(pg->dW_w && pg->db_w && pg->dW_p && pg->db_p && pg->dW_s && pg->db_s && pg->dW_h && pg->db_h,
               "head_backward: null parameter-gradient pointer");
  hipStream_t s = (hipStream_t)stream;
  const float* sv = (const float*)saved;
  float* w = (float*)ws;
  const HeadSaved hs = head_saved(B, d, mlp, K);
  const HeadBwd hb = head_bwd(B, d, mlp);
  bool vec = (d % 32) == 0 && (mlp % 32) == 0 && al16(sv) && al16(w);
  // dY rows of the last layer: the saved d loss / d logits has padded rows; an added g_logits has rows of K floats
  const bool vec_h = vec && (!g_logits || ((K % 4) == 0 && al16(g_logits)));
  auto D = [&](int l) { return dv ? (float*)dv[l] : nullptr; };
  auto D2 = [&](int l) { return (dq && dq[l] != dv[l]) ? (float*)dq[l] : nullptr; };
  BwdLayer Ls[4] = {};
  // logits = W_h h_s + b_h:  d h_s -> d z_s = d h_s (1 - h_s^2);  dW_h = dlogits^T h_s
  {
    BwdLayer& L = Ls[0];
    if (g_loss) L.Y = DY{sv + hs.dl, (const float*)g_loss, (const float*)g_logits, kpad(K), K};
    else L.Y = DY{(const float*)g_logits, nullptr, nullptr, K, K};
    L.W = (const float*)p->W_h; L.X = Comp{nullptr, nullptr, sv + hs.hs, 0, 0, mlp};
    L.o = TileOut{}; L.o.hsplit = 0; L.o.hid = sv + hs.hs; L.o.ldhid = mlp; L.o.Ch = w + hb.dzs; L.o.ldch = mlp;
    L.dW = (float*)pg->dW_h; L.db = (float*)pg->db_h; L.N = K; L.Kin = mlp;
  }
  // h_s = tanh(W_s [q_s + v_s | h_p] + b_s):  d(q_s + v_s), d z_p;  dW_s
  {
    BwdLayer& L = Ls[1];
    L.Y = DY{w + hb.dzs, nullptr, nullptr, mlp};
    L.W = (const float*)p->W_s; L.X = Comp{(const float*)q[2], (const float*)v[2], sv + hs.hp, d, d, d};
    L.o = TileOut{}; L.o.C = D(2); L.o.C2 = D2(2); L.o.ldc = d; L.o.hsplit = d; L.o.hid = sv + hs.hp; L.o.ldhid = d;
    L.o.Ch = w + hb.dzp; L.o.ldch = d;
    L.dW = (float*)pg->dW_s; L.db = (float*)pg->db_s; L.N = mlp; L.Kin = 2 * d;
  }
  // h_p = tanh(W_p [q_p + v_p | h_w] + b_p)
  {
    BwdLayer& L = Ls[2];
    L.Y = DY{w + hb.dzp, nullptr, nullptr, d};
    L.W = (const float*)p->W_p; L.X = Comp{(const float*)q[1], (const float*)v[1], sv + hs.hw, d, d, d};
    L.o = TileOut{}; L.o.C = D(1); L.o.C2 = D2(1); L.o.ldc = d; L.o.hsplit = d; L.o.hid = sv + hs.hw; L.o.ldhid = d;
    L.o.Ch = w + hb.dzw; L.o.ldch = d;
    L.dW = (float*)pg->dW_p; L.db = (float*)pg->db_p; L.N = d; L.Kin = 2 * d;
  }
  // h_w = tanh(W_w (q_w + v_w) + b_w)
  {
    BwdLayer& L = Ls[3];
    L.Y = DY{w + hb.dzw, nullptr, nullptr, d};
    L.W = (const float*)p->W_w; L.X = Comp{(const float*)q[0], (const float*)v[0], nullptr, d, d, 0};
    L.o = TileOut{}; L.o.C = D(0); L.o.C2 = D2(0); L.o.ldc = d; L.o.hsplit = 0x7fffffff;
    L.dW = (float*)pg->dW_w; L.db = (float*)pg->db_w; L.N = d; L.Kin = d;
  }
  for (int l = 0; l < 4; ++l) { Ls[l].M = B; Ls[l].accumulate = accumulate; }
  CA_CHECK_ARG(!((flags & COATTN_HEAD_PERSISTENT) && (flags & COATTN_FLAG_BF16_PROJ)),
               "head_backward: COATTN_HEAD_PERSISTENT has no reduced-precision form (drop one of the two flags)");
  if (flags & COATTN_HEAD_PERSISTENT) {
    BwdAll all = {};
    all.poison = dv ? (float*)dv[0] : (float*)pg->dW_w;          // element [0][0] of the last phase's first tile: workgroup 0 owns it
    for (int l = 0; l < 4; ++l) {
      all.L[l] = Ls[l];
      all.L[l].nx = (l < 3 || dv) ? ((B + 31) / 32) * ((Ls[l].Kin + 31) / 32) : 0;
    }
    all.vec0 = vec_h;
    all.bar = reinterpret_cast<unsigned*>(w + hb.total);            // two words behind the backward workspace
    CA_CHECK_ARG(hipMemsetAsync(all.bar, 0, kBarWords * 4, s) == hipSuccess, "head_backward: clearing the barrier words failed");
    if (vec) hipLaunchKernelGGL(head_bwd_persistent_kernel<true>, dim3(256), dim3(kThreads), 0, s, all);
    else hipLaunchKernelGGL(head_bwd_persistent_kernel<false>, dim3(256), dim3(kThreads), 0, s, all);
    CA_CHECK_LAUNCH("head_bwd_persistent");
    return 0;
  }
  const bool bf = (flags & COATTN_FLAG_BF16_PROJ) != 0;
  CA_TRY(launch_bwd(Ls[0], true, vec_h, bf, s));
  CA_TRY(launch_bwd(Ls[1], true, vec, bf, s));
  CA_TRY(launch_bwd(Ls[2], true, vec, bf, s));
  return launch_bwd(Ls[3], dv != nullptr, vec, bf, s);
}
