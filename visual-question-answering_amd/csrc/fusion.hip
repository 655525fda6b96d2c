// Fusion head of the baseline model on gfx950 (reference model.py VQABaselineNet: the tail of ImageBaselineEncoder.forward,
// QuestionBaselineEncoder.embedding_layer, VQABaselineNet.forward behind the two encoders), include/coattn_fusion.h v0.26.0:
//
//   inv_b  = 1 / max(||f_b||, 1e-12)                          F.normalize(fc7, p=2, dim=1), never stored as a [B, Di] copy
//   e_i    = tanh(inv_b (f W_i^T) + b_i)                      [B, J]    the row scale rides in the epilogue
//   e_q    = tanh(h W_q^T + b_q)                              [B, J]
//   m      = tanh(mask scale ((e_i e_q) W_m^T + b_m))         [B, Mh]   Linear -> Dropout -> Tanh: the reference's order
//   logits = m W_f^T + b_f                                    [B, K]
//
// The products are the attention head's kind (head.hip: B = 160 rows, contraction 1000 - 4096), so the tiles are its form and
// the forward and dX tile loops are shared with it (head_tile.h): 32 x 32 output tiles on v_mfma_f32_32x32x2_f32, one
// 512-thread workgroup each, the contraction split over the eight waves and summed through LDS in wave order; weight-gradient
// tiles one wave each, in the launch of their layer's dX tiles; unconditional raw buffer loads.  This file's own are its
// operand forms: the product e_i e_q as the A operand of m (MatOp: a policy of the shared loops) and the X operand of dW_m (j
// is never stored), the row scale inv_b on the dY operand of dW_i (db_i sums the unscaled values) -- the weight-gradient tile
// is all operand form and stays here whole --, and the epilogues: row scale, Philox dropout + tanh, the two tanh' products of
// one dX tile.  The dropout mask is v0.19.0's (philox.h, with dropout.hip) over element i = b Mh + n, drawn in the epilogue of
// m and regenerated in the epilogue of dpre: nothing of it is stored.  Forward: 4 launches {e_q, row norms} {e_i} {m}
// {logits, step + 1}; backward: 3 launches {dW_f, db_f, dpre} {dW_m, db_m, dp_i, dp_q} {dW_i, db_i, dW_q, db_q, dh}.
// Deterministic: no atomics.
#include "head_tile.h"
#include "philox.h"
#include <type_traits>
#include "../../include/coattn_fusion.h"

namespace {

// the tight extent of a [rows][ld] operand whose rows hold `cols` floats: rows >= `rows` start past it and read 0
__device__ __forceinline__ rsrc_t mat_rsrc(const float* p, int rows, int ld, int cols) {
  return mk_rsrc(p, ((long)(rows - 1) * ld + cols) * 4);
}

// the staged operand of head_tile.h's loops: X(m, k) = x0[m][k] (PROD: * x1[m][k]) over [M][K], rows ld floats apart;
// VEC: the rows are 16-byte aligned (g_logits with K % 4 != 0 is not)
template <bool VEC, bool PROD>
struct MatOp {
  rsrc_t r0, r1; int ld, K; Stage s0, s1;
  __device__ __forceinline__ MatOp(const float* x0, const float* x1, int M, int ld_, int K_)
      : r0(mat_rsrc(x0, M, ld_, K_)), r1(mat_rsrc(PROD ? x1 : x0, M, ld_, K_)), ld(ld_), K(K_) {}
  __device__ __forceinline__ void load(int lane, int m0, int k0) {
    stage_lin<VEC>(s0, r0, ld, K, lane, m0, k0);
    if constexpr (PROD) stage_lin<VEC>(s1, r1, ld, K, lane, m0, k0);
  }
  __device__ __forceinline__ void store(float* img, int lane) {
    if constexpr (PROD) {                            // both register sets are kept until here: no load is waited for early
#pragma unroll
      for (int i = 0; i < 4; ++i) s0.v[i] = s0.v[i] * s1.v[i];
    }
    stage_store<VEC>(s0, img, lane);
  }
};

// ---- dW tile (one WAVE): dW[n][k'] (+)= sum_m Y[m][n] (SCALE: * inv[m]) X(m, k');  db[n] (+)= sum_m Y[m][n], unscaled, from
// the tiles with k0 = 0.  X(m, k) = x0[m][k] (PROD: * x1[m][k]).  Rows in increasing m, two per MFMA.
struct DwJob {
  const float* Y; int ldy;        // [M][N]
  const float* inv;               // [M] (SCALE)
  const float* x0; const float* x1; int ldx;
  float* dW; float* db;           // [N][Kin] dense, [N]
  int N, Kin;
};
template <bool SCALE, bool PROD>
__device__ __forceinline__ void dw_tile(const DwJob& J, int M, int n0, int k0, int accumulate) {
  const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const rsrc_t yr = mat_rsrc(J.Y, M, J.ldy, J.N), ir = mk_rsrc(SCALE ? J.inv : nullptr, (long)M * 4);
  const rsrc_t xr = mat_rsrc(J.x0, M, J.ldx, J.Kin), xr1 = mat_rsrc(PROD ? J.x1 : J.x0, M, J.ldx, J.Kin);
  const bool a_ok = n0 + li < J.N;
  const int k = k0 + li;
  // a lane per tile column, two batch rows per instruction (the lane halves: rows m + lh); rows >= M are out of range and read 0
  const int avoff = a_ok ? (lh * J.ldy + n0 + li) * 4 : kOut;
  const int xvoff = k < J.Kin ? (lh * J.ldx + k) * 4 : kOut;
  f32x16 acc = {};
  float colsum = 0.f;
  float a0[16], b0[16], a1[16], b1[16], s0[16], s1[16];
  auto load = [&](float (&fa)[16], float (&fb)[16], float (&fs)[16], int mc) {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int m = mc + 2 * s;
      fa[s] = bl1(yr, avoff, m * J.ldy * 4);
      if constexpr (SCALE) fs[s] = bl1(ir, lh * 4, m * 4);
      fb[s] = bl1(xr, xvoff, m * J.ldx * 4);
      if constexpr (PROD) fs[s] = bl1(xr1, xvoff, m * J.ldx * 4);
    }
  };
  auto compute = [&](const float (&fa)[16], const float (&fb)[16], const float (&fs)[16]) {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      float a = fa[s], b = fb[s];
      if constexpr (SCALE) a *= fs[s];
      if constexpr (PROD) b *= fs[s];
      acc = mfma2(a, b, acc);
      colsum += fa[s];
    }
  };
  load(a0, b0, s0, 0);
  for (int mc = 0; mc < M; mc += 64) {                        // two chunks per trip: the register sets alternate
    if (mc + 32 < M) load(a1, b1, s1, mc + 32);
    compute(a0, b0, s0);
    if (mc + 32 >= M) break;
    if (mc + 64 < M) load(a0, b0, s0, mc + 64);
    compute(a1, b1, s1);
  }
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int n = n0 + crow32(g, lh);
    if (n < J.N && k < J.Kin) {
      float* p = J.dW + (long)n * J.Kin + k;
      *p = accumulate ? *p + acc[g] : acc[g];
    }
  }
  if (k0 == 0) {
    colsum = half_sum(colsum);
    if (lh == 0 && a_ok) J.db[n0 + li] = accumulate ? J.db[n0 + li] + colsum : colsum;
  }
}

// ---- forward launches ----------------------------------------------------------------------------------------------------
struct FusFwd {
  const float* a0; const float* a1; int lda;   // A operand (a1: the second factor of stage 2)
  const float* W; const float* bias; float* C; // W [N][K], bias [N], output [M][N] dense
  int M, N, K, ntiles;
  const float* f; int ld_f, Di; float* inv;    // stage 0 writes inv from f in its extra workgroups, stage 1 reads it
  unsigned* state; unsigned thr; float scale; int drop, advance;   // stage 2 draws mask step + 1; stage 3 stores step + 1
};

// STAGE 0: e_q tiles + the row norms; 1: e_i; 2: m; 3: logits
template <int STAGE>
__global__ __launch_bounds__(kThreads) void fusion_fwd_kernel(const FusFwd a) {
  __shared__ __attribute__((aligned(16))) float smem[kWaves * 2 * 32 * LDR];
  if (STAGE == 0 && (int)blockIdx.x >= a.ntiles) {
    // ss_b: a wave per row; lane l adds f[b][k]^2 for k = 4 l + 256 t + e in increasing k (one fma chain), the 64 lane sums
    // meet in wave_sum's fixed butterfly
    const int lane = threadIdx.x & 63;
    const int b = __builtin_amdgcn_readfirstlane(((int)blockIdx.x - a.ntiles) * kWaves + (int)(threadIdx.x >> 6));
    if (b >= a.M) return;
    const rsrc_t fr = mat_rsrc(a.f, a.M, a.ld_f, a.Di);
    float ss = 0.f;
    for (int k0 = 0; k0 < a.Di; k0 += 1024) {
      f32x4 v[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = k0 + 256 * t + 4 * lane;
        v[t] = bl4(fr, k < a.Di ? k * 4 : kOut, b * a.ld_f * 4);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = fmaf(v[t][e], v[t][e], ss);
    }
    ss = wave_sum(ss);
    if (lane == 0) a.inv[b] = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    return;
  }
  const int ntn = (a.N + 31) / 32;
  const int m0 = 32 * ((int)blockIdx.x / ntn), n0 = 32 * ((int)blockIdx.x % ntn);
  auto tile = [&](auto epi) {                                // (STAGE 2: the product e_i e_q is the A operand of m)
    fwd_tile<true, false>(MatOp<true, STAGE == 2>(a.a0, a.a1, a.M, a.lda, a.K), mat_rsrc(a.W, a.N, a.K, a.K), a.K, a.M, a.N,
                          a.K, m0, n0, smem, epi);
  };
  if constexpr (STAGE == 0) {
    tile([&](int m, int n, float s) { a.C[(long)m * a.N + n] = tanhf(s + a.bias[n]); });
  } else if constexpr (STAGE == 1) {
    tile([&](int m, int n, float s) { a.C[(long)m * a.N + n] = tanhf(a.inv[m] * s + a.bias[n]); });
  } else if constexpr (STAGE == 2) {
    Drop d = {};
    if (a.drop) d = drop_load(a.state, a.thr, a.scale, 1);
    tile([&](int m, int n, float s) {
      float pre = s + a.bias[n];
      if (a.drop) pre *= drop_factor(d, (unsigned)m * (unsigned)a.N + (unsigned)n);
      a.C[(long)m * a.N + n] = tanhf(pre);
    });
  } else {
    if (a.advance && blockIdx.x == 0 && threadIdx.x == 0) {  // the mask of stage 2 is drawn: its launch is complete
      const unsigned long long step = drop_step(a.state, 1);
      a.state[2] = (unsigned)step;
      a.state[3] = (unsigned)(step >> 32);
    }
    tile([&](int m, int n, float s) { a.C[(long)m * a.N + n] = s + a.bias[n]; });
  }
}

// ---- backward launches ---------------------------------------------------------------------------------------------------
struct FusBwd {
  const float* Y; int ldy; const float* W; int ldw; int Nc, Kout;   // the dX tiles: out(m, k') from Y [M][Nc], W [Nc][Kout]
  DwJob w0, w1;                   // the weight gradients of this launch (stage 2 has two)
  int M, nx, ng0, ng1, accumulate;
  const float* act0; const float* act1;   // stage 0: m; stage 1: e_i, e_q
  float* out0; float* out1;               // stage 0: dpre; stage 1: dp_i, dp_q; stage 2: dh
  unsigned* state; unsigned thr; float scale; int drop;
};

// STAGE 0: {dpre | dW_f, db_f}; 1: {dp_i, dp_q | dW_m, db_m}; 2: {dh | dW_i, db_i, dW_q, db_q}
template <int STAGE, bool VEC>
__global__ __launch_bounds__(kThreads) void fusion_bwd_kernel(const FusBwd a) {
  __shared__ __attribute__((aligned(16))) float smem[kWaves * 2 * 32 * LDR];
  int bid = (int)blockIdx.x;
  if (bid < a.nx) {
    const int ntk = (a.Kout + 31) / 32;
    const int m0 = 32 * (bid / ntk), k0 = 32 * (bid % ntk);
    auto tile = [&](auto epi) {
      dx_tile<false>(MatOp<VEC, false>(a.Y, nullptr, a.M, a.ldy, a.Nc), mat_rsrc(a.W, a.Nc, a.ldw, a.Kout), a.ldw, a.M, a.Nc,
                     a.Kout, m0, k0, smem, epi);
    };
    if constexpr (STAGE == 0) {
      Drop d = {};
      if (a.drop) d = drop_load(a.state, a.thr, a.scale, 0);
      tile([&](int m, int n, float s) {
        const float mv = a.act0[(long)m * a.Kout + n];
        float v = s * (1.f - mv * mv);
        if (a.drop) v *= drop_factor(d, (unsigned)m * (unsigned)a.Kout + (unsigned)n);
        a.out0[(long)m * a.Kout + n] = v;
      });
    } else if constexpr (STAGE == 1) {
      tile([&](int m, int n, float s) {
        const long i = (long)m * a.Kout + n;
        const float ei = a.act0[i], eq = a.act1[i];
        a.out0[i] = s * eq * (1.f - ei * ei);
        a.out1[i] = s * ei * (1.f - eq * eq);
      });
    } else {
      tile([&](int m, int n, float s) { a.out0[(long)m * a.Kout + n] = s; });
    }
    return;
  }
  bid -= a.nx;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  auto run = [&](const DwJob& J, int group, auto scale, auto prod) {
    const int ntk = (J.Kin + 31) / 32, ntn = (J.N + 31) / 32;
    const int tile = group * kWaves + wv;
    if (tile >= ntk * ntn) return;
    dw_tile<decltype(scale)::value, decltype(prod)::value>(J, a.M, 32 * (tile / ntk), 32 * (tile % ntk), a.accumulate);
  };
  typedef std::integral_constant<bool, true> T;
  typedef std::integral_constant<bool, false> F;
  if constexpr (STAGE == 0) run(a.w0, bid, F(), F());
  else if constexpr (STAGE == 1) run(a.w0, bid, F(), T());
  else {
    if (bid < a.ng0) run(a.w0, bid, T(), F());
    else run(a.w1, bid - a.ng0, F(), F());
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct Saved { size_t inv, ei, eq, m, total; };
inline Saved saved_plan(int B, int J, int Mh) {
  Saved s;
  size_t o = 0;
  s.inv = o; o += al64((size_t)B);
  s.ei = o; o += al64((size_t)B * J);
  s.eq = o; o += al64((size_t)B * J);
  s.m = o; o += al64((size_t)B * Mh);
  s.total = o;
  return s;
}
struct BwdWs { size_t dpre, dpi, dpq, total; };
inline BwdWs bwd_plan(int B, int J, int Mh) {
  BwdWs s;
  size_t o = 0;
  s.dpre = o; o += al64((size_t)B * Mh);
  s.dpi = o; o += al64((size_t)B * J);
  s.dpq = o; o += al64((size_t)B * J);
  s.total = o;
  return s;
}

bool width_ok(int n) { return n >= 4 && n <= 8192 && (n % 4) == 0; }
// every operand is addressed through a buffer descriptor with 32-bit byte offsets below 1 GB (2^28 floats)
bool shape_ok(long B, long Di, long H, long J, long Mh, long K) {
  if (B < 1 || K < 2 || !width_ok((int)Di) || !width_ok((int)H) || !width_ok((int)J) || !width_ok((int)Mh)) return false;
  if (Di != (int)Di || H != (int)H || J != (int)J || Mh != (int)Mh) return false;
  const long lim = 1L << 28;
  long widest = Di > H ? Di : H;
  widest = J > widest ? J : widest;
  widest = Mh > widest ? Mh : widest;
  widest = K > widest ? K : widest;
  return (B + 64) * widest < lim && (K + 32) * Mh < lim;     // (B Mh <= 2^31 - 4, the mask's index range, follows)
}

int check_call(const char* what, int B, int Di, int H, int J, int Mh, int K, int dtype, int flags) {
  CA_CHECK_ARG(dtype == COATTN_F32, "%s: unsupported dtype %d (only COATTN_F32)", what, dtype);
  CA_CHECK_ARG(flags == 0, "%s: flags %d not supported: the fusion head is built in exact fp32 only", what, flags);
  CA_CHECK_ARG(shape_ok(B, Di, H, J, Mh, K), "%s: shape B=%d Di=%d H=%d J=%d Mh=%d K=%d not supported (B >= 1; Di, H, J, Mh "
               "multiples of 4 in 4 .. 8192; K >= 2; (B + 64) max(Di, H, J, Mh, K) and (K + 32) Mh below 2^28: coattn_fusion_supported)", what, B, Di,
               H, J, Mh, K);
  return 0;
}
int check_operands(const char* what, const void* f, int64_t ld_f, const void* h, int64_t ld_h, const coattn_fusion_params* p,
                   int B, int Di, int H, float p_drop, const void* state, bool has_saved) {
  CA_CHECK_ARG(f && h && p, "%s: null f, h or params", what);
  CA_CHECK_ARG(p->W_i && p->b_i && p->W_q && p->b_q && p->W_m && p->b_m && p->W_f && p->b_f, "%s: null parameter", what);
  CA_CHECK_ARG(p_drop >= 0.0f && p_drop < 1.0f, "%s: p_drop = %g outside [0, 1) (NaN included)", what, (double)p_drop);
  CA_CHECK_ARG(p_drop == 0.0f || state, "%s: p_drop > 0 needs the dropout state", what);
  CA_CHECK_ARG(p_drop == 0.0f || has_saved, "%s: p_drop > 0 with saved == NULL: inference has no dropout", what);
  CA_CHECK_ARG(ld_f >= Di && ld_h >= H && (ld_f % 4) == 0 && (ld_h % 4) == 0 && ((long)B + 64) * ld_f < (1L << 28) &&
               ((long)B + 64) * ld_h < (1L << 28), "%s: ld_f = %lld, ld_h = %lld: each must be a multiple of 4, at least the row's "
               "width, with (B + 64) ld below 2^28", what, (long long)ld_f, (long long)ld_h);
  CA_CHECK_ARG(al16(f) && al16(h) && al16(p->W_i) && al16(p->b_i) && al16(p->W_q) && al16(p->b_q) && al16(p->W_m) && al16(p->b_m) &&
               al16(p->W_f) && al16(p->b_f) && (((uintptr_t)state) & 3) == 0,
               "%s: f, h and every parameter must be 16-byte aligned (the state: 4)", what);
  return 0;
}

template <int STAGE>
int launch_fwd(const FusFwd& a, int extra, hipStream_t s) {
  hipLaunchKernelGGL(fusion_fwd_kernel<STAGE>, dim3((unsigned)(a.ntiles + extra)), dim3(kThreads), 0, s, a);
  CA_CHECK_LAUNCH("fusion_forward");
  return 0;
}
template <int STAGE>
int launch_bwd(const FusBwd& a, bool vec, hipStream_t s) {
  const dim3 grid((unsigned)(a.nx + a.ng0 + a.ng1));
  if (vec) hipLaunchKernelGGL((fusion_bwd_kernel<STAGE, true>), grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((fusion_bwd_kernel<STAGE, false>), grid, dim3(kThreads), 0, s, a);
  CA_CHECK_LAUNCH("fusion_backward");
  return 0;
}
int groups(int N, int Kin) { return (((N + 31) / 32) * ((Kin + 31) / 32) + kWaves - 1) / kWaves; }

}  // namespace

extern "C" int coattn_fusion_supported(int B, int Di, int H, int J, int Mh, int K, int dtype) {
  return dtype == COATTN_F32 && shape_ok(B, Di, H, J, Mh, K) ? 1 : 0;
}

extern "C" int coattn_fusion_workspace_bytes(int B, int Di, int H, int J, int Mh, int K, int dtype, size_t* saved, size_t* ws_bwd) {
  CA_TRY(check_call("fusion_workspace_bytes", B, Di, H, J, Mh, K, dtype, 0));
  if (saved) *saved = saved_plan(B, J, Mh).total * sizeof(float);
  if (ws_bwd) *ws_bwd = bwd_plan(B, J, Mh).total * sizeof(float);
  return 0;
}

extern "C" int coattn_fusion_forward(const void* f, int64_t ld_f, const void* h, int64_t ld_h, const coattn_fusion_params* p,
                                     void* logits, void* saved, float p_drop, void* drop_state, int B, int Di, int H, int J, int Mh,
                                     int K, int dtype, int flags, void* stream) {
  CA_TRY(check_call("fusion_forward", B, Di, H, J, Mh, K, dtype, flags));
  CA_TRY(check_operands("fusion_forward", f, ld_f, h, ld_h, p, B, Di, H, p_drop, drop_state, saved != nullptr));
  CA_CHECK_ARG(logits, "fusion_forward: null logits");
  CA_CHECK_ARG(al16(logits) && al16(saved), "fusion_forward: logits and saved must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const Saved sp = saved_plan(B, J, Mh);
  float* sv = (float*)saved;
  if (!sv) {   // inference: the activations live in a stream-ordered allocation that is released behind the last launch
    void* tmp = nullptr;
    const hipError_t e = hipMallocAsync(&tmp, sp.total * sizeof(float), s);
    if (e != hipSuccess) {
      coattn_set_error("fusion_forward: stream-ordered scratch allocation failed: %s", hipGetErrorString(e));
      return -3;
    }
    sv = (float*)tmp;
  }
  const bool drop = p_drop > 0.0f;
  const DropHost dh = drop_host(p_drop);
  const int mt = (B + 31) / 32;
  FusFwd a = {};
  a.M = B; a.f = (const float*)f; a.ld_f = (int)ld_f; a.Di = Di; a.inv = sv + sp.inv;
  a.state = (unsigned*)drop_state; a.thr = dh.thr; a.scale = dh.scale; a.drop = drop ? 1 : 0; a.advance = drop ? 1 : 0;
  int rc = 0;
  // 1. e_q = tanh(h W_q^T + b_q), and the row norms in extra workgroups
  a.a0 = (const float*)h; a.lda = (int)ld_h; a.W = (const float*)p->W_q; a.bias = (const float*)p->b_q; a.C = sv + sp.eq;
  a.N = J; a.K = H; a.ntiles = mt * ((J + 31) / 32);
  rc = launch_fwd<0>(a, (B + kWaves - 1) / kWaves, s);
  // 2. e_i = tanh(inv (f W_i^T) + b_i)
  if (!rc) {
    a.a0 = (const float*)f; a.lda = (int)ld_f; a.W = (const float*)p->W_i; a.bias = (const float*)p->b_i; a.C = sv + sp.ei; a.K = Di;
    rc = launch_fwd<1>(a, 0, s);
  }
  // 3. m = tanh(mask scale ((e_i e_q) W_m^T + b_m))
  if (!rc) {
    a.a0 = sv + sp.ei; a.a1 = sv + sp.eq; a.lda = J; a.W = (const float*)p->W_m; a.bias = (const float*)p->b_m; a.C = sv + sp.m;
    a.N = Mh; a.K = J; a.ntiles = mt * ((Mh + 31) / 32);
    rc = launch_fwd<2>(a, 0, s);
  }
  // 4. logits = m W_f^T + b_f; the state's step + 1
  if (!rc) {
    a.a0 = sv + sp.m; a.a1 = nullptr; a.lda = Mh; a.W = (const float*)p->W_f; a.bias = (const float*)p->b_f; a.C = (float*)logits;
    a.N = K; a.K = Mh; a.ntiles = mt * ((K + 31) / 32);
    rc = launch_fwd<3>(a, 0, s);
  }
  if (!saved) (void)hipFreeAsync(sv, s);
  if (!rc) prof_mark(s, "fusion_forward");
  return rc;
}

extern "C" int coattn_fusion_backward(const void* f, int64_t ld_f, const void* h, int64_t ld_h, const coattn_fusion_params* p,
                                      const void* saved, const void* g_logits, void* dh, const coattn_fusion_param_grads* pg,
                                      int accumulate, float p_drop, void* drop_state, void* ws, int B, int Di, int H, int J, int Mh,
                                      int K, int dtype, int flags, void* stream) {
  CA_TRY(check_call("fusion_backward", B, Di, H, J, Mh, K, dtype, flags));
  CA_TRY(check_operands("fusion_backward", f, ld_f, h, ld_h, p, B, Di, H, p_drop, drop_state, true));
  CA_CHECK_ARG(saved && g_logits && pg && ws, "fusion_backward: null saved, g_logits, grads or ws");
  CA_CHECK_ARG(pg->W_i && pg->b_i && pg->W_q && pg->b_q && pg->W_m && pg->b_m && pg->W_f && pg->b_f,
               "fusion_backward: null parameter gradient");
  CA_CHECK_ARG(al16(saved) && al16(g_logits) && al16(dh) && al16(ws) && al16(pg->W_i) && al16(pg->b_i) && al16(pg->W_q) &&
               al16(pg->b_q) && al16(pg->W_m) && al16(pg->b_m) && al16(pg->W_f) && al16(pg->b_f),
               "fusion_backward: saved, g_logits, dh, ws and every gradient must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const Saved sp = saved_plan(B, J, Mh);
  const BwdWs bp = bwd_plan(B, J, Mh);
  const float* sv = (const float*)saved;
  float* w = (float*)ws;
  const DropHost dhh = drop_host(p_drop);
  const int mt = (B + 31) / 32;
  FusBwd a = {};
  a.M = B; a.accumulate = accumulate & 1;
  a.state = (unsigned*)drop_state; a.thr = dhh.thr; a.scale = dhh.scale; a.drop = p_drop > 0.0f ? 1 : 0;
  // 1. dm = g W_f -> dpre = dm (1 - m^2) mask;  dW_f = g^T m, db_f
  a.Y = (const float*)g_logits; a.ldy = K; a.W = (const float*)p->W_f; a.ldw = Mh; a.Nc = K; a.Kout = Mh;
  a.act0 = sv + sp.m; a.out0 = w + bp.dpre;
  a.w0 = DwJob{(const float*)g_logits, K, nullptr, sv + sp.m, nullptr, Mh, (float*)pg->W_f, (float*)pg->b_f, K, Mh};
  a.nx = mt * ((Mh + 31) / 32); a.ng0 = groups(K, Mh); a.ng1 = 0;
  CA_TRY(launch_bwd<0>(a, (K % 4) == 0, s));
  // 2. dj = dpre W_m -> dp_i = dj e_q (1 - e_i^2), dp_q = dj e_i (1 - e_q^2);  dW_m = dpre^T (e_i e_q), db_m
  a.Y = w + bp.dpre; a.ldy = Mh; a.W = (const float*)p->W_m; a.ldw = J; a.Nc = Mh; a.Kout = J;
  a.act0 = sv + sp.ei; a.act1 = sv + sp.eq; a.out0 = w + bp.dpi; a.out1 = w + bp.dpq;
  a.w0 = DwJob{w + bp.dpre, Mh, nullptr, sv + sp.ei, sv + sp.eq, J, (float*)pg->W_m, (float*)pg->b_m, Mh, J};
  a.nx = mt * ((J + 31) / 32); a.ng0 = groups(Mh, J);
  CA_TRY(launch_bwd<1>(a, true, s));
  // 3. dh = dp_q W_q;  dW_i = (dp_i inv)^T f, db_i = sum dp_i;  dW_q = dp_q^T h, db_q
  a.Y = w + bp.dpq; a.ldy = J; a.W = (const float*)p->W_q; a.ldw = H; a.Nc = J; a.Kout = H;
  a.act0 = nullptr; a.act1 = nullptr; a.out0 = (float*)dh; a.out1 = nullptr;
  a.w0 = DwJob{w + bp.dpi, J, sv + sp.inv, (const float*)f, nullptr, (int)ld_f, (float*)pg->W_i, (float*)pg->b_i, J, Di};
  a.w1 = DwJob{w + bp.dpq, J, nullptr, (const float*)h, nullptr, (int)ld_h, (float*)pg->W_q, (float*)pg->b_q, J, H};
  a.nx = dh ? mt * ((H + 31) / 32) : 0; a.ng0 = groups(J, Di); a.ng1 = groups(J, H);
  CA_TRY(launch_bwd<2>(a, true, s));
  prof_mark(s, "fusion_backward");
  return 0;
}
