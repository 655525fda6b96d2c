// Fused backward of the parallel co-attention (hand-derived; SURVEY.md section 8, checked
// against autograd of the reference by the oracle).  fp32 results; bwd_dq_kernel (channel-major V) uses the exact-f32
// MFMA 16x16x4, the big kernels live in coattn_bwd32.hip on the bf16 MFMA.
//
// H_v [N,d] is never stored: both big kernels recompute it from P_v, P_q and C (saved).
//
//   bwd_pre_kernel  (per sample, all levels)  one pass over V: da_v = V gv partials (the image side's softmax backward
//                   ds_v is finished in the prologues of the two big kernels); da_q = Q gq -> ds_q, dc_q partials.
//                   (dZ_q = ds_q (x) w_q (.) (1 - H_q^2) is not stored: the two big kernels form it from the saved H_q
//                   where they used to read it -- the same bytes for them, one read of H_q and one write of dZ_q
//                   less for this kernel -- and bwd_nat32_kernel sums the dw_q partial.)
//   bwd_dc32_kernel (coattn_bwd32.hip; per sample x level, orientation [d][n], bf16 MFMA with the exact 3-way
//                   split): H_v^T tile = P_v^T + P_q^T C -> dZ_v^T, and dC += P_q dZ_v^T + dZ_q P_v^T with the
//                   dZ_v^T / P_v^T fragments as MFMA B operands (contraction over d); cross-wave sum through
//                   LDS, dA = dC (.) (1 - C^2).
//   bwd_nat32_kernel (coattn_bwd32.hip; per sample x level, orientation [n][d], the loop of forward phase 2, on
//                   the bf16 MFMA with the exact 3-way split): H_v tile -> dZ_v tile, which is the B operand of
//                   dP_q += C dZ_v (contraction over N) and then the accumulator of dP_v = dZ_v + C^T dZ_q
//                   (stored as it lies); dw_v, db_v, db_q partials.
//   then MFMA GEMMs: dQ = a_q (x) gq + dA V^T + dP_q W_q;  dV = sum_l (a_v (x) gv + Q^T dA) +
//   (sum_l dP_v) W_v (skipped when the image features need no gradient);  dW_v, dW_q, biases.
#include "fused.h"
#include <stdlib.h>

namespace {

// partial da_v over 64 channel rows: part[b][kc][l][n] = sum_{k in chunk kc} V[b][k][n] gv[l][b][k].
// grid (d/64, B); thread <-> location n (rows of V are contiguous in n: fully coalesced).
__device__ __forceinline__ void dav_cm_block(const float* V, long v_sB, const float* gv, float* part, int B, int N, int d,
                                             int L, int kc, int b, int nkc, float (*g)[64]) {
  const int n = threadIdx.x;
  if (threadIdx.x < 192) {
    const int l = threadIdx.x >> 6, k = threadIdx.x & 63;
    g[l][k] = (l < L) ? gv[((size_t)l * B + b) * d + kc * 64 + k] : 0.f;
  }
  __syncthreads();
  if (n >= N) return;
  const float* vp = V + (size_t)b * v_sB + (size_t)kc * 64 * N + n;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll 16
  for (int k = 0; k < 64; ++k) {
    const float x = vp[(size_t)k * N];
    a0 = fmaf(x, g[0][k], a0);
    a1 = fmaf(x, g[1][k], a1);
    a2 = fmaf(x, g[2][k], a2);
  }
  float* o = part + (((size_t)b * nkc + kc) * 3) * N + n;
  o[0] = a0; o[N] = a1; o[2 * (size_t)N] = a2;
}

// location-major V [N][d]: da_v[l][n] = V[n][:] . gv[l][:], whole rows -> part[b][0][l][n] (one "chunk").
// grid (ceil(N / 16), B); a wave takes 4 rows, lanes along the channels (float4), three wave sums per row.
__device__ __forceinline__ void dav_lm_block(const float* __restrict__ V, long v_sB, const float* __restrict__ gv, float* __restrict__ part,
                                             int B, int N, int d, int L, int bx, int b) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* Vb = V + (size_t)b * v_sB;
  const int n0 = bx * 16 + 4 * w;
  if (n0 >= N) return;
  // the wave's four rows are requested together (rows past N: row N - 1 again, its sums dropped), the level vectors are
  // read once per 256-channel sweep, the twelve wave sums run as independent chains
  float a[4][3] = {};
  const float* rowp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rowp[i] = Vb + (size_t)min(n0 + i, N - 1) * d;
  for (int k = 4 * lane; k < d; k += 256) {
    f32x4 x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const f32x4*>(rowp[i] + k);
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gv + ((size_t)0 * B + b) * d + k);
    const f32x4 g1 = L > 1 ? *reinterpret_cast<const f32x4*>(gv + ((size_t)1 * B + b) * d + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 g2 = L > 2 ? *reinterpret_cast<const f32x4*>(gv + ((size_t)2 * B + b) * d + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[i][0] = fmaf(x[i][e], g0[e], a[i][0]);
        a[i][1] = fmaf(x[i][e], g1[e], a[i][1]);
        a[i][2] = fmaf(x[i][e], g2[e], a[i][2]);
      }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l) a[i][l] = wave_sum(a[i][l]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (n0 + i >= N) break;
      float* o = part + (size_t)b * 3 * N + n0 + i;
      o[0] = a[i][0]; o[N] = a[i][1]; o[2 * (size_t)N] = a[i][2];
    }
  }
}

struct PreArgs {
  const float* dav_part;                 // [B][nkc][3][N] partial da_v (bwd_dav_kernel: nkc = d/64; _lm: nkc = 1)
  int nkc;
  const float* Q[8];
  const float* gq;                       // [L][B][d]
  const float* av; const float* aq;      // saved
  // the da_v blocks ride along in the same launch (blocks past L*B): dav_gx blocks per sample
  const float* V; long v_sB; const float* gv; float* dav_out; int dav_lm, dav_gx;
  float* dsq;                            // [L*B][32] ds_q, zeros for t >= T
  float* dcs_part;                       // [2][L*B]
  const int* qlen;                       // [B] question lengths of the forward, or NULL: da_q rows t >= len_b count as 0, and
  float* dA;                             //   the rows t >= len_b of dA [L][B][T][N] are zeroed here (bwd_dc32_kernel skips them)
  int B, N, T, d, L;
  TnDyn dyn; TnDynPlan* plan_out;        // plan_out != NULL: ONE more workgroup (the launch's last) evaluates the split-K plan of the
                                         // weight gradients over the live question rows (fused.h tn_dyn_plan) and leaves it there,
  const unsigned* saved_bits;            //   over the forward's bitmap in `saved` when the forward's tag (row_tag, fused.h kRowTag)
  const unsigned* row_tag;               //   says it wrote one, else over all rows; the words it counted go to dyn.bits
  const float* gaq;                      // (bwd_pre_maps_kernel, coattn_backward_maps) [L][B][T] upstream gradient of a_q: da_q += G_aq
                                         // for t < len_b, read as 0 beyond (whatever the pad slots hold)
};

// Blocks [0, L*B): one workgroup (256 threads) per (sample, level), question side -- softmax backward of a_q
// (da_q = Q gq -> ds_q, dc_q partial).  Blocks past L*B: the da_v partials (one pass over V for all levels, independent
// of the question side: they fill the idle half of the chip).
// (Round 4, measured and not kept while this kernel also swept H_q into dZ_q: requesting a wave's rows together -- all 7 Q
//  rows of the da_q dot products, all 14 / 2 x 7 H_q rows of the sweep, the 4 V rows of a da_v wave -- costs registers the
//  da_v blocks of the same launch pay for with occupancy: 60 -> 102 / 128 VGPRs, 27.7 -> 32.6 / 37.3 us at N = 196,
//  22.7 -> 22.3 / 21.6 at N = 49.)
// GMAP: the map-gradient form (bwd_pre_maps_kernel); the body is shared so that bwd_pre_kernel's code object stays as it was.
template <bool GMAP>
__device__ __forceinline__ void bwd_pre_body(const PreArgs& a, float* lds) {
  if (a.plan_out && (int)blockIdx.x == a.L * a.B + a.dav_gx * a.B) {
    if (threadIdx.x < 64) {                          // one full wave
      const bool tagged = a.row_tag[0] == kRowTag && a.row_tag[1] == (unsigned)(a.B * a.T) && a.row_tag[2] == (unsigned)a.L;
      const TnDynPlan pl = tn_dyn_plan(a.dyn, tagged ? a.saved_bits : nullptr, a.B * a.T);
      if (threadIdx.x == 0) *a.plan_out = pl;
    }
    return;
  }
  const int d = a.d, T = a.T, B = a.B;
  if ((int)blockIdx.x >= a.L * B) {
    const int id = (int)blockIdx.x - a.L * B;
    if (a.dav_lm) dav_lm_block(a.V, a.v_sB, a.gv, a.dav_out, B, a.N, d, a.L, id % a.dav_gx, id / a.dav_gx);
    else dav_cm_block(a.V, a.v_sB, a.gv, a.dav_out, B, a.N, d, a.L, id % a.dav_gx, id / a.dav_gx, a.dav_gx,
                      reinterpret_cast<float(*)[64]>(lds));
    return;
  }
  float* daq = lds;                       // 32
  const int pairi = blockIdx.x, l = pairi / B, b = pairi - l * B;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t pair = (size_t)pairi;
  // ---- question side: da_q[t] = Q[t] . gq, one wave per row
  const float* Qp = a.Q[l] + (size_t)b * T * d;
  const float* gqp = a.gq + pair * d;
  for (int t0 = w; t0 < T; t0 += 16) {               // four of the wave's rows (t0, t0 + 4, ...) at a time, requested together
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 4 * lane; k < d; k += 256) {
      f32x4 x[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const f32x4*>(Qp + (size_t)min(t0 + 4 * i, T - 1) * d + k);
      const f32x4 g = *reinterpret_cast<const f32x4*>(gqp + k);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] += x[i][0] * g[0] + x[i][1] * g[1] + x[i][2] * g[2] + x[i][3] * g[3];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = wave_sum(acc[i]);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (t0 + 4 * i < T) daq[t0 + 4 * i] = acc[i];
    }
  }
  __syncthreads();
  if (w == 0) {
    // (a masked token has a_q = 0, so ds_q = 0 there; its da_q -- of whatever the pad row holds -- is read as 0 as well, so
    //  that not even the sign of that zero depends on the padding)
    const int tl = a.qlen ? min(max(a.qlen[b], 1), T) : T;
    const float aqv = (lane < T) ? a.aq[pair * T + lane] : 0.f;
    float x = (lane < tl) ? daq[lane] : 0.f;
    if constexpr (GMAP) {                            // da_q += G_aq on the live tokens; a pad slot's value is selected away
      const float g = a.gaq[pair * T + min(lane, T - 1)];
      x = (lane < tl) ? x + g : 0.f;
    }
    if (tl < T) {                                    // (length mask only) dA rows past the question
      float* da = a.dA + pair * (size_t)T * a.N;
      for (int i = tl * a.N + lane; i < T * a.N; i += 64) da[i] = 0.f;
    }
    const float dq = wave_sum(aqv * x);
    const float sq = aqv * (x - dq);
    if (lane < 32) a.dsq[pair * 32 + lane] = sq;                     // (lanes >= T: zeros)
    const float tot_q = wave_sum(sq);
    if (lane == 0) a.dcs_part[(size_t)a.L * B + pair] = tot_q;       // [2][L*B]
  }
}
__global__ __launch_bounds__(256) void bwd_pre_kernel(const PreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  bwd_pre_body<false>(a, lds);
}
__global__ __launch_bounds__(256) void bwd_pre_maps_kernel(const PreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  bwd_pre_body<true>(a, lds);
}


// dQ_l[b][t][k] = a_q,l[t] gq_l[k] + sum_n dA_l[t][n] V[b][k][n]   for all levels with one pass over V.
// grid (d/128, B); a wave owns 32 channels (two 16-wide MFMA column tiles); dA of the three levels is
// staged zero-padded in LDS and read as MFMA A operands (16 bytes = 4 k-steps per ds_read_b128).

// LM: V location-major [N][d] (dword loads, 64 contiguous bytes per 16 lanes); else channel-major [d][N].
template <int NT, bool ALIGNED, bool LM = false>
__global__ __launch_bounds__(256, 2) void bwd_dq_kernel(const DqArgs a) {
  constexpr int NPAD = 16 * NT;
  constexpr int LD = NPAD + 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* dAs = lds;                                  // 3 x kTRows x LD
  float* aqs = lds + 3 * kTRows * LD;                // 3 x 32
  const int b = blockIdx.y, N = a.N, T = a.T, d = a.d, L = a.L, B = a.B;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, q4 = lane >> 4;
  // stage dA of the three levels, zero padded: one wave per row, lanes along n
  for (int rr = w; rr < 3 * kTRows; rr += 4) {
    const int l = rr / kTRows, row = rr - l * kTRows;
    const bool live = l < L && row < T;
    const float* src = a.dA + (((size_t)l * B + b) * T + row) * N;
    float* dst = dAs + (l * kTRows + row) * LD;
    if (ALIGNED) {
      for (int c4 = lane; c4 < NPAD / 4; c4 += 64) {
        const int col = 4 * c4;
        *reinterpret_cast<f32x4*>(dst + col) =
            (live && col < N) ? *reinterpret_cast<const f32x4*>(src + col) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else {
      for (int col = lane; col < NPAD; col += 64) dst[col] = (live && col < N) ? src[col] : 0.f;
    }
  }
  if (tid < 96) {
    const int l = tid >> 5, t = tid & 31;
    aqs[tid] = (l < L && t < T) ? a.aq[((size_t)l * B + b) * T + t] : 0.f;
  }
  __syncthreads();
  const int kb = blockIdx.x * 128 + 32 * w;
  const float* Vb = a.V + (size_t)b * a.v_sB;
  const __amdgpu_buffer_rsrc_t rs_v = make_rsrc(Vb, (unsigned)d * N * 4u);
  f32x4 acc[3][2][2];
#pragma unroll
  for (int l = 0; l < 3; ++l)
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int c = 0; c < 2; ++c) acc[l][tt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  // B operand: lane (channel kb + 16c + j, quad q4) holds V[k][16g + 4*q4 + s], s = 0..3
  auto load_v = [&](int g, f32x4(&dst)[2]) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if constexpr (LM) {                            // rows n >= N lie beyond the buffer: read 0
#pragma unroll
        for (int s = 0; s < 4; ++s) dst[c][s] = buf_load1(rs_v, ((4 * q4 + s) * d + 16 * c + j) * 4, (16 * g * d + kb) * 4);
        continue;
      }
      const int voff = ((16 * c + j) * N + 4 * q4) * 4;
      if (ALIGNED) {
        dst[c] = buf_load4(rs_v, voff, (kb * N + 16 * g) * 4);
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) dst[c][s] = buf_load1(rs_v, voff + 4 * s, (kb * N + 16 * g) * 4);
      }
    }
  };
  f32x4 vb[2][2];
  load_v(0, vb[0]);
#pragma unroll
  for (int g = 0; g < NT; ++g) {
    if (g + 1 < NT) load_v(g + 1, vb[(g + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = min(16 * tt + j, kTRows - 1);
        const f32x4 a4 = *reinterpret_cast<const f32x4*>(&dAs[(l * kTRows + t) * LD + 16 * g + 4 * q4]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[l][tt][c] = mfma16(a4[s], vb[g & 1][c][s], acc[l][tt][c]);
      }
  }
  // epilogue: + a_q (x) gq ; rows t >= T fall outside the per-sample dQ buffer (stores dropped)
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    if (l < L) {
      const __amdgpu_buffer_rsrc_t rs_dq = make_rsrc(a.dQ[l] + (size_t)b * T * d, (unsigned)T * d * 4u);
      const float* gqp = a.gq + ((size_t)l * B + b) * d;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float g = gqp[kb + 16 * c + j];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int t = 16 * tt + 4 * q4 + r;
            const float v = fmaf(aqs[l * 32 + t], g, acc[l][tt][c][r]);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs_dq, (t * d + j) * 4 + 64 * c,
                                                  kb * 4, 0);
          }
      }
    }
  }
}

template <typename K>
hipError_t set_lds(K kern, size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

int launch_pre(const PreArgs& a, hipStream_t s) {
  const size_t lds = 768;                                           // the 3 x 64 g values of a channel-major da_v block; 32 da_q
  const dim3 grid(a.L * a.B + a.dav_gx * a.B + (a.plan_out ? 1 : 0));
  if (a.gaq) hipLaunchKernelGGL(bwd_pre_maps_kernel, grid, dim3(256), lds, s, a);
  else hipLaunchKernelGGL(bwd_pre_kernel, grid, dim3(256), lds, s, a);
  CA_CHECK_LAUNCH("bwd_pre");
  // (the image side's softmax backward -- ds_v from these partials -- happens in the prologues of bwd_dc32_kernel and
  //  bwd_nat32_kernel: fused.h softmax_bwd_v)
  return 0;
}

// ---- the host driver: fused_backward decides the route of a call once (decide_route), then runs its steps ---------------------

// where things lie in `saved` and in the workspace, and the sizes the steps share
struct Off { SavedOff so; FusedBwdOff wo; size_t BTd, BTN, BNd, Bd; };

// Every decision of a call, taken before its first launch, and the GEMM jobs the decisions are about.
struct Route {
  bool lm;                 // location-major image features (else channel-major)
  int np;                  // width of the fp32 mode's contractions (fused.h): 2 = hi + mid in the three fused kernels and in the GEMM
                           // launch (dW_v, dW_q, dQ = dP_q W_q), 3 = the exact split everywhere; dV (general GEMM) is always exact
  int tn_budget;           // split-K parts dW_v and dW_q share
  int ko_dpv, ko_sum3;     // developer knock-outs (wrong results)
  TnDyn dyn_all;           // bits != NULL: the pre-pass plans the weight gradients over the live question rows (fused.h TnDyn)
  TnGemm tnv, tnq;         // dW_v = (sum_l dP_v)^T V, dW_q = sum_l dP_q,l^T Q_l on the hand-scheduled A^T B kernels
  WGemm wdq;               // dQ_l = dP_q,l W_q against the W_q image the forward left in `saved` (fused.h dq_proj_job)
  bool tn_v, tn_q, wdq_ok; // which of the three those kernels take
  bool dq32;               // dA V on the bf16-MFMA kernel (both layouts; channel-major: aligned rows), else the exact-f32 one
  bool own_dq, combine;    // the dQ projection behind the weight gradients (COATTN_OWN_DQ) / its tiles inside their launch;
  bool late_dq;            // either way the dA V kernel then runs after the weight gradients
  bool dp_bf16;            // bwd_nat32 stores dP_v / dP_q as bf16
  bool sum_in_gemm;        // the weight-gradient kernel adds the three levels of dP_v while staging them (no dV: the frozen encoder)
  bool bf_tn, wide;        // both weight gradients on gemm_bf.hip's single-product kernel / on gemm_tn_wide.hip's 128 x 256 tiles
  bool red_in_dq;          // their partial sums ride in the dQ kernel's launch (RedJob),
  bool use_dyn;            // which then follows the device's plan (dyn_all)
};
struct RedJob { const float* part[2]; float* out[2]; int np[2]; long n; int acc; TnDyn dyn; };

void decide_route(const Ctx& c, const Off& o, Route& r) {
  const int B = c.B, N = c.N, T = c.T, d = c.d, L = c.L;
  // developer switches (builds with -DCOATTN_DEV_SWITCHES only; tools/ab_*.sh)
  static const int tn_budget_env = dev_env_int("COATTN_TN_PARTS", 0);
  static const int ko_dpv = dev_env_int("COATTN_KO_DPV", 0);      // knock-outs (wrong results): what would ONE sum_l dP_v array
  static const int ko_sum3 = dev_env_int("COATTN_KO_SUM3", 0);    // save in bwd_nat32's stores / the GEMM's reads
  static const int no_combine = dev_env_int("COATTN_NO_COMBINE", 0);
  // COATTN_OWN_DQ=1 (round 5, measured and NOT kept): the dQ projection as a launch of its own on the persistent pipeline of
  // gemm_h2.hip (bf16 pieces) between the weight gradients and the dA V kernel -- 98.9 + 28.5 us against 123.2 combined at
  // N = 196, 41.8 + 26.6 against 63.7 at N = 49: inside the weight-gradient launch its tiles fill the CUs the last parts leave,
  // which is worth as much as the faster kernel.
  static const int own_dq_env = dev_env_int("COATTN_OWN_DQ", 0);
  static const int dp_bf16_off = (dev_env_int("COATTN_DP_BF16", 1) == 0);
  static const int red_in_dq = dev_env_int("COATTN_RED_IN_DQ", 1);
  static const int live_env = dev_env_int("COATTN_DW_LIVE_ROWS", 1);   // 0: the host's static plan over all rows
  r = Route{};
  r.lm = v_is_lm(c.vl, N, d);
  r.np = (c.np_bwd == 2 && !c.bf16_proj) ? 2 : 3;
  r.tn_budget = tn_budget_env > 0 ? tn_budget_env : 32;
  r.ko_dpv = ko_dpv; r.ko_sum3 = ko_sum3;
  const int budget = r.tn_budget;
  float* part = c.ws + o.wo.part;
  // (exact mode: the forward's bitmap of the live question rows may be in `saved` -- live_rows: the shape and mode allow one,
  //  its tag says whether the forward wrote it; the plan of the weight gradients over those rows is a function of it and of
  //  shapes known here -- evaluated once, by an extra workgroup of the pre-pass, which copies the words it counted to `ws`)
  if (c.live_rows && L <= kDynLevels && (B * T + 31) / 32 <= kRowBitsMaxWords && budget > L) {
    r.dyn_all.bits = reinterpret_cast<const unsigned*>(c.ws + o.wo.rowbits);
    r.dyn_all.words = (B * T + 31) / 32; r.dyn_all.levels = L; r.dyn_all.P = budget; r.dyn_all.K0 = B * N;
    r.dyn_all.plan = reinterpret_cast<const TnDynPlan*>(c.ws + o.wo.dynplan);
  }
  // which of the backward's GEMMs take the hand-scheduled kernels (when all three do, they share ONE launch)
  TnGemm& tnv = r.tnv;
  tnv.A = c.ws + o.wo.dPv; tnv.a_ld = d; tnv.B = c.V; tnv.b_ld = (int)c.vl.sN; tnv.C = part; tnv.M = d; tnv.N = d; tnv.K = B * N;
  tnv.levels = 1; tnv.bf16 = c.bf16_proj; tnv.np = r.np;
  if (c.wgemm && r.lm && c.vl.sB == (long)N * c.vl.sN && c.vl.sN < (1L << 24)) {
    r.tn_v = gemm_tn_supported(tnv) != 0;            // location-major rows, samples abutting
  } else if (c.wgemm && !r.lm && c.vl.sD < (1L << 24)) {
    tnv.b_ld = (int)c.vl.sD; tnv.b_kdiv = N; tnv.b_sdiv = c.vl.sB;       // channel-major, read in place
    r.tn_v = gemm_tn_supported(tnv) != 0;
  }
  TnGemm& tnq = r.tnq;
  tnq.A = c.ws + o.wo.dPq; tnq.a_sl = (long)o.BTd; tnq.a_ld = d; tnq.b_ld = d; tnq.M = d; tnq.N = d; tnq.K = B * T; tnq.levels = L;
  for (int l = 0; l < L; ++l) tnq.b_ptrs[l] = c.Q[l];
  tnq.bf16 = c.bf16_proj; tnq.np = r.np;
  r.tn_q = c.wgemm && gemm_tn_supported(tnq);        // levels as extra split-K parts (gemm_tn.hip)
  r.dq32 = r.lm || (N % 4) == 0;
  // the dQ projection's image is written by the forward whenever this job is supported (the same test, api.hip
  // general_projections: fused.h dq_proj_job)
  WGemm& wdq = r.wdq;
  wdq = dq_proj_job(B, T, d, L, c.bf16_proj, r.np);
  r.wdq_ok = c.wgemm && gemm_w_supported(wdq);
  wdq.A = c.ws + o.wo.dPq; wdq.Wf = c.saved + o.so.wqT;
  for (int l = 0; l < L; ++l) wdq.c_ptrs[l] = c.dQ[l];
  // (a dQ projection on gemm_bf.hip -- 512-thread workgroups -- cannot ride in the weight-gradient launch; bilinear: dQ comes
  //  from its own projection [dP_q | dK] [W_q; W_b], so the dQ tiles do not ride there either -- which keeps the static plan)
  const bool all3 = r.dq32 && r.wdq_ok && r.tn_v && r.tn_q;
  r.own_dq = own_dq_env && !c.bil && all3 && !gemm_bf_supported(wdq) && gemm_h2_supported(wdq) && !no_combine;
  r.combine = all3 && !gemm_bf_supported(wdq) && !no_combine && !r.own_dq && !c.bil;
  r.late_dq = r.combine || r.own_dq;
  // Reduced-precision mode with a frozen image encoder (no dV) and all three consumers of dP_v / dP_q on gemm_bf.hip:
  // bwd_nat32 stores both as bf16 -- the GEMMs would round them on their way in anyway -- halving what it writes and
  // what they fetch.
  {
    TnGemm tv = tnv, tq = tnq;
    WGemm wq = wdq;
    tv.a_bf16 = tq.a_bf16 = wq.a_bf16 = 1;
    tv.a_term = L == 3 ? (long)o.BNd : 0;
    r.dp_bf16 = !dp_bf16_off && c.bf16_proj && !c.dV && L == 3 && d % 512 == 0 && all3 && gemm_bf_tn_supported(tv) &&
                gemm_bf_tn_supported(tq) && gemm_bf_supported(wq);
    if (r.dp_bf16) tnv.a_bf16 = tnq.a_bf16 = wdq.a_bf16 = 1;   // (a_sl, a_sz stay in elements)
  }
  r.sum_in_gemm = r.tn_v && L == 3 && !c.dV;
  if (r.sum_in_gemm) tnv.a_term = ko_sum3 ? 0 : (long)o.BNd;
  r.bf_tn = r.tn_v && r.tn_q && gemm_bf_tn_supported(tnv) && gemm_bf_tn_supported(tnq);
  // (gemm_bf.hip's weight-gradient launch carries no dQ tiles: below the 256 rows its own projection kernel wants -- B T = 128 ..
  //  224 with B N and B T multiples of 32 -- the projection is a launch of its own in front of the dA V kernel, which adds onto it)
  if (r.bf_tn) r.combine = r.own_dq = r.late_dq = false;
  if (!r.tn_v || !r.tn_q || r.bf_tn) return;
  // two-piece width: 128 x 256 tiles on 512-thread workgroups (gemm_tn_wide.hip) -- the same split-K partition, pieces and
  // order of products, so the same bits as the 128 x 128 kernel
  r.wide = gemm_tn_wide_supported(tnv) && gemm_tn_wide_supported(tnq) &&
           (!r.combine || (wdq.N % 256 == 0 && !wdq.f16 && (wdq.np == 2) == (tnv.np == 2)));
  const bool red_al = (((int64_t)d * d) & 3) == 0 &&
                      ((((uintptr_t)part) | ((uintptr_t)c.pg->dW_v) | ((uintptr_t)c.pg->dW_q)) & 15) == 0;
  r.red_in_dq = r.late_dq && r.dq32 && red_in_dq && red_al;
  // The forward left the bitmap of the question rows that are not all zeros in `saved` (exact mode; api.hip rowbits_in_saved):
  // dW_q = sum dP_q^T Q then contracts over those rows only, and the launch shares its `budget` parts between dW_v and the
  // levels of dW_q ON THE DEVICE (fused.h TnDyn) -- the partial sums are added by the dQ kernel's extra workgroups, which
  // evaluate the same plan.
  r.use_dyn = live_env && r.dyn_all.bits && r.wide && r.red_in_dq && tnq.K <= 8192 && !tnq.a_bf16 &&
              (tnq.K + 31) / 32 <= kRowBitsMaxWords && budget > L && budget <= kMaxParts && L <= kDynLevels;
}

// 1. per-sample pre-pass: one launch for the question side and the da_v partials (and the live-row plan)
int run_pre(const Ctx& c, const Route& r, const Off& o) {
  const int N = c.N, d = c.d, L = c.L;
  PreArgs pa;
  pa.V = c.V; pa.v_sB = c.vl.sB; pa.gv = c.gv; pa.dav_out = c.ws + o.wo.part; pa.dav_lm = r.lm ? 1 : 0;
  pa.dav_gx = r.lm ? (N + 15) / 16 : d / 64;
  pa.dav_part = c.ws + o.wo.part;
  pa.nkc = r.lm ? 1 : d / 64;
  for (int l = 0; l < 8; ++l) pa.Q[l] = l < L ? c.Q[l] : nullptr;
  pa.gq = c.gq; pa.av = c.saved + o.so.av; pa.aq = c.saved + o.so.aq;
  pa.dsq = c.ws + o.wo.dsq; pa.dcs_part = c.ws + o.wo.dcs_part; pa.qlen = c.qlen; pa.dA = c.ws + o.wo.dA;
  pa.gaq = c.g_aq;                                   // (coattn_backward_maps; NULL: the plain pre-pass)
  pa.B = c.B; pa.N = N; pa.T = c.T; pa.d = d; pa.L = L;
  pa.dyn = r.dyn_all; pa.plan_out = nullptr; pa.saved_bits = nullptr; pa.row_tag = nullptr;
  if (r.dyn_all.bits) {
    pa.saved_bits = reinterpret_cast<const unsigned*>(c.saved + o.so.rowbits);
    pa.row_tag = reinterpret_cast<const unsigned*>(c.saved + o.so.rowcnt) + kRowTagWord;
    pa.plan_out = reinterpret_cast<TnDynPlan*>(c.ws + o.wo.dynplan);
  }
  CA_TRY(launch_pre(pa, c.s));
  prof_mark(c.s, "bwd_pre");
  return 0;
}

// 2. the two recompute kernels' arguments (coattn_bwd32.hip)
BwdArgs recompute_args(const Ctx& c, const Route& r, const Off& o) {
  const float* saved = c.saved;
  float* ws = c.ws;
  BwdArgs ba;
  ba.Pv = saved + o.so.Pv; ba.Pq = saved + o.so.Pq; ba.C = saved + o.so.C;
  ba.Hq = saved + o.so.Hq; ba.dsq = ws + o.wo.dsq; ba.wq = (const float*)c.p->w_q; ba.dwq_part = ws + o.wo.dwq_part;
  ba.dav_part = ws + o.wo.part; ba.nkc = r.lm ? 1 : c.d / 64; ba.av = saved + o.so.av; ba.dcs_part = ws + o.wo.dcs_part;
  ba.wv = (const float*)c.p->w_v;
  ba.dPv = ws + o.wo.dPv; ba.dPq = ws + o.wo.dPq; ba.dA = ws + o.wo.dA; ba.dwv_part = ws + o.wo.dwv_part;
  ba.dbv_part = ws + o.wo.dbv_part; ba.dbq_part = ws + o.wo.dbq_part;
  ba.B = c.B; ba.N = c.N; ba.T = c.T; ba.d = c.d; ba.L = c.L;
  ba.bf16 = c.bf16_proj;
  ba.np = r.np;
  ba.ko_dpv = r.ko_dpv;
  ba.dp_bf16 = 0;                                    // (bwd_dc32 stores neither; bwd_nat32: Route::dp_bf16)
  ba.qlen = c.qlen;
  ba.gav = c.g_av;                                   // (coattn_backward_maps; NULL: the kernels without the G_av operand)
  return ba;
}

// 3. small parameter gradients from the per-(sample, level) partials (dw_v, db_v, db_q, dw_q; dc_v, dc_q as whole-array sums):
//    a few short workgroups in the hand-scheduled weight-gradient launch, else a launch of their own (run_small_reductions)
TnReduce small_reductions(const Ctx& c, const Off& o) {
  TnReduce small = {};
  const float* src[4] = {c.ws + o.wo.dwv_part, c.ws + o.wo.dbv_part, c.ws + o.wo.dbq_part, c.ws + o.wo.dwq_part};
  float* dst[4] = {(float*)c.pg->dw_v, (float*)c.pg->db_v, (float*)c.pg->db_q, (float*)c.pg->dw_q};
  for (int i = 0; i < 4; ++i) { small.src[i] = src[i]; small.dst[i] = dst[i]; }
  small.njobs = 4; small.nparts = c.L * c.B; small.n = c.d; small.accumulate = c.accumulate;
  small.sum_x[0] = c.ws + o.wo.dcs_part; small.sum_x[1] = c.ws + o.wo.dcs_part + (size_t)c.L * c.B;
  small.sum_out[0] = (float*)c.pg->dc_v; small.sum_out[1] = (float*)c.pg->dc_q; small.sum_n = (long)c.L * c.B;
  return small;
}
int run_small_reductions(const Ctx& c, const Off& o) {
  const TnReduce small = small_reductions(c, o);
  return launch_reduce_jobs(small.src, small.dst, 4, c.L * c.B, c.d, c.accumulate, c.s, small.sum_x, small.sum_out, small.sum_n);
}

// dQ_l (+)= dP_q,l W_q for all levels in one launch (batch z = level, C through the pointer table)
int run_dq_projection(const Ctx& c, const Route& r, const Off& o, bool onto_dq) {
  // (W_q split once by the forward's launch -- the same shape test decided there, api.hip general_projections --
  //  and read as MFMA fragments, gemm_w.hip)
  if (!onto_dq && r.wdq_ok) return launch_gemm_wx(&r.wdq, 1, c.s);
  const int d = c.d;
  coattn_gemm_desc g = {};
  g.A = c.ws + o.wo.dPq; g.a_sz = (int64_t)o.BTd; g.a_sm = d; g.a_sk = 1;
  g.B = c.p->W_q; g.b_sk = d; g.b_sn = 1;
  for (int l = 0; l < c.L; ++l) { g.c_ptrs[l] = c.dQ[l]; if (onto_dq) g.cin_ptrs[l] = c.dQ[l]; }
  if (onto_dq) { g.cin_sm = d; g.cin_sn = 1; g.beta = 1.f; }
  g.c_sm = d; g.c_sn = 1;
  g.M = c.B * c.T; g.N = d; g.K = d; g.batch = c.L;
  return launch_gemm_mode(g, c.bf16_proj, c.s);
}

template <int NT>
void launch_dq_f32(bool lm, bool al, dim3 grid, size_t lds, hipStream_t s, const DqArgs& da) {
  if (lm && al) hipLaunchKernelGGL((bwd_dq_kernel<NT, true, true>), grid, dim3(256), lds, s, da);
  else if (lm) hipLaunchKernelGGL((bwd_dq_kernel<NT, false, true>), grid, dim3(256), lds, s, da);
  else if (al) hipLaunchKernelGGL((bwd_dq_kernel<NT, true>), grid, dim3(256), lds, s, da);
  else hipLaunchKernelGGL((bwd_dq_kernel<NT, false>), grid, dim3(256), lds, s, da);
}

// dst_l (+)= a_q,l (x) gq_l + dA_l V^T: the bf16-MFMA kernel (coattn_bwd32.hip; red != NULL: with the weight gradients' partial
// sums in its launch) or the exact-f32 bwd_dq_kernel above
int run_dq(const Ctx& c, const Route& r, const Off& o, float* const* dst, const float* gq, int accumulate, const RedJob* red) {
  const int B = c.B, N = c.N, d = c.d, L = c.L;
  DqArgs da = {};
  da.accumulate = accumulate;
  if (red && r.dq32) {
    for (int i = 0; i < 2; ++i) { da.red_part[i] = red->part[i]; da.red_out[i] = red->out[i]; da.red_np[i] = red->np[i]; }
    da.red_n = red->n; da.red_acc = red->acc; da.red_jobs = 2; da.red_blocks = (int)((red->n / 4 + 255) / 256);
    da.red_dyn = red->dyn;
  }
  da.V = c.V; da.v_sB = c.vl.sB; da.dA = c.ws + o.wo.dA; da.aq = c.saved + o.so.aq; da.gq = gq;
  for (int l = 0; l < 8; ++l) da.dQ[l] = l < L ? dst[l] : nullptr;
  da.B = B; da.N = N; da.T = c.T; da.d = d; da.L = L;
  da.bf16 = c.bf16_proj; da.np = r.np;
  const bool al = (N % 4) == 0, lm = r.lm;
  const dim3 grid(d / 128, B);
  if (r.dq32) {
    CA_TRY(launch_bwd_dq32(da, lm ? 1 : 0, c.s));
  } else if (N <= 64) {
    launch_dq_f32<4>(lm, al, grid, (size_t)(3 * kTRows * (64 + 4) + 96) * sizeof(float), c.s, da);
  } else {
    const size_t lds = (size_t)(3 * kTRows * (208 + 4) + 96) * sizeof(float);
    static DeviceOnce once;
    CA_TRY(once.run([&] {
      hipError_t e = set_lds(bwd_dq_kernel<13, true>, lds);
      if (e == hipSuccess) e = set_lds(bwd_dq_kernel<13, false>, lds);
      if (e == hipSuccess) e = set_lds(bwd_dq_kernel<13, true, true>, lds);
      if (e == hipSuccess) e = set_lds(bwd_dq_kernel<13, false, true>, lds);
      return e;
    }, "bwd_dq"));
    launch_dq_f32<13>(lm, al, grid, lds, c.s, da);
  }
  CA_CHECK_LAUNCH("bwd_dq");
  prof_mark(c.s, "bwd_dq");
  return 0;
}
// the call's own dQ: added onto the projection by the bf16 kernel, written first by the exact-f32 one
int run_own_dq(const Ctx& c, const Route& r, const Off& o, const RedJob* red = nullptr) {
  return run_dq(c, r, o, c.dQ, c.gq, r.dq32 ? 1 : 0, red);
}

// one weight gradient on the hand-scheduled A^T B kernel (gemm_tn.hip): <= 32 split-K parts in g.C, then their sum
int run_dw_tn(const Ctx& c, const TnGemm& g, float* dW) {
  int ks, S;
  const int parts = gemm_tn_plan(g, 32, &ks, &S);
  CA_TRY(launch_gemm_tn(&g, &ks, &S, 1, c.s));
  return launch_reduce_partials(g.C, dW, parts, (int64_t)c.d * c.d, c.accumulate, c.s);
}

// The bilinear affinity: dK = dA V (the dA V pass, into dK), then ONE projection dQ = [dP_q | dK] [W_q; W_b] (K = 2d) on the
// pre-split-weight kernel, + a_q (x) gq; dW_b = sum_l dK_l^T Q_l on the weight-gradient kernel, db_b = column sums of dK.
int run_bilinear_dq_dwb(const Ctx& c, const Route& r, const Off& o) {
  const int B = c.B, T = c.T, d = c.d, L = c.L;
  const BilBwd* bil = c.bil;
  float* part = c.ws + o.wo.part;
  float* dk_ptrs[8] = {};
  for (int l = 0; l < L; ++l) dk_ptrs[l] = bil->dK + l * o.BTd;
  if (hipMemsetAsync(bil->zeros, 0, (size_t)L * o.Bd * sizeof(float), c.s) != hipSuccess) {
    coattn_set_error("fused backward: hipMemsetAsync failed");
    return -3;
  }
  CA_TRY(run_dq(c, r, o, dk_ptrs, bil->zeros, 0, nullptr));          // dK = dA V + a_q (x) 0, overwritten
  CA_TRY(launch_concat_cols(c.ws + o.wo.dPq, d, bil->dK, d, bil->dpk, (int64_t)L * B * T, c.s));
  CA_TRY(launch_concat_cols((const float*)c.p->W_q, d * d, bil->Wb, d * d, bil->wstack, 1, c.s));
  WGemm wj = dq_proj_job(B, T, d, L, 0, r.np);
  wj.K = 2 * d; wj.a_sm = 2 * d; wj.a_sz = 2 * (long)o.BTd; wj.A = bil->dpk; wj.Wf = bil->wimg;
  for (int l = 0; l < L; ++l) wj.c_ptrs[l] = c.dQ[l];
  if (c.wgemm && gemm_w_supported(wj)) {
    const WSplit job{bil->wstack, bil->wimg, d, 2 * d, 1, d, wimg_pieces(wj), nullptr};
    CA_TRY(launch_wsplit(&job, 1, c.s));
    CA_TRY(launch_gemm_wx(&wj, 1, c.s));
  } else {
    coattn_gemm_desc g = {};
    g.A = bil->dpk; g.a_sz = 2 * (int64_t)o.BTd; g.a_sm = 2 * d; g.a_sk = 1;
    g.B = bil->wstack; g.b_sk = d; g.b_sn = 1;
    for (int l = 0; l < L; ++l) g.c_ptrs[l] = c.dQ[l];
    g.c_sm = d; g.c_sn = 1;
    g.M = B * T; g.N = d; g.K = 2 * d; g.batch = L;
    CA_TRY(launch_gemm_f32(g, c.s));
  }
  for (int l = 0; l < L; ++l)
    CA_TRY(launch_rank1(c.saved + o.so.aq + (size_t)l * B * T, c.gq + l * o.Bd, c.dQ[l], B, T, d, (int64_t)T * d, d, 1, 1, c.s));
  prof_mark(c.s, "bwd_bilinear_dq");
  if (r.tn_q) {
    TnGemm tnb = r.tnq;
    tnb.A = bil->dK; tnb.a_bf16 = 0; tnb.C = part;
    CA_TRY(run_dw_tn(c, tnb, bil->dWb));
    CA_TRY(grad_colsum(nullptr, bil->dK, L * B * T, d, part, bil->dbb, c.accumulate, c.s));
  } else {
    CA_TRY(grad_bilinear_wb(bil->dK, c.Q, B, T, d, L, part, bil->dWb, bil->dbb, c.accumulate, c.s));
  }
  prof_mark(c.s, "bwd_bilinear_dwb");
  return 0;
}

// dV = sum_l (a_v,l (x) gv_l + Q_l^T dA_l)   (bilinear: K_l^T dA_l);  (sum_l dP_v) W_v is added by run_sum_dpv
int run_dv(const Ctx& c, const Off& o) {
  for (int l = 0; l < c.L; ++l) {
    const float* av = c.saved + o.so.av + (size_t)l * c.B * c.N;
    CA_TRY(launch_rank1(av, c.gv + l * o.Bd, c.dV, c.B, c.N, c.d, c.dvl.sB, c.dvl.sN, c.dvl.sD, l > 0 ? 1 : 0, c.s));
    CA_TRY(grad_dv_kt_da(c.bil ? c.bil->K + l * o.BTd : c.Q[l], c.ws + o.wo.dA + l * o.BTN, c.dV, c.dvl, c.B, c.N, c.T, c.d, c.s));
  }
  return 0;
}

// sum dP_v over the levels in place into level 0 (one streaming pass for L = 3; folding the sum into the weight-gradient
// GEMM's operand loads was measured slower: 302 vs 170 + 50 us) -- unless the weight-gradient kernel adds them itself
// (Route::sum_in_gemm) -- then dV += (sum_l dP_v) W_v
int run_sum_dpv(const Ctx& c, const Route& r, const Off& o) {
  float* dPv = c.ws + o.wo.dPv;
  const int64_t BNd = (int64_t)o.BNd;
  if (!r.sum_in_gemm && c.L == 3) CA_TRY(launch_add3_inplace(dPv, dPv + BNd, dPv + 2 * BNd, BNd, c.s));
  if (!r.sum_in_gemm && c.L != 3)
    for (int l = 1; l < c.L; ++l) CA_TRY(launch_add_inplace(dPv, dPv + l * BNd, BNd, 1, c.s));
  if (c.dV) CA_TRY(grad_dv_wv(c.p->W_v, dPv, c.dV, c.dvl, c.B, c.N, c.d, c.bf16_proj, c.s));
  return 0;
}

// 5a. weight gradients, reduced-precision mode at wide shapes (config 4): the single-product kernel of gemm_bf.hip, 256 x 256
// tiles; the parts of the two products share two rounds of workgroups in proportion to their contraction lengths
int run_dw_bf_tn(const Ctx& c, const Route& r, const Off& o) {
  const int B = c.B, d = c.d;
  float* part = c.ws + o.wo.part;
  TnGemm both[2] = {r.tnv, r.tnq};
  const int ntiles = (d / 256) * (d / 256);
  int total = (bf_tn_rounds() * 256 + ntiles - 1) / ntiles;
  total = total < 2 ? 2 : (total > kMaxParts ? kMaxParts : total);
  const double kv = (double)B * c.N, kq = (double)c.L * B * c.T;
  int pv = (int)(total * kv / (kv + kq) + 0.5);
  pv = pv < 1 ? 1 : (pv > total - 1 ? total - 1 : pv);
  int spp[2], parts[2];
  parts[0] = gemm_bf_tn_plan(both[0], pv, &spp[0]);
  both[1].C = part + (size_t)parts[0] * d * d;
  parts[1] = gemm_bf_tn_plan(both[1], total - pv, &spp[1]);
  CA_CHECK_ARG(parts[0] + parts[1] <= kMaxParts, "fused backward: %d split-K parts exceed the workspace", parts[0] + parts[1]);
  CA_TRY(run_small_reductions(c, o));
  CA_TRY(launch_gemm_bf_tn(both, spp, parts, 2, c.s));
  prof_mark(c.s, "bwd_gemm_dw");
  CA_TRY(launch_reduce_partials2(part, (float*)c.pg->dW_v, parts[0], both[1].C, (float*)c.pg->dW_q, parts[1], (int64_t)d * d,
                                 c.accumulate, c.s));
  prof_mark(c.s, "reduce_partials");
  return 0;
}

// 5b. both weight gradients in one launch: 32 split-K parts (x 16 tiles = the 512 workgroup slots) shared in proportion to the
// contraction lengths, so that all workgroups run about equally long; with them the small reductions and (Route::combine) the
// dQ projection's tiles; behind them the late dQ pass, which adds the partial sums (Route::red_in_dq)
int run_dw_tn_pair(const Ctx& c, const Route& r, const Off& o) {
  const int B = c.B, d = c.d, L = c.L;
  float* part = c.ws + o.wo.part;
  TnGemm both[2] = {r.tnv, r.tnq};
  const TnReduce small = small_reductions(c, o);
  const double kv = (double)B * c.N, kq = (double)L * B * c.T;
  const int budget = r.tn_budget;
  int pv = (int)((double)budget * kv / (kv + kq) + 0.5);
  pv = pv < 1 ? 1 : (pv > budget - 1 ? budget - 1 : pv);
  const int pq = (budget - pv) / L > 0 ? (budget - pv) / L * L : L;
  int ks[2], S[2];
  const int parts_v = r.wide ? gemm_tn_wide_plan(both[0], pv, &ks[0], &S[0]) : gemm_tn_plan(both[0], pv, &ks[0], &S[0]);
  both[1].C = r.use_dyn ? part : part + (size_t)parts_v * d * d;
  const int parts_q = r.wide ? gemm_tn_wide_plan(both[1], pq, &ks[1], &S[1]) : gemm_tn_plan(both[1], pq, &ks[1], &S[1]);
  CA_CHECK_ARG(parts_v + parts_q <= kMaxParts, "fused backward: %d split-K parts exceed the workspace", parts_v + parts_q);
  const WGemm* wextra = r.combine ? &r.wdq : nullptr;
  if (r.wide) CA_TRY(launch_gemm_tn_wide(both, ks, S, 2, c.s, &small, wextra, r.use_dyn ? &r.dyn_all : nullptr));
  else CA_TRY(launch_gemm_tn(both, ks, S, 2, c.s, &small, wextra));
  prof_mark(c.s, r.combine ? "bwd_gemm" : "bwd_gemm_dw");
  if (r.own_dq) {
    CA_TRY(run_dq_projection(c, r, o, false));
    prof_mark(c.s, "bwd_gemm_dq_projection");
  }
  if (r.red_in_dq) {
    RedJob red = {};
    red.part[0] = part; red.out[0] = (float*)c.pg->dW_v; red.np[0] = parts_v;
    red.part[1] = both[1].C; red.out[1] = (float*)c.pg->dW_q; red.np[1] = parts_q;
    red.n = (long)d * d; red.acc = c.accumulate;
    if (r.use_dyn) red.dyn = r.dyn_all;
    return run_own_dq(c, r, o, &red);
  }
  if (r.late_dq) CA_TRY(run_own_dq(c, r, o));
  CA_TRY(launch_reduce_partials2(part, (float*)c.pg->dW_v, parts_v, both[1].C, (float*)c.pg->dW_q, parts_q, (int64_t)d * d,
                                 c.accumulate, c.s));
  prof_mark(c.s, "reduce_partials");
  return 0;
}

// 5c. the weight gradients one by one: each on the hand-scheduled A^T B kernel (gemm_tn.hip) if it takes the job, else on the
// general GEMM
int run_dw_separate(const Ctx& c, const Route& r, const Off& o) {
  const int B = c.B, N = c.N, d = c.d;
  float* part = c.ws + o.wo.part;
  float* dPv = c.ws + o.wo.dPv;
  CA_TRY(run_small_reductions(c, o));
  // dW_v[j][k] = sum_{b,n} dP_v[b][n][j] V[b][k][n]
  if (r.tn_v) {
    CA_TRY(run_dw_tn(c, r.tnv, (float*)c.pg->dW_v));
  } else if (r.lm && c.vl.sB == (long)N * d) {
    // location-major, samples abutting: one flat contraction over m = (b, n), split-K over the B*N rows
    CA_TRY(grad_dw_splitk(dPv, c.V, B * N, d, part, (float*)c.pg->dW_v, c.accumulate, c.bf16_proj, c.s));
  } else {
    CA_TRY(grad_dw_sample_groups(dPv, c.V, c.vl, B, N, d, part, (float*)c.pg->dW_v, c.accumulate, c.bf16_proj, c.s));
  }
  // dW_q[j][k] = sum_l sum_m dP_q,l[m][j] Q_l[m][k]: levels as the inner loop, split-K over the B*T rows
  if (r.tn_q) {
    TnGemm tnq = r.tnq;
    tnq.C = part;
    return run_dw_tn(c, tnq, (float*)c.pg->dW_q);
  }
  return grad_dw_splitk(c.ws + o.wo.dPq, nullptr, B * c.T, d, part, (float*)c.pg->dW_q, c.accumulate, c.bf16_proj, c.s, c.Q, c.L,
                        (long)o.BTd);
}

}  // namespace

size_t fused_bwd_ws_floats(int B, int N, int T, int d, int L) { return fused_bwd_off(B, N, T, d, L).total; }

int fused_backward_supported(int B, int N, int T, int d, int L) { return fused_supported(B, N, T, d, L); }

// dQ_l = a_q (x) gq + dA V^T + dP_q W_q ;  dV = sum_l (a_v (x) gv + Q^T dA) + (sum_l dP_v) W_v.  The projection writes dQ first
// and the bf16 dA V kernel adds onto it (the GEMM is 24 us faster without an accumulate input); channel-major features with
// unaligned rows (N % 4 != 0): the exact-f32 kernel first, then the projection onto it.  When the projection shares the
// weight-gradient launch (Route::late_dq), the dA V kernel runs after that launch.
int fused_backward(const Ctx& c) {
  const int B = c.B, N = c.N, T = c.T, d = c.d, L = c.L;
  CA_CHECK_ARG(fused_backward_supported(B, N, T, d, L), "fused backward: unsupported shape");
  CA_CHECK_ARG(v_is_lm(c.vl, N, d) || v_is_cm(c.vl, N, d),
               "fused backward: image features must be channel-major [B,d,N] or location-major [B,N,d]");
  CA_CHECK_ARG(N <= 256, "fused backward: N > 256");
  const Off o{saved_off(B, N, T, d, L), fused_bwd_off(B, N, T, d, L), (size_t)B * T * d, (size_t)B * T * N, (size_t)B * N * d,
              (size_t)B * d};
  Route r;
  decide_route(c, o, r);
  CA_TRY(run_pre(c, r, o));
  BwdArgs ba = recompute_args(c, r, o);
  CA_TRY(launch_bwd_dc32(ba, c.s));                  // dC, dA
  prof_mark(c.s, "bwd_dc32");
  ba.dp_bf16 = r.dp_bf16 ? 1 : 0;
  CA_TRY(launch_bwd_nat32(ba, c.s));                 // dP_q, dP_v, dw_v, db_v, db_q
  prof_mark(c.s, "bwd_nat32");
  if (c.bil) {
    CA_TRY(run_bilinear_dq_dwb(c, r, o));
  } else if (!r.late_dq) {
    if (r.dq32) {
      CA_TRY(run_dq_projection(c, r, o, false));
      prof_mark(c.s, "bwd_gemm_dq_projection");
    }
    CA_TRY(run_own_dq(c, r, o));
  }
  if (c.dV) CA_TRY(run_dv(c, o));
  if (!r.dq32 && !c.bil) CA_TRY(run_dq_projection(c, r, o, true));
  CA_TRY(run_sum_dpv(c, r, o));
  if (r.bf_tn) return run_dw_bf_tn(c, r, o);
  if (r.tn_v && r.tn_q) return run_dw_tn_pair(c, r, o);
  return run_dw_separate(c, r, o);
}
