// Cross entropy of the train step on gfx950 (reference main.py:94 / :214: nn.CrossEntropyLoss() on the logits of
// MLPClassifier, mean over the batch) together with its gradient: one workgroup per row -- log-sum-exp, loss and
// d logits = (softmax - onehot) / B in one pass -- and a fixed-order sum of the row losses by the workgroup that finishes
// last (an integer ticket; no float atomics: deterministic).  (SURVEY.md section 8f-1.  The MLPClassifier itself stays on the stock PyTorch-ROCm modules: a
// composition of this library's GEMM for its four B-row products was built and measured in round 1 -- 30 launches,
// 0.53 ms against ~0.2 ms for the stock head -- and was removed again in round 2; see DESIGN.md.)
#include "common.h"

namespace {

__device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  return r;
}
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return r;
}

// row_loss[i] = (logsumexp(z_i) - z_i[label_i]) * inv_b ; dlogits = (softmax(z_i) - onehot(label_i)) * inv_b.
// A label outside [0, K) makes the row's loss NaN and raises the status word (nn.CrossEntropyLoss raises there:
// coattn_ce_status reports it at the caller's next synchronisation point).
// The mean rides in the same launch: the workgroup that finishes LAST (a ticket from status[1], which it leaves at 0 for the
// next call) adds the B row losses in sum_all_kernel's fixed order -- whichever workgroup that is, the same bits.  status[0]
// and status[1] are 0 when the launch starts (the caller's memset, or the answer head's last layer: head.hip).
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                      float* row_loss, float* __restrict__ dlogits, int K,
                                                      float inv_b, int* status, int ldd, float* __restrict__ loss, int B) {
  __shared__ float sh[4];
  __shared__ unsigned ticket;
  const int i = blockIdx.x;
  const float* z = logits + (long)i * K;
  float m = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) m = fmaxf(m, z[k]);
  m = block_max(m, sh);
  float s = 0.f;
  for (int k = threadIdx.x; k < K; k += 256) s += expf(z[k] - m);
  s = block_sum(s, sh);
  const long long lab = labels[i];
  const bool ok = lab >= 0 && lab < K;
  if (threadIdx.x == 0) {                             // (before the gradient row is stored: the fence has nothing of it to wait for)
    __hip_atomic_store(&row_loss[i], ok ? (logf(s) + m - z[lab]) * inv_b : NAN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!ok) status[0] = i + 1;                       // (any offending row: the writers race benignly)
    __threadfence();                                  // the row loss is visible device-wide before the ticket is taken
    ticket = atomicAdd(reinterpret_cast<unsigned*>(status) + 1, 1u);
  }
  if (dlogits) {
    const float inv = inv_b / s;
    for (int k = threadIdx.x; k < ldd; k += 256)     // rows ldd >= K floats apart, the padding zeroed
      dlogits[(long)i * ldd + k] = k < K ? expf(z[k] - m) * inv - ((ok && k == lab) ? inv_b : 0.f) : 0.f;
  }
  __syncthreads();
  if (ticket != (unsigned)(B - 1)) return;
  __threadfence();
  float acc = 0.f;                                    // (sum_all_kernel's order: strided per thread, wave sums, (0 + 1) + (2 + 3))
  for (int r = threadIdx.x; r < B; r += 256) acc += __hip_atomic_load(&row_loss[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    loss[0] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    reinterpret_cast<unsigned*>(status)[1] = 0u;
  }
}

// ---- soft answer targets (VQA: at most A (answer, score) pairs per sample; include/coattn.h "soft answer targets") --------
// The dense target t[b][k] = sum over the slots a with ans_idx[b][a] == k of ans_score[b][a] never exists in memory: the row's A
// slots go to LDS once and every thread forms t for its own k from them (A broadcast reads and compares per class; slot order,
// so duplicates add in a fixed order).  An empty slot (index -1) contributes 0 and its score is not read.
constexpr int kMaxAns = 16;

struct Slots {
  int idx[kMaxAns];
  float sc[kMaxAns];              // the slot's score (0 for an empty slot)
  float scb[kMaxAns];             // sc * inv_b, rounded HERE: the gradient's  e * inv - t / B  then has the hard-label kernel's shape
};
// thread a < A loads slot a; behind the barrier every thread knows the row's S = sum of scores and whether an index is out of range
__device__ __forceinline__ void load_slots(Slots& sl, const int* __restrict__ ans_idx, const float* __restrict__ ans_score, int A,
                                           int row, int K, float inv_b, float& S, bool& ok) {
  if ((int)threadIdx.x < A) {
    const int a = ans_idx[(long)row * A + threadIdx.x];
    const float v = a >= 0 ? ans_score[(long)row * A + threadIdx.x] : 0.f;
    sl.idx[threadIdx.x] = a;
    sl.sc[threadIdx.x] = v;
    sl.scb[threadIdx.x] = v * inv_b;
  }
  __syncthreads();
  S = 0.f;
  ok = true;
  for (int a = 0; a < A; ++a) {
    ok = ok && sl.idx[a] >= -1 && sl.idx[a] < K;
    S += sl.sc[a];
  }
}
__device__ __forceinline__ float target_of(const int* idx, const float* sc, int A, int k) {
  float t = 0.f;
  for (int a = 0; a < A; ++a) t += idx[a] == k ? sc[a] : 0.f;
  return t;
}
// min(t, 1) that lets a NaN through (fminf would return its other argument: a NaN score in a live slot would become a target of 1)
__device__ __forceinline__ float clamp_one(float t) { return t > 1.f ? 1.f : t; }
// max(z, 0) + log1p(exp(-|z|)): finite for every finite z
__device__ __forceinline__ float softplus_safe(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float sigmoid_safe(float z) {
  const float e = expf(-fabsf(z));
  return (z >= 0.f ? 1.f : e) / (1.f + e);
}

// KIND = COATTN_LOSS_SOFT_CE: row = S lse(z) - sum_k t z,                      d / dz = (S softmax(z) - t) / B
// KIND = COATTN_LOSS_BCE    : row = sum_k softplus(z) - min(t, 1) z,           d / dz = (sigmoid(z) - min(t, 1)) / B
//                             (min(t, 1) = clamp_one: a NaN target stays NaN, as SOFT_CE's does through S and t z)
// Everything else -- one workgroup per row, the padded gradient row, the status word for an index outside [-1, K), the mean by
// the last-ticket workgroup in sum_all's order -- is ce_rows_kernel's.  For a row whose only slot is (label, 1) the soft cross
// entropy's expressions reduce to ce_rows_kernel's operation for operation (S = 1, t z = z[label], t / B = inv_b): same bits.
template <int KIND>
__global__ __launch_bounds__(256) void soft_rows_kernel(const float* __restrict__ logits, const int* __restrict__ ans_idx,
                                                        const float* __restrict__ ans_score, int A, float* row_loss,
                                                        float* __restrict__ dlogits, int K, float inv_b, int* status, int ldd,
                                                        float* __restrict__ loss, int B) {
  __shared__ float sh[4];
  __shared__ unsigned ticket;
  __shared__ Slots sl;
  const int i = blockIdx.x;
  const float* z = logits + (long)i * K;
  float S;
  bool ok;
  load_slots(sl, ans_idx, ans_score, A, i, K, inv_b, S, ok);
  float m = 0.f, s = 1.f, row;
  if constexpr (KIND == COATTN_LOSS_SOFT_CE) {
    m = -INFINITY;
    for (int k = threadIdx.x; k < K; k += 256) m = fmaxf(m, z[k]);
    m = block_max(m, sh);
    s = 0.f;
    float tz = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
      s += expf(z[k] - m);
      const float t = target_of(sl.idx, sl.sc, A, k);
      tz += t != 0.f ? t * z[k] : 0.f;                // (a class without a target may be masked with -inf: 0 * -inf is no term)
    }
    s = block_sum(s, sh);
    if (m == INFINITY) s = INFINITY;                  // a +inf logit: logsumexp = +inf, softmax NaN there and 0 elsewhere (torch.logsumexp)
    tz = block_sum(tz, sh);
    row = (S * (logf(s) + m) - tz) * inv_b;
  } else {
    float acc = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) acc += softplus_safe(z[k]) - clamp_one(target_of(sl.idx, sl.sc, A, k)) * z[k];
    row = block_sum(acc, sh) * inv_b;
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(&row_loss[i], ok ? row : NAN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!ok) status[0] = i + 1;
    __threadfence();
    ticket = atomicAdd(reinterpret_cast<unsigned*>(status) + 1, 1u);
  }
  if (dlogits) {
    if constexpr (KIND == COATTN_LOSS_SOFT_CE) {
      const float inv = S * (inv_b / s);
      for (int k = threadIdx.x; k < ldd; k += 256)
        dlogits[(long)i * ldd + k] = k < K ? expf(z[k] - m) * inv - target_of(sl.idx, sl.scb, A, k) : 0.f;
    } else {
      for (int k = threadIdx.x; k < ldd; k += 256)
        dlogits[(long)i * ldd + k] = k < K ? (sigmoid_safe(z[k]) - clamp_one(target_of(sl.idx, sl.sc, A, k))) * inv_b : 0.f;
    }
  }
  __syncthreads();
  if (ticket != (unsigned)(B - 1)) return;
  __threadfence();
  float acc = 0.f;
  for (int r = threadIdx.x; r < B; r += 256) acc += __hip_atomic_load(&row_loss[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    loss[0] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    reinterpret_cast<unsigned*>(status)[1] = 0u;
  }
}

// Evaluation: pred[i] = argmax_k z[i][k] (the lowest index among equal maxima; a NaN logit counts as the maximum, the lowest
// such index winning, as in numpy and torch), row score = min(1, t[i][pred[i]]) (a NaN score in a live slot stays NaN) -- the
// VQA accuracy of the predicted answer -- and the fixed-order sum of the row scores by the last-ticket workgroup, as above.
// (the index reduction rides on wave_max: -(float)k is exact for k < 2^24)
__global__ __launch_bounds__(256) void vqa_score_kernel(const float* __restrict__ logits, const int* __restrict__ ans_idx,
                                                        const float* __restrict__ ans_score, int A, int* __restrict__ pred,
                                                        float* __restrict__ row_score, float* row_ws, int K, int* status,
                                                        float* __restrict__ score_sum, int B) {
  __shared__ float sh[4];
  __shared__ unsigned ticket;
  __shared__ Slots sl;
  const int i = blockIdx.x;
  const float* z = logits + (long)i * K;
  float S;
  bool ok;
  load_slots(sl, ans_idx, ans_score, A, i, K, 1.f, S, ok);
  float best = -INFINITY;
  int at = threadIdx.x < (unsigned)K ? (int)threadIdx.x : K;     // (K: no candidate; thread 0 always has one, so pred < K)
  int nan_at = K;                                                // the thread's lowest index of a NaN logit (K: none)
  for (int k = threadIdx.x; k < K; k += 256) {
    const float v = z[k];
    if (v > best) { best = v; at = k; }
    if (v != v && nan_at == K) nan_at = k;
  }
  const float m = block_max(best, sh);
  int p = (int)-block_max(best == m ? -(float)at : -(float)K, sh);
  const int pn = (int)-block_max(-(float)nan_at, sh);            // numpy's and torch's argmax: the first NaN wins
  if (pn < K) p = pn;
  if (threadIdx.x == 0) {
    const float sc = ok ? clamp_one(target_of(sl.idx, sl.sc, A, p)) : NAN;
    pred[i] = p;
    if (row_score) row_score[i] = sc;
    __hip_atomic_store(&row_ws[i], sc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!ok) status[0] = i + 1;
    __threadfence();
    ticket = atomicAdd(reinterpret_cast<unsigned*>(status) + 1, 1u);
  }
  __syncthreads();
  if (ticket != (unsigned)(B - 1)) return;
  __threadfence();
  float acc = 0.f;
  for (int r = threadIdx.x; r < B; r += 256) acc += __hip_atomic_load(&row_ws[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    score_sum[0] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    reinterpret_cast<unsigned*>(status)[1] = 0u;
  }
}

}  // namespace

// rows + mean for the answer head (head.hip): row_loss [B] scratch, dlogits [B][ldd] (ldd = 0: K) or NULL.
// zeroed: status[0] and status[1] have been cleared by an earlier launch on this stream (head.hip's logits layer)
int launch_ce_rows(const float* logits, const void* labels, float* row_loss, float* dlogits, float* loss, int B, int K,
                   int* status, hipStream_t s, int ldd, bool zeroed) {
  if (!zeroed && hipMemsetAsync(status, 0, 16, s) != hipSuccess) {       // (a memset node under graph capture)
    coattn_set_error("ce: clearing the status word failed");
    return -3;
  }
  hipLaunchKernelGGL(ce_rows_kernel, dim3(B), dim3(256), 0, s, logits, (const long long*)labels, row_loss, dlogits, K,
                     1.0f / (float)B, status, ldd > 0 ? ldd : K, loss, B);
  CA_CHECK_LAUNCH("ce_rows");
  return 0;
}

// the soft-target rows + mean, for coattn_soft_loss_forward and the answer head (head.hip): launch_ce_rows' arguments with the
// slots in place of the labels
int launch_soft_rows(const float* logits, const void* ans_idx, const void* ans_score, int A, int kind, float* row_loss,
                     float* dlogits, float* loss, int B, int K, int* status, hipStream_t s, int ldd, bool zeroed) {
  if (!zeroed && hipMemsetAsync(status, 0, 16, s) != hipSuccess) {
    coattn_set_error("soft loss: clearing the status word failed");
    return -3;
  }
  if (kind == COATTN_LOSS_SOFT_CE)
    hipLaunchKernelGGL(soft_rows_kernel<COATTN_LOSS_SOFT_CE>, dim3(B), dim3(256), 0, s, logits, (const int*)ans_idx,
                       (const float*)ans_score, A, row_loss, dlogits, K, 1.0f / (float)B, status, ldd > 0 ? ldd : K, loss, B);
  else
    hipLaunchKernelGGL(soft_rows_kernel<COATTN_LOSS_BCE>, dim3(B), dim3(256), 0, s, logits, (const int*)ans_idx,
                       (const float*)ans_score, A, row_loss, dlogits, K, 1.0f / (float)B, status, ldd > 0 ? ldd : K, loss, B);
  CA_CHECK_LAUNCH("soft_rows");
  return 0;
}
// argument checks shared by the three entry points that take soft targets
int check_soft_targets(const char* what, const void* ans_idx, const void* ans_score, int A, int kind) {
  CA_CHECK_ARG(A >= 1 && A <= kMaxAns, "%s: A=%d answer slots per sample (1..%d supported)", what, A, kMaxAns);
  CA_CHECK_ARG(kind == COATTN_LOSS_SOFT_CE || kind == COATTN_LOSS_BCE,
               "%s: unknown loss kind %d (COATTN_LOSS_SOFT_CE = 1, COATTN_LOSS_BCE = 2)", what, kind);
  CA_CHECK_ARG(ans_idx && ans_score, "%s: null ans_idx / ans_score", what);
  return 0;
}

extern "C" int coattn_ce_workspace_bytes(int B, int K, int dtype, size_t* ws) {
  CA_CHECK_ARG(dtype == COATTN_F32, "unsupported dtype %d (only COATTN_F32)", dtype);
  CA_CHECK_ARG(B > 0 && K > 0, "bad B=%d / K=%d", B, K);
  if (ws) *ws = (al64((size_t)B) + 64) * sizeof(float);        // row losses + the status word (its own 256 bytes)
  return 0;
}

// Synchronises `stream` and reports whether the coattn_ce_forward / coattn_head_forward call that last used this
// workspace / saved buffer met a label outside [0, K): -2 (message: the offending row) or 0.
static int status_check(const int* status_dev, void* stream, const char* what) {
  int host = 0;
  if (hipMemcpyAsync(&host, status_dev, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
    coattn_set_error("%s: reading the status word failed", what);
    return -3;
  }
  if (host != 0) {
    coattn_set_error("%s: label of row %d is outside [0, K) (nn.CrossEntropyLoss: 'Target out of bounds')", what, host - 1);
    return -2;
  }
  return 0;
}

extern "C" int coattn_ce_status(const void* ws, int B, void* stream) {
  CA_CHECK_ARG(ws && B > 0, "ce_status: bad argument");
  return status_check(reinterpret_cast<const int*>((const float*)ws + al64((size_t)B)), stream, "cross entropy");
}
int head_status_check(const int* status_dev, void* stream) { return status_check(status_dev, stream, "answer head"); }

extern "C" int coattn_ce_forward(const void* logits, const void* labels, void* loss, void* dlogits, void* ws, int B,
                                 int K, int dtype, void* stream) {
  CA_CHECK_ARG(dtype == COATTN_F32, "unsupported dtype %d (only COATTN_F32)", dtype);
  CA_CHECK_ARG(B > 0 && B <= (1 << 24) && K > 0, "bad B=%d / K=%d", B, K);
  CA_CHECK_ARG(logits && labels && loss && ws, "ce_forward: null argument");                   // dlogits may be NULL
  hipStream_t s = (hipStream_t)stream;
  return launch_ce_rows((const float*)logits, labels, (float*)ws, (float*)dlogits, (float*)loss, B, K,
                        reinterpret_cast<int*>((float*)ws + al64((size_t)B)), s, 0, false);
}

extern "C" int coattn_soft_loss_forward(const void* logits, const void* ans_idx, const void* ans_score, int A, int kind,
                                        void* loss, void* dlogits, void* ws, int B, int K, int dtype, void* stream) {
  CA_CHECK_ARG(dtype == COATTN_F32, "unsupported dtype %d (only COATTN_F32)", dtype);
  CA_CHECK_ARG(B > 0 && B <= (1 << 24) && K > 0, "bad B=%d / K=%d", B, K);
  CA_TRY(check_soft_targets("soft_loss_forward", ans_idx, ans_score, A, kind));
  CA_CHECK_ARG(logits && loss && ws, "soft_loss_forward: null argument");                       // dlogits may be NULL
  return launch_soft_rows((const float*)logits, ans_idx, ans_score, A, kind, (float*)ws, (float*)dlogits, (float*)loss, B, K,
                          reinterpret_cast<int*>((float*)ws + al64((size_t)B)), (hipStream_t)stream, 0, false);
}

extern "C" int coattn_vqa_score(const void* logits, const void* ans_idx, const void* ans_score, int A, void* pred,
                                void* row_score, void* score_sum, void* ws, int B, int K, int dtype, void* stream) {
  CA_CHECK_ARG(dtype == COATTN_F32, "unsupported dtype %d (only COATTN_F32)", dtype);
  CA_CHECK_ARG(B > 0 && B <= (1 << 24) && K > 0 && K <= (1 << 24), "bad B=%d / K=%d", B, K);
  CA_TRY(check_soft_targets("vqa_score", ans_idx, ans_score, A, COATTN_LOSS_SOFT_CE));
  CA_CHECK_ARG(logits && pred && score_sum && ws, "vqa_score: null argument");                  // row_score may be NULL
  hipStream_t s = (hipStream_t)stream;
  int* status = reinterpret_cast<int*>((float*)ws + al64((size_t)B));
  if (hipMemsetAsync(status, 0, 16, s) != hipSuccess) {
    coattn_set_error("vqa_score: clearing the status word failed");
    return -3;
  }
  hipLaunchKernelGGL(vqa_score_kernel, dim3(B), dim3(256), 0, s, (const float*)logits, (const int*)ans_idx,
                     (const float*)ans_score, A, (int*)pred, (float*)row_score, (float*)ws, K, status, (float*)score_sum, B);
  CA_CHECK_LAUNCH("vqa_score");
  return 0;
}
