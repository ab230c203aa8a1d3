// Scoring given audio under the model (mvn_score_columns): per-position log-likelihood, entropy and rank of the target
// from the head's logits, and their per-sequence sums -- READ ONLY, no probability tensor.
//
//   y = logits / temperature                      (formed as (l - max l) / T: the subtraction is exact where it matters)
//   logp[b,s]    = y_t - logsumexp_q(y)           nats
//   entropy[b,s] = log(sum_q e_q) - (sum_q e_q d_q) / sum_q e_q,   d_q = y_q - max y, e_q = exp(d_q)
//                                                 (= -sum p log p; a class with e_q = 0 adds exactly 0, never 0 * -inf)
//   log(sum_q e_q) = log1p(sum over the classes below the maximum) where ONE class holds the maximum: a column whose
//                                                 other classes add up to less than an ulp of 1 keeps a logp and an
//                                                 entropy of the right size instead of 0
//   rank[b,s]    = #{q : l_q > l_t} + #{q < t : l_q == l_t}        on the RAW logits: T > 0 keeps their order, and a
//                                                 division could round two different logits onto one value
//   seq_nll[b]   = -sum_s logp[b,s],   seq_correct[b] = #{s : rank == 0}
//
// The kernels mirror the loss forward's two forms (trainer.hip): the column form (Q <= 256: lane = column, a class row
// per register, rows through a raw buffer with scalar offsets) and one thread per column with 64-bit addresses (any Q,
// any row length).  They store nothing per class: a workgroup writes its columns' outputs and ONE partial sum of logp
// and of the correct columns into the caller's scratch -- every slot the second kernel reads, so the scratch needs no
// initialisation -- and score_reduce_kernel adds one sequence's partials in a fixed order in double.  No atomics: two
// calls return the same bits.
#include <cmath>

#include "common.h"

namespace mvn {

constexpr int SQ = 64;  // class rows per wave = registers per thread (Q <= 4 * SQ)

// what a thread carries of its column (or of its wave's quarter of it) after the exponential pass
struct ScoreAcc {
  float rest, top;  // sum of e_q over the classes below the maximum, number of classes AT the maximum (e_q = 1)
  float s2;         // sum_q e_q d_q (the classes at the maximum add 0)
  int above;        // classes ranked before the target
};

__device__ __forceinline__ void score_class(ScoreAcc &a, float l, int q, float m, float lt, int tq, float inv_t,
                                            bool entropy) {
  const float d = (l - m) * inv_t;
  const float e = sm_exp(d);  // exp(-inf) = 0: padding rows and masked classes
  a.rest += l == m ? 0.f : e;
  a.top += l == m ? 1.f : 0.f;
  if (entropy) a.s2 += e > 0.f ? e * d : 0.f;
  a.above += (l > lt || (l == lt && q < tq)) ? 1 : 0;
}

// the column's results, from the whole column's sums
__device__ __forceinline__ void score_store(const ScoreAcc &a, float m, float lt, float inv_t, size_t at,
                                            float *__restrict__ logp, float *__restrict__ entropy,
                                            int32_t *__restrict__ rank, float &lp) {
  const float ls = a.top == 1.f ? log1pf(a.rest) : logf(a.top + a.rest);
  lp = (lt - m) * inv_t - ls;
  if (logp) logp[at] = lp;
  if (entropy) entropy[at] = ls - a.s2 / (a.top + a.rest);
  if (rank) rank[at] = a.above;
}

// MASK (mvn_score_columns_len): sequence b counts its columns s < valid[b] only (clamped to [0, S]); the others store
// logp = entropy = 0 and rank = -1 and are SELECTED out of the two sums, whatever their logits hold.
__device__ __forceinline__ void score_store_masked(size_t at, float *__restrict__ logp, float *__restrict__ entropy,
                                                   int32_t *__restrict__ rank) {
  if (logp) logp[at] = 0.f;
  if (entropy) entropy[at] = 0.f;
  if (rank) rank[at] = -1;
}

// 64 columns per workgroup, wave w holds class rows [64w, 64w + 64) of them, lane = column.  Lanes past the end of the
// row work on column 0 (valid memory, nothing of it stored).  Two LDS exchanges: (max, target's logit), then the sums.
template <bool ENTROPY, bool MASK>
__device__ __forceinline__ void score_cols(const float *__restrict__ y, const long long *__restrict__ target, int Q,
                                           int S, float inv_t, float *__restrict__ logp,
                                           float *__restrict__ entropy, int32_t *__restrict__ rank,
                                           float *__restrict__ nll_part, int32_t *__restrict__ ok_part,
                                           const int32_t *__restrict__ valid) {
  __shared__ float part[4][4][64];
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = blockIdx.x * 64 + lane;
  const bool live = s < S;
  const __amdgpu_buffer_rsrc_t yb = col_rsrc(y + (size_t)b * Q * S);
  const int voff = 4 * (live ? s : 0), row = 4 * S;
  const long long tg = target[(size_t)b * S + (live ? s : 0)];
  const int tq = (int)min(max(tg, 0LL), (long long)(Q - 1));
  float v[SQ];
  float m = -INFINITY, lt = -INFINITY;  // lt: the target's logit, in the wave that holds its row
#pragma unroll
  for (int i = 0; i < SQ; ++i) {
    const int q = SQ * wave + i;
    v[i] = q < Q ? col_ld(yb, voff, q * row) : -INFINITY;
    if (q == tq) lt = v[i];
    m = fmaxf(m, v[i]);
  }
  part[0][wave][lane] = m;
  part[1][wave][lane] = lt;
  __syncthreads();
  m = fmaxf(fmaxf(part[0][0][lane], part[0][1][lane]), fmaxf(part[0][2][lane], part[0][3][lane]));
  lt = part[1][tq / SQ][lane];
  __syncthreads();
  ScoreAcc a = {0.f, 0.f, 0.f, 0};
#pragma unroll
  for (int i = 0; i < SQ; ++i) score_class(a, v[i], SQ * wave + i, m, lt, tq, inv_t, ENTROPY);
  part[0][wave][lane] = a.rest;
  part[1][wave][lane] = a.s2;
  part[2][wave][lane] = __int_as_float(a.above);
  part[3][wave][lane] = a.top;
  __syncthreads();
  if (wave != 0) return;
  a.rest = (part[0][0][lane] + part[0][1][lane]) + (part[0][2][lane] + part[0][3][lane]);
  a.top = (part[3][0][lane] + part[3][1][lane]) + (part[3][2][lane] + part[3][3][lane]);
  a.s2 = (part[1][0][lane] + part[1][1][lane]) + (part[1][2][lane] + part[1][3][lane]);
  a.above = (__float_as_int(part[2][0][lane]) + __float_as_int(part[2][1][lane])) +
            (__float_as_int(part[2][2][lane]) + __float_as_int(part[2][3][lane]));
  float lp = 0.f;
  const bool counted = MASK ? s < min(max(valid[b], 0), S) : live;
  if (counted)
    score_store(a, m, lt, inv_t, (size_t)b * S + s, logp, ENTROPY ? entropy : nullptr, rank, lp);
  else if (MASK && live)
    score_store_masked((size_t)b * S + s, logp, ENTROPY ? entropy : nullptr, rank);
  const float nll = wave_sum(counted ? -lp : 0.f);
  const float ok = wave_sum(counted && a.above == 0 ? 1.f : 0.f);
  if (lane == 0) {
    const size_t wg = (size_t)b * gridDim.x + blockIdx.x;
    nll_part[wg] = nll;
    ok_part[wg] = (int)ok;
  }
}

// (held to the four waves per SIMD of the loss kernels: 128 registers hold the 64 class rows and what is summed)
template <bool ENTROPY>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void score_cols_kernel(
    const float *__restrict__ y, const long long *__restrict__ target, int Q, int S, float inv_t,
    float *__restrict__ logp, float *__restrict__ entropy, int32_t *__restrict__ rank, float *__restrict__ nll_part,
    int32_t *__restrict__ ok_part) {
  score_cols<ENTROPY, false>(y, target, Q, S, inv_t, logp, entropy, rank, nll_part, ok_part, nullptr);
}

template <bool ENTROPY>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void score_cols_len_kernel(
    const float *__restrict__ y, const long long *__restrict__ target, int Q, int S, float inv_t,
    float *__restrict__ logp, float *__restrict__ entropy, int32_t *__restrict__ rank, float *__restrict__ nll_part,
    int32_t *__restrict__ ok_part, const int32_t *__restrict__ valid) {
  score_cols<ENTROPY, true>(y, target, Q, S, inv_t, logp, entropy, rank, nll_part, ok_part, valid);
}

// any Q, any row length: one thread per column, 64-bit addresses, the column walked twice
// (MASK: a column at or beyond valid[b] reads nothing)
template <bool MASK>
__device__ __forceinline__ void score_wide(const float *__restrict__ y, const long long *__restrict__ target, int Q,
                                           int S, float inv_t, float *__restrict__ logp, float *__restrict__ entropy,
                                           int32_t *__restrict__ rank, float *__restrict__ nll_part,
                                           int32_t *__restrict__ ok_part, const int32_t *__restrict__ valid,
                                           const long long s) {
  const int b = blockIdx.y;
  float nll = 0.f, ok = 0.f;
  if (MASK && s < S && s >= min(max(valid[b], 0), S)) {
    score_store_masked((size_t)b * S + s, logp, entropy, rank);
  } else if (s < S) {
    const float *col = y + (size_t)b * Q * S + s;
    const long long tg = target[(size_t)b * S + s];
    const int tq = (int)min(max(tg, 0LL), (long long)(Q - 1));
    const float lt = col[(size_t)tq * S];
    float m = -INFINITY;
    for (int q = 0; q < Q; ++q) m = fmaxf(m, col[(size_t)q * S]);
    ScoreAcc a = {0.f, 0.f, 0.f, 0};
    for (int q = 0; q < Q; ++q) score_class(a, col[(size_t)q * S], q, m, lt, tq, inv_t, entropy != nullptr);
    float lp;
    score_store(a, m, lt, inv_t, (size_t)b * S + s, logp, entropy, rank, lp);
    nll = -lp;
    ok = a.above == 0 ? 1.f : 0.f;
  }
  __shared__ float ns[4], cs[4];
  nll = wave_sum(nll);
  ok = wave_sum(ok);
  if ((threadIdx.x & 63) == 0) {
    ns[threadIdx.x >> 6] = nll;
    cs[threadIdx.x >> 6] = ok;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t wg = (size_t)b * gridDim.x + blockIdx.x;
    nll_part[wg] = (ns[0] + ns[1]) + (ns[2] + ns[3]);
    ok_part[wg] = (int)((cs[0] + cs[1]) + (cs[2] + cs[3]));
  }
}

__global__ __launch_bounds__(256) void score_wide_kernel(const float *__restrict__ y,
                                                         const long long *__restrict__ target, int Q, int S,
                                                         float inv_t, float *__restrict__ logp,
                                                         float *__restrict__ entropy, int32_t *__restrict__ rank,
                                                         float *__restrict__ nll_part,
                                                         int32_t *__restrict__ ok_part) {
  score_wide<false>(y, target, Q, S, inv_t, logp, entropy, rank, nll_part, ok_part, nullptr,
                    (long long)blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void score_wide_len_kernel(const float *__restrict__ y,
                                                             const long long *__restrict__ target, int Q, int S,
                                                             float inv_t, float *__restrict__ logp,
                                                             float *__restrict__ entropy, int32_t *__restrict__ rank,
                                                             float *__restrict__ nll_part,
                                                             int32_t *__restrict__ ok_part,
                                                             const int32_t *__restrict__ valid) {
  score_wide<true>(y, target, Q, S, inv_t, logp, entropy, rank, nll_part, ok_part, valid,
                   (long long)blockIdx.x * blockDim.x + threadIdx.x);
}

// One wave per sequence: lane i adds partials i, i + 64, ... in double, then a fixed butterfly -- the same order, hence
// the same bits, on every call.  `parts` = 0 (an empty sequence) stores zeros.
__global__ __launch_bounds__(64) void score_reduce_kernel(const float *__restrict__ nll_part,
                                                          const int32_t *__restrict__ ok_part, int parts,
                                                          float *__restrict__ seq_nll,
                                                          int32_t *__restrict__ seq_correct) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double nll = 0.0;
  int ok = 0;
  for (int i = lane; i < parts; i += 64) {
    nll += (double)nll_part[(size_t)b * parts + i];
    ok += ok_part[(size_t)b * parts + i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nll += __shfl_xor(nll, o, 64);
    ok += __shfl_xor(ok, o, 64);
  }
  if (lane == 0) {
    if (seq_nll) seq_nll[b] = (float)nll;
    if (seq_correct) seq_correct[b] = ok;
  }
}

}  // namespace mvn

extern "C" {

// one float and one int32 slot per 64-column workgroup (the wide form uses a quarter of them)
size_t mvn_score_scratch_floats(int batch, int s_len) {
  if (batch <= 0 || s_len <= 0) return 0;
  return 2 * (size_t)batch * (size_t)((s_len + 63) / 64);
}

// (mvn_score_columns and its _len form share this; `valid` == NULL launches the unmasked kernels)
static int score_columns_impl(const char *what, const float *logits, const long long *target, int batch, int classes,
                              int s_len, float temperature, float *logp, float *entropy, int32_t *rank,
                              float *seq_nll, int32_t *seq_correct, float *scratch, size_t scratch_floats,
                              const int32_t *valid, void *stream) {
  if (batch < 0 || classes < 1 || s_len < 0 || batch > 65535) {
    mvn::set_error("%s: bad argument (batch in [0, 65535], classes >= 1, s_len >= 0)", what);
    return MVN_ERR_BAD_ARG;
  }
  if (!(temperature > 0.f) || std::isinf(temperature)) {  // (NaN fails the comparison)
    mvn::set_error("%s: bad argument (temperature %g is not a finite number above 0)", what,
                   (double)temperature);
    return MVN_ERR_BAD_ARG;
  }
  if (batch == 0) return MVN_OK;
  const size_t need = mvn_score_scratch_floats(batch, s_len);
  if ((s_len > 0 && (!logits || !target)) || (need > 0 && !scratch) || scratch_floats < need) {
    mvn::set_error("%s: bad argument (logits, target or scratch missing, or scratch of %zu floats "
                   "where mvn_score_scratch_floats asks for %zu)", what, scratch_floats, need);
    return MVN_ERR_BAD_ARG;
  }
  const float inv_t = 1.0f / temperature;
  // (the column form addresses a sequence's (Q, S) tensor with 32-bit offsets: common.h rows_fit_rsrc)
  const bool cols = classes <= 4 * mvn::SQ && mvn::rows_fit_rsrc(classes, s_len);
  const int parts = s_len == 0 ? 0 : cols ? (s_len + 63) / 64 : (s_len + 255) / 256;
  float *nll_part = scratch;
  int32_t *ok_part = (int32_t *)(scratch + (size_t)batch * parts);
  if (s_len > 0) {
    if (cols && valid) {
      const auto kernel = entropy ? mvn::score_cols_len_kernel<true> : mvn::score_cols_len_kernel<false>;
      hipLaunchKernelGGL(kernel, dim3(parts, batch), dim3(256), 0, (hipStream_t)stream, logits, target, classes,
                         s_len, inv_t, logp, entropy, rank, nll_part, ok_part, valid);
    } else if (cols) {
      const auto kernel = entropy ? mvn::score_cols_kernel<true> : mvn::score_cols_kernel<false>;
      hipLaunchKernelGGL(kernel, dim3(parts, batch), dim3(256), 0, (hipStream_t)stream, logits, target, classes,
                         s_len, inv_t, logp, entropy, rank, nll_part, ok_part);
    } else if (valid) {
      hipLaunchKernelGGL(mvn::score_wide_len_kernel, dim3(parts, batch), dim3(256), 0, (hipStream_t)stream, logits,
                         target, classes, s_len, inv_t, logp, entropy, rank, nll_part, ok_part, valid);
    } else {
      hipLaunchKernelGGL(mvn::score_wide_kernel, dim3(parts, batch), dim3(256), 0, (hipStream_t)stream, logits,
                         target, classes, s_len, inv_t, logp, entropy, rank, nll_part, ok_part);
    }
    const int rc = mvn::check_hip(hipGetLastError(), what);
    if (rc != MVN_OK) return rc;
  }
  if (seq_nll || seq_correct) {
    hipLaunchKernelGGL(mvn::score_reduce_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, nll_part, ok_part,
                       parts, seq_nll, seq_correct);
    return mvn::check_hip(hipGetLastError(), what);
  }
  return MVN_OK;
}

int mvn_score_columns(const float *logits, const long long *target, int batch, int classes, int s_len,
                      float temperature, float *logp, float *entropy, int32_t *rank, float *seq_nll,
                      int32_t *seq_correct, float *scratch, size_t scratch_floats, void *stream) {
  return score_columns_impl("mvn_score_columns", logits, target, batch, classes, s_len, temperature, logp, entropy,
                            rank, seq_nll, seq_correct, scratch, scratch_floats, nullptr, stream);
}

int mvn_score_columns_len(const float *logits, const long long *target, int batch, int classes, int s_len,
                          float temperature, float *logp, float *entropy, int32_t *rank, float *seq_nll,
                          int32_t *seq_correct, float *scratch, size_t scratch_floats, const int32_t *valid,
                          void *stream) {
  return score_columns_impl("mvn_score_columns_len", logits, target, batch, classes, s_len, temperature, logp,
                            entropy, rank, seq_nll, seq_correct, scratch, scratch_floats, valid, stream);
}

}  // extern "C"
