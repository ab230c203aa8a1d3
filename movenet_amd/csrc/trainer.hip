// The trainer's element-wise tail as single passes (row F3 of SURVEY.md section 8):
//
//   mvn_softmax_ce_forward   head logits -> probabilities (in place) + the loss
//                            cross_entropy(PROBABILITIES, target) + the accuracy,
//                            one read and one write of the (B,Q,S) tensor
//                            (movenet/wavenet.py:189-191 + pytorch_lightning_trainer.py:64-66)
//   mvn_softmax_ce_backward  probabilities + target -> gradient w.r.t. the LOGITS, written
//                            straight into mvn_backward's padded dlogit tensor: the gradient
//                            of the loss through cross_entropy's own log-softmax and through
//                            the model's softmax in one read and one write
//   mvn_softmax_ce_*_ex      the same pair with the loss rule chosen: MVN_LOSS_MODEL is the negative log-likelihood
//                            of softmax(logits) itself -- same probabilities, one exponential pass forward, a
//                            streaming p - onehot backward (ce_model_bwd_kernel)
//   mvn_softmax_ce_*_len     the _ex pair over sequences of their own length: a device array of per-sequence column
//                            counts, the columns beyond a sequence's count left out of the loss and zeroed in dlogit
//   mvn_adamw_step           torch.optim.AdamW / Adam over ONE flat parameter / gradient /
//                            moment buffer (pytorch_lightning_trainer.py:186-189)
//   mvn_adamw_ema_step       the same step, with an exponential moving average of the parameters
//                            updated in the same launch
//
// The arithmetic of the first two is that of softmax_cols_kernel (sequence.hip) followed by
// ce_probs_cols_kernel (common.hip), operation for operation: the fused forms return the same
// bits as the two-kernel forms (one exponential for all of them: common.h sm_exp; one division per column).
#include "common.h"

namespace mvn {

constexpr int TQ = 64;  // class rows per wave = registers per thread (Q <= 256)

__device__ __forceinline__ float t_col_reduce(float v, float (*part)[64], int wave, int lane, bool is_max) {
  part[wave][lane] = v;
  __syncthreads();
  const float a = part[0][lane], b = part[1][lane], c = part[2][lane], d = part[3][lane];
  __syncthreads();
  return is_max ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : (a + b) + (c + d);
}

// 64 columns per workgroup, wave w holds class rows [64w, 64w+64) of them, lane = column (r4c: raw-buffer column accesses and
// ONE division per column -- common.h col_ld / sm_exp -- 4100 -> ~1900 vector instructions per wave, four waves per SIMD
// instead of two)
// MODEL (MVN_LOSS_MODEL): the loss is the column's own -log p_target = (m + log sum) - l_target, from the max and the
// exp-sum above: the target's logit is picked up as the column is loaded, and the second log-softmax (64 exponentials
// and two reductions per thread) is not formed.  Probabilities and accuracy: the same instructions under both rules.
// MASK (the _len entry points): sequence b counts its columns s < valid[b] only, valid[b] clamped to [0, S].  The
// forward forms and stores every column's probabilities as without it and SELECTS the other columns out of the two
// sums, so that a NaN or an infinity in them adds exactly 0; the backward zeroes them as it zeroes [S, s_cols).
// MASK = false never reads `valid`: those instantiations are the kernels they were.
__device__ __forceinline__ int valid_cols(const int32_t *__restrict__ valid, int b, int S) {
  return min(max(valid[b], 0), S);
}

template <bool MODEL, bool MASK>
__device__ __forceinline__ void softmax_ce_fwd_cols(float *__restrict__ y, const long long *__restrict__ target, int Q,
                                                    int S, float *__restrict__ loss_part,
                                                    int32_t *__restrict__ correct_part,
                                                    const int32_t *__restrict__ valid) {
  __shared__ float part[4][64];
  __shared__ int argp[4][64];
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = blockIdx.x * 64 + lane;
  const bool live = s < S;
  const __amdgpu_buffer_rsrc_t yb = col_rsrc(y + (size_t)b * Q * S);
  const int voff = 4 * (live ? s : 0), row = 4 * S;
  const long long tg = live ? target[(size_t)b * S + s] : 0;
  const int tq = (int)min(max(tg, 0LL), (long long)(Q - 1));
  float v[TQ];
  float m = -INFINITY, pt = 0.f;  // pt: the target's probability (REFERENCE) or its raw logit (MODEL)
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    const int q = TQ * wave + i;
    v[i] = q < Q ? col_ld(yb, voff, q * row) : -INFINITY;
    v[i] = live ? v[i] : -INFINITY;
    if (MODEL && q == tq) pt = v[i];
    m = fmaxf(m, v[i]);
  }
  m = t_col_reduce(m, part, wave, lane, true);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    v[i] = sm_exp(v[i] - m);  // exp(-inf) = 0 for the padding rows
    sum += v[i];
  }
  sum = t_col_reduce(sum, part, wave, lane, false);
  const float inv = 1.0f / sum;
  // probabilities (wavenet.py:189-191), then (REFERENCE) cross_entropy ON them: a second log-softmax
  float m2 = -INFINITY;
  int arg = 0;
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    const int q = TQ * wave + i;
    if (q < Q) {
      v[i] = v[i] * inv;
      if (live) col_st(v[i], yb, voff, q * row);
      if (v[i] > m2) {  // strict: first maximum inside this wave's rows
        m2 = v[i];
        arg = q;
      }
      if (!MODEL && q == tq) pt = v[i];
    } else {
      v[i] = -INFINITY;
    }
  }
  const float wave_m2 = m2;
  m2 = t_col_reduce(m2, part, wave, lane, true);
  float sum2 = 0.f;
  if (!MODEL) {
#pragma unroll
    for (int i = 0; i < TQ; ++i) sum2 += sm_exp(v[i] - m2);
    sum2 = t_col_reduce(sum2, part, wave, lane, false);
  }
  argp[wave][lane] = wave_m2 == m2 ? arg : 0x7fffffff;
  const float pt_all = t_col_reduce(pt, part, wave, lane, false);  // one wave holds it, the others 0
  float loss = 0.f;
  int ok = 0;
  if (wave == 0 && live) {
    const int a0 = min(min(argp[0][lane], argp[1][lane]), min(argp[2][lane], argp[3][lane]));
    loss = MODEL ? (m + logf(sum)) - pt_all : (m2 + logf(sum2)) - pt_all;
    ok = a0 == tq;
    if (MASK) {
      const bool counted = s < valid_cols(valid, b, S);
      loss = counted ? loss : 0.f;
      ok = counted ? ok : 0;
    }
  }
  if (wave == 0) {
    loss = wave_sum(loss);
    const float okf = wave_sum((float)ok);
    if (lane == 0) {
      const int wg = blockIdx.y * gridDim.x + blockIdx.x;
      loss_part[wg] = loss;
      correct_part[wg] = (int)okf;
    }
  }
}

__global__ __launch_bounds__(256) void softmax_ce_fwd_cols_kernel(float *__restrict__ y,
                                                                  const long long *__restrict__ target,
                                                                  int Q, int S, float *__restrict__ loss_part,
                                                                  int32_t *__restrict__ correct_part) {
  softmax_ce_fwd_cols<false, false>(y, target, Q, S, loss_part, correct_part, nullptr);
}

// (with fewer uses of the column to order its work by, the compiler kept loads and exponentials of the whole column
// live at once: 183 registers, two waves per SIMD; held to the four of the reference form)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void softmax_ce_model_fwd_cols_kernel(
    float *__restrict__ y, const long long *__restrict__ target, int Q, int S, float *__restrict__ loss_part,
    int32_t *__restrict__ correct_part) {
  softmax_ce_fwd_cols<true, false>(y, target, Q, S, loss_part, correct_part, nullptr);
}

// The masked twins, under the bounds of the kernels above, rule for rule (DESIGN.md 4.5 has what they compile to).
__global__ __launch_bounds__(256) void softmax_ce_fwd_cols_len_kernel(float *__restrict__ y,
                                                                      const long long *__restrict__ target, int Q,
                                                                      int S, float *__restrict__ loss_part,
                                                                      int32_t *__restrict__ correct_part,
                                                                      const int32_t *__restrict__ valid) {
  softmax_ce_fwd_cols<false, true>(y, target, Q, S, loss_part, correct_part, valid);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void softmax_ce_model_fwd_cols_len_kernel(
    float *__restrict__ y, const long long *__restrict__ target, int Q, int S, float *__restrict__ loss_part,
    int32_t *__restrict__ correct_part, const int32_t *__restrict__ valid) {
  softmax_ce_fwd_cols<true, true>(y, target, Q, S, loss_part, correct_part, valid);
}

// (r4c: the column's probabilities are the only array a thread keeps -- the exponentials are formed twice, the second time
// where the gradient is written, and sum_q dprobs_q p_q comes from two sums of the first pass -- so that four waves fit a
// SIMD: 248 -> ~110 registers)
// MASK: the columns that count end at valid[b] instead of S, and a workgroup that holds none of them stores its zeros
// before it reads anything.
template <bool MASK>
__device__ __forceinline__ void softmax_ce_bwd_cols(const float *__restrict__ p, const long long *__restrict__ target,
                                                    int Q, int S, float scale, const float *__restrict__ upstream,
                                                    float *__restrict__ dlogit, long long d_sb, int d_ld, int col0,
                                                    int s_cols, const int32_t *__restrict__ valid) {
  __shared__ float part[4][64], part2[4][64], part3[4][64];
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = blockIdx.x * 64 + lane;
  const int Sv = MASK ? valid_cols(valid, b, S) : S;
  if (MASK && (int)blockIdx.x * 64 >= Sv) {  // (workgroup-uniform, ahead of every barrier)
    if (s >= s_cols) return;
    const __amdgpu_buffer_rsrc_t zb = col_rsrc(dlogit + (size_t)b * d_sb);
    const int zvoff = 4 * (col0 + s), zrow = 4 * d_ld;
#pragma unroll
    for (int i = 0; i < TQ; ++i) {
      const int q = TQ * wave + i;
      if (q < Q) col_st(0.f, zb, zvoff, q * zrow);
    }
    return;
  }
  const bool live = s < Sv;
  const __amdgpu_buffer_rsrc_t pb = col_rsrc(p + (size_t)b * Q * S);
  const int voff = 4 * (live ? s : 0), row = 4 * S;
  float pv[TQ];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    const int q = TQ * wave + i;
    pv[i] = q < Q ? col_ld(pb, voff, q * row) : -INFINITY;
    pv[i] = live ? pv[i] : -INFINITY;
    m = fmaxf(m, pv[i]);
  }
  m = t_col_reduce(m, part, wave, lane, true);
  const long long tg = live ? target[(size_t)b * S + s] : 0;
  const int tq = (int)min(max(tg, 0LL), (long long)(Q - 1));
  // one pass: sum_q e_q, sum_q e_q p_q and p_target (e_q = exp(p_q - m); absent rows: e = 0, p taken as 0)
  float sum = 0.f, s2 = 0.f, pt = 0.f;
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    const int q = TQ * wave + i;
    const float e = sm_exp(pv[i] - m);
    const float pz = (live && q < Q) ? pv[i] : 0.f;
    sum += e;
    s2 += e * pz;
    pt += q == tq ? pz : 0.f;
  }
  part[wave][lane] = sum;
  part2[wave][lane] = s2;
  part3[wave][lane] = pt;
  __syncthreads();
  sum = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
  s2 = (part2[0][lane] + part2[1][lane]) + (part2[2][lane] + part2[3][lane]);
  pt = (part3[0][lane] + part3[1][lane]) + (part3[2][lane] + part3[3][lane]);
  if (upstream) scale *= *upstream;
  const float inv = 1.0f / sum;
  // dprobs_q = scale (softmax(p)_q - onehot_q); dlogit_q = p_q (dprobs_q - sum_k dprobs_k p_k)
  const float dot = scale * (s2 * inv - pt);
  if (s >= s_cols) return;
  const __amdgpu_buffer_rsrc_t db = col_rsrc(dlogit + (size_t)b * d_sb);
  const int dvoff = 4 * (col0 + s), drow = 4 * d_ld;
  float m_again = m;
  asm volatile("" : "+v"(m_again));  // (or the first pass's 64 exponentials stay in registers for this one)
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    const int q = TQ * wave + i;
    if (q < Q) {
      const float e = sm_exp(pv[i] - m_again);
      const float g = scale * (e * inv - (q == tq ? 1.0f : 0.0f));
      col_st(live ? pv[i] * (g - dot) : 0.f, db, dvoff, q * drow);
    }
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void softmax_ce_bwd_cols_kernel(const float *__restrict__ p,
                                                                  const long long *__restrict__ target,
                                                                  int Q, int S, float scale,
                                                                  const float *__restrict__ upstream,
                                                                  float *__restrict__ dlogit, long long d_sb,
                                                                  int d_ld, int col0, int s_cols) {
  softmax_ce_bwd_cols<false>(p, target, Q, S, scale, upstream, dlogit, d_sb, d_ld, col0, s_cols, nullptr);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void softmax_ce_bwd_cols_len_kernel(
    const float *__restrict__ p, const long long *__restrict__ target, int Q, int S, float scale,
    const float *__restrict__ upstream, float *__restrict__ dlogit, long long d_sb, int d_ld, int col0, int s_cols,
    const int32_t *__restrict__ valid) {
  softmax_ce_bwd_cols<true>(p, target, Q, S, scale, upstream, dlogit, d_sb, d_ld, col0, s_cols, valid);
}

// any Q: one thread per column, the column walked several times (slow path)
template <bool MODEL, bool MASK>
__device__ __forceinline__ void softmax_ce_fwd_wide(float *__restrict__ y, const long long *__restrict__ target, int Q,
                                                    int S, float *__restrict__ loss_part,
                                                    int32_t *__restrict__ correct_part,
                                                    const int32_t *__restrict__ valid, const int s) {
  const int b = blockIdx.y;
  float loss = 0.f;
  int ok = 0;
  if (s < S) {
    float *col = y + (size_t)b * Q * S + s;
    const long long tg = target[(size_t)b * S + s];
    const int tq = (int)min(max(tg, 0LL), (long long)(Q - 1));
    const float lt = MODEL ? col[(size_t)tq * S] : 0.f;  // the target's logit, before the column is overwritten
    float m = -INFINITY;
    for (int q = 0; q < Q; ++q) m = fmaxf(m, col[(size_t)q * S]);
    float sum = 0.f;
    for (int q = 0; q < Q; ++q) {
      const float ev = sm_exp(col[(size_t)q * S] - m);
      col[(size_t)q * S] = ev;
      sum += ev;
    }
    float m2 = -INFINITY;
    int arg = 0;
    const float inv = 1.0f / sum;
    for (int q = 0; q < Q; ++q) {
      const float pq = col[(size_t)q * S] * inv;
      col[(size_t)q * S] = pq;
      if (pq > m2) {
        m2 = pq;
        arg = q;
      }
    }
    if (MODEL) {
      loss = (m + logf(sum)) - lt;
    } else {
      float sum2 = 0.f;
      for (int q = 0; q < Q; ++q) sum2 += sm_exp(col[(size_t)q * S] - m2);
      loss = (m2 + logf(sum2)) - col[(size_t)tq * S];
    }
    ok = arg == tq;
    if (MASK) {
      const bool counted = s < valid_cols(valid, b, S);
      loss = counted ? loss : 0.f;
      ok = counted ? ok : 0;
    }
  }
  __shared__ float ls[4];
  __shared__ int cs[4];
  loss = wave_sum(loss);
  const float okf = wave_sum((float)ok);
  if ((threadIdx.x & 63) == 0) {
    ls[threadIdx.x >> 6] = loss;
    cs[threadIdx.x >> 6] = (int)okf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int wg = blockIdx.y * gridDim.x + blockIdx.x;
    loss_part[wg] = (ls[0] + ls[1]) + (ls[2] + ls[3]);
    correct_part[wg] = (cs[0] + cs[1]) + (cs[2] + cs[3]);
  }
}

template <bool MODEL>
__global__ __launch_bounds__(256) void softmax_ce_fwd_kernel(float *__restrict__ y,
                                                             const long long *__restrict__ target, int Q, int S,
                                                             float *__restrict__ loss_part,
                                                             int32_t *__restrict__ correct_part) {
  softmax_ce_fwd_wide<MODEL, false>(y, target, Q, S, loss_part, correct_part, nullptr,
                                    blockIdx.x * blockDim.x + threadIdx.x);
}

template <bool MODEL>
__global__ __launch_bounds__(256) void softmax_ce_fwd_len_kernel(float *__restrict__ y,
                                                                 const long long *__restrict__ target, int Q, int S,
                                                                 float *__restrict__ loss_part,
                                                                 int32_t *__restrict__ correct_part,
                                                                 const int32_t *__restrict__ valid) {
  softmax_ce_fwd_wide<MODEL, true>(y, target, Q, S, loss_part, correct_part, valid,
                                   blockIdx.x * blockDim.x + threadIdx.x);
}

// (MASK: a thread at or beyond valid[b] takes the zeroing branch of the columns [S, s_cols) and reads no probability)
template <bool MASK>
__device__ __forceinline__ void softmax_ce_bwd_wide(const float *__restrict__ p, const long long *__restrict__ target,
                                                    int Q, int S, float scale, const float *__restrict__ upstream,
                                                    float *__restrict__ dlogit, long long d_sb, int d_ld, int col0,
                                                    int s_cols, const int32_t *__restrict__ valid, const int s) {
  const int b = blockIdx.y;
  if (s >= s_cols) return;
  float *dcol = dlogit + (size_t)b * d_sb + col0 + s;
  if (s >= (MASK ? valid_cols(valid, b, S) : S)) {
    for (int q = 0; q < Q; ++q) dcol[(size_t)q * d_ld] = 0.f;
    return;
  }
  if (upstream) scale *= *upstream;
  const float *col = p + (size_t)b * Q * S + s;
  float m = -INFINITY;
  for (int q = 0; q < Q; ++q) m = fmaxf(m, col[(size_t)q * S]);
  float sum = 0.f;
  for (int q = 0; q < Q; ++q) sum += sm_exp(col[(size_t)q * S] - m);
  const float inv = 1.0f / sum;
  const long long tg = target[(size_t)b * S + s];
  const int tq = (int)min(max(tg, 0LL), (long long)(Q - 1));
  float dot = 0.f;
  for (int q = 0; q < Q; ++q) {
    const float pq = col[(size_t)q * S];
    dot += scale * (sm_exp(pq - m) * inv - (q == tq ? 1.0f : 0.0f)) * pq;
  }
  for (int q = 0; q < Q; ++q) {
    const float pq = col[(size_t)q * S];
    dcol[(size_t)q * d_ld] = pq * (scale * (sm_exp(pq - m) * inv - (q == tq ? 1.0f : 0.0f)) - dot);
  }
}

__global__ __launch_bounds__(256) void softmax_ce_bwd_kernel(const float *__restrict__ p,
                                                             const long long *__restrict__ target, int Q, int S,
                                                             float scale, const float *__restrict__ upstream,
                                                             float *__restrict__ dlogit, long long d_sb, int d_ld,
                                                             int col0, int s_cols) {
  softmax_ce_bwd_wide<false>(p, target, Q, S, scale, upstream, dlogit, d_sb, d_ld, col0, s_cols, nullptr,
                             blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void softmax_ce_bwd_len_kernel(const float *__restrict__ p,
                                                                 const long long *__restrict__ target, int Q, int S,
                                                                 float scale, const float *__restrict__ upstream,
                                                                 float *__restrict__ dlogit, long long d_sb, int d_ld,
                                                                 int col0, int s_cols,
                                                                 const int32_t *__restrict__ valid) {
  softmax_ce_bwd_wide<true>(p, target, Q, S, scale, upstream, dlogit, d_sb, d_ld, col0, s_cols, valid,
                            blockIdx.x * blockDim.x + threadIdx.x);
}

// MODEL rule (MVN_LOSS_MODEL): dlogit = scale upstream (p - onehot(target)) -- no exponential, no sum over the column, so
// nothing of the column forms above is kept (no 64-register column, no LDS): a streaming kernel, one read of the
// probabilities and one write of the window.  A thread owns FOUR consecutive columns of the dlogit tensor, counted
// from the ROW's start (so that its 16-byte store is aligned whenever the rows are: mvn_backward's (B, Q, Sp) tensor,
// whatever dlogit_col0), and walks MB_ROWS class rows with them: the four targets are read once per thread, each row
// is one 16-byte load and one 16-byte store.  The probabilities' four columns sit dlogit_col0 elements off that grid:
// their type carries the 4-byte alignment they have, and so does the store's (gfx950 serves either with one
// instruction).  64-bit addresses throughout: any Q, any row length -- the one kernel serves the shapes of both
// column forms.  Groups that straddle an edge of the window take the element-wise tail below.
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
constexpr int MB_ROWS = 16;

// MASK: the columns that count end at Sv = valid[b] instead of S.  A group that lies whole inside [Sv, s_cols) stores
// 16 bytes of zeros per row and reads nothing; one that straddles Sv takes the element-wise tail, like one at S.
template <bool MASK>
__device__ __forceinline__ void ce_model_bwd(const float *__restrict__ p, const long long *__restrict__ target, int Q,
                                             int S, float scale, const float *__restrict__ upstream,
                                             float *__restrict__ dlogit, long long d_sb, int d_ld, int col0,
                                             int s_cols, const int32_t *__restrict__ valid) {
  const int b = blockIdx.z, q0 = blockIdx.y * MB_ROWS;
  // first column of the thread's group in the dlogit row, and the window position it maps to (may be negative)
  const long long a0 = 4LL * ((long long)(col0 >> 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x);
  const long long s0 = a0 - col0;
  if (s0 >= s_cols || s0 + 3 < 0) return;
  const int Sv = MASK ? valid_cols(valid, b, S) : S;
  if (upstream) scale *= *upstream;
  const bool whole = s0 >= 0 && s0 + 3 < Sv;  // the whole group inside [0, Sv)
  const long long *trow = target + ((long long)b * S + s0);
  int tq[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long tg = (whole || (s0 + e >= 0 && s0 + e < Sv)) ? trow[e] : 0;
    tq[e] = (int)min(max(tg, 0LL), (long long)(Q - 1));
  }
  const float *prow = p + ((long long)b * Q * S + s0);  // (dereferenced only where 0 <= s < S)
  float *drow = dlogit + ((long long)b * d_sb + a0);
  const int q1 = min(Q, q0 + MB_ROWS);
  if (MASK && s0 >= Sv && s0 + 3 < s_cols) {  // (s0 >= Sv >= 0) nothing here counts
    const f4u zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int q = q0; q < q1; ++q) *(f4u *)(drow + (size_t)q * d_ld) = zero;
    return;
  }
  if (whole) {  // one load, one store per row
#pragma unroll 4
    for (int q = q0; q < q1; ++q) {
      const f4u pv = *(const f4u *)(prow + (size_t)q * S);
      f4u g;
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = scale * (pv[e] - (q == tq[e] ? 1.0f : 0.0f));
      *(f4u *)(drow + (size_t)q * d_ld) = g;
    }
    return;
  }
  for (int q = q0; q < q1; ++q) {  // an edge of the window: element by element; [Sv, s_cols) is zeroed
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long s = s0 + e;
      if (s < 0 || s >= s_cols) continue;
      const float g = s < Sv ? scale * (prow[(size_t)q * S + e] - (q == tq[e] ? 1.0f : 0.0f)) : 0.f;
      drow[(size_t)q * d_ld + e] = g;
    }
  }
}

__global__ __launch_bounds__(256) void ce_model_bwd_kernel(const float *__restrict__ p,
                                                           const long long *__restrict__ target, int Q, int S,
                                                           float scale, const float *__restrict__ upstream,
                                                           float *__restrict__ dlogit, long long d_sb, int d_ld,
                                                           int col0, int s_cols) {
  ce_model_bwd<false>(p, target, Q, S, scale, upstream, dlogit, d_sb, d_ld, col0, s_cols, nullptr);
}

__global__ __launch_bounds__(256) void ce_model_bwd_len_kernel(const float *__restrict__ p,
                                                               const long long *__restrict__ target, int Q, int S,
                                                               float scale, const float *__restrict__ upstream,
                                                               float *__restrict__ dlogit, long long d_sb, int d_ld,
                                                               int col0, int s_cols,
                                                               const int32_t *__restrict__ valid) {
  ce_model_bwd<true>(p, target, Q, S, scale, upstream, dlogit, d_sb, d_ld, col0, s_cols, valid);
}

// ---- AdamW / Adam over a flat buffer ------------------------------------------------------
// torch.optim.AdamW's arithmetic (its _single_tensor_adam, no amsgrad, no maximize):
//   p *= 1 - lr wd  (decoupled)  |  g += wd p  (Adam's L2 form)
//   m = m + (g - m)(1 - b1);  v = b2 v + (1 - b2) g g
//   p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// Elements inside one of the (up to 4) skip ranges are left alone: parameters that received
// no gradient this step (torch skips them too: no decay, no moment update).
struct AdamSkip {
  unsigned long long lo[4], hi[4];
  int n;
};
__global__ __launch_bounds__(256) void adamw_flat_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                         float *__restrict__ m, float *__restrict__ v,
                                                         unsigned long long n, float lr, float beta1,
                                                         float beta2, float eps, float wd, float bc1,
                                                         float bc2_sqrt, int decoupled, AdamSkip skip) {
  const unsigned long long i0 = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= n) return;
  const float step_size = lr / bc1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned long long i = i0 + e;
    if (i >= n) return;
    bool skipped = false;
    for (int k = 0; k < skip.n; ++k) skipped = skipped || (i >= skip.lo[k] && i < skip.hi[k]);
    if (skipped) continue;
    float pv = p[i], gv = g[i];
    if (decoupled)
      pv = pv * (1.0f - lr * wd);
    else
      gv = gv + wd * pv;
    const float mv = m[i] + (gv - m[i]) * (1.0f - beta1);
    const float vv = beta2 * v[i] + (1.0f - beta2) * gv * gv;
    m[i] = mv;
    v[i] = vv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    p[i] = pv - step_size * (mv / denom);
  }
}

// The same step with an exponential moving average of the parameters kept behind it (mvn_adamw_ema_step): p, m and v
// by adamw_flat_kernel's expressions, one for one (same inputs, same bits), then
//   ema = ema + (p_new - ema) w        w = 1 - decay_t, from the host
// on the value p was just given, while it is still in a register: one more read and write per element, no second pass.
// A skipped element's average is left alone with its parameter.
__global__ __launch_bounds__(256) void adamw_ema_flat_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                             float *__restrict__ m, float *__restrict__ v,
                                                             float *__restrict__ ema, unsigned long long n, float lr,
                                                             float beta1, float beta2, float eps, float wd, float bc1,
                                                             float bc2_sqrt, int decoupled, float ema_w,
                                                             AdamSkip skip) {
  const unsigned long long i0 = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= n) return;
  const float step_size = lr / bc1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned long long i = i0 + e;
    if (i >= n) return;
    bool skipped = false;
    for (int k = 0; k < skip.n; ++k) skipped = skipped || (i >= skip.lo[k] && i < skip.hi[k]);
    if (skipped) continue;
    float pv = p[i], gv = g[i];
    if (decoupled)
      pv = pv * (1.0f - lr * wd);
    else
      gv = gv + wd * pv;
    const float mv = m[i] + (gv - m[i]) * (1.0f - beta1);
    const float vv = beta2 * v[i] + (1.0f - beta2) * gv * gv;
    m[i] = mv;
    v[i] = vv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    const float pn = pv - step_size * (mv / denom);
    p[i] = pn;
    const float ev = ema[i];
    ema[i] = ev + (pn - ev) * ema_w;
  }
}

}  // namespace mvn

extern "C" {

// (the plain entry points, their _ex and their _len forms share these: `what` is the name the caller's error text
// carries; `valid` == NULL launches the unmasked kernels)
static int softmax_ce_forward_impl(const char *what, float *logits_probs, const long long *target, int batch,
                                   int classes, int s_len, float *loss_part, int32_t *correct_part, int loss_rule,
                                   const int32_t *valid, void *stream) {
  if (!logits_probs || !target || !loss_part || !correct_part || batch < 0 || classes < 2 || s_len < 0) {
    mvn::set_error("%s: bad argument", what);
    return MVN_ERR_BAD_ARG;
  }
  if (loss_rule != MVN_LOSS_REFERENCE && loss_rule != MVN_LOSS_MODEL) {
    mvn::set_error("%s: bad argument (loss_rule %d is neither MVN_LOSS_REFERENCE nor MVN_LOSS_MODEL)", what, loss_rule);
    return MVN_ERR_BAD_ARG;
  }
  if (batch == 0 || s_len == 0) return MVN_OK;
  const bool model = loss_rule == MVN_LOSS_MODEL;
  // (the column form addresses a sequence's (Q, S) tensor with 32-bit offsets: common.h rows_fit_rsrc)
  const bool cols = classes <= 4 * mvn::TQ && mvn::rows_fit_rsrc(classes, s_len);
  const dim3 grid(cols ? (s_len + 63) / 64 : (s_len + 255) / 256, batch);
  if (valid) {
    const auto kernel = cols ? (model ? mvn::softmax_ce_model_fwd_cols_len_kernel : mvn::softmax_ce_fwd_cols_len_kernel)
                             : (model ? mvn::softmax_ce_fwd_len_kernel<true> : mvn::softmax_ce_fwd_len_kernel<false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, logits_probs, target, classes, s_len,
                       loss_part, correct_part, valid);
  } else {
    const auto kernel = cols ? (model ? mvn::softmax_ce_model_fwd_cols_kernel : mvn::softmax_ce_fwd_cols_kernel)
                             : (model ? mvn::softmax_ce_fwd_kernel<true> : mvn::softmax_ce_fwd_kernel<false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, logits_probs, target, classes, s_len,
                       loss_part, correct_part);
  }
  return mvn::check_hip(hipGetLastError(), what);
}

static int softmax_ce_backward_impl(const char *what, const float *probs, const long long *target, int batch,
                                    int classes, int s_len, float scale, const float *upstream, float *dlogit,
                                    long long dlogit_batch_stride, int dlogit_ld, int dlogit_col0, int dlogit_cols,
                                    int loss_rule, const int32_t *valid, void *stream) {
  if (!probs || !target || !dlogit || batch < 0 || classes < 2 || s_len < 0 || dlogit_cols < s_len ||
      dlogit_col0 < 0 || dlogit_ld < dlogit_col0 + dlogit_cols) {
    mvn::set_error("%s: bad argument", what);
    return MVN_ERR_BAD_ARG;
  }
  if (loss_rule != MVN_LOSS_REFERENCE && loss_rule != MVN_LOSS_MODEL) {
    mvn::set_error("%s: bad argument (loss_rule %d is neither MVN_LOSS_REFERENCE nor MVN_LOSS_MODEL)", what, loss_rule);
    return MVN_ERR_BAD_ARG;
  }
  if (batch == 0 || dlogit_cols == 0) return MVN_OK;
  if (loss_rule == MVN_LOSS_MODEL) {
    // groups of four dlogit columns from the row's start: those that overlap the window [col0, col0 + cols)
    const long long groups = ((long long)dlogit_col0 + dlogit_cols + 3) / 4 - dlogit_col0 / 4;
    const long long rows = (classes + mvn::MB_ROWS - 1) / mvn::MB_ROWS;
    if (rows > 65535 || batch > 65535) {
      mvn::set_error("%s: more than 65535 x %d classes or 65535 sequences", what, mvn::MB_ROWS);
      return MVN_ERR_BAD_ARG;
    }
    const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)rows, batch);
    if (valid)
      hipLaunchKernelGGL(mvn::ce_model_bwd_len_kernel, grid, dim3(256), 0, (hipStream_t)stream, probs, target,
                         classes, s_len, scale, upstream, dlogit, dlogit_batch_stride, dlogit_ld, dlogit_col0,
                         dlogit_cols, valid);
    else
      hipLaunchKernelGGL(mvn::ce_model_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, probs, target, classes,
                         s_len, scale, upstream, dlogit, dlogit_batch_stride, dlogit_ld, dlogit_col0, dlogit_cols);
  } else if (classes <= 4 * mvn::TQ && mvn::rows_fit_rsrc(classes, s_len) && mvn::rows_fit_rsrc(classes, dlogit_ld)) {
    const dim3 grid((dlogit_cols + 63) / 64, batch);
    if (valid)
      hipLaunchKernelGGL(mvn::softmax_ce_bwd_cols_len_kernel, grid, dim3(256), 0, (hipStream_t)stream, probs, target,
                         classes, s_len, scale, upstream, dlogit, dlogit_batch_stride, dlogit_ld, dlogit_col0,
                         dlogit_cols, valid);
    else
      hipLaunchKernelGGL(mvn::softmax_ce_bwd_cols_kernel, grid, dim3(256), 0, (hipStream_t)stream, probs, target,
                         classes, s_len, scale, upstream, dlogit, dlogit_batch_stride, dlogit_ld, dlogit_col0,
                         dlogit_cols);
  } else {
    const dim3 grid((dlogit_cols + 255) / 256, batch);
    if (valid)
      hipLaunchKernelGGL(mvn::softmax_ce_bwd_len_kernel, grid, dim3(256), 0, (hipStream_t)stream, probs, target,
                         classes, s_len, scale, upstream, dlogit, dlogit_batch_stride, dlogit_ld, dlogit_col0,
                         dlogit_cols, valid);
    else
      hipLaunchKernelGGL(mvn::softmax_ce_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, probs, target, classes,
                         s_len, scale, upstream, dlogit, dlogit_batch_stride, dlogit_ld, dlogit_col0, dlogit_cols);
  }
  return mvn::check_hip(hipGetLastError(), what);
}

int mvn_softmax_ce_forward(float *logits_probs, const long long *target, int batch, int classes, int s_len,
                           float *loss_part, int32_t *correct_part, void *stream) {
  return softmax_ce_forward_impl("mvn_softmax_ce_forward", logits_probs, target, batch, classes, s_len, loss_part,
                                 correct_part, MVN_LOSS_REFERENCE, nullptr, stream);
}

int mvn_softmax_ce_forward_ex(float *logits_probs, const long long *target, int batch, int classes, int s_len,
                              float *loss_part, int32_t *correct_part, int loss_rule, void *stream) {
  return softmax_ce_forward_impl("mvn_softmax_ce_forward_ex", logits_probs, target, batch, classes, s_len,
                                 loss_part, correct_part, loss_rule, nullptr, stream);
}

int mvn_softmax_ce_forward_len(float *logits_probs, const long long *target, int batch, int classes, int s_len,
                               float *loss_part, int32_t *correct_part, int loss_rule, const int32_t *valid,
                               void *stream) {
  return softmax_ce_forward_impl("mvn_softmax_ce_forward_len", logits_probs, target, batch, classes, s_len,
                                 loss_part, correct_part, loss_rule, valid, stream);
}

int mvn_softmax_ce_backward(const float *probs, const long long *target, int batch, int classes, int s_len,
                            float scale, const float *upstream, float *dlogit, long long dlogit_batch_stride,
                            int dlogit_ld, int dlogit_col0, int dlogit_cols, void *stream) {
  return softmax_ce_backward_impl("mvn_softmax_ce_backward", probs, target, batch, classes, s_len, scale, upstream,
                                  dlogit, dlogit_batch_stride, dlogit_ld, dlogit_col0, dlogit_cols,
                                  MVN_LOSS_REFERENCE, nullptr, stream);
}

int mvn_softmax_ce_backward_ex(const float *probs, const long long *target, int batch, int classes, int s_len,
                               float scale, const float *upstream, float *dlogit, long long dlogit_batch_stride,
                               int dlogit_ld, int dlogit_col0, int dlogit_cols, int loss_rule, void *stream) {
  return softmax_ce_backward_impl("mvn_softmax_ce_backward_ex", probs, target, batch, classes, s_len, scale,
                                  upstream, dlogit, dlogit_batch_stride, dlogit_ld, dlogit_col0, dlogit_cols,
                                  loss_rule, nullptr, stream);
}

int mvn_softmax_ce_backward_len(const float *probs, const long long *target, int batch, int classes, int s_len,
                                float scale, const float *upstream, float *dlogit, long long dlogit_batch_stride,
                                int dlogit_ld, int dlogit_col0, int dlogit_cols, int loss_rule, const int32_t *valid,
                                void *stream) {
  return softmax_ce_backward_impl("mvn_softmax_ce_backward_len", probs, target, batch, classes, s_len, scale,
                                  upstream, dlogit, dlogit_batch_stride, dlogit_ld, dlogit_col0, dlogit_cols,
                                  loss_rule, valid, stream);
}

int mvn_adamw_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, int decoupled,
                   const size_t *skip_ranges, int n_skip, void *stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || step < 1 || n_skip < 0 || n_skip > 4 ||
      (n_skip > 0 && !skip_ranges)) {
    mvn::set_error("mvn_adamw_step: bad argument (step >= 1, at most 4 skip ranges)");
    return MVN_ERR_BAD_ARG;
  }
  if (n == 0) return MVN_OK;
  mvn::AdamSkip sk;
  sk.n = n_skip;
  for (int k = 0; k < 4; ++k) {
    sk.lo[k] = k < n_skip ? skip_ranges[2 * k] : 0;
    sk.hi[k] = k < n_skip ? skip_ranges[2 * k + 1] : 0;
  }
  // bias corrections in double on the host, like torch (python floats)
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  const size_t threads = (n + 3) / 4;
  hipLaunchKernelGGL(mvn::adamw_flat_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, (unsigned long long)n, lr, beta1,
                     beta2, eps, weight_decay, bc1, bc2_sqrt, decoupled, sk);
  return mvn::check_hip(hipGetLastError(), "mvn_adamw_step");
}

int mvn_adamw_ema_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *ema, size_t n,
                       float lr, float beta1, float beta2, float eps, float weight_decay, int step, int decoupled,
                       float ema_weight, const size_t *skip_ranges, int n_skip, void *stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !ema || step < 1 || n_skip < 0 || n_skip > 4 ||
      (n_skip > 0 && !skip_ranges)) {
    mvn::set_error("mvn_adamw_ema_step: bad argument (ema set, step >= 1, at most 4 skip ranges)");
    return MVN_ERR_BAD_ARG;
  }
  if (!(ema_weight > 0.f && ema_weight <= 1.f)) {  // (NaN fails both comparisons)
    mvn::set_error("mvn_adamw_ema_step: bad argument (ema_weight %g lies outside (0, 1])", (double)ema_weight);
    return MVN_ERR_BAD_ARG;
  }
  if (n == 0) return MVN_OK;
  mvn::AdamSkip sk;
  sk.n = n_skip;
  for (int k = 0; k < 4; ++k) {
    sk.lo[k] = k < n_skip ? skip_ranges[2 * k] : 0;
    sk.hi[k] = k < n_skip ? skip_ranges[2 * k + 1] : 0;
  }
  // bias corrections as mvn_adamw_step forms them
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  const size_t threads = (n + 3) / 4;
  hipLaunchKernelGGL(mvn::adamw_ema_flat_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, ema, (unsigned long long)n, lr, beta1,
                     beta2, eps, weight_decay, bc1, bc2_sqrt, decoupled, ema_weight, sk);
  return mvn::check_hip(hipGetLastError(), "mvn_adamw_ema_step");
}

}  // extern "C"
