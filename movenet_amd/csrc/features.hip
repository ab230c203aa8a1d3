// Local conditioning on acoustic feature frames: the log-mel front end and the frame up-sampler.
//
//   lm_decode_kernel   class indices -> the waveform mu_law_decode_kernel gives (0 for an index outside [0, Q))
//   lm_dft_kernel      32 bins x 32 frames of |DFT|^2 per workgroup on the fp32 matrix cores: A = the twiddle rows of the
//                      tile's bins, B = the windowed frames, the N-term sum split over the four waves (and two
//                      accumulators each) and put together in a fixed order through the LDS
//   lm_mel_kernel      fbank x P, the floor and the log
//   uf_project_kernel  bias + W mel at frame rate;  uf_interp_kernel  the interpolated rows, 16 bytes per store
//   uf_dp_kernel       dP[b, c, j]: the weighted sum of the dctx columns that touch frame j (a wave per frame)
//   uf_dw_kernel       dW += dP mel^T, dbias += sum dP (a wave per word);  uf_dmel_kernel  dmel = W^T dP
//   uf_project_win_kernel, uf_dw_win_kernel, uf_dmel_win_kernel  the same three over a window of 2 k + 1 frames whose
//                      ends repeat the edge frames; uf_interp_kernel and uf_dp_kernel serve both
//   uf_window_kernel   columns [t0, t0 + n) of the generators' TIME-major context, straight from frame-rate rows and /
//                      or the label's vector: uf_interp_kernel's expression, then the vector, 16 bytes
//                      per store along the channels
//
// No atomics anywhere; every sum has one order, so two calls give the same bits.
#include "common.h"

#include <cmath>

namespace mvn {

typedef float lm_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kLmThreads = 256;  // four waves: one quarter of the N-term sum each
constexpr int kLmTile = 32;      // bins and frames per workgroup (one 32 x 32 MFMA tile)
constexpr int kLmMinFft = 32, kLmMaxFft = 2048;
constexpr int kUfThreads = 256;
constexpr int kUfSegment = 16;   // frames per workgroup of uf_dp_kernel (four per wave)
// The sizes every index and grid of this file is safe for, refused beyond (include/movenet_hip.h): a row of at most 2^30
// samples or frames, frames at most 2^24 samples apart (2 hop and j hop + hop stay far inside 32 / 64 bits), and in the
// front end at most 2^31 - 1 samples in the whole batch (the decode kernel's grid).
constexpr int kFeatMaxRow = 1 << 30, kFeatMaxHop = 1 << 24;
constexpr long long kLmMaxSamples = 0x7FFFFFFFLL;

__host__ __device__ inline int lm_frames(int T, int hop) { return T / hop + 1; }
__host__ __device__ inline int lm_frames_ld(int F) { return (F + kLmTile - 1) / kLmTile * kLmTile; }

__global__ __launch_bounds__(256) void lm_decode_kernel(const int32_t *__restrict__ q, float *__restrict__ x, size_t n,
                                                        int Q) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int v = q[i];
  const float mu = (float)(Q - 1);
  const float y = ((float)v / mu) * 2.0f - 1.0f;  // (the expression of mu_law_decode_kernel)
  const float r = copysignf((expf(fabsf(y) * log1pf(mu)) - 1.0f) / mu, y);
  x[i] = (v < 0 || v >= Q) ? 0.f : r;
}

// One k-step of the tile's product: n = the lane half's sample of the frame, m = (bin n) mod N its twiddle.
__device__ __forceinline__ void lm_step(const float *__restrict__ tw, const float *__restrict__ win,
                                        const float *__restrict__ xb, int N, int T, int bin, int n, long long t0,
                                        bool live, lm_f32x16 &re, lm_f32x16 &im) {
  const int m = (bin * n) & (N - 1);
  const long long t = t0 + n;
  const float xv = (live && t >= 0 && t < T) ? xb[t] : 0.f;
  const float bv = win[n] * xv;
  re = __builtin_amdgcn_mfma_f32_32x32x2f32(tw[m], bv, re, 0, 0, 0);
  im = __builtin_amdgcn_mfma_f32_32x32x2f32(tw[N + m], bv, im, 0, 0, 0);
}

// grid (frame tiles, bin tiles, batch).  Dynamic LDS: twiddle (2N) | window (N) | the waves' partial tiles (4 x 2 x 1024).
__global__ __launch_bounds__(kLmThreads) void lm_dft_kernel(const float *__restrict__ x, int T, int N, int hop, int F,
                                                            const float *__restrict__ window,
                                                            const float *__restrict__ twiddle, float *__restrict__ P,
                                                            int p_ld) {
  extern __shared__ float lm_lds[];
  float *tw = lm_lds, *win = lm_lds + 2 * N, *red = lm_lds + 3 * N;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  const int r = lane & 31, h = lane >> 5;
  const int bins = N / 2 + 1, b = blockIdx.z;
  const int bin0 = blockIdx.y * kLmTile, j0 = blockIdx.x * kLmTile;
  for (int i = tid; i < 2 * N; i += kLmThreads) tw[i] = twiddle[i];
  for (int i = tid; i < N; i += kLmThreads) win[i] = window[i];
  __syncthreads();

  const int bin = bin0 + r, j = j0 + r;  // this lane's row of A and column of B
  const bool live = j < F;
  const long long t0 = (long long)j * hop - N / 2;
  const float *xb = x + (size_t)b * T;
  const int quarter = N / 4, nbeg = wave * quarter;  // N >= 32: at least four k-steps per wave
  lm_f32x16 re0 = {0}, im0 = {0}, re1 = {0}, im1 = {0};
  for (int s = 0; s < quarter; s += 8) {  // (a quarter is a multiple of 8)
    lm_step(tw, win, xb, N, T, bin, nbeg + s + h, t0, live, re0, im0);
    lm_step(tw, win, xb, N, T, bin, nbeg + s + 2 + h, t0, live, re1, im1);
    lm_step(tw, win, xb, N, T, bin, nbeg + s + 4 + h, t0, live, re0, im0);
    lm_step(tw, win, xb, N, T, bin, nbeg + s + 6 + h, t0, live, re1, im1);
  }
  // C/D: column = lane & 31 (frame), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (bin)
  float *mine = red + wave * 2 * kLmTile * kLmTile;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
    mine[row * kLmTile + r] = re0[g] + re1[g];
    mine[kLmTile * kLmTile + row * kLmTile + r] = im0[g] + im1[g];
  }
  __syncthreads();
  constexpr int kTile2 = kLmTile * kLmTile;
  for (int e = tid; e < kTile2; e += kLmThreads) {
    const float re = (red[e] + red[2 * kTile2 + e]) + (red[4 * kTile2 + e] + red[6 * kTile2 + e]);
    const float im = (red[kTile2 + e] + red[3 * kTile2 + e]) + (red[5 * kTile2 + e] + red[7 * kTile2 + e]);
    const int ob = bin0 + e / kLmTile, oj = j0 + (e & (kLmTile - 1));
    if (ob < bins && oj < F) P[((size_t)b * bins + ob) * p_ld + oj] = re * re + im * im;
  }
}

// grid (ceil(F / 64), M, batch): a lane per frame, the bins in order
__global__ __launch_bounds__(kWave) void lm_mel_kernel(const float *__restrict__ P, int bins, int p_ld, int F,
                                                       const float *__restrict__ fbank, float floor, int energies,
                                                       float *__restrict__ out, int M, int mel_ld) {
  const int j = blockIdx.x * kWave + threadIdx.x, m = blockIdx.y, b = blockIdx.z;
  if (j >= F) return;
  const float *fb = fbank + (size_t)m * bins;
  const float *p = P + (size_t)b * bins * p_ld + j;
  float acc = 0.f;
#pragma unroll 8
  for (int k = 0; k < bins; ++k) acc = fmaf(fb[k], p[(size_t)k * p_ld], acc);
  out[((size_t)b * M + m) * mel_ld + j] = energies ? acc : logf(fmaxf(acc, floor));
}

// ---- the frame up-sampler ----------------------------------------------------------------------------------------
// grid (ceil(F / 64), C, batch): proj[b, c, j] = bias[c] + sum_m W[c, m] mel[b, m, j]
__global__ __launch_bounds__(kWave) void uf_project_kernel(const float *__restrict__ mel, int mel_ld,
                                                           const float *__restrict__ w, const float *__restrict__ bias,
                                                           int M, int F, int C, float *__restrict__ proj) {
  const int j = blockIdx.x * kWave + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (j >= F) return;
  const float *wr = w + (size_t)c * M;
  const float *mb = mel + (size_t)b * M * mel_ld + j;
  float acc = bias[c];
#pragma unroll 4
  for (int m = 0; m < M; ++m) acc = fmaf(wr[m], mb[(size_t)m * mel_ld], acc);
  proj[((size_t)b * C + c) * F + j] = acc;
}

__device__ __forceinline__ float uf_at(const float *__restrict__ row, int F, int hop, float rhop, long long t) {
  const int j = (int)(t / hop), j1 = min(j + 1, F - 1);
  const float a = (float)(int)(t - (long long)j * hop) * rhop;
  return fmaf(a, row[j1], (1.0f - a) * row[j]);
}

// grid (ceil(T / 1024), C, batch): four columns per thread, one 16-byte store where all four exist
__global__ __launch_bounds__(kUfThreads) void uf_interp_kernel(const float *__restrict__ proj, int F, int C, int hop,
                                                               int T, float *__restrict__ ctx, int ctx_ld) {
  const int c = blockIdx.y, b = blockIdx.z;
  const long long t = 4LL * ((long long)blockIdx.x * kUfThreads + threadIdx.x);
  if (t >= T) return;
  const float *row = proj + ((size_t)b * C + c) * F;
  float *out = ctx + ((size_t)b * C + c) * ctx_ld + t;
  const float rhop = 1.0f / (float)hop;
  if (t + 4 <= T) {
    float4 v;
    v.x = uf_at(row, F, hop, rhop, t);
    v.y = uf_at(row, F, hop, rhop, t + 1);
    v.z = uf_at(row, F, hop, rhop, t + 2);
    v.w = uf_at(row, F, hop, rhop, t + 3);
    *reinterpret_cast<float4 *>(out) = v;
  } else {
    for (int i = 0; t + i < T; ++i) out[i] = uf_at(row, F, hop, rhop, t + i);
  }
}

// grid (ceil(F / kUfSegment), C, batch).  Frame j collects (1 - a) of the columns [j hop, (j + 1) hop), a of the columns
// [(j - 1) hop, j hop) and, as the last frame, the a of its own columns as well (j1 stops at F - 1).
__global__ __launch_bounds__(kUfThreads) void uf_dp_kernel(const float *__restrict__ dctx, int dctx_ld, int F, int C,
                                                           int hop, int T, float *__restrict__ dP) {
  const int c = blockIdx.y, b = blockIdx.z;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  const float *row = dctx + ((size_t)b * C + c) * dctx_ld;
  const float rhop = 1.0f / (float)hop;
  for (int j = blockIdx.x * kUfSegment + wave; j < min(F, (int)(blockIdx.x + 1) * kUfSegment); j += kUfThreads / kWave) {
    float acc = 0.f;
    for (int i = lane; i < 2 * hop; i += kWave) {
      const bool before = i < hop;  // a column of frame j - 1
      const int o = before ? i : i - hop;
      const long long t = (long long)(before ? j - 1 : j) * hop + o;
      if (t < 0 || t >= T) continue;
      const float a = (float)o * rhop;
      const float wgt = before ? a : (j == F - 1 ? (1.0f - a) + a : 1.0f - a);
      acc = fmaf(wgt, row[t], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) dP[((size_t)b * C + c) * F + j] = acc;
  }
}

// grid (M + 1, C): a wave per word -- dW[c, m] for m < M, dbias[c] for m == M -- over the (b, j) pairs in order
__global__ __launch_bounds__(kWave) void uf_dw_kernel(const float *__restrict__ dP, const float *__restrict__ mel,
                                                      int mel_ld, int B, int M, int F, int C, float *__restrict__ dw,
                                                      float *__restrict__ dbias) {
  const int m = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
  const bool is_bias = m == M;
  if (is_bias ? dbias == nullptr : dw == nullptr) return;  // (workgroup-uniform)
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const float *d = dP + ((size_t)b * C + c) * F;
    const float *mr = mel + ((size_t)b * M + (is_bias ? 0 : m)) * mel_ld;
    for (int j = lane; j < F; j += kWave) acc = is_bias ? acc + d[j] : fmaf(d[j], mr[j], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    if (is_bias) dbias[c] += acc;
    else dw[(size_t)c * M + m] += acc;
  }
}

// grid (ceil(F / 64), M, batch): dmel[b, m, j] = sum_c W[c, m] dP[b, c, j]
__global__ __launch_bounds__(kWave) void uf_dmel_kernel(const float *__restrict__ dP, const float *__restrict__ w, int M,
                                                        int F, int C, float *__restrict__ dmel, int dmel_ld) {
  const int j = blockIdx.x * kWave + threadIdx.x, m = blockIdx.y, b = blockIdx.z;
  if (j >= F) return;
  const float *d = dP + (size_t)b * C * F + j;
  float acc = 0.f;
#pragma unroll 4
  for (int c = 0; c < C; ++c) acc = fmaf(w[(size_t)c * M + m], d[(size_t)c * F], acc);
  dmel[((size_t)b * M + m) * dmel_ld + j] = acc;
}

// ---- the frame up-sampler with a window of neighbouring frames ---------------------------------------------
// w is (C, M, taps), taps = 2 k + 1; frame j + d stands for frame cl(j + d) = min(max(j + d, 0), F - 1) of the F given.
constexpr int kUfMaxTaps = 33;

__device__ __forceinline__ int uf_cl(int i, int F) { return min(max(i, 0), F - 1); }

// grid (ceil(F / 64), C, batch): proj[b, c, j] = bias[c] + sum_m sum_d W[c, m, d + k] mel[b, m, cl(j + d)], rows
// proj_ld words apart (F in the up-sampler's scratch).  A lane per
// frame: the taps reads of a row are 64 consecutive words each (the clamped ends repeat one), the weights are
// wave-uniform; taps = 1 is uf_project_kernel's sum, term by term.
__global__ __launch_bounds__(kWave) void uf_project_win_kernel(const float *__restrict__ mel, int mel_ld,
                                                               const float *__restrict__ w,
                                                               const float *__restrict__ bias, int M, int F, int C,
                                                               int taps, float *__restrict__ proj, int proj_ld) {
  const int j = blockIdx.x * kWave + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (j >= F) return;
  const int k = taps >> 1;
  const float *wr = w + (size_t)c * M * taps;
  const float *mb = mel + (size_t)b * M * mel_ld;
  float acc = bias[c];
  for (int m = 0; m < M; ++m) {
    const float *row = mb + (size_t)m * mel_ld;
    const float *wm = wr + (size_t)m * taps;
    for (int d = -k; d <= k; ++d) acc = fmaf(wm[d + k], row[uf_cl(j + d, F)], acc);
  }
  proj[((size_t)b * C + c) * proj_ld + j] = acc;
}

// grid (M taps + 1, C): a wave per word -- dW[c, m, d + k] for x = m taps + d + k < M taps, dbias[c] for x == M taps --
// over the (b, j) pairs in order (uf_dw_kernel's order: taps = 1 gives its bits)
__global__ __launch_bounds__(kWave) void uf_dw_win_kernel(const float *__restrict__ dP, const float *__restrict__ mel,
                                                          int mel_ld, int B, int M, int F, int C, int taps,
                                                          float *__restrict__ dw, float *__restrict__ dbias) {
  const int x = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
  const bool is_bias = x == M * taps;
  if (is_bias ? dbias == nullptr : dw == nullptr) return;  // (workgroup-uniform)
  const int m = is_bias ? 0 : x / taps, d = is_bias ? 0 : x - m * taps - (taps >> 1);
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const float *dp = dP + ((size_t)b * C + c) * F;
    const float *mr = mel + ((size_t)b * M + m) * mel_ld;
    for (int j = lane; j < F; j += kWave) acc = is_bias ? acc + dp[j] : fmaf(dp[j], mr[uf_cl(j + d, F)], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    if (is_bias) dbias[c] += acc;
    else dw[(size_t)c * M * taps + x] += acc;
  }
}

// grid (ceil(F / 64), M, batch): dmel[b, m, i] = sum_c sum_d sum_{j : cl(j + d) = i} W[c, m, d + k] dP[b, c, j], a lane
// per word (gather form).  The frames j with cl(j + d) = i are [lo, hi]: i - d alone for an interior i, every j <= -d
// for i = 0 and every j >= F - 1 - d for i = F - 1 (both, i.e. every j, where F = 1), cut to [0, F - 1] -- at most
// k + 1 of them, and none where i - d falls outside.  taps = 1 is uf_dmel_kernel's sum, term by term.
__global__ __launch_bounds__(kWave) void uf_dmel_win_kernel(const float *__restrict__ dP, const float *__restrict__ w,
                                                            int M, int F, int C, int taps, float *__restrict__ dmel,
                                                            int dmel_ld) {
  const int i = blockIdx.x * kWave + threadIdx.x, m = blockIdx.y, b = blockIdx.z;
  if (i >= F) return;
  const int k = taps >> 1;
  float acc = 0.f;
  for (int c = 0; c < C; ++c) {
    const float *dp = dP + ((size_t)b * C + c) * F;
    const float *wm = w + ((size_t)c * M + m) * taps;
    for (int d = -k; d <= k; ++d) {
      const int lo = i == 0 ? 0 : max(i - d, 0), hi = i == F - 1 ? F - 1 : min(i - d, F - 1);
      const float wv = wm[d + k];
      for (int j = lo; j <= hi; ++j) acc = fmaf(wv, dp[j], acc);
    }
  }
  dmel[((size_t)b * M + m) * dmel_ld + i] = acc;
}

// ---- one window of the generators' time-major context -------------------------------------------------
// win (rows, n, C): win[r, t - t0, c] = uf_at(proj[r mod proj_rows, c, :], t) [+ glob[r, c]] for t in [t0, t0 + n) --
// the word uf_interp_kernel stores at (c, t), moved by transpose_ctx_kernel and then summed with the label's vector by
// context_add_global_kernel (row[i] + v); proj == nullptr: glob[r, c] itself (that kernel's fill).
// grid (ceil(n / tt), rows), tt columns per workgroup; a thread forms V consecutive channels of one column and stores
// them at once (V = 4: 16 bytes, a wave's stores back to back along c and then t).
constexpr int kUwPerGroup = 1024;  // stores per workgroup (four per thread)

template <int V>
__global__ __launch_bounds__(kUfThreads) void uf_window_kernel(const float *__restrict__ proj, int proj_ld,
                                                               int proj_rows, int F, const float *__restrict__ glob,
                                                               int C, int hop, int t0, int n, int tt,
                                                               float *__restrict__ win) {
  const int r = blockIdx.y, cv = C / V;
  const int tl0 = blockIdx.x * tt, cols = min(tt, n - tl0);
  const float *rows = proj ? proj + (size_t)(r % proj_rows) * C * proj_ld : nullptr;
  const float *gv = glob ? glob + (size_t)r * C : nullptr;
  float *out = win + ((size_t)r * n + tl0) * C;
  const float rhop = 1.0f / (float)hop;
  for (int e = threadIdx.x; e < cols * cv; e += kUfThreads) {
    const int tl = e / cv, c = (e - tl * cv) * V;
    const long long t = (long long)t0 + tl0 + tl;
    float v[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if (rows) {
        v[i] = uf_at(rows + (size_t)(c + i) * proj_ld, F, hop, rhop, t);
        if (gv) v[i] = v[i] + gv[c + i];
      } else {
        v[i] = gv[c + i];
      }
    }
    float *o = out + (size_t)tl * C + c;
    if constexpr (V == 4) {
      *reinterpret_cast<float4 *>(o) = float4{v[0], v[1], v[2], v[3]};
    } else {
      o[0] = v[0];
    }
  }
}

// the frame-rate product of the windowed up-sampler, for its scratch or for a caller's tensor
static int uf_launch_project(const char *stage, const float *mel, int mel_ld, const float *w, const float *bias,
                             int batch, int M, int F, int C, int taps, float *proj, int proj_ld, hipStream_t st) {
  hipLaunchKernelGGL(uf_project_win_kernel, dim3((F + kWave - 1) / kWave, C, batch), dim3(kWave), 0, st, mel, mel_ld, w,
                     bias, M, F, C, taps, proj, proj_ld);
  return check_hip(hipGetLastError(), stage);
}

static bool lm_shape_ok(int batch, int T, int N, int hop) {
  return batch >= 0 && batch <= 65535 && T >= 1 && T <= kFeatMaxRow && (long long)batch * T <= kLmMaxSamples &&
         N >= kLmMinFft && N <= kLmMaxFft && (N & (N - 1)) == 0 && hop >= 1 && hop <= N;
}

static int uf_refuse(const char *what, const char *why) {
  set_error("%s: %s", what, why);
  return MVN_ERR_BAD_ARG;
}

// what the forward and the backward of the up-sampler refuse alike; 0: fine
static int uf_check(const char *what, int batch, int M, int F, int C, int hop, int T, const float *scratch,
                    size_t scratch_floats) {
  if (batch < 0 || batch > 65535 || M < 1 || M > 65535 || F < 1 || C < 1 || C > 65535 || hop < 1 || T < 1)
    return uf_refuse(what, "bad argument (a size below 1, or batch / n_mels / channels above 65535)");
  if (F > kFeatMaxRow || T > kFeatMaxRow || hop > kFeatMaxHop)
    return uf_refuse(what, "bad argument (frames or n_samples above 2^30, or hop above 2^24)");
  if ((long long)F < ((long long)T - 1) / hop + 1) return uf_refuse(what, "too few frames for n_samples");
  if (!scratch || scratch_floats < (size_t)batch * C * F) return uf_refuse(what, "scratch missing or too small");
  return MVN_OK;
}

}  // namespace mvn

extern "C" {

size_t mvn_logmel_scratch_floats(int batch, int n_samples, int n_fft, int hop) {
  if (!mvn::lm_shape_ok(batch, n_samples, n_fft, hop) || batch < 1) return 0;
  const int F = mvn::lm_frames(n_samples, hop);
  return (size_t)batch * n_samples + (size_t)batch * (n_fft / 2 + 1) * mvn::lm_frames_ld(F);
}

int mvn_logmel_frontend(const int32_t *index, int batch, int n_samples, int classes, int n_fft, int hop, int n_mels,
                        const float *window, const float *twiddle, const float *fbank, float floor, int energies,
                        float *mel, int mel_ld, float *scratch, size_t scratch_floats, void *stream) {
  const char *what = "mvn_logmel_frontend";
  if (!index || !window || !twiddle || !fbank || !mel || !scratch) return mvn::uf_refuse(what, "bad argument (null pointer)");
  if (!mvn::lm_shape_ok(batch, n_samples, n_fft, hop))
    return mvn::uf_refuse(what, "bad argument (n_fft a power of two in [32, 2048], hop in [1, n_fft], batch in [0, 65535], "
                                "n_samples in [1, 2^30], batch * n_samples below 2^31)");
  if (n_mels < 1 || n_mels > 65535 || classes < 2 || !(floor > 0.0f))
    return mvn::uf_refuse(what, "bad argument (n_mels in [1, 65535], classes >= 2, floor > 0)");
  const int F = mvn::lm_frames(n_samples, hop), p_ld = mvn::lm_frames_ld(F), bins = n_fft / 2 + 1;
  if (mel_ld < F) return mvn::uf_refuse(what, "mel_ld is below the frame count");
  if (batch == 0) return MVN_OK;
  if (scratch_floats < mvn_logmel_scratch_floats(batch, n_samples, n_fft, hop))
    return mvn::uf_refuse(what, "scratch too small");
  hipStream_t st = (hipStream_t)stream;
  float *x = scratch, *P = scratch + (size_t)batch * n_samples;
  const size_t n = (size_t)batch * n_samples;
  hipLaunchKernelGGL(mvn::lm_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, index, x, n, classes);
  int rc = mvn::check_hip(hipGetLastError(), "logmel_frontend (decode)");
  if (rc) return rc;
  const size_t lds = (size_t)(3 * n_fft + 8 * mvn::kLmTile * mvn::kLmTile) * sizeof(float);  // at most 56 KiB
  hipLaunchKernelGGL(mvn::lm_dft_kernel, dim3(p_ld / mvn::kLmTile, (bins + mvn::kLmTile - 1) / mvn::kLmTile, batch),
                     dim3(mvn::kLmThreads), lds, st, (const float *)x, n_samples, n_fft, hop, F, window, twiddle, P, p_ld);
  rc = mvn::check_hip(hipGetLastError(), "logmel_frontend (dft)");
  if (rc) return rc;
  hipLaunchKernelGGL(mvn::lm_mel_kernel, dim3((F + mvn::kWave - 1) / mvn::kWave, n_mels, batch), dim3(mvn::kWave), 0, st,
                     (const float *)P, bins, p_ld, F, fbank, floor, energies, mel, n_mels, mel_ld);
  return mvn::check_hip(hipGetLastError(), "logmel_frontend (mel)");
}

size_t mvn_upsample_features_scratch_floats(int batch, int channels, int frames) {
  if (batch < 1 || channels < 1 || frames < 1) return 0;
  return (size_t)batch * channels * frames;
}

int mvn_upsample_features(const float *mel, int mel_ld, const float *w, const float *bias, int batch, int n_mels,
                          int frames, int channels, int hop, int n_samples, float *ctx, int ctx_ld, float *scratch,
                          size_t scratch_floats, void *stream) {
  const char *what = "mvn_upsample_features";
  if (!mel || !w || !bias || !ctx) return mvn::uf_refuse(what, "bad argument (null pointer)");
  int rc = mvn::uf_check(what, batch, n_mels, frames, channels, hop, n_samples, scratch, scratch_floats);
  if (rc) return rc;
  if (mel_ld < frames || ctx_ld < n_samples) return mvn::uf_refuse(what, "a row stride is below its row's length");
  if ((ctx_ld & 3) != 0 || ((uintptr_t)ctx & 15u) != 0)
    return mvn::uf_refuse(what, "ctx must be 16-byte aligned and ctx_ld a multiple of 4");
  if (batch == 0) return MVN_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mvn::uf_project_kernel, dim3((frames + mvn::kWave - 1) / mvn::kWave, channels, batch),
                     dim3(mvn::kWave), 0, st, mel, mel_ld, w, bias, n_mels, frames, channels, scratch);
  rc = mvn::check_hip(hipGetLastError(), "upsample_features (project)");
  if (rc) return rc;
  const int per = 4 * mvn::kUfThreads;
  hipLaunchKernelGGL(mvn::uf_interp_kernel, dim3((n_samples + per - 1) / per, channels, batch), dim3(mvn::kUfThreads), 0,
                     st, (const float *)scratch, frames, channels, hop, n_samples, ctx, ctx_ld);
  return mvn::check_hip(hipGetLastError(), "upsample_features (interpolate)");
}

int mvn_upsample_features_backward(const float *dctx, int dctx_ld, const float *mel, int mel_ld, const float *w,
                                   int batch, int n_mels, int frames, int channels, int hop, int n_samples, float *dw,
                                   float *dbias, float *dmel, int dmel_ld, float *scratch, size_t scratch_floats,
                                   void *stream) {
  const char *what = "mvn_upsample_features_backward";
  if (!dctx || !mel || !w) return mvn::uf_refuse(what, "bad argument (null pointer)");
  int rc = mvn::uf_check(what, batch, n_mels, frames, channels, hop, n_samples, scratch, scratch_floats);
  if (rc) return rc;
  if (mel_ld < frames || dctx_ld < n_samples || (dmel && dmel_ld < frames))
    return mvn::uf_refuse(what, "a row stride is below its row's length");
  if (batch == 0) return MVN_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mvn::uf_dp_kernel, dim3((frames + mvn::kUfSegment - 1) / mvn::kUfSegment, channels, batch),
                     dim3(mvn::kUfThreads), 0, st, dctx, dctx_ld, frames, channels, hop, n_samples, scratch);
  rc = mvn::check_hip(hipGetLastError(), "upsample_features_backward (dP)");
  if (rc) return rc;
  if (dw || dbias) {
    hipLaunchKernelGGL(mvn::uf_dw_kernel, dim3(n_mels + 1, channels), dim3(mvn::kWave), 0, st, (const float *)scratch,
                       mel, mel_ld, batch, n_mels, frames, channels, dw, dbias);
    rc = mvn::check_hip(hipGetLastError(), "upsample_features_backward (dW)");
    if (rc) return rc;
  }
  if (dmel) {
    hipLaunchKernelGGL(mvn::uf_dmel_kernel, dim3((frames + mvn::kWave - 1) / mvn::kWave, n_mels, batch),
                       dim3(mvn::kWave), 0, st, (const float *)scratch, w, n_mels, frames, channels, dmel, dmel_ld);
    rc = mvn::check_hip(hipGetLastError(), "upsample_features_backward (dmel)");
  }
  return rc;
}

int mvn_upsample_features_win(const float *mel, int mel_ld, const float *w, const float *bias, int batch, int n_mels,
                              int frames, int channels, int taps, int hop, int n_samples, float *ctx, int ctx_ld,
                              float *scratch, size_t scratch_floats, void *stream) {
  const char *what = "mvn_upsample_features_win";
  if (!mel || !w || !bias || !ctx) return mvn::uf_refuse(what, "bad argument (null pointer)");
  if (taps < 1 || taps > mvn::kUfMaxTaps || (taps & 1) == 0)
    return mvn::uf_refuse(what, "bad argument (taps must be odd, in [1, 33])");
  int rc = mvn::uf_check(what, batch, n_mels, frames, channels, hop, n_samples, scratch, scratch_floats);
  if (rc) return rc;
  if (mel_ld < frames || ctx_ld < n_samples) return mvn::uf_refuse(what, "a row stride is below its row's length");
  if ((ctx_ld & 3) != 0 || ((uintptr_t)ctx & 15u) != 0)
    return mvn::uf_refuse(what, "ctx must be 16-byte aligned and ctx_ld a multiple of 4");
  if (batch == 0) return MVN_OK;
  hipStream_t st = (hipStream_t)stream;
  rc = mvn::uf_launch_project("upsample_features_win (project)", mel, mel_ld, w, bias, batch, n_mels, frames, channels,
                              taps, scratch, frames, st);
  if (rc) return rc;
  const int per = 4 * mvn::kUfThreads;
  hipLaunchKernelGGL(mvn::uf_interp_kernel, dim3((n_samples + per - 1) / per, channels, batch), dim3(mvn::kUfThreads), 0,
                     st, (const float *)scratch, frames, channels, hop, n_samples, ctx, ctx_ld);
  return mvn::check_hip(hipGetLastError(), "upsample_features_win (interpolate)");
}

int mvn_upsample_features_win_backward(const float *dctx, int dctx_ld, const float *mel, int mel_ld, const float *w,
                                       int batch, int n_mels, int frames, int channels, int taps, int hop,
                                       int n_samples, float *dw, float *dbias, float *dmel, int dmel_ld,
                                       float *scratch, size_t scratch_floats, void *stream) {
  const char *what = "mvn_upsample_features_win_backward";
  if (!dctx || !mel || !w) return mvn::uf_refuse(what, "bad argument (null pointer)");
  if (taps < 1 || taps > mvn::kUfMaxTaps || (taps & 1) == 0)
    return mvn::uf_refuse(what, "bad argument (taps must be odd, in [1, 33])");
  int rc = mvn::uf_check(what, batch, n_mels, frames, channels, hop, n_samples, scratch, scratch_floats);
  if (rc) return rc;
  if (mel_ld < frames || dctx_ld < n_samples || (dmel && dmel_ld < frames))
    return mvn::uf_refuse(what, "a row stride is below its row's length");
  if (batch == 0) return MVN_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mvn::uf_dp_kernel, dim3((frames + mvn::kUfSegment - 1) / mvn::kUfSegment, channels, batch),
                     dim3(mvn::kUfThreads), 0, st, dctx, dctx_ld, frames, channels, hop, n_samples, scratch);
  rc = mvn::check_hip(hipGetLastError(), "upsample_features_win_backward (dP)");
  if (rc) return rc;
  if (dw || dbias) {
    hipLaunchKernelGGL(mvn::uf_dw_win_kernel, dim3(n_mels * taps + 1, channels), dim3(mvn::kWave), 0, st,
                       (const float *)scratch, mel, mel_ld, batch, n_mels, frames, channels, taps, dw, dbias);
    rc = mvn::check_hip(hipGetLastError(), "upsample_features_win_backward (dW)");
    if (rc) return rc;
  }
  if (dmel) {
    hipLaunchKernelGGL(mvn::uf_dmel_win_kernel, dim3((frames + mvn::kWave - 1) / mvn::kWave, n_mels, batch),
                       dim3(mvn::kWave), 0, st, (const float *)scratch, w, n_mels, frames, channels, taps, dmel,
                       dmel_ld);
    rc = mvn::check_hip(hipGetLastError(), "upsample_features_win_backward (dmel)");
  }
  return rc;
}

int mvn_project_features(const float *mel, int mel_ld, const float *w, const float *bias, int batch, int n_mels,
                         int frames, int channels, int taps, float *proj, int proj_ld, void *stream) {
  const char *what = "mvn_project_features";
  if (!mel || !w || !bias || !proj) return mvn::uf_refuse(what, "bad argument (null pointer)");
  if (taps < 1 || taps > mvn::kUfMaxTaps || (taps & 1) == 0)
    return mvn::uf_refuse(what, "bad argument (taps must be odd, in [1, 33])");
  // (the up-sampler's size checks: no hop and no samples here, and proj stands where its scratch does)
  int rc = mvn::uf_check(what, batch, n_mels, frames, channels, 1, 1, proj,
                         (size_t)(batch > 0 ? batch : 0) * (channels > 0 ? channels : 0) * (frames > 0 ? frames : 0));
  if (rc) return rc;
  if (mel_ld < frames || proj_ld < frames) return mvn::uf_refuse(what, "a row stride is below its row's length");
  if (batch == 0) return MVN_OK;
  return mvn::uf_launch_project("project_features", mel, mel_ld, w, bias, batch, n_mels, frames, channels, taps, proj,
                                proj_ld, (hipStream_t)stream);
}

int mvn_context_window(const float *proj, int proj_ld, int proj_rows, int frames, const float *glob, int rows,
                       int channels, int hop, int t0, int n, float *win, void *stream) {
  const char *what = "mvn_context_window";
  if (!win) return mvn::uf_refuse(what, "bad argument (win is NULL)");
  if (!proj && !glob) return mvn::uf_refuse(what, "bad argument (proj and glob are both NULL: nothing to write)");
  if (rows < 0 || rows > 65535 || channels < 1 || channels > 65535 || n < 1)
    return mvn::uf_refuse(what, "bad argument (a size below 1, or rows / channels above 65535)");
  if (t0 < 0) return mvn::uf_refuse(what, "bad argument (t0 is negative)");
  if (n > mvn::kFeatMaxRow || (long long)t0 + n > mvn::kFeatMaxRow)
    return mvn::uf_refuse(what, "bad argument (n, or t0 + n, above 2^30)");
  if (proj) {
    if (proj_rows < 1 || frames < 1 || hop < 1 || proj_ld < frames)
      return mvn::uf_refuse(what, "bad argument (proj_rows, frames or hop below 1, or proj_ld below frames)");
    if (frames > mvn::kFeatMaxRow || hop > mvn::kFeatMaxHop)
      return mvn::uf_refuse(what, "bad argument (frames above 2^30, or hop above 2^24)");
    if ((long long)frames < ((long long)t0 + n - 1) / hop + 1) {
      mvn::set_error("%s: too few frames for columns [%d, %lld): %d given at hop %d", what, t0, (long long)t0 + n, frames,
                     hop);
      return MVN_ERR_BAD_ARG;
    }
  }
  if (rows == 0) return MVN_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (channels & 3) == 0 && ((uintptr_t)win & 15u) == 0;
  const int cv = vec ? channels / 4 : channels;
  const int tt = cv >= mvn::kUwPerGroup ? 1 : mvn::kUwPerGroup / cv;
  const dim3 grid((unsigned)((n + tt - 1) / tt), (unsigned)rows);
  if (!proj) proj_ld = proj_rows = frames = hop = 1;  // (not read)
  if (vec)
    hipLaunchKernelGGL(mvn::uf_window_kernel<4>, grid, dim3(mvn::kUfThreads), 0, st, proj, proj_ld, proj_rows, frames, glob,
                       channels, hop, t0, n, tt, win);
  else
    hipLaunchKernelGGL(mvn::uf_window_kernel<1>, grid, dim3(mvn::kUfThreads), 0, st, proj, proj_ld, proj_rows, frames, glob,
                       channels, hop, t0, n, tt, win);
  return mvn::check_hip(hipGetLastError(), "mvn_context_window");
}

}  // extern "C"
