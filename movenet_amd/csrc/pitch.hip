// A frame-wise pitch tracker and the distance between two pitch tracks.
//
//   pt_decode_kernel    class indices -> the waveform mu_law_decode_kernel gives (0 for an index outside [0, Q)),
//                       lm_decode_kernel's expression, into the caller's scratch
//   pt_frames_kernel    YIN, one workgroup per (frame, row): the frame's L = win + tau_max samples in the LDS, the
//                       difference function d(tau) = sum_n (x[n] - x[n + tau])^2 with a lag per lane, its running sum
//                       over tau, the cumulative-mean-normalised c(tau), the pick and the parabolic refinement
//   pt_distance_kernel  F0 RMSE in cents, voicing-decision and gross errors of two period tracks, a wave per sequence
//
// No atomics anywhere; every sum has one order, so two calls give the same bits, and a frame reads nothing but its own
// L samples: a row's results do not depend on the other rows, and a non-finite sample stays inside the frames that
// cover it.
#include "common.h"

#include <cmath>

namespace mvn {

constexpr int kPtThreads = 256;              // four waves
constexpr int kPtWaves = kPtThreads / kWave;
constexpr int kPtMinWin = 16, kPtMaxWin = 4096, kPtMinLag = 2, kPtMaxLag = 1024;
constexpr int kPtPerThread = kPtMaxLag / kPtThreads;  // lags per thread of the scan and the pick (consecutive ones)
constexpr int kPtMaxRow = 1 << 30, kPtMaxHop = 1 << 24;
constexpr long long kPtMaxSamples = 0x7FFFFFFFLL;
constexpr int kPtMaxGroups = 1 << 22;        // workgroups of one launch; a workgroup walks frames beyond that
constexpr int kPtNone = 0x7FFFFFFF;          // "no lag below the threshold"

__host__ __device__ inline int pt_frames(int T, int hop) { return T / hop + 1; }

__global__ __launch_bounds__(256) void pt_decode_kernel(const int32_t *__restrict__ q, float *__restrict__ x, size_t n,
                                                        int Q) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int v = q[i];
  const float mu = (float)(Q - 1);
  const float y = ((float)v / mu) * 2.0f - 1.0f;  // (the expression of mu_law_decode_kernel)
  const float r = copysignf((expf(fabsf(y) * log1pf(mu)) - 1.0f) / mu, y);
  x[i] = (v < 0 || v >= Q) ? 0.f : r;
}

// Dynamic LDS: xs (L) | dl (kPtMaxLag + 1 words used up to tau_max: d, then c, by lag).
// grid (min(F, kPtMaxGroups / batch), batch); a workgroup takes frames blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(kPtThreads) void pt_frames_kernel(const float *__restrict__ x, int T, int win, int hop,
                                                               int tau_min, int tau_max, float threshold, int F,
                                                               float *__restrict__ period, float *__restrict__ aper,
                                                               float *__restrict__ cmnd) {
  extern __shared__ float pt_lds[];
  __shared__ float s_wave[kPtWaves];   // the waves' sums of d, then their minima of c
  __shared__ int s_tau[kPtWaves], s_first[kPtWaves];
  const int L = win + tau_max;
  float *xs = pt_lds, *dl = pt_lds + L;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  const int b = blockIdx.y;
  const float *xb = x + (size_t)b * T;

  for (int j = blockIdx.x; j < F; j += gridDim.x) {
    const long long s0 = (long long)j * hop - L / 2;
    for (int i = tid; i < L; i += kPtThreads) {
      const long long t = s0 + i;
      xs[i] = (t >= 0 && t < T) ? xb[t] : 0.f;
    }
    __syncthreads();

    // d(tau), a lag per lane: x[n] is one word for the wave (a broadcast), x[n + tau] 64 consecutive words.  A wave
    // whose lags all lie beyond tau_max skips the pass (wave-uniform).
    for (int base = wave * kWave; base < tau_max; base += kPtThreads) {
      const int tau = base + lane + 1;
      const float *xt = xs + min(tau, tau_max);  // (a lane beyond tau_max reads inside the frame and stores nothing)
      float acc = 0.f;
#pragma unroll 8
      for (int n = 0; n < win; ++n) {
        const float df = xs[n] - xt[n];
        acc = fmaf(df, df, acc);
      }
      if (tau <= tau_max) dl[tau] = acc;
    }
    __syncthreads();

    // The running sum of d over tau: a thread owns the kPtPerThread consecutive lags from t0, the threads' sums are
    // scanned inside the wave and the waves' totals added in order.
    const int t0 = tid * kPtPerThread + 1;
    float dv[kPtPerThread], run = 0.f;
#pragma unroll
    for (int i = 0; i < kPtPerThread; ++i) {
      dv[i] = t0 + i <= tau_max ? dl[t0 + i] : 0.f;
      run += dv[i];
    }
    float incl = run;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const float up = __shfl_up(incl, o, kWave);
      if (lane >= o) incl += up;
    }
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    float before = __shfl_up(incl, 1, kWave);  // the sum of the lags below t0 inside this wave ...
    if (lane == 0) before = 0.f;
    {
      float w = 0.f;
      for (int i = 0; i < wave; ++i) w += s_wave[i];
      before = w + before;  // ... and of the waves in front of it
    }
    // (dl[t0 ..] is read and written by its owner alone; s_wave is reused only after the next barrier)
    float cv[kPtPerThread], best = INFINITY;
    int best_tau = kPtNone, first = kPtNone;
    float sum = before;
#pragma unroll
    for (int i = 0; i < kPtPerThread; ++i) {
      const int tau = t0 + i;
      sum += dv[i];
      cv[i] = sum > 0.f || sum != sum ? dv[i] * (float)tau / sum : 1.0f;  // (a NaN sum stays NaN, a zero sum is c = 1)
      if (tau <= tau_max) {
        dl[tau] = cv[i];
        if (tau >= tau_min) {
          if (cv[i] < threshold && first == kPtNone) first = tau;
          if (cv[i] < best) {
            best = cv[i];
            best_tau = tau;
          }
        }
      }
    }
    if (tid == 0) dl[0] = 1.0f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, kWave);
      const int ot = __shfl_xor(best_tau, o, kWave), of = __shfl_xor(first, o, kWave);
      if (ob < best || (ob == best && ot < best_tau)) {
        best = ob;
        best_tau = ot;
      }
      first = min(first, of);
    }
    __syncthreads();  // (every s_wave read above is done; every c is in dl)
    if (lane == 0) {
      s_wave[wave] = best;
      s_tau[wave] = best_tau;
      s_first[wave] = first;
    }
    __syncthreads();

    if (cmnd) {
      float *cj = cmnd + ((size_t)b * F + j) * (size_t)(tau_max + 1);
      for (int i = tid; i <= tau_max; i += kPtThreads) cj[i] = dl[i];
    }
    if (tid == 0) {
      for (int i = 1; i < kPtWaves; ++i) {
        if (s_wave[i] < best || (s_wave[i] == best && s_tau[i] < best_tau)) {
          best = s_wave[i];
          best_tau = s_tau[i];
        }
        first = min(first, s_first[i]);
      }
      const bool voiced = first != kPtNone;
      int ts = voiced ? first : best_tau;
      if (ts == kPtNone) ts = tau_min;  // (no c compares below +inf: every c of the range is NaN)
      if (voiced)
        while (ts + 1 <= tau_max && dl[ts + 1] < dl[ts]) ++ts;
      const float c1 = dl[ts];
      float p = (float)ts;
      if (ts - 1 >= 1 && ts + 1 <= tau_max) {
        const float c0 = dl[ts - 1], c2 = dl[ts + 1];
        if (c1 <= c0 && c1 <= c2) {
          const float den = 2.0f * ((c0 - 2.0f * c1) + c2);
          if (den != 0.f) p += (c0 - c2) / den;
        }
      }
      period[(size_t)b * F + j] = voiced ? p : 0.0f;
      aper[(size_t)b * F + j] = c1;
    }
    __syncthreads();  // (xs and dl are free for the next frame)
  }
}

__device__ __forceinline__ double pt_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int pt_wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (batch), one wave: lane i takes frames lo + i, lo + i + 64, ... then a fixed butterfly.
__global__ __launch_bounds__(kWave) void pt_distance_kernel(const float *__restrict__ pa, const float *__restrict__ pb,
                                                            int F, const int32_t *__restrict__ first,
                                                            const int32_t *__restrict__ count, double gross_ratio,
                                                            double *__restrict__ rmse, int32_t *__restrict__ counts) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const long long f0 = first[s], n = count[s];
  const int lo = (int)min(max(f0, 0LL), (long long)F);
  const int hi = (int)min(max(f0 + n, (long long)lo), (long long)F);
  const float *a = pa + (size_t)s * F, *b = pb + (size_t)s * F;
  double se = 0.0;
  int both = 0, vuv = 0, gross = 0;
  for (int f = lo + lane; f < hi; f += kWave) {
    const float ta = a[f], tb = b[f];
    const bool va = ta > 0.f, vb = tb > 0.f;  // (a voiced frame's period is at least 1/2; 0 and NaN are unvoiced)
    if (va && vb) {
      const double e = 1200.0 * log2((double)tb / (double)ta);
      se += e * e;
      ++both;
      if (fabs((double)ta / (double)tb - 1.0) > gross_ratio) ++gross;
    } else if (va != vb) {
      ++vuv;
    }
  }
  se = pt_wave_sum_f64(se);
  both = pt_wave_sum_i32(both);
  vuv = pt_wave_sum_i32(vuv);
  gross = pt_wave_sum_i32(gross);
  if (lane == 0) {
    rmse[s] = both > 0 ? sqrt(se / (double)both) : 0.0;
    counts[4 * s] = both;
    counts[4 * s + 1] = vuv;
    counts[4 * s + 2] = gross;
    counts[4 * s + 3] = hi - lo;
  }
}

static int pt_refuse(const char *what, const char *why) {
  set_error("%s: bad argument (%s)", what, why);
  return MVN_ERR_BAD_ARG;
}

static bool pt_shape_ok(int batch, int T, int win, int tau_max) {
  return batch >= 0 && batch <= 65535 && T >= 1 && T <= kPtMaxRow && (long long)batch * T <= kPtMaxSamples &&
         win >= kPtMinWin && win <= kPtMaxWin && tau_max >= kPtMinLag && tau_max <= kPtMaxLag;
}

}  // namespace mvn

extern "C" {

// the decoded signal (asked for with `wave` as well: the call takes one scratch whichever entry is used)
size_t mvn_pitch_scratch_floats(int batch, int n_samples, int win, int tau_max) {
  if (!mvn::pt_shape_ok(batch, n_samples, win, tau_max) || batch < 1) return 0;
  return (size_t)batch * n_samples;
}

int mvn_pitch_frames(const int32_t *index, const float *wave, int batch, int n_samples, int classes, int win, int hop,
                     int tau_min, int tau_max, float threshold, float *period, float *aper, float *cmnd,
                     float *scratch, size_t scratch_floats, void *stream) {
  const char *what = "mvn_pitch_frames";
  if ((index != nullptr) == (wave != nullptr)) return mvn::pt_refuse(what, "exactly one of index and wave must be given");
  if (!period || !aper || !scratch) return mvn::pt_refuse(what, "period, aper or scratch is NULL");
  if (!mvn::pt_shape_ok(batch, n_samples, win, tau_max))
    return mvn::pt_refuse(what, "win in [16, 4096], tau_max in [2, 1024], batch in [0, 65535], n_samples in [1, 2^30], "
                                "batch * n_samples below 2^31");
  if (tau_min < 1 || tau_min > tau_max) return mvn::pt_refuse(what, "tau_min must lie in [1, tau_max]");
  if (hop < 1 || hop > mvn::kPtMaxHop) return mvn::pt_refuse(what, "hop must lie in [1, 2^24]");
  if (!(threshold > 0.0f && threshold <= 1.0f)) return mvn::pt_refuse(what, "threshold must lie in (0, 1]");
  if (index && classes < 2) return mvn::pt_refuse(what, "classes must be at least 2");
  if (batch == 0) return MVN_OK;
  if (scratch_floats < mvn_pitch_scratch_floats(batch, n_samples, win, tau_max))
    return mvn::pt_refuse(what, "scratch too small");
  hipStream_t st = (hipStream_t)stream;
  const float *x = wave;
  if (index) {
    const size_t n = (size_t)batch * n_samples;
    hipLaunchKernelGGL(mvn::pt_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, index, scratch, n,
                       classes);
    const int rc = mvn::check_hip(hipGetLastError(), "pitch_frames (decode)");
    if (rc) return rc;
    x = scratch;
  }
  const int F = mvn::pt_frames(n_samples, hop);
  const int gx = F < mvn::kPtMaxGroups / batch ? F : mvn::kPtMaxGroups / batch;  // (batch <= 65535: at least 64)
  const size_t lds = (size_t)(win + tau_max + tau_max + 1) * sizeof(float);      // at most 28 KiB
  hipLaunchKernelGGL(mvn::pt_frames_kernel, dim3(gx, batch), dim3(mvn::kPtThreads), lds, st, x, n_samples, win, hop,
                     tau_min, tau_max, threshold, F, period, aper, cmnd);
  return mvn::check_hip(hipGetLastError(), "pitch_frames (frames)");
}

int mvn_pitch_distance(const float *period_a, const float *period_b, int batch, int frames, const int32_t *first,
                       const int32_t *count, double gross_ratio, double *rmse_cents, int32_t *counts, void *stream) {
  const char *what = "mvn_pitch_distance";
  if (batch < 1 || frames < 1 || batch > 65535) return mvn::pt_refuse(what, "batch in [1, 65535], frames >= 1");
  if (!period_a || !period_b || !first || !count || !rmse_cents || !counts)
    return mvn::pt_refuse(what, "period_a, period_b, first, count, rmse_cents or counts missing");
  if (!(gross_ratio > 0.0) || std::isinf(gross_ratio))
    return mvn::pt_refuse(what, "gross_ratio must be finite and above 0");
  hipLaunchKernelGGL(mvn::pt_distance_kernel, dim3(batch), dim3(mvn::kWave), 0, (hipStream_t)stream, period_a, period_b,
                     frames, first, count, gross_ratio, rmse_cents, counts);
  return mvn::check_hip(hipGetLastError(), what);
}

}  // extern "C"
