// A pitch track as two local-conditioning channels: a continuous log-F0 and the voicing flag.
//
//   pf_features_kernel  one workgroup per row.  Frame j is voiced where period[j] > 0 (0, a negative value and NaN are
//                       unvoiced).  Pass 1 walks the row's chunks from the last to the first with a reverse min-scan of
//                       (voiced ? j : F) -- the nearest voiced frame at or above j -- and parks it, as an integer's bits,
//                       in the frame's own word of the voicing row.  Pass 2 walks them from the first to the last with
//                       an inclusive max-scan of (voiced ? j : -1) -- the nearest voiced frame at or below j --, reads the
//                       parked index back (the thread that wrote the word reads it), forms lf and writes both rows.
//
// A chunk is kPfThreads frames, one per thread; the scan value of the chunks already walked is carried in a register.
// No atomics; a frame's result depends on its row's periods alone and every expression has one order, so the same bits
// come out on every call and at every batch position.
#include "common.h"

#include <cmath>

namespace mvn {

constexpr int kPfThreads = 256;  // four waves; also the frames of one chunk
constexpr int kPfWaves = kPfThreads / kWave;
constexpr int kPfMaxFrames = 1 << 30;

// log2 of the frame's frequency over f_ref: formed in double, rounded once
__device__ __forceinline__ float pf_log_f0(float period, double rate, double f_ref) {
  return (float)log2(rate / ((double)period * f_ref));
}

__global__ __launch_bounds__(kPfThreads) void pf_features_kernel(const float *__restrict__ period, int F, float rate,
                                                                 float f_ref, const float *__restrict__ shift,
                                                                 float *out, long long row_stride,
                                                                 long long chan_stride) {
  __shared__ int s_wave[kPfWaves];
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  const int b = blockIdx.x;
  const float *pb = period + (size_t)b * F;
  float *o_lf = out + (long long)b * row_stride, *o_v = o_lf + chan_stride;
  const double rate_d = (double)rate, f_ref_d = (double)f_ref;
  const float sh = shift ? shift[b] : 0.0f;
  const int chunks = (F + kPfThreads - 1) / kPfThreads;  // (F <= 2^30: no overflow)

  // pass 1: next[j] = the lowest voiced frame >= j, F where there is none
  int carry = F;
  for (int c = chunks - 1; c >= 0; --c) {
    const int j = c * kPfThreads + tid;
    const bool in = j < F;
    int key = (in && pb[j] > 0.0f) ? j : F;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int other = __shfl_down(key, o, kWave);
      if (lane + o < kWave) key = min(key, other);
    }
    if (lane == 0) s_wave[wave] = key;  // (the wave's minimum)
    __syncthreads();
    int after = carry, total = carry;
#pragma unroll
    for (int i = kPfWaves - 1; i >= 0; --i) {
      if (i > wave) after = min(after, s_wave[i]);
      total = min(total, s_wave[i]);
    }
    key = min(key, after);
    if (in) o_v[j] = __int_as_float(key);
    carry = total;
    __syncthreads();  // (s_wave is free for the next chunk)
  }

  // pass 2: prev[j] = the highest voiced frame <= j, -1 where there is none
  carry = -1;
  for (int c = 0; c < chunks; ++c) {
    const int j = c * kPfThreads + tid;
    const bool in = j < F;
    const float per = in ? pb[j] : 0.0f;
    const bool voiced = per > 0.0f;
    int key = voiced ? j : -1;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int other = __shfl_up(key, o, kWave);
      if (lane >= o) key = max(key, other);
    }
    if (lane == kWave - 1) s_wave[wave] = key;  // (the wave's maximum)
    __syncthreads();
    int before = carry, total = carry;
#pragma unroll
    for (int i = 0; i < kPfWaves; ++i) {
      if (i < wave) before = max(before, s_wave[i]);
      total = max(total, s_wave[i]);
    }
    const int p = max(key, before);
    if (in) {
      const int n = voiced ? j : __float_as_int(o_v[j]);
      float lf;
      if (voiced) {
        lf = pf_log_f0(per, rate_d, f_ref_d);
      } else if (p < 0) {
        lf = n < F ? pf_log_f0(pb[n], rate_d, f_ref_d) : 0.0f;  // (before the first voiced frame; no voiced frame)
      } else if (n >= F) {
        lf = pf_log_f0(pb[p], rate_d, f_ref_d);                 // (after the last voiced frame)
      } else {
        const float a = (float)(j - p) / (float)(n - p);
        const float lp = pf_log_f0(pb[p], rate_d, f_ref_d), ln = pf_log_f0(pb[n], rate_d, f_ref_d);
        lf = fmaf(a, ln, (1.0f - a) * lp);
      }
      o_lf[j] = lf + sh;
      o_v[j] = voiced ? 1.0f : 0.0f;
    }
    carry = total;
    __syncthreads();
  }
}

static int pf_refuse(const char *why) {
  set_error("mvn_pitch_features: bad argument (%s)", why);
  return MVN_ERR_BAD_ARG;
}

}  // namespace mvn

extern "C" {

int mvn_pitch_features(const float *period, int batch, int frames, float rate, float f_ref, const float *shift,
                       float *out, long long row_stride, long long chan_stride, void *stream) {
  if (!period || !out) return mvn::pf_refuse("period or out is NULL");
  if (frames < 1 || frames > mvn::kPfMaxFrames) return mvn::pf_refuse("frames must lie in [1, 2^30]");
  if (batch < 0 || batch > 65535) return mvn::pf_refuse("batch must lie in [0, 65535]");
  if (!(rate > 0.0f) || std::isinf(rate) || !(f_ref > 0.0f) || std::isinf(f_ref))
    return mvn::pf_refuse("rate and f_ref must be finite and above 0");
  // the two rows of a sequence, and the row pairs of two sequences, must not share a word
  if (chan_stride < frames) return mvn::pf_refuse("chan_stride must be at least frames: the two rows would overlap");
  if (batch > 1 && row_stride < chan_stride + frames)
    return mvn::pf_refuse("row_stride must be at least chan_stride + frames: two sequences' rows would overlap");
  if (batch == 0) return MVN_OK;
  hipLaunchKernelGGL(mvn::pf_features_kernel, dim3(batch), dim3(mvn::kPfThreads), 0, (hipStream_t)stream, period,
                     frames, rate, f_ref, shift, out, row_stride, chan_stride);
  return mvn::check_hip(hipGetLastError(), "mvn_pitch_features");
}

}  // extern "C"
