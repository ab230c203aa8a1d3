// Distance between two feature tensors (mvn_feature_distance): the log-spectral distance and the mean absolute
// difference of two (B, M, F) fp32 tensors over ONE span of frames per sequence -- READ ONLY.
//
//   d        = (double)a[b,m,f] - (double)b[b,m,f]           f in [first_b, first_b + count_b), m in [0, M)
//   rms_f    = sqrt((1/M) sum_m d^2)
//   lsd[b]   = (10 / ln 10) (1/count_b) sum_f rms_f          dB where the features are natural logs of power
//   l1[b]    = (1 / (M count_b)) sum_f sum_m |d|             in the features' own unit
//   per_frame[b,f] = (float)(rms_f 10 / ln 10) inside the span, 0.0f outside it (optional)
//
// Lane = frame (the contiguous axis: a wave's load of one bin is 256 contiguous bytes), kFrames frames per workgroup,
// grid (ceil(F / kFrames), B).  A lane walks the M bins of its frame with two double accumulators, the workgroup adds
// its lanes' (rms_f, sum_m |d|) by a butterfly inside the wave and across its four waves through LDS, and stores ONE
// pair of doubles into the caller's scratch -- every slot the second kernel reads, so the scratch needs no
// initialisation.  feature_distance_reduce_kernel adds a sequence's pairs in a fixed order.  No atomics; the blocks sit
// at multiples of kFrames whatever the span is and a sequence's sums see nothing of the other sequences: the same
// inputs give the same bits on every call and in every batch.  A lane outside the span loads nothing, so what the
// tensors hold there (NaN, inf, nothing initialised) never reaches a result.
#include "common.h"

namespace mvn {

constexpr int kFrames = 256;                               // frames per workgroup = threads
constexpr double kDbPerNat = 10.0 / 2.302585092994046;     // 10 / ln 10

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the span of sequence b, clamped to [0, F) (the range check proper is the host's: ops.feature_distance)
__device__ __forceinline__ void clamped_span(const int32_t *__restrict__ first, const int32_t *__restrict__ count, int b,
                                             int F, int &lo, int &hi) {
  const long long f0 = first[b], n = count[b];
  lo = (int)min(max(f0, 0LL), (long long)F);
  hi = (int)min(max(f0 + n, (long long)lo), (long long)F);
}

__global__ __launch_bounds__(kFrames) void feature_distance_kernel(const float *__restrict__ a,
                                                                   const float *__restrict__ b_, int M, int F,
                                                                   const int32_t *__restrict__ first,
                                                                   const int32_t *__restrict__ count,
                                                                   float *__restrict__ per_frame,
                                                                   double *__restrict__ part) {
  __shared__ double red[2][kFrames / 64];
  const int b = blockIdx.y;
  const long long f = (long long)blockIdx.x * kFrames + threadIdx.x;
  int lo, hi;
  clamped_span(first, count, b, F, lo, hi);
  double rms = 0.0, l1 = 0.0;
  if (f >= lo && f < hi) {
    const float *pa = a + (size_t)b * M * F + f, *pb = b_ + (size_t)b * M * F + f;
    double s2 = 0.0;
#pragma unroll 8
    for (int m = 0; m < M; ++m) {
      const double d = (double)pa[(size_t)m * F] - (double)pb[(size_t)m * F];
      s2 += d * d;
      l1 += fabs(d);
    }
    rms = sqrt(s2 / (double)M);
  }
  if (per_frame && f < F) per_frame[(size_t)b * F + f] = (float)(rms * kDbPerNat);
  rms = wave_sum_f64(rms);
  l1 = wave_sum_f64(l1);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = rms;
    red[1][threadIdx.x >> 6] = l1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t wg = (size_t)b * gridDim.x + blockIdx.x;
    part[2 * wg] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    part[2 * wg + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// One wave per sequence: lane i adds pairs i, i + 64, ... then a fixed butterfly -- the same order on every call.
__global__ __launch_bounds__(64) void feature_distance_reduce_kernel(const double *__restrict__ part, int parts, int M,
                                                                     int F, const int32_t *__restrict__ first,
                                                                     const int32_t *__restrict__ count,
                                                                     double *__restrict__ lsd,
                                                                     double *__restrict__ l1) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double rms = 0.0, ab = 0.0;
  for (int i = lane; i < parts; i += 64) {
    rms += part[2 * ((size_t)b * parts + i)];
    ab += part[2 * ((size_t)b * parts + i) + 1];
  }
  rms = wave_sum_f64(rms);
  ab = wave_sum_f64(ab);
  if (lane == 0) {
    int lo, hi;
    clamped_span(first, count, b, F, lo, hi);
    const int n = hi - lo;  // (an empty span: every pair is 0.0, and nothing is divided)
    lsd[b] = n > 0 ? kDbPerNat * (rms / (double)n) : 0.0;
    l1[b] = n > 0 ? ab / ((double)M * (double)n) : 0.0;
  }
}

}  // namespace mvn

extern "C" {

// two doubles (four floats) per workgroup of kFrames frames
size_t mvn_feature_distance_scratch_floats(int batch, int frames) {
  if (batch <= 0 || frames <= 0) return 0;
  return 4 * (size_t)batch * (size_t)((frames + mvn::kFrames - 1) / mvn::kFrames);
}

int mvn_feature_distance(const float *a, const float *b, int batch, int n_mels, int frames, const int32_t *first,
                         const int32_t *count, double *lsd, double *l1, float *per_frame, float *scratch,
                         size_t scratch_floats, void *stream) {
  const char *what = "mvn_feature_distance";
  if (batch < 1 || n_mels < 1 || frames < 1 || batch > 65535) {
    mvn::set_error("%s: bad argument (batch in [1, 65535], n_mels >= 1, frames >= 1)", what);
    return MVN_ERR_BAD_ARG;
  }
  if (!a || !b || !first || !count || !lsd || !l1) {
    mvn::set_error("%s: bad argument (a, b, first, count, lsd or l1 missing)", what);
    return MVN_ERR_BAD_ARG;
  }
  const size_t need = mvn_feature_distance_scratch_floats(batch, frames);
  if (!scratch || scratch_floats < need || ((uintptr_t)scratch & 7) != 0) {
    mvn::set_error("%s: bad argument (scratch missing, not 8-byte aligned, or of %zu floats where "
                   "mvn_feature_distance_scratch_floats asks for %zu)", what, scratch_floats, need);
    return MVN_ERR_BAD_ARG;
  }
  const int parts = (frames + mvn::kFrames - 1) / mvn::kFrames;
  double *part = (double *)scratch;
  hipLaunchKernelGGL(mvn::feature_distance_kernel, dim3(parts, batch), dim3(mvn::kFrames), 0, (hipStream_t)stream, a, b,
                     n_mels, frames, first, count, per_frame, part);
  const int rc = mvn::check_hip(hipGetLastError(), what);
  if (rc != MVN_OK) return rc;
  hipLaunchKernelGGL(mvn::feature_distance_reduce_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, part, parts,
                     n_mels, frames, first, count, lsd, l1);
  return mvn::check_hip(hipGetLastError(), what);
}

}  // extern "C"
