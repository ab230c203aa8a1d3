// The loader's waveform front end (movenet/dataset.py:253-289 without the decoder): interleaved int16 PCM of a batch of
// clips of different lengths -> (B, N) class indices, in two kernels.
//
//   af_resample_kernel   channel mean + sinc_interp_hann resample of the WHOLE clip to N frames (lowpass_filter_width 6,
//                        roll-off 0.99), fp32 y, and the (min, max) of every tile of outputs
//   af_quantise_kernel   the clip's (min, max) from the tile partials, min-max normalise, mu-law, clamp -> int32 index
//
// Per output sample k of a clip of n frames (g = gcd(n, N), orig = n/g, new = N/g, s = 0.99 min(orig, new)/orig):
//   c = k orig/new,  y[k] = sum_i m[i] h(i - c),  u = (i - c) s,  h = s sinc(pi u) cos^2(pi u/12) for |u| < 6, else 0
// k orig is a 64-bit integer product; i0 = floor(c) and the phase (k orig) mod new are taken from it exactly, so the
// float part of a tap's argument is (i - i0) - phase/new: a small integer minus a fraction, whatever the clip's length.
//
// Clips come through a DEVICE descriptor array (one launch per batch, not per clip).  Every read of the upload is
// bounded by the descriptor's own span [offset, offset + frames channels), and a descriptor whose span does not lie
// inside [0, pcm_len) -- or whose ratio n/N needs a longer window than the LDS tile holds (n <= 100 N always fits) --
// is never read through: its row of indices is filled with -1.
#include "common.h"

#include <cmath>

namespace mvn {

constexpr int kAfTile = 1024;   // output samples per workgroup
constexpr int kAfWin = 8192;    // fp32 input window in LDS (32 KiB)
constexpr int kAfMinSub = 64;   // a workgroup walks its tile in sub-tiles of at least this many outputs
constexpr int kAfThreads = 256;
constexpr int kAfTapBlock = 128;  // the windowed form sums an output's taps in blocks of this many (af_resample)

struct AfGeom {
  long long orig, neu;
  float s;   // base / orig: the tap argument's scale and the filter's gain
  int W;     // taps reach i0 - W .. i0 + W + 1
  int sub;   // outputs per staged window
  bool ok;
};

__device__ __forceinline__ long long af_gcd(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// s, W and sub of the reduced ratio g.orig : g.neu; g.ok cleared where the window of kAfMinSub outputs does not fit
__device__ __forceinline__ void af_geom_taps(AfGeom &g) {
  const double sd = 0.99 * (double)(g.orig < g.neu ? g.orig : g.neu) / (double)g.orig;
  g.s = (float)sd;
  g.W = (int)(6.0 / sd) + 1;
  const long long room = (long long)kAfWin - 2LL * g.W - 4;
  if (room < 0) {
    g.ok = false;
    return;
  }
  const long long sub = 1 + room * g.neu / g.orig;
  g.sub = (int)(sub < kAfTile ? sub : kAfTile);
  if (g.sub < kAfMinSub) g.ok = false;
}

__device__ __forceinline__ AfGeom af_geom(const mvn_audio_clip &c, long long pcm_len, int N) {
  AfGeom g;
  g.ok = c.frames >= 1 && c.channels >= 1 && c.offset >= 0 &&
         c.offset + (long long)c.frames * c.channels <= pcm_len;
  g.orig = g.neu = 1;
  g.s = 0.f;
  g.W = g.sub = 0;
  if (!g.ok) return g;
  const long long a = af_gcd(c.frames, N);
  g.orig = c.frames / a;
  g.neu = N / a;
  af_geom_taps(g);
  return g;
}

__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }

// The by-rate form (mvn_audio_frontend_var): clip b is resampled to ITS OWN n_out frames into a row of `width`; the rest
// of the row is silence.  The descriptor, and what it makes of a row: N outputs to form (the whole width for a
// descriptor that is refused, so that the whole row is marked), by the geometry of the plain form for N.
struct AfRow {
  mvn_audio_clip c;
  AfGeom g;
  int N;
};
__device__ __forceinline__ AfRow af_row_var(const mvn_audio_clip_var &v, long long pcm_len, int width) {
  AfRow r;
  r.c.offset = v.offset;
  r.c.frames = v.frames;
  r.c.channels = v.channels;
  const bool fits = v.n_out >= 1 && v.n_out <= width;
  r.N = fits ? v.n_out : width;
  r.g = af_geom(r.c, pcm_len, r.N);
  if (!fits) r.g.ok = false;
  if (!r.g.ok) r.N = width;
  return r;
}

// The windowed by-rate form (mvn_audio_frontend_window): row b is the columns [out_first, out_first + n_out) of the
// resample of a whole FILE from rate_in to rate_out, of which only the span the taps of those columns reach was
// uploaded.  AfAt places a row in its file: column k of the row is the file's output j0 + k, frame i of the file is
// frame i - first of the span, and m[i] = 0 outside [0, file_frames).  (The other two forms are j0 = first = 0 with
// the span the whole clip.)
struct AfAt {
  long long j0, first, file_frames;
};
struct AfWinRow {
  mvn_audio_clip c;  // the uploaded span: offset, span_frames, channels
  AfGeom g;
  AfAt at;
  int N;
  float lo, hi;  // the given normalisation range, hi > lo; else lo = hi = 0: the window's own
};
__device__ __forceinline__ AfWinRow af_row_window(const mvn_audio_clip_window &v, long long pcm_len, int width) {
  AfWinRow r;
  r.c.offset = v.offset;
  r.c.frames = v.span_frames;
  r.c.channels = v.channels;
  r.at.j0 = v.out_first;
  r.at.first = v.span_first;
  r.at.file_frames = v.file_frames;
  r.N = width;
  const bool given = v.hi > v.lo && v.hi - v.lo < INFINITY;  // (NaN or an infinite range: not given)
  r.lo = given ? v.lo : 0.f;
  r.hi = given ? v.hi : 0.f;
  AfGeom &g = r.g;
  g.orig = g.neu = 1;
  g.s = 0.f;
  g.W = g.sub = 0;
  g.ok = false;
  if (v.n_out < 1 || v.n_out > width) return r;
  if (v.rate_in < 1 || v.rate_out < 1 || v.channels < 1 || v.span_frames < 1) return r;
  const long long span = (long long)v.span_frames * v.channels;
  if (v.offset < 0 || span > pcm_len || v.offset > pcm_len - span) return r;
  const long long a = af_gcd(v.rate_in, v.rate_out);
  g.orig = v.rate_in / a;
  g.neu = v.rate_out / a;
  g.ok = true;
  af_geom_taps(g);
  if (!g.ok) return r;
  g.ok = false;
  // n_file = ceil(file_frames neu / orig); a file whose products leave 62 bits has no window
  if (v.file_frames < 1 || v.file_frames > (1LL << 62) / g.neu) return r;
  const long long n_file = (v.file_frames * g.neu + g.orig - 1) / g.orig;
  if (v.out_first < 0 || v.out_first > n_file - v.n_out) return r;
  // the span covers every frame of the file the window's taps reach
  const long long need_lo = max(0LL, (v.out_first * g.orig) / g.neu - g.W);
  const long long need_hi = min(v.file_frames - 1, ((v.out_first + v.n_out - 1) * g.orig) / g.neu + g.W + 1);
  if (v.span_first < 0 || v.span_first > need_lo || need_hi - v.span_first >= (long long)v.span_frames) return r;
  g.ok = true;
  r.N = v.n_out;
  return r;
}

// VAR = false: N outputs per row, rows N apart (the plain form, as it was).  VAR = true: N of `width` outputs.
// WIN (with VAR): the row's place in its file is `at`; without it `at` is not looked at.  WIN also sums an output's
// taps in blocks of kAfTapBlock: each block from 0 by fmaf in ascending d, the block sums added in ascending order.
// One chain of fmaf over 2 W + 2 taps loses accuracy as sqrt(taps) -- 1.4e-6 against float64 at 100 : 1, 1216 taps,
// where float32 numpy's pairwise sum stays near 2e-7 -- and blocks of 128 hold it near 4e-7.  An output of at most
// kAfTapBlock taps (rate_in <= 10 rate_out) is ONE block, to which nothing is added: the other forms' bits.
template <bool VAR, bool WIN = false>
__device__ __forceinline__ void af_resample(const int16_t *__restrict__ pcm, const mvn_audio_clip &c, const AfGeom &g,
                                            int N, int width, float *__restrict__ y, float2 *__restrict__ part,
                                            const AfAt at = AfAt{0, 0, 0}) {
  __shared__ float win[kAfWin];
  __shared__ float red[2 * (kAfThreads / kWave)];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int t0 = blockIdx.x * kAfTile, t1 = min(N, t0 + kAfTile);
  float *yb = y + (size_t)b * (VAR ? width : N);
  if (!g.ok) {  // (workgroup-uniform) nothing of the upload is read
    for (int k = t0 + tid; k < t1; k += kAfThreads) yb[k] = 0.f;
    if (tid == 0) part[(size_t)b * gridDim.x + blockIdx.x] = make_float2(0.f, 0.f);
    return;
  }
  if (VAR) {  // the silence behind the clip; a tile that holds nothing else ends here (workgroup-uniform)
    for (int k = max(N, t0) + tid; k < min(width, t0 + kAfTile); k += kAfThreads) yb[k] = 0.f;
    if (t0 >= N) return;
  }
  const int16_t *src = pcm + c.offset;
  const int ch = c.channels, W = g.W;
  const float den = 32768.0f * (float)ch, s = g.s, fneu = (float)g.neu;
  const float kPi = 3.14159265358979323846f;
  float mn = INFINITY, mx = -INFINITY;
  for (int k0 = t0; k0 < t1; k0 += g.sub) {
    const int k1 = min(t1, k0 + g.sub);
    const long long j0 = WIN ? at.j0 : 0LL;
    const long long lo = ((j0 + k0) * g.orig) / g.neu - W;
    const long long hi = ((j0 + (k1 - 1)) * g.orig) / g.neu + W + 1;
    const int len = (int)min(hi - lo + 1, (long long)kAfWin);  // (af_geom sized sub so that the window fits)
    __syncthreads();  // the previous window has been consumed
    for (int j = tid; j < len; j += kAfThreads) {
      const long long i = lo + j;
      float v = 0.f;  // m[i] = 0 outside the clip
      const long long is = WIN ? i - at.first : i;  // its place in the upload: every read stays inside the span
      if (i >= 0 && is >= 0 && is < c.frames && (!WIN || i < at.file_frames)) {
        int sum = 0;
        for (int q = 0; q < ch; ++q) sum += src[is * ch + q];
        v = (float)sum / den;
      }
      win[j] = v;
    }
    __syncthreads();
    for (int k = k0 + tid; k < k1; k += kAfThreads) {
      const long long p = (j0 + k) * g.orig;
      const long long i0 = p / g.neu;
      const float frac = (float)(p - i0 * g.neu) / fneu;
      const float *w = win + (int)(i0 - lo);
      float acc = 0.f, blocks = 0.f;
      for (int d = -W; d <= W + 1; ++d) {
        if (WIN && d != -W && (d + W) % kAfTapBlock == 0) {  // a block is full
          blocks += acc;
          acc = 0.f;
        }
        const float u = ((float)d - frac) * s;
        float h = 0.f;
        if (fabsf(u) < 6.0f) {
          const float sinc = u == 0.f ? 1.0f : sinpif(u) / (kPi * u);
          const float cw = cospif(u / 12.0f);
          h = s * sinc * (cw * cw);
        }
        acc = fmaf(w[d], h, acc);
      }
      if (WIN && 2 * W + 2 > kAfTapBlock) acc = blocks + acc;
      yb[k] = acc;
      mn = fminf(mn, acc);
      mx = fmaxf(mx, acc);
    }
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  const int wave = tid / kWave;
  if ((tid & (kWave - 1)) == 0) {
    red[2 * wave] = mn;
    red[2 * wave + 1] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < kAfThreads / kWave; ++v) {
      mn = fminf(mn, red[2 * v]);
      mx = fmaxf(mx, red[2 * v + 1]);
    }
    part[(size_t)b * gridDim.x + blockIdx.x] = make_float2(mn, mx);
  }
}

__global__ __launch_bounds__(kAfThreads) void af_resample_kernel(const int16_t *__restrict__ pcm, long long pcm_len,
                                                                 const mvn_audio_clip *__restrict__ clips, int N,
                                                                 float *__restrict__ y, float2 *__restrict__ part) {
  const mvn_audio_clip c = clips[blockIdx.y];
  const AfGeom g = af_geom(c, pcm_len, N);
  af_resample<false>(pcm, c, g, N, N, y, part);
}

__global__ __launch_bounds__(kAfThreads) void af_resample_var_kernel(const int16_t *__restrict__ pcm,
                                                                     long long pcm_len,
                                                                     const mvn_audio_clip_var *__restrict__ clips,
                                                                     int width, float *__restrict__ y,
                                                                     float2 *__restrict__ part) {
  const AfRow r = af_row_var(clips[blockIdx.y], pcm_len, width);
  af_resample<true>(pcm, r.c, r.g, r.N, width, y, part);
}

__global__ __launch_bounds__(kAfThreads) void af_resample_window_kernel(const int16_t *__restrict__ pcm,
                                                                        long long pcm_len,
                                                                        const mvn_audio_clip_window *__restrict__ clips,
                                                                        int width, float *__restrict__ y,
                                                                        float2 *__restrict__ part) {
  const AfWinRow r = af_row_window(clips[blockIdx.y], pcm_len, width);
  af_resample<true, true>(pcm, r.c, r.g, r.N, width, y, part, r.at);
}

// audio <- (audio - min) / (max - min); audio * 2 - 1 (dataset.py:271-275), a clip with max == min left as it is (the
// silent clip of the reference's `sum() == 0` test); then the mu-law of mu_law_encode_kernel, clamped to 0 .. Q-1
// (an un-normalised resample may overshoot [-1, 1]).
// VAR: the (min, max) runs over the tiles that hold the clip's N outputs, of the `tiles` slots a row has; the columns
// behind them get the class mu-law gives 0.0.  WIN: a range ghi > glo is the (min, max) to normalise by, given with
// the row (workgroup-uniform); without one the row's own.
template <bool VAR, bool WIN = false>
__device__ __forceinline__ void af_quantise(const AfGeom &g, int N, int width, int Q, int normalize, int tiles,
                                            const float *__restrict__ y, const float2 *__restrict__ part,
                                            int32_t *__restrict__ idx, float glo = 0.f, float ghi = 0.f) {
  __shared__ float red[2 * (kAfThreads / kWave)];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int t0 = blockIdx.x * kAfTile, t1 = min(N, t0 + kAfTile);
  int32_t *ib = idx + (size_t)b * (VAR ? width : N);
  if (!g.ok) {
    for (int k = t0 + tid; k < t1; k += kAfThreads) ib[k] = -1;
    return;
  }
  if (VAR) {  // (workgroup-uniform)
    const int silence = (int)((float)(Q - 1) / 2.0f + 0.5f);
    for (int k = max(N, t0) + tid; k < min(width, t0 + kAfTile); k += kAfThreads) ib[k] = silence;
    if (t0 >= N) return;
  }
  const int own = VAR ? (N + kAfTile - 1) / kAfTile : tiles;
  float mn = INFINITY, mx = -INFINITY;
  if (WIN && normalize && ghi > glo) {
    mn = glo;
    mx = ghi;
  } else if (normalize) {  // every workgroup folds the clip's partials in the same order: one (min, max) per clip, reproducibly
    for (int t = tid; t < own; t += kAfThreads) {
      const float2 p = part[(size_t)b * tiles + t];
      mn = fminf(mn, p.x);
      mx = fmaxf(mx, p.y);
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    if ((tid & (kWave - 1)) == 0) {
      red[2 * (tid / kWave)] = mn;
      red[2 * (tid / kWave) + 1] = mx;
    }
    __syncthreads();
    mn = red[0];
    mx = red[1];
    for (int v = 1; v < kAfThreads / kWave; ++v) {
      mn = fminf(mn, red[2 * v]);
      mx = fmaxf(mx, red[2 * v + 1]);
    }
  }
  const bool scale = normalize && mx != mn;
  const float mu = (float)(Q - 1), range = mx - mn, lmu = log1pf(mu);
  const float *yb = y + (size_t)b * (VAR ? width : N);
  for (int k = t0 + tid; k < t1; k += kAfThreads) {
    float v = yb[k];
    if (scale) {
      v = (v - mn) / range;
      v = v * 2.0f - 1.0f;
    }
    const float z = copysignf(log1pf(mu * fabsf(v)) / lmu, v);
    const int q = (int)((z + 1.0f) / 2.0f * mu + 0.5f);
    ib[k] = min(max(q, 0), Q - 1);
  }
}

__global__ __launch_bounds__(kAfThreads) void af_quantise_kernel(const mvn_audio_clip *__restrict__ clips,
                                                                 long long pcm_len, int N, int Q, int normalize,
                                                                 int tiles, const float *__restrict__ y,
                                                                 const float2 *__restrict__ part,
                                                                 int32_t *__restrict__ idx) {
  const AfGeom g = af_geom(clips[blockIdx.y], pcm_len, N);
  af_quantise<false>(g, N, N, Q, normalize, tiles, y, part, idx);
}

__global__ __launch_bounds__(kAfThreads) void af_quantise_var_kernel(const mvn_audio_clip_var *__restrict__ clips,
                                                                     long long pcm_len, int width, int Q,
                                                                     int normalize, int tiles,
                                                                     const float *__restrict__ y,
                                                                     const float2 *__restrict__ part,
                                                                     int32_t *__restrict__ idx) {
  const AfRow r = af_row_var(clips[blockIdx.y], pcm_len, width);
  af_quantise<true>(r.g, r.N, width, Q, normalize, tiles, y, part, idx);
}

__global__ __launch_bounds__(kAfThreads) void af_quantise_window_kernel(const mvn_audio_clip_window *__restrict__ clips,
                                                                        long long pcm_len, int width, int Q,
                                                                        int normalize, int tiles,
                                                                        const float *__restrict__ y,
                                                                        const float2 *__restrict__ part,
                                                                        int32_t *__restrict__ idx) {
  const AfWinRow r = af_row_window(clips[blockIdx.y], pcm_len, width);
  af_quantise<true, true>(r.g, r.N, width, Q, normalize, tiles, y, part, idx, r.lo, r.hi);
}

}  // namespace mvn

extern "C" {

size_t mvn_audio_frontend_scratch_floats(int batch, int n_out) {
  if (batch < 1 || n_out < 1) return 0;
  return 2 * (size_t)batch * (size_t)((n_out + mvn::kAfTile - 1) / mvn::kAfTile);
}

int mvn_audio_frontend(const int16_t *pcm, long long pcm_len, const mvn_audio_clip *clips, int batch, int classes,
                       int n_out, int normalize, float *y, float *scratch, int32_t *index, void *stream) {
  if (!pcm || !clips || !y || !scratch || !index || pcm_len < 1 || batch < 1 || batch > 65535 || n_out < 1 ||
      classes < 2 || classes > 65536) {
    mvn::set_error("mvn_audio_frontend: bad argument");
    return MVN_ERR_BAD_ARG;
  }
  if (((uintptr_t)scratch & 7u) != 0) {
    mvn::set_error("mvn_audio_frontend: scratch must be 8-byte aligned");
    return MVN_ERR_BAD_ARG;
  }
  const int tiles = (n_out + mvn::kAfTile - 1) / mvn::kAfTile;
  const dim3 grid(tiles, batch);
  hipLaunchKernelGGL(mvn::af_resample_kernel, grid, dim3(mvn::kAfThreads), 0, (hipStream_t)stream, pcm, pcm_len,
                     clips, n_out, y, (float2 *)scratch);
  int rc = mvn::check_hip(hipGetLastError(), "audio_frontend (resample)");
  if (rc) return rc;
  hipLaunchKernelGGL(mvn::af_quantise_kernel, grid, dim3(mvn::kAfThreads), 0, (hipStream_t)stream, clips, pcm_len,
                     n_out, classes, normalize, tiles, (const float *)y, (const float2 *)scratch, index);
  return mvn::check_hip(hipGetLastError(), "audio_frontend (quantise)");
}

size_t mvn_audio_frontend_var_scratch_floats(int batch, int width) {
  return mvn_audio_frontend_scratch_floats(batch, width);
}

int mvn_audio_frontend_var(const int16_t *pcm, long long pcm_len, const mvn_audio_clip_var *clips, int batch,
                           int classes, int width, int normalize, float *y, float *scratch, int32_t *index,
                           void *stream) {
  if (!pcm || !clips || !y || !scratch || !index || pcm_len < 1 || batch < 1 || batch > 65535 || width < 1 ||
      classes < 2 || classes > 65536) {
    mvn::set_error("mvn_audio_frontend_var: bad argument");
    return MVN_ERR_BAD_ARG;
  }
  if (((uintptr_t)scratch & 7u) != 0) {
    mvn::set_error("mvn_audio_frontend_var: scratch must be 8-byte aligned");
    return MVN_ERR_BAD_ARG;
  }
  const int tiles = (width + mvn::kAfTile - 1) / mvn::kAfTile;
  const dim3 grid(tiles, batch);
  hipLaunchKernelGGL(mvn::af_resample_var_kernel, grid, dim3(mvn::kAfThreads), 0, (hipStream_t)stream, pcm, pcm_len,
                     clips, width, y, (float2 *)scratch);
  int rc = mvn::check_hip(hipGetLastError(), "audio_frontend_var (resample)");
  if (rc) return rc;
  hipLaunchKernelGGL(mvn::af_quantise_var_kernel, grid, dim3(mvn::kAfThreads), 0, (hipStream_t)stream, clips, pcm_len,
                     width, classes, normalize, tiles, (const float *)y, (const float2 *)scratch, index);
  return mvn::check_hip(hipGetLastError(), "audio_frontend_var (quantise)");
}

size_t mvn_audio_frontend_window_scratch_floats(int batch, int width) {
  return mvn_audio_frontend_scratch_floats(batch, width);
}

int mvn_audio_frontend_window(const int16_t *pcm, long long pcm_len, const mvn_audio_clip_window *clips, int batch,
                              int classes, int width, int normalize, float *y, float *scratch, int32_t *index,
                              void *stream) {
  if (!pcm || !clips || !y || !scratch || !index || pcm_len < 1 || batch < 1 || batch > 65535 || width < 1 ||
      classes < 2 || classes > 65536) {
    mvn::set_error("mvn_audio_frontend_window: bad argument");
    return MVN_ERR_BAD_ARG;
  }
  if (((uintptr_t)scratch & 7u) != 0) {
    mvn::set_error("mvn_audio_frontend_window: scratch must be 8-byte aligned");
    return MVN_ERR_BAD_ARG;
  }
  const int tiles = (width + mvn::kAfTile - 1) / mvn::kAfTile;
  const dim3 grid(tiles, batch);
  hipLaunchKernelGGL(mvn::af_resample_window_kernel, grid, dim3(mvn::kAfThreads), 0, (hipStream_t)stream, pcm,
                     pcm_len, clips, width, y, (float2 *)scratch);
  int rc = mvn::check_hip(hipGetLastError(), "audio_frontend_window (resample)");
  if (rc) return rc;
  hipLaunchKernelGGL(mvn::af_quantise_window_kernel, grid, dim3(mvn::kAfThreads), 0, (hipStream_t)stream, clips,
                     pcm_len, width, classes, normalize, tiles, (const float *)y, (const float2 *)scratch, index);
  return mvn::check_hip(hipGetLastError(), "audio_frontend_window (quantise)");
}

}  // extern "C"
