// The loader's waveform front end (movenet/dataset.py:253-289 without the decoder): interleaved int16 PCM of a batch of
// clips of different lengths -> (B, width) class indices, in two kernels.
//
//   af_resample_kernel   channel mean + sinc_interp_hann resample to the row's N frames (lowpass_filter_width 6,
//                        roll-off 0.99), fp32 y, and the (min, max) of every tile of outputs
//   af_quantise_kernel   the row's (min, max) from the tile partials, min-max normalise, mu-law, clamp -> int32 index
//
// ONE form serves the three entry points.  A row (AfRow) is N <= width outputs, silence behind them, that are the
// columns [j0, j0 + N) of the resample orig : new of a FILE of file_frames frames, formed from an uploaded span whose
// frame 0 is the file's frame `first`.  The three descriptors only say how a row is found:
//   mvn_audio_clip          the whole clip to N = width = n_out frames: j0 = first = 0, the span is the file
//   mvn_audio_clip_var      the whole clip to its own N = n_out <= width frames: placed as above
//   mvn_audio_clip_window   N columns at out_first of a file's resample rate_in : rate_out, and a range to normalise by
//
// Per output j of a file of n frames (orig : new the reduced ratio, s = 0.99 min(orig, new)/orig):
//   c = j orig/new,  y[j] = sum_i m[i] h(i - c),  u = (i - c) s,  h = s sinc(pi u) cos^2(pi u/12) for |u| < 6, else 0
// j orig is a 64-bit integer product; i0 = floor(c) and the phase (j orig) mod new are taken from it exactly, so the
// float part of a tap's argument is (i - i0) - phase/new: a small integer minus a fraction, whatever the file's length.
//
// Rows come through a DEVICE descriptor array (one launch per batch, not per clip).  Every read of the upload is
// bounded by the descriptor's own span [offset, offset + frames channels), and a descriptor whose span does not lie
// inside [0, pcm_len) -- or whose ratio needs a longer window than the LDS tile holds (n <= 100 N always fits) --
// is never read through: its row of indices is filled with -1.
#include "common.h"

#include <cmath>
#include <cstdint>
#include <string>

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

// A row's place in its file: column k of the row is the file's output j0 + k, frame i of the file is frame i - first
// of the span, and m[i] = 0 outside [0, file_frames).
struct AfAt {
  long long j0, first, file_frames;
};

struct AfRow {
  mvn_audio_clip c;  // the uploaded span: offset, frames, channels
  AfGeom g;
  AfAt at;
  int N;          // outputs to form; `width` where g.ok is false, so that the whole row is marked
  float lo, hi;   // the given normalisation range, hi > lo; else lo = hi = 0: the row's own
};

// [offset, offset + frames channels) lies inside [0, pcm_len); frames, channels in [1, 2^31), so no sum or product
// here leaves 64 bits whatever the offset
constexpr bool af_span_ok(long long offset, long long frames, long long channels, long long pcm_len) {
  return offset >= 0 && frames * channels <= pcm_len && offset <= pcm_len - frames * channels;
}
static_assert(af_span_ok(10, 45, 2, 100), "a span ending exactly at pcm_len lies inside");
static_assert(!af_span_ok(11, 45, 2, 100), "one sample past pcm_len");
static_assert(!af_span_ok(-1, 45, 2, 100), "offset = -1");
static_assert(!af_span_ok(INT64_MAX, 50, 2, 1000) && !af_span_ok(INT64_MAX - 10, 50, 2, 1000), "offset near 2^63");
static_assert(!af_span_ok(0, INT32_MAX, INT32_MAX, 1LL << 40), "the largest span, without overflow");

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

// the refused row of `width` columns over the span (offset, frames, channels); the builders below fill in the rest
__device__ __forceinline__ AfRow af_row_refused(long long offset, int frames, int channels, int width) {
  AfRow r;
  r.c.offset = offset;
  r.c.frames = frames;
  r.c.channels = channels;
  r.g.orig = r.g.neu = 1;
  r.g.s = 0.f;
  r.g.W = r.g.sub = 0;
  r.g.ok = false;
  r.at = AfAt{0, 0, frames};
  r.N = width;
  r.lo = r.hi = 0.f;
  return r;
}

// The by-rate form (mvn_audio_frontend_var): the whole clip, resampled to ITS OWN n_out frames
__device__ __forceinline__ AfRow af_row(const mvn_audio_clip_var &v, long long pcm_len, int width) {
  AfRow r = af_row_refused(v.offset, v.frames, v.channels, width);
  if (v.n_out < 1 || v.n_out > width) return r;
  if (v.frames < 1 || v.channels < 1 || !af_span_ok(v.offset, v.frames, v.channels, pcm_len)) return r;
  const long long a = af_gcd(v.frames, v.n_out);
  r.g.orig = v.frames / a;
  r.g.neu = v.n_out / a;
  r.g.ok = true;
  af_geom_taps(r.g);
  if (r.g.ok) r.N = v.n_out;
  return r;
}

// The plain form (mvn_audio_frontend): the by-rate form with n_out = width for every clip
__device__ __forceinline__ AfRow af_row(const mvn_audio_clip &c, long long pcm_len, int width) {
  return af_row(mvn_audio_clip_var{c.offset, c.frames, c.channels, width, 0}, pcm_len, width);
}

// The windowed by-rate form (mvn_audio_frontend_window): row b is the columns [out_first, out_first + n_out) of the
// resample of a whole FILE from rate_in to rate_out, of which only the span the taps of those columns reach was
// uploaded.
__device__ __forceinline__ AfRow af_row(const mvn_audio_clip_window &v, long long pcm_len, int width) {
  AfRow r = af_row_refused(v.offset, v.span_frames, v.channels, width);
  r.at = AfAt{v.out_first, v.span_first, v.file_frames};
  const bool given = v.hi > v.lo && v.hi - v.lo < INFINITY;  // (NaN or an infinite range: not given)
  r.lo = given ? v.lo : 0.f;
  r.hi = given ? v.hi : 0.f;
  AfGeom &g = r.g;
  if (v.n_out < 1 || v.n_out > width) return r;
  if (v.rate_in < 1 || v.rate_out < 1 || v.channels < 1 || v.span_frames < 1) return r;
  if (!af_span_ok(v.offset, v.span_frames, v.channels, pcm_len)) return r;
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

__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }

// Row blockIdx.y, tile blockIdx.x: r.N of `width` outputs by r.g, placed in their file by r.at; y = 0 behind them,
// and in the whole row where r.g.ok is false.
// BLOCKS (the windowed form) sums an output's taps in blocks of kAfTapBlock: each block from 0 by fmaf in ascending d,
// the block sums added in ascending order.  One chain of fmaf over 2 W + 2 taps loses accuracy as sqrt(taps) --
// 1.4e-6 against float64 at 100 : 1, 1216 taps, where float32 numpy's pairwise sum stays near 2e-7 -- and blocks of
// 128 hold it near 4e-7.  An output of at most kAfTapBlock taps (rate_in <= 10 rate_out) is ONE block, to which
// nothing is added: the bits of the one chain the other two forms keep at every ratio.
template <bool BLOCKS>
__device__ __forceinline__ void af_resample(const int16_t *__restrict__ pcm, const AfRow &r, int width,
                                            float *__restrict__ y, float2 *__restrict__ part) {
  __shared__ float win[kAfWin];
  __shared__ float red[2 * (kAfThreads / kWave)];
  const mvn_audio_clip &c = r.c;
  const AfGeom &g = r.g;
  const AfAt &at = r.at;
  const int b = blockIdx.y, tid = threadIdx.x, N = r.N;
  const int t0 = blockIdx.x * kAfTile, t1 = min(N, t0 + kAfTile);
  float *yb = y + (size_t)b * width;
  if (!g.ok) {  // (workgroup-uniform) nothing of the upload is read
    for (int k = t0 + tid; k < t1; k += kAfThreads) yb[k] = 0.f;
    if (tid == 0) part[(size_t)b * gridDim.x + blockIdx.x] = make_float2(0.f, 0.f);
    return;
  }
  // the silence behind the clip; a tile that holds nothing else ends here (workgroup-uniform)
  for (int k = max(N, t0) + tid; k < min(width, t0 + kAfTile); k += kAfThreads) yb[k] = 0.f;
  if (t0 >= N) return;
  const int16_t *src = pcm + c.offset;
  const int ch = c.channels, W = g.W;
  const float den = 32768.0f * (float)ch, s = g.s, fneu = (float)g.neu;
  const float kPi = 3.14159265358979323846f;
  float mn = INFINITY, mx = -INFINITY;
  for (int k0 = t0; k0 < t1; k0 += g.sub) {
    const int k1 = min(t1, k0 + g.sub);
    const long long lo = ((at.j0 + k0) * g.orig) / g.neu - W;
    const long long hi = ((at.j0 + (k1 - 1)) * g.orig) / g.neu + W + 1;
    const int len = (int)min(hi - lo + 1, (long long)kAfWin);  // (af_geom_taps sized sub so that the window fits)
    __syncthreads();  // the previous window has been consumed
    for (int j = tid; j < len; j += kAfThreads) {
      const long long i = lo + j;
      float v = 0.f;  // m[i] = 0 outside the file
      const long long is = i - at.first;  // its place in the upload: every read stays inside the span
      if (i >= 0 && is >= 0 && is < c.frames && i < at.file_frames) {
        int sum = 0;
        for (int q = 0; q < ch; ++q) sum += src[is * ch + q];
        v = (float)sum / den;
      }
      win[j] = v;
    }
    __syncthreads();
    for (int k = k0 + tid; k < k1; k += kAfThreads) {
      const long long p = (at.j0 + k) * g.orig;
      const long long i0 = p / g.neu;
      const float frac = (float)(p - i0 * g.neu) / fneu;
      const float *w = win + (int)(i0 - lo);
      float acc = 0.f, blocks = 0.f;
      for (int d = -W; d <= W + 1; ++d) {
        if (BLOCKS && d != -W && (d + W) % kAfTapBlock == 0) {  // a block is full
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
      if (BLOCKS && 2 * W + 2 > kAfTapBlock) acc = blocks + acc;
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

template <class Clip, bool BLOCKS>
__global__ __launch_bounds__(kAfThreads) void af_resample_kernel(const int16_t *__restrict__ pcm, long long pcm_len,
                                                                 const Clip *__restrict__ clips, int width,
                                                                 float *__restrict__ y, float2 *__restrict__ part) {
  const AfRow r = af_row(clips[blockIdx.y], pcm_len, width);
  af_resample<BLOCKS>(pcm, r, width, y, part);
}

// audio <- (audio - min) / (max - min); audio * 2 - 1 (dataset.py:271-275), a clip with max == min left as it is (the
// silent clip of the reference's `sum() == 0` test); then the mu-law of mu_law_encode_kernel, clamped to 0 .. Q-1
// (an un-normalised resample may overshoot [-1, 1]).
// The (min, max) is r.hi > r.lo where the row gives one (workgroup-uniform), else it runs over the tiles that hold the
// row's N outputs, of the `tiles` slots a row has; the columns behind them get the class mu-law gives 0.0.
//
// EMPH (mvn_audio_frontend_emph): what is quantised is the pre-emphasised row e[k] = (vn[k] - a vn[k-1]) / (1 + a) of
// af_emphasise, vn the value formed above for column k and vn[-1] = 0 -- the ROW's column 0 has no predecessor, a
// window's first column included.  Column k - 1 may lie in the previous tile: y is complete, it is read from there
// and normalised by the same expressions.  e goes to `emph` as well, 0 behind the row's N columns and in a refused
// row.  EMPH = false is the kernel as it was, instruction for instruction.
__device__ __forceinline__ float af_emphasise(float v, float prev, float a) {
#pragma clang fp contract(off)
  const float t = a * prev;
  return (v - t) / (1.0f + a);
}

template <bool EMPH>
__device__ __forceinline__ void af_quantise(const AfRow &r, int width, int Q, int normalize, int tiles,
                                            const float *__restrict__ y, const float2 *__restrict__ part,
                                            int32_t *__restrict__ idx, float a, float *__restrict__ emph) {
  __shared__ float red[2 * (kAfThreads / kWave)];
  const int b = blockIdx.y, tid = threadIdx.x, N = r.N;
  const int t0 = blockIdx.x * kAfTile, t1 = min(N, t0 + kAfTile);
  int32_t *ib = idx + (size_t)b * width;
  float *eb = EMPH ? emph + (size_t)b * width : nullptr;
  if (!r.g.ok) {
    for (int k = t0 + tid; k < t1; k += kAfThreads) {
      ib[k] = -1;
      if (EMPH) eb[k] = 0.f;
    }
    return;
  }
  const int silence = (int)((float)(Q - 1) / 2.0f + 0.5f);
  for (int k = max(N, t0) + tid; k < min(width, t0 + kAfTile); k += kAfThreads) {
    ib[k] = silence;
    if (EMPH) eb[k] = 0.f;
  }
  if (t0 >= N) return;  // (workgroup-uniform)
  const int own = (N + kAfTile - 1) / kAfTile;
  float mn = INFINITY, mx = -INFINITY;
  if (normalize && r.hi > r.lo) {
    mn = r.lo;
    mx = r.hi;
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
  const float *yb = y + (size_t)b * width;
  for (int k = t0 + tid; k < t1; k += kAfThreads) {
    float v = yb[k];
    if (scale) {
      v = (v - mn) / range;
      v = v * 2.0f - 1.0f;
    }
    if (EMPH) {
      float prev = k > 0 ? yb[k - 1] : 0.f;
      if (scale && k > 0) {
        prev = (prev - mn) / range;
        prev = prev * 2.0f - 1.0f;
      }
      v = af_emphasise(v, prev, a);
      eb[k] = v;
    }
    const float z = copysignf(log1pf(mu * fabsf(v)) / lmu, v);
    const int q = (int)((z + 1.0f) / 2.0f * mu + 0.5f);
    ib[k] = min(max(q, 0), Q - 1);
  }
}

template <class Clip>
__global__ __launch_bounds__(kAfThreads) void af_quantise_kernel(const Clip *__restrict__ clips, long long pcm_len,
                                                                 int width, int Q, int normalize, int tiles,
                                                                 const float *__restrict__ y,
                                                                 const float2 *__restrict__ part,
                                                                 int32_t *__restrict__ idx) {
  const AfRow r = af_row(clips[blockIdx.y], pcm_len, width);
  af_quantise<false>(r, width, Q, normalize, tiles, y, part, idx, 0.f, nullptr);
}

template <class Clip>
__global__ __launch_bounds__(kAfThreads) void af_quantise_emph_kernel(const Clip *__restrict__ clips, long long pcm_len,
                                                                      int width, int Q, int normalize, int tiles,
                                                                      const float *__restrict__ y,
                                                                      const float2 *__restrict__ part,
                                                                      int32_t *__restrict__ idx, float a,
                                                                      float *__restrict__ emph) {
  const AfRow r = af_row(clips[blockIdx.y], pcm_len, width);
  af_quantise<true>(r, width, Q, normalize, tiles, y, part, idx, a, emph);
}

// The entry points: `what` is the entry point's name without its mvn_ prefix.  `emph` non-null (mvn_audio_frontend_emph):
// the second launch is the pre-emphasising quantise kernel with coefficient `a`; null: the two launches as they were.
template <class Clip, bool BLOCKS>
static int audio_frontend_launch(const char *what, const int16_t *pcm, long long pcm_len, const Clip *clips, int batch,
                                 int classes, int width, int normalize, float *y, float *scratch, int32_t *index,
                                 void *stream, float a = 0.f, float *emph = nullptr) {
  if (!pcm || !clips || !y || !scratch || !index || pcm_len < 1 || batch < 1 || batch > 65535 || width < 1 ||
      classes < 2 || classes > 65536) {
    set_error("mvn_%s: bad argument", what);
    return MVN_ERR_BAD_ARG;
  }
  if (((uintptr_t)scratch & 7u) != 0) {
    set_error("mvn_%s: scratch must be 8-byte aligned", what);
    return MVN_ERR_BAD_ARG;
  }
  const int tiles = (width + kAfTile - 1) / kAfTile;
  const dim3 grid(tiles, batch);
  hipLaunchKernelGGL((af_resample_kernel<Clip, BLOCKS>), grid, dim3(kAfThreads), 0, (hipStream_t)stream, pcm, pcm_len,
                     clips, width, y, (float2 *)scratch);
  int rc = check_hip(hipGetLastError(), (std::string(what) + " (resample)").c_str());
  if (rc) return rc;
  if (emph)
    hipLaunchKernelGGL((af_quantise_emph_kernel<Clip>), grid, dim3(kAfThreads), 0, (hipStream_t)stream, clips, pcm_len,
                       width, classes, normalize, tiles, (const float *)y, (const float2 *)scratch, index, a, emph);
  else
    hipLaunchKernelGGL((af_quantise_kernel<Clip>), grid, dim3(kAfThreads), 0, (hipStream_t)stream, clips, pcm_len,
                       width, classes, normalize, tiles, (const float *)y, (const float2 *)scratch, index);
  return check_hip(hipGetLastError(), (std::string(what) + " (quantise)").c_str());
}

// ---- finished samples to 16-bit PCM (mvn_pcm16_chunk) ----------------------------------------------------------------
// Class q of column t0 + j of row b -> pcm[b pcm_stride + j]: the mu-law expansion of mu_law_decode_kernel (its float
// expression, so its bits), then what the sample logger's WAV writer does to that float in float64 numpy: clip to
// [-1, 1], times 32767, round half to even.  The value depends on the class alone; a class outside [0, Q) is clamped,
// as the generators clamp a pick.
//
// A pure stream.  Thread i of a row owns the four columns h + 4 i .. h + 4 i + 3, h = 1 where the row's first PCM
// element sits on an odd int16 (so that every quad starts on 4 bytes): one 16-byte load of the int32 columns (they are
// only 4-byte aligned: the load is typed so), two int16 pairs packed into one 8-byte store (typed as 4-byte aligned).
// The thread behind the last full quad writes what is left -- the head column where h = 1 and up to three tail
// columns: a packed pair where two are left, single int16 stores otherwise.  Nothing outside [0, n) of a row is read
// or written.
constexpr int kPcmThreads = 256;

typedef int32_t pcm_i32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t pcm_u32x2 __attribute__((ext_vector_type(2), aligned(4)));

// the float mu_law_decode_kernel gives for class q, clamped to [0, Q)
__device__ __forceinline__ float pcm_decode(int q, int Q, float mu, float lmu) {
  q = min(max(q, 0), Q - 1);
  const float y = ((float)q / mu) * 2.0f - 1.0f;  // (the expression of mu_law_decode_kernel)
  return copysignf((expf(fabsf(y) * lmu) - 1.0f) / mu, y);
}

__device__ __forceinline__ uint32_t pcm16_round(double x) {
  const double v = fmin(fmax(x, -1.0), 1.0) * 32767.0;
  return (uint32_t)(uint16_t)(int16_t)(int)rint(v);  // rint: half to even, as numpy's round
}

__device__ __forceinline__ uint32_t pcm16_of(int q, int Q, float mu, float lmu) {
  return pcm16_round((double)pcm_decode(q, Q, mu, lmu));
}

__global__ __launch_bounds__(kPcmThreads) void pcm16_chunk_kernel(const int32_t *__restrict__ samples, int batch,
                                                                  int sample_stride, int t0, int n, int Q,
                                                                  int16_t *__restrict__ pcm, int pcm_stride) {
  const float mu = (float)(Q - 1), lmu = log1pf(mu);
  const int i = blockIdx.x * kPcmThreads + threadIdx.x;
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const int32_t *src = samples + (size_t)b * sample_stride + t0;
    int16_t *dst = pcm + (size_t)b * pcm_stride;
    const int h = (int)(((uintptr_t)dst >> 1) & 1u);  // n >= 1 here: the head column exists
    const int quads = (n - h) / 4;
    if (i < quads) {
      const int c = h + 4 * i;
      const pcm_i32x4 q = *(const pcm_i32x4 *)(src + c);
      pcm_u32x2 w;
      w.x = pcm16_of(q.x, Q, mu, lmu) | (pcm16_of(q.y, Q, mu, lmu) << 16);
      w.y = pcm16_of(q.z, Q, mu, lmu) | (pcm16_of(q.w, Q, mu, lmu) << 16);
      *(pcm_u32x2 *)(dst + c) = w;
    } else if (i == quads) {
      if (h) dst[0] = (int16_t)pcm16_of(src[0], Q, mu, lmu);
      int c = h + 4 * quads;  // 0 .. 3 columns left, the first of them on 4 bytes
      if (n - c >= 2) {
        *(uint32_t *)(dst + c) = pcm16_of(src[c], Q, mu, lmu) | (pcm16_of(src[c + 1], Q, mu, lmu) << 16);
        c += 2;
      }
      if (c < n) dst[c] = (int16_t)pcm16_of(src[c], Q, mu, lmu);
    }
  }
}

// ---- ... through the de-emphasis filter (mvn_pcm16_deemph_chunk) ----------------------------------------------------
// The inverse of the front end's pre-emphasis, fused into the conversion: with x the float of pcm_decode, per row and
// in column order, in double,
//   y = ((1 + a) x) + (a y_prev),   pcm = pcm16_round(y),   y_prev = y
// two products and a sum, each rounded once (no fma), y_prev from state[b] at entry and back there at exit.  The
// recurrence is DEFINED sequentially, so that the bits do not depend on how a clip is cut into chunks; it is therefore
// run sequentially -- no scan, which would round differently.  One wave per row.  Per 64 columns every lane decodes its
// own column (expf and the product by 1 + a: the expensive part, in parallel), then the wave walks the 64 columns
// together: it reads lane j's product with a cross-lane read and every lane forms the same y (a product and a sum in
// the dependent chain), lane j keeping it for its column.  The next 64 classes are loaded before the walk.  A column
// is stored as one int16, whatever the row's alignment.  Nothing outside [0, n) of a row is read or written.
__device__ __forceinline__ double wave_read(double v, int lane) {  // (lane: wave-uniform)
  const long long u = __double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)u, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(u >> 32), lane);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__global__ __launch_bounds__(kWave) void pcm16_deemph_chunk_kernel(const int32_t *__restrict__ samples, int batch,
                                                                   int sample_stride, int t0, int n, int Q, double a,
                                                                   double *__restrict__ state,
                                                                   int16_t *__restrict__ pcm, int pcm_stride) {
#pragma clang fp contract(off)
  const float mu = (float)(Q - 1), lmu = log1pf(mu);
  const double gain = 1.0 + a;
  const int lane = threadIdx.x;
  for (int b = blockIdx.x; b < batch; b += gridDim.x) {
    const int32_t *src = samples + (size_t)b * sample_stride + t0;
    int16_t *dst = pcm + (size_t)b * pcm_stride;
    double prev = state[b];
    int q = lane < n ? src[lane] : 0;
    for (int c0 = 0; c0 < n; c0 += kWave) {
      const int m = min(n - c0, kWave), c = c0 + lane;
      const int q_next = c + kWave < n ? src[c + kWave] : 0;
      const double xs = gain * (double)pcm_decode(q, Q, mu, lmu);
      double mine = 0.0;
#pragma unroll
      for (int j = 0; j < kWave; ++j) {
        if (j >= m) break;  // (wave-uniform)
        const double fed = a * prev;
        prev = wave_read(xs, j) + fed;
        if (lane == j) mine = prev;
      }
      if (lane < m) dst[c] = (int16_t)pcm16_round(mine);
      q = q_next;
    }
    if (lane == 0) state[b] = prev;
  }
}

}  // namespace mvn

// what mvn_pcm16_chunk and mvn_pcm16_deemph_chunk refuse alike; `what` is the entry point's name
static int pcm16_check(const char *what, const int32_t *samples, int batch, int sample_stride, int t0, int n,
                       int classes, const int16_t *pcm, int pcm_stride) {
  if (!samples || !pcm) {
    mvn::set_error("%s: bad argument (NULL samples or pcm)", what);
    return MVN_ERR_BAD_ARG;
  }
  if (batch < 1 || n < 0 || t0 < 0 || (long long)t0 + (long long)n > (long long)sample_stride || pcm_stride < n) {
    mvn::set_error("%s: bad argument (batch %d, t0 %d, n %d, sample_stride %d, pcm_stride %d)", what, batch, t0, n,
                   sample_stride, pcm_stride);
    return MVN_ERR_BAD_ARG;
  }
  if (classes < 2 || classes > 32768) {
    mvn::set_error("%s: bad argument (classes %d outside 2 .. 32768)", what, classes);
    return MVN_ERR_BAD_ARG;
  }
  return MVN_OK;
}

extern "C" {

int mvn_pcm16_chunk(const int32_t *samples, int batch, int sample_stride, int t0, int n, int classes, int16_t *pcm,
                    int pcm_stride, void *stream) {
  const int rc = pcm16_check("mvn_pcm16_chunk", samples, batch, sample_stride, t0, n, classes, pcm, pcm_stride);
  if (rc) return rc;
  if (n == 0) return MVN_OK;
  const int threads = n / 4 + 1;  // one per quad and the one behind them
  const dim3 grid((threads + mvn::kPcmThreads - 1) / mvn::kPcmThreads, batch < 65535 ? batch : 65535);
  hipLaunchKernelGGL(mvn::pcm16_chunk_kernel, grid, dim3(mvn::kPcmThreads), 0, (hipStream_t)stream, samples, batch,
                     sample_stride, t0, n, classes, pcm, pcm_stride);
  return mvn::check_hip(hipGetLastError(), "pcm16_chunk");
}

int mvn_pcm16_deemph_chunk(const int32_t *samples, int batch, int sample_stride, int t0, int n, int classes, float coef,
                           double *state, int16_t *pcm, int pcm_stride, void *stream) {
  const int rc = pcm16_check("mvn_pcm16_deemph_chunk", samples, batch, sample_stride, t0, n, classes, pcm, pcm_stride);
  if (rc) return rc;
  if (!state || ((uintptr_t)state & 7u) != 0) {
    mvn::set_error("mvn_pcm16_deemph_chunk: bad argument (state NULL or not 8-byte aligned)");
    return MVN_ERR_BAD_ARG;
  }
  if (!(coef >= 0.0f && coef < 1.0f)) {  // (a NaN fails both)
    mvn::set_error("mvn_pcm16_deemph_chunk: bad argument (coef %g outside [0, 1))", (double)coef);
    return MVN_ERR_BAD_ARG;
  }
  if (n == 0) return MVN_OK;
  hipLaunchKernelGGL(mvn::pcm16_deemph_chunk_kernel, dim3(batch), dim3(mvn::kWave), 0, (hipStream_t)stream, samples,
                     batch, sample_stride, t0, n, classes, (double)coef, state, pcm, pcm_stride);
  return mvn::check_hip(hipGetLastError(), "pcm16_deemph_chunk");
}

size_t mvn_audio_frontend_scratch_floats(int batch, int n_out) {
  if (batch < 1 || n_out < 1) return 0;
  return 2 * (size_t)batch * (size_t)((n_out + mvn::kAfTile - 1) / mvn::kAfTile);
}

int mvn_audio_frontend(const int16_t *pcm, long long pcm_len, const mvn_audio_clip *clips, int batch, int classes,
                       int n_out, int normalize, float *y, float *scratch, int32_t *index, void *stream) {
  return mvn::audio_frontend_launch<mvn_audio_clip, false>("audio_frontend", pcm, pcm_len, clips, batch, classes,
                                                           n_out, normalize, y, scratch, index, stream);
}

size_t mvn_audio_frontend_var_scratch_floats(int batch, int width) {
  return mvn_audio_frontend_scratch_floats(batch, width);
}

int mvn_audio_frontend_var(const int16_t *pcm, long long pcm_len, const mvn_audio_clip_var *clips, int batch,
                           int classes, int width, int normalize, float *y, float *scratch, int32_t *index,
                           void *stream) {
  return mvn::audio_frontend_launch<mvn_audio_clip_var, false>("audio_frontend_var", pcm, pcm_len, clips, batch,
                                                               classes, width, normalize, y, scratch, index, stream);
}

size_t mvn_audio_frontend_window_scratch_floats(int batch, int width) {
  return mvn_audio_frontend_scratch_floats(batch, width);
}

int mvn_audio_frontend_window(const int16_t *pcm, long long pcm_len, const mvn_audio_clip_window *clips, int batch,
                              int classes, int width, int normalize, float *y, float *scratch, int32_t *index,
                              void *stream) {
  return mvn::audio_frontend_launch<mvn_audio_clip_window, true>("audio_frontend_window", pcm, pcm_len, clips, batch,
                                                                 classes, width, normalize, y, scratch, index, stream);
}

int mvn_audio_frontend_emph(int form, const int16_t *pcm, long long pcm_len, const void *clips, int batch, int classes,
                            int width, int normalize, float coef, float *y, float *scratch, int32_t *index,
                            float *emph, void *stream) {
  if (!emph || !(coef >= 0.0f && coef < 1.0f)) {  // (a NaN fails both)
    mvn::set_error("mvn_audio_frontend_emph: bad argument (emph NULL, or coef %g outside [0, 1))", (double)coef);
    return MVN_ERR_BAD_ARG;
  }
  switch (form) {
    case MVN_AUDIO_FORM_CLIP:
      return mvn::audio_frontend_launch<mvn_audio_clip, false>("audio_frontend_emph", pcm, pcm_len,
                                                               (const mvn_audio_clip *)clips, batch, classes, width,
                                                               normalize, y, scratch, index, stream, coef, emph);
    case MVN_AUDIO_FORM_VAR:
      return mvn::audio_frontend_launch<mvn_audio_clip_var, false>("audio_frontend_emph", pcm, pcm_len,
                                                                   (const mvn_audio_clip_var *)clips, batch, classes,
                                                                   width, normalize, y, scratch, index, stream, coef,
                                                                   emph);
    case MVN_AUDIO_FORM_WINDOW:
      return mvn::audio_frontend_launch<mvn_audio_clip_window, true>("audio_frontend_emph", pcm, pcm_len,
                                                                     (const mvn_audio_clip_window *)clips, batch,
                                                                     classes, width, normalize, y, scratch, index,
                                                                     stream, coef, emph);
  }
  mvn::set_error("mvn_audio_frontend_emph: bad argument (form %d)", form);
  return MVN_ERR_BAD_ARG;
}

}  // extern "C"
