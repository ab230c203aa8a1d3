// The loader's video front end (movenet/dataset.py:292-310 behind the decoder): uint8 frames of any resolution, RGB or
// gray, of a batch of clips in one upload -> (B, n, 64, 64) uint8 gray levels, in one kernel.
//
// Per frame: L = uint8(0.2989 r + 0.587 g + 0.114 b) (fp32 products and sums, each rounded, the cast truncating), then
// the bilinear resize of torch.nn.functional.interpolate(L.float(), (64, 64), align_corners=False, antialias=A),
// rounded half to even.  Without antialias output i reads source position (i + 0.5) in/out - 0.5 (clamped at 0) and its
// right neighbour; with it, a triangle filter of half-width max(in/out, 1) around (i + 0.5) in/out, the taps clipped to
// the image and the weights normalised by their sum.  Both passes are evaluated in fp64 (positions, weights and sums):
// the level is then the rounding of the exact value to ~1e-12, which lies inside what torch's own fp32 evaluation
// deviates from its fp64 one, and every case whose weights are exact in fp32 (identity, 2:1, 4:1) gives torch's bytes.
//
// One workgroup (4 waves) per (clip, frame, band of kVfBand output rows).  A wave takes a source row of the band: it
// loads the row 16 bytes per lane from 4-byte-aligned addresses (row pitch is W channels bytes, unpadded, and clip
// offsets are arbitrary, so the bytes are funnel-shifted into place; the first and last bytes of the upload come through
// bounded byte loads), converts it to gray bytes in a wave-private LDS row, and its 64 lanes -- one per output column --
// run the horizontal taps from there into the fp64 LDS tile (source row, 64).  The vertical taps run from the tile, a
// thread per output pixel, the band's source rows taken kVfRows at a time; the sum walks the taps in ascending order
// whatever the chunking, so there are no atomics and two launches give the same bytes.  Without antialias only the two
// source rows of each output row are read.
//
// Descriptors are device data and are checked here: a clip whose span [offset, offset + n H W channels) does not lie
// inside [0, pix_len), whose channels is not 1 or 3, or whose H or W is outside [1, 4096], is not read at all; its
// status is non-zero and its levels are zero.
#include "common.h"

namespace mvn {

constexpr int kVfOut = 64;       // output rows and columns
constexpr int kVfBand = 4;       // output rows per workgroup: kVfBand x 64 outputs, one per thread
constexpr int kVfThreads = kVfBand * kVfOut;
constexpr int kVfWaves = kVfThreads / kWave;
constexpr int kVfRows = 64;      // source rows per tile: 64 x 64 fp64 = 32 KiB
constexpr int kVfMaxDim = 4096;  // H, W limit: a gray row fits kVfRowBytes
constexpr int kVfRowBytes = kVfMaxDim + 16;  // (12-byte groups of a gray source row round up past 4096)

// One axis of the resize for one output index: taps [lo, lo + n) of the source, weight of tap k by vf_weight.
struct VfAxis {
  int lo, n;
  double center, invscale, norm;  // antialias: w_k = max(0, 1 - |(k + lo - center + 0.5) invscale|) norm
  double l1;                      // no antialias: w_0 = 1 - l1, w_1 = l1 (n == 1 where the neighbour is clamped)
};

__device__ __forceinline__ double vf_tri(const VfAxis &a, int k) {
  const double x = fabs(((double)(k + a.lo) - a.center + 0.5) * a.invscale);
  return x < 1.0 ? 1.0 - x : 0.0;
}

__device__ __forceinline__ double vf_weight(const VfAxis &a, int k, int antialias) {
  if (antialias) return vf_tri(a, k) * a.norm;
  return k == 0 ? 1.0 - a.l1 : a.l1;
}

__device__ __forceinline__ VfAxis vf_axis(int i, int in, int antialias) {
  VfAxis a;
  const double scale = (double)in / (double)kVfOut;
  a.center = a.invscale = a.norm = a.l1 = 0.0;
  if (antialias) {
    const double support = scale >= 1.0 ? scale : 1.0;
    a.invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
    a.center = scale * ((double)i + 0.5);
    const long long lo = max((long long)(a.center - support + 0.5), 0LL);
    const long long hi = min((long long)(a.center + support + 0.5), (long long)in);
    a.lo = (int)lo;
    a.n = (int)(hi - lo);
    double total = 0.0;
    for (int k = 0; k < a.n; ++k) total += vf_tri(a, k);
    a.norm = total != 0.0 ? 1.0 / total : 1.0;
  } else {
    double src = scale * ((double)i + 0.5) - 0.5;
    if (src < 0.0) src = 0.0;
    a.lo = min((int)src, in - 1);
    a.n = a.lo < in - 1 ? 2 : 1;
    a.l1 = fmin(fmax(src - (double)a.lo, 0.0), 1.0);
    if (a.n == 1) a.l1 = 0.0;  // (torch reads the same pixel twice with weights summing to 1)
  }
  return a;
}

// 0: the clip is read; otherwise why it is not.
__device__ __forceinline__ int vf_check(const mvn_video_clip &c, long long pix_len, int n_frames) {
  if (c.channels != 1 && c.channels != 3) return 2;
  if (c.height < 1 || c.height > kVfMaxDim || c.width < 1 || c.width > kVfMaxDim) return 3;
  const long long span = (long long)n_frames * c.height * c.width * c.channels;  // (< 2^31 x 2^26: no overflow)
  if (c.offset < 0 || span > pix_len || c.offset > pix_len - span) return 1;
  return 0;
}

// The 12 bytes pix[p .. p + 12) as three little-endian words; bytes at or past `end` (<= pix_len) come back as
// anything that may be read.  Nothing outside [0, pix_len) is touched.
__device__ __forceinline__ void vf_load12(const uint8_t *__restrict__ pix, long long pix_len, long long p,
                                          long long end, uint32_t (&out)[3]) {
  const uintptr_t addr = (uintptr_t)(pix + p);
  const unsigned m = (unsigned)(addr & 3u);
  if (p - (long long)m >= 0 && p - (long long)m + 16 <= pix_len) {
    const uint32_t *w = (const uint32_t *)(pix + (p - (long long)m));  // 4-byte aligned, 16 bytes inside the upload
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    out[0] = __builtin_amdgcn_alignbyte(w1, w0, m);
    out[1] = __builtin_amdgcn_alignbyte(w2, w1, m);
    out[2] = __builtin_amdgcn_alignbyte(w3, w2, m);
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      uint32_t v = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const long long q = p + 4 * i + b;
        if (q < end) v |= (uint32_t)pix[q] << (8 * b);
      }
      out[i] = v;
    }
  }
}

// rgb_to_grayscale on uint8: separate fp32 multiplies and adds, left to right, truncated (never fused: a fused form
// changes the level of some triples).
__device__ __forceinline__ uint32_t vf_gray(uint32_t r, uint32_t g, uint32_t b) {
  const float s = __fadd_rn(__fadd_rn(__fmul_rn(0.2989f, (float)r), __fmul_rn(0.587f, (float)g)),
                            __fmul_rn(0.114f, (float)b));
  return (uint32_t)(int)s;
}

__global__ __launch_bounds__(kVfThreads) void vf_kernel(const uint8_t *__restrict__ pix, long long pix_len,
                                                        const mvn_video_clip *__restrict__ clips, int n_frames,
                                                        int antialias, uint8_t *__restrict__ levels,
                                                        int32_t *__restrict__ status) {
  __shared__ double tile[kVfRows * kVfOut];
  __shared__ uint32_t grow[kVfWaves][kVfRowBytes / 4];
  constexpr int kBands = kVfOut / kVfBand;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int band = blockIdx.x % kBands;
  const long long cf = blockIdx.x / kBands;  // clip n_frames + frame
  const int clip = (int)(cf / n_frames), frame = (int)(cf % n_frames);
  const mvn_video_clip c = clips[clip];
  const int bad = vf_check(c, pix_len, n_frames);
  uint8_t *out = levels + ((size_t)cf * kVfOut + (size_t)band * kVfBand) * kVfOut;  // the band's kVfBand x 64 bytes
  if (frame == 0 && band == 0 && tid == 0) status[clip] = bad;
  if (bad) {  // (workgroup-uniform) nothing of the upload is read
    out[tid] = 0;
    return;
  }
  const int H = c.height, W = c.width, ch = c.channels;
  const long long pitch = (long long)W * ch;
  const long long base = c.offset + (long long)frame * H * pitch;  // the frame's first byte
  const int groups = (int)((pitch + 11) / 12);                     // 12-byte groups of a row: 4 RGB or 12 gray pixels

  const VfAxis ax = vf_axis(lane, W, antialias);               // this lane's output column (the same in every wave)
  const VfAxis ay = vf_axis(band * kVfBand + wave, H, antialias);  // this thread's output row
  // the band's source rows: with antialias the contiguous range of its rows' taps, kVfRows at a time; without, slot
  // 2 r + t is tap t of output row r
  const VfAxis first = vf_axis(band * kVfBand, H, antialias), last = vf_axis(band * kVfBand + kVfBand - 1, H, antialias);
  const int y_lo = first.lo, y_hi = antialias ? last.lo + last.n : 0;
  const int n_chunks = antialias ? (y_hi - y_lo + kVfRows - 1) / kVfRows : 1;
  double acc = 0.0;
  for (int chunk = 0; chunk < n_chunks; ++chunk) {
    const int c_lo = y_lo + chunk * kVfRows;
    const int n_slots = antialias ? min(kVfRows, y_hi - c_lo) : 2 * kVfBand;
    if (chunk) __syncthreads();  // the previous tile has been consumed
    for (int s0 = 0; s0 < n_slots; s0 += kVfWaves) {
      const int slot = s0 + wave;
      int y = -1;  // (wave-uniform)
      if (slot < n_slots) {
        if (antialias) {
          y = c_lo + slot;
        } else {
          const VfAxis r = vf_axis(band * kVfBand + (slot >> 1), H, 0);
          y = (slot & 1) < r.n ? r.lo + (slot & 1) : -1;
        }
      }
      if (y >= 0) {
        const long long row = base + (long long)y * pitch, end = row + pitch;
        for (int q = lane; q < groups; q += kWave) {
          uint32_t w[3];
          vf_load12(pix, pix_len, row + 12LL * q, end, w);
          if (ch == 3) {
            const uint32_t g0 = vf_gray(w[0] & 255u, (w[0] >> 8) & 255u, (w[0] >> 16) & 255u);
            const uint32_t g1 = vf_gray(w[0] >> 24, w[1] & 255u, (w[1] >> 8) & 255u);
            const uint32_t g2 = vf_gray((w[1] >> 16) & 255u, w[1] >> 24, w[2] & 255u);
            const uint32_t g3 = vf_gray((w[2] >> 8) & 255u, (w[2] >> 16) & 255u, w[2] >> 24);
            grow[wave][q] = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
          } else {
            grow[wave][3 * q] = w[0];
            grow[wave][3 * q + 1] = w[1];
            grow[wave][3 * q + 2] = w[2];
          }
        }
      }
      __syncthreads();  // the gray rows are written
      if (y >= 0) {
        const uint8_t *g = (const uint8_t *)grow[wave];
        double h = 0.0;
        for (int k = 0; k < ax.n; ++k) h += (double)g[ax.lo + k] * vf_weight(ax, k, antialias);
        tile[slot * kVfOut + lane] = h;
      }
      __syncthreads();  // ... and read: the next rows may overwrite them
    }
    // vertical taps of this chunk, ascending
    if (antialias) {
      const int k0 = max(0, c_lo - ay.lo), k1 = min(ay.n, c_lo + n_slots - ay.lo);
      for (int k = k0; k < k1; ++k) acc += tile[(ay.lo + k - c_lo) * kVfOut + lane] * vf_weight(ay, k, 1);
    } else {
      for (int k = 0; k < ay.n; ++k) acc += tile[(2 * wave + k) * kVfOut + lane] * vf_weight(ay, k, 0);
    }
  }
  const double v = fmin(fmax(rint(acc), 0.0), 255.0);  // rint: half to even
  out[tid] = (uint8_t)(int)v;
}

}  // namespace mvn

extern "C" {

int mvn_video_frontend(const uint8_t *pix, long long pix_len, const mvn_video_clip *clips, int batch, int n_frames,
                       int antialias, uint8_t *levels, int32_t *status, void *stream) {
  if (!pix || !clips || !levels || !status) {
    mvn::set_error("mvn_video_frontend: bad argument (a null pointer)");
    return MVN_ERR_BAD_ARG;
  }
  if (pix_len < 0 || batch < 0 || n_frames < 1) {
    mvn::set_error("mvn_video_frontend: bad argument (pix_len %lld, batch %d, n_frames %d)", pix_len, batch, n_frames);
    return MVN_ERR_BAD_ARG;
  }
  if (antialias != 0 && antialias != 1) {
    mvn::set_error("mvn_video_frontend: bad argument (antialias must be 0 or 1, got %d)", antialias);
    return MVN_ERR_BAD_ARG;
  }
  if (batch == 0) return MVN_OK;
  const long long blocks = (long long)batch * n_frames * (mvn::kVfOut / mvn::kVfBand);
  if (blocks > 0x7FFFFFFFLL) {
    mvn::set_error("mvn_video_frontend: bad argument (%d clips x %d frames exceed one launch's grid)", batch, n_frames);
    return MVN_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(mvn::vf_kernel, dim3((unsigned)blocks), dim3(mvn::kVfThreads), 0, (hipStream_t)stream, pix,
                     pix_len, clips, n_frames, antialias, levels, status);
  return mvn::check_hip(hipGetLastError(), "video_frontend");
}

}  // extern "C"
