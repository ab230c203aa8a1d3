// The five building blocks as calls of their own (mvn_block_*): CausalConv1d, DilatedCausalConv1d,
// GatedResidualConv1d and DenseConv of movenet/modules.py, forward and backward, on tensors the CALLER lays out
// (pointer, row stride, length: any ld >= len, any 4-byte alignment -- a PyTorch-contiguous (B, C, T) with odd T goes in
// as it is).  ResidualConvStack is the gated layer called per layer by the host.
//
// Two forms (mvn_block_last_form):
//   GENERIC  any dims within MVN_GEN_GENERIC's limits.  Every product is one launch of gemm_wx_kernel (fp32 MFMAs) or
//            wgrad2_kernel + slab_reduce_kernel (three-plane bf16 split, per-workgroup slabs summed in a fixed order) of
//            gemm_family.h with the two Op structs below, which describe operands as SEGMENTS of rows: a tensor, a
//            column shift and the column range in which the shifted tensor exists.  A two-tap product is the segments
//            x(j) and x(j + d); the right-aligned slices of the reference (input[:, :, -n:], skip[:, :, -s:], the last
//            n columns of a context) are shifts, never copies.  The gate and its derivative are element-wise kernels.
//   FUSED64  the gated layer's FORWARD at C = K = 64: one kernel per layer (gated64_fused_kernel), z never leaves the CU.
//            Its backward is composed from the generic family.
// No float atomics anywhere: parameter gradients accumulate by one read-modify-write per word, after a fixed-order sum.
#include "gemm_family.h"

namespace mvn {

// ---------------------------------------------------------------------------------------------------------------
// operand segments
// ---------------------------------------------------------------------------------------------------------------
struct BSeg {  // rows [0, rows) of a (B, rows, ld) tensor; value at column t is p[t + shift], zero outside [lo, hi)
  const float *p, *p2;  // p2: second factor (z = tanh * sigmoid), same geometry
  long long sb;
  int ld, rows, shift, lo, hi, lrelu;  // lrelu: leaky-ReLU applied to the value
};
struct BWEnt {  // a weight block: W(row, col) = p[row * rs + col * cs]; p == NULL: zero / not wanted
  float *p;
  int rs, cs;
};
struct BOut {  // output rows of a product
  int rows;
  float *out;  // out[t + oshift] for t in [olo, ohi)
  long long osb;
  int old, oshift, olo, ohi;
  const float *b0, *b1;  // biases (NULL: none)
  BSeg add;              // added in (the residual connection); add.p == NULL: nothing
  BSeg der;              // result multiplied by leaky-ReLU'(der); der.p == NULL: nothing
};

__device__ __forceinline__ float bseg_value(const BSeg &s, int b, int r, int t) {
  const int tc = max(min(t, s.hi - 1), s.lo);  // (an empty range has lo = hi = shift = 0: column 0 exists)
  const size_t o = (size_t)b * s.sb + (size_t)r * s.ld + (tc + s.shift);
  float v = s.p[o];
  if (s.p2) v *= s.p2[o];
  if (s.lrelu) v = leaky(v);
  return (t >= s.lo && t < s.hi) ? v : 0.f;
}

// Y = W X over time for gemm_wx_kernel: X rows are up to four segments one after the other along k, Y rows up to two
struct BlkGemmOp {
  int K, t_begin, t_end;
  BSeg xs[4];
  int xend[4];  // running row totals of xs
  BOut ms[2];
  BWEnt wt[2][4];
  __device__ __forceinline__ void find_k(int k, int &si, int &kr) const {
    si = 0;
    kr = k;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (k >= xend[i]) {
        si = i + 1;
        kr = k - xend[i];
      }
  }
  __device__ __forceinline__ float w(int m, int k) const {
    if (k >= K) return 0.f;
    const int mi = m >= ms[0].rows ? 1 : 0, row = m - (mi ? ms[0].rows : 0);
    if (row >= ms[mi].rows) return 0.f;
    int si, kr;
    find_k(k, si, kr);
    const BWEnt e = wt[mi][si];
    return e.p ? e.p[(size_t)row * e.rs + (size_t)kr * e.cs] : 0.f;
  }
  __device__ __forceinline__ float x(int b, int k, int t) const {
    if (k >= K || t >= t_end) return 0.f;
    int si, kr;
    find_k(k, si, kr);
    return bseg_value(xs[si], b, kr, t);
  }
  __device__ __forceinline__ void store(int b, int m, int t, float v) const {
    const int mi = m >= ms[0].rows ? 1 : 0, row = m - (mi ? ms[0].rows : 0);
    const BOut &o = ms[mi];
    if (row >= o.rows || t < o.olo || t >= o.ohi) return;
    if (o.b0) v += o.b0[row];
    if (o.b1) v += o.b1[row];
    if (o.add.p) v += bseg_value(o.add, b, row, t);
    if (o.der.p) v *= bseg_value(o.der, b, row, t) > 0.f ? 1.0f : kLeakySlope;
    o.out[(size_t)b * o.osb + (size_t)row * o.old + (t + o.oshift)] = v;
  }
  __device__ __forceinline__ void epilogue(int b, int mb, int t, int lane, const f32x16 &a0, const f32x16 &a1) const {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = mb * 64 + acc_row(r, lane);
      store(b, m, t, a0[r]);
      store(b, m + 32, t, a1[r]);
    }
  }
};

// dW = A X^T over time for wgrad2_kernel (slab form): A rows up to two segments, X rows up to four.  Rows past the
// segments (the kernel's 128 / 64-row blocks) are absent A rows (range empty) or X rows that read the `safe` row --
// a row that exists over all of [0, t_end) -- and whose products slab_reduce_kernel drops (dw == NULL).
template <bool PRODUCT>
struct BlkWgOp {
  int t_begin, t_end, lrelu;
  BSeg as[2], xs[4];
  int xend[4];
  BWEnt dwt[2][4];
  float *dbv[2][2];  // up to two bias gradients per A segment take the same row sums (filter bias, context bias)
  const float *safe;
  long long safe_sb;
  static constexpr bool X_PRODUCT = PRODUCT;
  static constexpr bool HAS_BIAS = true;
  static constexpr bool X_ABSENT_ROWS = false;
  __device__ __forceinline__ float xmap(float v) const { return lrelu ? leaky(v) : v; }
  __device__ __forceinline__ bool find_a(int m, int &ai, int &row) const {
    ai = m >= as[0].rows ? 1 : 0;
    row = m - (ai ? as[0].rows : 0);
    return row < as[ai].rows;
  }
  __device__ __forceinline__ bool find_x(int n, int &si, int &row) const {
    si = 0;
    row = n;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (n >= xend[i]) {
        si = i + 1;
        row = n - xend[i];
      }
    return n < xend[3];
  }
  __device__ __forceinline__ const float *a_ptr(int b, int m) const {
    int ai, row;
    if (!find_a(m, ai, row)) return safe + (size_t)b * safe_sb;
    const BSeg &s = as[ai];
    return s.p + (size_t)b * s.sb + (size_t)row * s.ld + s.shift;
  }
  __device__ __forceinline__ int a_lo(int m) const {
    int ai, row;
    return find_a(m, ai, row) ? as[ai].lo : 0;
  }
  __device__ __forceinline__ int a_hi(int m) const {
    int ai, row;
    return find_a(m, ai, row) ? as[ai].hi : 0;
  }
  __device__ __forceinline__ const float *x_ptr(int b, int n) const {
    int si, row;
    if (!find_x(n, si, row)) return safe + (size_t)b * safe_sb;
    const BSeg &s = xs[si];
    return s.p + (size_t)b * s.sb + (size_t)row * s.ld + s.shift;
  }
  __device__ __forceinline__ const float *x_ptr2(int b, int n) const {
    int si, row;
    if (!find_x(n, si, row)) return safe + (size_t)b * safe_sb;
    const BSeg &s = xs[si];
    return s.p2 + (size_t)b * s.sb + (size_t)row * s.ld + s.shift;
  }
  __device__ __forceinline__ int x_lo(int n) const {
    int si, row;
    return find_x(n, si, row) ? xs[si].lo : t_begin;
  }
  __device__ __forceinline__ int x_hi(int n) const {
    int si, row;
    return find_x(n, si, row) ? xs[si].hi : t_end;
  }
  __device__ __forceinline__ float *dw(int m, int n) const {
    int ai, ar, si, xr;
    if (!find_a(m, ai, ar) || !find_x(n, si, xr)) return nullptr;
    const BWEnt e = dwt[ai][si];
    return e.p ? e.p + (size_t)ar * e.rs + (size_t)xr * e.cs : nullptr;
  }
  __device__ __forceinline__ float *db(int) const { return nullptr; }  // (blk_bias_reduce_kernel does the biases)
};

// bias gradients: one wave per A row adds up the workgroups' row sums in a fixed order; one read-modify-write per word
template <class Op>
__global__ void blk_bias_reduce_kernel(Op op, const float *__restrict__ bias_part, int nparts, int m_rows_pad) {
  const int m = blockIdx.x, lane = threadIdx.x;
  int ai, row;
  if (!op.find_a(m, ai, row)) return;
  float *d0 = op.dbv[ai][0], *d1 = op.dbv[ai][1];
  if (!d0 && !d1) return;
  float s = 0.f;
  for (int p = lane; p < nparts; p += 64) s += bias_part[(size_t)p * m_rows_pad + m];
  s = wave_sum(s);
  if (lane == 0) {
    if (d0) d0[row] += s;
    if (d1) d1[row] += s;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// element-wise: the gate and its derivative
// ---------------------------------------------------------------------------------------------------------------
// th, sg hold the pre-activations f, g on entry and tanh(f), sigmoid(g) on return
__global__ void blk_gate_kernel(float *th, long long tsb, int tld, float *sg, long long gsb, int gld, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (t >= n) return;
  float *pt = th + (size_t)b * tsb + (size_t)c * tld + t, *pg = sg + (size_t)b * gsb + (size_t)c * gld + t;
  *pt = tanh_fast(*pt);
  *pg = sigmoid_fast(*pg);
}
// df holds dz on entry; df = dz sg (1 - th^2), dg = dz th sg (1 - sg)   (both (B, C, n) with ld = n)
__global__ void blk_gate_bwd_kernel(float *df, float *dg, int C, const float *th, long long tsb, int tld,
                                    const float *sg, long long gsb, int gld, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (t >= n) return;
  const size_t o = ((size_t)b * C + c) * n + t;
  const float dz = df[o], tv = th[(size_t)b * tsb + (size_t)c * tld + t], sv = sg[(size_t)b * gsb + (size_t)c * gld + t];
  df[o] = dz * sv * (1.0f - tv * tv);
  dg[o] = dz * tv * sv * (1.0f - sv);
}

// ---------------------------------------------------------------------------------------------------------------
// FUSED64: one gated layer forward, C = K = 64.  A workgroup (four waves) owns 128 output columns of one sequence,
// a wave 32 of them with all 128 rows (four 32 x 32 fp32 MFMA tiles, 64 accumulators):
//   1. f | g = W_fg [x(j); x(j + d)] (+ W_ctx ctx): k runs over (channel, tap) pairs as the weights lie in memory, in
//      chunks of 16 through LDS (W chunk 16 x 128, X chunk 16 x 128 columns), double buffered;
//   2. the gate in registers; tanh / sigmoid stored only when they are to be saved; z into LDS (64 x 128, over the idle
//      X chunks) -- never to HBM;
//   3. residual | skip = [W_r; W_s] z, W in the same 16-deep chunks, B operand straight from the z tile;
//   4. + bias (+ x(j + d) on the residual rows); the skip rows keep columns >= s0 only.
// Every global access along time is one dword per lane at a clamped column: rows may start at any 4-byte address.
// LDS: 2 x 16 x 129 + 64 x 128 floats = 48.1 KB -- three workgroups per CU by LDS, two by registers.
// ---------------------------------------------------------------------------------------------------------------
struct Fused64Args {
  const float *x, *ctx;  // ctx: NULL or the context already advanced to its last n columns
  long long xsb, csb;
  int xld, cld;
  const float *wf, *wg, *bf, *bg, *wcf, *wcg, *bcf, *bcg, *wr, *br, *ws, *bs;
  float *res, *skip, *th, *sg;
  long long rsb, ssb, tsb, gsb;
  int rld, sld, tld, gld;
  int n, d, s0;  // output columns, dilation, first column of the skip that is kept
};
constexpr int FZ_TT = 128, FZ_WP = 129;

__global__ __launch_bounds__(256, 2) void gated64_fused_kernel(Fused64Args a) {
  __shared__ float lds[2 * 16 * FZ_WP + 64 * FZ_TT];
  float *Ws = lds, *Xs = lds + 2 * 16 * FZ_WP, *Zs = Xs;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, t0 = blockIdx.x * FZ_TT;
  const int col = tid & 127, kh = tid >> 7;  // X staging: column, k parity
  const int wk = tid & 15, wm = tid >> 4;    // W staging: k inside the chunk, row wm + 16 j
  const int tcol = min(t0 + col, a.n - 1);   // clamped: columns past n compute on a copy of column n - 1, never stored
  const float *xb = a.x + (size_t)b * a.xsb + tcol;
  const float *cb = a.ctx ? a.ctx + (size_t)b * a.csb + tcol : nullptr;
  const int li = lane & 31, lh = lane >> 5;

  f32x16 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  float wreg[8], xreg[8];
  auto gload1 = [&](int c) {
    const int k0 = 16 * c;
    if (c < 8) {  // k = 2 channel + tap
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = wm + 16 * j;
        wreg[j] = m < 64 ? a.wf[m * 128 + k0 + wk] : a.wg[(m - 64) * 128 + k0 + wk];
        const int k = k0 + kh + 2 * j;
        xreg[j] = xb[(size_t)(k >> 1) * a.xld + (k & 1) * a.d];
      }
    } else {  // the context's 64 channels
      const int kc = k0 - 128;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = wm + 16 * j;
        wreg[j] = m < 64 ? a.wcf[m * 64 + kc + wk] : a.wcg[(m - 64) * 64 + kc + wk];
        xreg[j] = cb[(size_t)(kc + kh + 2 * j) * a.cld];
      }
    }
  };
  auto gload2 = [&](int c) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int m = wm + 16 * j;
      wreg[j] = m < 64 ? a.wr[m * 64 + 16 * c + wk] : a.ws[(m - 64) * 64 + 16 * c + wk];
    }
  };
  auto wstore = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 8; ++j) Ws[(buf * 16 + wk) * FZ_WP + wm + 16 * j] = wreg[j];
  };
  auto xstore = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 8; ++j) Xs[(buf * 16 + kh + 2 * j) * FZ_TT + col] = xreg[j];
  };

  // ---- 1. f | g ----
  const int nchunk = a.ctx ? 12 : 8;
  gload1(0);
  wstore(0);
  xstore(0);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunk) gload1(c + 1);
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int kr = buf * 16 + 2 * kk + lh;
      const float bv = Xs[kr * FZ_TT + 32 * wave + li];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[kr * FZ_WP + 32 * mi + li], bv, acc[mi], 0, 0, 0);
    }
    if (c + 1 < nchunk) {
      wstore(buf ^ 1);
      xstore(buf ^ 1);
    }
    __syncthreads();
  }

  // ---- 2. gate (every wave has left the X chunks: the z tile may overwrite them) ----
  const int t = t0 + 32 * wave + li;
  const bool live = t < a.n;
  const bool save = a.th != nullptr;
  gload2(0);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * mi + acc_row(r, lane);
      float fb = 0.f, gb = 0.f;
      if (a.bf) fb += a.bf[row];
      if (a.bg) gb += a.bg[row];
      if (a.ctx) {
        fb += a.bcf[row];
        gb += a.bcg[row];
      }
      const float tv = tanh_fast(acc[mi][r] + fb), sv = sigmoid_fast(acc[mi + 2][r] + gb);
      if (save && live) {
        a.th[(size_t)b * a.tsb + (size_t)row * a.tld + t] = tv;
        a.sg[(size_t)b * a.gsb + (size_t)row * a.gld + t] = sv;
      }
      Zs[row * FZ_TT + 32 * wave + li] = tv * sv;
    }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  // ---- 3. residual | skip ----
  wstore(0);
  __syncthreads();
  for (int c = 0; c < 4; ++c) {
    const int buf = c & 1;
    if (c + 1 < 4) gload2(c + 1);
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int kq = 2 * kk + lh;
      const float bv = Zs[(16 * c + kq) * FZ_TT + 32 * wave + li];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[(buf * 16 + kq) * FZ_WP + 32 * mi + li], bv, acc[mi], 0, 0, 0);
    }
    if (c + 1 < 4) wstore(buf ^ 1);
    __syncthreads();
  }

  // ---- 4. stores ----
  if (!live) return;
  const float *xr = a.x + (size_t)b * a.xsb + t + a.d;
  float *ro = a.res + (size_t)b * a.rsb + t;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * mi + acc_row(r, lane);
      ro[(size_t)row * a.rld] = acc[mi][r] + a.br[row] + xr[(size_t)row * a.xld];
    }
  if (t >= a.s0) {
    float *so = a.skip + (size_t)b * a.ssb + (t - a.s0);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * mi + acc_row(r, lane);
        so[(size_t)row * a.sld] = acc[mi + 2][r] + a.bs[row];
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int g_block_form = 0;

static BSeg seg(const float *p, int channels, int ld, int rows, int shift, int lo, int hi) {
  BSeg s;
  s.p = p; s.p2 = nullptr; s.sb = (long long)channels * ld; s.ld = ld; s.rows = rows; s.lrelu = 0;
  if (hi <= lo) shift = lo = hi = 0;  // exists nowhere: reads column 0, selects zero
  s.shift = shift; s.lo = lo; s.hi = hi;
  return s;
}
static BSeg seg(const mvn_block_tensor *v, int rows, int shift, int lo, int hi) {
  return seg(v->p, rows, v->ld, rows, shift, lo, hi);
}
static BSeg no_seg() {
  BSeg s;
  s.p = s.p2 = nullptr; s.sb = 0; s.ld = 0; s.rows = 0; s.shift = s.lo = s.hi = s.lrelu = 0;
  return s;
}
static BOut out_rows(float *p, int rows, int ld, int oshift, int olo, int ohi, const float *b0, const float *b1) {
  BOut o;
  o.rows = rows; o.out = p; o.osb = (long long)rows * ld; o.old = ld; o.oshift = oshift; o.olo = olo; o.ohi = ohi;
  o.b0 = b0; o.b1 = b1; o.add = no_seg(); o.der = no_seg();
  return o;
}
static BWEnt went(const float *p, int rs, int cs) {
  BWEnt e;
  e.p = const_cast<float *>(p); e.rs = rs; e.cs = cs;
  return e;
}
static void gemm_init(BlkGemmOp &g, int t_end) {
  g.K = 0; g.t_begin = 0; g.t_end = t_end;
  for (int i = 0; i < 4; ++i) { g.xs[i] = no_seg(); g.xend[i] = 0; }
  for (int i = 0; i < 2; ++i) {
    g.ms[i] = out_rows(nullptr, 0, 0, 0, 0, 0, nullptr, nullptr);
    for (int j = 0; j < 4; ++j) g.wt[i][j] = went(nullptr, 0, 0);
  }
}
static void gemm_finish(BlkGemmOp &g) {
  int tot = 0;
  for (int i = 0; i < 4; ++i) { tot += g.xs[i].rows; g.xend[i] = tot; }
  g.K = tot;
}
template <class Op>
static void wg_init(Op &w, int t_end, const float *safe, long long safe_sb) {
  w.t_begin = 0; w.t_end = t_end; w.lrelu = 0; w.safe = safe; w.safe_sb = safe_sb;
  for (int i = 0; i < 4; ++i) { w.xs[i] = no_seg(); w.xend[i] = 0; }
  for (int i = 0; i < 2; ++i) {
    w.as[i] = no_seg();
    w.dbv[i][0] = w.dbv[i][1] = nullptr;
    for (int j = 0; j < 4; ++j) w.dwt[i][j] = went(nullptr, 0, 0);
  }
}

// floats one weight-gradient launch needs: a slab and a row-sum vector per workgroup
static size_t wg_floats(long long m_rows, long long n_rows, long long batch, long long nt) {
  const long long chunks = (nt + W2_CHUNK - 1) / W2_CHUNK, mpad = (m_rows + 127) / 128 * 128, npad = (n_rows + 63) / 64 * 64;
  return (size_t)(chunks * batch * (mpad * npad + mpad));
}
template <class Op>
static void launch_blk_wgrad(Op &w, int batch, float *scratch, hipStream_t s) {
  int tot = 0;
  for (int i = 0; i < 4; ++i) { tot += w.xs[i].rows; w.xend[i] = tot; }
  const int m_rows = w.as[0].rows + w.as[1].rows, n_rows = tot, nt = w.t_end;
  const int chunks = (nt + W2_CHUNK - 1) / W2_CHUNK;
  const int mb = (m_rows + 127) / 128, nb = (n_rows + 63) / 64, mpad = mb * 128, npad = nb * 64;
  float *bias_part = scratch, *part = scratch + (size_t)chunks * batch * mpad;
  dim3 grid(chunks * batch, mb * nb);
  hipLaunchKernelGGL((wgrad2_kernel<Op, 1>), grid, dim3(256), 0, s, w, nb, chunks, bias_part, mpad, part, npad);
  hipLaunchKernelGGL(slab_reduce_kernel<Op>, dim3(mpad * npad / 32), dim3(32 * RED_SEG), 0, s, w, part, chunks * batch,
                     mpad, npad);
  if (w.dbv[0][0] || w.dbv[0][1] || w.dbv[1][0] || w.dbv[1][1])
    hipLaunchKernelGGL(blk_bias_reduce_kernel<Op>, dim3(m_rows), dim3(64), 0, s, w, bias_part, chunks * batch, mpad);
}
static void launch_blk_gemm(BlkGemmOp &g, int batch, hipStream_t s) {
  gemm_finish(g);
  launch_gemm(g, g.ms[0].rows + g.ms[1].rows, batch, s);
}

static int check_tensor(const char *fn, const char *name, const mvn_block_tensor *v) {
  if (!v || !v->p) {
    set_error("%s: bad argument: %s is NULL", fn, name);
    return MVN_ERR_BAD_ARG;
  }
  if (v->len < 1 || v->ld < v->len) {
    set_error("%s: bad argument: %s has length %d, row stride %d (need ld >= length >= 1)", fn, name, v->len, v->ld);
    return MVN_ERR_BAD_ARG;
  }
  if ((long long)v->ld * 4 >= (1LL << 31)) {
    set_error("%s: %s has rows of %lld bytes: rows of 2^31 bytes or more are not supported", fn, name, (long long)v->ld * 4);
    return MVN_ERR_UNSUPPORTED;
  }
  return MVN_OK;
}
static int check_batch(const char *fn, int batch) {
  if (batch < 1 || batch > 65535) {
    set_error("%s: bad argument: batch %d outside [1, 65535]", fn, batch);
    return MVN_ERR_BAD_ARG;
  }
  return MVN_OK;
}
static int check_len(const char *fn, const char *name, const mvn_block_tensor *v, int want) {
  if (v->len != want) {
    set_error("%s: bad argument: %s has length %d, expected %d", fn, name, v->len, want);
    return MVN_ERR_BAD_ARG;
  }
  return MVN_OK;
}
static int check_scratch(const char *fn, const float *scratch, size_t have, size_t need) {
  if (need && (!scratch || have < need)) {
    set_error("%s: bad argument: scratch of %zu floats, %zu needed", fn, scratch ? have : (size_t)0, need);
    return MVN_ERR_BAD_ARG;
  }
  return MVN_OK;
}
static int check_conv_dims(const char *fn, int cin, int cout) {
  if (cin < 1 || cin > 1024 || cout < 1 || cout > 1024) {
    set_error("%s: channels %d -> %d outside [1, 1024]", fn, cin, cout);
    return MVN_ERR_BAD_DIMS;
  }
  return MVN_OK;
}
static int check_gated_dims(const char *fn, int C, int K, int d) {
  if (C < 1 || C > 256 || K < 1 || K > 256) {
    set_error("%s: residual channels %d / skip channels %d outside [1, 256]", fn, C, K);
    return MVN_ERR_BAD_DIMS;
  }
  if (d < 1) {
    set_error("%s: bad argument: dilation %d", fn, d);
    return MVN_ERR_BAD_ARG;
  }
  return MVN_OK;
}
#define BLK_TRY(expr)            \
  do {                           \
    const int rc_ = (expr);      \
    if (rc_ != MVN_OK) return rc_; \
  } while (0)

// the two-tap convolutions: taps at x[t + s0] and x[t + s1], outputs t in [0, n)
static int conv2_forward(const char *fn, const float *w, const float *bias, int cin, int cout, int s0, int s1,
                         const mvn_block_tensor *x, const mvn_block_tensor *y, int n, int batch, hipStream_t s) {
  BlkGemmOp g;
  gemm_init(g, n);
  g.xs[0] = seg(x, cin, s0, max(0, -s0), n);
  g.xs[1] = seg(x, cin, s1, 0, n);
  g.wt[0][0] = went(w, 2 * cin, 2);
  g.wt[0][1] = went(w + 1, 2 * cin, 2);
  g.ms[0] = out_rows(y->p, cout, y->ld, 0, 0, n, bias, nullptr);
  launch_blk_gemm(g, batch, s);
  g_block_form = MVN_BLOCK_FORM_GENERIC;
  return check_hip(hipGetLastError(), fn);
}
// x has T columns, dy has n; tap i reads x[t + si]
static int conv2_backward(const char *fn, const float *w, int cin, int cout, int s0, int s1, const mvn_block_tensor *x,
                          const mvn_block_tensor *dy, const mvn_block_tensor *dx, float *dw, float *dbias, int n,
                          int batch, float *scratch, hipStream_t s) {
  const int T = x->len;
  if (dx) {  // dx[c][t] = sum_m w[m][c][0] dy[m][t - s0] + w[m][c][1] dy[m][t - s1]
    BlkGemmOp g;
    gemm_init(g, T);
    g.xs[0] = seg(dy, cout, -s0, max(0, s0), min(T, n + s0));
    g.xs[1] = seg(dy, cout, -s1, max(0, s1), min(T, n + s1));
    g.wt[0][0] = went(w, 2, 2 * cin);
    g.wt[0][1] = went(w + 1, 2, 2 * cin);
    g.ms[0] = out_rows(dx->p, cin, dx->ld, 0, 0, T, nullptr, nullptr);
    launch_blk_gemm(g, batch, s);
  }
  if (dw || dbias) {
    BlkWgOp<false> wg;
    // the safe row: tap 1 of x exists over all of [0, n)
    wg_init(wg, n, x->p + s1, (long long)cin * x->ld);
    wg.as[0] = seg(dy, cout, 0, 0, n);
    wg.xs[0] = seg(x, cin, s0, max(0, -s0), n);
    wg.xs[1] = seg(x, cin, s1, 0, n);
    wg.dwt[0][0] = went(dw, 2 * cin, 2);
    wg.dwt[0][1] = went(dw ? dw + 1 : nullptr, 2 * cin, 2);
    wg.dbv[0][0] = dbias;
    launch_blk_wgrad(wg, batch, scratch, s);
  }
  g_block_form = MVN_BLOCK_FORM_GENERIC;
  return check_hip(hipGetLastError(), fn);
}

static size_t gated_fwd_floats(int C, int K, int batch, int n, bool saved) {
  if (saved || (C == 64 && K == 64)) return 0;
  return (size_t)2 * batch * C * n;
}
static size_t gated_bwd_floats(int C, int K, int batch, int n, bool has_ctx) {
  const size_t fg = wg_floats(2 * C, (has_ctx ? 3 : 2) * C, batch, n), rs = wg_floats(C + K, C, batch, n);
  return (size_t)2 * batch * C * n + (fg > rs ? fg : rs);
}
static size_t dense_bwd_floats(int K, int Q, int batch, int S) {
  const size_t w2 = wg_floats(Q, Q, batch, S), w1 = wg_floats(Q, K, batch, S);
  return (size_t)batch * Q * S + (w2 > w1 ? w2 : w1);
}

}  // namespace mvn

using namespace mvn;

extern "C" {

int mvn_block_last_form(void) { return g_block_form; }

size_t mvn_block_conv_scratch_floats(int cin, int cout, int batch, int t_len) {
  if (cin < 1 || cin > 1024 || cout < 1 || cout > 1024 || batch < 1 || t_len < 1) return 0;
  return wg_floats(cout, 2 * cin, batch, t_len);
}

int mvn_block_causal_forward(const float *w, const float *bias, int cin, int cout, const mvn_block_tensor *x,
                             const mvn_block_tensor *y, int batch, void *stream) {
  const char *fn = "mvn_block_causal_forward";
  BLK_TRY(check_conv_dims(fn, cin, cout));
  BLK_TRY(check_batch(fn, batch));
  if (!w) {
    set_error("%s: bad argument: w is NULL", fn);
    return MVN_ERR_BAD_ARG;
  }
  BLK_TRY(check_tensor(fn, "x", x));
  BLK_TRY(check_tensor(fn, "y", y));
  BLK_TRY(check_len(fn, "y", y, x->len));
  return conv2_forward(fn, w, bias, cin, cout, -1, 0, x, y, x->len, batch, (hipStream_t)stream);
}

int mvn_block_causal_backward(const float *w, int cin, int cout, const mvn_block_tensor *x, const mvn_block_tensor *dy,
                              const mvn_block_tensor *dx, float *dw, float *dbias, int batch, float *scratch,
                              size_t scratch_floats, void *stream) {
  const char *fn = "mvn_block_causal_backward";
  BLK_TRY(check_conv_dims(fn, cin, cout));
  BLK_TRY(check_batch(fn, batch));
  if (!w) {
    set_error("%s: bad argument: w is NULL", fn);
    return MVN_ERR_BAD_ARG;
  }
  BLK_TRY(check_tensor(fn, "x", x));
  BLK_TRY(check_tensor(fn, "dy", dy));
  BLK_TRY(check_len(fn, "dy", dy, x->len));
  if (dx) {
    BLK_TRY(check_tensor(fn, "dx", dx));
    BLK_TRY(check_len(fn, "dx", dx, x->len));
  }
  if (dw || dbias) BLK_TRY(check_scratch(fn, scratch, scratch_floats, wg_floats(cout, 2 * cin, batch, x->len)));
  return conv2_backward(fn, w, cin, cout, -1, 0, x, dy, dx, dw, dbias, x->len, batch, scratch, (hipStream_t)stream);
}

int mvn_block_dilated_forward(const float *w, const float *bias, int channels, int dilation, const mvn_block_tensor *x,
                              const mvn_block_tensor *y, int batch, void *stream) {
  const char *fn = "mvn_block_dilated_forward";
  BLK_TRY(check_gated_dims(fn, channels, channels, dilation));
  BLK_TRY(check_batch(fn, batch));
  if (!w) {
    set_error("%s: bad argument: w is NULL", fn);
    return MVN_ERR_BAD_ARG;
  }
  BLK_TRY(check_tensor(fn, "x", x));
  if (x->len <= dilation) {
    set_error("%s: bad argument: T = %d does not exceed the dilation d = %d", fn, x->len, dilation);
    return MVN_ERR_BAD_ARG;
  }
  BLK_TRY(check_tensor(fn, "y", y));
  BLK_TRY(check_len(fn, "y", y, x->len - dilation));
  return conv2_forward(fn, w, bias, channels, channels, 0, dilation, x, y, x->len - dilation, batch, (hipStream_t)stream);
}

int mvn_block_dilated_backward(const float *w, int channels, int dilation, const mvn_block_tensor *x,
                               const mvn_block_tensor *dy, const mvn_block_tensor *dx, float *dw, float *dbias, int batch,
                               float *scratch, size_t scratch_floats, void *stream) {
  const char *fn = "mvn_block_dilated_backward";
  BLK_TRY(check_gated_dims(fn, channels, channels, dilation));
  BLK_TRY(check_batch(fn, batch));
  if (!w) {
    set_error("%s: bad argument: w is NULL", fn);
    return MVN_ERR_BAD_ARG;
  }
  BLK_TRY(check_tensor(fn, "x", x));
  if (x->len <= dilation) {
    set_error("%s: bad argument: T = %d does not exceed the dilation d = %d", fn, x->len, dilation);
    return MVN_ERR_BAD_ARG;
  }
  const int n = x->len - dilation;
  BLK_TRY(check_tensor(fn, "dy", dy));
  BLK_TRY(check_len(fn, "dy", dy, n));
  if (dx) {
    BLK_TRY(check_tensor(fn, "dx", dx));
    BLK_TRY(check_len(fn, "dx", dx, x->len));
  }
  if (dw || dbias) BLK_TRY(check_scratch(fn, scratch, scratch_floats, wg_floats(channels, 2 * channels, batch, n)));
  return conv2_backward(fn, w, channels, channels, 0, dilation, x, dy, dx, dw, dbias, n, batch, scratch,
                        (hipStream_t)stream);
}

size_t mvn_block_gated_scratch_floats(int residual_channels, int skip_channels, int batch, int t_len, int dilation,
                                      int has_context, int backward) {
  const int C = residual_channels, K = skip_channels;
  if (C < 1 || C > 256 || K < 1 || K > 256 || batch < 1 || dilation < 1 || t_len <= dilation) return 0;
  const int n = t_len - dilation;
  // (never zero for a valid shape: callers allocate what this returns)
  const size_t need = backward ? gated_bwd_floats(C, K, batch, n, has_context != 0) : gated_fwd_floats(C, K, batch, n, false);
  return need > 64 ? need : 64;
}

static int check_gated_common(const char *fn, const mvn_block_gated_params *p, int C, int K, int d,
                              const mvn_block_tensor *x, const mvn_block_tensor *ctx, int batch) {
  BLK_TRY(check_gated_dims(fn, C, K, d));
  BLK_TRY(check_batch(fn, batch));
  if (!p || !p->filter_w || !p->gate_w || !p->residual_w || !p->residual_b || !p->skip_w || !p->skip_b) {
    set_error("%s: bad argument: NULL parameter pointer", fn);
    return MVN_ERR_BAD_ARG;
  }
  BLK_TRY(check_tensor(fn, "x", x));
  if (x->len <= d) {
    set_error("%s: bad argument: T = %d does not exceed the dilation d = %d", fn, x->len, d);
    return MVN_ERR_BAD_ARG;
  }
  if (ctx) {
    BLK_TRY(check_tensor(fn, "context", ctx));
    if (!p->ctx_filter_w || !p->ctx_filter_b || !p->ctx_gate_w || !p->ctx_gate_b) {
      set_error("%s: bad argument: a context needs the four context-conv parameters", fn);
      return MVN_ERR_BAD_ARG;
    }
    if (ctx->len < x->len - d) {
      set_error("%s: bad argument: context of %d columns, the layer has T - d = %d", fn, ctx->len, x->len - d);
      return MVN_ERR_BAD_ARG;
    }
  }
  return MVN_OK;
}

int mvn_block_gated_forward(const mvn_block_gated_params *p, int residual_channels, int skip_channels, int dilation,
                            const mvn_block_tensor *x, const mvn_block_tensor *context, const mvn_block_tensor *residual,
                            const mvn_block_tensor *skip, const mvn_block_tensor *th, const mvn_block_tensor *sg,
                            int batch, float *scratch, size_t scratch_floats, void *stream) {
  const char *fn = "mvn_block_gated_forward";
  const int C = residual_channels, K = skip_channels, d = dilation;
  BLK_TRY(check_gated_common(fn, p, C, K, d, x, context, batch));
  const int n = x->len - d;
  BLK_TRY(check_tensor(fn, "residual", residual));
  BLK_TRY(check_len(fn, "residual", residual, n));
  BLK_TRY(check_tensor(fn, "skip", skip));
  if (skip->len > n) {
    set_error("%s: bad argument: skip of %d columns, the layer has T - d = %d", fn, skip->len, n);
    return MVN_ERR_BAD_ARG;
  }
  if ((th == nullptr) != (sg == nullptr)) {
    set_error("%s: bad argument: th and sg are saved together or not at all", fn);
    return MVN_ERR_BAD_ARG;
  }
  if (th) {
    BLK_TRY(check_tensor(fn, "th", th));
    BLK_TRY(check_len(fn, "th", th, n));
    BLK_TRY(check_tensor(fn, "sg", sg));
    BLK_TRY(check_len(fn, "sg", sg, n));
    if (th->ld != sg->ld) {  // (the generic form reads z = th * sg at one offset)
      set_error("%s: bad argument: th and sg must share a row stride (%d, %d)", fn, th->ld, sg->ld);
      return MVN_ERR_BAD_ARG;
    }
  }
  BLK_TRY(check_scratch(fn, scratch, scratch_floats, gated_fwd_floats(C, K, batch, n, th != nullptr)));
  hipStream_t s = (hipStream_t)stream;
  const int s0 = n - skip->len, coff = context ? context->len - n : 0;

  if (C == 64 && K == 64) {
    Fused64Args a;
    a.x = x->p; a.xsb = (long long)C * x->ld; a.xld = x->ld;
    a.ctx = context ? context->p + coff : nullptr;
    a.csb = context ? (long long)C * context->ld : 0; a.cld = context ? context->ld : 0;
    a.wf = p->filter_w; a.wg = p->gate_w; a.bf = p->filter_b; a.bg = p->gate_b;
    a.wcf = p->ctx_filter_w; a.wcg = p->ctx_gate_w; a.bcf = p->ctx_filter_b; a.bcg = p->ctx_gate_b;
    a.wr = p->residual_w; a.br = p->residual_b; a.ws = p->skip_w; a.bs = p->skip_b;
    a.res = residual->p; a.rsb = (long long)C * residual->ld; a.rld = residual->ld;
    a.skip = skip->p; a.ssb = (long long)K * skip->ld; a.sld = skip->ld;
    a.th = th ? th->p : nullptr; a.sg = sg ? sg->p : nullptr;
    a.tsb = th ? (long long)C * th->ld : 0; a.tld = th ? th->ld : 0;
    a.gsb = sg ? (long long)C * sg->ld : 0; a.gld = sg ? sg->ld : 0;
    a.n = n; a.d = d; a.s0 = s0;
    hipLaunchKernelGGL(gated64_fused_kernel, dim3((n + FZ_TT - 1) / FZ_TT, batch), dim3(256), 0, s, a);
    g_block_form = MVN_BLOCK_FORM_FUSED64;
    return check_hip(hipGetLastError(), fn);
  }

  mvn_block_tensor tv, gv;
  if (th) {
    tv = *th;
    gv = *sg;
  } else {
    tv.p = scratch; tv.ld = n; tv.len = n;
    gv.p = scratch + (size_t)batch * C * n; gv.ld = n; gv.len = n;
  }
  {  // f | g (pre-activations into the tanh / sigmoid buffers)
    BlkGemmOp g;
    gemm_init(g, n);
    g.xs[0] = seg(x, C, 0, 0, n);
    g.xs[1] = seg(x, C, d, 0, n);
    if (context) g.xs[2] = seg(context, C, coff, 0, n);
    g.wt[0][0] = went(p->filter_w, 2 * C, 2);
    g.wt[0][1] = went(p->filter_w + 1, 2 * C, 2);
    g.wt[1][0] = went(p->gate_w, 2 * C, 2);
    g.wt[1][1] = went(p->gate_w + 1, 2 * C, 2);
    if (context) {
      g.wt[0][2] = went(p->ctx_filter_w, C, 1);
      g.wt[1][2] = went(p->ctx_gate_w, C, 1);
    }
    g.ms[0] = out_rows(tv.p, C, tv.ld, 0, 0, n, p->filter_b, context ? p->ctx_filter_b : nullptr);
    g.ms[1] = out_rows(gv.p, C, gv.ld, 0, 0, n, p->gate_b, context ? p->ctx_gate_b : nullptr);
    launch_blk_gemm(g, batch, s);
  }
  hipLaunchKernelGGL(blk_gate_kernel, dim3((n + 255) / 256, C, batch), dim3(256), 0, s, tv.p, (long long)C * tv.ld, tv.ld,
                     gv.p, (long long)C * gv.ld, gv.ld, n);
  {  // residual | skip from z = tanh * sigmoid
    BlkGemmOp g;
    gemm_init(g, n);
    g.xs[0] = seg(&tv, C, 0, 0, n);
    g.xs[0].p2 = gv.p;
    g.wt[0][0] = went(p->residual_w, C, 1);
    g.wt[1][0] = went(p->skip_w, C, 1);
    g.ms[0] = out_rows(residual->p, C, residual->ld, 0, 0, n, p->residual_b, nullptr);
    g.ms[0].add = seg(x, C, d, 0, n);
    g.ms[1] = out_rows(skip->p, K, skip->ld, -s0, s0, n, p->skip_b, nullptr);
    launch_blk_gemm(g, batch, s);
  }
  g_block_form = MVN_BLOCK_FORM_GENERIC;
  return check_hip(hipGetLastError(), fn);
}

int mvn_block_gated_backward(const mvn_block_gated_params *p, const mvn_block_gated_grads *grads, int residual_channels,
                             int skip_channels, int dilation, const mvn_block_tensor *x, const mvn_block_tensor *context,
                             const mvn_block_tensor *th, const mvn_block_tensor *sg, const mvn_block_tensor *d_residual,
                             const mvn_block_tensor *d_skip, const mvn_block_tensor *dx, const mvn_block_tensor *dcontext,
                             int batch, float *scratch, size_t scratch_floats, void *stream) {
  const char *fn = "mvn_block_gated_backward";
  const int C = residual_channels, K = skip_channels, d = dilation;
  BLK_TRY(check_gated_common(fn, p, C, K, d, x, context, batch));
  const int n = x->len - d;
  if (!grads) {
    set_error("%s: bad argument: grads is NULL", fn);
    return MVN_ERR_BAD_ARG;
  }
  BLK_TRY(check_tensor(fn, "th", th));
  BLK_TRY(check_len(fn, "th", th, n));
  BLK_TRY(check_tensor(fn, "sg", sg));
  BLK_TRY(check_len(fn, "sg", sg, n));
  if (th->ld != sg->ld) {
    set_error("%s: bad argument: th and sg must share a row stride (%d, %d)", fn, th->ld, sg->ld);
    return MVN_ERR_BAD_ARG;
  }
  if (!d_residual && !d_skip) {
    set_error("%s: bad argument: d_residual and d_skip are both NULL", fn);
    return MVN_ERR_BAD_ARG;
  }
  if (d_residual) {
    BLK_TRY(check_tensor(fn, "d_residual", d_residual));
    BLK_TRY(check_len(fn, "d_residual", d_residual, n));
  }
  if (d_skip) {
    BLK_TRY(check_tensor(fn, "d_skip", d_skip));
    if (d_skip->len > n) {
      set_error("%s: bad argument: d_skip of %d columns, the layer has T - d = %d", fn, d_skip->len, n);
      return MVN_ERR_BAD_ARG;
    }
  }
  if (dx) {
    BLK_TRY(check_tensor(fn, "dx", dx));
    BLK_TRY(check_len(fn, "dx", dx, x->len));
  }
  if (dcontext) {
    if (!context) {
      set_error("%s: bad argument: dcontext without a context", fn);
      return MVN_ERR_BAD_ARG;
    }
    BLK_TRY(check_tensor(fn, "dcontext", dcontext));
    BLK_TRY(check_len(fn, "dcontext", dcontext, context->len));
  }
  BLK_TRY(check_scratch(fn, scratch, scratch_floats, gated_bwd_floats(C, K, batch, n, context != nullptr)));
  hipStream_t s = (hipStream_t)stream;
  const int coff = context ? context->len - n : 0, T = x->len;
  const int s0 = d_skip ? n - d_skip->len : n;
  float *df = scratch, *dg = scratch + (size_t)batch * C * n, *wscr = dg + (size_t)batch * C * n;

  {  // dz = Wr^T d_residual + Ws^T d_skip
    BlkGemmOp g;
    gemm_init(g, n);
    if (d_residual) g.xs[0] = seg(d_residual, C, 0, 0, n);
    if (d_skip) g.xs[1] = seg(d_skip, K, -s0, s0, n);
    g.wt[0][0] = went(p->residual_w, 1, C);
    g.wt[0][1] = went(p->skip_w, 1, C);
    g.ms[0] = out_rows(df, C, n, 0, 0, n, nullptr, nullptr);
    launch_blk_gemm(g, batch, s);
  }
  hipLaunchKernelGGL(blk_gate_bwd_kernel, dim3((n + 255) / 256, C, batch), dim3(256), 0, s, df, dg, C, th->p,
                     (long long)C * th->ld, th->ld, sg->p, (long long)C * sg->ld, sg->ld, n);
  if (dx) {  // dx[t] = Wf0^T df[t] + Wg0^T dg[t] + Wf1^T df[t - d] + Wg1^T dg[t - d] + d_residual[t - d]
    BlkGemmOp g;
    gemm_init(g, T);
    g.xs[0] = seg(df, C, n, C, 0, 0, n);
    g.xs[1] = seg(dg, C, n, C, 0, 0, n);
    g.xs[2] = seg(df, C, n, C, -d, d, T);
    g.xs[3] = seg(dg, C, n, C, -d, d, T);
    g.wt[0][0] = went(p->filter_w, 2, 2 * C);
    g.wt[0][1] = went(p->gate_w, 2, 2 * C);
    g.wt[0][2] = went(p->filter_w + 1, 2, 2 * C);
    g.wt[0][3] = went(p->gate_w + 1, 2, 2 * C);
    g.ms[0] = out_rows(dx->p, C, dx->ld, 0, 0, T, nullptr, nullptr);
    if (d_residual) g.ms[0].add = seg(d_residual, C, -d, d, T);
    launch_blk_gemm(g, batch, s);
  }
  if (dcontext) {  // written in full: zero in front of the columns the layer used
    const int Tc = context->len;
    BlkGemmOp g;
    gemm_init(g, Tc);
    g.xs[0] = seg(df, C, n, C, -coff, coff, Tc);
    g.xs[1] = seg(dg, C, n, C, -coff, coff, Tc);
    g.wt[0][0] = went(p->ctx_filter_w, 1, C);
    g.wt[0][1] = went(p->ctx_gate_w, 1, C);
    g.ms[0] = out_rows(dcontext->p, C, dcontext->ld, 0, 0, Tc, nullptr, nullptr);
    launch_blk_gemm(g, batch, s);
  }
  const bool want_fg = grads->filter_w || grads->gate_w || grads->filter_b || grads->gate_b ||
                       (context && (grads->ctx_filter_w || grads->ctx_gate_w || grads->ctx_filter_b || grads->ctx_gate_b));
  if (want_fg) {
    BlkWgOp<false> wg;
    wg_init(wg, n, x->p, (long long)C * x->ld);
    wg.as[0] = seg(df, C, n, C, 0, 0, n);
    wg.as[1] = seg(dg, C, n, C, 0, 0, n);
    wg.xs[0] = seg(x, C, 0, 0, n);
    wg.xs[1] = seg(x, C, d, 0, n);
    if (context) wg.xs[2] = seg(context, C, coff, 0, n);
    wg.dwt[0][0] = went(grads->filter_w, 2 * C, 2);
    wg.dwt[0][1] = went(grads->filter_w ? grads->filter_w + 1 : nullptr, 2 * C, 2);
    wg.dwt[1][0] = went(grads->gate_w, 2 * C, 2);
    wg.dwt[1][1] = went(grads->gate_w ? grads->gate_w + 1 : nullptr, 2 * C, 2);
    wg.dbv[0][0] = grads->filter_b;
    wg.dbv[1][0] = grads->gate_b;
    if (context) {
      wg.dwt[0][2] = went(grads->ctx_filter_w, C, 1);
      wg.dwt[1][2] = went(grads->ctx_gate_w, C, 1);
      wg.dbv[0][1] = grads->ctx_filter_b;
      wg.dbv[1][1] = grads->ctx_gate_b;
    }
    launch_blk_wgrad(wg, batch, wscr, s);
  }
  const bool want_r = d_residual && (grads->residual_w || grads->residual_b);
  const bool want_s = d_skip && (grads->skip_w || grads->skip_b);
  if (want_r || want_s) {
    BlkWgOp<true> wg;
    wg_init(wg, n, th->p, (long long)C * th->ld);
    if (want_r) wg.as[0] = seg(d_residual, C, 0, 0, n);
    if (want_s) wg.as[1] = seg(d_skip, K, -s0, s0, n);
    wg.xs[0] = seg(th, C, 0, 0, n);
    wg.xs[0].p2 = sg->p;
    wg.dwt[0][0] = went(grads->residual_w, C, 1);
    wg.dwt[1][0] = went(grads->skip_w, C, 1);
    wg.dbv[0][0] = grads->residual_b;
    wg.dbv[1][0] = grads->skip_b;
    launch_blk_wgrad(wg, batch, wscr, s);
  }
  g_block_form = MVN_BLOCK_FORM_GENERIC;
  return check_hip(hipGetLastError(), fn);
}

size_t mvn_block_dense_scratch_floats(int in_channels, int out_channels, int batch, int s_len, int backward) {
  const int K = in_channels, Q = out_channels;
  if (K < 1 || K > 256 || Q < 1 || Q > 1024 || batch < 1 || s_len < 1) return 0;
  return backward ? dense_bwd_floats(K, Q, batch, s_len) : (size_t)batch * Q * s_len;
}

static int check_dense_dims(const char *fn, int K, int Q) {
  if (K < 1 || K > 256 || Q < 1 || Q > 1024) {
    set_error("%s: channels %d -> %d outside [1, 256] -> [1, 1024]", fn, K, Q);
    return MVN_ERR_BAD_DIMS;
  }
  return MVN_OK;
}

int mvn_block_dense_forward(const float *w1, const float *b1, const float *w2, const float *b2, int in_channels,
                            int out_channels, const mvn_block_tensor *x, const mvn_block_tensor *hidden,
                            const mvn_block_tensor *y, int batch, float *scratch, size_t scratch_floats, void *stream) {
  const char *fn = "mvn_block_dense_forward";
  const int K = in_channels, Q = out_channels;
  BLK_TRY(check_dense_dims(fn, K, Q));
  BLK_TRY(check_batch(fn, batch));
  if (!w1 || !b1 || !w2 || !b2) {
    set_error("%s: bad argument: NULL parameter pointer", fn);
    return MVN_ERR_BAD_ARG;
  }
  BLK_TRY(check_tensor(fn, "x", x));
  const int S = x->len;
  BLK_TRY(check_tensor(fn, "y", y));
  BLK_TRY(check_len(fn, "y", y, S));
  mvn_block_tensor hv;
  if (hidden) {
    BLK_TRY(check_tensor(fn, "hidden", hidden));
    BLK_TRY(check_len(fn, "hidden", hidden, S));
    hv = *hidden;
  } else {
    BLK_TRY(check_scratch(fn, scratch, scratch_floats, (size_t)batch * Q * S));
    hv.p = scratch; hv.ld = S; hv.len = S;
  }
  hipStream_t s = (hipStream_t)stream;
  {
    BlkGemmOp g;
    gemm_init(g, S);
    g.xs[0] = seg(x, K, 0, 0, S);
    g.xs[0].lrelu = 1;
    g.wt[0][0] = went(w1, K, 1);
    g.ms[0] = out_rows(hv.p, Q, hv.ld, 0, 0, S, b1, nullptr);
    launch_blk_gemm(g, batch, s);
  }
  {
    BlkGemmOp g;
    gemm_init(g, S);
    g.xs[0] = seg(&hv, Q, 0, 0, S);
    g.xs[0].lrelu = 1;
    g.wt[0][0] = went(w2, Q, 1);
    g.ms[0] = out_rows(y->p, Q, y->ld, 0, 0, S, b2, nullptr);
    launch_blk_gemm(g, batch, s);
  }
  g_block_form = MVN_BLOCK_FORM_GENERIC;
  return check_hip(hipGetLastError(), fn);
}

int mvn_block_dense_backward(const float *w1, const float *w2, int in_channels, int out_channels,
                             const mvn_block_tensor *x, const mvn_block_tensor *hidden, const mvn_block_tensor *dy,
                             const mvn_block_tensor *dx, float *dw1, float *db1, float *dw2, float *db2, int batch,
                             float *scratch, size_t scratch_floats, void *stream) {
  const char *fn = "mvn_block_dense_backward";
  const int K = in_channels, Q = out_channels;
  BLK_TRY(check_dense_dims(fn, K, Q));
  BLK_TRY(check_batch(fn, batch));
  if (!w1 || !w2) {
    set_error("%s: bad argument: NULL parameter pointer", fn);
    return MVN_ERR_BAD_ARG;
  }
  BLK_TRY(check_tensor(fn, "x", x));
  const int S = x->len;
  BLK_TRY(check_tensor(fn, "hidden", hidden));
  BLK_TRY(check_len(fn, "hidden", hidden, S));
  BLK_TRY(check_tensor(fn, "dy", dy));
  BLK_TRY(check_len(fn, "dy", dy, S));
  if (dx) {
    BLK_TRY(check_tensor(fn, "dx", dx));
    BLK_TRY(check_len(fn, "dx", dx, S));
  }
  BLK_TRY(check_scratch(fn, scratch, scratch_floats, dense_bwd_floats(K, Q, batch, S)));
  hipStream_t s = (hipStream_t)stream;
  float *dh = scratch, *wscr = scratch + (size_t)batch * Q * S;
  {  // dh = (W2^T dy) leaky'(h)
    BlkGemmOp g;
    gemm_init(g, S);
    g.xs[0] = seg(dy, Q, 0, 0, S);
    g.wt[0][0] = went(w2, 1, Q);
    g.ms[0] = out_rows(dh, Q, S, 0, 0, S, nullptr, nullptr);
    g.ms[0].der = seg(hidden, Q, 0, 0, S);
    launch_blk_gemm(g, batch, s);
  }
  if (dx) {  // dx = (W1^T dh) leaky'(x)
    BlkGemmOp g;
    gemm_init(g, S);
    g.xs[0] = seg(dh, Q, S, Q, 0, 0, S);
    g.wt[0][0] = went(w1, 1, K);
    g.ms[0] = out_rows(dx->p, K, dx->ld, 0, 0, S, nullptr, nullptr);
    g.ms[0].der = seg(x, K, 0, 0, S);
    launch_blk_gemm(g, batch, s);
  }
  if (dw2 || db2) {
    BlkWgOp<false> wg;
    wg_init(wg, S, x->p, (long long)K * x->ld);
    wg.lrelu = 1;
    wg.as[0] = seg(dy, Q, 0, 0, S);
    wg.xs[0] = seg(hidden, Q, 0, 0, S);
    wg.dwt[0][0] = went(dw2, Q, 1);
    wg.dbv[0][0] = db2;
    launch_blk_wgrad(wg, batch, wscr, s);
  }
  if (dw1 || db1) {
    BlkWgOp<false> wg;
    wg_init(wg, S, x->p, (long long)K * x->ld);
    wg.lrelu = 1;
    wg.as[0] = seg(dh, Q, S, Q, 0, 0, S);
    wg.xs[0] = seg(x, K, 0, 0, S);
    wg.dwt[0][0] = went(dw1, K, 1);
    wg.dbv[0][0] = db1;
    launch_blk_wgrad(wg, batch, wscr, s);
  }
  g_block_form = MVN_BLOCK_FORM_GENERIC;
  return check_hip(hipGetLastError(), fn);
}

}  // extern "C"
