// One gated residual layer of the full-sequence forward, PERSISTENT form (C = K = 64, fp32):
// reference arithmetic movenet/modules.py:67-93 -- f,g = dilated k=2 convs;
// z = tanh(f) sigmoid(g); x' = x + Wr z + br; skip (+)= Ws z + bs for t >= RF - 1.
//
// The tile kernel (fused_layer64p_kernel) is built like the backward halves (fused_bwd.h): a
// 256-thread workgroup, two per CU, walks 32-column tiles of its chunk, and BOTH products run in the
// transposed form with their weights in REGISTERS for the whole launch:
//   F'[t][m] = sum_k X[k][t] W[k][m]   X = [x(t-d); x(t)] staged once per tile (128 x 32, pitch 36)
//     wave -> (32 t x 32 channels, tap): filter AND gate block of its channels over the 64 rows
//     of its tap (2 x 32 weights per lane); the two taps' partial sums meet through LDS, each
//     wave finishing half of the block: gate in registers, z / tanh / sigmoid to LDS tiles
//   Y'[t][m2] = sum_c Z[c][t] Wrs[c][m2]   wave -> one 32 x 32 block of [residual | skip] (32 weights)
//   epilogue through the staging tiles as whole-row float4 accesses: tanh, sigmoid, x' = (y + br) + x
//   (x from the staged tile), skip (+)= y + bs.
// The next tile's X waits in registers, then in the second X buffer; five barriers per tile.
// It replaced a per-tile kernel that streamed its 48 KB of weights from L2 through LDS for every
// 128-column tile (21 barriers per tile, 43 % matrix-core utilisation, 174 us per layer at config 2).
// Summation order differs from the two-kernel form (gemm_wx_staged_kernel<FgOpT> then <RsOp>: one
// 128-deep chain) -- two 64-deep partial sums: same values to fp32 rounding, not the same bits.
#pragma once
#include <cstdlib>
#include <type_traits>
#include "common.h"
#include "gemm_family.h"
#include "fused_bwd.h"

namespace mvn {

constexpr int FP_C = 64;  // channels (C = K) of every persistent forward layer kernel

struct FusedFwdPArgs {
  int t_begin, t_end, d, t_skip0, t_base, first_layer;
  const float *wf, *wg;          // (64 out, 64 in, 2 taps)
  const float *wr, *ws;          // (64 out, 64 in)
  const float *br, *bs;          // (64)
  Act xin, xout, th, sg, skip;   // xout.p == NULL: last layer; th/sg.p == NULL: nothing saved
  // conditioned layers (strip kernel only): f,g += Wc ctx(t) + bc   (modules.py:58-63, :75-77)
  const float *wcf = nullptr, *wcg = nullptr, *bcf = nullptr, *bcg = nullptr;  // (64, 64), (64)
  Act ctx = Act{nullptr, 0, 0};
  const float *wpack = nullptr;  // fused_fwd_bf3.h: the layer's LDS image, written once per forward call (or NULL)
  const float *gbias = nullptr;  // global conditioning (fused_layer64s_bf3_kernel<true>): (batch, 128) f | g bias of this layer
};

// 32-column tiles, 256 threads, TWO workgroups per CU (65 KB of LDS each) whose phases run under each
// other's MFMAs.  (A 64-column form -- 512 threads, one workgroup per CU -- was measured and removed.)
__global__ __launch_bounds__(256, 2) void fused_layer64p_kernel(FusedFwdPArgs a, int chunks_per_b, int chunk_t) {
  constexpr int C = 64, TT = 32, LD = TT + 4, NTH = 256;
  extern __shared__ __attribute__((aligned(16))) float fp_lds[];
  float (*X)[128][LD] = (float (*)[128][LD])fp_lds;              // [2]: x(t - d) rows | x(t) rows
  float (*Z)[LD] = (float (*)[LD])(fp_lds + 2 * 128 * LD);       // gated activation
  float (*S1)[LD] = (float (*)[LD])(fp_lds + (2 * 128 + 64) * LD);   // f partials -> tanh -> x'
  float (*S2)[LD] = (float (*)[LD])(fp_lds + (2 * 128 + 128) * LD);  // g partials -> sigmoid -> skip
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / chunks_per_b, ch = blockIdx.x - b * chunks_per_b;
  const int li = lane & 31, lh = lane >> 5, h4 = 4 * lh;
  const int tb = (a.t_begin & ~TILE_ALIGN) + ch * chunk_t, te = min(a.t_end, tb + chunk_t);
  const int skip_lo = max(a.t_begin, a.t_skip0);

  // ---- the weights reach their registers through LDS: a lane's values lie 512 (256) bytes apart
  // in the (out, in, tap) / (out, in) tensors -- fetched straight from global memory every wave
  // instruction touched 64 cache lines, 49 000 line requests per workgroup: longer than its tiles
  // (three passes of 32 KB through the tile buffers: filter, gate, residual | skip)
  const int cc = wave & 1, kh = wave / 2;     // first product: block cc, tap kh
  const int t2 = wave >> 2, mt = wave & 3;    // second product: block (t2, mt)
  float wfr[32], wgr[32], wrs[32];
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    const float *src = pass == 0 ? a.wf : pass == 1 ? a.wg : a.wr;
    for (int i = tid; i < (pass < 2 ? 2048 : 1024); i += NTH) *(f4 *)&fp_lds[4 * i] = *(const f4 *)&src[4 * i];
    if (pass == 2)
      for (int i = tid; i < 1024; i += NTH) *(f4 *)&fp_lds[4096 + 4 * i] = *(const f4 *)&a.ws[4 * i];
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
      if (pass < 2) {
        const float v = fp_lds[((32 * cc + li) * C + 2 * kk + lh) * 2 + kh];
        if (pass == 0) wfr[kk] = v; else wgr[kk] = v;
      } else {
        wrs[kk] = fp_lds[(mt < 2 ? 0 : 4096) + (32 * (mt & 1) + li) * C + 2 * kk + lh];
      }
    }
    __syncthreads();
  }
  const float bias2 = (mt < 2 ? a.br : a.bs)[32 * (mt & 1) + li];

  // ---- staging: thread -> rows (tid / TPR) + 32 p, columns 4 (tid % TPR) .. +3
  constexpr int TPR = TT / 4;  // threads per row
  const int srow = tid / TPR, st = 4 * (tid % TPR);
  f4 xreg[4], kreg[2];
  auto interior = [&](int t0) { return t0 >= a.t_begin && t0 + TT <= te; };
  auto gload_x = [&](int t0) {
    int srow_q = srow;
    asm volatile("" : "+v"(srow_q));
    const int t = t0 + st;
    if (interior(t0)) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        xreg[p] = ldg4(a.xin.at(b, (32 * p + srow_q) & (C - 1), 0) + t - (p < 2 ? a.d : 0));
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        xreg[p] = ld4_edge(a.xin.at(b, (32 * p + srow_q) & (C - 1), 0) - (p < 2 ? a.d : 0), t, a.t_begin, te);
    }
  };
  // the skip accumulator's old values for this tile (columns t - t_base, live from skip_lo)
  auto gload_skip = [&](int t0) {
    int srow_q = srow;
    asm volatile("" : "+v"(srow_q));
    const int t = t0 + st;
    if (a.first_layer || t0 + TT <= skip_lo) {
      kreg[0] = kreg[1] = kZero4;
    } else if (t0 >= skip_lo && t0 + TT <= te) {
#pragma unroll
      for (int p = 0; p < 2; ++p) kreg[p] = ldg4(a.skip.at(b, 32 * p + srow_q, 0) + (t - a.t_base));
    } else {
#pragma unroll
      for (int p = 0; p < 2; ++p) kreg[p] = ld4_edge(a.skip.at(b, 32 * p + srow_q, 0) - a.t_base, t, skip_lo, te);
    }
  };
  auto lstore_x = [&](int buf) {
#pragma unroll
    for (int p = 0; p < 4; ++p) *(f4 *)&X[buf][32 * p + srow][st] = xreg[p];
  };
  // rows srow + 32 p (p < 2) of a 64-row staging tile -> dst, columns inside [lo, te)
  auto store_rows = [&](const Act &dst, float (*S)[LD], int t0, int lo, int col_shift) {
    const int t = t0 + st;
    float *base = dst.p + (size_t)b * dst.sb + (t - col_shift);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int row = 32 * p + srow;
      const f4 v = *(const f4 *)&S[row][st];
      float *q = base + (size_t)row * dst.ld;
      if (t >= lo && t + 3 < te) {
        *(f4 *)q = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (t + e >= lo && t + e < te) q[e] = f4_get(v, e);
      }
    }
  };

  gload_x(tb);
  lstore_x(0);
  __syncthreads();
  int cur = 0;
  for (int t0 = tb; t0 < te; t0 += TT, cur ^= 1) {
    const bool more = t0 + TT < te;
    gload_skip(t0);
    if (more) gload_x(t0 + TT);
    __builtin_amdgcn_sched_barrier(0);
    // ---- f | g partial sums of this wave's tap: 2 x 32 MFMAs, LDS operands one step ahead
    f32x16 accf, accg;
#pragma unroll
    for (int r = 0; r < 16; ++r) accf[r] = accg[r] = 0.f;
    {
      float av[2][8];
      auto fetch = [&](int g, int S) {
#pragma unroll
        for (int i = 0; i < 8; ++i) av[S][i] = X[cur][64 * kh + 2 * (8 * g + i) + lh][li];
      };
      fetch(0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int S = g & 1;
        if (g + 1 < 4) fetch(g + 1, S ^ 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          accf = __builtin_amdgcn_mfma_f32_32x32x2f32(av[S][i], wfr[8 * g + i], accf, 0, 0, 0);
          accg = __builtin_amdgcn_mfma_f32_32x32x2f32(av[S][i], wgr[8 * g + i], accg, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- the taps meet: this wave finishes t-groups q = 2 kh, 2 kh + 1 of its block and hands the
    // other two to its partner (the same block, other tap) through the staging tiles
    // (the t-group index is a compile-time constant on either side of the branch: indexed at run
    // time the accumulator registers were moved through s_set_gpr_idx, 24 switches per tile)
    auto hand_over = [&](auto QB) {
      constexpr int q0 = decltype(QB)::value;
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        const int q = q0 + qq, tc = 8 * q + h4;
        *(f4 *)&S1[32 * cc + li][tc] = f4{accf[4 * q], accf[4 * q + 1], accf[4 * q + 2], accf[4 * q + 3]};
        *(f4 *)&S2[32 * cc + li][tc] = f4{accg[4 * q], accg[4 * q + 1], accg[4 * q + 2], accg[4 * q + 3]};
      }
    };
    if (kh == 0) hand_over(std::integral_constant<int, 2>()); else hand_over(std::integral_constant<int, 0>());
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the loads above have had the MFMAs to land (cf. fused_bwd.h)
    __syncthreads();
    auto finish = [&](auto QB) {
      constexpr int q0 = decltype(QB)::value;
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        const int q = q0 + qq, tc = 8 * q + h4;
        const f4 pf = *(const f4 *)&S1[32 * cc + li][tc], pg = *(const f4 *)&S2[32 * cc + li][tc];
        f4 tv, sv;
        tv.x = tanh_fast(accf[4 * q] + pf.x);     sv.x = sigmoid_fast(accg[4 * q] + pg.x);
        tv.y = tanh_fast(accf[4 * q + 1] + pf.y); sv.y = sigmoid_fast(accg[4 * q + 1] + pg.y);
        tv.z = tanh_fast(accf[4 * q + 2] + pf.z); sv.z = sigmoid_fast(accg[4 * q + 2] + pg.z);
        tv.w = tanh_fast(accf[4 * q + 3] + pf.w); sv.w = sigmoid_fast(accg[4 * q + 3] + pg.w);
        *(f4 *)&Z[32 * cc + li][tc] = f4{tv.x * sv.x, tv.y * sv.y, tv.z * sv.z, tv.w * sv.w};
        *(f4 *)&S1[32 * cc + li][tc] = tv;  // (the slots this lane has just read)
        *(f4 *)&S2[32 * cc + li][tc] = sv;
      }
    };
    if (kh == 0) finish(std::integral_constant<int, 0>()); else finish(std::integral_constant<int, 2>());
    if (more) lstore_x(cur ^ 1);
    __syncthreads();
    // ---- tanh / sigmoid leave for the backward pass; residual | skip block of this wave
    // (their four row stores per thread are issued between the MFMA steps below)
    auto store_row = [&](const Act &dst, float (*S)[LD], int p) {
      const int t = t0 + st, row = 32 * p + srow;
      const f4 v = *(const f4 *)&S[row][st];
      float *q = dst.p + (size_t)b * dst.sb + (size_t)row * dst.ld + t;
      if (t >= a.t_begin && t + 3 < te) {
        *(f4 *)q = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (t + e >= a.t_begin && t + e < te) q[e] = f4_get(v, e);
      }
    };
    f32x16 accy;
#pragma unroll
    for (int r = 0; r < 16; ++r) accy[r] = 0.f;
    {
      float zv[2][8];
      auto fetch = [&](int g, int S) {
#pragma unroll
        for (int i = 0; i < 8; ++i) zv[S][i] = Z[2 * (8 * g + i) + lh][32 * t2 + li];
      };
      fetch(0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int S = g & 1;
        if (g + 1 < 4) fetch(g + 1, S ^ 1);
        if (a.th.p) store_row(g < 2 ? a.th : a.sg, g < 2 ? S1 : S2, g & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) accy = __builtin_amdgcn_mfma_f32_32x32x2f32(zv[S][i], wrs[8 * g + i], accy, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();  // tanh / sigmoid have been read: the staging tiles take x' and the skip term
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int tc = 32 * t2 + 8 * q + h4, row = 32 * (mt & 1) + li;
      f4 v = f4{accy[4 * q] + bias2, accy[4 * q + 1] + bias2, accy[4 * q + 2] + bias2, accy[4 * q + 3] + bias2};
      if (mt < 2) {
        const f4 x = *(const f4 *)&X[cur][C + row][tc];
        *(f4 *)&S1[row][tc] = f4{v.x + x.x, v.y + x.y, v.z + x.z, v.w + x.w};
      } else {
        *(f4 *)&S2[row][tc] = v;
      }
    }
    __syncthreads();
    if (a.xout.p) store_rows(a.xout, S1, t0, a.t_begin, 0);
    {
      // skip (+)= term, columns t - t_base, live from skip_lo
      const int t = t0 + st;
      float *base = a.skip.p + (size_t)b * a.skip.sb + (t - a.t_base);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int row = 32 * p + srow;
        const f4 v = *(const f4 *)&S2[row][st], o = kreg[p];
        const f4 r = a.first_layer ? v : f4{o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w};
        float *q = base + (size_t)row * a.skip.ld;
        if (t >= skip_lo && t + 3 < te) {
          *(f4 *)q = r;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (t + e >= skip_lo && t + e < te) q[e] = f4_get(r, e);
        }
      }
    }
    __syncthreads();  // the staging tiles are free for the next tile's partial sums
  }
}

// ----------------------------------------------------------------------------------------
// STRIP form: one WAVE owns a strip of 32 time columns and runs the whole layer on it without a
// single barrier (r2b timing builds: the tile kernel above, 32 and 64 columns, spent 45 % of its time with waves
// waiting at barriers for a sibling whose SIMD is held by another wave's MFMA burst).
//   * both weight matrices sit in LDS for the whole launch (96 KB, read-only), laid out per MFMA
//     block and lane so that one ds_read_b128 feeds four MFMAs (A operand: lane -> output row);
//   * the strip's input, [x(t-d); x(t)] for 32 columns, goes from global memory straight into 64
//     registers per lane as the B operand (lane -> column); the k order pairs channel c (lane
//     half 0) with c + 4 (lane half 1), c running over the channels with bit 2 clear -- which
//     are exactly the channels a lane of that half holds in the ACCUMULATOR layout (rows
//     (r & 3) + 8 (r >> 2) + 4 lh), so that
//       - f and g of a channel meet in one lane: gate in registers, no exchange;
//       - z, computed in accumulator order, IS the B operand of the second product;
//       - the residual add finds x(t) of its channel in the lane's own input registers;
//   * tanh, sigmoid, x' and the skip term leave as dword stores, 128 contiguous bytes per channel
//     and lane half (a whole cache line); the skip accumulator's old values are fetched under
//     the second product into the dead x(t-d) registers.
// Per strip and wave: 384 MFMAs, 96 ds_read_b128, ~290 vector-memory instructions.  The two
// waves of a SIMD are independent: one's loads and stores run under the other's MFMAs.
// ----------------------------------------------------------------------------------------
// HAS_CTX: the conditioned layer -- the context is a third K block of the first product (96 KB of
// f|g weights), its 32 registers are the ones the unconditioned kernel uses to fetch x(t) a strip ahead.
// Strips start at multiples of 32 columns of the absolute time axis (rows are 256-byte aligned: every
// 128-byte row segment a store instruction writes is ONE cache line, not two halves: 148.6 -> 142.4 us
// per layer), and tanh / sigmoid -- written once, read by the backward pass much later -- leave with
// the non-temporal hint (-> 135.8 us; on x' and the skip sums, which the next layer reads, it costs 5 us).
//
// Where the text lives: the strip scaffold is written once, csrc/fwd_layer64s_body.inc, and is the body of
// fused_layer64s_kernel<HAS_CTX> (the fp32-MFMA form described here) and of its siblings -- bf16 x 3
// (fused_fwd_bf3.h), one bf16 plane (fused_bf16.h).  The kernels' signatures stand together in fused_bf16.h,
// in front of the LAYER_FORMS table, where every policy's helpers are in sight.  This header holds what
// the body shares with the dense strip kernels.
constexpr int FS_AUX_SAVE = 2;  // nt
#define FS_FENCE(x) asm volatile("" : "+s"(x))  // (a row pitch `ld`: its row * ld products are re-formed behind it)
// the product policies of fwd_layer64s_body.inc (FS_FORM)
#define FS_FORM_F32 0
#define FS_FORM_BF3 1
#define FS_FORM_BF16 2
#define FS_FORM_CTXW2 3

// A packed weight image (BYTES of it, from `src_`) into the LDS array `lds_` by the workgroup's 512 threads (reads
// `tid`), linearly: every load is in flight before the first store.  Text, not a function: as a __forceinline__
// function the partly filled last vector came out zero-filled in front of its masked load (four v_mov per copy) and
// the loads took other registers -- other instructions in every kernel that copies an image.
#define LDS_IMAGE_COPY(lds_, src_, BYTES)                                   \
  {                                                                         \
    typedef float f4_ __attribute__((ext_vector_type(4)));                  \
    constexpr int N16 = (BYTES) / 16, PER = (N16 + 511) / 512;              \
    const f4_ *src = (const f4_ *)(src_);                                   \
    f4_ v[PER];                                                             \
    _Pragma("unroll") for (int i = 0; i < PER; ++i) {                       \
      const int at = tid + 512 * i;                                         \
      if (at < N16) v[i] = src[at];                                         \
    }                                                                       \
    _Pragma("unroll") for (int i = 0; i < PER; ++i) {                       \
      const int at = tid + 512 * i;                                         \
      if (at < N16) ((f4_ *)(lds_))[at] = v[i];                             \
    }                                                                       \
  }

// ----------------------------------------------------------------------------------------
// The strip form for the head's 1x1 convs with 64 x 256 weights (conv1 forward: 64 -> 256 rows,
// leaky-ReLU in and out; its data gradient: 256 -> 64 rows through W^T, times the leaky-ReLU
// derivative): the generic kernel reads a 64-row input once per 64-row OUTPUT block (conv1: four
// times) and ran at 1.5 TB/s.  Same recipe as fused_layer64s_kernel: weights in LDS (64 KB), the
// strip's input in registers as the B operand, raw buffer accesses, no barrier.
//   IN: 0 identity, 1 leaky-ReLU on load;  OUT: 1 leaky(y + bias), 2 y * leaky'(ref)
// ----------------------------------------------------------------------------------------
struct DenseStripArgs {
  int t_begin, t_end, t_out_end;
  const float *wmat;  // W[m][k] = TRANSPOSED ? wmat[k * ldw + m] : wmat[m * ldw + k]
  int ldw;
  const float *bias;
  Act xin, yout, ref;
};

// M = output rows per workgroup (blockIdx.y selects the row block): 64 x 256 weights for conv1
// (one block of 256 rows), 256 x 128 for conv2 and its data gradient (two blocks: the input is
// read twice instead of four times, 128 of its 256 rows' weights = 128 KB in LDS).
template <int K, int M, int IN, int OUT, bool TRANSPOSED>
__global__ __launch_bounds__(512, 1) void dense_strip_kernel(DenseStripArgs a, int chunks_per_b, int chunk_t) {
  static_assert(K * M <= 32768 && K % 8 == 0 && M % 32 == 0, "at most 128 KB of weights");
  constexpr int NB = M / 32, NK4 = K / 8;
  extern __shared__ __attribute__((aligned(16))) float ds_lds[];
  float *W = ds_lds, *BI = ds_lds + K * M;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / chunks_per_b, ch = blockIdx.x - b * chunks_per_b;
  const int m_base = blockIdx.y * M;
  const int li = lane & 31, lh = lane >> 5;
  const int tb = (a.t_begin & ~TILE_ALIGN) + ch * chunk_t, te = min(a.t_end, tb + chunk_t);
  for (int r = tid; r < K * M; r += 512) {  // source order: coalesced
    const int m = TRANSPOSED ? r % M : r / K, k = TRANSPOSED ? r / M : r % K;
    const int kk = k >> 1;
    const float v = TRANSPOSED ? a.wmat[(size_t)k * a.ldw + m_base + m] : a.wmat[(size_t)(m_base + m) * a.ldw + k];
    W[(((m >> 5) * NK4 + (kk >> 2)) * 64 + (m & 31) + 32 * (k & 1)) * 4 + (kk & 3)] = v;
  }
  if (OUT != 2 && tid < M) BI[tid] = a.bias[m_base + tid];
  __syncthreads();
  const unsigned wa = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)W + 16u * lane;
  typedef float dsv4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) dsv4 lds_v4;
  constexpr int RSRC = 0x00020000;
  const __amdgpu_buffer_rsrc_t xb = __builtin_amdgcn_make_buffer_rsrc((void *)(a.xin.p + (size_t)b * a.xin.sb), 0, 0x7FFFFFFF, RSRC);
  const __amdgpu_buffer_rsrc_t yb = __builtin_amdgcn_make_buffer_rsrc(
      (void *)(a.yout.p + (size_t)b * a.yout.sb + (size_t)m_base * a.yout.ld), 0, 0x7FFFFFFF, RSRC);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      (void *)(a.ref.p + (size_t)b * a.ref.sb + (size_t)m_base * a.ref.ld), 0, 0x7FFFFFFF, RSRC);
  int xld4 = 4 * a.xin.ld, yld4 = 4 * a.yout.ld, rld4 = 4 * a.ref.ld;
  for (int t0 = tb + 32 * wave; t0 < te; t0 += 32 * 8) {
    const int t = t0 + li;
    const bool live = t >= a.t_begin && t < te, out_live = live && t < a.t_out_end;
    const int tc = live ? t : a.t_begin;
    const int ox = 4 * (lh * a.xin.ld + tc), oy = 4 * (4 * lh * a.yout.ld + tc), orf = 4 * (4 * lh * a.ref.ld + tc);
    float xr[K / 2];
    FS_FENCE(xld4);
#pragma unroll
    for (int kk = 0; kk < K / 2; ++kk) {
      float v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xb, ox, 2 * kk * xld4, 0));
      if (IN == 1) v = leaky(v);
      xr[kk] = live ? v : 0.f;
    }
    // (all of the strip's loads are issued before its first MFMA: the scheduler otherwise requests
    // a K = 256 input just in time, 65 registers and a memory round trip every few MFMAs)
    __builtin_amdgcn_sched_barrier(0);
    f32x16 acc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
    for (int k4 = 0; k4 < NK4; ++k4) {
      dsv4 aw[NB];
#pragma unroll
      for (int blk = 0; blk < NB; ++blk) aw[blk] = *(const lds_v4 *)(uintptr_t)(wa + 4u * (unsigned)((blk * NK4 + k4) * 256));
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int blk = 0; blk < NB; ++blk)
          acc[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[blk][e], xr[4 * k4 + e], acc[blk], 0, 0, 0);
    }
    FS_FENCE(yld4);
    FS_FENCE(rld4);
    if (out_live) {
#pragma unroll
      for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m0 = 32 * blk + (r & 3) + 8 * (r >> 2);
          float y = acc[blk][r];
          if (OUT == 0) {
            y = y + BI[m0 + 4 * lh];
          } else if (OUT == 1) {
            y = leaky(y + BI[m0 + 4 * lh]);
          } else {
            const float rv = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rb, orf, m0 * rld4, 0));
            y = y * (rv > 0.f ? 1.0f : kLeakySlope);
          }
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y), yb, oy, m0 * yld4, 0);
        }
    }
  }
}

// `m_total` output rows = m_total / M row blocks
template <int K, int M, int IN, int OUT, bool TRANSPOSED>
static int launch_dense_strip(const DenseStripArgs &a, int m_total, int batch, hipStream_t s) {
  const int nt = a.t_end - (a.t_begin & ~TILE_ALIGN);
  if (a.t_end <= a.t_begin || batch <= 0) return MVN_OK;
  int chunks, chunk_t;
  fb_chunks(nt, batch * (m_total / M), 1, &chunks, &chunk_t, 256);
  const void *fn = (const void *)dense_strip_kernel<K, M, IN, OUT, TRANSPOSED>;
  const int rc = ensure_max_dynamic_lds(fn, "hipFuncSetAttribute(dense_strip)");
  if (rc) return rc;
  hipLaunchKernelGGL((dense_strip_kernel<K, M, IN, OUT, TRANSPOSED>), dim3(chunks * batch, m_total / M), dim3(512),
                     (K * M + M) * sizeof(float), s, a, chunks, chunk_t);
  return MVN_OK;
}

}  // namespace mvn
