// fp32 products on the bf16 matrix cores: the strip forward of an audio-only layer, form "bf16 x 3".
//
// CDNA4's fp32 MFMA (v_mfma_f32_32x32x2_f32: 64 cycles for 4096 FLOP) is 1/16 of its bf16 MFMA
// (v_mfma_f32_32x32x16_bf16: <= 32 cycles for 32768 FLOP), and an fp32 MFMA holds the SIMD's vector
// lanes while it runs (scripts/probes/mfma_valu_overlap.hip) where a bf16 MFMA leaves 24 of its 32
// cycles to other instructions.  An fp32 number is EXACTLY the sum of three bf16 numbers
//     x = h + m + l,   h = top16(x),  m = top16(x - h),  l = top16(x - h - m)      (8 + 8 + 8 mantissa bits;
// the two subtractions are exact), so a product of two fp32 numbers is the sum of nine bf16 products, each
// exact in the fp32 accumulator; the six of them with weight >= 2^-16 (hh, hm, mh, mm, hl, lh) carry
// everything above 2^-24 of the product -- what an fp32 multiply keeps.  Six bf16 MFMAs replace the eight fp32
// MFMAs of a 32 x 32 x 16 block: 2.7 - 5 x less matrix time (scripts/probes/mfma_bf16_split.hip: 2048 -> 470
// cycles per block and SIMD, the split of the B operand included), with fp32's exponent range (no scaling,
// no overflow: bf16 has fp32's exponent) and fp32-class error (numpy model in DESIGN 4.3b: max error of a
// 256-term product 4.7e-7 of the output range against 5.7e-7 for fp32 sums in numpy's order).
//
// Same structure as fused_layer64s_kernel<false> (fused_fwd.h): one wave owns a strip of 32 columns, no
// barrier, the strip's input goes from global memory into registers in ACCUMULATOR order and is the B operand;
// gate in registers; z in accumulator order is the second product's B operand.  What changes:
//   * weights in LDS as three bf16 planes, [block][k-step of 16][plane][lane][8 bf16]: one ds_read_b128 per
//     plane feeds an MFMA's A operand (lane -> output row, lane half -> which 8 of the step's 16 inputs); 144 KB;
//   * a k-step takes 8 consecutive input registers of the lane (8 channels of its lane half), split into three
//     packed planes (22 vector instructions) that all four row blocks share: 6 MFMAs each;
//   * per strip 288 bf16 MFMAs instead of 384 fp32 ones, 144 ds_read_b128 instead of 96.
#pragma once
#include "bf3.h"

namespace mvn {

// acc += A (three planes at LDS byte address `wa`, 1 KB apart) x B (three planes): smallest terms first
__device__ __forceinline__ void bf3_mfma6(f32x16 &acc, unsigned wa, const u32x4 &bh, const u32x4 &bm, const u32x4 &bl) {
  typedef __attribute__((address_space(3))) u32x4 lds_u4;
  const u32x4 ah = *(const lds_u4 *)(uintptr_t)wa;
  const u32x4 am = *(const lds_u4 *)(uintptr_t)(wa + 1024u);
  const u32x4 al = *(const lds_u4 *)(uintptr_t)(wa + 2048u);
#if MVN_EXP == 74  // (timing build of fused_bwd_l.h: no MFMAs)
#define BF3_MF(a_, b_) acc[0] += __uint_as_float(a_[0] ^ b_[0])
#else
#define BF3_MF(a_, b_) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a_), __builtin_bit_cast(bf16x8, b_), acc, 0, 0, 0)
#endif
  BF3_MF(al, bh);
  BF3_MF(ah, bl);
  BF3_MF(am, bm);
  BF3_MF(am, bh);
  BF3_MF(ah, bm);
  BF3_MF(ah, bh);
#undef BF3_MF
}

// acc[0..3] += W (4 row blocks, NKS k-steps, three planes each in LDS) x B, software-pipelined: step (ks, blk)
// requests the NEXT step's three A planes first, then issues its six MFMAs with a pair of the next k-step's B
// values split between them -- a ds_read has six MFMAs (>= 192 cycles) to arrive, the 88 vector instructions of a
// split are spread over the 24 MFMAs of a k-step, which leave 24 of their 32 cycles to them.  The scheduling
// groups pin that order (the compiler's own put each read right in front of its MFMA: 44 % of the wave cycles
// were waits on LDS, SQ_WAIT_ANY of the build without global accesses).
//   BVAL: expression of (ks_, e_) = value e_ of k-step ks_'s eight
#define BF3_PRODUCT(NKS, WA, WB, BVAL)                                                                              \
  {                                                                                                                 \
    typedef __attribute__((address_space(3))) u32x4 lds_u4_;                                                        \
    u32x4 A_[2][3], B_[2][3];                                                                                       \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                              \
      const int ks_ = 0;                                                                                            \
      float p0_, p1_;                                                                                               \
      { const int e_ = 2 * i_; p0_ = (BVAL); }                                                                      \
      { const int e_ = 2 * i_ + 1; p1_ = (BVAL); }                                                                  \
      unsigned h_, m_, l_;                                                                                          \
      bf3_split2(p0_, p1_, h_, m_, l_);                                                                             \
      B_[0][0][i_] = h_; B_[0][1][i_] = m_; B_[0][2][i_] = l_;                                                      \
    }                                                                                                               \
    _Pragma("unroll") for (int pl_ = 0; pl_ < 3; ++pl_) A_[0][pl_] = *(const lds_u4_ *)(uintptr_t)((WA) + 1024u * pl_); \
    _Pragma("unroll") for (int ksx_ = 0; ksx_ < (NKS); ++ksx_) {                                                    \
      _Pragma("unroll") for (int blk_ = 0; blk_ < 4; ++blk_) {                                                      \
        const int s_ = ksx_ * 4 + blk_;                                                                             \
        if (s_ + 1 < 4 * (NKS)) {                                                                                   \
          const int nk_ = (s_ + 1) >> 2, nb_ = (s_ + 1) & 3;                                                        \
          const unsigned ad_ = (nb_ < 2 ? (WA) : (WB)) + 3072u * (unsigned)((nb_ & 1) * (NKS) + nk_);               \
          _Pragma("unroll") for (int pl_ = 0; pl_ < 3; ++pl_)                                                       \
            A_[(s_ + 1) & 1][pl_] = *(const lds_u4_ *)(uintptr_t)(ad_ + 1024u * pl_);                               \
        }                                                                                                           \
        if (ksx_ + 1 < (NKS)) {                                                                                     \
          const int ks_ = ksx_ + 1;                                                                                 \
          float p0_, p1_;                                                                                           \
          { const int e_ = 2 * blk_; p0_ = (BVAL); }                                                                \
          { const int e_ = 2 * blk_ + 1; p1_ = (BVAL); }                                                            \
          unsigned h_, m_, l_;                                                                                      \
          bf3_split2(p0_, p1_, h_, m_, l_);                                                                         \
          B_[(ksx_ + 1) & 1][0][blk_] = h_; B_[(ksx_ + 1) & 1][1][blk_] = m_; B_[(ksx_ + 1) & 1][2][blk_] = l_;     \
        }                                                                                                           \
        const u32x4 ah_ = A_[s_ & 1][0], am_ = A_[s_ & 1][1], al_ = A_[s_ & 1][2];                                  \
        const u32x4 bh_ = B_[ksx_ & 1][0], bm_ = B_[ksx_ & 1][1], bl_ = B_[ksx_ & 1][2];                            \
        BF3_MF1(acc[blk_], al_, bh_);                                                                               \
        BF3_MF1(acc[blk_], ah_, bl_);                                                                               \
        BF3_MF1(acc[blk_], am_, bm_);                                                                               \
        BF3_MF1(acc[blk_], am_, bh_);                                                                               \
        BF3_MF1(acc[blk_], ah_, bm_);                                                                               \
        BF3_MF1(acc[blk_], ah_, bh_);                                                                               \
        __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);                                                          \
        _Pragma("unroll") for (int g_ = 0; g_ < 6; ++g_) {                                                          \
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                        \
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                                                        \
        }                                                                                                           \
      }                                                                                                             \
    }                                                                                                               \
  }
#define BF3_MF1(c_, a_, b_) \
  c_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a_), __builtin_bit_cast(bf16x8, b_), c_, 0, 0, 0)

constexpr int FS3_W1_BYTES = 4 * 8 * 3 * 1024, FS3_W2_BYTES = 4 * 4 * 3 * 1024;  // 96 KB + 48 KB
constexpr int FS3_LDS_BYTES = FS3_W1_BYTES + FS3_W2_BYTES + 128 * 4;

// The layer's weights as the kernel's LDS image: W1 [4 blocks][8 k-steps][3 planes][64 lanes][8 bf16], W2 [4][4][3][64][8],
// then br | bs as floats.  Input register j of a lane of half lh holds channel (j & 3) + 8 (j >> 2) + 4 lh; k-step ks
// takes registers 8 ks' .. 8 ks' + 7: ks 0..3 of x(t) (tap 1), ks 4..7 of x(t - d) (tap 0).  `img` may be LDS or global.
template <class Ptr>
__device__ __forceinline__ void fs3_stage_weights(Ptr img, const float *wf, const float *wg, const float *wr,
                                                  const float *ws, const float *br, const float *bs, int tid, int nthreads) {
  unsigned short *W1 = (unsigned short *)img;
  unsigned short *W2 = (unsigned short *)(img + FS3_W1_BYTES);
  float *BI = (float *)(img + FS3_W1_BYTES + FS3_W2_BYTES);
  for (int sI = tid; sI < 2 * 8192; sI += nthreads) {
    const int g = sI >> 13, r = sI & 8191;        // g: 0 filter, 1 gate; source (out, in, tap)
    const int tap = r & 1, kc = (r >> 1) & 63, cm = r >> 7;
    const int lhs = (kc >> 2) & 1, j = (kc & 3) + 4 * (kc >> 3);
    const int blk = 2 * g + (cm >> 5), ln = (cm & 31) + 32 * lhs, ks = (tap ? 0 : 4) + (j >> 3);
    unsigned short h, m, l;
    bf3_split1((g ? wg : wf)[r], h, m, l);
    const int at = (((blk * 8 + ks) * 3) * 64 + ln) * 8 + (j & 7);
    W1[at] = h;
    W1[at + 512] = m;
    W1[at + 1024] = l;
  }
  for (int sI = tid; sI < 2 * 4096; sI += nthreads) {
    const int g = sI >> 12, r = sI & 4095;        // g: 0 residual, 1 skip; source (out, in)
    const int kc = r & 63, m2 = r >> 6;
    const int lhs = (kc >> 2) & 1, j = (kc & 3) + 4 * (kc >> 3);
    const int blk = 2 * g + (m2 >> 5), ln = (m2 & 31) + 32 * lhs, ks = j >> 3;
    unsigned short h, m, l;
    bf3_split1((g ? ws : wr)[r], h, m, l);
    const int at = (((blk * 4 + ks) * 3) * 64 + ln) * 8 + (j & 7);
    W2[at] = h;
    W2[at + 512] = m;
    W2[at + 1024] = l;
  }
  for (int i = tid; i < 128; i += nthreads) BI[i] = i < 64 ? br[i] : bs[i - 64];
}

// up to FS3_PACK_LAYERS layers per launch (blockIdx.y = layer): images FS3_PACK_F floats apart
constexpr int FS3_PACK_LAYERS = 32, FS3_PACK_F = FS3_LDS_BYTES / 4;
struct Fs3PackArgs {
  const float *wf[FS3_PACK_LAYERS], *wg[FS3_PACK_LAYERS], *wr[FS3_PACK_LAYERS], *ws[FS3_PACK_LAYERS];
  const float *br[FS3_PACK_LAYERS], *bs[FS3_PACK_LAYERS];
};
// the context convs of the same layers, for the pack kernels of the conditioned forms (fsc_pack_kernel below,
// fb16c_pack_kernel in fused_bf16.h)
struct Fb16cPackArgs {
  const float *wcf[FS3_PACK_LAYERS], *wcg[FS3_PACK_LAYERS], *bcf[FS3_PACK_LAYERS], *bcg[FS3_PACK_LAYERS];
};
__global__ __launch_bounds__(256) void fs3_pack_kernel(Fs3PackArgs p, float *dst) {
  const int l = blockIdx.y;
  fs3_stage_weights((unsigned char *)(dst + (size_t)l * FS3_PACK_F), p.wf[l], p.wg[l], p.wr[l], p.ws[l], p.br[l], p.bs[l],
                    blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}
// (fused_layer64s_bf3_kernel itself: the strip scaffold, csrc/fwd_layer64s_body.inc, under FS_FORM_BF3 -- its signature
// stands in fused_bf16.h with the other strip kernels')

// ----------------------------------------------------------------------------------------
// The CONDITIONED layer (fused_layer64s_kernel<true>, fused_fwd.h) with what fits of this on it: its f | g product has
// three K blocks (x(t - d), x(t), context: 96 KB of fp32 MFMA operands, 144 KB as bf16 planes) and does not fit
// as planes beside anything; the residual | skip product does (48 KB instead of 32: 145 KB in all) and runs on the
// bf16 matrix cores -- 96 bf16 MFMAs per strip instead of 128 fp32 ones, a quarter of the kernel's fp32 MFMA time
// gone.  The layer's LDS image (W1 in fp32 MFMA order, W2 as planes, the four bias vectors) is written once per
// forward call by fsc_pack_kernel and copied linearly (the staging loops of the fp32 kernel: ~8 us per launch).
// ----------------------------------------------------------------------------------------
// LDS image (exactly the CU's 160 KB): the x(t - d) block of W1 as planes (48 KB: it too on the bf16 matrix cores), the
// x(t) and context blocks as fp32 MFMA operands (64 KB), W2 as planes (48 KB).  The four bias vectors do not fit any
// more: each lives in ONE register (lane i holds element i) and is read by ds_bpermute where the LDS copy was read.
constexpr int FSC_XD_BYTES = 4 * 4 * 3 * 1024;                               // [4 blocks][4 k-steps][3 planes][64 lanes][8 bf16]
constexpr int FSC_W1_BYTES = 4 * 16 * 1024;                                  // [4 blocks][16 k-step groups][64 lanes][4] floats
constexpr int FSC_LDS_BYTES = FSC_XD_BYTES + FSC_W1_BYTES + FS3_W2_BYTES, FSC_PACK_F = FSC_LDS_BYTES / 4;
static_assert(FSC_LDS_BYTES == 160 * 1024, "the conditioned layer's image fills a CU's LDS");
__global__ __launch_bounds__(256) void fsc_pack_kernel(Fs3PackArgs p, Fb16cPackArgs c, float *dst) {
  const int l = blockIdx.y, tid = blockIdx.x * 256 + threadIdx.x, nthreads = gridDim.x * 256;
  unsigned char *img = (unsigned char *)(dst + (size_t)l * FSC_PACK_F);
  unsigned short *XD = (unsigned short *)img;
  float *W1 = (float *)(img + FSC_XD_BYTES);
  unsigned short *W2 = (unsigned short *)(img + FSC_XD_BYTES + FSC_W1_BYTES);
  constexpr int NK1 = 16;
  for (int sI = tid; sI < 2 * 8192; sI += nthreads) {  // filter | gate, source (out, in, tap)
    const int g = sI >> 13, r = sI & 8191;
    const int tap = r & 1, kc = (r >> 1) & 63, cm = r >> 7;
    const int lhs = (kc >> 2) & 1, j = (kc & 3) + 4 * (kc >> 3);
    const int blk = 2 * g + (cm >> 5), ln = (cm & 31) + 32 * lhs;
    const float w = (g ? p.wg[l] : p.wf[l])[r];
    if (tap) {  // x(t): fp32 MFMA operand, k-step groups 0..7
      W1[((blk * NK1 + (j >> 2)) * 64 + ln) * 4 + (j & 3)] = w;
    } else {    // x(t - d): three planes, k-step j >> 3
      unsigned short h, m, lo;
      bf3_split1(w, h, m, lo);
      const int at = (((blk * 4 + (j >> 3)) * 3) * 64 + ln) * 8 + (j & 7);
      XD[at] = h;
      XD[at + 512] = m;
      XD[at + 1024] = lo;
    }
  }
  for (int sI = tid; sI < 2 * 4096; sI += nthreads) {  // context convs, source (out, in): k-step groups 8..15
    const int g = sI >> 12, r = sI & 4095;
    const int kc = r & 63, cm = r >> 6;
    const int lhs = (kc >> 2) & 1, kk = 32 + (kc & 3) + 4 * (kc >> 3);
    const int blk = 2 * g + (cm >> 5), ln = (cm & 31) + 32 * lhs;
    W1[((blk * NK1 + (kk >> 2)) * 64 + ln) * 4 + (kk & 3)] = (g ? c.wcg[l] : c.wcf[l])[r];
  }
  for (int sI = tid; sI < 2 * 4096; sI += nthreads) {  // residual | skip as planes (fs3_stage_weights' layout)
    const int g = sI >> 12, r = sI & 4095;
    const int kc = r & 63, m2 = r >> 6;
    const int lhs = (kc >> 2) & 1, j = (kc & 3) + 4 * (kc >> 3);
    const int blk = 2 * g + (m2 >> 5), ln = (m2 & 31) + 32 * lhs, ks = j >> 3;
    unsigned short h, m, lo;
    bf3_split1((g ? p.ws[l] : p.wr[l])[r], h, m, lo);
    const int at = (((blk * 4 + ks) * 3) * 64 + ln) * 8 + (j & 7);
    W2[at] = h;
    W2[at + 512] = m;
    W2[at + 1024] = lo;
  }
}

// (fused_layer64s_ctxw2_kernel itself: the strip scaffold, csrc/fwd_layer64s_body.inc, under FS_FORM_CTXW2 -- its
// signature stands in fused_bf16.h with the other strip kernels')


// ----------------------------------------------------------------------------------------
// The head's two forward convolutions (dense_strip_kernel, fused_fwd.h) in the same form: weights as three bf16
// planes in LDS -- K x M x 6 bytes, 96 KB for conv1 (64 -> 256 rows, all of them in one workgroup) and for conv2
// in FOUR row blocks of 64 (256 inputs; the fp32 kernel held two blocks of 128: the input is read four times here
// instead of twice, which the matrix cores' time pays for) -- the strip's input in registers, split eight values
// at a time, six MFMAs per block and k-step.  `wimg`: the block's LDS image from ds3_pack_kernel, or NULL
// (converted here).
//   IN: 0 identity, 1 leaky-ReLU on load;  OUT: 0 y + bias, 1 leaky(y + bias), 2 y * leaky'(ref) (the head's data
// gradients, weights TRANSPOSED: their leaky-ReLU reference values are requested BEFORE the products -- the fp32
// strip form had no register left for that and lost to the generic kernel, 454 against 342 us)
// ----------------------------------------------------------------------------------------
template <int K, int M, bool TRANSPOSED>
__device__ __forceinline__ void ds3_stage(unsigned char *img, const float *wmat, int ldw, const float *bias, int m_base,
                                          int tid, int nthreads) {
  constexpr int NKS = K / 16;
  unsigned short *W = (unsigned short *)img;
  float *BI = (float *)(img + K * M * 6);
  for (int r = tid; r < K * M; r += nthreads) {  // source order: coalesced (W[m][k] = TRANSPOSED ? wmat[k][m] : wmat[m][k])
    const int m = TRANSPOSED ? r % M : r / K, k = TRANSPOSED ? r / M : r % K;
    // input register kk of a lane of half lh holds row 2 kk + lh; k-step ks takes registers 8 ks .. 8 ks + 7
    const int lhs = k & 1, kk = k >> 1, ks = kk >> 3, e = kk & 7;
    unsigned short h, mm, l;
    bf3_split1(TRANSPOSED ? wmat[(size_t)k * ldw + m_base + m] : wmat[(size_t)(m_base + m) * ldw + k], h, mm, l);
    const int at = ((((m >> 5) * NKS + ks) * 3) * 64 + (m & 31) + 32 * lhs) * 8 + e;
    W[at] = h;
    W[at + 512] = mm;
    W[at + 1024] = l;
  }
  for (int i = tid; i < M; i += nthreads) BI[i] = bias ? bias[m_base + i] : 0.f;
}
template <int K, int M, bool TRANSPOSED>
__global__ __launch_bounds__(256) void ds3_pack_kernel(const float *wmat, int ldw, const float *bias, float *dst) {
  constexpr int IMG_F = (K * M * 6 + M * 4) / 4;
  ds3_stage<K, M, TRANSPOSED>((unsigned char *)(dst + (size_t)blockIdx.y * IMG_F), wmat, ldw, bias, blockIdx.y * M,
                              blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

template <int K, int M, int IN, int OUT, bool TRANSPOSED>
__global__ __launch_bounds__(512, 1) void dense_strip_bf3_kernel(DenseStripArgs a, const float *wimg, int chunks_per_b,
                                                                 int chunk_t) {
  static_assert(K * M * 6 + M * 4 <= 160 * 1024 - 1024 && K % 16 == 0 && M % 32 == 0, "the planes fit a CU's LDS");
  constexpr int NB = M / 32, NKS = K / 16, IMG_BYTES = K * M * 6 + M * 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char ds3_lds[];
  float *BI = (float *)(ds3_lds + K * M * 6);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / chunks_per_b, ch = blockIdx.x - b * chunks_per_b;
  const int m_base = blockIdx.y * M;
  const int li = lane & 31, lh = lane >> 5;
  const int tb = (a.t_begin & ~TILE_ALIGN) + ch * chunk_t, te = min(a.t_end, tb + chunk_t);
  if (wimg) {
    LDS_IMAGE_COPY(ds3_lds, wimg + (size_t)blockIdx.y * (IMG_BYTES / 4), IMG_BYTES);
  } else {
    ds3_stage<K, M, TRANSPOSED>(ds3_lds, a.wmat, a.ldw, a.bias, m_base, tid, 512);
  }
  __syncthreads();
  const unsigned wa = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)ds3_lds + 16u * lane;
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
    float rv[OUT == 2 ? NB * 16 : 1];
    if (OUT == 2) {
      FS_FENCE(rld4);
#pragma unroll
      for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          rv[OUT == 2 ? blk * 16 + r : 0] =
              __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rb, orf, (32 * blk + (r & 3) + 8 * (r >> 2)) * rld4, 0));
    }
    float xr[K / 2];
    FS_FENCE(xld4);
#pragma unroll
    for (int kk = 0; kk < K / 2; ++kk) {
      float v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xb, ox, 2 * kk * xld4, 0));
      if (IN == 1) v = leaky(v);
      xr[kk] = live ? v : 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x16 acc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      u32x4 bh, bm, bl;
      bf3_split8(&xr[8 * ks], bh, bm, bl);
#pragma unroll
      for (int blk = 0; blk < NB; ++blk) {
        // (base + offset: every plane within a ds_read's 16-bit offset of one of two bases)
        const unsigned off = 3072u * (unsigned)(blk * NKS + ks);
        bf3_mfma6(acc[blk], wa + off, bh, bm, bl);
      }
    }
    FS_FENCE(yld4);
    if (out_live) {
#pragma unroll
      for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m0 = 32 * blk + (r & 3) + 8 * (r >> 2);
          float y = acc[blk][r];
          if (OUT == 2) y *= rv[OUT == 2 ? blk * 16 + r : 0] > 0.f ? 1.0f : kLeakySlope;
          else y += BI[m0 + 4 * lh];
          if (OUT == 1) y = leaky(y);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y), yb, oy, m0 * yld4, 0);
        }
    }
  }
}

// `m_total` output rows = m_total / M row blocks; `img`: m_total / M packed images (or NULL)
template <int K, int M, int IN, int OUT, bool TRANSPOSED = false>
static int launch_dense_strip_bf3(const DenseStripArgs &a, const float *img, int m_total, int batch, hipStream_t s) {
  const int nt = a.t_end - (a.t_begin & ~TILE_ALIGN);
  if (a.t_end <= a.t_begin || batch <= 0) return MVN_OK;
  int chunks, chunk_t;
  fb_chunks(nt, batch * (m_total / M), 1, &chunks, &chunk_t, 256);
  const void *fn = (const void *)dense_strip_bf3_kernel<K, M, IN, OUT, TRANSPOSED>;
  const int rc = ensure_max_dynamic_lds(fn, "hipFuncSetAttribute(dense_strip_bf3)");
  if (rc) return rc;
  hipLaunchKernelGGL((dense_strip_bf3_kernel<K, M, IN, OUT, TRANSPOSED>), dim3(chunks * batch, m_total / M), dim3(512),
                     K * M * 6 + M * 4, s, a, img, chunks, chunk_t);
  return MVN_OK;
}
template <int K, int M, bool TRANSPOSED = false>
static void launch_ds3_pack(const float *wmat, int ldw, const float *bias, int m_total, float *dst, hipStream_t s) {
  hipLaunchKernelGGL((ds3_pack_kernel<K, M, TRANSPOSED>), dim3(8, m_total / M), dim3(256), 0, s, wmat, ldw, bias, dst);
}
constexpr size_t DS3_IMG1_F = (64 * 256 * 6 + 256 * 4) / 4, DS3_IMG2_F = (256 * 64 * 6 + 64 * 4) / 4;
constexpr size_t DS3_IMG_F = DS3_IMG1_F + 4 * DS3_IMG2_F;      // forward: conv1 + conv2's four blocks
constexpr size_t DS3_BWD_IMG_F = 4 * DS3_IMG2_F + DS3_IMG2_F;  // backward: conv2^T's four blocks + conv1^T

// MOVENET_HIP_FORWARD_MFMA=f32 keeps the fp32-MFMA strip kernel and the head's fp32 kernels (tests); common.h: Switches
static bool forward_bf3_enabled() { return !switches().forward_f32; }

}  // namespace mvn
