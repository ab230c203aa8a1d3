// bf16 mixed precision for the audio-only C = K = 64 layer stack (mvn_forward_bf16 / mvn_backward_bf16): every product
// of a gated layer takes its operands rounded ONCE to bf16 (round to nearest even: v_cvt_pk_bf16_f32, which keeps a NaN
// a NaN) and runs as ONE v_mfma_f32_32x32x16_bf16 per 32 x 32 x 16 block with fp32 accumulation, where the exact
// kernels (fused_fwd_bf3.h, fused_bwd_l.h) split each fp32 operand into three bf16 planes and issue six.  Rounded:
//   forward   x(t), x(t - d) and z = tanh sigmoid as products' inputs, the four weight tensors;
//   backward  dxo, dskip and the four weight tensors (dz and input-gradient products), df | dg, x and z (weight
//             gradients).
// Everything else stays fp32: biases, the gate arithmetic and its derivative, the residual add, the skip sum, the bias
// gradients, every tensor in HBM (saved activations, A' / P0, the weight-gradient slabs) and the reductions.  The two
// kernels below keep the dataflow, the buffers and the launch geometry of their exact twins; what they drop is the split
// (44 vector instructions per eight values there, four v_cvt_pk_bf16_f32 here) and two thirds of the weight images.
//
// GLOBAL (mvn_forward_bf16_global / mvn_backward_bf16_global; DESIGN 7.3, choice (a)): the class label's term, ONE fp32
// 2C-vector gb[l][b] per (layer, sequence) from global_bias_kernel, nothing in it rounded to bf16.
//   forward   the f | g accumulators START from gb (128 floats of LDS behind br | bs) instead of from zero: one LDS read
//             per accumulator register and no add in front of tanh / sigmoid (the accumulator-start form: 85.0 us per
//             layer launch at config 2 against 68.0 for <false>; the add-after-the-product form of
//             fused_layer64s_bf3_kernel<true> was not built here, so the two forms have NOT been measured against each
//             other);
//   backward  r[l][b] = sum_t (df | dg)(b, :, t) from the fp32 tile in LDS behind barrier B2, four registers per thread
//             as the bias gradients' bsum[], one 128-float partial per workgroup, summed in double and in chunk order by
//             global_rowsum_reduce_kernel (global_cond.h).  No dfg tensor is written or read.  120.2 us per layer
//             launch against 119.1 for <false>, plus 6.2 us for the reduce launch.
// GLOBAL = false is each kernel as it was: every added line sits under `if constexpr (GLOBAL)`.
#pragma once
#include "fused_bwd_l.h"
#include "global_cond.h"

namespace mvn {

// (b16_pack2 / b16_pack8 / b16_one / B16_MFMA, the conversions of both directions, stand in fused_bwd_l.h)

// ----------------------------------------------------------------------------------------
// Forward: fused_layer64s_bf3_kernel with one plane.  LDS image [block][k-step][lane][8 bf16] (1 KB per block and
// k-step): W1 4 x 8 KB, W2 4 x 4 KB, then br | bs as floats -- 48.5 KB against 144.5.
// ----------------------------------------------------------------------------------------
constexpr int FB16_W1_BYTES = 4 * 8 * 1024, FB16_W2_BYTES = 4 * 4 * 1024;
constexpr int FB16_LDS_BYTES = FB16_W1_BYTES + FB16_W2_BYTES + 128 * 4;
constexpr int FB16_PACK_F = FB16_LDS_BYTES / 4;
// CTX (conditioned layers): the f | g image holds 12 k-steps per block -- [Wcf; Wcg] behind the two taps -- and bcf | bcg
// follow br | bs as floats: 48 + 16 KB of weights, 65 KB in all.
constexpr int FB16C_W1_BYTES = 4 * 12 * 1024;
constexpr int FB16C_LDS_BYTES = FB16C_W1_BYTES + FB16_W2_BYTES + 256 * 4;
constexpr int FB16C_PACK_F = FB16C_LDS_BYTES / 4;

// fs3_stage_weights' element order, one bf16 per weight
template <int NKS1 = 8>
__device__ __forceinline__ void fb16_stage_weights(unsigned char *img, const float *wf, const float *wg, const float *wr,
                                                   const float *ws, const float *br, const float *bs, int tid, int nthreads) {
  unsigned short *W1 = (unsigned short *)img;
  unsigned short *W2 = (unsigned short *)(img + 4 * NKS1 * 1024);
  float *BI = (float *)(img + 4 * NKS1 * 1024 + FB16_W2_BYTES);
  for (int sI = tid; sI < 2 * 8192; sI += nthreads) {
    const int g = sI >> 13, r = sI & 8191;  // g: 0 filter, 1 gate; source (out, in, tap)
    const int tap = r & 1, kc = (r >> 1) & 63, cm = r >> 7;
    const int lhs = (kc >> 2) & 1, j = (kc & 3) + 4 * (kc >> 3);
    const int blk = 2 * g + (cm >> 5), ln = (cm & 31) + 32 * lhs, ks = (tap ? 0 : 4) + (j >> 3);
    W1[((blk * NKS1 + ks) * 64 + ln) * 8 + (j & 7)] = b16_one((g ? wg : wf)[r]);
  }
  for (int sI = tid; sI < 2 * 4096; sI += nthreads) {
    const int g = sI >> 12, r = sI & 4095;  // g: 0 residual, 1 skip; source (out, in)
    const int kc = r & 63, m2 = r >> 6;
    const int lhs = (kc >> 2) & 1, j = (kc & 3) + 4 * (kc >> 3);
    const int blk = 2 * g + (m2 >> 5), ln = (m2 & 31) + 32 * lhs, ks = j >> 3;
    W2[((blk * 4 + ks) * 64 + ln) * 8 + (j & 7)] = b16_one((g ? ws : wr)[r]);
  }
  for (int i = tid; i < 128; i += nthreads) BI[i] = i < 64 ? br[i] : bs[i - 64];
}
// the conditioned layer's image: the audio-only element order at 12 k-steps per block, [Wcf; Wcg] (out, in) as k-steps
// 8..11 in the residual | skip image's order, bcf | bcg behind br | bs
__device__ __forceinline__ void fb16c_stage_weights(unsigned char *img, const float *wf, const float *wg, const float *wr,
                                                    const float *ws, const float *br, const float *bs, const float *wcf,
                                                    const float *wcg, const float *bcf, const float *bcg, int tid, int nthreads) {
  fb16_stage_weights<12>(img, wf, wg, wr, ws, br, bs, tid, nthreads);
  unsigned short *W1 = (unsigned short *)img;
  float *BC = (float *)(img + FB16C_W1_BYTES + FB16_W2_BYTES) + 128;
  for (int sI = tid; sI < 2 * 4096; sI += nthreads) {
    const int g = sI >> 12, r = sI & 4095;  // g: 0 filter, 1 gate; source (out, in)
    const int kc = r & 63, m2 = r >> 6;
    const int lhs = (kc >> 2) & 1, j = (kc & 3) + 4 * (kc >> 3);
    const int blk = 2 * g + (m2 >> 5), ln = (m2 & 31) + 32 * lhs, ks = 8 + (j >> 3);
    W1[((blk * 12 + ks) * 64 + ln) * 8 + (j & 7)] = b16_one((g ? wcg : wcf)[r]);
  }
  for (int i = tid; i < 128; i += nthreads) BC[i] = i < 64 ? bcf[i] : bcg[i - 64];
}

__global__ __launch_bounds__(256) void fb16_pack_kernel(Fs3PackArgs p, float *dst) {
  const int l = blockIdx.y;
  fb16_stage_weights((unsigned char *)(dst + (size_t)l * FB16_PACK_F), p.wf[l], p.wg[l], p.wr[l], p.ws[l], p.br[l], p.bs[l],
                     blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}
__global__ __launch_bounds__(256) void fb16c_pack_kernel(Fs3PackArgs p, Fb16cPackArgs c, float *dst) {
  const int l = blockIdx.y;
  fb16c_stage_weights((unsigned char *)(dst + (size_t)l * FB16C_PACK_F), p.wf[l], p.wg[l], p.wr[l], p.ws[l], p.br[l], p.bs[l],
                      c.wcf[l], c.wcg[l], c.bcf[l], c.bcg[l], blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// acc[blk] += W[blk] (NKS k-steps of the image at LDS byte address wa, from k-step KS0 of the block's STRIDE) x B, B value
// e of k-step ks = bval(ks, e)
template <int NKS, int STRIDE = NKS, int KS0 = 0, class BV>
__device__ __forceinline__ void fb16_product(f32x16 (&acc)[4], unsigned wa, BV bval) {
  typedef __attribute__((address_space(3))) u32x4 lds_u4;
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    u32x4 bq;
#pragma unroll
    for (int i = 0; i < 4; ++i) bq[i] = b16_pack2(bval(ks, 2 * i), bval(ks, 2 * i + 1));
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      const u32x4 aq = *(const lds_u4 *)(uintptr_t)(wa + 1024u * (unsigned)(blk * STRIDE + KS0 + ks));
      B16_MFMA(acc[blk], aq, bq);
    }
  }
}

// ----------------------------------------------------------------------------------------
// The forward STRIP layer kernels: one scaffold (csrc/fwd_layer64s_body.inc), included behind each kernel's parameter
// list under the kernel's product policy FS_FORM.  They stand together here because this header sees every policy's
// helpers.  As with the backward (fused_bwd_l.h), the body is TEXT, not a function the kernels call.
// ----------------------------------------------------------------------------------------
// fp32 MFMAs (fused_fwd.h; MOVENET_HIP_FORWARD_MFMA=f32, or a context with no room for the ctxw2 images).  HAS_CTX: the
// context is a third K block of the first product, in the registers that otherwise fetch x(t) a strip ahead.
#define FS_FORM FS_FORM_F32
template <bool HAS_CTX>
__global__ __launch_bounds__(512, 1) void fused_layer64s_kernel(FusedFwdPArgs a, int chunks_per_b, int chunk_t)
#include "fwd_layer64s_body.inc"
#undef FS_FORM

// bf16 x 3 (fused_fwd_bf3.h).  GLOBAL (global conditioning): a label is constant in time, so its context
// term is ONE 2C-vector per (layer, sequence), gbias = [Wcf e_b + bcf | Wcg e_b + bcg] (global_cond.h:
// global_bias_kernel); the instantiation keeps it in 128 floats of LDS behind br | bs and adds it to the f | g
// pre-activations in front of tanh / sigmoid.
#define FS_FORM FS_FORM_BF3
template <bool GLOBAL>
__global__ __launch_bounds__(512, 1) void fused_layer64s_bf3_kernel(FusedFwdPArgs a, int chunks_per_b, int chunk_t)
#include "fwd_layer64s_body.inc"
#undef FS_FORM

// the conditioned layer with x(t - d) and the second product as planes (fused_fwd_bf3.h: fsc_pack_kernel's image)
#define FS_FORM FS_FORM_CTXW2
__global__ __launch_bounds__(512, 1) void fused_layer64s_ctxw2_kernel(FusedFwdPArgs a, int chunks_per_b, int chunk_t)
#include "fwd_layer64s_body.inc"
#undef FS_FORM

// one bf16 plane.  GLOBAL: the f | g accumulators start from the label's vector (the head of this file).  CTX
// (mvn_forward_bf16_ctx; never together with GLOBAL): the conditioned layer -- K = 192, the context as k-steps 8..11 of
// a 12-k-step image, the accumulators started from bcf | bcg (one vector for all sequences).
#define FS_FORM FS_FORM_BF16
template <bool GLOBAL, bool CTX = false>
__global__ __launch_bounds__(512, 1) void fused_layer64s_bf16_kernel(FusedFwdPArgs a, int chunks_per_b, int chunk_t)
#include "fwd_layer64s_body.inc"
#undef FS_FORM


// ----------------------------------------------------------------------------------------
// The forward's layer forms, one row each: what a launch needs besides the layer's arguments.  (The table stands here
// because this header sees every forward kernel: fused_fwd.h, fused_fwd_bf3.h and the ones above.)  sequence.hip picks
// one row per call, in front of the first launch (plan_forward), and every layer of the call goes through
// launch_layer_form with it; launch_layer_pack writes the row's L weight images where the z scratch holds them.
// ----------------------------------------------------------------------------------------
struct LayerForm {
  const char *attr_what;                                  // error text of the kernel's dynamic-LDS attribute
  void (*kernel)(FusedFwdPArgs, int, int);                // nullptr: the generic two-kernel form (sequence.hip: run_fg / RsOp)
  int block, lds_bytes;                                   // threads per workgroup, dynamic LDS
  int per_cu, granule;                                    // fb_chunks: workgroups per CU, columns a chunk is a multiple of
  int pack_f;                                             // floats from one layer's LDS image to the next; 0: no image
  const char *pack_what;                                  // error text of the pack launch
  void (*pack)(Fs3PackArgs, float *);                     // the image's pack kernel: this one, or the one that
  void (*pack_ctx)(Fs3PackArgs, Fb16cPackArgs, float *);  // takes the context convs as well
};
enum LayerFormId {
  FORM_GENERIC, FORM_F32_TILE, FORM_F32_STRIP, FORM_F32_STRIP_CTX, FORM_BF3_STRIP, FORM_BF3_STRIP_BIAS, FORM_CTXW2_STRIP,
  FORM_BF16_STRIP, FORM_BF16_STRIP_BIAS, FORM_BF16_STRIP_CTX, N_LAYER_FORMS
};
constexpr int F32_TILE_LDS_BYTES = (2 * 128 + 3 * 64) * (32 + 4) * (int)sizeof(float);
constexpr int F32_STRIP_LDS_BYTES = (16384 + 8192 + 256) * (int)sizeof(float), F32_STRIP_CTX_LDS_BYTES = F32_STRIP_LDS_BYTES + 8192 * 4;
constexpr int GBIAS_LDS_BYTES = 128 * 4;  // the bias forms: the sequence's f | g vector behind the image
// strip kernels: 512 threads, one workgroup per CU, chunks of whole rounds of the 8 waves' 32-column strips; the tile
// kernel: 256 threads, two workgroups per CU, 32-column tiles
static const LayerForm LAYER_FORMS[N_LAYER_FORMS] = {
    /* GENERIC            */ {nullptr, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr},
    /* F32_TILE           */ {"hipFuncSetAttribute(fused_layer64p)", fused_layer64p_kernel, 256, F32_TILE_LDS_BYTES, 2, 32, 0, nullptr, nullptr, nullptr},
    /* F32_STRIP          */ {"hipFuncSetAttribute(fused_layer64s)", fused_layer64s_kernel<false>, 512, F32_STRIP_LDS_BYTES, 1, 256, 0, nullptr, nullptr, nullptr},
    /* F32_STRIP_CTX      */ {"hipFuncSetAttribute(fused_layer64s)", fused_layer64s_kernel<true>, 512, F32_STRIP_CTX_LDS_BYTES, 1, 256, 0, nullptr, nullptr, nullptr},
    /* BF3_STRIP          */ {"hipFuncSetAttribute(fused_layer64s_bf3)", fused_layer64s_bf3_kernel<false>, 512, FS3_LDS_BYTES, 1, 256, FS3_PACK_F, "fs3_pack", fs3_pack_kernel, nullptr},
    /* BF3_STRIP_BIAS     */ {"hipFuncSetAttribute(fused_layer64s_bf3<global>)", fused_layer64s_bf3_kernel<true>, 512, FS3_LDS_BYTES + GBIAS_LDS_BYTES, 1, 256, FS3_PACK_F, "fs3_pack", fs3_pack_kernel, nullptr},
    /* CTXW2_STRIP        */ {"hipFuncSetAttribute(fused_layer64s_ctxw2)", fused_layer64s_ctxw2_kernel, 512, FSC_LDS_BYTES, 1, 256, FSC_PACK_F, "fsc_pack", nullptr, fsc_pack_kernel},
    /* BF16_STRIP         */ {"hipFuncSetAttribute(fused_layer64s_bf16)", fused_layer64s_bf16_kernel<false>, 512, FB16_LDS_BYTES, 1, 256, FB16_PACK_F, "fb16_pack", fb16_pack_kernel, nullptr},
    /* BF16_STRIP_BIAS    */ {"hipFuncSetAttribute(fused_layer64s_bf16<global>)", fused_layer64s_bf16_kernel<true>, 512, FB16_LDS_BYTES + GBIAS_LDS_BYTES, 1, 256, FB16_PACK_F, "fb16_pack", fb16_pack_kernel, nullptr},
    /* BF16_STRIP_CTX     */ {"hipFuncSetAttribute(fused_layer64s_bf16_ctx)", fused_layer64s_bf16_kernel<false, true>, 512, FB16C_LDS_BYTES, 1, 256, FB16C_PACK_F, "fb16c_pack", nullptr, fb16c_pack_kernel},
};
// The z scratch of a call: the chosen form's L images from its start, FWD_IMG_STRIDE_F floats reserved per layer whatever
// the form, then the head's images (sequence.hip; the backward's head images follow those).  The head's offset is
// computed from this one stride, not from the chosen row, so it is the same address in every mode: no form's image
// may be larger.
constexpr int FWD_IMG_STRIDE_F = FS3_PACK_F > FSC_PACK_F ? FS3_PACK_F : FSC_PACK_F;
static_assert(FS3_PACK_F <= FWD_IMG_STRIDE_F && FSC_PACK_F <= FWD_IMG_STRIDE_F && FB16_PACK_F <= FWD_IMG_STRIDE_F &&
                  FB16C_PACK_F <= FWD_IMG_STRIDE_F,
              "a layer image larger than the stride the head's image offset is computed from would overlap the head's");
static_assert(FS3_PACK_LAYERS == GC_LAYERS, "fill_ctx_tables fills the pack kernels' and global_cond.h's tables alike");

// The context-conv pointer tables of layers l0 .. l0 + n - 1 (the unused tail repeats the last layer): A is Fb16cPackArgs
// or GlobalCondArgs
template <class A>
static void fill_ctx_tables(const mvn_params *p, int l0, int n, A *a) {
  for (int i = 0; i < FS3_PACK_LAYERS; ++i) {
    const int l = l0 + std::min(i, n - 1);
    a->wcf[i] = p->ctx_filter_w[l]; a->wcg[i] = p->ctx_gate_w[l];
    a->bcf[i] = p->ctx_filter_b[l]; a->bcg[i] = p->ctx_gate_b[l];
  }
}
// the LDS images of layers 0 .. L-1 into `dst` (L x f.pack_f floats), one launch per 32 layers
static int launch_layer_pack(const LayerForm &f, const mvn_params *p, int L, float *dst, hipStream_t s) {
  for (int l0 = 0; l0 < L; l0 += FS3_PACK_LAYERS) {
    const int n = std::min(FS3_PACK_LAYERS, L - l0);
    Fs3PackArgs pa;
    for (int i = 0; i < FS3_PACK_LAYERS; ++i) {
      const int l = l0 + std::min(i, n - 1);
      pa.wf[i] = p->filter_w[l]; pa.wg[i] = p->gate_w[l]; pa.wr[i] = p->residual_w[l]; pa.ws[i] = p->skip_w[l];
      pa.br[i] = p->residual_b[l]; pa.bs[i] = p->skip_b[l];
    }
    float *const img = dst + (size_t)l0 * f.pack_f;
    if (f.pack_ctx) {
      Fb16cPackArgs pc;
      fill_ctx_tables(p, l0, n, &pc);
      hipLaunchKernelGGL(f.pack_ctx, dim3(8, n), dim3(256), 0, s, pa, pc, img);
    } else {
      hipLaunchKernelGGL(f.pack, dim3(8, n), dim3(256), 0, s, pa, img);
    }
  }
  return check_hip(hipGetLastError(), f.pack_what);
}
// one layer in form `f` (not the generic one); the caller has raised the kernel's dynamic-LDS limit (f.attr_what)
static void launch_layer_form(const LayerForm &f, const FusedFwdPArgs &a, int batch, hipStream_t s) {
  const int nt = a.t_end - (a.t_begin & ~TILE_ALIGN);
  if (a.t_end <= a.t_begin || batch <= 0) return;
  int chunks, chunk_t;
  fb_chunks(nt, batch, f.per_cu, &chunks, &chunk_t, f.granule);
  hipLaunchKernelGGL(f.kernel, dim3(chunks * batch), dim3(f.block), f.lds_bytes, s, a, chunks, chunk_t);
}

// ----------------------------------------------------------------------------------------
// Backward: the scaffold of bwd_layer64_kernel (bwd_layer64_body.inc, described in fused_bwd_l.h) under the one-plane
// operand policy -- same roles, tiles, barriers, scatter outputs (A', P0) and slab / bias-partial formats
// (reduce_layer64_kernel and bwd_scatter_combine_kernel are shared).
// ----------------------------------------------------------------------------------------
// GLOBAL (mvn_backward_bf16_global): the row sums of df | dg leave in g_part.  WRITE_DFG (mvn_backward_bf16_ctx; never
// together with GLOBAL): the fp32 df | dg tile also written to a.dfg for the context pass, as bwd_layer64_kernel<true> does.
#define FBL_BF3 0
template <bool GLOBAL, bool WRITE_DFG = false>
__global__ __launch_bounds__(512, 1) void bwd_layer64_bf16_kernel(FusedBwdLArgs a, int chunks_per_b, int chunk_t,
                                                                 float *__restrict__ rs_bias_part, float *__restrict__ rs_part,
                                                                 float *__restrict__ fg_part, float *__restrict__ g_part)
#include "bwd_layer64_body.inc"
#undef FBL_BF3

// The layer backward's kernels, [bf16][plain | dfg output | label row sums]: what a launch needs besides its arguments
// (the fp32 label's row sums come from the dfg output and a kernel of their own: global_cond.h)
struct BwdLayerForm {
  const void *kernel[3];
  size_t lds_bytes;
  const char *name, *attr_what;
};
static const BwdLayerForm BWD_LAYER_FORMS[2] = {
    {{(const void *)bwd_layer64_kernel<false>, (const void *)bwd_layer64_kernel<true>, nullptr}, FBL_LDS_BYTES, "bwd_layer64",
     "hipFuncSetAttribute(bwd_layer64)"},
    {{(const void *)bwd_layer64_bf16_kernel<false>, (const void *)bwd_layer64_bf16_kernel<false, true>,
      (const void *)bwd_layer64_bf16_kernel<true>}, FBL16_LDS_BYTES, "bwd_layer64_bf16", "hipFuncSetAttribute(bwd_layer64_bf16)"},
};

// One layer's backward (a.dfg given: the form that writes df | dg) and the reduction of its slabs.  g_part / rowsum (both
// or neither; bf16 only): the GLOBAL instantiation leaves a 128-float partial of the df | dg row sums per workgroup in
// g_part (as many as the plan's bias partials), and rowsum (batch, 128) of this layer receives their sums.
template <class RsOp, class FgOp>
static int launch_bwd_layer64(bool bf16, const FusedBwdLArgs &a, const RsOp &rs, const FgOp &fg, int batch,
                              const FusedBwdLPlan &pl, hipStream_t s, float *g_part = nullptr, float *rowsum = nullptr) {
  if (pl.chunks <= 0) return MVN_OK;
  const BwdLayerForm &f = BWD_LAYER_FORMS[bf16];
  auto refuse = [&](const char *why) {
    set_error("%s: %s", f.name, why);
    return MVN_ERR_BAD_ARG;
  };
  const int ldt = a.th.ld;
  const bool wd = a.dfg.p != nullptr, glob = g_part != nullptr;
  if ((wd && a.dfg.ld != ldt) || a.sg.ld != ldt || a.xin.ld != ldt || a.oa.ld != ldt || a.op.ld != ldt || a.gp.ld != ldt ||
      (a.ga.p && a.ga.ld != ldt))
    return refuse("the (B, ch, Tp) views must share one row pitch");
  if (glob && wd) return refuse("the label's row sums and a dfg output do not go together");
  if (glob != (rowsum != nullptr)) return refuse("g_part and rowsum go together");
  const void *fn = f.kernel[wd ? 1 : glob ? 2 : 0];
  // (not reached from backward_impl: plan_backward hands out a g_part under bf16 only; it keeps a null kernel unlaunched)
  if (!fn) return refuse("no form with the label's row sums");
  const int n = pl.chunks * batch;
  const int rc = ensure_max_dynamic_lds(fn, f.attr_what);
  if (rc) return rc;
  void *args[] = {(void *)&a, (void *)&pl.chunks, (void *)&pl.chunk_t, (void *)&pl.bias, (void *)&pl.rs, (void *)&pl.fg,
                  (void *)&g_part};  // (the fp32 kernels take the first six)
  if (check_hip(hipLaunchKernel(fn, dim3(n), dim3(512), args, f.lds_bytes, s), f.name)) return MVN_ERR_LAUNCH;
  hipLaunchKernelGGL((reduce_layer64_kernel<RsOp, FgOp>), dim3(260 + 128 * 128 / 32), dim3(32 * RED_SEG), 0, s, rs, pl.rs,
                     pl.bias, n, fg, pl.fg, n);
  if (glob) {  // (a failed launch would leave the caller's zero-filled rowsum: silently zero context gradients)
    hipLaunchKernelGGL(global_rowsum_reduce_kernel, dim3(batch), dim3(128), 0, s, g_part, pl.chunks, rowsum);
    return check_hip(hipGetLastError(), "bwd_layer64_bf16<global>: reduce launches");
  }
  return MVN_OK;
}

}  // namespace mvn
