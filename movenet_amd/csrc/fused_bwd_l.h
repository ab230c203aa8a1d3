// Backward of one gated residual layer as ONE kernel (C = K = 64), r4: the two halves of fused_bwd.h
// joined so that df | dg never crosses HBM (it was written once and read twice: 384 of the 896 floats a
// layer's backward moved per position).  The reference arithmetic is movenet/modules.py:67-93 differentiated:
//   dz  = Wr^T dxo + Ws^T dskip,   df = dz sg (1 - th^2),   dg = dz th sg (1 - sg)
//   dWr += dxo z^T, dWs += dskip z^T, dbr += sum_t dxo, dbs += sum_t dskip           (z = th sg)
//   dWf|dWg[o][c][tap 1] += dfg[o][t] x[c][t],   [tap 0] += dfg[o][t] x[c][t - d]
//   dx[u] = [u >= t_lo] (dxo[u] + W1^T dfg[u]) + [u + d < T] W0^T dfg[u + d]
// The last line is what kept the halves apart: dx[u] needs dfg at u AND at u + d, i.e. another tile.  Here the
// gradient w.r.t. a layer's input leaves in SCATTER form, as two tensors
//   A'[u] = dxo[u] + W1^T dfg[u]   (u in [t_lo, T)),     P0[t] = W0^T dfg[t]   (t in [t_lo, T)),
// both products of the SAME dfg tile, and the layer below stages its dxo as A'[t] (t >= up_lo) + P0[t + up_d]
// (t + up_d < T): the dilation shift moves from the producer's operand (two tiles of dfg) to the consumer's load
// (a second 64-row tensor).  Per position the backward of a layer reads A', P0, dskip, tanh, sigmoid, x(t), x(t - d)
// (448 floats) and writes A', P0 (128): 576 floats against 896.
//
// A 512-thread workgroup (one per CU) owns 64-column tiles; LDS: U (128 x 64: [dxo; dskip], later [x(t - d); x(t)]),
// G (tanh | sigmoid, overwritten in place by df | dg), O ([dxo -> A'; P0]: the output staging tile), all fp32 with
// pitch 68, and [Wr | Ws]^T as three bf16 planes (48 KB, the dz product's A operand): 150 KB.  Every product runs on
// the bf16 matrix cores in the bf16 x 3 form (bf3.h), each phase as an OPERAND PIPELINE -- the LDS reads of stage s + 1
// are issued ahead of the split and the six MFMAs of stage s:
//   phase 1 (12 slots per wave): wave (K half, t block, c block) forms its half of a 32 c x 32 t block of dz (K = 64
//            of the tile's 128 rows, read across rows; weights from LDS) and ONE block of the residual / skip weight
//            gradient (K = time); the tile's x rows are in flight meanwhile and land in U behind the barrier;
//   gate:    the two K halves of a block meet through the idle P0 staging rows, each wave handing over the half of its
//            partial sums the other one finishes: all eight waves turn tanh | sigmoid into df | dg in place;
//   phase 2 (20 slots): wave (tap, K half, channel block) forms both 32-step blocks of its tap's product with its 48 plane
//            registers of W_tap, every wave owns two blocks of the filter / gate weight gradient; the next tile's loads
//            are issued in parts between the slots; the K halves meet in O.
// Both phases are software-pipelined INSIDE the wave (r4c, bf3_slot in bf3.h): a slot issues the LDS reads of the next
// operand, then the six MFMAs of this one with, behind them, this operand's m and l planes and the next operand's h plane.
// Five barriers per tile (the two halves had three each).  Slabs and bias partial sums leave in wgrad2's format;
// reduce_layer64_kernel adds them up.
//
// Where its time goes (timing builds 71-74 and the stamps of build 76, config 2, same box, us per layer): 198-209 as built,
// 190 without any global access, 130 without MFMAs -- an ON-CHIP time.  By the stamps a tile costs 23.6 k cycles, 16.8 k of
// them in the two phases, where every stage is a split of eight values (44 vector instructions) feeding six MFMAs (54.9 M
// vector instructions per launch = 1900 per wave and tile, matrix pipe busy 36 %).  The two waves of a SIMD do NOT share it
// evenly: waves 0-3 (the older ones) finish phase 2 in 8.1 k cycles and wait 3.5 k at the barrier, waves 4-7 take 10.9 k
// (phase 1: 4.8 k / 6.1 k) -- the SIMD issues from the older wave whenever it can, and a straight-line stream of MFMAs and
// vector instructions always can.  Tried on that (r4c; scripts/probes/simd_pairing.hip, dot2_split.hip;
// same-box timing builds, none kept): waves 4-7 entering a phase 128 .. 320 cycles late (no change, not even the sleep's
// cost: the partner fills in); static or per-stage alternating s_setprio (+1 .. +3 %); idle cycles in front of every MFMA so
// that the partner's MFMAs fit in between (+7 .. +40 %: they do not); the residuals through v_dot2c_f32_bf16 (28
// instructions per split instead of 44, but the instruction runs at a quarter of the rate).  Kept: the split of operand s + 1
// and the low planes of operand s BEHIND the MFMAs of operand s (bf3_slot): waves 0-3 phase 2 8.1 k -> 6.6 k cycles, waves
// 4-7 10.9 k -> 10.5 k, the kernel 1 - 2 % (203.9 -> 202.1 us on one box, 213.9 -> 209.2 on another).  In the probe two
// waves running [44 vector instructions][6 MFMAs] loops share a SIMD at 222 cycles per stage (pipe bound 192) when every
// stage ends in a branch, 246 - 250 with four stages between branches, and this kernel's unrolled phases run at 262 - 272.
// Measured earlier, none kept: the split's residuals as packed
// subtractions (36 instructions instead of 44: 212.6 against 205.5 us -- a v_pk_add_f32 costs more than the two adds it
// replaces); two wave roles (waves 0-3 the data path over full K with 96 plane registers of tap weights and no K halves
// to meet, waves 4-7 both weight gradients as 2 x 2 blocks: 52 splits per SIMD and tile instead of 64, four barriers
// instead of five) -- 209 against 198 us: the prefetched tile no longer fits the register file and waits in scratch.
// Operands split ONCE into planes in LDS was built too (r4b, a whole second kernel, parity green on its first run): tiles as
// [row][64 t] bf16 x three planes written by the staging threads and by the gate, row operands fetched with one ds_read_b128
// per plane, operands read across the tile's rows with two ds_read_b64_tr_b16 per plane (the CDNA4 transposed read;
// scripts/probes/tr_read.hip pins its lane map: element j of lane (li, lh) = tile[r0 + 8 lh + j][c0 + li]), 700 vector
// instructions per wave and tile instead of 1900.  The planes are 1.5 x the bytes, so the dz weights leave LDS for
// registers, and 96 plane registers of resident weights do not fit beside the accumulators: the compiler keeps part of them
// in scratch and reloads them in front of the MFMAs that need them (225 us per layer); streamed from packed images per tile
// instead (dz weights: 204 us; tap weights too: 234 us -- the tile's own loads queue behind 144 KB of weight loads per tile
// and CU).  Same box, the form above: 187-195 us.  With 256 registers per wave at two waves per SIMD and 160 KB of LDS the
// two forms meet at the same place from opposite sides.  (Four waves of 512 registers per CU would NOT be the next step: a
// wave never overlaps its own vector instructions with its own MFMAs -- scripts/probes/simd_pairing.hip -- only the SIMD's
// other wave's work hides under an MFMA.)
#pragma once
#include "fused_bwd.h"
#include "fused_fwd.h"
#include "fused_fwd_bf3.h"

namespace mvn {

struct FusedBwdLArgs {
  int t_lo, t_end, d;      // outputs and dfg cover [t_lo = A_{l+1}, t_end = T); d = this layer's dilation
  int t_skip0, t_base;
  int up_lo, up_d;         // the layer above: its A' holds values from up_lo = t_lo + up_d, its P0 is read at t + up_d
  const float *wr, *ws;    // (64 out, 64 in) each
  const float *wf, *wg;    // (64 out, 64 in, 2 taps) each
  Act ga, gp;              // A', P0 of the layer above; ga.p == NULL: last layer (its residual output is unused)
  Act dskip, th, sg, xin;
  Act oa, op;              // A'[t], P0[t] of this layer, t in [t_lo, t_end)
  Act dfg;                 // conditioned layers: df | dg written for the context pass (bwd_dctx_wgctx64_kernel)
};

constexpr int FBL_TILE_F = 128 * W2_LD;                 // floats per LDS tile
constexpr int FBL_WIMG_BYTES = 2 * 8 * 3 * 1024;        // [c block][k-step][plane][lane][8 bf16]
constexpr int FBL_LDS_BYTES = 3 * FBL_TILE_F * 4 + FBL_WIMG_BYTES;  // 150 KB

__device__ __forceinline__ f4 f4_add(const f4 &x, const f4 &y) { return f4{x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w}; }

// The one-plane form (fused_bf16.h: operands rounded ONCE to bf16, one MFMA per block): [Wr | Ws]^T is a 16 KB image (48 KB
// as planes), the tap weights of a wave 16 registers (48): 118 KB of LDS in all.
constexpr int FBL16_WIMG_BYTES = 2 * 8 * 1024;  // [c block][k-step][lane][8 bf16]
constexpr int FBL16_LDS_BYTES = 3 * FBL_TILE_F * 4 + FBL16_WIMG_BYTES;
typedef float f32x2_b16 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_b16 __attribute__((ext_vector_type(2)));
// {bf16(a), bf16(b)} in one register, a in the low half (round to nearest even)
__device__ __forceinline__ unsigned b16_pack2(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_b16{a, b}, bf16x2_b16));
}
__device__ __forceinline__ u32x4 b16_pack8(const float *x) {
  return u32x4{b16_pack2(x[0], x[1]), b16_pack2(x[2], x[3]), b16_pack2(x[4], x[5]), b16_pack2(x[6], x[7])};
}
__device__ __forceinline__ unsigned short b16_one(float w) { return __builtin_bit_cast(unsigned short, (__bf16)w); }
#define B16_MFMA(acc_, a_, b_) \
  acc_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a_), __builtin_bit_cast(bf16x8, b_), acc_, 0, 0, 0)

// ----------------------------------------------------------------------------------------
// Both layer kernels are one SCAFFOLD (bwd_layer64_body.inc) -- LDS carve, wave roles, staging loads and stores, gate
// derivative, K-half exchanges, outputs, row sums, slabs -- under one of two OPERAND POLICIES, which say how a product's
// operands are formed and fed to the matrix cores: BF3 (bwd_layer64_kernel: bf16 x 3, exact, each phase an operand
// pipeline) or one plane (bwd_layer64_bf16_kernel in fused_bf16.h).  A policy supplies four sections, each marked
// [policy] in the body and written in place under `if constexpr (BF3)`:
//   the store of one element of the [Wr | Ws]^T image;  the tap-weight registers and their fill;
//   the 12 slots of phase 1;  the 20 slots of phase 2 (each with its operand fetchers).
// The body is TEXT, included behind each kernel's parameter list with FBL_BF3 set, not a function the kernels call:
// the fp32 kernels sit at 256 registers, and every form that let the compiler optimise a section apart from the
// scaffold before joining them (policy structs, a body template behind two wrapper kernels) cost them scratch.  As text
// all five instantiations compile to the instructions they compiled to as two kernels.
// The BF3 policy also pins its instruction order (scheduling fences around the slot loops) and carries the timing
// builds' hooks (MVN_EXP 71-74, 76); under the one-plane policy both are absent.
// GLOBAL (one plane only): the row sums of df | dg leave in g_part, one 128-float partial per workgroup.
// WRITE_DFG: the fp32 df | dg tile is also written to a.dfg, for the context pass / the fp32 label's row sums.
// ----------------------------------------------------------------------------------------
#define FBL_BF3 1
template <bool WRITE_DFG>
__global__ __launch_bounds__(512, 1) void bwd_layer64_kernel(FusedBwdLArgs a, int chunks_per_b, int chunk_t,
                                                            float *__restrict__ rs_bias_part, float *__restrict__ rs_part,
                                                            float *__restrict__ fg_part)
#include "bwd_layer64_body.inc"
#undef FBL_BF3

// The gradient w.r.t. the FIRST layer's input in dense form, for the embedding / causal-conv gradient:
// dx0[t] = [t >= t_lo] A'[t] + [t + d < T] P0[t + d],  t in [0, T).
__global__ __launch_bounds__(256) void bwd_scatter_combine_kernel(Act oa, Act op, Act dx, int C, int t_lo, int d, int T) {
  const int b = blockIdx.z, c = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T || c >= C) return;
  const float va = t >= t_lo ? *oa.at(b, c, t) : 0.f;
  const float vp = t + d < T ? *op.at(b, c, t + d) : 0.f;
  *dx.at(b, c, t) = va + vp;
}

// Launch geometry of the fused layer backward (one round of one workgroup per CU): false when the scratch cannot
// hold its slabs (the caller then keeps the two-half form for the whole pass).
struct FusedBwdLPlan {
  int chunks = 0, chunk_t = 0;
  float *bias = nullptr, *rs = nullptr, *fg = nullptr;
  size_t used = 0;  // floats of `slab` taken
};
// (With both pointers given and n_max >= 1 the answer is true whatever t_lo is: chunks is either <= n_max already or
// recut to ceil(tiles / ceil(tiles / n_max)) <= n_max, so n * per_wg <= slab_floats and n * 128 <= bias_floats.  A
// scratch that holds one layer therefore holds every layer.)
static bool bwd_layer64_plan(int cus, int t_lo, int t_end, int batch, float *bias_scratch, size_t bias_floats, float *slab,
                             size_t slab_floats, FusedBwdLPlan *pl) {
  const int nt = t_end - (t_lo & ~TILE_ALIGN);
  if (t_end <= t_lo || batch <= 0) return true;
  fb_chunks_on(cus, nt, batch, 1, &pl->chunks, &pl->chunk_t);
  if (!bias_scratch || !slab) return false;
  // short sequences (the parity tests' sizes): fewer, longer chunks so that the slabs fit the scratch
  const size_t per_wg = 128 * 64 + 128 * 128;
  const size_t n_max = std::min(slab_floats / per_wg, bias_floats / 128) / (size_t)batch;
  if (n_max < 1) return false;
  if ((size_t)pl->chunks > n_max) {
    const int tiles = (nt + W2_T - 1) / W2_T;
    const int chunk_tiles = (tiles + (int)n_max - 1) / (int)n_max;
    pl->chunks = (tiles + chunk_tiles - 1) / chunk_tiles;
    pl->chunk_t = chunk_tiles * W2_T;
  }
  const size_t n = (size_t)pl->chunks * batch;
  pl->used = n * per_wg;
  if (pl->used > slab_floats || n * 128 > bias_floats) return false;
  pl->bias = bias_scratch;
  pl->rs = slab;
  pl->fg = slab + n * 128 * 64;
  return true;
}
// (launch_bwd_layer64 stands in fused_bf16.h, which sees both policies' kernels)

}  // namespace mvn
