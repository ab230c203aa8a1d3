// FOLD variant of the pipelined generator (C = K = 64, Q = 256): the dependent chain of a
// layer is ONE mat-vec + gate + LDS exchange instead of two.
//
// In the PIPE kernel (generate_pipe.hip) a layer costs two dependent phases: z = gate(Wc x + ..)
// and then x' = x + Wr z + br, each with its own LDS exchange and barrier (1244 cycles per layer,
// DESIGN.md 4.1).  Here the residual 1x1 of layer j is folded into the current-tap filter/gate
// matrix of layer j+1 (reference arithmetic: movenet/modules.py:67-93 -- f,g = conv(x), x' = x +
// conv_residual(z) -- restated for the product of the two linear maps):
//
//     fg_{j+1} = Wc_{j+1} x_{j+1} + past-tap part
//              = (Wc_{j+1} Wr_j) z_j + [ Wc_{j+1} x_j + Wc_{j+1} br_j + past-tap part ]
//                `-- critical: one mat-vec on z_j --'  `-- known one phase earlier: helper waves --'
//
// A stage holds THREE layers (10 layer stages + the head = 11 workgroups per sequence).  Its
// inbox carries 3C granules {xp, zl, sk}: xp = the stream WITHOUT the previous stage's last
// residual term, zl = that stage's last gated activation -- the two the chain waits for -- and
// sk = the running skip sum, which travels on a lane of its own (sent and awaited off the chain,
// after the stage's third phase).  The two ends differ: stage 0 has no previous layer, so the head
// sends it xp alone and its zl / sk terms are not formed; the last layer stage feeds the head, which
// reads zl and sk but no xp', so its helpers send sk' first and no xp'.
// Waves 0-3 (the chain) compute
//     z_0 = gate(Wc_0 xp + (Wc_0 Wr_prev) zl + pf_0)
//     z_1 = gate((Wc_1 Wr_0) z_0 + base_1 + pf_1)
//     z_2 = gate((Wc_2 Wr_1) z_1 + (Wc_2 Wr_0) z_0 + base_2 + pf_2)   -> sent on as the next stage's zl
//           (the z_0 term from registers, while the LDS reads of z_1 are in flight)
// with their five matrices in registers; waves 4-7 (the helpers) compute one phase ahead
//     base_1 = Wc_1 xp + (Wc_1 Wr_prev) zl,    x_0 = xp + Wr_prev zl
//     base_2 = Wc_2 x_0  [+ the chain's term]
//     (third phase)                             x_1 = x_0 + Wr_0 z_0 + br_0
//                                               x_2 = x_1 + Wr_1 z_1 + br_1   -> xp' = x_2 + br_2 sent early
// and, after the third phase, sk' = sk + Ws_prev zl + Ws_0 z_0 + Ws_1 z_1 + biases (the skip 1x1
// of a stage's LAST layer is added by the next stage, the head for the last one).  The constant
// vectors Wc_1 br_0 and Wc_2 (br_0 + br_1) are packed once and ride in pf_1 / pf_2.  The
// explicit x_0, x_1, x_2 feed the dilation queues off the critical path, exactly as in PIPE.
// The hop: EVERY wave of a stage polls the stage's xp | zl granules itself (the head's waves: zl) and keeps them in a
// strip of LDS of its own, which it reads back behind its own write -- the LDS serves a wave's accesses in order, so
// between "granules visible" and a lane's first ds_read there is neither a wait for the write nor a barrier (one wave
// polling for all needed both, eleven times per sample).  The waves meet at the phase-0 barrier (the head: conv1's).
//
// The products Wc Wr are formed once at pack time (fp64 sums, rounded to fp32).  The folded
// form is the same real-number function as the reference's; its fp32 rounding differs from
// the layer-by-layer order at the 1e-7 level (logits within 2e-5 of the range, greedy
// fixtures bit-exact: tests/test_generate_gpu.py).
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "gen_common.h"
#include "pipe_common.h"

namespace mvn {

namespace fold {
constexpr int C = 64, Q = 256, NT = 512, LPS = 3;
constexpr int KQ = 4, KPER = 16, NF4 = 4;  // thread 4c + kq owns rows (c, C + c) x 16 inputs
constexpr int MAT_F = 2 * C * C;           // one 2C x C matrix (or two C x C ones) in the per-thread order
// a stage section: 14 matrices, then the vectors
enum { M_A0 = 0, M_A0P, M_A1, M_A2, M_B2P,       // chain waves: registers
       M_B1, M_B1P, M_B2, M_RR, M_RS,            // helper waves: registers; RR = {Wr_prev; Wr_0}, RS = {Wr_1; Ws_1}
       M_WP0, M_WP1, M_WP2, M_SS,                // LDS: past taps of the three layers, SS = {Ws_prev; Ws_0}
       N_MAT };
constexpr int N_LDS_MAT = 4;
// vectors: cb1[2C] = Wc_1 br_0, cb2[2C] = Wc_2 (br_0 + br_1), then bs_prev, br_0, bs_0, br_1, bs_1, br_2 [C each]
constexpr int V_CB1 = 0, V_CB2 = 2 * C, V_BSP = 4 * C, V_BR0 = 5 * C, V_BS0 = 6 * C, V_BR1 = 7 * C,
              V_BS1 = 8 * C, V_BR2 = 9 * C, VEC_F = 10 * C;
constexpr int STAGE_F = N_MAT * MAT_F + VEC_F;
constexpr int CTX_LAYER_F = MAT_F + 2 * C;  // as in the PIPE variant
constexpr int EMB_F = 2 * Q * C;
constexpr int W1_F = Q * C, W2_F = Q * Q, WSL_F = C * C;
constexpr int HEAD_F = W1_F + Q + W2_F + Q + WSL_F + C;
constexpr int GRAN = 3 * C;                 // granules per inbox: xp | zl | sk
// LDS floats: layer stage matrices + vectors; head stage the embedding tables (32768) + vectors
constexpr int LDS_FLOATS = N_LDS_MAT * MAT_F + 1536 + 16;
// r3, several sequences per pipeline ("rounds"): a stage is busy ~1.1 us of a 15 us step, so a
// pipeline serves up to GMAX sequences in turn -- weights shared, one inbox per sequence and
// stage, the LDS step vectors shared (they live within one turn).  What must survive from a
// sequence's turn to its next is the past-tap part of its f/g sums (pf, pg: six floats per
// channel), kept in LDS behind the vectors; the head keeps two class indices per sequence.
constexpr int GMAX = 8;
constexpr int PFS_F = 8;                    // floats per channel and sequence: pf0 pg0 pf1 pg1 | pf2 pg2 - -
constexpr int PFS_ALL_F = GMAX * C * PFS_F;
// the head stage keeps, behind its 16 index words there, conv2's partial sums by k-slice: [8 waves][Q]
constexpr int HEAD_PART_OFF = 16, HEAD_PART_F = 8 * Q;
static_assert(PFS_ALL_F >= HEAD_PART_OFF + HEAD_PART_F, "MULTI: the head's partial sums fit behind the index words");
// behind both: the waves' inbox strips, [8 waves][xp | zl] -- every wave of a stage polls the stage's granules itself and
// reads its inputs back from its own strip (the LDS serves a wave's accesses in order: no wait, no barrier in between)
constexpr int WIN_F = 2 * C, WIN_ALL_F = (NT / 64) * WIN_F;
constexpr int WIN_OFF_ONE = LDS_FLOATS + HEAD_PART_OFF + HEAD_PART_F;  // MULTI = false (the layer stages use LDS_FLOATS and the strips)
constexpr int WIN_OFF_MULTI = LDS_FLOATS + PFS_ALL_F;
constexpr int LDS_FLOATS_ONE = WIN_OFF_ONE + WIN_ALL_F, LDS_FLOATS_MULTI = WIN_OFF_MULTI + WIN_ALL_F;
static_assert(LDS_FLOATS_ONE * sizeof(float) <= 160 * 1024, "one sequence per pipeline: a CU's LDS");
static_assert(LDS_FLOATS_MULTI * sizeof(float) <= 160 * 1024, "several sequences per pipeline: a CU's LDS");
}  // namespace fold

// A thread's share of a matrix: 32 floats = 8 float4 of the packed order.  Two formats:
//  * PAIR (the 2C x C matrices): w[k] = {row c, row C + c} at input k of the thread's 16: one
//    packed FMA against {x_k, x_k} (an op_sel broadcast) advances BOTH rows, the four
//    accumulators end as {f, g} -- 16 FMAs + 3 packed adds for the two rows, where separate
//    rows cost 16 + 6 + 2 (the kernel is bound by VALU issue: scripts/probes/issue_rates.hip)
//  * SPLIT (two unrelated C x C matrices): a() = w[0..8) is row c of the first against
//    inputs {2i, 2i + 1}, b() = w[8..16) the same row of the second
struct FoldMat {
  v2f w[16];
};
__device__ __forceinline__ void fold_load(FoldMat &m, const float *sec, int t) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f4 v = ((const f4 *)sec)[i * 256 + t];
    m.w[2 * i] = v2f{v.x, v.y};
    m.w[2 * i + 1] = v2f{v.z, v.w};
  }
}
// acc (+)= w * {x.y, x.y}: the compiler finds the op_sel form for the high element of a
// register pair only every other time (it copies .w to a fresh register first), so it is spelled out
__device__ __forceinline__ v2f pk_fma_hi(v2f w, v2f xpair, v2f acc) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0]" : "+v"(acc) : "v"(w), "v"(xpair));
  return acc;
}
__device__ __forceinline__ v2f pk_mul_hi(v2f w, v2f xpair) {
  v2f r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1]" : "=v"(r) : "v"(w), "v"(xpair));
  return r;
}
// PAIR format: acc[j] (+)= w[4i + j] * {x[i][j], x[i][j]}
template <bool INIT>
__device__ __forceinline__ void pair_acc(v2f (&acc)[4], const v2f (&w)[16], const f4 (&x)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (INIT && i == 0) {
      acc[0] = w[0] * v2f{x[0].x, x[0].x};
      acc[1] = w[1] * v2f{x[0].y, x[0].y};
      acc[2] = w[2] * v2f{x[0].z, x[0].z};
      acc[3] = pk_mul_hi(w[3], v2f{x[0].z, x[0].w});
    } else {
      acc[0] = __builtin_elementwise_fma(w[4 * i], v2f{x[i].x, x[i].x}, acc[0]);
      acc[1] = __builtin_elementwise_fma(w[4 * i + 1], v2f{x[i].y, x[i].y}, acc[1]);
      acc[2] = __builtin_elementwise_fma(w[4 * i + 2], v2f{x[i].z, x[i].z}, acc[2]);
      acc[3] = pk_fma_hi(w[4 * i + 3], v2f{x[i].z, x[i].w}, acc[3]);
    }
  }
}
__device__ __forceinline__ v2f pair_sum(const v2f (&acc)[4]) { return (acc[0] + acc[2]) + (acc[1] + acc[3]); }
// acc (+)= w * {x.x, x.x}: pk_fma_hi's twin for the low element of a register pair
__device__ __forceinline__ v2f pk_fma_lo(v2f w, v2f xpair, v2f acc) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(w), "v"(xpair));
  return acc;
}
__device__ __forceinline__ v2f pk_mul_lo(v2f w, v2f xpair) {
  v2f r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(w), "v"(xpair));
  return r;
}
// pair_acc<true> with EVERY broadcast spelled as an op_sel form, against inputs held as four 128-bit registers: the
// same 16 products into the same four accumulators in the same order.  For a block whose other instructions do not
// lead the compiler to fold the broadcasts (it copies each input to a fresh register pair there: 16 moves more).
typedef float vf4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void pair_acc_sel(v2f (&acc)[4], const v2f (&w)[16], const vf4 (&x)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const v2f lo = v2f{x[i].x, x[i].y}, hi = v2f{x[i].z, x[i].w};
    if (i == 0) {
      acc[0] = pk_mul_lo(w[0], lo);
      acc[1] = pk_mul_hi(w[1], lo);
      acc[2] = pk_mul_lo(w[2], hi);
      acc[3] = pk_mul_hi(w[3], hi);
    } else {
      acc[0] = pk_fma_lo(w[4 * i], lo, acc[0]);
      acc[1] = pk_fma_hi(w[4 * i + 1], lo, acc[1]);
      acc[2] = pk_fma_lo(w[4 * i + 2], hi, acc[2]);
      acc[3] = pk_fma_hi(w[4 * i + 3], hi, acc[3]);
    }
  }
}
// SPLIT format, half H: one row against the 16 inputs
template <int H>
__device__ __forceinline__ float split_dot(const v2f (&w)[16], const f4 (&x)[4]) {
  v2f a0 = w[8 * H] * v2f{x[0].x, x[0].y}, a1 = w[8 * H + 1] * v2f{x[0].z, x[0].w};
  v2f a2 = w[8 * H + 2] * v2f{x[1].x, x[1].y}, a3 = w[8 * H + 3] * v2f{x[1].z, x[1].w};
  a0 = __builtin_elementwise_fma(w[8 * H + 4], v2f{x[2].x, x[2].y}, a0);
  a1 = __builtin_elementwise_fma(w[8 * H + 5], v2f{x[2].z, x[2].w}, a1);
  a2 = __builtin_elementwise_fma(w[8 * H + 6], v2f{x[3].x, x[3].y}, a2);
  a3 = __builtin_elementwise_fma(w[8 * H + 7], v2f{x[3].z, x[3].w}, a3);
  const v2f t = (a0 + a2) + (a1 + a3);
  return t.x + t.y;
}

// LDS accesses by byte address: base register + immediate (an address formed from the dynamic
// LDS symbol is a register per address; 20 of them spilled the chain's weights)
typedef __attribute__((address_space(3))) float lds_f;
typedef __attribute__((address_space(3))) vf4 lds_f4;
__device__ __forceinline__ f4 as_f4(vf4 v) {
  f4 r;
  r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w;
  return r;
}
__device__ __forceinline__ f4 lds_load4(unsigned addr) { return as_f4(*(const lds_f4 *)(uintptr_t)addr); }
__device__ __forceinline__ unsigned lds_addr(const float *p) { return (unsigned)(uintptr_t)(lds_f *)p; }
#define LDSF(addr, off) (*(lds_f *)(uintptr_t)((addr) + 4u * (unsigned)(off)))
template <int N4>
__device__ __forceinline__ void ldsv(f4 (&x)[N4], unsigned addr, int off) {
#pragma unroll
  for (int i = 0; i < N4; ++i) x[i] = lds_load4(addr + 4u * (unsigned)off + 16u * i);
}

// PAIR-format matrix streamed from LDS (eight float4 at waddr + 4096 i) against 16 inputs at xaddr
__device__ __forceinline__ v2f pair_dot_lds(unsigned waddr, unsigned xaddr) {
  v2f acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f4 wa = lds_load4(waddr + 4096u * (2 * i)), wb = lds_load4(waddr + 4096u * (2 * i + 1));
    const f4 x = lds_load4(xaddr + 16u * i);
    if (i == 0) {
      acc[0] = v2f{wa.x, wa.y} * v2f{x.x, x.x};
      acc[1] = v2f{wa.z, wa.w} * v2f{x.y, x.y};
      acc[2] = v2f{wb.x, wb.y} * v2f{x.z, x.z};
      acc[3] = pk_mul_hi(v2f{wb.z, wb.w}, v2f{x.z, x.w});
    } else {
      acc[0] = __builtin_elementwise_fma(v2f{wa.x, wa.y}, v2f{x.x, x.x}, acc[0]);
      acc[1] = __builtin_elementwise_fma(v2f{wa.z, wa.w}, v2f{x.y, x.y}, acc[1]);
      acc[2] = __builtin_elementwise_fma(v2f{wb.x, wb.y}, v2f{x.z, x.z}, acc[2]);
      acc[3] = pk_fma_hi(v2f{wb.z, wb.w}, v2f{x.z, x.w}, acc[3]);
    }
  }
  return pair_sum(acc);
}
// SPLIT-format half H of a matrix streamed from LDS
template <int H>
__device__ __forceinline__ float split_dot_lds(unsigned waddr, unsigned xaddr) {
  f4 w[4], x[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w[i] = lds_load4(waddr + 4096u * (4 * H + i));
    x[i] = lds_load4(xaddr + 16u * i);
  }
  v2f a0 = v2f{w[0].x, w[0].y} * v2f{x[0].x, x[0].y}, a1 = v2f{w[0].z, w[0].w} * v2f{x[0].z, x[0].w};
  v2f a2 = v2f{w[1].x, w[1].y} * v2f{x[1].x, x[1].y}, a3 = v2f{w[1].z, w[1].w} * v2f{x[1].z, x[1].w};
  a0 = __builtin_elementwise_fma(v2f{w[2].x, w[2].y}, v2f{x[2].x, x[2].y}, a0);
  a1 = __builtin_elementwise_fma(v2f{w[2].z, w[2].w}, v2f{x[2].z, x[2].w}, a1);
  a2 = __builtin_elementwise_fma(v2f{w[3].x, w[3].y}, v2f{x[3].x, x[3].y}, a2);
  a3 = __builtin_elementwise_fma(v2f{w[3].z, w[3].w}, v2f{x[3].z, x[3].w}, a3);
  const v2f t = (a0 + a2) + (a1 + a3);
  return t.x + t.y;
}

// MULTI = false: one sequence per pipeline (nseq == nb), the form every config-2 figure up to
// batch 16 is measured on.  MULTI = true: pipeline b serves sequences b, b + nb, b + 2 nb, ... < nseq.
// SEQ: the head reads each sequence's sampling settings from a.per_seq (mvn_generate_seq); the layer stages do not differ.
// GUIDED (mvn_generate_guided): MULTI and SEQ with nseq = 2 nb -- pipeline b serves the unconditional row b and the
// conditional row b + nb of pair b in its two turns; only the head stage differs (pipe_common.h: head_loop).
template <bool MULTI, bool SEQ, bool GUIDED = false>
__global__ __launch_bounds__(512, 2) void gen_fold_kernel(KArgs<SEQ, GUIDED> a, u64 *hand, unsigned *err, int NS, int nb, int nseq) {
  using namespace fold;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // (xcd, slot) -> (pipeline, stage): a pipeline of NS <= 32 stages sits in one XCD (speed only;
  // every edge verifies its own placement below).  The CUs an XCD has left over behind its whole pipelines
  // (config 2: 32 - 2 x 11 = 10) form further pipelines ACROSS XCDs (80 CUs: seven more) -- slower hops, which
  // does not matter where they are used: launches whose step is bound by the stages' service time per turn.
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int in_xcd = (PIPE_XCD_CUS / NS) * NS;  // slots of an XCD's whole pipelines
  int b, s;
  if (slot < in_xcd) {
    b = xcd + 8 * (slot / NS);
    s = slot % NS;
  } else {
    const int idx = xcd * (PIPE_XCD_CUS - in_xcd) + (slot - in_xcd);
    b = 8 * (PIPE_XCD_CUS / NS) + idx / NS;
    s = idx % NS;
  }
  if (b >= nb) return;
  if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;  // sticky status
  const int L = a.L;
  const int s_next = s + 1 == NS ? 0 : s + 1;
  const int G = MULTI ? (nseq - b + nb - 1) / nb : 1;  // sequences of this pipeline
  int bq = b;                                           // the sequence whose turn it is
  u64 *inbox = hand + ((size_t)b * NS + s) * GRAN;
  u64 *outbox = hand + ((size_t)b * NS + s_next) * GRAN;
  int *iflag = (int *)(smem + LDS_FLOATS - 16);  // [0] ok flag, [3] fast-edge flag
  float *pfs = smem + LDS_FLOATS;                // MULTI: [GMAX][C][PFS_F] (layer stages), head: indices
  float *win = smem + (MULTI ? WIN_OFF_MULTI : WIN_OFF_ONE) + WIN_F * __builtin_amdgcn_readfirstlane(wave);  // this wave's inbox strip
  const bool fast_edge = pipe_edge_is_fast(err + 16, b, s, s_next, NS, iflag);

  // ================= layer stage: layers l0 .. l0 + nl - 1 =================
  // Two forms, chosen per workgroup (s is block-uniform).  FIRST: stage 0 has no previous layer -- its inbox carries xp
  // alone (the head sends no zl and no skip sum), x_0 = xp, its skip sum starts at 0, and the products against
  // A0', B1', Wr_prev and Ws_prev (packed as zeros for it) are not formed.  Each of them added w * 0 to a finite
  // sum, which is exact; the one assumption is that the weights are finite (0 * inf would have been a NaN).
  auto layer_stage = [&](auto first_stage) {
    constexpr bool FIRST = decltype(first_stage)::value;
    const bool last = s == NS - 2;  // feeds the head, which reads zl' and sk' only
    const int l0 = s * LPS, nl = min(LPS, L - l0);
    const bool chain = tid < 256;
    const int t = tid & 255, c = t >> 2, kq = t & 3;
    const bool lead = kq == 0;
    float *lmat = smem;                  // WP0 | WP1 | WP2 | SS
    // LDS vectors, addressed as constant offsets from two per-lane bases (kept opaque so that
    // every access is base register + immediate instead of a register per address)
    constexpr int O_XP = 0;              // [C] inbox: stream without the last residual term
    constexpr int O_ZL = C;              // [C] inbox: previous stage's last gated activation
    constexpr int O_Z0 = 2 * C, O_Z1 = 3 * C;
    constexpr int O_X0 = 4 * C;          // [C] layer 0's input, explicit
    constexpr int O_B1 = 5 * C, O_B2 = 7 * C;  // [2C] each, helper -> chain
    constexpr int O_PAST = 9 * C;        // [LPS][C] popped queue entries
    constexpr int O_CTX = 12 * C;        // [C] context vector of the step being prepared
    constexpr int O_VEC = 13 * C;        // [VEC_F] the stage's constant vectors
    float *vec = smem + N_LDS_MAT * MAT_F;
    unsigned vc = lds_addr(vec) + 4u * c;          // this lane's channel
    unsigned vq = lds_addr(vec) + 4u * KPER * kq;  // this lane's 16 inputs
    asm volatile("" : "+v"(vc), "+v"(vq));
    // the wave's strip holds xp | zl as the vectors do (O_XP, O_ZL): byte offset from the vectors, wave-uniform
    unsigned wo = lds_addr(win) - lds_addr(vec);
    u64 *ob = outbox + c;                // granules of this lane's channel: xp' | zl' (+ C) | sk' (+ 2C)
    const u64 *ibs = inbox + 2 * C + c;
    float *ring = a.state + (size_t)b * a.state_per_seq;
    auto bind = [&](int g) {  // MULTI: the pointers of sequence b + g nb
      bq = b + g * nb;
      inbox = hand + ((size_t)bq * NS + s) * GRAN;
      outbox = hand + ((size_t)bq * NS + s_next) * GRAN;
      ob = outbox + c;
      ibs = inbox + 2 * C + c;
      ring = a.state + (size_t)bq * a.state_per_seq;
    };
    const float *sec = a.w + EMB_F + (size_t)s * STAGE_F;
    const float *vecs = sec + N_MAT * MAT_F;

    // chain waves: A0, A0', A1, A2, B2'; helper waves: B1, B1', B2, RR, RS
    FoldMat m0, m1 = {}, m2, m3, m4;
    {
      const int first = chain ? M_A0 : M_B1;
      fold_load(m0, sec + (size_t)(first + 0) * MAT_F, t);
      if (!FIRST) fold_load(m1, sec + (size_t)(first + 1) * MAT_F, t);  // A0' / B1'
      fold_load(m2, sec + (size_t)(first + 2) * MAT_F, t);
      fold_load(m3, sec + (size_t)(first + 3) * MAT_F, t);
      fold_load(m4, sec + (size_t)(first + 4) * MAT_F, t);
      const f4 *src = (const f4 *)(sec + (size_t)M_WP0 * MAT_F);
      for (int i = tid; i < N_LDS_MAT * MAT_F / 4; i += NT) ((f4 *)lmat)[i] = src[i];
    }
    // (the two groups never need each other's per-lane values: one set of registers serves
    // both -- chain: pf/pg of the three layers and the four folded-bias constants; helpers:
    // the explicit inputs xs of the three layers (queue pushes) and the six biases)
    float pf[LPS], pg[LPS];
    float (&xs)[LPS] = pf;
    int doff[LPS], dmask[LPS];
    // the stage's bias vectors live in LDS behind the step vectors (read where needed: the six
    // per-lane copies cost the chain its registers)
    for (int i = tid; i < VEC_F; i += NT) vec[O_VEC + i] = vecs[i];
    // the step vectors start as zeros: a stage with fewer than LPS real layers never writes the popped entries of the
    // missing ones, and their (zero) past-tap matrices would multiply whatever the LDS held -- 0 * NaN is a NaN
    for (int i = tid; i < O_VEC; i += NT) vec[i] = 0.f;
#pragma unroll
    for (int j = 0; j < LPS; ++j) {
      pf[j] = 0.f; pg[j] = 0.f;
      const int l = l0 + j;
      dmask[j] = j < nl ? (1 << (l % a.layer_size)) - 1 : 0;
      doff[j] = j < nl ? ring_offset(l, a.layer_size, C) : 0;
    }

    // Off the critical path: push this step's layer inputs into the dilation queues, pop the
    // entries step tn needs (helper lead lanes), then the past-tap half of step tn's f/g sums
    // (chain waves, matrices streamed from LDS).  Addresses are rebuilt here behind an
    // optimisation fence (the chain needs the registers, this code has slack).
    // MULTI: a turn's service time is what bounds the step beyond ~5 sequences per pipeline, and
    // most of it was the round trip of these pops (128 sequences' queues are 100 MB: MALL / HBM,
    // not L2).  The entries step tn needs were pushed at least two steps ago (dilation 1 takes
    // this step's value instead), so they are requested at the TOP of the turn and arrive under
    // the wait for the inbox and the chain.
    float (&popv)[LPS] = pg;  // (helper lanes only, which never touch pg: three registers the MULTI forms do not have to spare)
    auto prefetch_pops = [&](int tn) {
      if (MULTI && !chain && lead) {
        int cq = c;
        asm volatile("" : "+v"(cq));
#pragma unroll
        for (int j = 0; j < LPS; ++j)
          if (j < nl) popv[j] = ring_load(ring + doff[j] + cq + (tn & dmask[j]) * C);
      }
    };
    auto precompute = [&](int tn, bool push, bool popped) {
      int tq = t;
      asm volatile("" : "+v"(tq));
      const int cq = tq >> 2, kk = tq & 3;
      if (!chain && lead) {
#pragma unroll
        for (int j = 0; j < LPS; ++j)
          if (j < nl) {
            float *base = ring + doff[j] + cq;
            if (push) base[((tn - 1) & dmask[j]) * C] = xs[j];
            const float pv = (push && dmask[j] == 0) ? xs[j]
                             : (MULTI && popped) ? popv[j] : ring_load(base + (tn & dmask[j]) * C);
            vec[O_PAST + j * C + cq] = pv;
          }
      }
      if (a.ctx_tm && chain && tq < C) vec[O_CTX + tq] = a.ctx_tm[(size_t)bq * a.ctx_stride_b + (size_t)tn * C + tq];
      __syncthreads();
      if (chain) {
        const unsigned wm = lds_addr(lmat) + 16u * tq, xq = lds_addr(vec) + 4u * (O_PAST + KPER * kk);
        const v2f p0 = pair_dot_lds(wm, xq);
        const v2f p1 = pair_dot_lds(wm + 4u * MAT_F, xq + 4u * C);
        const v2f p2 = pair_dot_lds(wm + 8u * MAT_F, xq + 8u * C);
        pf[0] = chan_sum<KQ>(p0.x);
        pg[0] = chan_sum<KQ>(p0.y);
        pf[1] = chan_sum<KQ>(p1.x) + vec[O_VEC + V_CB1 + cq];
        pg[1] = chan_sum<KQ>(p1.y) + vec[O_VEC + V_CB1 + C + cq];
        pf[2] = chan_sum<KQ>(p2.x) + vec[O_VEC + V_CB2 + cq];
        pg[2] = chan_sum<KQ>(p2.y) + vec[O_VEC + V_CB2 + C + cq];
        if (a.ctx_tm) {
          // 1x1 context convs (modules.py:58-63, :75-77), weights streamed from L2
#pragma unroll
          for (int j = 0; j < LPS; ++j)
            if (j < nl) {
              const float *wc = a.wctx + (size_t)(l0 + j) * CTX_LAYER_F;
              pf[j] += chan_sum<KQ>(dot_stream<NF4>((const f4 *)wc, 256, tq, vec + O_CTX + KPER * kk)) + wc[MAT_F + cq];
              pg[j] += chan_sum<KQ>(dot_stream<NF4>((const f4 *)wc + NF4 * 256, 256, tq, vec + O_CTX + KPER * kk)) +
                       wc[MAT_F + C + cq];
            }
        }
      }
    };
    // MULTI: a sequence's pf / pg between its turns (lead lanes of the chain waves write, the four
    // lanes of a channel read the same 32 bytes)
    auto save_pf = [&](int g) {
      if (MULTI && chain && lead) {
        float *q = pfs + ((size_t)g * C + c) * PFS_F;
        *(f4 *)q = f4{pf[0], pg[0], pf[1], pg[1]};
        *(v2f *)(q + 4) = v2f{pf[2], pg[2]};
      }
    };
    auto load_pf = [&](int g) {
      if (MULTI && chain) {
        const float *q = pfs + ((size_t)g * C + c) * PFS_F;
        const f4 v = *(const f4 *)q;
        const v2f w = *(const v2f *)(q + 4);
        pf[0] = v.x; pg[0] = v.y; pf[1] = v.z; pg[1] = v.w; pf[2] = w.x; pg[2] = w.y;
      }
    };
    if (tid == 0) iflag[0] = 1;  // cleared by a wave whose hand-off times out
    __syncthreads();
    if (MULTI) {
      for (int g = 0; g < G; ++g) {
        bind(g);
        precompute(a.t_begin, false, false);
        save_pf(g);
        __syncthreads();  // the chain waves have read this sequence's popped entries: the next one's may land
      }
    } else {
      precompute(a.t_begin, false, false);
    }

    bool alive = true;
    for (int ts = a.t_begin; ts < a.t_end && alive; ++ts)
    for (int g = 0; g < G; ++g) {
      if (MULTI) {
        bind(g);
        if (ts + 1 < a.t_end) prefetch_pops(ts + 1);
      }
      const unsigned epoch = (unsigned)(ts - a.t_begin + 1);
      {
        // EVERY wave takes the 2C granules itself: lane i takes 2i, 2i + 1 (xp for i < 32, zl above) with one 16-byte load
        // (FIRST: xp alone) and leaves them in the wave's own strip, which the wave alone reads -- behind its own write,
        // so neither a wait for the write nor a barrier stands between "granules visible" and the first ds_read
        float v[2];
        const bool ok = FIRST ? wait_inbox64(inbox, epoch, err, v) : wait_inbox<2>(inbox, epoch, err, v);
        if (ok && (!FIRST || lane < 32)) {
          float *dst = win + 2 * lane;  // O_XP and O_ZL are adjacent
          dst[0] = v[0];
          dst[1] = v[1];
        }
        if (!ok && lane == 0) iflag[0] = 0;  // (the wave runs the step on stale values and leaves with the others below)
        asm volatile("" ::: "memory");
      }
      asm volatile("" : "+s"(wo));  // (added to the bases where used: not one more address register across the step)
      MVN_STAMP(b, s, ts - a.t_begin, 0);
      load_pf(g);
      float xv = 0.f;  // helper lead lanes: the explicit stream
      MVN_FINE(b, s, ts - a.t_begin, 0, 0);
      // ---- phase 0
      if (chain) {
        f4 xa[NF4], xb[NF4];
        ldsv<NF4>(xa, vq + wo, O_XP);
        if (!FIRST) ldsv<NF4>(xb, vq + wo, O_ZL);
        v2f acc[4];
        pair_acc<true>(acc, m0.w, xa);
        if (!FIRST) pair_acc<false>(acc, m1.w, xb);
        const v2f fg = pair_sum(acc);
        const float f = chan_sum<KQ>(fg.x) + pf[0];
        const float g = chan_sum<KQ>(fg.y) + pg[0];
        const float z = gate_fast(f, g);
        if (lead) LDSF(vc, O_Z0) = z;
        MVN_FINE(b, s, ts - a.t_begin, 1, 0);
      } else {
        f4 xa[NF4], xb[NF4];
        ldsv<NF4>(xa, vq + wo, O_XP);
        if (!FIRST) ldsv<NF4>(xb, vq + wo, O_ZL);
        v2f acc[4];
        pair_acc<true>(acc, m0.w, xa);
        if (!FIRST) pair_acc<false>(acc, m1.w, xb);
        const v2f fg = pair_sum(acc);
        float r = 0.f;                                             // (FIRST: the + 0 keeps a -0 of xp what it was, +0)
        if (!FIRST) r = split_dot<0>(m3.w, xb);                    // Wr_prev zl
        const float f = chan_sum<KQ>(fg.x);
        const float g = chan_sum<KQ>(fg.y);
        if (!FIRST) r = chan_sum<KQ>(r);
        if (lead) {
          xv = LDSF(vc + wo, O_XP) + r;               // x_0 (br_prev already inside xp)
          LDSF(vc, O_X0) = xv;
          xs[0] = xv;
          LDSF(vc, O_B1) = f;
          LDSF(vc, O_B1 + C) = g;
        }
        MVN_FINE(b, s, ts - a.t_begin, 6, 256);
      }
      lds_barrier();
      MVN_FINE(b, s, ts - a.t_begin, 2, 0);
      // ---- phase 1
      v2f b2 = {0.f, 0.f};  // chain: (Wc_2 Wr_0) z_0, this thread's 16 inputs; helpers: .x = their 16 terms of Wr_0 z_0
      // z_0, this lane's 16 inputs: both groups read it here; the chain keeps it across the phase-1 barrier for its
      // second product on it, (Wc_2 Wr_0) z_0, which is first needed at the end of phase 2 (one set of registers for both
      // groups: held in the chain's branch alone, the 16 registers would be live through the helpers' phase 1 as well)
      vf4 z0v[NF4];
#pragma unroll
      for (int i = 0; i < NF4; ++i) z0v[i] = *(const lds_f4 *)(uintptr_t)(vq + 4u * O_Z0 + 16u * i);
      if (chain) {
        const f4 xz[NF4] = {as_f4(z0v[0]), as_f4(z0v[1]), as_f4(z0v[2]), as_f4(z0v[3])};
        v2f acc[4];
        pair_acc<true>(acc, m2.w, xz);
        const v2f fg = pair_sum(acc);
        const float f = chan_sum<KQ>(fg.x) + (LDSF(vc, O_B1) + pf[1]);
        const float g = chan_sum<KQ>(fg.y) + (LDSF(vc, O_B1 + C) + pg[1]);
        const float z = gate_fast(f, g);
        if (lead) LDSF(vc, O_Z1) = z;
        MVN_FINE(b, s, ts - a.t_begin, 3, 0);
      } else {
        // x_1 = x_0 + Wr_0 z_0 + br_0 is first needed for x_2, in phase 2, but xp' must not leave the stage after zl':
        // the next stage waits for both in ONE inbox wait, and xp' is off the critical chain.  So the product is
        // split over the two phases: this thread's 16 terms of Wr_0 z_0 are summed here and held in b2.x (the
        // register pair the chain keeps its own b2 in); the cross-lane adds and the stream update wait for phase 2.
        // (Measured, DESIGN 4.1c: this phase closes on the helpers again, ~100 cycles later; the hop gives back more.)
        f4 xa[NF4];
        ldsv<NF4>(xa, vq, O_X0);
        const f4 xz0[NF4] = {as_f4(z0v[0]), as_f4(z0v[1]), as_f4(z0v[2]), as_f4(z0v[3])};
        v2f acc[4];
        pair_acc<true>(acc, m2.w, xa);                             // Wc_2 x_0
        b2.x = split_dot<1>(m3.w, xz0);                            // Wr_0 z_0, before the sum over the channel's lanes
        asm volatile("" : "+v"(b2));                               // formed here, not sunk behind the barrier
        const v2f fg = pair_sum(acc);
        const float f = chan_sum<KQ>(fg.x);
        const float g = chan_sum<KQ>(fg.y);
        if (lead) {
          LDSF(vc, O_B2) = f;
          LDSF(vc, O_B2 + C) = g;
        }
        MVN_FINE(b, s, ts - a.t_begin, 7, 256);
      }
      lds_barrier();
      MVN_FINE(b, s, ts - a.t_begin, 4, 0);
      // ---- phase 2: the chain's z_2 and the helpers' xp' leave as granules; the skip sum follows
      if (chain) {
        // the four reads of z_1 go out first; while the LDS serves them (about 128 cycles in which nothing else on the
        // chain is ready) the SIMD issues (Wc_2 Wr_0) z_0 from the registers kept since phase 1.  Two fences hold the
        // product in that window: the first (behind the reads, which may not sink past it) keeps it behind the barrier,
        // the second makes b2 a value BEFORE z_1's first quartet is one (every accumulator chain of the next product starts
        // on that quartet), so the waits for the reads stand behind the product.
        vf4 z1v[NF4];
#pragma unroll
        for (int i = 0; i < NF4; ++i) z1v[i] = *(const lds_f4 *)(uintptr_t)(vq + 4u * O_Z1 + 16u * i);
        asm volatile("" : "+v"(z0v[0]), "+v"(z0v[1]), "+v"(z0v[2]), "+v"(z0v[3]) : : "memory");
        v2f acc[4], acc2[4];
        pair_acc_sel(acc2, m4.w, z0v);
        b2 = pair_sum(acc2);
        asm volatile("" : "+v"(b2), "+v"(z1v[0]));
        const f4 xz[NF4] = {as_f4(z1v[0]), as_f4(z1v[1]), as_f4(z1v[2]), as_f4(z1v[3])};
        pair_acc<true>(acc, m3.w, xz);
        const v2f fg = pair_sum(acc) + b2;
        const float f = chan_sum<KQ>(fg.x) + (LDSF(vc, O_B2) + pf[2]);
        const float g = chan_sum<KQ>(fg.y) + (LDSF(vc, O_B2 + C) + pg[2]);
        const float z = gate_fast(f, g);
        if (lead) put_granule(ob + C, epoch, z, fast_edge);
        MVN_FINE(b, s, ts - a.t_begin, 5, 0);
      } else {
        u64 sk_peek = 0;
        if (!FIRST) sk_peek = peek_granule(ibs);
        // the residual biases, read by every lane in front of z_1 (volatile: not to be sunk into the lead lanes' block
        // behind the cross-lane adds, where the LDS round trip stood in front of the xp' put)
        const float br0v = *(volatile lds_f *)(uintptr_t)(vc + 4u * (O_VEC + V_BR0));
        const float br1v = *(volatile lds_f *)(uintptr_t)(vc + 4u * (O_VEC + V_BR1));
        const float br2v = *(volatile lds_f *)(uintptr_t)(vc + 4u * (O_VEC + V_BR2));
        f4 xz[NF4];
        ldsv<NF4>(xz, vq, O_Z1);
        // the stream: x_1, x_2 for the queue pushes, and xp' = x_2 + br_2 for the next stage (the head does not read it)
        auto stream = [&](bool send) {
          float br0 = send ? br0v : LDSF(vc, O_VEC + V_BR0), br1 = send ? br1v : LDSF(vc, O_VEC + V_BR1),
                br2 = send ? br2v : LDSF(vc, O_VEC + V_BR2);
          float r0 = b2.x;                                         // Wr_0 z_0: the 16 terms summed in phase 1
          float r = split_dot<0>(m4.w, xz);                        // Wr_1 z_1
          asm volatile("" : "+v"(br0), "+v"(br1), "+v"(br2));      // (in registers before the cross-lane adds)
          r0 = chan_sum<KQ>(r0);
          r = chan_sum<KQ>(r);
          if (lead) {
            xv = (xv + br0) + r0;       // x_1
            xs[1] = xv;
            xv = (xv + br1) + r;        // x_2
            xs[2] = xv;
            if (send) put_granule(ob, epoch, xv + br2, fast_edge);
          }
          MVN_FINE(b, s, ts - a.t_begin, 8, 256);
        };
        // skip lane: sk' = sk + (Ws_prev zl + bs_prev) + (Ws_0 z_0 + bs_0) + (Ws_1 z_1 + bs_1)
        auto skip = [&] {
          float k1 = split_dot<1>(m4.w, xz);
          unsigned wss = lds_addr(lmat + 3 * MAT_F) + 16u * t;  // SS = {Ws_prev; Ws_0}
          asm volatile("" : "+v"(wss));
          float kp = 0.f;
          if (!FIRST) kp = split_dot_lds<0>(wss, vq + wo + 4u * O_ZL);
          float k0 = split_dot_lds<1>(wss, vq + 4u * O_Z0);
          if (!FIRST) kp = chan_sum<KQ>(kp);
          k0 = chan_sum<KQ>(k0);
          k1 = chan_sum<KQ>(k1);
          if (lead) {
            const float bs0 = LDSF(vc, O_VEC + V_BS0), bs1 = LDSF(vc, O_VEC + V_BS1);
            float sk0 = 0.f;  // FIRST: the skip sum starts here
            if (!FIRST) {
              const float bsp = LDSF(vc, O_VEC + V_BSP);
              const float skin = (unsigned)(sk_peek >> 32) == epoch ? __uint_as_float((unsigned)sk_peek)
                                                                    : wait_granule(ibs, epoch, err);
              sk0 = skin + (kp + bsp);
            }
            put_granule(ob + 2 * C, epoch, (sk0 + (k0 + bs0)) + (k1 + bs1), fast_edge);
          }
          MVN_FINE(b, s, ts - a.t_begin, 9, 256);
        };
        if (last) {
          // the head cannot form its first activation without sk': here the skip lane is ON the step's critical path,
          // so it goes first, and the stream (needed after the closing barrier only) is not sent at all
          skip();
          stream(false);
        } else {
          stream(true);
          skip();
        }
      }
      MVN_STAMP(b, s, ts - a.t_begin, 1);
      lds_barrier();  // iflag and the step's LDS vectors are settled for everyone
      if (iflag[0] == 0) {  // some wave's hand-off timed out (checked after the step: off the chain)
        alive = false;
        break;
      }
      if (ts + 1 < a.t_end) {
        precompute(ts + 1, true, true);
        save_pf(g);
      } else if (!chain && lead) {
        // last step of the launch: push only (the next launch pops in its prologue)
        int cq = c;
        asm volatile("" : "+v"(cq));
#pragma unroll
        for (int j = 0; j < LPS; ++j)
          if (j < nl) ring[doff[j] + cq + (ts & dmask[j]) * C] = xs[j];
      }
    }
  };
  if (s < NS - 1) {
    if (s == 0)
      layer_stage(std::true_type{});
    else
      layer_stage(std::false_type{});
    return;
  }

  // ============================ head stage ============================
  {
    float *tab = smem;                    // embedding tables [2][Q][C] (128 KB)
    float *vec = smem + N_LDS_MAT * MAT_F;
    float *a0 = vec + C;                  // [C] lrelu(skip)  (the last layer's gated activation: in every wave's strip)
    float *a1 = a0 + C;                   // [Q] conv1's result: wave w writes, and alone reads, a1[32 w .. 32 w + 31]
    float *b2l = a1 + Q;                  // [Q] conv2's bias (wave 0 reads it with the partial sums: four registers less)
    float *part = pfs + HEAD_PART_OFF;    // [8][Q] conv2's partial sums: row w = wave w's k-slice, all outputs
    const float *E0 = tab, *E1 = tab + Q * C;
    const float *hw = a.w + EMB_F + (size_t)(NS - 1) * STAGE_F;
    const f4 *W1p = (const f4 *)hw, *W2p = (const f4 *)(hw + W1_F + Q);
    const float *b1 = hw + W1_F, *b2 = hw + W1_F + Q + W2_F;
    const f4 *WSp = (const f4 *)(hw + W1_F + Q + W2_F + Q);
    const float *bsl = hw + W1_F + Q + W2_F + Q + WSL_F;
    int *hidx = (int *)pfs;  // MULTI: [GMAX][2] = {idx_cur, idx_prev} of each sequence between its turns

    // last layer's skip 1x1: thread (cs = tid >> 3, q8 = tid & 7), 8 inputs;
    // conv1: thread (o1 = tid >> 1, q1 = tid & 1), 32 inputs; conv2 by k-slices: thread (wave, lane), outputs
    // 4 lane .. 4 lane + 3 x inputs 32 wave .. 32 wave + 31 -- the 32 values conv1 has just left in this very wave.
    // The packed section is pack_head_f32's [r][i8][tid] for thread (og = tid >> 3, q2 = tid & 7): this thread takes
    // what tid = 8 lane + wave took there (uncoalesced, once per launch)
    const int o1 = tid >> 1, q1 = tid & 1, og = tid >> 3, q2 = tid & 7;
    v2f wsl[4], w1[16], w2[4][16];
    {
      const f4 *src = (const f4 *)a.w;
      f4 *dst = (f4 *)tab;
      for (int i = tid; i < EMB_F / 4; i += NT) dst[i] = src[i];
      loadn<2>(wsl, WSp, NT, tid);
      loadn<8>(w1, W1p, NT, tid);
#pragma unroll
      for (int r = 0; r < 4; ++r) loadn<8>(w2[r], W2p + r * 8 * NT, NT, 8 * lane + wave);
    }
    const float b1r = b1[o1];
    if (tid < Q) b2l[tid] = b2[tid];
    const float bslr = bsl[og];
    if (tid == 0) iflag[0] = 1;  // cleared by a wave whose hand-off times out
    __syncthreads();

    // (head_loop starts a step with xp = the causal conv's two embedding rows alone: stage 0 reads no zl and no sk)
    // the strip's two addresses (lanes' writes, the skip 1x1's reads) are formed in the step, in front of the wait,
    // from the thread index: held across the step they cost the per-sequence form two spilled registers
    const unsigned zs = lds_addr(win);  // this wave's strip: zl alone is used
    unsigned zrd = 0;
    auto await = [&](const u64 *inbox, unsigned epoch) {  // every wave, into its own strip (head_loop: WAVE_INBOX)
      unsigned zq = __builtin_amdgcn_readfirstlane(zs), tq = tid;
      asm volatile("" : "+s"(zq), "+v"(tq));
      const unsigned wa = zq + 8u * (tq & 63u);
      zrd = zq + 32u * (tq & 7u);
      float v[2];
      const bool ok = wait_inbox64(inbox + C, epoch, err, v);  // zl (the last stage sends no xp')
      if (ok && lane < 32) {
        LDSF(wa, 0) = v[0];
        LDSF(wa, 1) = v[1];
      }
      asm volatile("" ::: "memory");
      return ok;
    };
    auto logits = [&](const u64 *inbox, unsigned epoch, bool do_head) {
      MVN_FINE(b, NS - 1, epoch - 1, 0, 0);
      const u64 sk_peek = peek_granule(inbox + 2 * C + og);
      float sv = 0.f;
      if (do_head) {
        // the last layer's skip 1x1 (modules.py:90-91)
        f4 x[2];
        ldsv<2>(x, zrd, 0);  // behind this wave's own write
        sv = dotn<2>(wsl, x);
        sv = quad_sum(sv);
        sv += other_quad(sv);
      }
      // the skip lane ends here, every step (the step's skip sums have then been consumed all
      // along the pipeline before the next sample enters it)
      float skin = 0.f;
      if (q2 == 0)
        skin = (unsigned)(sk_peek >> 32) == epoch ? __uint_as_float((unsigned)sk_peek)
                                                  : wait_granule(inbox + 2 * C + og, epoch, err);
      MVN_FINE(b, NS - 1, epoch - 1, 1, 0);
      if (!do_head) {
        lds_barrier();  // (the one meeting of such a step: no wave is ever more than a step behind wave 0's send)
        return;
      }
      // skip sum, then the head's first leaky-ReLU (modules.py:140)
      if (q2 == 0) a0[og] = leaky(skin + (sv + bslr));
      lds_barrier();
      // conv1, and conv2 over the wave's own k-slice: the wave that forms a1[32 w ..] is the one that reads it, so no
      // barrier and no other wave's LDS traffic stands between the two (the LDS serves a wave's accesses in order)
      f4 x[8];
      {
        ldsn<8>(x, a0 + 32 * q1);
        float hsum = dotn<8>(w1, x);
        hsum += dpp_mov<DPP_XOR1>(hsum);
        const float h = leaky(hsum + b1r);  // both lanes of a pair hold it
        if (q1 == 0) a1[o1] = h;
        asm volatile("" ::: "memory");
        ldsn<8>(x, a1 + 32 * wave);  // one address per wave: a broadcast, no bank conflict
      }
      MVN_FINE(b, NS - 1, epoch - 1, 3, 0);
      ((f4 *)part)[64 * wave + lane] = f4{dotn<8>(w2[0], x), dotn<8>(w2[1], x), dotn<8>(w2[2], x), dotn<8>(w2[3], x)};
      lds_barrier();
      MVN_FINE(b, NS - 1, epoch - 1, 4, 0);
    };
    // wave 0: the logits of classes 4 lane .. 4 lane + 3 = the eight slices' partial sums, added as the DPP tree of
    // head_conv2_f32 adds them -- ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), then the bias: the same bits
    auto take = [&](const float *, int) {
      f4 p[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) p[j] = ((const f4 *)part)[64 * j + lane];
      const f4 b2v = ((const f4 *)b2l)[lane];
      f4 r;
      r.x = (((p[0].x + p[1].x) + (p[2].x + p[3].x)) + ((p[4].x + p[5].x) + (p[6].x + p[7].x))) + b2v.x;
      r.y = (((p[0].y + p[1].y) + (p[2].y + p[3].y)) + ((p[4].y + p[5].y) + (p[6].y + p[7].y))) + b2v.y;
      r.z = (((p[0].z + p[1].z) + (p[2].z + p[3].z)) + ((p[4].z + p[5].z) + (p[6].z + p[7].z))) + b2v.z;
      r.w = (((p[0].w + p[1].w) + (p[2].w + p[3].w)) + ((p[4].w + p[5].w) + (p[6].w + p[7].w))) + b2v.w;
      return r;
    };
    // (SEND_AHEAD for one sequence per pipeline only: several sequences in turn pay the row's read, which stands behind
    // the read of the turn's indices, in front of every wait -- DESIGN 4.1c)
    head_loop<C, GRAN, MULTI, SEQ, 2, 0, GUIDED, true, !MULTI>(a, hand, NS, nb, b, G, fast_edge, E0, E1, iflag, hidx, part, await, logits,
                                                 take);
  }
}

// ---- packing ---------------------------------------------------------------------------
// Per-layer parameter pointers of the (up to) four layers a stage section is built from:
// index 0 = the previous stage's last layer (NULL for stage 0), 1..3 = the stage's own layers
// (NULL where the model has fewer layers: such a layer is packed as zeros, which makes it the
// identity -- z = gate(0, 0) = 0, no residual, no skip contribution).
struct FoldLayers {
  const float *fw[4], *gw[4], *rw[4], *rb[4], *sw[4], *sb[4];
};
__device__ __forceinline__ double fold_wc(const FoldLayers &p, int j, int row, int k) {  // current tap
  return p.fw[j] ? (double)fg_elem(p.fw[j], p.gw[j], fold::C, row, fold::C + k) : 0.0;
}
__device__ __forceinline__ double fold_wr(const FoldLayers &p, int j, int o, int k) {
  return p.rw[j] ? (double)p.rw[j][(size_t)o * fold::C + k] : 0.0;
}
__device__ __forceinline__ double fold_br(const FoldLayers &p, int j, int o) { return p.rb[j] ? (double)p.rb[j][o] : 0.0; }

__global__ void pack_fold_stage_kernel(FoldLayers p, float *__restrict__ dst) {
  using namespace fold;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= STAGE_F) return;
  if (i >= N_MAT * MAT_F) {
    const int o = i - N_MAT * MAT_F;
    double v = 0.0;
    if (o < V_CB2) {            // cb1 = Wc_1 br_0
      for (int m = 0; m < C; ++m) v += fold_wc(p, 2, o - V_CB1, m) * fold_br(p, 1, m);
    } else if (o < V_BSP) {     // cb2 = Wc_2 (br_0 + br_1)
      for (int m = 0; m < C; ++m) v += fold_wc(p, 3, o - V_CB2, m) * (fold_br(p, 1, m) + fold_br(p, 2, m));
    } else if (o < V_BR0) v = p.sb[0] ? p.sb[0][o - V_BSP] : 0.0;
    else if (o < V_BS0) v = fold_br(p, 1, o - V_BR0);
    else if (o < V_BR1) v = p.sb[1] ? p.sb[1][o - V_BS0] : 0.0;
    else if (o < V_BS1) v = fold_br(p, 2, o - V_BR1);
    else if (o < V_BR2) v = p.sb[2] ? p.sb[2][o - V_BS1] : 0.0;
    else v = fold_br(p, 3, o - V_BR2);
    dst[i] = (float)v;
    return;
  }
  // matrix element in the per-thread order: [2 NF4][t (256)] float4; thread t = 4c + kq owns rows
  // (c, C + c) x inputs 16 kq .. 16 kq + 15 (FoldMat)
  const int mat = i / MAT_F, r = i - mat * MAT_F;
  const int e = r & 3, v4 = r >> 2, t = v4 & 255, i4 = v4 >> 8;
  const bool split = mat == M_RR || mat == M_RS || mat == M_SS;
  // SPLIT: float4 i4 of half i4 / 4 holds inputs 4 (i4 % 4) + e of row t / KQ;
  // PAIR: float4 i4 holds {row c, row C + c} at inputs 2 i4 and 2 i4 + 1
  const int row = split ? (i4 / NF4) * C + t / KQ : (e & 1) * C + t / KQ;
  const int k = KPER * (t % KQ) + (split ? 4 * (i4 % NF4) + e : 2 * i4 + (e >> 1));
  double v = 0.0;
  auto prod = [&](int jc, int jr) {  // (Wc_jc Wr_jr)[row][k]
    double acc = 0.0;
    for (int m = 0; m < C; ++m) acc += fold_wc(p, jc, row, m) * fold_wr(p, jr, m, k);
    return acc;
  };
  auto ws = [&](int j, int o) { return p.sw[j] ? (double)p.sw[j][(size_t)o * C + k] : 0.0; };
  auto wp = [&](int j) { return p.fw[j] ? (double)fg_elem(p.fw[j], p.gw[j], C, row, k) : 0.0; };  // past tap
  switch (mat) {
    case M_A0: v = fold_wc(p, 1, row, k); break;
    case M_A0P: v = prod(1, 0); break;
    case M_A1: v = prod(2, 1); break;
    case M_A2: v = prod(3, 2); break;
    case M_B2P: v = prod(3, 1); break;
    case M_B1: v = fold_wc(p, 2, row, k); break;
    case M_B1P: v = prod(2, 0); break;
    case M_B2: v = fold_wc(p, 3, row, k); break;
    case M_RR: v = row < C ? fold_wr(p, 0, row, k) : fold_wr(p, 1, row - C, k); break;
    case M_RS: v = row < C ? fold_wr(p, 2, row, k) : ws(2, row - C); break;
    case M_WP0: v = wp(1); break;
    case M_WP1: v = wp(2); break;
    case M_WP2: v = wp(3); break;
    case M_SS: v = row < C ? ws(0, row) : ws(1, row - C); break;
  }
  dst[i] = (float)v;
}

// the fp32 head's sections (pipe_common.h: pack_head_f32), then the last layer's skip 1x1 and its bias
__global__ void pack_fold_head_kernel(const float *w1, const float *b1, const float *w2, const float *b2,
                                      const float *sw_last, const float *sb_last, float *__restrict__ dst, int qm) {
  using namespace fold;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (pack_head_f32(i, C, C / 2, qm, w1, b1, w2, b2, dst)) return;
  if (i < W1_F + Q + W2_F + Q + WSL_F) {
    // last layer's skip 1x1: [2][tid (512)] float4, thread (cs = tid >> 3, q8 = tid & 7) owns 8 inputs
    const int ii = i - (W1_F + Q + W2_F + Q);
    const int e = ii & 3, v = ii >> 2, tid = v & (NT - 1), i2 = v >> 9;
    dst[i] = sw_last ? sw_last[(size_t)(tid >> 3) * C + 8 * (tid & 7) + 4 * i2 + e] : 0.f;
  } else if (i < HEAD_F) {
    dst[i] = sb_last ? sb_last[i - (W1_F + Q + W2_F + Q + WSL_F)] : 0.f;
  }
}

static int fold_stages(const mvn_dims *d) { return (n_layers(d) + fold::LPS - 1) / fold::LPS + 1; }
static bool fold_ok(const mvn_dims *d) {
  // (r4: Q in {64, 128, 256} -- the head runs 256 classes wide, a smaller model's are padded at pack time)
  return d->residual_channels == 64 && d->skip_channels == 64 && head_q_ok(d->input_channels) &&
         n_layers(d) >= 1 && fold_stages(d) <= PIPE_XCD_CUS;
}
static size_t fold_inbox_floats(const mvn_dims *) { return 2 * fold::GRAN; }
static int fold_pipelines(const mvn_dims *d) { return 8 * (PIPE_XCD_CUS / fold_stages(d)); }  // co-resident pipelines
static int fold_pipelines_max(const mvn_dims *d) {  // ... plus the pipelines the XCDs' left-over CUs form across XCDs
  const int NS = fold_stages(d);
  return fold_pipelines(d) + 8 * (PIPE_XCD_CUS - (PIPE_XCD_CUS / NS) * NS) / NS;
}
static int fold_max_batch(const mvn_dims *d) { return fold::GMAX * fold_pipelines_max(d); }     // GMAX sequences each
// Pipelines a launch of `batch` sequences runs on: one sequence each up to fold_pipelines(d) (the fastest step);
// rounds on those while the pipeline's latency bounds the step (up to FOLD_LATENCY_ROUNDS each); every pipeline
// the chip holds beyond that, where the step is rounds x the stages' service time per turn
constexpr int FOLD_LATENCY_ROUNDS = 5;
static int fold_launch_pipelines(const mvn_dims *d, int batch) {
  const int p = fold_pipelines(d);
  if (batch <= p) return batch;
  return batch <= FOLD_LATENCY_ROUNDS * p ? p : fold_pipelines_max(d);
}
static size_t fold_weights_floats(const mvn_dims *d) {
  return (size_t)fold::EMB_F + (size_t)(fold_stages(d) - 1) * fold::STAGE_F + fold::HEAD_F;
}

// (context section: the PIPE variant's per-layer layout -- same thread mapping --, packed by it)
static int fold_pack(const mvn_dims *d, const mvn_params *p, float *packed, float *ctx_section, hipStream_t s) {
  using namespace fold;
  const int L = n_layers(d), NSL = fold_stages(d) - 1;
  pack_embed(C, p->causal_w, packed, d->input_channels, s);
  for (int st = 0; st < NSL; ++st) {
    FoldLayers fl;
    for (int j = 0; j < 4; ++j) {
      const int l = st * LPS - 1 + j;
      const bool ok = l >= 0 && l < L;
      fl.fw[j] = ok ? p->filter_w[l] : nullptr;
      fl.gw[j] = ok ? p->gate_w[l] : nullptr;
      fl.rw[j] = ok ? p->residual_w[l] : nullptr;
      fl.rb[j] = ok ? p->residual_b[l] : nullptr;
      fl.sw[j] = ok ? p->skip_w[l] : nullptr;
      fl.sb[j] = ok ? p->skip_b[l] : nullptr;
    }
    hipLaunchKernelGGL(pack_fold_stage_kernel, dim3((STAGE_F + 255) / 256), dim3(256), 0, s, fl,
                       packed + EMB_F + (size_t)st * STAGE_F);
  }
  // the head adds the skip 1x1 of the last stage's THIRD layer (index NSL * LPS - 1); when the
  // model ends earlier that slot is a zero layer (packed as zeros here) and the real last
  // layer's skip term was already added inside its stage
  const int l_tail = NSL * LPS - 1;
  const bool tail_real = l_tail < L;
  hipLaunchKernelGGL(pack_fold_head_kernel, dim3((HEAD_F + 255) / 256), dim3(256), 0, s, p->head1_w, p->head1_b,
                     p->head2_w, p->head2_b, tail_real ? p->skip_w[l_tail] : nullptr,
                     tail_real ? p->skip_b[l_tail] : nullptr, packed + EMB_F + (size_t)NSL * STAGE_F, d->input_channels);
  const int rc = check_hip(hipGetLastError(), "fold_pack");
  return rc || !ctx_section ? rc : pipe_pack_ctx(d, p, ctx_section, s);
}

// Up to fold_pipelines(d) sequences: one sequence per pipeline (gen_fold_kernel<false>).  More:
// the pipelines serve ceil(batch / pipelines) sequences each in turn (gen_fold_kernel<true>).
// `guided`: batch = 2 pairs rows on exactly `pairs` pipelines, two turns each (gen_fold_kernel<true, true, true>).
static int fold_launch_any(const GenArgs &a, const mvn_dims *d, int batch, float *hand, size_t hand_floats_total,
                           size_t status_offset_floats, hipStream_t s, bool guided) {
  using namespace fold;
  PipeLaunch p;
  p.name = FOLD_VARIANT.name;
  p.NT = NT;
  p.NS = fold_stages(d);
  p.GRAN = GRAN;
  p.pipes = guided ? batch / 2 : fold_launch_pipelines(d, batch);
  const bool multi = guided || batch > p.pipes;
  p.fn = guided ? (const void *)gen_fold_kernel<true, true, true> : a.per_seq ? (multi ? (const void *)gen_fold_kernel<true, true> : (const void *)gen_fold_kernel<false, true>)
                   : (multi ? (const void *)gen_fold_kernel<true, false> : (const void *)gen_fold_kernel<false, false>);
  p.lds_bytes = (multi ? LDS_FLOATS_MULTI : LDS_FLOATS_ONE) * sizeof(float);
  // the kernel's own map: whole pipelines inside the XCDs, or every CU (the left-over ones form pipelines across XCDs)
  p.slots = p.pipes <= fold_pipelines(d) ? (p.pipes + 7) / 8 * p.NS : PIPE_XCD_CUS;
  p.batch = batch;
  p.max_batch = fold_max_batch(d);
  p.per_pipe = GMAX;
  return pipe_launch_common(p, a, hand, hand_floats_total, status_offset_floats, s);
}
static int fold_launch(const GenArgs &a, const mvn_dims *d, int batch, float *hand, size_t hand_floats_total,
                       size_t status_offset_floats, hipStream_t s) {
  return fold_launch_any(a, d, batch, hand, hand_floats_total, status_offset_floats, s, false);
}
static int fold_launch_guided(const GenArgs &a, const mvn_dims *d, int pairs, float *hand, size_t hand_floats_total,
                              size_t status_offset_floats, hipStream_t s) {
  return fold_launch_any(a, d, 2 * pairs, hand, hand_floats_total, status_offset_floats, s, true);
}

#ifndef __HIP_DEVICE_COMPILE__  // (the device pass would emit the constant, host function pointers and all)
const GenVariant FOLD_VARIANT = {
    MVN_GEN_FOLD, "FOLD", fold_ok, fold_stages, fold_inbox_floats, fold_max_batch, fold_launch_pipelines,
    fold_weights_floats, fold_pack, fold_launch, fold_launch_guided,
    "FOLD variant needs C=K=64, Q in {64,128,256}, 256 CUs and batch <= %d for these dims "
    "(ceil(L/3)+1 stages per sequence, 32 per XCD)"};
#endif

}  // namespace mvn

#ifdef MVN_PIPE_STAMPS
extern "C" int mvn_debug_read_stamps_fold(unsigned long long *out, size_t n) { return mvn::debug_read(mvn::g_stamps, out, n, "read stamps"); }
extern "C" int mvn_debug_read_fine_fold(unsigned long long *out, size_t n) { return mvn::debug_read(mvn::g_fine, out, n, "read fine"); }
#endif
