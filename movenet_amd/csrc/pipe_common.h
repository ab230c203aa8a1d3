// Shared by the pipelined generator kernels (generate_pipe.hip: fp32, C = 64 / 128; generate_fold.hip: fp32,
// C = 64, folded layers; generate_pipe_h16.hip: fp16 operands, C = 128): placement and its handshake, the granule
// hand-off, cross-lane moves as DPP, the gate, the step-closing choice (double softmax or, MVN_SAMPLE_MODEL, the
// model's own softmax; top-k / top-p truncation; arg-max / inverse-CDF sample), the head stage's step loop and the
// fp32 head's packing.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "gen_common.h"

namespace mvn {

typedef unsigned long long u64;
typedef float4 f4;

constexpr int PIPE_XCD_CUS = 32;  // CUs per XCD: one workgroup (133 KB of LDS) per CU
constexpr unsigned PIPE_SPIN_LIMIT = 1u << 23;
constexpr int HEAD_Q = 256, HEAD_NT = 512;  // every pipelined head: 256 classes wide, 512 threads

// How the pipelined generators are launched.  Default: hipLaunchCooperativeKernel -- the runtime then guarantees
// what the hand-offs need, every stage of every pipeline co-resident (it refuses the launch otherwise, and does not
// run the grid beside another kernel of the process).  With an ORDINARY launch that guarantee is only the host's
// occupancy check: a second stream or process holding CUs starves a stage, which spins up to PIPE_SPIN_LIMIT polls
// per wait before it raises the sticky status word and the caller reruns on a kernel without hand-offs
// (worst case ~2.3 s per starved wait at ~0.28 us per poll with s_sleep).
// The ordinary launch is taken in exactly two cases:
//   * a profiler's tool library is attached to the process (rocprofv3 / rocprofiler-sdk tool, rocprof v1 / v2): the cooperative
//     queue the HIP runtime creates is torn down at process exit inside libhsa-runtime64 AFTER rocprofiler-sdk has
//     finalised its queue interception -- every rocprofv3 run of a process that had made one cooperative launch
//     ended in SIGSEGV at exit (r3: stack resolved in profiles/r03_exit_crash.md; same step time either way);
//   * MOVENET_PIPE_COOPERATIVE_LAUNCH=0 asks for it (=1 forces the cooperative form even under a profiler).
inline bool pipe_profiler_attached() {
  for (const char *v : {"ROCP_TOOL_LIBRARIES", "ROCPROFILER_REGISTER_FORCE_LOAD", "HSA_TOOLS_LIB", "ROCP_METRICS"})
    if (const char *e = getenv(v))
      if (e[0]) return true;
  if (const char *pre = getenv("LD_PRELOAD"))
    if (strstr(pre, "rocprof")) return true;
  bool found = false;
  if (FILE *f = fopen("/proc/self/maps", "r")) {  // a tool library injected any other way
    char line[512];
    while (!found && fgets(line, sizeof line, f))
      // (not libroctracer64 / librocprofiler-register: every PyTorch process maps those)
      found = strstr(line, "librocprofiler-sdk-tool") || strstr(line, "librocprofiler64");
    fclose(f);
  }
  return found;
}
inline bool pipe_cooperative_launch() {
  static const bool on = [] {
    const char *e = getenv("MOVENET_PIPE_COOPERATIVE_LAUNCH");
    if (e && (e[0] == '0' || e[0] == '1')) return e[0] == '1';
    return !pipe_profiler_attached();
  }();
  return on;
}

// Placement of gen_pipe_kernel and gen_pipe_h16_kernel (gen_fold_kernel has a map of its own).  Workgroup i is
// dispatched to XCD i % 8 (observed; every edge verifies its placement in pipe_edge_is_fast, so this is speed
// only -- but co-residency needs <= 32 workgroups per XCD, which the host checks with the arithmetic below).  A
// pipeline of NS <= 32 stages sits in one XCD so that its hops stay inside one L2: floor(32 / NS) pipelines in each
// of the 8 XCDs; a longer one spans pipe_span(NS) adjacent XCDs.
__host__ __device__ inline int pipe_span(int NS) { return (NS + PIPE_XCD_CUS - 1) / PIPE_XCD_CUS; }
inline int pipe_pipelines_of(int NS) {  // co-resident pipelines of NS stages
  return NS <= PIPE_XCD_CUS ? 8 * (PIPE_XCD_CUS / NS) : 8 / pipe_span(NS);
}
inline int pipe_grid_slots(int NS, int pipes) {  // the grid is 8 workgroups (one per XCD) per slot
  return NS <= PIPE_XCD_CUS ? (pipes + 7) / 8 * NS : (NS + pipe_span(NS) - 1) / pipe_span(NS);
}
// workgroup `block` -> pipeline b, stage s; false: a workgroup with nothing to do
__device__ __forceinline__ bool pipe_place(unsigned block, int NS, int &b, int &s) {
  const int xcd = block & 7, slot = block >> 3;
  if (NS <= PIPE_XCD_CUS) {
    b = xcd + 8 * (slot / NS);
    s = slot % NS;
    return true;
  }
  const int XS = pipe_span(NS), SPX = (NS + XS - 1) / XS;
  b = xcd / XS;
  s = (xcd % XS) * SPX + slot;
  return slot < SPX && s < NS;
}

// Placement handshake of edge (b, s) -> (b, s_next): publish my XCC id (+1), read my consumer's.  `xcc`: the
// [nb * NS] placement words, zeroed by the launch's memset; `iflag`: the stage's LDS flag words ([3] is used here).
// True when both ends were found on one XCD; unknown (time-out) => false, the safe form.
__device__ __forceinline__ bool pipe_edge_is_fast(unsigned *xcc, int b, int s, int s_next, int NS, int *iflag) {
  const unsigned mine = (__builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xF) + 1;  // HW_REG_XCC_ID[3:0]
  if (threadIdx.x == 0) {
    __hip_atomic_store(xcc + b * NS + s, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned other = 0;
    for (unsigned spins = 0; spins < (1u << 20) && other == 0; ++spins) {
      other = __hip_atomic_load(xcc + b * NS + s_next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (other == 0) __builtin_amdgcn_s_sleep(8);
    }
    iflag[3] = (other == mine) ? 1 : 0;
  }
  __syncthreads();
  const bool fast = iflag[3] != 0;
  __syncthreads();
  return fast;
}

#ifdef MVN_PIPE_STAMPS
// Diagnostic build only (python -m movenet_amd.csrc.build --stamps): wall-clock
// (s_memrealtime, 100 MHz) stamps of "inbox complete" and "outbox sent" per stage
// for the first 64 steps of a launch; read back with mvn_debug_read_stamps().
static __device__ unsigned long long g_stamps[16][16][64][4];
#define MVN_STAMP(bb, ss, step, which)                                              \
  do {                                                                              \
    if ((bb) < 16 && (ss) < 16 && (step) < 64 && threadIdx.x == 0) {                \
      g_stamps[bb][ss][step][which] = __builtin_amdgcn_s_memrealtime();             \
      g_stamps[bb][ss][step][2 + (which)] = __builtin_amdgcn_s_memtime();           \
    }                                                                               \
  } while (0)
// finer shader-clock stamps inside a stage (thread `who`)
static __device__ unsigned long long g_fine[16][16][64][12];
#define MVN_FINE(bb, ss, step, slot, who)                                           \
  do {                                                                              \
    if ((bb) < 16 && (ss) < 16 && (step) < 64 && threadIdx.x == (who))              \
      g_fine[bb][ss][step][slot] = __builtin_amdgcn_s_memtime();                    \
  } while (0)
// body of the mvn_debug_read_* exports (a set per translation unit: g_stamps / g_fine are static)
template <class T>
inline int debug_read(const T &sym, unsigned long long *out, size_t n, const char *what) {
  if (n > sizeof(T) / 8) n = sizeof(T) / 8;
  return check_hip(hipMemcpyFromSymbol(out, HIP_SYMBOL(sym), n * 8), what);
}
#else
#define MVN_STAMP(bb, ss, step, which) do {} while (0)
#define MVN_FINE(bb, ss, step, slot, who) do {} while (0)
#endif

// `same_xcd`: producer and consumer were FOUND (from HW_REG_XCC_ID, exchanged at kernel
// start) to sit on one XCD.  They then share one L2, so a plain store (write-through L1,
// line kept in that L2) is seen by the consumer's L1-bypassing polls: ~0.33 us per hop
// instead of ~0.6.  Otherwise the granule is stored sc1 (write-through to memory), the
// placement-independent form.  Placement only ever selects between two correct forms.
__device__ __forceinline__ void put_granule(u64 *g, unsigned epoch, float v, bool same_xcd) {
  const u64 x = ((u64)epoch << 32) | (u64)__float_as_uint(v);
  // same XCD: a relaxed WORKGROUP-scope atomic store -- on gfx950 the same write-through
  // global_store_dwordx2 as a plain store (line kept in the shared L2), but an atomic in the
  // memory model: never deferred, merged or torn by the compiler
  if (same_xcd)
    __hip_atomic_store(g, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else
    __hip_atomic_store(g, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Wave 0 only.  One 16-byte load fetches two granules, and the 64 lanes of a load cover
// 1 KB of the inbox contiguously: lane i owns granules 128*k + 2*i and 128*k + 2*i + 1 for
// k < GL/2 (v[2k], v[2k+1]).  Each granule is still validated by its own epoch word; a
// 16-byte aligned load never tears an 8-byte store.  Returns false on time-out / raised
// error word (wave-uniform).
typedef unsigned v4u __attribute__((ext_vector_type(4)));

// Two granules (16 bytes at p, per lane) polled with TWO loads in flight: a poll samples L2
// every half round trip instead of every whole one, which takes ~0.4 round trips off the
// expected detection delay of a hop.  The loop lives in one asm block on fixed registers
// (v240-v247, clobbered): registers with a load in flight must never be copied or renamed by
// the compiler, which a loop-carried C variable cannot promise.  Wave-uniform result: 1 when
// both epochs match in every active lane (v0, v1 = the values), 0 after 64 double polls.
__device__ __forceinline__ int poll16(const u64 *p, unsigned epoch, float &v0, float &v1) {
  int st;
  unsigned r0, r1;
  u64 tmp;  // lane mask scratch
  asm volatile(
      "s_movk_i32 %[st], 64\n\t"
      "global_load_dwordx4 v[240:243], %[p], off sc1\n"
      "1:\n\t"
      "global_load_dwordx4 v[244:247], %[p], off sc1\n\t"
      "s_waitcnt vmcnt(1)\n\t"
      "v_cmp_eq_u32 vcc, %[ep], v241\n\t"
      "v_cmp_eq_u32 %[t], %[ep], v243\n\t"
      "s_and_b64 vcc, vcc, %[t]\n\t"
      "s_cmp_eq_u64 vcc, exec\n\t"
      "s_cbranch_scc1 2f\n\t"
      "global_load_dwordx4 v[240:243], %[p], off sc1\n\t"
      "s_waitcnt vmcnt(1)\n\t"
      "v_cmp_eq_u32 vcc, %[ep], v245\n\t"
      "v_cmp_eq_u32 %[t], %[ep], v247\n\t"
      "s_and_b64 vcc, vcc, %[t]\n\t"
      "s_cmp_eq_u64 vcc, exec\n\t"
      "s_cbranch_scc1 3f\n\t"
      "s_sub_u32 %[st], %[st], 1\n\t"
      "s_cmp_lg_u32 %[st], 0\n\t"
      "s_cbranch_scc1 1b\n\t"
      "s_waitcnt vmcnt(0)\n\t"
      "s_mov_b32 %[st], 0\n\t"
      "s_branch 4f\n"
      "2:\n\t"
      "s_waitcnt vmcnt(0)\n\t"
      "v_mov_b32 %[r0], v240\n\t"
      "v_mov_b32 %[r1], v242\n\t"
      "s_mov_b32 %[st], 1\n\t"
      "s_branch 4f\n"
      "3:\n\t"
      "s_waitcnt vmcnt(0)\n\t"
      "v_mov_b32 %[r0], v244\n\t"
      "v_mov_b32 %[r1], v246\n\t"
      "s_mov_b32 %[st], 1\n"
      "4:\n"
      : [st] "=&s"(st), [r0] "=&v"(r0), [r1] "=&v"(r1), [t] "=&s"(tmp)
      : [p] "v"(p), [ep] "s"(epoch)
      : "vcc", "scc", "memory", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247");
  v0 = __uint_as_float(r0);
  v1 = __uint_as_float(r1);
  return st;
}
// The bounded wait around poll16(): false on time-out / raised error word (wave-uniform).
__device__ __forceinline__ bool wait16(const u64 *p, unsigned epoch, unsigned *err, float &v0, float &v1) {
  for (unsigned calls = 1;; ++calls) {
    if (poll16(p, epoch, v0, v1)) return true;
    const unsigned e = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 || calls > PIPE_SPIN_LIMIT / 128) {
      if ((threadIdx.x & 63) == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
  }
}

// The skip granule was sent a stage time ago: its load is issued at the START of the phase
// that ends with its use (the round trip through L2 would otherwise sit on the skip lane, and
// through it on the head); the spin loop is only the fallback.
__device__ __forceinline__ u64 peek_granule(const u64 *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One granule of the skip lane, polled by the lane that owns the channel (off the chain: it was
// sent a whole stage time ago).  A time-out raises the status word; the caller carries on with
// the stale value (the host sees the word).
__device__ __forceinline__ float wait_granule(const u64 *p, unsigned epoch, unsigned *err) {
  for (unsigned spins = 1;; ++spins) {
    unsigned lo, hi;
    {
      typedef unsigned v2u __attribute__((ext_vector_type(2)));
      v2u g;
      asm volatile("global_load_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(g) : "v"(p) : "memory");
      lo = g.x;
      hi = g.y;
    }
    if (hi == epoch) return __uint_as_float(lo);
    if ((spins & 255u) == 0) {
      const unsigned e = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (e != 0 || spins > PIPE_SPIN_LIMIT) {
        __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return __uint_as_float(lo);
      }
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

template <int GL>
__device__ __forceinline__ bool wait_inbox(const u64 *in, unsigned epoch, unsigned *err,
                                           float (&v)[GL]) {
  static_assert(GL == 2 || GL == 4, "one or two 16-byte loads per lane");
  const int lane = threadIdx.x & 63;
  const u64 *p = in + 2 * lane;
  if (GL == 2) return wait16(p, epoch, err, v[0], v[1]);
  for (unsigned spins = 1;; ++spins) {
    v4u g0, g1;
    asm volatile("global_load_dwordx4 %0, %2, off sc1\n\t"
                 "global_load_dwordx4 %1, %2, off offset:1024 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(g0), "=&v"(g1) : "v"(p) : "memory");
    const bool ok = g0.y == epoch && g0.w == epoch && g1.y == epoch && g1.w == epoch;
    if (__all(ok)) {
      v[0] = __uint_as_float(g0.x);
      v[1] = __uint_as_float(g0.z);
      v[GL - 2] = __uint_as_float(g1.x);
      v[GL - 1] = __uint_as_float(g1.z);
      return true;
    }
    if ((spins & 255u) == 0) {
      const unsigned e = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (e != 0 || spins > PIPE_SPIN_LIMIT) {
        if (lane == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
      }
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

// 64 granules (512 bytes) of an inbox: lanes 0-31 take two each with one 16-byte load (lanes
// 32-63 repeat them).  v[0], v[1] = granules 2 (lane & 31), + 1 of `in`.  Wave-uniform result.
__device__ __forceinline__ bool wait_inbox64(const u64 *in, unsigned epoch, unsigned *err, float (&v)[2]) {
  return wait16(in + 2 * (threadIdx.x & 31), epoch, err, v[0], v[1]);
}

// ---- cross-lane moves as DPP (one VALU op) instead of ds_bpermute (an LDS round trip)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
constexpr int DPP_XOR1 = 0xB1;         // quad_perm [1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;         // quad_perm [2,3,0,1]
constexpr int DPP_HALF_MIRROR = 0x141; // lane i <-> 7-i inside each group of 8
constexpr int DPP_MIRROR = 0x140;      // lane i <-> 15-i inside each row of 16

// sum over each aligned group of 4 lanes, result in all 4
__device__ __forceinline__ float quad_sum(float v) {
  v += dpp_mov<DPP_XOR1>(v);
  v += dpp_mov<DPP_XOR2>(v);
  return v;
}
// after quad_sum: the value held by the OTHER quad of the same group of 8
__device__ __forceinline__ float other_quad(float v) { return dpp_mov<DPP_HALF_MIRROR>(v); }

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v = quad_sum(v);
  v += dpp_mov<DPP_HALF_MIRROR>(v);
  v += dpp_mov<DPP_MIRROR>(v);  // every lane of a row of 16 now holds the row sum
  return (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  v = fmaxf(v, dpp_mov<DPP_XOR1>(v));
  v = fmaxf(v, dpp_mov<DPP_XOR2>(v));
  v = fmaxf(v, dpp_mov<DPP_HALF_MIRROR>(v));
  v = fmaxf(v, dpp_mov<DPP_MIRROR>(v));
  return fmaxf(fmaxf(lane_value(v, 0), lane_value(v, 16)), fmaxf(lane_value(v, 32), lane_value(v, 48)));
}

// tanh(f) * sigmoid(g) from two v_exp_f32 and one reciprocal-based division:
//   tanh(f) = (1 - e^-2|f|) / (1 + e^-2|f|) * sign(f),  sigmoid(g) = 1 / (1 + e^-g)
// Absolute error ~1e-7 (fp32 rounding of an O(1) value); ~12 VALU ops vs ~100 for
// the libm forms, and this sits on the per-layer critical path.
__device__ __forceinline__ float gate_fast(float f, float g) {
  const float a = __expf(-2.0f * fabsf(f));       // in (0, 1]
  const float e = __expf(-g);                      // may overflow to +inf: 1/inf = 0 is right
  const float num = copysignf(1.0f - a, f);
  const float den = (1.0f + a) * (1.0f + e);
  return num * __builtin_amdgcn_rcpf(den);  // v_rcp_f32: 1 ulp
}

// (value, index) arg-max combine: larger value wins, smaller index on ties
__device__ __forceinline__ void argmax_take(float &bv, int &bi, float ov, int oi) {
  if (ov > bv || (ov == bv && oi < bi)) {
    bv = ov;
    bi = oi;
  }
}
template <int CTRL>
__device__ __forceinline__ int dpp_movi(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}


typedef float v2f __attribute__((ext_vector_type(2)));

// N4*4-term dot product as packed FMAs (v_pk_fma_f32) in two (N4 = 4) or four independent
// chains, combined in a fixed order.  w: 2*N4 float2, x: the inputs already fetched from LDS.
template <int N4>
__device__ __forceinline__ float dotn(const v2f (&w)[2 * N4], const f4 (&x)[N4]) {
  v2f a0 = {0.f, 0.f}, a1 = {0.f, 0.f}, a2 = {0.f, 0.f}, a3 = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < N4; i += 2) {
    a0 = __builtin_elementwise_fma(w[2 * i], v2f{x[i].x, x[i].y}, a0);
    a1 = __builtin_elementwise_fma(w[2 * i + 1], v2f{x[i].z, x[i].w}, a1);
    a2 = __builtin_elementwise_fma(w[2 * i + 2], v2f{x[i + 1].x, x[i + 1].y}, a2);
    a3 = __builtin_elementwise_fma(w[2 * i + 3], v2f{x[i + 1].z, x[i + 1].w}, a3);
  }
  const v2f t = (a0 + a2) + (a1 + a3);
  return t.x + t.y;
}
template <int N4>
__device__ __forceinline__ void ldsn(f4 (&x)[N4], const float *p) {
#pragma unroll
  for (int i = 0; i < N4; ++i) x[i] = ((const f4 *)p)[i];
}
// N4 float4 of a [..][stride] block -> 2*N4 float2 registers
template <int N4>
__device__ __forceinline__ void loadn(v2f (&w)[2 * N4], const f4 *src, int stride, int idx) {
#pragma unroll
  for (int i = 0; i < N4; ++i) {
    const f4 v = src[i * stride + idx];
    w[2 * i] = v2f{v.x, v.y};
    w[2 * i + 1] = v2f{v.z, v.w};
  }
}
// Two rows against the same LDS vector, the vector fetched four float4 at a time with one
// chunk of look-ahead: at N4 = 16 only 32-48 of its 64 registers are live at once (the
// whole vector next to 128 weight registers spills).  Same accumulation order as dotn.
template <int N4>
__device__ __forceinline__ void dot2_lds(const v2f (&wa)[2 * N4], const v2f (&wb)[2 * N4],
                                         const float *xp, float &ra, float &rb) {
  constexpr int CH = 4, NCH = N4 / CH;
  static_assert(N4 % CH == 0, "whole chunks");
  v2f a0 = {0.f, 0.f}, a1 = {0.f, 0.f}, a2 = {0.f, 0.f}, a3 = {0.f, 0.f};
  v2f b0 = {0.f, 0.f}, b1 = {0.f, 0.f}, b2 = {0.f, 0.f}, b3 = {0.f, 0.f};
  f4 x[N4];
#pragma unroll
  for (int i = 0; i < CH; ++i) x[i] = ((const f4 *)xp)[i];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    if (ch + 1 < NCH) {
#pragma unroll
      for (int i = CH * (ch + 1); i < CH * (ch + 2); ++i) x[i] = ((const f4 *)xp)[i];
    }
    if (NCH > 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = CH * ch; i < CH * (ch + 1); i += 2) {
      const v2f x0 = {x[i].x, x[i].y}, x1 = {x[i].z, x[i].w};
      const v2f x2 = {x[i + 1].x, x[i + 1].y}, x3 = {x[i + 1].z, x[i + 1].w};
      a0 = __builtin_elementwise_fma(wa[2 * i], x0, a0);
      a1 = __builtin_elementwise_fma(wa[2 * i + 1], x1, a1);
      a2 = __builtin_elementwise_fma(wa[2 * i + 2], x2, a2);
      a3 = __builtin_elementwise_fma(wa[2 * i + 3], x3, a3);
      b0 = __builtin_elementwise_fma(wb[2 * i], x0, b0);
      b1 = __builtin_elementwise_fma(wb[2 * i + 1], x1, b1);
      b2 = __builtin_elementwise_fma(wb[2 * i + 2], x2, b2);
      b3 = __builtin_elementwise_fma(wb[2 * i + 3], x3, b3);
    }
    if (NCH > 1) __builtin_amdgcn_sched_barrier(0);
  }
  const v2f ta = (a0 + a2) + (a1 + a3), tb = (b0 + b2) + (b1 + b3);
  ra = ta.x + ta.y;
  rb = tb.x + tb.y;
}
// one row of dot2_lds (same chunking, same accumulation order as its `a` half)
template <int N4>
__device__ __forceinline__ float dot1_lds(const v2f (&wa)[2 * N4], const float *xp) {
  constexpr int CH = 4, NCH = N4 / CH;
  static_assert(N4 % CH == 0, "whole chunks");
  v2f a0 = {0.f, 0.f}, a1 = {0.f, 0.f}, a2 = {0.f, 0.f}, a3 = {0.f, 0.f};
  f4 x[N4];
#pragma unroll
  for (int i = 0; i < CH; ++i) x[i] = ((const f4 *)xp)[i];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    if (ch + 1 < NCH) {
#pragma unroll
      for (int i = CH * (ch + 1); i < CH * (ch + 2); ++i) x[i] = ((const f4 *)xp)[i];
    }
    if (NCH > 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = CH * ch; i < CH * (ch + 1); i += 2) {
      a0 = __builtin_elementwise_fma(wa[2 * i], v2f{x[i].x, x[i].y}, a0);
      a1 = __builtin_elementwise_fma(wa[2 * i + 1], v2f{x[i].z, x[i].w}, a1);
      a2 = __builtin_elementwise_fma(wa[2 * i + 2], v2f{x[i + 1].x, x[i + 1].y}, a2);
      a3 = __builtin_elementwise_fma(wa[2 * i + 3], v2f{x[i + 1].z, x[i + 1].w}, a3);
    }
    if (NCH > 1) __builtin_amdgcn_sched_barrier(0);
  }
  const v2f ta = (a0 + a2) + (a1 + a3);
  return ta.x + ta.y;
}
// dotn() with the weights fetched on the fly (LDS or L2), four float4 at a time so that
// only 32 registers are live; same accumulators and order as dotn: bit-identical to it
template <int N4>
__device__ __forceinline__ float dot_stream(const f4 *wsrc, int stride, int idx, const float *xsrc) {
  v2f a0 = {0.f, 0.f}, a1 = {0.f, 0.f}, a2 = {0.f, 0.f}, a3 = {0.f, 0.f};
#pragma unroll
  for (int i0 = 0; i0 < N4; i0 += 4) {
    f4 w[4], x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i] = wsrc[(i0 + i) * stride + idx];
      x[i] = ((const f4 *)xsrc)[i0 + i];
    }
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
      a0 = __builtin_elementwise_fma(v2f{w[i].x, w[i].y}, v2f{x[i].x, x[i].y}, a0);
      a1 = __builtin_elementwise_fma(v2f{w[i].z, w[i].w}, v2f{x[i].z, x[i].w}, a1);
      a2 = __builtin_elementwise_fma(v2f{w[i + 1].x, w[i + 1].y}, v2f{x[i + 1].x, x[i + 1].y}, a2);
      a3 = __builtin_elementwise_fma(v2f{w[i + 1].z, w[i + 1].w}, v2f{x[i + 1].z, x[i + 1].w}, a3);
    }
  }
  const v2f t = (a0 + a2) + (a1 + a3);
  return t.x + t.y;
}
// sum over the KQ lanes that share a channel (result in all of them)
template <int KQ>
__device__ __forceinline__ float chan_sum(float v) {
  v += dpp_mov<DPP_XOR1>(v);
  if (KQ == 4) v += dpp_mov<DPP_XOR2>(v);
  return v;
}


// Wave 0 closes a step alone: lane i owns the logits of classes 4i .. 4i+3 (Q = 256); every
// reduction is intra-wave (DPP + readlane), no barrier.  Returns the class WaveNet.generate
// picks for time u: softmax (wavenet.py:189-191), [/ T], softmax again, then multinomial by
// inverse CDF on the Philox uniform of (seed, u, b) or the first arg-max (:227-233); under
// MVN_SAMPLE_MODEL a sampled step draws from softmax(logits / T) instead (choose_class).
// v_exp_f32 / v_rcp_f32 forms (1-2 ulp): the choice depends on the ORDER of the
// probabilities, which these monotone maps preserve.
// Greedy decoding, the common case: when the largest logit leads the runner-up by a clear margin,
// the first arg-max of softmax(softmax(logits)) IS the arg-max of the logits, and ONE wave-wide
// reduction (value, index, runner-up) replaces the max, two sums and the arg-max of the full
// form below (~850 -> ~350 cycles of the head stage).  Why 1e-3 is clear: e = exp(l - max) of the
// runner-up is <= e^-0.001 = 0.999 (v_exp_f32 errs by 1-2 ulp of 6e-8), the first softmax keeps the
// ratio and its largest probability is >= 1/Q = 1/256, so the second softmax's inputs differ by
// >= 3.9e-6 and its exponentials by >= 60 ulp below 1.0; the final scaling is monotone.  Ties and
// near-ties (margin below 1e-3, NaNs) return false: the caller runs the full form.
__device__ __forceinline__ bool greedy_pick_clear(const float (&lg)[4], int lane, int &pick) {
  float bv = lg[0], sv = -INFINITY;
  int bi = 4 * lane;
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const bool up = lg[k] > bv;
    sv = up ? bv : fmaxf(sv, lg[k]);
    bi = up ? 4 * lane + k : bi;
    bv = up ? lg[k] : bv;
  }
  auto merge = [&](float ov, int oi, float os) {
    const bool up = ov > bv;
    sv = fmaxf(fmaxf(sv, os), up ? bv : ov);  // (equal maxima: the runner-up becomes the maximum, margin 0)
    bi = up ? oi : bi;
    bv = up ? ov : bv;
  };
  merge(dpp_mov<DPP_XOR1>(bv), dpp_movi<DPP_XOR1>(bi), dpp_mov<DPP_XOR1>(sv));
  merge(dpp_mov<DPP_XOR2>(bv), dpp_movi<DPP_XOR2>(bi), dpp_mov<DPP_XOR2>(sv));
  merge(dpp_mov<DPP_HALF_MIRROR>(bv), dpp_movi<DPP_HALF_MIRROR>(bi), dpp_mov<DPP_HALF_MIRROR>(sv));
  merge(dpp_mov<DPP_MIRROR>(bv), dpp_movi<DPP_MIRROR>(bi), dpp_mov<DPP_MIRROR>(sv));
  // every lane of a row of 16 now holds the row's triple; the four rows meet as scalars
  float rv = lane_value(bv, 0), rs = lane_value(sv, 0);
  int ri = __builtin_amdgcn_readlane(bi, 0);
#pragma unroll
  for (int row = 16; row < 64; row += 16) {
    const float ov = lane_value(bv, row), os = lane_value(sv, row);
    const int oi = __builtin_amdgcn_readlane(bi, row);
    const bool up = ov > rv;
    rs = fmaxf(fmaxf(rs, os), up ? rv : ov);
    ri = up ? oi : ri;
    rv = up ? ov : rv;
  }
  pick = ri;
  return rv - rs >= 1e-3f;
}

// The reference's double softmax of a step, unnormalised: e[k] = exp(p_k - max p) with p = softmax(lg) * inv_t
// (inv_t: 1 / T of a sampled step, 1 for a greedy one); returns the sum of e over the wave.
__device__ __forceinline__ float double_softmax(const float (&lg)[4], float m, float inv_t, int lane, int Q,
                                                float (&e)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) e[k] = __expf(lg[k] - m);
  const float sm = wave_sum_dpp((e[0] + e[1]) + (e[2] + e[3]));
  const float rs = __builtin_amdgcn_rcpf(sm) * inv_t;
  float p[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) p[k] = e[k] * rs;
  // max over p = rs exactly: the largest e is exp(0) = 1.0 (v_exp_f32 of 0 is exact), 1.0 * rs = rs,
  // and rounding is monotone for the others (e <= 1)  -- one wave-wide max reduction less per step
  const float m2 = rs;
  // (classes >= Q are the padding of a head that runs 256 wide for a smaller model: logit -inf, p = 0 -- and no mass
  // in this second softmax either, where exp(0 - m2) would give each of them some)
#pragma unroll
  for (int k = 0; k < 4; ++k) e[k] = 4 * lane + k < Q ? __expf(p[k] - m2) : 0.f;
  return wave_sum_dpp((e[0] + e[1]) + (e[2] + e[3]));
}

// Inverse CDF over the wave's 256 weights p (lane i: classes 4i .. 4i+3, need not sum to one): the smallest class
// whose running sum exceeds uniform * total, `fallback` if none does (Q - 1 without truncation).
// POSITIVE (truncated steps): only a class of positive weight may be picked.  In exact arithmetic the smallest
// qualifying class always has one; in fp32 the running sums of neighbouring classes are associated differently, and
// a class truncation has zeroed could otherwise qualify by a rounding before the kept class in front of it does.
template <bool POSITIVE>
__device__ __forceinline__ int sample_cdf(const float (&p)[4], float uniform, int lane, int fallback) {
  const float lsum = (p[0] + p[1]) + (p[2] + p[3]);
  // inclusive scan of the lane totals in class order: four DPP row shifts inside each row of 16
  // lanes (zeros shifted in), then the totals of the rows below as scalars (six __shfl_up steps
  // = six LDS-crossbar round trips before: ~0.25 us of every sampled step)
  float incl = lsum;
  incl += dpp_mov<0x111>(incl);  // row_shr:1
  incl += dpp_mov<0x112>(incl);  // row_shr:2
  incl += dpp_mov<0x114>(incl);  // row_shr:4
  incl += dpp_mov<0x118>(incl);  // row_shr:8
  {
    const float r0 = lane_value(incl, 15), r1 = lane_value(incl, 31), r2 = lane_value(incl, 47);
    const int row = lane >> 4;
    incl += row == 0 ? 0.f : row == 1 ? r0 : row == 2 ? r0 + r1 : (r0 + r1) + r2;
  }
  const float total = lane_value(incl, 63);
  const float target = uniform * total;
  const float cdf = incl - lsum;
  int cand = fallback;
  bool hit = false;
#pragma unroll
  for (int k = 3; k >= 0; --k) {
    // walk down so that the smallest qualifying class wins
    const float c_k = cdf + (k == 0 ? p[0] : k == 1 ? p[0] + p[1]
                                            : k == 2 ? (p[0] + p[1]) + p[2]
                                                     : ((p[0] + p[1]) + p[2]) + p[3]);
    if (c_k > target && (!POSITIVE || p[k] > 0.f)) {
      cand = 4 * lane + k;
      hit = true;
    }
  }
  // the smallest qualifying class over the wave = the candidate of the FIRST lane that has one
  // (classes ascend with the lane): one ballot and one readlane instead of a min-reduction
  const unsigned long long lanes = __builtin_amdgcn_ballot_w64(hit);
  return lanes ? __builtin_amdgcn_readlane(cand, __builtin_ctzll(lanes)) : fallback;
}

// Top-k / top-p truncation of a sampled step (include/movenet_hip.h, mvn_generate_trunc), wave 0: lane i holds the
// weights p >= 0 of classes 4i .. 4i+3.  Non-negative floats order like their bit patterns, so both thresholds are
// found EXACTLY, without a sort, by a radix select on the pattern, most significant bit first (31 rounds each; the
// sign bit is clear): a candidate bit stays set when the classes at or above the candidate still
//   top-k:  number >= top_k          (one ballot + popcount per register: scalar, no cross-lane move)
//   top-p:  hold >= top_p * S        (one wave_sum_dpp; S = what top-k kept, summed the same way)
// Both predicates only shrink as the candidate grows -- the fp32 sum too: every addition of non-negative terms is
// monotone in each of them -- so the greedy bit walk ends on the largest threshold that satisfies them: the top_k-th
// largest weight, and the largest weight value whose head of the distribution reaches top_p * S.  Classes below
// max(theta_k, theta_p), and the padding of a smaller model (>= Q), are zeroed in p.  Returns the highest-indexed
// kept class, the draw's fallback.  The largest weight is never dropped: no candidate above it is ever accepted.
__device__ __forceinline__ int truncate_weights(float (&p)[4], int top_k, float top_p, int lane, int Q) {
  unsigned u[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = __float_as_uint(p[k]);
  unsigned theta = 0;  // wave-uniform throughout
  if (top_k > 0) {
#pragma unroll 1
    for (int bit = 30; bit >= 0; --bit) {
      const unsigned cand = theta | (1u << bit);  // (> 0: a padding class, weight +0, never counts)
      int n = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) n += __builtin_popcountll(__builtin_amdgcn_ballot_w64(u[k] >= cand));
      if (n >= top_k) theta = cand;
    }
  }
  if (top_p < 1.f) {
    auto mass_from = [&](unsigned lo) {
      return wave_sum_dpp(((u[0] >= lo ? p[0] : 0.f) + (u[1] >= lo ? p[1] : 0.f)) +
                          ((u[2] >= lo ? p[2] : 0.f) + (u[3] >= lo ? p[3] : 0.f)));
    };
    const float need = top_p * mass_from(theta);
    unsigned tp = 0;
#pragma unroll 1
    for (int bit = 30; bit >= 0; --bit) {
      const unsigned cand = tp | (1u << bit);
      if (mass_from(cand > theta ? cand : theta) >= need) tp = cand;
    }
    theta = tp > theta ? tp : theta;
  }
  int top = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool keep = u[k] >= theta && 4 * lane + k < Q;
    p[k] = keep ? p[k] : 0.f;
    top = keep ? 4 * lane + k : top;
  }
  const unsigned long long lanes = __builtin_amdgcn_ballot_w64(top >= 0);
  return lanes ? __builtin_amdgcn_readlane(top, 63 - __builtin_clzll(lanes)) : Q - 1;
}

// `uniform`: philox_uniform(seed, u, b), formed by the caller BEFORE it waits for the step's input (ten
// Philox rounds of integer multiplies: ~0.15 us that do not depend on the logits).
// `sampling` (MVN_SAMPLE_*, wave-uniform) is read on sampled steps only: a greedy step leaves through its own
// branch first, the same code under both rules.  `top_k` / `top_p` (wave-uniform; 0 / 1: off) likewise: a sampled
// step with either set truncates its weights, whichever rule formed them, before the same inverse CDF.
__device__ __forceinline__ int choose_class(const float (&lg)[4], float temperature, int sampling, int top_k,
                                            float top_p, float uniform, int lane, int Q) {
  if (!(temperature > 0.f)) {
    int pick;
    if (greedy_pick_clear(lg, lane, pick)) return pick;
    const float m = wave_max_dpp(fmaxf(fmaxf(lg[0], lg[1]), fmaxf(lg[2], lg[3])));
    float e[4], p[4];
    const float rs2 = __builtin_amdgcn_rcpf(double_softmax(lg, m, 1.0f, lane, Q, e));
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = e[k] * rs2;  // the distribution generate() uses
    float bv = p[0];
    int bi = 4 * lane;
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (p[k] > bv) {  // strict: first maximum
        bv = p[k];
        bi = 4 * lane + k;
      }
    argmax_take(bv, bi, dpp_mov<DPP_XOR1>(bv), dpp_movi<DPP_XOR1>(bi));
    argmax_take(bv, bi, dpp_mov<DPP_XOR2>(bv), dpp_movi<DPP_XOR2>(bi));
    argmax_take(bv, bi, dpp_mov<DPP_HALF_MIRROR>(bv), dpp_movi<DPP_HALF_MIRROR>(bi));
    argmax_take(bv, bi, dpp_mov<DPP_MIRROR>(bv), dpp_movi<DPP_MIRROR>(bi));
    float rv = lane_value(bv, 0);
    pick = __builtin_amdgcn_readlane(bi, 0);
#pragma unroll
    for (int row = 16; row < 64; row += 16)
      argmax_take(rv, pick, lane_value(bv, row), __builtin_amdgcn_readlane(bi, row));
    return pick;
  }
  const float m = wave_max_dpp(fmaxf(fmaxf(lg[0], lg[1]), fmaxf(lg[2], lg[3])));
  const float inv_t = __builtin_amdgcn_rcpf(temperature);
  float p[4];
  if (sampling == MVN_SAMPLE_MODEL) {
    // softmax(logits / T), unnormalised: 1 / T folded into the exponent, no second softmax, and no division by
    // the sum either -- the inverse CDF scales its uniform by the total.  The largest weight is exp(0) = 1, so the
    // total lies in [1, 256]; a padding class (logit -inf) has exp(-inf) = 0 exactly.
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = __expf((lg[k] - m) * inv_t);
  } else {
    float e[4];
    const float rs2 = __builtin_amdgcn_rcpf(double_softmax(lg, m, inv_t, lane, Q, e));
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = e[k] * rs2;  // the distribution generate() uses
  }
  if (top_k > 0 || top_p < 1.f) {
    const int top = truncate_weights(p, top_k, top_p, lane, Q);
    return sample_cdf<true>(p, uniform, lane, top);
  }
  return sample_cdf<false>(p, uniform, lane, Q - 1);
}

// fp32 conv2 of the head: thread (og = tid >> 3, q2 = tid & 7) holds 4 output rows x 32 inputs in w2; the eight
// threads of a row group meet by DPP, and threads q2 < 4 store logits 4 og + q2
__device__ __forceinline__ void head_conv2_f32(const v2f (&w2)[4][16], const float *a1, float *lgb, int og, int q2,
                                               float b2r) {
  f4 x[8];
  ldsn<8>(x, a1 + 32 * q2);
  float s0 = dotn<8>(w2[0], x), s1 = dotn<8>(w2[1], x);
  float s2 = dotn<8>(w2[2], x), s3 = dotn<8>(w2[3], x);
  s0 = quad_sum(s0); s0 += other_quad(s0);
  s1 = quad_sum(s1); s1 += other_quad(s1);
  s2 = quad_sum(s2); s2 += other_quad(s2);
  s3 = quad_sum(s3); s3 += other_quad(s3);
  const int sel = q2 & 3;
  if (q2 < 4) lgb[4 * og + sel] = (sel == 0 ? s0 : sel == 1 ? s1 : sel == 2 ? s2 : s3) + b2r;
}

// The step loop of the head stage (the last stage of pipeline b; its consumer is stage 0), for every pipelined
// kernel.  Wave 0 closes every step alone (softmax, choice) and immediately opens the next one: it gathers the two
// embedding rows of the causal conv (modules.py:28-30 on a one-hot input; E0 / E1: the [Q][C] tables of the two
// taps) and hands them to stage 0, so no barrier sits between the choice and the next step's first hop.
// A granule row is GRAN = (1 + NZ) C wide: the residual stream, then NZ lanes that start a step as zeros (PIPE: the
// skip sum; FOLD: zl and the skip sum).  NZ_SENT of them are written as zeros for stage 0 (all, unless stage 0
// knows them to be zero and does not read them: FOLD).  What differs between the kernels is passed in:
//   await(inbox, epoch)            wave 0: wait for the head's input of this step, store it to LDS; false on time-out
//   logits(inbox, epoch, do_head)  all waves, behind a barrier: the dense head into lgb[256], closed by a barrier
//                                  (do_head is block-uniform; false: no logits are needed for this step)
//   take(lgb, lane)                wave 0, behind that barrier: the float4 of logits 4 lane .. 4 lane + 3.  Default: the
//                                  read of lgb; FOLD sums its waves' partial sums here instead (generate_fold.hip)
// WAVE_INBOX (FOLD): await is called by EVERY wave and stores the input where that wave alone reads it; no barrier
// follows it -- logits() meets at its own first barrier, also when do_head is false -- and iflag[0], set to 1 by the
// caller in front of a barrier, is cleared by a wave whose wait times out.
// SEND_AHEAD (FOLD; C = 64, one channel per lane of wave 0): the E0 row of a send is the row of idx_prev, which was
// idx_cur for the whole step before -- wave 0 reads its channel of E0[idx_cur] at the top of the step, in front of the
// wait for the step's input, and the value moves to idx_prev's place where the index does (a launch's first send, in
// front of the step loop, reads both rows; MULTI re-reads the indices from hidx at the top of a turn, and the row
// behind them -- FOLD leaves its MULTI forms on send_h0).  One LDS read less between the pick and the put; the sum is
// E1 + E0 as before.
// iflag / hidx: LDS words ([0]: the hand-off's ok flag; MULTI: [GMAX][2] = {idx_cur, idx_prev} of each sequence
// between its turns).
// SEQ (mvn_generate_seq): the settings of a step are those of the sequence whose turn it is, a.per_seq[bq], loaded
// where the uniform is formed -- before the wait for the step's input, off the dependent chain.
// GUIDED (mvn_generate_guided; MULTI and SEQ, G = 2, nb = pairs): pipeline b serves pair b -- turn 0 its unconditional
// row b, turn 1 its conditional row b + nb.  Turn 0 keeps the row's logits in wave 0's registers and closes nothing;
// turn 1 forms the guided logits from the two rows', makes the one choice by the conditional row's settings and opens
// the next step of BOTH rows (unconditional first: stage 0 serves it first).  No hand-off is added: stage 0 waits for
// its row's next input one turn longer, through the same bounded waits.
struct HeadLgbRead {
  __device__ __forceinline__ f4 operator()(const float *lgb, int lane) const { return ((const f4 *)lgb)[lane]; }
};
template <int C, int GRAN, bool MULTI, bool SEQ, int NZ, int NZ_SENT = NZ, bool GUIDED = false, bool WAVE_INBOX = false,
          bool SEND_AHEAD = false, class Await, class Logits, class Take = HeadLgbRead>
__device__ __forceinline__ void head_loop(const KArgs<SEQ, GUIDED> &a, u64 *hand, int NS, int nb, int b, int G, bool fast_edge,
                                          const float *E0, const float *E1, int *iflag, int *hidx, const float *lgb,
                                          Await await, Logits logits, Take take = Take()) {
  static_assert(GRAN == (1 + NZ) * C && NZ_SENT <= NZ, "residual stream + NZ zero lanes");
  static_assert(!SEND_AHEAD || C == 64, "SEND_AHEAD: one channel per lane of wave 0");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = NS - 1;
  int bq;  // the sequence whose turn it is: b + g nb
  const u64 *inbox;
  u64 *outbox;
  int32_t *samples;
  auto bind = [&](int g) {
    bq = b + g * nb;
    inbox = hand + ((size_t)bq * NS + s) * GRAN;
    outbox = hand + (size_t)bq * NS * GRAN;
    samples = a.samples + (size_t)bq * a.stride;
  };
  int idx_cur = 0, idx_prev = -1;
  auto send_h0 = [&](unsigned ep) {  // wave 0
    const int ic = min(max(idx_cur, 0), a.Q - 1), ip = min(idx_prev, a.Q - 1);
#pragma unroll
    for (int j = 0; j < C / 64; ++j) {
      const int ch = lane + 64 * j;
      float v = E1[ic * C + ch];
      if (ip >= 0) v += E0[ip * C + ch];
      put_granule(outbox + ch, ep, v, fast_edge);
#pragma unroll
      for (int z = 1; z <= NZ_SENT; ++z) put_granule(outbox + z * C + ch, ep, 0.f, fast_edge);
    }
  };
  // SEND_AHEAD, wave 0: this lane's channel of E0's row of idx_cur / of idx_prev (unused where the index is < 0)
  [[maybe_unused]] float e0_cur = 0.f, e0_prev = 0.f;
  auto send_ahead = [&](unsigned ep) {  // wave 0: send_h0 with idx_prev's row already in e0_prev
    float v = E1[min(max(idx_cur, 0), a.Q - 1) * C + lane];
    if (idx_prev >= 0) v += e0_prev;
    put_granule(outbox + lane, ep, v, fast_edge);
#pragma unroll
    for (int z = 1; z <= NZ_SENT; ++z) put_granule(outbox + z * C + lane, ep, 0.f, fast_edge);
  };
  for (int g = 0; g < G; ++g) {
    bind(g);
    if (wave == 0) {
      idx_cur = samples[a.t_begin];
      idx_prev = a.t_begin > 0 ? samples[a.t_begin - 1] : -1;
      if (a.t_begin < a.t_end) send_h0(1u);
      MVN_STAMP(b, s, 0, 1);
      if (MULTI && lane == 0) {
        hidx[2 * g] = idx_cur;
        hidx[2 * g + 1] = idx_prev;
      }
    }
  }
  if (MULTI) __syncthreads();

  [[maybe_unused]] float lgu[4] = {0.f, 0.f, 0.f, 0.f};  // GUIDED, wave 0: the unconditional row's logits of this step
  [[maybe_unused]] float sm1 = 0.f;                       // GUIDED: the pair's scale - 1 (wave-uniform)
  if constexpr (GUIDED) {
    static_assert(MULTI && SEQ, "a guided launch is a MULTI, SEQ launch of two turns per pipeline");
    sm1 = a.guidance[b] - 1.0f;
  }
  for (int ts = a.t_begin; ts < a.t_end; ++ts)
  for (int g = 0; g < G; ++g) {
    if (MULTI) {
      bind(g);
      if (wave == 0) {  // (written by this wave's lane 0 a whole round ago)
        idx_cur = hidx[2 * g];
        idx_prev = hidx[2 * g + 1];
      }
    }
    const unsigned epoch = (unsigned)(ts - a.t_begin + 1);
    const int u = ts + 1;
    const bool want_out = (a.logits_out || a.choices_out) && u >= a.logits_t0;
    const bool do_head = u < a.n_total && (u >= a.n_given || want_out);  // block-uniform
    int next_idx = 0;
    // this step's Philox uniform, formed while the step's input is still on its way (the fence
    // keeps it from being sunk to its use behind the head's barriers)
    float uni = 0.f;
    SeqSampling ss = seq_sampling((const GenScalarArgs &)a, bq);
    bool settings_turn = true;  // GUIDED: the settings, and the uniform, are the conditional row's -- turn 1 only
    if constexpr (GUIDED) settings_turn = g == 1;
    if (SEQ && wave == 0 && settings_turn) ss = seq_sampling(a, bq);
    if (wave == 0 && ss.temperature > 0.f) {
      uni = philox_uniform(ss.seed, (uint32_t)u, ss.row);
      asm volatile("" : "+v"(uni));
    }
    if constexpr (SEND_AHEAD) {
      if (wave == 0) {  // (MULTI: idx_cur is this turn's, just re-read from hidx)
        e0_cur = idx_cur >= 0 ? E0[min(idx_cur, a.Q - 1) * C + lane] : 0.f;
        asm volatile("" : "+v"(e0_cur));  // in a register before the wait, not sunk to the send
      }
    }
    if constexpr (WAVE_INBOX) {
      if (wave == 0 && u < a.n_given) next_idx = samples[u];  // prompt / teacher forcing
      if (!await(inbox, epoch) && lane == 0) iflag[0] = 0;
    } else {
      if (wave == 0) {
        if (u < a.n_given) next_idx = samples[u];  // prompt / teacher forcing
        const bool ok = await(inbox, epoch);
        if (lane == 0) iflag[0] = ok ? 1 : 0;
      }
      lds_barrier();
    }
    MVN_STAMP(b, s, ts - a.t_begin, 0);
    logits(inbox, epoch, do_head);
    if constexpr (GUIDED) {
      if (wave == 0) {
        const f4 lv = do_head ? take(lgb, lane) : f4{0.f, 0.f, 0.f, 0.f};
        if (do_head && a.logits_out && u >= a.logits_t0 && 4 * lane < a.Q)  // each row's own raw logits
          ((f4 *)(a.logits_out + ((size_t)bq * (a.n_total - a.logits_t0) + (u - a.logits_t0)) * a.Q))[lane] = lv;
        if (g == 0) {
          lgu[0] = lv.x; lgu[1] = lv.y; lgu[2] = lv.z; lgu[3] = lv.w;
        } else {
          int pick = 0;
          if (do_head) {
            // (classes >= Q, the padding of a 256-wide head, keep their -inf: -inf - -inf would be a NaN)
            const float lc[4] = {lv.x, lv.y, lv.z, lv.w};
            float lg[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) lg[k] = 4 * lane + k < a.Q ? guided_logit(lc[k], lgu[k], sm1) : lc[k];
            pick = choose_class(lg, ss.temperature, a.sampling, ss.top_k, ss.top_p, uni, lane, a.Q);
            if (u >= a.n_given) next_idx = pick;
          }
          idx_prev = idx_cur;  // (one pair of indices: both rows consume the same samples)
          idx_cur = next_idx;
          e0_prev = e0_cur;
          if (ts + 1 < a.t_end) {  // (SEND_AHEAD: one row read ahead, two puts)
            bind(0);
            SEND_AHEAD ? send_ahead(epoch + 1) : send_h0(epoch + 1);
            bind(1);
            SEND_AHEAD ? send_ahead(epoch + 1) : send_h0(epoch + 1);
          }
          if (lane == 0) {
            if (do_head) {
#pragma unroll
              for (int r = 0; r < 2; ++r) {
                const size_t row = (size_t)(b + r * nb);
                if (a.choices_out && u >= a.logits_t0) a.choices_out[row * a.n_total + u] = pick;
                if (u >= a.n_given) a.samples[row * a.stride + u] = pick;
              }
            }
            hidx[0] = hidx[2] = idx_cur;
            hidx[1] = hidx[3] = idx_prev;
          }
        }
      }
    } else
    if (wave == 0) {
      int pick = 0;
      if (do_head) {
        // lane i owns classes 4i..4i+3; every reduction is intra-wave (DPP + readlane)
        const f4 lv = take(lgb, lane);
        const float lg[4] = {lv.x, lv.y, lv.z, lv.w};
        // (rows of a.Q logits: the padding of a smaller model is not written; fp16 PIPE takes Q = 256 only)
        if (a.logits_out && u >= a.logits_t0 && 4 * lane < a.Q)
          ((f4 *)(a.logits_out + ((size_t)bq * (a.n_total - a.logits_t0) + (u - a.logits_t0)) * a.Q))[lane] = lv;
        pick = choose_class(lg, ss.temperature, a.sampling, ss.top_k, ss.top_p, uni, lane, a.Q);
        if (u >= a.n_given) next_idx = pick;
      }
      idx_prev = idx_cur;
      idx_cur = next_idx;
      e0_prev = e0_cur;
      if (ts + 1 < a.t_end) SEND_AHEAD ? send_ahead(epoch + 1) : send_h0(epoch + 1);
      MVN_STAMP(b, s, ts + 1 - a.t_begin, 1);
      MVN_FINE(b, s, ts - a.t_begin, 5, 0);
      if (do_head && lane == 0) {
        if (a.choices_out && u >= a.logits_t0) a.choices_out[(size_t)bq * a.n_total + u] = pick;
        if (u >= a.n_given) samples[u] = pick;
      }
      if (MULTI && lane == 0) {
        hidx[2 * g] = idx_cur;
        hidx[2 * g + 1] = idx_prev;
      }
    }
    if (iflag[0] == 0) return;  // hand-off timed out
  }
}

// ---- packing of the fp32 head (PIPE and FOLD) -----------------------------------------------------------------
// Element i of the sections conv1 | b1 | conv2 | b2 (W1_F + Q + W2_F + Q floats) in the per-thread register order;
// false when i lies behind them.  C: conv1's inputs, W1N = C / 2 of them per thread.  `qm`: the MODEL's class count
// (64, 128 or 256).  The head always runs 256 classes wide: classes >= qm are padding -- zero rows and columns,
// conv2 bias -inf, so that their logits are -inf (probability 0 in the first softmax; choose_class masks them in
// the second) and they are never picked.
__device__ __forceinline__ bool pack_head_f32(int i, int C, int W1N, int qm, const float *w1, const float *b1,
                                              const float *w2, const float *b2, float *__restrict__ dst) {
  constexpr int Q = HEAD_Q, NT = HEAD_NT;
  const int W1_F = Q * C, W2_F = Q * Q;
  if (i < W1_F) {
    // conv1: [W1N/4][tid (512)] float4, thread (o1 = tid>>1, q1 = tid&1) owns W1N inputs
    const int e = i & 3, v = i >> 2, tid = v & (NT - 1), i4 = v >> 9;
    const int o = tid >> 1;
    dst[i] = o < qm ? w1[(size_t)o * C + W1N * (tid & 1) + 4 * i4 + e] : 0.f;
  } else if (i < W1_F + Q) {
    dst[i] = i - W1_F < qm ? b1[i - W1_F] : 0.f;
  } else if (i < W1_F + Q + W2_F) {
    // conv2: [4 r][8][tid (512)] float4, thread (og = tid>>3, q2 = tid&7): output 4 og + r, inputs 32 q2 ..
    // (FOLD reads this section through the permutation tid = 8 lane + wave: its wave w owns inputs 32 w .., all outputs)
    const int ii = i - W1_F - Q;
    const int e = ii & 3, v = ii >> 2, tid = v & (NT - 1), rest = v >> 9, r = rest >> 3, i8 = rest & 7;
    const int o = 4 * (tid >> 3) + r, k = 32 * (tid & 7) + 4 * i8 + e;
    dst[i] = (o < qm && k < qm) ? w2[(size_t)o * qm + k] : 0.f;
  } else if (i < W1_F + Q + W2_F + Q) {
    const int o = i - W1_F - Q - W2_F;
    dst[i] = o < qm ? b2[o] : -INFINITY;
  } else {
    return false;
  }
  return true;
}

}  // namespace mvn
