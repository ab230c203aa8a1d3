// Shared by the generator kernels (generate.hip, generate_pipe.hip, generate_fold.hip, generate_pipe_h16.hip).
#pragma once
#include "common.h"

namespace mvn {

// GenScalarArgs: what a kernel takes where one temperature, seed, top_k and top_p hold for the whole launch -- the
// kernel argument of every instantiation that existed before mvn_generate_seq, layout unchanged (their code is the
// same to the instruction).  GenSeqArgs (below) adds the per-sequence array: the kernel argument of the SEQ
// instantiations, layout unchanged too.  GenArgs adds the guidance scales: what the host drivers pass around, and the
// kernel argument of the GUIDED instantiations.
struct GenScalarArgs {
  int L, layer_size, Q, C, K;
  const float *w;
  float *state;
  long long state_per_seq;
  int32_t *samples;
  int stride, n_total, n_given, t_begin, t_end;
  float temperature;
  uint64_t seed;
  float *logits_out;
  int32_t *choices_out;
  int logits_t0;
  int sampling;  // MVN_SAMPLE_*: the rule of a sampled step (temperature > 0); greedy steps do not consult it
  // truncation of a sampled step's weights before the draw (mvn_generate_trunc): keep the top_k largest (0: off;
  // the host passes 0 for top_k >= Q), then the smallest head of them that holds top_p of their mass (1: off)
  int top_k;
  float top_p;
  // local conditioning (NULL = audio only): context (B, n_total, C) time-major and the
  // packed context-conv section of the weight blob
  const float *ctx_tm;
  long long ctx_stride_b;
  const float *wctx;
};
struct GenSeqArgs : GenScalarArgs {
  // mvn_generate_seq: DEVICE array of one entry per sequence of the launch (NULL on every other entry point); the
  // kernels' SEQ instantiations read temperature, top_k, top_p, seed and row from it instead of the scalars above
  const mvn_seq_sampling *per_seq;
};
struct GenArgs : GenSeqArgs {
  // mvn_generate_guided: DEVICE array of one classifier-free guidance scale per pair of the launch (NULL on every other
  // entry point; read by the GUIDED instantiations alone).  Rows [0, pairs) are then the unconditional rows, rows
  // [pairs, 2 pairs) the conditional ones
  const float *guidance;
};
// The guided logits of a step (include/movenet_hip.h, mvn_generate_guided): sub, mul, add in fp32, `sm1` = s - 1.  The
// library is built with -ffp-contract=off, so nothing is fused: s = 1 returns lc.
__device__ __forceinline__ float guided_logit(float lc, float lu, float sm1) {
  const float d = lc - lu;
  const float m = sm1 * d;
  return lc + m;
}
// The kernel argument of an instantiation.  A launch hands every kernel a GenArgs; a scalar instantiation's
// parameter is its leading GenScalarArgs, a SEQ one's its leading GenSeqArgs (the bases sit at offset 0).
template <bool SEQ, bool GUIDED = false>
struct KArgsOf { typedef GenScalarArgs type; };
template <>
struct KArgsOf<true, false> { typedef GenSeqArgs type; };
template <>
struct KArgsOf<true, true> { typedef GenArgs type; };
template <bool SEQ, bool GUIDED = false>
using KArgs = typename KArgsOf<SEQ, GUIDED>::type;

// What a step of sequence b samples by: the launch's scalars with row = b (what every kernel did before
// mvn_generate_seq), or, by the kernel argument's type, entry b of a.per_seq.  b is uniform over the wave or
// block that makes the choice, so the loads are uniform; an entry that never passed mvn_seq_sampling_check only
// changes which class is drawn (every consumer keeps its index in [0, Q) whatever the values).
struct SeqSampling {
  float temperature;
  int top_k;
  float top_p;
  uint64_t seed;
  uint32_t row;  // second Philox counter word
};
__device__ __forceinline__ SeqSampling seq_sampling(const GenScalarArgs &a, int b) {
  return {a.temperature, a.top_k, a.top_p, a.seed, (uint32_t)b};
}
__device__ __forceinline__ SeqSampling seq_sampling(const GenSeqArgs &a, int b) {
  const mvn_seq_sampling *s = a.per_seq + b;
  return {s->temperature, s->top_k, s->top_p, s->seed, s->row};
}

__device__ __forceinline__ int ring_offset(int l, int layer_size, int C) {
  const int stack = l / layer_size, pos = l - stack * layer_size;
  return C * (stack * ((1 << layer_size) - 1) + ((1 << pos) - 1));
}

// LDS-only barrier: outstanding global loads (the weight prefetch) stay in
// flight across it.  __syncthreads() would add a full vmcnt(0) drain whenever a
// global store is pending.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__device__ __forceinline__ float ring_load(const float *p) {
  // agent-scope relaxed load: served by L2, never by a stale L1 line
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// full f/g matrix element: row o in [0,2C) (filter | gate), column k in [0,2C)
// (tap 0 = past | tap 1 = current)
__device__ __forceinline__ float fg_elem(const float *fw, const float *gw, int C, int o, int k) {
  const int tap = k >= C, kc = k - tap * C;
  const float *w = o < C ? fw : gw;
  const int oc = o < C ? o : o - C;
  return w[((size_t)oc * C + kc) * 2 + tap];
}
__device__ __forceinline__ float rs_elem(const float *rw, const float *sw, int C, int o, int k) {
  return o < C ? rw[(size_t)o * C + k] : sw[(size_t)(o - C) * C + k];
}


// class counts the 256-wide heads of the tuned generators take (padded at pack time: generate_fold.hip)
inline bool head_q_ok(int q) { return q == 64 || q == 128 || q == 256; }

// ---- one generator kernel as the host sees it ------------------------------------------------
// Everything generate.hip asks about a variant: it walks one table of these (GENERIC and STREAM defined there, the
// pipelined three one each in their own file) and knows no variant by name.  A pipelined variant hands activations
// from stage to stage through one inbox per (sequence, stage) in the state's hand-off area; a one-launch kernel has
// no stages (`stages` and the three members behind it are NULL) and takes any batch.
struct GenVariant {
  int id;            // MVN_GEN_*
  const char *name;  // in messages
  bool (*ok)(const mvn_dims *);                            // the dims it takes
  int (*stages)(const mvn_dims *);                         // per pipeline, as the hand-off area is sized
  size_t (*inbox_floats)(const mvn_dims *);                // per (sequence, stage): the file's GRAN eight-byte granules
  int (*max_batch)(const mvn_dims *);                      // sequences one launch holds on 256 CUs
  int (*launch_pipelines)(const mvn_dims *, int batch);    // pipelines a launch of `batch` sequences runs on
  size_t (*weights_floats)(const mvn_dims *);              // packed blob without the context section
  // `ctx_section`: where the context convs' section goes, NULL for a model without them
  int (*pack)(const mvn_dims *, const mvn_params *, float *packed, float *ctx_section, hipStream_t);
  // `hand`: the hand-off area, `hand_total` floats long, its status word `status_off` floats in (pipelined only)
  int (*launch)(const GenArgs &, const mvn_dims *, int batch, float *hand, size_t hand_total, size_t status_off,
                hipStream_t);
  // mvn_generate_guided: `pairs` pairs, 2 pairs rows (a.per_seq and a.guidance set); NULL: the variant has no guided form.
  // A pipelined variant runs it on `pairs` pipelines of exactly two turns each: at most launch_pipelines(d, any) pairs
  int (*launch_guided)(const GenArgs &, const mvn_dims *, int pairs, float *hand, size_t hand_total,
                       size_t status_off, hipStream_t);
  const char *needs;  // the "does not fit" message: a format with at most one %d, the batch limit for the dims
};
extern const GenVariant PIPE_VARIANT, PIPE_F16_VARIANT, FOLD_VARIANT;

// ---- shared by the three pipelined variants (defined in generate_pipe.hip) ---------------
// One launch of a pipelined generator kernel (KArgs<SEQ>, u64 *hand, unsigned *err, int NS, int nb, int nseq):
// co-residency and capacity check (MVN_ERR_UNSUPPORTED), hand-off area bounds (MVN_ERR_BAD_ARG), the memsets of
// every polled word, then a cooperative launch where available and allowed (pipe_common.h), else an ordinary one.
struct PipeLaunch {
  const void *fn;       // the kernel
  const char *name;     // the variant, for messages
  int NT;               // threads per workgroup
  size_t lds_bytes;     // dynamic LDS
  int NS, GRAN;         // stages per pipeline, granules per inbox
  int slots;            // grid = 8 workgroups (one per XCD) per slot
  int pipes, batch;     // pipelines launched, sequences they serve
  int max_batch, per_pipe;  // the variant's limits: sequences per launch, per pipeline
};
int pipe_launch_common(const PipeLaunch &p, const GenArgs &a, float *hand, size_t hand_floats_total,
                       size_t status_offset_floats, hipStream_t s);
// embedding tables [tap 2][256][C] of a packed blob, C = 64 or 128; classes >= qm (the model's count) are zero
void pack_embed(int C, const float *causal_w, float *dst, int qm, hipStream_t s);
// context section of PIPE and FOLD (one per-layer layout, C = 64 or 128)
int pipe_pack_ctx(const mvn_dims *d, const mvn_params *p, float *ctx_section, hipStream_t s);

}  // namespace mvn
