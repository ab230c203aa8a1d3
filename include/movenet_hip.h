/*
 * movenet_hip.h -- C ABI of the MI355X-native WaveNet decoder path.
 *
 * The reference (cosmicBboy/movenet) is pure Python/PyTorch and has NO native
 * interface; the boundary a drop-in must honour is the Python API of
 * movenet/wavenet.py (WaveNet.forward :158-191, WaveNet.generate :193-239,
 * receptive_fields :125-134).  This header is the C-ABI layer UNDER that API:
 * every entry point below names the reference lines whose arithmetic it
 * replaces.  movenet_amd/_native.py binds it with ctypes; INTEGRATION.md shows
 * the stub a movenet maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (e.g. the PyTorch
 *    caching allocator) unless the parameter is documented as a host array;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); all
 *    work is enqueued on it and nothing synchronises the host;
 *  - functions return MVN_OK (0) or a negative MVN_ERR_* code and never throw;
 *    mvn_last_error() returns a host string for the calling thread;
 *  - one host thread per GPU; no internal threads; no hidden allocations (the
 *    sizing helpers (mvn_*_floats) size the caller-provided workspaces).
 *  - tensors are fp32, layouts are the reference's: audio (B, Q, T) one-hot is
 *    represented by its class indices (B, T) int32; weights arrive in the
 *    reference's state_dict layouts.
 */
#ifndef MOVENET_HIP_H
#define MOVENET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVN_ABI_VERSION 2  /* r4: mvn_upsample_video_backward takes a scratch buffer; new entry points */

#define MVN_OK 0
#define MVN_ERR_BAD_DIMS (-1)      /* unsupported / inconsistent dimensions   */
#define MVN_ERR_BAD_ARG (-2)       /* NULL pointer, negative size, bad range  */
#define MVN_ERR_TOO_SHORT (-3)     /* T < receptive_fields (ValueError in the
                                      reference, movenet/wavenet.py:141-146)  */
#define MVN_ERR_LAUNCH (-4)        /* HIP launch/runtime error                */
#define MVN_ERR_UNSUPPORTED (-5)   /* variant not available for these dims    */

/* movenet/wavenet.py:75-91 constructor arguments (context_in_channels is used
 * by the video encoder only and is not part of the decoder kernels). */
typedef struct mvn_dims {
  int32_t layer_size;        /* dilations 2^0 .. 2^(layer_size-1) per stack  */
  int32_t stack_size;
  int32_t input_channels;    /* Q: mu-law classes                            */
  int32_t residual_channels; /* C                                            */
  int32_t skip_channels;     /* K                                            */
} mvn_dims;

/* Device pointers to the decoder parameters in the reference's own layouts
 * (movenet/modules.py:19-26, :36-43, :52-65, :136-137).  Per-layer members are
 * HOST arrays of n_layers device pointers.  ctx_* may be NULL (audio-only). */
typedef struct mvn_params {
  const float *causal_w;              /* causal_conv.conv.weight (C,Q,2)     */
  const float *const *filter_w;       /* conv_filter.conv.weight (C,C,2)     */
  const float *const *gate_w;         /* conv_gate.conv.weight   (C,C,2)     */
  const float *const *residual_w;     /* conv_residual.weight    (C,C,1)     */
  const float *const *residual_b;     /* conv_residual.bias      (C)         */
  const float *const *skip_w;         /* conv_skip.weight        (K,C,1)     */
  const float *const *skip_b;         /* conv_skip.bias          (K)         */
  const float *const *ctx_filter_w;   /* context_conv_filter.weight (C,C,1)  */
  const float *const *ctx_filter_b;
  const float *const *ctx_gate_w;     /* context_conv_gate.weight (C,C,1)    */
  const float *const *ctx_gate_b;
  const float *head1_w;               /* dense_conv.conv1.weight (Q,K,1)     */
  const float *head1_b;               /* dense_conv.conv1.bias   (Q)         */
  const float *head2_w;               /* dense_conv.conv2.weight (Q,Q,1)     */
  const float *head2_b;               /* dense_conv.conv2.bias   (Q)         */
} mvn_params;

int mvn_abi_version(void);
/* The library's kernel-form switches (MOVENET_HIP_* environment variables; the tests cross-check kernel forms
 * with them) are parsed once per process at first use; this parses them again. */
int mvn_reload_switches(void);
const char *mvn_last_error(void);

/* movenet/wavenet.py:125-134 (receptive_fields) and :136-147
 * (compute_output_size; returns MVN_ERR_TOO_SHORT where the reference raises
 * ValueError). */
int mvn_receptive_fields(const mvn_dims *dims);
int mvn_output_size(const mvn_dims *dims, int t_len);

/* ------------------------------------------------------------------------
 * Autoregressive generation (replaces the loop of movenet/wavenet.py:217-237:
 * window forward -> [probs/T] -> softmax -> multinomial|argmax -> one-hot
 * scatter) by a ring-buffer ("fast WaveNet") formulation that is
 * result-equivalent: each layer keeps the last `dilation`
 * inputs it saw, one generated sample costs one pass over the weights.
 * ------------------------------------------------------------------------ */

/* Kernel variants: GENERIC handles any dims (C,K <= 256, Q <= 1024); STREAM
 * (C=K=64, Q=256) runs one workgroup per sequence and streams the weights from
 * L2 through double-buffered registers; PIPE see below.                        */
#define MVN_GEN_AUTO 0
#define MVN_GEN_GENERIC 1
#define MVN_GEN_STREAM 2
#define MVN_GEN_PIPE 3 /* C=K in {64,128}, Q=256: layer pipeline over ceil(L/4)+1 (C=64)
                          or L+1 (C=128) CUs, weights resident in registers/LDS,
                          activations handed on as 8-byte granules; needs all stages
                          co-resident, at most 32 per XCD: 24 pipelines at config 2, 4 at
                          config 5 (61 stages, two XCDs each); a pipeline serves up to 8
                          (C=64) / 16 (C=128) sequences in turn within one launch: 192 /
                          64 sequences.  Config 5: 73 us per step for 1 .. 64 sequences.   */

#define MVN_GEN_PIPE_F16 4 /* C=K=128, Q=256: the PIPE structure with FP16 OPERANDS and FP32
                              ACCUMULATION (BASELINE configs[4]; precedent: torch.autocast,
                              movenet/trainer.py:124): weights and every product's vector
                              operand rounded to fp16, sums in fp32 (v_mfma_f32_16x16x32_f16 in
                              the layer stages, v_dot2c_f32_f16 in the head); two layers
                              per stage, ceil(L/2)+1 stages (31 for 60 layers: one XCD): 8
                              pipelines per launch, each serving up to 8 sequences in turn (64
                              per launch).  Never chosen by MVN_GEN_AUTO: fp32 is the default.   */

#define MVN_GEN_FOLD 5 /* C=K=64, Q=256: the PIPE structure with the residual 1x1 of layer j folded
                          into the filter/gate matrix of layer j+1 (products formed at pack
                          time): ONE dependent mat-vec + gate per layer instead of two; three
                          layers per stage, ceil(L/3)+1 stages (11 for 30 layers): 16 pipelines
                          inside XCDs + 7 across them, each serving up to 8 sequences in turn
                          within one launch (184 sequences).  Config 2: 14.7 us per step for 16
                          sequences (PIPE: 17.5), 15.4 for 64, 15.9 for 128, 21.1 for 184 (STREAM:
                          79): what MVN_GEN_AUTO runs whenever it holds the batch.              */

/* Resolve MVN_GEN_AUTO for `dims` and `batch` sequences per launch; returns the
 * variant or a negative error.  The packed weight layout depends on the variant:
 * pack and generate must be given the same resolved value. */
int mvn_gen_variant(const mvn_dims *dims, int requested, int batch);

/* Pipelines (workgroup chains with resident weights) a launch of `batch` sequences of the
 * pipelined `variant` (PIPE, PIPE_F16, FOLD) runs on -- its sequences take turns on them,
 * ceil(batch / pipelines) each; 0 for the other variants, negative on bad dims.  FOLD at
 * config 2: `batch` up to 16, 16 up to 80 sequences (whole pipelines inside one XCD: the
 * pipeline's latency bounds the step), 23 beyond (plus seven across XCDs: the step is
 * rounds x the stages' service time there).  For cost models (generation.auto_plan). */
int mvn_gen_launch_pipelines(const mvn_dims *dims, int variant, int batch);

/* 1 when the pipelined generators (MVN_GEN_PIPE / _PIPE_F16 / _FOLD) of this process are launched with
 * hipLaunchCooperativeKernel -- the default: the runtime guarantees the co-residency their hand-offs
 * need -- 0 when with an ordinary launch: a profiler's tool library is attached (rocprofv3: the
 * cooperative queue's tear-down crashes the process at exit under rocprofiler-sdk) or
 * MOVENET_PIPE_COOPERATIVE_LAUNCH=0 asks for it.  Decided once per process. */
int mvn_gen_launch_is_cooperative(void);

/* Size in floats of the packed weight blob / of the generator state (dilation
 * queues, plus the PIPE variant's hand-off area when the dims allow PIPE). */
size_t mvn_gen_weights_floats(const mvn_dims *dims, int variant);
size_t mvn_gen_state_floats(const mvn_dims *dims, int batch);

/* Float offset, inside the state, of the PIPE variant's status word (int32, zero =
 * no hand-off timed out since the state was last zeroed; read it after synchronising
 * the stream); (size_t)-1 when the dims have no PIPE hand-off area. */
size_t mvn_gen_status_offset(const mvn_dims *dims, int batch);

/* state_dict layouts -> the variant's streaming layout (done once per weight
 * update; DESIGN.md "Data layout in HBM"). */
int mvn_gen_pack_weights(const mvn_dims *dims, int variant, const mvn_params *params,
                         float *packed, void *stream);

/* Advance every sequence over the time steps t in [t_begin, t_end).
 *
 *  samples      (batch, sample_stride) int32 class indices.  Step t consumes
 *               samples[b][t] and predicts time t+1; when t+1 >= n_given and
 *               t+1 < n_total the chosen class is written to samples[b][t+1].
 *               Columns < n_given are never written (prompt / teacher forcing).
 *  state        mvn_gen_state_floats() floats; must be zero before t = 0 and is
 *               carried between calls (calls must cover t contiguously from 0).
 *  temperature  > 0: sample from softmax(softmax(logits)/T) (the reference's
 *               double softmax, movenet/wavenet.py:227-231); <= 0: first argmax
 *               of softmax(softmax(logits)) (:233).
 *  seed         Philox4x32-10 key; the draw for (b, t) does not depend on the
 *               launch partition.
 *  logits_out   optional (batch, n_total - logits_t0, Q): raw head output
 *               predicting time u is stored at [b][u - logits_t0] for u >= logits_t0.
 *  choices_out  optional (batch, n_total) int32: the class the model picks for
 *               time u, also where samples[] is teacher-forced (u >= logits_t0).
 *  context_tm   optional local conditioning, see mvn_transpose_context below.
 */
int mvn_generate(const mvn_dims *dims, int variant, const float *packed, float *state,
                 int32_t *samples, int batch, int sample_stride, int n_total, int n_given,
                 int t_begin, int t_end, float temperature, uint64_t seed,
                 float *logits_out, int32_t *choices_out, int logits_t0,
                 const float *context_tm, void *stream);

/* The rule a sampled step (temperature > 0) draws by.  REFERENCE: softmax(softmax(logits)/T), as
 * above -- its second softmax sees inputs in [0, 1], so the draw is close to uniform whatever the
 * logits say.  MODEL: the distribution the network was trained to predict,
 *     p_q = exp((l_q - max l) / T) / sum_j exp((l_j - max l) / T)
 * over the step's raw fp32 head logits l.  Both draw by the same inverse CDF on the same Philox
 * uniform of (seed, time, sequence): the smallest class q with sum_{j<=q} p_j > uniform * total,
 * Q - 1 if none qualifies.  Padding classes of a 256-wide head (logit -inf) get probability 0. */
#define MVN_SAMPLE_REFERENCE 0
#define MVN_SAMPLE_MODEL 1

/* mvn_generate with the sampling rule chosen: `sampling` is MVN_SAMPLE_REFERENCE (what mvn_generate
 * passes) or MVN_SAMPLE_MODEL; any other value is MVN_ERR_BAD_ARG, before any launch.  The rule
 * changes only the choice of a sampled step: temperature <= 0 is the same greedy arg-max under
 * both, and logits_out, the state and the network arithmetic do not depend on it. */
int mvn_generate_ex(const mvn_dims *dims, int variant, const float *packed, float *state,
                    int32_t *samples, int batch, int sample_stride, int n_total, int n_given,
                    int t_begin, int t_end, float temperature, uint64_t seed,
                    float *logits_out, int32_t *choices_out, int logits_t0,
                    const float *context_tm, int sampling, void *stream);

/* mvn_generate_ex with top-k and top-p (nucleus) truncation of a sampled step; mvn_generate_ex passes
 * (0, 1.0f): both off.  A sampled step (temperature > 0) forms fp32 weights w_q >= 0 over the Q classes,
 * not necessarily normalised -- MODEL: exp((l_q - max l) / T); REFERENCE: the double softmax.
 * Truncation sets some of them to zero before the unchanged inverse-CDF draw on the unchanged Philox
 * uniform of (seed, time, sequence):
 *  1. top_k = k >= 0.  0: off; k >= Q: the same as off.  theta_k is the k-th largest value of w,
 *     counted with multiplicity over the Q real classes; class q is kept iff w_q >= theta_k.  Exact
 *     ties at the threshold are all kept.  "Kept" is a statement about the fp32 weights: where fewer
 *     than k of them are positive (small T: the others underflowed to +0), theta_k is +0 and every
 *     class is kept -- those of weight zero without effect, since a class of weight zero is never
 *     drawn, kept or not (3.).
 *  2. top_p = p in (0, 1].  1.0: off.  Applied after top-k: with S the sum of the weights top-k kept,
 *     theta_p is the largest weight value v for which the sum of the kept weights >= v reaches p * S;
 *     class q is kept iff w_q >= max(theta_k, theta_p).  The largest weight always survives, so the
 *     kept set is never empty.
 *  3. The draw: the smallest class q whose running sum over the truncated weights exceeds
 *     uniform * total_kept.  If rounding lets no class qualify, the highest-indexed kept class --
 *     never a dropped one.  A truncated draw never returns a class whose fp32 weight is zero unless
 *     it is that fallback.
 *  4. With both off, mvn_generate_ex's behaviour to the bit (the Q - 1 fallback included).  Greedy
 *     steps (temperature <= 0) ignore both knobs.  Truncation applies under either rule: it acts on
 *     whatever weights the step draws from.  logits_out, the state and the network arithmetic never
 *     depend on the knobs.
 * The thresholds are exact for the fp32 weights (a radix select on their bit patterns: no sort, no
 * tolerance); the sums of 2. are fp32 sums.
 * top_k < 0, or top_p outside (0, 1] (NaN included): MVN_ERR_BAD_ARG with a mvn_last_error() text,
 * before any launch and before any buffer is touched. */
int mvn_generate_trunc(const mvn_dims *dims, int variant, const float *packed, float *state,
                       int32_t *samples, int batch, int sample_stride, int n_total, int n_given,
                       int t_begin, int t_end, float temperature, uint64_t seed,
                       float *logits_out, int32_t *choices_out, int logits_t0,
                       const float *context_tm, int sampling, int top_k, float top_p, void *stream);

/* Per-sequence sampling settings: what mvn_generate_trunc takes once per launch (temperature, seed,
 * top_k, top_p), once per SEQUENCE of the launch -- a sweep over settings on one prompt is one launch
 * instead of one per setting, and a sequence's draws depend on its own (seed, row) alone: not on its
 * position in the batch, nor on how a caller splits a batch into launches. */
typedef struct mvn_seq_sampling { /* 24 bytes, one per sequence of the launch */
  float temperature;              /* <= 0 (or NaN): this sequence decodes greedily */
  int32_t top_k;                  /* 0: off */
  float top_p;                    /* 1.0: off */
  uint32_t row;                   /* second Philox counter word of this sequence (what `b` is on the scalar path) */
  uint64_t seed;                  /* Philox key of this sequence */
} mvn_seq_sampling;

/* Host-only validator and normaliser of `batch` entries in HOST memory for a model of `classes` classes;
 * touches no GPU.  The rules of mvn_generate_trunc's scalars, row by row: top_k < 0, or top_p outside
 * (0, 1] (NaN included), is MVN_ERR_BAD_ARG with a mvn_last_error() text that names the first offending
 * row, and nothing is modified; otherwise every top_k >= classes becomes 0 in place, so that "off" is off
 * to the bit.  temperature, row and seed take any value. */
int mvn_seq_sampling_check(mvn_seq_sampling *host, int batch, int classes);

/* mvn_generate_trunc with the four settings per sequence: `per_seq` is a DEVICE array of `batch` entries
 * that has passed mvn_seq_sampling_check (NULL: MVN_ERR_BAD_ARG); it is read by the kernel, so it must stay
 * unchanged until the launch has run.  `sampling` (the rule) stays one value per call.
 * The step of sequence b that predicts time u does exactly what mvn_generate_trunc does with per_seq[b]'s
 * temperature, top_k and top_p, on the uniform philox_uniform(per_seq[b].seed, u, per_seq[b].row): with
 * every entry (T, k, p, seed, row = b) the call is mvn_generate_trunc(T, seed, k, p) to the bit -- samples,
 * logits_out and choices_out.  Greedy and sampled sequences may share a launch.  In the pipelined variants
 * a pipeline serves several sequences in turn: the settings follow the sequence.
 * Entries that never passed the check cause no out-of-range access; which class they draw is unspecified. */
int mvn_generate_seq(const mvn_dims *dims, int variant, const float *packed, float *state,
                     int32_t *samples, int batch, int sample_stride, int n_total, int n_given,
                     int t_begin, int t_end, const mvn_seq_sampling *per_seq,
                     float *logits_out, int32_t *choices_out, int logits_t0,
                     const float *context_tm, int sampling, void *stream);

/* Classifier-free guidance.  A guided launch holds `pairs` pairs = 2 * pairs rows of
 * samples, state (that of batch = 2 * pairs: mvn_gen_state_floats), per_seq, logits_out, choices_out and
 * context_tm: rows [0, pairs) are the UNCONDITIONAL rows, rows [pairs, 2 * pairs) the CONDITIONAL ones, and pair p
 * is rows p and p + pairs.  The caller gives both rows of a pair the same prompt; they differ only in their
 * context_tm rows (video, or zeros, against the same plus the label's vector).
 * The step of pair p that predicts time u forms, over the raw fp32 head logits l_u, l_c of its two rows,
 *     l[q] = l_c[q] + (guidance[p] - 1) * (l_c[q] - l_u[q])        for q < Q
 * in fp32 in exactly this order -- subtract, multiply, add, nothing fused -- so a scale of 1 gives l_c to the
 * bit.  Padding classes q >= Q of a 256-wide head keep their -inf (the formula is not applied to them).  The
 * guided logits then go through the unchanged choice of mvn_generate_seq with the settings of the CONDITIONAL
 * row's entry, per_seq[p + pairs] (temperature, top_k, top_p, seed, row), under `sampling`; a greedy step takes
 * the arg-max of the guided logits by the same greedy rule.  The pick is written to samples[u] (u >= n_given)
 * and to choices_out of BOTH rows, and both rows consume it at the next step.  Columns u < n_given (prompt /
 * teacher forcing) must hold the same in both rows of a pair.  Where a caller breaks that contract the result is
 * defined per variant: MVN_GEN_GENERIC consumes each row's own column, the pipelined variants (PIPE, PIPE_F16,
 * FOLD) keep one pair of indices per pair and feed both rows the conditional row's column.  logits_out rows stay each row's own raw logits; the state and the network arithmetic never depend on
 * the scales.  Chunked launches (t_begin / t_end) carry state as those of mvn_generate do.
 *
 * mvn_gen_guided_max_pairs: host-only arithmetic -- the pairs one guided launch of `variant` takes for `dims`;
 * 0: the variant has no guided form (MVN_GEN_STREAM) or does not take the dims; negative on bad dims.  A
 * pipelined variant serves pair p on pipeline p in two consecutive turns (unconditional row first), so its limit
 * is its pipeline count for the dims (FOLD at config 2: 23); MVN_GEN_GENERIC runs one workgroup per pair and
 * returns 0x3FFFFFFF.
 *
 * Refused before any launch and before any buffer is touched: per_seq or guidance NULL, or pairs < 1:
 * MVN_ERR_BAD_ARG; pairs above the limit, or a variant without a guided form: MVN_ERR_UNSUPPORTED with a
 * mvn_last_error() text that names the limit.  `per_seq` (2 * pairs entries that have passed
 * mvn_seq_sampling_check) and `guidance` (pairs floats) are DEVICE arrays the host cannot validate: a
 * non-finite scale only changes which class is drawn and never causes an out-of-range access (every consumer
 * of a pick clamps it to [0, Q)). */
int mvn_gen_guided_max_pairs(const mvn_dims *dims, int variant);
int mvn_generate_guided(const mvn_dims *dims, int variant, const float *packed, float *state,
                        int32_t *samples, int pairs, int sample_stride, int n_total, int n_given,
                        int t_begin, int t_end, const mvn_seq_sampling *per_seq, const float *guidance,
                        float *logits_out, int32_t *choices_out, int logits_t0,
                        const float *context_tm, int sampling, void *stream);

/* Local conditioning in generation (BUILD DEFINITION, the reference raises: SURVEY.md
 * Q7): step t adds the context column of time t to every layer's filter/gate sums.
 * context_tm is (batch, n_total, C) TIME-major (one coalesced 4C-byte read per step);
 * mvn_transpose_context builds it from the (batch, C, ctx_ld) output of
 * mvn_upsample_video.  GENERIC and PIPE variants only. */
int mvn_transpose_context(const float *ctx, int ctx_ld, int batch, int channels, int t_len,
                          float *context_tm, void *stream);

/* A launch whose local conditioning arrives as a WINDOW of the time-major context (additive, ABI version unchanged;
 * DESIGN.md section 4.1g).  The one general call: the parameters of mvn_generate_trunc, mvn_generate_seq and
 * mvn_generate_guided together, and in place of context_tm
 *   context_win  DEVICE (rows, ctx_len, C) fp32, time-major: columns [ctx_t0, ctx_t0 + ctx_len) of every row's context,
 *                rows = batch (guided: 2 * batch, unconditional rows first), a row ctx_len * C floats from the next
 *   ctx_t0, ctx_len  the first column the buffer holds and how many
 *   per_seq      NULL: temperature, seed, top_k and top_p hold for every sequence (mvn_generate_trunc); a DEVICE array:
 *                mvn_generate_seq's, and the four scalars are not read
 *   guidance     NULL, or mvn_generate_guided's DEVICE scales; `batch` then counts PAIRS and per_seq is required
 * Which context columns a launch over [t_begin, t_end) reads, by variant, as the kernels have it:
 *   MVN_GEN_GENERIC, MVN_GEN_STREAM          column t in the step t it runs: exactly [t_begin, t_end)
 *   MVN_GEN_PIPE, MVN_GEN_PIPE_F16, MVN_GEN_FOLD  column t_begin in the prologue, column t + 1 during step t while
 *                                            t + 1 < t_end (the look-ahead stops at the launch's end): exactly
 *                                            [t_begin, t_end)
 * and no element of context_win outside those columns is read, whatever it holds.  With ctx_t0 = 0, ctx_len = n_total
 * and the whole context_tm the call is the matching one of the three to the bit.
 * MVN_ERR_BAD_ARG with a mvn_last_error() text that names both column ranges: context_win NULL, ctx_len < 1,
 * ctx_t0 < 0, or [t_begin, t_end) not inside [ctx_t0, ctx_t0 + ctx_len) (an empty launch lies inside any window).
 * Otherwise everything mvn_generate_guided (where guidance is given) and then mvn_generate_seq / mvn_generate_trunc
 * refuse, in their order.  Every refusal comes before any launch and before any buffer is touched. */
int mvn_generate_windowed(const mvn_dims *dims, int variant, const float *packed, float *state, int32_t *samples,
                          int batch, int sample_stride, int n_total, int n_given, int t_begin, int t_end,
                          float temperature, uint64_t seed, int top_k, float top_p, const mvn_seq_sampling *per_seq,
                          const float *guidance, float *logits_out, int32_t *choices_out, int logits_t0,
                          const float *context_win, int ctx_t0, int ctx_len, int sampling, void *stream);

/* ------------------------------------------------------------------------
 * Full-sequence forward (replaces movenet/wavenet.py:166-191: causal conv ->
 * L gated residual layers -> sum of skips -> dense head -> [drop last] ->
 * [softmax]) and its backward.  Used for training, for forward() and to prime
 * the generator's queues from a prompt.
 *
 * Activations live on an ABSOLUTE time axis: every per-layer tensor is
 * (batch, channels, Tp) with Tp = mvn_padded_len(T) and column t = input time
 * t; layer l's input is valid for t >= A_l (A_0 = 0, A_{l+1} = A_l + d_l), so
 * the reference's right-aligned slices (modules.py:84, :91) become "same t".
 * Skip/head tensors are (batch, channels, Sp), Sp = mvn_padded_len(S + 31),
 * S = T - RF + 1; the column of time t is t - ((RF-1) & ~31), i.e. the S valid
 * columns start at column (RF-1) & 31, so that column == t (mod 32): 16-byte
 * accesses and the 128-byte cache lines line up on both time axes.
 * ------------------------------------------------------------------------ */
int mvn_padded_len(int n); /* n rounded up to a multiple of 64 */

/* Caller-provided device buffers (floats).  n_act = save ? L+1 : 2. */
typedef struct mvn_fwd_buffers {
  float *acts;  /* n_act x (B, C, Tp): layer inputs; acts[0] = causal conv out;
                   save: plane L (the last layer's residual output, which nothing
                   uses) is never written                                       */
  float *th;    /* save: L x (B, C, Tp) tanh(f);      else NULL                 */
  float *sg;    /* save: L x (B, C, Tp) sigmoid(g);   else NULL                 */
  float *z;     /* (B, C, Tp) scratch: the gated activation of the unfused layer
                   kernels; the fused paths keep z on chip and write the layers'
                   packed weight images here (fused_fwd_bf3.h).  SHARED by the two
                   passes: mvn_backward stages images (and, in bf16, slabs) of its
                   own in it, so its contents are undefined after either call; every
                   other saved tensor is left bit-identical by mvn_backward, which
                   may therefore run again over the same saved forward           */
  float *skip;  /* (B, K, Sp) sum of skips                                      */
  float *a1;    /* (B, Q, Sp) head hidden activation lrelu(conv1(lrelu(skip)))  */
  const float *ctx; /* optional local conditioning (B, C, ctx_ld), column t = time t
                       (output of mvn_upsample_video); NULL = audio only.  BUILD
                       DEFINITION of the alignment: the reference raises at
                       modules.py:75-77                          */
  int32_t ctx_ld;
  const float *dense_audio; /* optional (B, Q, dense_ld) fp32 input that is NOT one-hot: the
                               causal conv then runs as a dense product and `index` is
                               ignored (may be NULL); NULL = use `index`                */
  int32_t dense_ld;
} mvn_fwd_buffers;

/* out: (B, Q, S_out) contiguous, S_out = S - (remove_last ? 1 : 0); softmax over
 * Q when `normalize` (the reference's inverted flag output_unnormalized=True,
 * wavenet.py:189-191); written in full, its rows need no alignment (any S_out); may be
 * NULL when S_out == 0.  save != 0 keeps what mvn_backward needs in `buf`.
 * No buffer has to be initialised: the library reads only what it (or the caller, for the
 * inputs' columns < t_len) has written.  Every argument is checked before the first launch:
 * a call that returns MVN_ERR_BAD_ARG / _BAD_DIMS / _TOO_SHORT / _UNSUPPORTED has written
 * nothing.
 * index: class of step t of sequence b at index[b * index_stride + t], t < t_len.  A class outside
 * [0, input_channels) is not an error: it is taken as the nearest end (negative -> 0, too large ->
 * input_channels - 1), by this call and its siblings and IDENTICALLY by mvn_backward and its siblings,
 * so the embedding gradient of such a step goes to the table row the forward read. */
int mvn_forward(const mvn_dims *dims, const mvn_params *params, const int32_t *index,
                int index_stride, int batch, int t_len, const mvn_fwd_buffers *buf, float *out,
                int normalize, int remove_last, int save, void *stream);

/* mvn_forward with FP16 OPERANDS and FP32 ACCUMULATION in every product of the layers and
 * the head (BASELINE configs[4] "fp16 MFMA 1x1 convs"; reference precedent for reduced
 * precision: torch.autocast, movenet/trainer.py:124): weights and the activations entering a
 * product are rounded to fp16 as they are staged, multiplied by v_mfma_f32_32x32x16_f16 and
 * summed in fp32; the causal conv's gather, biases, gating, residual adds, the skip sum, the
 * softmax and every tensor in HBM stay fp32 -- the rounding points of MVN_GEN_PIPE_F16.  Same
 * arguments and buffers as mvn_forward; `save` keeps th/sg/acts, but mvn_backward
 * differentiates the fp32 forward: train in fp32 (the default). */
int mvn_forward_f16(const mvn_dims *dims, const mvn_params *params, const int32_t *index,
                    int index_stride, int batch, int t_len, const mvn_fwd_buffers *buf, float *out,
                    int normalize, int remove_last, int save, void *stream);

/* mvn_forward with BF16 OPERANDS and FP32 ACCUMULATION in the products of the gated layers (opt-in
 * mixed-precision training; the reference trains under torch.autocast, movenet/trainer.py:124):
 * x(t), x(t - d), z = tanh sigmoid and the four weight tensors of each layer are rounded to bf16
 * (round to nearest even) as they are staged and multiplied by ONE v_mfma_f32_32x32x16_bf16 per
 * block; the embedding / causal conv, biases, gating, residual adds, the skip sum, the head, the
 * softmax and every tensor in HBM stay fp32.  Same arguments and buffers as mvn_forward; `save`
 * keeps what mvn_backward_bf16 differentiates.  Audio-only, residual_channels = skip_channels = 64,
 * any input_channels; anything else (or a context) returns MVN_ERR_UNSUPPORTED and launches nothing. */
int mvn_forward_bf16(const mvn_dims *dims, const mvn_params *params, const int32_t *index,
                     int index_stride, int batch, int t_len, const mvn_fwd_buffers *buf, float *out,
                     int normalize, int remove_last, int save, void *stream);

/* Gradients, same layouts as mvn_params (members may not be NULL except ctx_*);
 * mvn_backward ACCUMULATES into them (zero them first for a fresh gradient). */
typedef struct mvn_param_grads {
  float *causal_w;
  float *const *filter_w;
  float *const *gate_w;
  float *const *residual_w;
  float *const *residual_b;
  float *const *skip_w;
  float *const *skip_b;
  float *head1_w;
  float *head1_b;
  float *head2_w;
  float *head2_b;
  float *const *ctx_filter_w; /* only used (and required) when fwd->ctx != NULL */
  float *const *ctx_filter_b;
  float *const *ctx_gate_w;
  float *const *ctx_gate_b;
} mvn_param_grads;

/* Scratch for the backward pass (floats). */
typedef struct mvn_bwd_buffers {
  float *dx_a;   /* (B, C, Tp) */
  float *dx_b;   /* (B, C, Tp) */
  float *dfg;    /* (B, 2C, Tp) */
  float *dskip;  /* (B, K, Sp) */
  float *da1;    /* (B, Q, Sp) */
  float *dlogit; /* (B, Q, Sp) */
  float *dctx;   /* (B, C, Tp) gradient w.r.t. fwd->ctx, written in full (not accumulated):
                    columns >= t_len are zero; NULL when audio only */
} mvn_bwd_buffers;

/* dout: gradient w.r.t. mvn_forward's `out` (same shape); `out` itself is needed
 * when normalize != 0 (softmax backward).  dout == NULL: the caller has already written the
 * gradient w.r.t. the LOGITS into bwd->dlogit (layout (B, Q, Sp), the column of output
 * position s is s + ((RF-1) & 31), columns of positions >= S_out zero) -- what
 * mvn_softmax_ce_backward does.  Requires the forward ran with save.
 * Part of the work is enqueued on a stream the library owns (one per device) and joined
 * back into `stream` with events before the call returns: to the caller it is ordinary
 * stream-ordered work.  da1 / dlogit / dfg double as scratch of the weight gradients, and so
 * does fwd->z.  index_stride / dense_ld / ctx_ld are checked as in mvn_forward.  S_out == 0
 * (t_len == RF with remove_last): MVN_OK, nothing is launched, `out` / `dout` may be NULL.
 * Every refusal of mvn_backward and its siblings below is decided in front of the first launch -- also the
 * ones that depend on the scratch sizes (buffers the bf16 / one-kernel layer backward cannot run, a context
 * pass whose slabs do not fit at some layer, input_channels > 8192 without dense audio): a refused call has
 * written nothing and leaves mvn_last_backward_form() and mvn_last_embed_form() as they were.
 * index: as in mvn_forward -- a class outside [0, input_channels) is taken as the nearest end, identically in
 * both passes (every form of the embedding gradient clamps as the forward's gather does). */
int mvn_backward(const mvn_dims *dims, const mvn_params *params, const mvn_param_grads *grads,
                 const int32_t *index, int index_stride, int batch, int t_len,
                 const mvn_fwd_buffers *fwd, const mvn_bwd_buffers *bwd, const float *out,
                 const float *dout, int normalize, int remove_last, void *stream);

/* The backward of mvn_forward_bf16: mvn_backward's arguments and buffers, with the layers' products on
 * bf16 operands (dxo, dskip and the weights in the dz / input-gradient products; df | dg, x and z in
 * the weight-gradient products) and fp32 accumulation; the head, the embedding gradient and every
 * buffer stay fp32.  Same dims as mvn_forward_bf16; a batch / length whose scratch the bf16 layer
 * kernel cannot place returns MVN_ERR_UNSUPPORTED before anything is launched -- every refusal does (the note at
 * mvn_backward): also "cannot run these buffers", which used to follow the head's backward. */
int mvn_backward_bf16(const mvn_dims *dims, const mvn_params *params, const mvn_param_grads *grads,
                      const int32_t *index, int index_stride, int batch, int t_len,
                      const mvn_fwd_buffers *fwd, const mvn_bwd_buffers *bwd, const float *out,
                      const float *dout, int normalize, int remove_last, void *stream);

/* Diagnostic: which form the layer loop of the process's last mvn_backward took -- 0 none yet,
 * 1 the generic two-kernel forms (any dims), 2 the two fused halves per layer (C = K = 64,
 * csrc/fused_bwd.h), 3 ONE kernel per layer with the input gradient in scatter form
 * (csrc/fused_bwd_l.h, the default at C = K = 64), 4 the bf16 layer kernel of mvn_backward_bf16
 * (csrc/fused_bf16.h), 5 and 6 forms 3 and 4 with the label's row sums.  Tests assert on it so that a silent
 * fall-back to a slower form cannot pass for the fast one. */
#define MVN_BWD_FORM_GENERIC 1
#define MVN_BWD_FORM_HALVES 2
#define MVN_BWD_FORM_ONE 3
#define MVN_BWD_FORM_BF16 4
#define MVN_BWD_FORM_ONE_GLOBAL 5 /* form 3 with the label's row sums: mvn_backward_global */
#define MVN_BWD_FORM_BF16_GLOBAL 6 /* form 4 with the label's row sums: mvn_backward_bf16_global */
int mvn_last_backward_form(void);

/* Diagnostic: which form the embedding gradient (the causal conv's weight gradient) of the process's last
 * mvn_backward or sibling took -- 0 none yet, 1 the dense product (fwd->dense_audio given), 2 the product on the
 * matrix cores (C = 64, Q = 256), 3 the LDS read-modify-write kernel (C = 64, Q < 256), 4 one table copy per
 * (chunk, sequence) summed in chunk order, 5 global atomics.  Forms 2 to 4 need room for their per-chunk tables in
 * the backward's scratch; a call without that room (or, for form 4, with a table that is no multiple of 64 floats)
 * takes form 5.  Forms 2 to 4 add every table word's steps and copies in a fixed order and give the same bits
 * whenever they run; form 5 adds to the table with global atomics, so its last bits vary from run to run.
 * Tests assert on it for the reason given at mvn_last_backward_form; a refused call leaves it as it was. */
#define MVN_EMBED_FORM_DENSE 1
#define MVN_EMBED_FORM_MFMA 2
#define MVN_EMBED_FORM_LDS 3
#define MVN_EMBED_FORM_TABLES 4
#define MVN_EMBED_FORM_ATOMICS 5
int mvn_last_embed_form(void);

/* ------------------------------------------------------------------------
 * Global conditioning on a class label (BUILD DEFINITION): sequence b carries a
 * C-vector e_b that enters every gated layer where local context does, as a column constant in time:
 *     f_l(b, :, t) += Wcf_l (ctx(b, :, t) + e_b) + bcf_l      (the same for g_l with Wcg_l, bcg_l)
 * General path (any dims, with or without video): add e_b to the context and run the conditioned
 * entry points.  For the generators mvn_context_add_global adds global (batch, channels) to every
 * time row of the (batch, t_len, channels) time-major context_tm; fill != 0 writes the rows
 * instead (no video: the buffer need not be initialised).
 * ------------------------------------------------------------------------ */
int mvn_context_add_global(float *context_tm, const float *global, int batch, int channels, int t_len,
                           int fill, void *stream);

/* Fast path: residual_channels = skip_channels = 64, fp32, no video.  The label's term of a layer
 * is ONE 2C-vector per sequence, so no layer runs a context product:
 *   mvn_global_bias           gbias (L, batch, 128) = [Wcf_l e_b + bcf_l | Wcg_l e_b + bcg_l], e (batch, 64)
 *   mvn_forward_global        mvn_forward with buf->ctx == NULL; the layers add gbias[l][b] to their
 *                             filter / gate pre-activations in front of tanh / sigmoid
 *   mvn_backward_global       mvn_backward for such a forward.  scratch: mvn_global_scratch_floats() floats
 *                             (the layer kernel's second pair of gradient tensors, its weight-gradient
 *                             slabs and bias partials; scratch_floats says how many there are);
 *                             rowsum (L, batch, 128) receives sum_t (df | dg)(b, :, t) of every layer
 *                             (zero it first: a call without output columns launches nothing)
 *   mvn_global_bias_backward  grads->ctx_filter_w / _b / ctx_gate_w / _b of every layer are WRITTEN with
 *                             sum_b rowsum (x) e_b and sum_b rowsum; de (batch, 64) = sum_l Wcf_l^T r_f +
 *                             Wcg_l^T r_g
 * General path: mvn_backward_scratch is mvn_backward (same arguments, same results, fwd->ctx the context
 * the label has joined) with the conditioned layers' one-kernel form taking its second pair of gradient
 * tensors, slabs and bias partials from `scratch` (mvn_global_scratch_floats() floats) instead of dlogit /
 * da1, which are too small for them at short outputs and small Q: MVN_BWD_FORM_ONE wherever the switches
 * allow it.  Without a context, or with a scratch too small, it is mvn_backward.
 * mvn_global_fast_path: 1 when mvn_forward_global and mvn_backward_global run this batch / length
 * under the process's MOVENET_HIP_* switches, else 0 (take the general path); the two refuse with
 * MVN_ERR_UNSUPPORTED, before anything is launched, exactly where it returns 0.  So does every other refusal of
 * mvn_backward_global and mvn_backward_scratch (the note at mvn_backward): buffers the one-kernel layer backward
 * cannot run, or a context pass that finds no room at some layer, no longer come after the head's backward.
 * mvn_last_backward_form() reports MVN_BWD_FORM_ONE_GLOBAL after mvn_backward_global. */
int mvn_global_fast_path(const mvn_dims *dims, int batch, int t_len);
int mvn_global_bias(const mvn_dims *dims, const mvn_params *params, const float *e, int batch,
                    float *gbias, void *stream);
int mvn_forward_global(const mvn_dims *dims, const mvn_params *params, const int32_t *index,
                       int index_stride, int batch, int t_len, const mvn_fwd_buffers *buf, float *out,
                       int normalize, int remove_last, int save, const float *gbias, void *stream);
int mvn_backward_global(const mvn_dims *dims, const mvn_params *params, const mvn_param_grads *grads,
                        const int32_t *index, int index_stride, int batch, int t_len,
                        const mvn_fwd_buffers *fwd, const mvn_bwd_buffers *bwd, const float *out,
                        const float *dout, int normalize, int remove_last, float *scratch,
                        size_t scratch_floats, float *rowsum, void *stream);
int mvn_backward_scratch(const mvn_dims *dims, const mvn_params *params, const mvn_param_grads *grads,
                         const int32_t *index, int index_stride, int batch, int t_len,
                         const mvn_fwd_buffers *fwd, const mvn_bwd_buffers *bwd, const float *out,
                         const float *dout, int normalize, int remove_last, float *scratch,
                         size_t scratch_floats, void *stream);
size_t mvn_global_scratch_floats(const mvn_dims *dims, int batch, int t_len);
int mvn_global_bias_backward(const mvn_dims *dims, const mvn_params *params,
                             const mvn_param_grads *grads, const float *rowsum, const float *e,
                             int batch, float *de, void *stream);

/* The fast path on bf16 operands (csrc/fused_bf16.h): mvn_forward_bf16 / mvn_backward_bf16 with the
 * label's term.  gbias is mvn_global_bias's, fp32 and never rounded: the layers' filter / gate
 * accumulators start from gbias[l][b] instead of zero.  The backward's layer kernel sums the rows of
 * its fp32 df | dg itself (no dfg tensor is written): rowsum (L, batch, 128) receives
 * sum_t (df | dg)(b, :, t) of every layer, for mvn_global_bias_backward (zero it first: a call without
 * output columns launches nothing).  scratch: mvn_global_bf16_scratch_floats() floats -- the layer
 * kernel's weight-gradient slabs, bias partials and row-sum partials, so that short outputs and small
 * Q run too.  Every sum runs in a fixed order: two calls give the same bits.
 * Refused before anything is launched or written: MVN_ERR_UNSUPPORTED for residual_channels or
 * skip_channels != 64, for buf->ctx / fwd->ctx != NULL and for a batch / length the bf16 layer kernels
 * cannot place (mvn_global_bf16_path returns 0 exactly there, 1 elsewhere; it consults no switch);
 * MVN_ERR_BAD_ARG for a NULL gbias / scratch / rowsum or scratch_floats below
 * mvn_global_bf16_scratch_floats().  "Before anything is launched" holds for every refusal of the backward (the
 * note at mvn_backward).  mvn_last_backward_form() reports MVN_BWD_FORM_BF16_GLOBAL. */
int mvn_global_bf16_path(const mvn_dims *dims, int batch, int t_len);
size_t mvn_global_bf16_scratch_floats(const mvn_dims *dims, int batch, int t_len);
int mvn_forward_bf16_global(const mvn_dims *dims, const mvn_params *params, const int32_t *index,
                            int index_stride, int batch, int t_len, const mvn_fwd_buffers *buf,
                            float *out, int normalize, int remove_last, int save, const float *gbias,
                            void *stream);
int mvn_backward_bf16_global(const mvn_dims *dims, const mvn_params *params,
                             const mvn_param_grads *grads, const int32_t *index, int index_stride,
                             int batch, int t_len, const mvn_fwd_buffers *fwd,
                             const mvn_bwd_buffers *bwd, const float *out, const float *dout,
                             int normalize, int remove_last, float *scratch, size_t scratch_floats,
                             float *rowsum, void *stream);

/* Video context on bf16 operands (csrc/fused_bf16.h): mvn_forward_bf16 / mvn_backward_bf16 for conditioned layers,
 * buf->ctx / fwd->ctx the (B, 64, ctx_ld) context as in mvn_forward.  Forward: f | g is ONE contraction over K = 192,
 * bf(W_fg) bf([x(t - d); x(t)]) + bf([Wcf; Wcg]) bf(ctx(t)), in fp32 accumulators that start from bcf | bcg (fp32, never
 * rounded); ctx and the context weights are rounded once as they are staged.  Backward: the layer kernel's arithmetic is
 * mvn_backward_bf16's (the context term does not enter dx); its fp32 df | dg tile also goes to bwd->dfg, from which the
 * context pass of mvn_backward forms dctx, the context-conv weight and bias gradients in fp32 from the unrounded dfg,
 * ctx and weights.  Where mvn_backward_bf16 runs a shape, the layer pass cuts each sequence into the same chunks: zero
 * context weights and biases give its logits and gradients to the bit.
 * scratch: mvn_bf16_ctx_scratch_floats() floats (the layer kernel's second pair of gradient tensors, the two passes'
 * slabs and bias partials: dlogit / da1 / fwd->z are too small for them at short outputs and small Q).
 * Refused before anything is launched or written: MVN_ERR_UNSUPPORTED for residual_channels or skip_channels != 64,
 * rows (t_len, ctx_ld) beyond 2^21 and a batch / length the kernels cannot place (mvn_bf16_ctx_path returns 0 exactly
 * there, for any ctx_ld <= 2^21; it consults no switch); MVN_ERR_BAD_ARG for no ctx, no dctx, no dfg, no context-conv
 * parameters or gradients, ctx_ld < t_len, no scratch or one below mvn_bf16_ctx_scratch_floats(); the same holds for
 * slabs that do not fit the scratch in either pass (MVN_ERR_UNSUPPORTED; the note at mvn_backward).
 * mvn_last_backward_form() reports MVN_BWD_FORM_BF16_CTX.  mvn_forward_bf16, mvn_backward_bf16 and the _global pair keep
 * refusing a context. */
#define MVN_BWD_FORM_BF16_CTX 7 /* form 4 for conditioned layers: mvn_backward_bf16_ctx */
int mvn_bf16_ctx_path(const mvn_dims *dims, int batch, int t_len);
size_t mvn_bf16_ctx_scratch_floats(const mvn_dims *dims, int batch, int t_len);
int mvn_forward_bf16_ctx(const mvn_dims *dims, const mvn_params *params, const int32_t *index,
                         int index_stride, int batch, int t_len, const mvn_fwd_buffers *buf, float *out,
                         int normalize, int remove_last, int save, void *stream);
int mvn_backward_bf16_ctx(const mvn_dims *dims, const mvn_params *params, const mvn_param_grads *grads,
                          const int32_t *index, int index_stride, int batch, int t_len,
                          const mvn_fwd_buffers *fwd, const mvn_bwd_buffers *bwd, const float *out,
                          const float *dout, int normalize, int remove_last, float *scratch,
                          size_t scratch_floats, void *stream);

/* ------------------------------------------------------------------------
 * Local conditioning: video encoder + learned upsampler (movenet/wavenet.py:94-118,
 * :149-156).  video (B, F, 64, 64, Cin) fp32 -> Conv3d(k=(1,64,64)) -> (B, C, F)
 * -> 3 x ConvTranspose1d(k=10, stride=10) -> ctx (B, C, 1000 F).
 * Intermediates are caller-provided (B, C, mvn_padded_len(n)) buffers with
 * n = F, 10 F, 100 F; ctx has row stride ctx_ld >= 1000 F.
 * ------------------------------------------------------------------------ */
typedef struct mvn_video_params {
  const float *conv_w;   /* video_conv.weight (C, Cin, 1, 64, 64) */
  const float *conv_b;   /* video_conv.bias   (C)                 */
  const float *up_w[3];  /* video_transpose.{0,1,2}.weight (C, C, 10) = (in, out, tap) */
  const float *up_b[3];  /* video_transpose.{0,1,2}.bias   (C)    */
} mvn_video_params;

typedef struct mvn_video_grads { /* accumulated into */
  float *conv_w;
  float *conv_b;
  float *up_w[3];
  float *up_b[3];
} mvn_video_grads;

int mvn_upsample_video(const mvn_dims *dims, const mvn_video_params *vp, const float *video,
                       int batch, int frames, int cin, float *enc, float *u1, float *u2, float *ctx,
                       int ctx_ld, void *stream);

/* d_u2, d_u1, d_enc: scratch of the same shapes as u2, u1, enc.  `scratch` (r4): room for the per-workgroup
 * weight-gradient slabs of the up-sampler's backward kernel (C = 64), mvn_upsample_video_scratch_floats(dims, batch,
 * frames) floats; NULL or smaller than that: the scratch is not touched and the gradients of all three layers are
 * added with atomics instead (correct, ~5x slower, and the summation order then varies from run to run).  Every pointer is checked before the first launch (a refused call
 * has written nothing).  With C = 64 the kernel reads the rows of dctx, d_u2 and d_u1 sixteen bytes at a time: dctx_ld
 * must be a multiple of 4 and the three pointers 16-byte aligned, otherwise the call is refused with MVN_ERR_BAD_ARG
 * (mvn_padded_len rows of an allocator's buffer always are). */
size_t mvn_upsample_video_scratch_floats(const mvn_dims *dims, int batch, int frames);
int mvn_upsample_video_backward(const mvn_dims *dims, const mvn_video_params *vp,
                                const mvn_video_grads *vg, const float *video, int batch, int frames,
                                int cin, const float *enc, const float *u1, const float *u2,
                                const float *dctx, int dctx_ld, float *d_u2, float *d_u1,
                                float *d_enc, float *scratch, size_t scratch_floats, void *stream);

/* Fill the generator's dilation queues from a saved forward (acts of a prompt
 * of t_len >= RF samples): equivalent to mvn_generate over t in [0, t_len-1). */
int mvn_gen_prime_from_forward(const mvn_dims *dims, const mvn_fwd_buffers *fwd, int batch,
                               int t_len, float *state, void *stream);

/* (B,Q,T) one-hot fp32 <-> (B,T) int32 indices: movenet/dataset.py:285-288 and
 * the scatter at movenet/wavenet.py:235-237.  onehot_to_index writes -1 where a
 * column is not exactly one-hot (the host wrapper then refuses the input). */
int mvn_onehot_to_index(const float *onehot, int32_t *index, int batch, int classes, int t_len,
                        void *stream);
int mvn_index_to_onehot(const int32_t *index, int index_stride, float *onehot, int batch,
                        int classes, int t_len, void *stream);

/* Plumbing for the host wrappers (no reference counterpart): publish up to 64 device 32-bit words
 * to the HOST without a copy engine or a stream synchronisation -- the one-hot validation's
 * minimum index (the reference feeds one-hot tensors to a dense conv and never looks) and the
 * trainer's per-step log scalars (loss, accuracy, gradient norm).  `host_words` points to n + 1
 * words in pinned, device-visible host memory (hipHostMalloc / torch pin_memory()): one wave on
 * `stream` stores words[0..n) to host_words[0..n), then `seq` to host_words[n] (system-scope
 * release); the host polls host_words[n] == seq and so waits for exactly the kernels queued in
 * front of this one -- a stream-synchronising read (tensor.item()) waits for everything the
 * caller has enqueued since. */
int mvn_publish_words(const uint32_t *words, int n, int32_t seq, uint32_t *host_words, void *stream);

/* The trainer's loss and accuracy on the model output (row F3 of SURVEY.md section 8;
 * movenet/pytorch_lightning_trainer.py:64-66): cross_entropy applied to PROBABILITIES
 * (SURVEY Q2), i.e.  loss = mean over (b,s) of  logsumexp_q(probs[b,:,s]) - probs[b,target,s],
 * accuracy = mean of [first argmax_q probs[b,:,s] == target[b,s]].
 *   probs (B, Q, S) fp32, target (B, S) int64 class indices.
 * forward: per-workgroup partial sums, loss_part / correct_part have mvn_ce_parts(B,S)
 *   entries each, ZEROED by the caller (not every slot is written for every shape) and
 *   summed by it in a fixed order: deterministic.
 * backward: dprobs = scale * upstream * (softmax_q(probs) - onehot(target)); scale = 1/(B*S) for
 *   the mean, `upstream` = device pointer to the scalar gradient of the loss (NULL: 1), read
 *   by the kernel so that the host never has to synchronise for it. */
int mvn_ce_parts(int batch, int s_len);
int mvn_ce_on_probs_forward(const float *probs, const long long *target, int batch, int classes,
                            int s_len, float *loss_part, int32_t *correct_part, void *stream);
int mvn_ce_on_probs_backward(const float *probs, const long long *target, int batch, int classes,
                             int s_len, float scale, const float *upstream, float *dprobs,
                             void *stream);

/* The same loss and accuracy FUSED with the model's final softmax (wavenet.py:189-191):
 * forward turns the head's logits (B, Q, S) into probabilities IN PLACE and accumulates the
 * loss / accuracy partial sums of mvn_ce_on_probs_forward in the same pass (same slots, same
 * bits); backward writes d loss / d logits -- through cross_entropy's log-softmax AND the
 * model's softmax -- into a (B, Q, dlogit_ld) tensor at columns dlogit_col0 .. +dlogit_cols
 * (zero for the dlogit_cols - s_len trailing columns), i.e. straight into mvn_backward's
 * dlogit buffer (call mvn_backward with dout = NULL). */
int mvn_softmax_ce_forward(float *logits_probs, const long long *target, int batch, int classes,
                           int s_len, float *loss_part, int32_t *correct_part, void *stream);
int mvn_softmax_ce_backward(const float *probs, const long long *target, int batch, int classes,
                            int s_len, float scale, const float *upstream, float *dlogit,
                            long long dlogit_batch_stride, int dlogit_ld, int dlogit_col0,
                            int dlogit_cols, void *stream);

/* The loss the fused pair differentiates.  REFERENCE: the two calls above -- cross_entropy applied to
 * the model's PROBABILITIES, a second softmax over values in [0, 1], so the loss of a column lies in
 * [ln(e + Q - 1) - 1, ln Q].  MODEL: the negative log-likelihood of the model's own softmax(logits),
 *     loss = mean over (b,s) of  logsumexp_q(logits[b,:,s]) - logits[b,target,s]   (nats),
 *     dlogit_q = scale * upstream * (p_q - [q == target]),
 * formed from the max and the exp-sum the softmax takes anyway: one exponential pass forward, none
 * backward. */
#define MVN_LOSS_REFERENCE 0
#define MVN_LOSS_MODEL 1

/* mvn_softmax_ce_forward / _backward with the loss rule chosen: `loss_rule` is MVN_LOSS_REFERENCE (what
 * the two calls above pass) or MVN_LOSS_MODEL; any other value is MVN_ERR_BAD_ARG, before any launch and
 * before any buffer is touched.  The rule changes the loss and its gradient only: the probabilities
 * written in place are the same bits under both, and so are the accuracy counts (first maximum of the
 * probabilities, target clamped to [0, Q-1]); slots, their zero-initialisation contract and the dlogit
 * window (columns [col0, col0 + s_len) written, [col0 + s_len, col0 + cols) zeroed, nothing outside) are
 * those of the calls above.  Under MODEL the target's logit is read before the column is overwritten,
 * and the backward reads no logits: only the probabilities and the target. */
int mvn_softmax_ce_forward_ex(float *logits_probs, const long long *target, int batch, int classes,
                              int s_len, float *loss_part, int32_t *correct_part, int loss_rule,
                              void *stream);
int mvn_softmax_ce_backward_ex(const float *probs, const long long *target, int batch, int classes,
                               int s_len, float scale, const float *upstream, float *dlogit,
                               long long dlogit_batch_stride, int dlogit_ld, int dlogit_col0,
                               int dlogit_cols, int loss_rule, void *stream);

/* The _ex pair for sequences of their own length: `valid` is a DEVICE array of `batch` int32, read by the kernels
 * and clamped there to [0, s_len]; sequence b counts its columns s < valid[b] only.
 *   forward   the probabilities are written in place for EVERY column, the same bits as _ex; loss_part and
 *             correct_part receive the counted columns only.  A column that is not counted is selected out, not
 *             multiplied by 0: it adds exactly 0 even where its logits are NaN or infinite.  Slots, their
 *             zero-initialisation contract and the fixed-order summation are those of _ex; the caller divides by
 *             max(sum_b valid[b], 1) for the mean.
 *   backward  columns [col0, col0 + valid[b]) of sequence b's window get the gradient with the caller's `scale`,
 *             columns [col0 + valid[b], col0 + cols) get +0.0f whatever the probabilities there hold, nothing
 *             outside the window is touched.  Workgroups that hold no counted column store zeros and read nothing.
 * valid == NULL is the _ex call, kernel for kernel.  Refusals as _ex, before any launch. */
int mvn_softmax_ce_forward_len(float *logits_probs, const long long *target, int batch, int classes,
                               int s_len, float *loss_part, int32_t *correct_part, int loss_rule,
                               const int32_t *valid, void *stream);
int mvn_softmax_ce_backward_len(const float *probs, const long long *target, int batch, int classes,
                                int s_len, float scale, const float *upstream, float *dlogit,
                                long long dlogit_batch_stride, int dlogit_ld, int dlogit_col0,
                                int dlogit_cols, int loss_rule, const int32_t *valid, void *stream);

/* Scoring GIVEN audio under the model: per-position log-likelihood of the target from the head's logits, read
 * only -- no probability tensor is formed and `logits` comes back bit for bit.  With y = logits / temperature:
 *     logp[b,s]      = y_t - logsumexp_q(y[b,:,s])                       (nats)
 *     entropy[b,s]   = -sum_q p_q log p_q of softmax(y); a class with p_q = 0 (a -inf logit included) adds exactly 0
 *     rank[b,s]      = #{q : y_q > y_t} + #{q < t : y_q == y_t}, compared on the logits themselves (temperature > 0
 *                      keeps their order): 0 exactly where the first-maximum accuracy rule of the loss calls above
 *                      counts the column as correct
 *     seq_nll[b]     = -sum_s logp[b,s]
 *     seq_correct[b] = #{s : rank[b,s] == 0}
 *   logits   (B, Q, S) fp32 as mvn_forward leaves them, rows at any 4-byte alignment
 *   target   (B, S) int64, clamped to [0, Q-1] as the loss calls clamp it
 *   logp, entropy, rank  (B, S) each; seq_nll, seq_correct  (B,) each; any of the five NULL: not formed, not written
 *   scratch  mvn_score_scratch_floats(B, S) floats, NOT initialised by the caller: the first kernel writes every
 *            per-workgroup partial sum the second one reads, and that one adds a sequence's partials in a fixed
 *            order in double (no atomics: two calls on the same input return the same bits)
 * temperature must be finite and above 0; that, or a scratch that is too small, is MVN_ERR_BAD_ARG before any
 * launch and before any buffer is touched.  Q <= 256 with a sequence's (Q, S) tensor inside 2^31 bytes runs the
 * column form of the loss calls (32-bit buffer offsets), anything else one thread per column with 64-bit
 * addresses.  A column that is entirely -inf is undefined.  S == 0 stores zeros in seq_nll / seq_correct. */
size_t mvn_score_scratch_floats(int batch, int s_len);
int mvn_score_columns(const float *logits, const long long *target, int batch, int classes, int s_len,
                      float temperature, float *logp, float *entropy, int32_t *rank, float *seq_nll,
                      int32_t *seq_correct, float *scratch, size_t scratch_floats, void *stream);

/* mvn_score_columns for sequences of their own length: `valid` as in mvn_softmax_ce_forward_len (DEVICE, `batch`
 * int32, clamped to [0, s_len] by the kernel; NULL: the call above).  A column s >= valid[b] gets logp = 0.0f,
 * entropy = 0.0f and rank = -1, whatever its logits hold, and seq_nll / seq_correct run over the counted columns only
 * -- same slots, same fixed order, in double, no atomics. */
int mvn_score_columns_len(const float *logits, const long long *target, int batch, int classes, int s_len,
                          float temperature, float *logp, float *entropy, int32_t *rank, float *seq_nll,
                          int32_t *seq_correct, float *scratch, size_t scratch_floats, const int32_t *valid,
                          void *stream);

/* One optimizer step of torch.optim.AdamW (decoupled != 0) or torch.optim.Adam (decoupled == 0,
 * weight decay added to the gradient) over flat fp32 buffers of n elements
 * (movenet/pytorch_lightning_trainer.py:186-189; arithmetic of torch's _single_tensor_adam,
 * amsgrad off).  step counts from 1.  skip_ranges: HOST array of n_skip <= 4 [lo, hi) element
 * ranges left untouched (parameters without a gradient this step). */
int mvn_adamw_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   int decoupled, const size_t *skip_ranges, int n_skip, void *stream);

/* mvn_adamw_step with an exponential moving average (EMA) of the parameters kept in the same launch.
 * param, exp_avg and exp_avg_sq come out as mvn_adamw_step leaves them, bit for bit; behind that, for
 * every element that is stepped,
 *     ema[i] = ema[i] + (param_new[i] - ema[i]) * ema_weight,
 * ema_weight = 1 - decay of this update, formed by the caller (in double, then rounded to float).
 *   ema         DEVICE, n floats, distinct from the other four buffers; the caller initialises it
 *               (to the parameters)
 *   ema_weight  in (0, 1]; 1 makes ema a copy of the stepped elements
 * Elements inside a skip range are left untouched in ema as in the other buffers.  A null ema or an
 * ema_weight outside (0, 1] (NaN included) is MVN_ERR_BAD_ARG, like mvn_adamw_step's own refusals before
 * any launch; n == 0 is MVN_OK. */
int mvn_adamw_ema_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *ema,
                       size_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int step, int decoupled, float ema_weight, const size_t *skip_ranges, int n_skip,
                       void *stream);

/* mu-law companding either side of the model (movenet/dataset.py:278-289 encode ->
 * one-hot; movenet/callbacks.py:66-76 argmax -> decode).  The reference calls torchaudio,
 * which is absent offline and pinned by no fixture: formula of RESEARCH.md:156-163,
 * PARITY UNPINNED.  Shipping indices instead of (B,Q,T) one-hot floats removes a
 * 256x larger host->device copy. */
int mvn_mu_law_encode(const float *x, int32_t *index, size_t n, int classes, void *stream);
int mvn_mu_law_decode(const int32_t *index, float *x, size_t n, int classes, void *stream);

/* Finished samples to 16-bit PCM, for handing audio out while it is being generated: for row b < batch and column
 * j < n, pcm[b * pcm_stride + j] is the PCM value of class samples[b * sample_stride + t0 + j].  To the bit, that is
 * what the sample logger's WAV writer stores for mvn_mu_law_decode of the class: the float mvn_mu_law_decode gives,
 * then (in double) clipped to [-1, 1], multiplied by 32767 and rounded half to even.  The value depends on the class
 * alone; a class outside [0, classes) is clamped to the nearest end, as the generators clamp a pick.
 *   samples  DEVICE (batch, sample_stride) int32, e.g. the generators' sample buffer
 *   pcm      DEVICE int16, rows pcm_stride elements apart (2-byte aligned is enough; nothing outside [0, n) of a
 *            row is written)
 * One launch, a pure stream.  MVN_ERR_BAD_ARG with a mvn_last_error() text, before any launch: a NULL pointer,
 * batch < 1, n < 0, t0 < 0, t0 + n > sample_stride, pcm_stride < n, classes outside 2 .. 32768.  n == 0 is MVN_OK
 * without a launch. */
int mvn_pcm16_chunk(const int32_t *samples, int batch, int sample_stride, int t0, int n, int classes, int16_t *pcm,
                    int pcm_stride, void *stream);

/* mvn_pcm16_chunk through the DE-EMPHASIS filter, the inverse of mvn_audio_frontend_emph's pre-emphasis, with the
 * filter's state carried from call to call.  Per row b, columns in order, with x the float mvn_mu_law_decode gives for
 * the (clamped) class and a = coef, both widened to double:
 *     y   = ((1 + a) * x) + (a * y_prev)     two products and one sum, each rounded once in double, no fma
 *     pcm = y clipped to [-1, 1], times 32767, rounded half to even (as above)
 *     y_prev = y
 * y_prev is state[b] at entry and is written back to state[b] at exit; the caller zeroes it before a row's column 0.
 * The recurrence is defined -- and run -- sequentially in time (one wave per row, rows in parallel), so a clip cut into
 * chunks of any lengths gives the bits of the whole clip in one call.
 *   state  DEVICE, batch doubles, 8-byte aligned
 *   coef   in [0, 1)
 * Refusals as mvn_pcm16_chunk, and: state NULL or not 8-byte aligned, coef outside [0, 1) (NaN included) --
 * MVN_ERR_BAD_ARG before any launch.  n == 0 is MVN_OK without a launch: the state is left as it is. */
int mvn_pcm16_deemph_chunk(const int32_t *samples, int batch, int sample_stride, int t0, int n, int classes, float coef,
                           double *state, int16_t *pcm, int pcm_stride, void *stream);

/* The loader's waveform front end (movenet/dataset.py:253-289 behind the decoder): a batch of clips of different
 * lengths, as interleaved int16 PCM in one upload, -> (batch, n_out) int32 class indices.  Per clip: channel mean of
 * pcm / 32768; resample of the whole clip to n_out frames by torchaudio's sinc_interp_hann rule (lowpass_filter_width
 * 6, roll-off 0.99), the taps evaluated in place; when `normalize`, y <- 2 (y - min)/(max - min) - 1
 * unless max == min; mu-law of mvn_mu_law_encode, clamped to 0 .. classes-1.
 *   pcm      DEVICE, pcm_len int16 elements
 *   clips    DEVICE, one descriptor per clip: element offset of its first sample, frames, channels
 *   y        DEVICE (batch, n_out) fp32: the resampled waveform before normalisation (written in full)
 *   scratch  DEVICE mvn_audio_frontend_scratch_floats(batch, n_out) floats, 8-byte aligned: (min, max) per tile
 *   index    DEVICE (batch, n_out) int32
 * The descriptors are read on the device, so they are checked there: a clip whose span does not lie inside
 * [0, pcm_len), or with frames > 100 n_out-ish (the window of one output tile no longer fits the LDS; frames <=
 * 100 n_out always fits), is not read at all and its row of `index` is filled with -1.  8-bit PCM is shipped as
 * (v - 128) << 8, 24- and 32-bit PCM rounded to 16 bits, by the host.  Two launches, no atomics: bit-reproducible. */
typedef struct {
  int64_t offset;
  int32_t frames;
  int32_t channels;
} mvn_audio_clip;
size_t mvn_audio_frontend_scratch_floats(int batch, int n_out);
int mvn_audio_frontend(const int16_t *pcm, long long pcm_len, const mvn_audio_clip *clips, int batch, int classes,
                       int n_out, int normalize, float *y, float *scratch, int32_t *index, void *stream);

/* The front end by RATE: clip b is resampled, as a whole, to its own n_out frames -- the arithmetic of the call above
 * for that clip alone with that n_out, bit for bit, the min-max normalisation over those n_out values only -- into
 * row b of (batch, width) outputs; columns [n_out, width) get y = 0 and the class mu-law gives 0.0,
 * (int)((classes - 1) / 2.0f + 0.5f).  A descriptor with n_out outside [1, width], or one the call above would
 * refuse, is not read through: its whole row of `index` is -1 (and of `y` 0).  `reserved` is ignored.
 *   y, index  DEVICE (batch, width);  scratch  mvn_audio_frontend_var_scratch_floats(batch, width) floats, 8-byte
 *   aligned.  Host refusals as above, with width in n_out's place. */
typedef struct {
  int64_t offset;
  int32_t frames;
  int32_t channels;
  int32_t n_out;
  int32_t reserved;
} mvn_audio_clip_var;
size_t mvn_audio_frontend_var_scratch_floats(int batch, int width);
int mvn_audio_frontend_var(const int16_t *pcm, long long pcm_len, const mvn_audio_clip_var *clips, int batch,
                           int classes, int width, int normalize, float *y, float *scratch, int32_t *index,
                           void *stream);

/* The front end by rate on a WINDOW of a file: row b is the columns [out_first, out_first + n_out) of the resample of
 * its whole file from rate_in to rate_out, formed from the span of source frames those columns' taps reach -- the only
 * part of the file that is uploaded.  With g = gcd(rate_in, rate_out), orig = rate_in / g, new = rate_out / g, and s, W
 * as for the calls above from (orig, new): the file's resample has n_file = ceil(file_frames new / orig) outputs, and
 * for the global output index j (64-bit) p = j orig, i0 = p / new, frac = (p mod new) / new,
 *   y = sum_{d = -W}^{W + 1} m[i0 + d] h(d - frac),   m = 0 outside [0, file_frames),
 * taps and channel mean those of the calls above.  The 2 W + 2 products are summed in blocks of 128 -- each block from
 * 0 by fmaf in ascending d, the block sums added in ascending order -- so that a long filter (1216 taps at 100 : 1)
 * keeps the accuracy of a short one.  Nothing in a sample depends on where its row starts: a window is a crop of the
 * whole file's resample by this call, to the bit; and up to 128 taps (rate_in <= 10 rate_out) the sum is one block,
 * the bits of mvn_audio_frontend_var where its frames : n_out reduces to the same orig : new.  Columns [n_out, width) get y = 0 and the
 * silence class, as there.  When `normalize`: by (lo, hi) where hi > lo (and hi - lo finite) -- the host's per-file
 * gain -- else by the window's own (min, max), max == min left alone.
 *   clips     DEVICE, one 64-byte descriptor per row
 *   y, index  DEVICE (batch, width);  scratch  mvn_audio_frontend_window_scratch_floats(batch, width) floats, 8-byte
 *   aligned.  Host refusals as above.
 * Checked on the device; a refused row has index = -1 and y = 0 and nothing of the upload is read for it:
 *   - the span [offset, offset + span_frames channels) does not lie inside [0, pcm_len), or span_frames < 1;
 *   - n_out outside [1, width];
 *   - rate_in, rate_out or channels < 1;
 *   - a ratio whose window of 64 outputs does not fit the LDS tile (rate_in <= 100 rate_out always fits);
 *   - out_first < 0 or out_first + n_out > n_file (file_frames < 1, or file_frames new >= 2^62, has no n_file);
 *   - the span does not cover [i0(out_first) - W, i0(out_first + n_out - 1) + W + 1] intersected with
 *     [0, file_frames): span_first above its first frame, or span_first + span_frames - 1 below its last.
 * Two launches, no atomics: bit-reproducible, and a row does not depend on its place in the batch. */
typedef struct {
  int64_t offset;      /* element offset of the uploaded span in pcm */
  int64_t span_first;  /* source frame index of the span's first frame */
  int64_t out_first;   /* global output index of the row's first column */
  int64_t file_frames; /* frames in the whole file */
  int32_t span_frames; /* frames in the uploaded span */
  int32_t channels;
  int32_t n_out;
  int32_t rate_in;
  int32_t rate_out;
  float lo, hi;        /* given normalisation range; hi <= lo: the window's own */
  int32_t reserved;
} mvn_audio_clip_window;
size_t mvn_audio_frontend_window_scratch_floats(int batch, int width);
int mvn_audio_frontend_window(const int16_t *pcm, long long pcm_len, const mvn_audio_clip_window *clips, int batch,
                              int classes, int width, int normalize, float *y, float *scratch, int32_t *index,
                              void *stream);

/* Any of the three front ends above with PRE-EMPHASIS in front of mu-law.  `form` says which call this one stands for
 * and with it what `clips` points at (mvn_audio_clip, _var or _window records); every other argument, the device-side
 * refusals and the first launch (the resample, y and the (min, max) partials) are that call's.  With vn[k] the value that
 * call hands to mu-law for column k of a row -- normalised when `normalize`, the raw resample otherwise -- the second
 * launch quantises
 *     e[k] = (vn[k] - coef * vn[k-1]) / (1 + coef),   vn[-1] := 0,
 * in float, each operation rounded once (no fma), so |e| <= 1 wherever |vn| <= 1.  k - 1 is column k - 1 of the SAME
 * ROW: the row's first column has no predecessor, also where a window starts in the middle of its file.  The
 * normalisation range is the un-emphasised row's, as before.
 *   coef   in [0, 1); 0 gives the indices of the call it stands for
 *   emph   DEVICE (batch, width) fp32: e, written in full -- 0 in the columns behind a row's n_out, which get the
 *          silence class as before, and in a refused row, whose indices are -1 as before
 * emph == NULL, a coef outside [0, 1) (NaN included) or an unknown form is MVN_ERR_BAD_ARG before any launch, like the
 * host refusals of the call it stands for.  Two launches, no atomics: bit-reproducible. */
#define MVN_AUDIO_FORM_CLIP 0
#define MVN_AUDIO_FORM_VAR 1
#define MVN_AUDIO_FORM_WINDOW 2
int mvn_audio_frontend_emph(int form, const int16_t *pcm, long long pcm_len, const void *clips, int batch, int classes,
                            int width, int normalize, float coef, float *y, float *scratch, int32_t *index,
                            float *emph, void *stream);

/* The loader's video front end (movenet/dataset.py:292-310 behind the decoder): a batch of clips of different
 * resolutions, as interleaved uint8 frames in one upload, -> (batch, n_frames, 64, 64) uint8 gray levels.  Per frame:
 * L = uint8(0.2989 r + 0.587 g + 0.114 b), fp32 products and sums each rounded, the cast truncating (skipped for
 * channels == 1); then torch's bilinear resize of L to 64 x 64 with align_corners=False and antialias as given,
 * rounded half to even.  No division by 255: the levels are 0 .. 255.
 *   pix      DEVICE, pix_len bytes: every clip's n_frames frames, each (n_frames, height, width, channels) uint8, rows
 *            of width * channels bytes without padding; offsets and the pointer itself need no alignment
 *   clips    DEVICE, one descriptor per clip: byte offset of its first frame, height, width, channels (3: RGB, 1: gray)
 *   levels   DEVICE (batch, n_frames, 64, 64) uint8, written in full
 *   status   DEVICE (batch,) int32: 0, or why the clip was not read
 * The descriptors are read on the device, so they are checked there: a clip whose span does not lie inside
 * [0, pix_len) (status 1), whose channels is not 1 or 3 (status 2), or whose height or width is outside [1, 4096]
 * (status 3) is not read at all and its levels are zero.  On the host, a null pointer, pix_len < 0, batch < 0,
 * n_frames < 1, antialias other than 0 or 1, or batch * n_frames * 16 workgroups beyond 2^31 - 1 is MVN_ERR_BAD_ARG
 * before any launch; batch == 0 is MVN_OK and launches nothing.  One launch, no atomics: bit-reproducible. */
typedef struct {
  int64_t offset;
  int32_t height, width, channels, reserved;
} mvn_video_clip;
int mvn_video_frontend(const uint8_t *pix, long long pix_len, const mvn_video_clip *clips, int batch, int n_frames,
                       int antialias, uint8_t *levels, int32_t *status, void *stream);

/* ---- The five building blocks as calls of their own (csrc/blocks.hip; additive, ABI version unchanged) ----
 * movenet/modules.py's CausalConv1d, DilatedCausalConv1d, GatedResidualConv1d and DenseConv, forward and backward, on
 * tensors the caller lays out (ResidualConvStack is the gated layer, called once per layer).  All data is fp32 on the
 * device.  A tensor is (batch, channels, len) behind `p` with row stride `ld` floats and batch stride channels * ld:
 * any ld >= len and any 4-byte alignment works (a PyTorch-contiguous (B, C, T) with odd T goes in as it is), and columns
 * at or beyond len are neither read nor written.  Weights have PyTorch's layouts: (out, in, 2) for the two-tap convs,
 * (out, in) for the 1x1 convs.
 *
 * Semantics (n = T - d is the gated / dilated layer's output length):
 *   causal   y[:, :, t] = W[:, :, 0] x[:, :, t - 1] + W[:, :, 1] x[:, :, t] (+ bias), x[-1] = 0;   y.len == x.len
 *   dilated  y[:, :, j] = W[:, :, 0] x[:, :, j] + W[:, :, 1] x[:, :, j + d] (+ bias);              y.len == x.len - d
 *   gated    f | g = dilated convs (+ the context's 1x1 convs and their biases on the LAST n columns of the context);
 *            z = tanh(f) sigmoid(g); residual = Wr z + br + x[:, :, d:]; skip = (Ws z + bs)[:, :, n - skip.len:]
 *            th / sg (both or neither): tanh(f) and sigmoid(g), (B, C, n) with one row stride -- what the backward reads
 *   dense    y = W2 leaky_relu(W1 leaky_relu(x) + b1) + b2; hidden: the first conv's output (NULL: kept in scratch)
 *
 * Gradients: data gradients (dx, dcontext) are written in full -- dcontext over all of the context's columns, zero in
 * front of the ones the layer used -- and a NULL tensor skips that product.  Parameter gradients ACCUMULATE (the rule
 * of mvn_param_grads); a NULL pointer means "not wanted".  d_residual or d_skip (not both) may be NULL: that output
 * received no gradient.  Summation runs in a fixed order (per-workgroup slabs added up by one thread per word, no float
 * atomics): two calls on the same data give the same bits.
 *
 * Every argument is checked before the first launch and a refused call has written nothing: NULL pointers, ld < len,
 * lengths that do not fit each other, T <= d, a context shorter than n and a scratch below the sizing function's answer
 * are MVN_ERR_BAD_ARG; channel counts beyond 256 (residual, skip, the head's input) / 1024 (the head's output, the
 * causal conv) are MVN_ERR_BAD_DIMS; rows of 2^31 bytes or more are MVN_ERR_UNSUPPORTED.  The sizing functions are
 * host arithmetic (0 for shapes the calls refuse, never 0 otherwise).
 *
 * mvn_block_last_form(): the kernel form of the most recent block call of this process (0 before any) -- FUSED64 after a
 * gated forward at C = K = 64 (one kernel per layer, z never written to memory), GENERIC after every other call,
 * the backward passes at C = K = 64 included (they are composed from the generic kernel family). */
typedef struct mvn_block_tensor {
  float *p;
  int32_t ld;  /* row stride, floats */
  int32_t len; /* columns */
} mvn_block_tensor;

typedef struct mvn_block_gated_params {
  const float *filter_w, *filter_b; /* (C, C, 2); bias (C) or NULL */
  const float *gate_w, *gate_b;
  const float *ctx_filter_w, *ctx_filter_b; /* (C, C), (C): read only when a context is given */
  const float *ctx_gate_w, *ctx_gate_b;
  const float *residual_w, *residual_b; /* (C, C), (C) */
  const float *skip_w, *skip_b;         /* (K, C), (K) */
} mvn_block_gated_params;

typedef struct mvn_block_gated_grads { /* accumulated into; NULL: not wanted */
  float *filter_w, *filter_b;
  float *gate_w, *gate_b;
  float *ctx_filter_w, *ctx_filter_b;
  float *ctx_gate_w, *ctx_gate_b;
  float *residual_w, *residual_b;
  float *skip_w, *skip_b;
} mvn_block_gated_grads;

#define MVN_BLOCK_FORM_GENERIC 1
#define MVN_BLOCK_FORM_FUSED64 2
int mvn_block_last_form(void);

/* scratch of the causal / dilated backward (channels in, channels out, the OUTPUT length) */
size_t mvn_block_conv_scratch_floats(int cin, int cout, int batch, int t_len);
int mvn_block_causal_forward(const float *w, const float *bias, int cin, int cout, const mvn_block_tensor *x,
                             const mvn_block_tensor *y, int batch, void *stream);
int mvn_block_causal_backward(const float *w, int cin, int cout, const mvn_block_tensor *x, const mvn_block_tensor *dy,
                              const mvn_block_tensor *dx, float *dw, float *dbias, int batch, float *scratch,
                              size_t scratch_floats, void *stream);
int mvn_block_dilated_forward(const float *w, const float *bias, int channels, int dilation, const mvn_block_tensor *x,
                              const mvn_block_tensor *y, int batch, void *stream);
int mvn_block_dilated_backward(const float *w, int channels, int dilation, const mvn_block_tensor *x,
                               const mvn_block_tensor *dy, const mvn_block_tensor *dx, float *dw, float *dbias, int batch,
                               float *scratch, size_t scratch_floats, void *stream);

/* t_len: the layer's INPUT length T.  backward == 0: what the forward needs when th / sg are not given */
size_t mvn_block_gated_scratch_floats(int residual_channels, int skip_channels, int batch, int t_len, int dilation,
                                      int has_context, int backward);
int mvn_block_gated_forward(const mvn_block_gated_params *p, int residual_channels, int skip_channels, int dilation,
                            const mvn_block_tensor *x, const mvn_block_tensor *context, const mvn_block_tensor *residual,
                            const mvn_block_tensor *skip, const mvn_block_tensor *th, const mvn_block_tensor *sg,
                            int batch, float *scratch, size_t scratch_floats, void *stream);
int mvn_block_gated_backward(const mvn_block_gated_params *p, const mvn_block_gated_grads *grads, int residual_channels,
                             int skip_channels, int dilation, const mvn_block_tensor *x, const mvn_block_tensor *context,
                             const mvn_block_tensor *th, const mvn_block_tensor *sg, const mvn_block_tensor *d_residual,
                             const mvn_block_tensor *d_skip, const mvn_block_tensor *dx, const mvn_block_tensor *dcontext,
                             int batch, float *scratch, size_t scratch_floats, void *stream);

size_t mvn_block_dense_scratch_floats(int in_channels, int out_channels, int batch, int s_len, int backward);
int mvn_block_dense_forward(const float *w1, const float *b1, const float *w2, const float *b2, int in_channels,
                            int out_channels, const mvn_block_tensor *x, const mvn_block_tensor *hidden,
                            const mvn_block_tensor *y, int batch, float *scratch, size_t scratch_floats, void *stream);
int mvn_block_dense_backward(const float *w1, const float *w2, int in_channels, int out_channels,
                             const mvn_block_tensor *x, const mvn_block_tensor *hidden, const mvn_block_tensor *dy,
                             const mvn_block_tensor *dx, float *dw1, float *db1, float *dw2, float *db2, int batch,
                             float *scratch, size_t scratch_floats, void *stream);

/* ---- Local conditioning on log-mel frames (csrc/features.hip; additive, ABI version unchanged) ----
 * The feature front end: (batch, n_samples) int32 class indices -> (batch, n_mels, F) fp32 log-mel frames,
 * F = n_samples / hop + 1 (integer division).  With N = n_fft:
 *   x[b, t]  the mu-law decode of index[b, t] by the formula of the decode call above; 0 for t outside [0, n_samples)
 *            and for an index outside [0, classes) (nothing is raised)
 *   frame j  covers samples [j hop - N/2, j hop + N/2), times the window w[n]
 *   P[k]     |sum_n w[n] x[n] e^{-2 pi i k n / N}|^2, k = 0 .. N/2
 *   mel      log(max(sum_k fbank[m, k] P[k], floor)), natural log; `energies` != 0: the sum itself, no floor, no log
 * The kernel knows no mel scale; it reads three DEVICE tables: window (N), twiddle (2 N: cos(2 pi m / N) for m < N, then
 * sin(2 pi m / N), indexed by (k n) mod N) and fbank (n_mels, N/2 + 1).  The DFT is a product on the fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32), fp32 throughout, every sum in a fixed order, no atomics: two calls give the same bits.
 *   mel      DEVICE (batch, n_mels, mel_ld) with mel_ld >= F; only the first F columns of a row are written
 *   scratch  DEVICE, at least the sizing call's answer in floats (the decoded signal and the power spectra)
 * MVN_ERR_BAD_ARG before any launch: a null pointer, n_fft not a power of two in [32, 2048], hop outside [1, n_fft],
 * n_mels < 1, floor <= 0 (NaN included), batch < 0, n_samples < 1, classes < 2, mel_ld < F, a scratch that is too
 * small, batch or n_mels above 65535, n_samples above 2^30, batch * n_samples above 2^31 - 1.  batch == 0 is MVN_OK
 * and launches nothing. */
size_t mvn_logmel_scratch_floats(int batch, int n_samples, int n_fft, int hop);
int mvn_logmel_frontend(const int32_t *index, int batch, int n_samples, int classes, int n_fft, int hop, int n_mels,
                        const float *window, const float *twiddle, const float *fbank, float floor, int energies,
                        float *mel, int mel_ld, float *scratch, size_t scratch_floats, void *stream);

/* The frame up-sampler: mel (batch, n_mels, frames), w (channels, n_mels), bias (channels) -> ctx (batch, channels,
 * n_samples).  With j = t / hop, a = (t mod hop) / hop, j1 = min(j + 1, frames - 1):
 *   ctx[b, c, t] = bias[c] + sum_m w[c, m] ((1 - a) mel[b, m, j] + a mel[b, m, j1])
 * formed as the 1x1 product at frame rate (into scratch) and the interpolation of its rows, stored 16 bytes at a time:
 * ctx must be 16-byte aligned and ctx_ld a multiple of 4 (>= n_samples).  Needs frames >= (n_samples - 1) / hop + 1.
 * Any channels >= 1 and n_mels >= 1 (each at most 65535).  scratch: the sizing call's floats.
 *
 * The backward: dctx (batch, channels, n_samples) -> dw (channels, n_mels) and dbias (channels), both ACCUMULATED INTO
 * (NULL: not wanted), and dmel (batch, n_mels, frames), written in full (NULL: not wanted).  dP[b, c, j], the weighted
 * sum of the up to 2 hop columns of dctx that touch frame j, is formed first (one workgroup per row segment); then
 * dw = sum dP mel^T, dbias = sum dP, dmel = w^T dP at frame rate.  A frame no column touches has dP = 0 and dmel = 0
 * exactly.  Fixed order, no atomics.  Every refusal (MVN_ERR_BAD_ARG: null pointers, sizes below 1, a row stride
 * below its length, a misaligned ctx / ctx_ld, too few frames, a small scratch, batch < 0, frames or n_samples above
 * 2^30, hop above 2^24) comes before the first launch and writes nothing; batch == 0 is MVN_OK. */
size_t mvn_upsample_features_scratch_floats(int batch, int channels, int frames);
int mvn_upsample_features(const float *mel, int mel_ld, const float *w, const float *bias, int batch, int n_mels,
                          int frames, int channels, int hop, int n_samples, float *ctx, int ctx_ld, float *scratch,
                          size_t scratch_floats, void *stream);
int mvn_upsample_features_backward(const float *dctx, int dctx_ld, const float *mel, int mel_ld, const float *w,
                                   int batch, int n_mels, int frames, int channels, int hop, int n_samples, float *dw,
                                   float *dbias, float *dmel, int dmel_ld, float *scratch, size_t scratch_floats,
                                   void *stream);

/* The frame up-sampler with a window of neighbouring frames (additive, ABI version unchanged): w is
 * (channels, n_mels, taps) in nn.Conv1d's own layout, taps = 2 k + 1 for k frames of context on each side.  With
 * F = frames, the number of frames GIVEN, and cl(i) = min(max(i, 0), F - 1):
 *   proj[b, c, j] = bias[c] + sum_{d = -k..k} sum_m w[c, m, d + k] mel[b, m, cl(j + d)]               j = 0 .. F - 1
 *   ctx[b, c, t]  = (1 - a) proj[b, c, j] + a proj[b, c, min(j + 1, F - 1)]       j = t / hop, a = (t mod hop) / hop
 * Edge frames are replicated, not zero-filled (a log-mel of 0.0 is a loud frame, not silence), and the clamp is to the
 * last frame of the tensor handed in, surplus frames included, as j1 above.  No element of a mel row at or beyond
 * column F is read.  proj goes into scratch (the sizing call above); the rows are interpolated and stored as above, so
 * ctx has the alignment rules of mvn_upsample_features.  taps == 1 gives that call's bits.
 *
 * The backward: dP[b, c, j] exactly as above, then
 *   dbias[c]          += sum_{b, j} dP[b, c, j]
 *   dw[c, m, d + k]   += sum_b sum_j dP[b, c, j] mel[b, m, cl(j + d)]
 *   dmel[b, m, i]      = sum_d sum_{j : cl(j + d) = i} sum_c w[c, m, d + k] dP[b, c, j]
 * An interior frame i collects j = i - d; frame 0 collects every j <= -d and frame F - 1 every j >= F - 1 - d, so the
 * two edge frames sum several (j, d) pairs each, and with F <= k every tap of every frame clamps.  dmel is formed in
 * gather form, one thread per word: fixed order, no atomics, the same bits on every call.  dw and dbias are
 * ACCUMULATED INTO, dmel is written in full (its first F columns of each row), and each of the three may be NULL.
 * MVN_ERR_BAD_ARG before any launch, with nothing written: everything the two calls above refuse (null pointers,
 * sizes below 1, a row stride below its length, a misaligned ctx / ctx_ld, too few frames, a small scratch, the size
 * limits), and taps even, below 1 or above 33.  batch == 0 is MVN_OK. */
int mvn_upsample_features_win(const float *mel, int mel_ld, const float *w, const float *bias, int batch, int n_mels,
                              int frames, int channels, int taps, int hop, int n_samples, float *ctx, int ctx_ld,
                              float *scratch, size_t scratch_floats, void *stream);
int mvn_upsample_features_win_backward(const float *dctx, int dctx_ld, const float *mel, int mel_ld, const float *w,
                                       int batch, int n_mels, int frames, int channels, int taps, int hop,
                                       int n_samples, float *dw, float *dbias, float *dmel, int dmel_ld,
                                       float *scratch, size_t scratch_floats, void *stream);

/* The frame-rate half of mvn_upsample_features_win with its result kept, and one window of the generators' time-major
 * context formed from it (additive, ABI version unchanged).
 *
 * mvn_project_features: mel (batch, n_mels, frames), w (channels, n_mels, taps), bias (channels) -> proj (batch,
 * channels, proj_ld), the first `frames` columns of a row written: the bits mvn_upsample_features_win leaves in its
 * scratch for the same inputs (the same kernel through the same launcher, edge frames clamped to the `frames` given).
 * MVN_ERR_BAD_ARG before any launch: what that call refuses of these arguments (null pointers, taps, sizes below 1,
 * batch / n_mels / channels above 65535, frames above 2^30, mel_ld or proj_ld below frames).  batch == 0 is MVN_OK.
 *
 * mvn_context_window: win (rows, n, channels) time-major, columns [t0, t0 + n) of every row.  With F = frames,
 * j = t / hop, a = (t mod hop) / hop, p = proj[r mod proj_rows] (proj is (proj_rows, channels, proj_ld)):
 *   win[r, t - t0, c] = ((1 - a) p[c, j] + a p[c, min(j + 1, F - 1)])  [+ glob[r, c]]         t = t0 .. t0 + n - 1
 *   proj == NULL   win[r, t - t0, c] = glob[r, c]: the label-only window, the same for every t0
 *   glob == NULL   no label; glob is (rows, channels), zeros in the unconditional rows of a guided pair
 *   proj_rows      the two rows of a guided pair share one projection: rows = 2 * proj_rows
 * The contract is bit equality with columns [t0, t0 + n) of mvn_upsample_features_win over any n_samples >= t0 + n
 * followed by mvn_transpose_context and mvn_context_add_global: a = (float)(t mod hop) * (1.0f / (float)hop), the word
 * is fmaf(a, p[c, j1], (1.0f - a) * p[c, j]) as in that call's interpolation, and the label's vector is added last.
 * t0 need not be a multiple of hop or of 4.  A thread stores four channels at once (16 bytes) where channels is a
 * multiple of 4 and win 16-byte aligned, one otherwise; fixed order, no atomics; nothing outside win's rows * n *
 * channels floats is written.
 * MVN_ERR_BAD_ARG before any launch, with nothing written: win NULL; proj and glob both NULL; rows < 0, channels or
 * n below 1; t0 < 0; rows or channels above 65535; t0 + n above 2^30; with proj: proj_rows, frames or hop below 1,
 * proj_ld below frames, frames above 2^30, hop above 2^24, frames below (t0 + n - 1) / hop + 1 (the text names the
 * columns).  rows == 0 is MVN_OK. */
int mvn_project_features(const float *mel, int mel_ld, const float *w, const float *bias, int batch, int n_mels,
                         int frames, int channels, int taps, float *proj, int proj_ld, void *stream);
int mvn_context_window(const float *proj, int proj_ld, int proj_rows, int frames, const float *glob, int rows,
                       int channels, int hop, int t0, int n, float *win, void *stream);

/* ---- Distance between two feature tensors (csrc/metrics.hip; additive, ABI version unchanged) ----
 * a, b (batch, n_mels, frames) fp32, contiguous, DEVICE, read only; first, count (batch) int32, DEVICE: sequence s
 * counts its frames [first[s], first[s] + count[s]).  With d = (double)a[s,m,f] - (double)b[s,m,f] over that span:
 *     rms_f          = sqrt((1 / n_mels) sum_m d^2)
 *     lsd[s]         = (10 / ln 10) (1 / count[s]) sum_f rms_f     dB where the features are natural logs of power
 *     l1[s]          = (1 / (n_mels count[s])) sum_f sum_m |d|
 *     per_frame[s,f] = (float)(rms_f 10 / ln 10) inside the span, 0.0f outside it
 *   lsd, l1    DEVICE (batch) double each; count[s] == 0 stores 0.0 in both (nothing is divided)
 *   per_frame  DEVICE (batch, frames) fp32, written in full; NULL: not formed, not written
 *   scratch    DEVICE, 8-byte aligned, mvn_feature_distance_scratch_floats(batch, frames) floats, NOT initialised by
 *              the caller: one pair of doubles per workgroup of 256 frames, all of them written by the first kernel
 * No frame outside a sequence's span is read, whatever it holds; the kernels clamp the span to [0, frames) and the
 * caller checks the range proper.  Every sum is formed in double in a fixed order, no atomics: the same inputs give
 * the same bits on every call, and a sequence's results do not depend on the other sequences of the launch.
 * MVN_ERR_BAD_ARG before any launch: a null pointer (per_frame excepted), batch, n_mels or frames below 1, batch above
 * 65535, a scratch that is too small or misaligned. */
size_t mvn_feature_distance_scratch_floats(int batch, int frames);
int mvn_feature_distance(const float *a, const float *b, int batch, int n_mels, int frames, const int32_t *first,
                         const int32_t *count, double *lsd, double *l1, float *per_frame, float *scratch,
                         size_t scratch_floats, void *stream);

/* ---- A frame-wise pitch tracker and the distance of two pitch tracks (csrc/pitch.hip; additive, ABI version
 * unchanged) ----
 * mvn_pitch_frames: the YIN estimator, one result per frame.  Exactly one of `index` and `wave` is non-NULL, both
 * (batch, n_samples), DEVICE, read only:
 *   index    int32 class indices; x is their mu-law decode by the formula of mvn_mu_law_decode (the float
 *            mvn_logmel_frontend forms), 0 for an index outside [0, classes) (nothing is raised)
 *   wave     fp32 samples, taken as they are; `classes` is ignored
 *   x[t] = 0 for t outside [0, n_samples)
 * F = n_samples / hop + 1 frames (integer division; mvn_logmel_frontend's frames).  With L = win + tau_max, frame j
 * covers samples [s_j, s_j + L), s_j = j hop - L / 2 (integer division).  For tau = 1 .. tau_max:
 *   d(tau) = sum_{n = 0}^{win - 1} (x[s_j + n] - x[s_j + n + tau])^2      the squared differences themselves, in fp32
 *   c(0) = 1,  c(tau) = d(tau) tau / sum_{k = 1}^{tau} d(k),  1 where that sum is 0 (a constant frame)
 *   tau_0   the smallest tau in [tau_min, tau_max] with c(tau) < threshold.  Found: the frame is VOICED and tau* is
 *           where the walk `while tau + 1 <= tau_max and c(tau + 1) < c(tau)` from tau_0 stops.  None: the frame is
 *           UNVOICED and tau* is the smallest tau of the range that attains the minimum of c.
 *   refinement, only where 1 <= tau* - 1, tau* + 1 <= tau_max and c(tau*) <= both neighbours:
 *           tau* + (c(tau* - 1) - c(tau* + 1)) / (2 (c(tau* - 1) - 2 c(tau*) + c(tau* + 1))), offset 0 where the
 *           denominator is 0; tau* otherwise.  |refined - tau*| <= 1/2.
 *   period  DEVICE (batch, F) fp32: the refined period in samples of a voiced frame, exactly 0.0f for an unvoiced one
 *   aper    DEVICE (batch, F) fp32: c(tau*)
 *   cmnd    DEVICE (batch, F, tau_max + 1) fp32: c(0 .. tau_max) of every frame; NULL: not formed in memory, not written
 *   scratch DEVICE, mvn_pitch_scratch_floats(...) floats (the decoded signal), required with either entry
 * Fixed order, no atomics: the same inputs give the same bits on every call; a row's results do not depend on the other
 * rows of the launch; a non-finite sample affects only the frames whose span contains it.
 * MVN_ERR_BAD_ARG before any launch, with nothing written: both or neither of index / wave; period, aper or scratch
 * NULL; win outside [16, 4096]; tau_max outside [2, 1024]; tau_min outside [1, tau_max]; hop outside [1, 2^24];
 * threshold not in (0, 1] (NaN included); classes < 2 with index; batch < 0 or above 65535; n_samples < 1 or above
 * 2^30; batch * n_samples above 2^31 - 1; a scratch that is too small.  batch == 0 is MVN_OK and launches nothing. */
size_t mvn_pitch_scratch_floats(int batch, int n_samples, int win, int tau_max);
int mvn_pitch_frames(const int32_t *index, const float *wave, int batch, int n_samples, int classes, int win, int hop,
                     int tau_min, int tau_max, float threshold, float *period, float *aper, float *cmnd,
                     float *scratch, size_t scratch_floats, void *stream);

/* mvn_pitch_distance: two period tracks (batch, frames) fp32, DEVICE, read only, as mvn_pitch_frames writes them (a
 * frame is voiced where its period is above 0); first, count (batch) int32, DEVICE.  Over the frames
 * [first[s], first[s] + count[s]) of sequence s, clamped to [0, frames):
 *   both    frames voiced in a and in b;    vuv   frames voiced in exactly one of them
 *   e_f     1200 log2(period_b / period_a) in double on the `both` frames
 *   gross   the `both` frames with |period_a / period_b - 1| > gross_ratio
 *   rmse_cents[s] = sqrt(sum e_f^2 / both), 0.0 where both == 0      DEVICE (batch) double
 *   counts  DEVICE (batch, 4) int32: both, vuv, gross, the clamped count
 * Sums in double in a fixed order, no atomics; no frame outside a span is read.
 * MVN_ERR_BAD_ARG before any launch: a null pointer, batch or frames below 1, batch above 65535, gross_ratio not finite
 * or <= 0. */
int mvn_pitch_distance(const float *period_a, const float *period_b, int batch, int frames, const int32_t *first,
                       const int32_t *count, double gross_ratio, double *rmse_cents, int32_t *counts, void *stream);

/* ---- A pitch track as two local-conditioning channels (csrc/pitch_features.hip; additive, ABI version unchanged;
 * DESIGN 4.5j) ----
 * mvn_pitch_features: period (batch, frames) fp32, DEVICE, read only, as mvn_pitch_frames writes it.  Frame j of a row
 * is voiced, v[j], where period[j] > 0 (0, a negative value and NaN are unvoiced).  With
 *   lf[j] = (float) log2((double)rate / ((double)period[j] * (double)f_ref))                         for a voiced j,
 *   lf[j] = fmaf(a, lf[n], (1.0f - a) * lf[p]),  a = (float)(j - p) / (float)(n - p)                 for an unvoiced j
 * between p, the nearest voiced frame below it, and n, the nearest above it; lf of the first voiced frame in front of
 * it and of the last voiced frame behind it; 0 in a row without a voiced frame:
 *   out[b * row_stride + j]               = lf[j] + shift[b]       (shift: DEVICE (batch) fp32, octaves; NULL: zeros)
 *   out[b * row_stride + chan_stride + j] = v[j] ? 1.0f : 0.0f
 * Strides in floats: row_stride = (M + 2) * ld, chan_stride = ld and out = base + M * ld write channels M and M + 1 of
 * a (batch, M + 2, ld) tensor; nothing but those 2 * frames words of a sequence is written.  `out` must not overlap
 * `period`.  One workgroup per row, fixed order, no atomics: the same bits on every call and at every batch position.
 * MVN_ERR_BAD_ARG before any launch, with nothing written: period or out NULL; frames < 1 or above 2^30; batch < 0 or
 * above 65535; rate or f_ref not finite and above 0 (NaN included); chan_stride < frames; with batch > 1, row_stride <
 * chan_stride + frames.  batch == 0 is MVN_OK and launches nothing. */
int mvn_pitch_features(const float *period, int batch, int frames, float rate, float f_ref, const float *shift,
                       float *out, long long row_stride, long long chan_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOVENET_HIP_H */
