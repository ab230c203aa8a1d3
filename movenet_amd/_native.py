"""ctypes binding of libmovenet_hip.so (the C ABI in include/movenet_hip.h).

There is deliberately NO fallback: if the library is missing or fails to load,
every entry point raises ``NativeLibraryError`` -- the product never routes
through PyTorch ops or the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

# MOVENET_HIP_LIB selects another build of the SAME library (the diagnostic twin with
# in-kernel stamps); it is not a fallback mechanism.
LIB_PATH = os.environ.get("MOVENET_HIP_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "lib", "libmovenet_hip.so")

MVN_OK = 0
MVN_ERR_BAD_DIMS = -1
MVN_ERR_BAD_ARG = -2
MVN_ERR_TOO_SHORT = -3
MVN_ERR_LAUNCH = -4
MVN_ERR_UNSUPPORTED = -5

GEN_AUTO, GEN_GENERIC, GEN_STREAM, GEN_PIPE, GEN_PIPE_F16, GEN_FOLD = 0, 1, 2, 3, 4, 5
BWD_FORM_GENERIC, BWD_FORM_HALVES, BWD_FORM_ONE = 1, 2, 3  # mvn_last_backward_form (include/movenet_hip.h)
BWD_FORM_BF16 = 4  # mvn_backward_bf16's layer kernel
BLOCK_FORM_GENERIC, BLOCK_FORM_FUSED64 = 1, 2  # mvn_block_last_form: the kernel form of the last block call
BWD_FORM_ONE_GLOBAL = 5  # mvn_backward_global: BWD_FORM_ONE with the label's row sums of df | dg
BWD_FORM_BF16_GLOBAL = 6  # mvn_backward_bf16_global: BWD_FORM_BF16 with the row sums formed inside the layer kernel
BWD_FORM_BF16_CTX = 7  # mvn_backward_bf16_ctx: BWD_FORM_BF16 writing df | dg for the fp32 context pass
# mvn_last_embed_form: the embedding gradient's kernel form in the last backward (include/movenet_hip.h)
EMBED_FORM_DENSE, EMBED_FORM_MFMA, EMBED_FORM_LDS, EMBED_FORM_TABLES, EMBED_FORM_ATOMICS = 1, 2, 3, 4, 5
SAMPLE_REFERENCE, SAMPLE_MODEL = 0, 1  # mvn_generate_ex's rule of a sampled step (include/movenet_hip.h)
SAMPLING_RULES = {"reference": SAMPLE_REFERENCE, "model": SAMPLE_MODEL}
LOSS_REFERENCE, LOSS_MODEL = 0, 1  # mvn_softmax_ce_*_ex's loss rule (include/movenet_hip.h)
LOSS_RULES = {"reference": LOSS_REFERENCE, "model": LOSS_MODEL}
PIPE_VARIANTS = (GEN_PIPE, GEN_PIPE_F16, GEN_FOLD)  # variants with a hand-off status word


class NativeLibraryError(RuntimeError):
    pass


class Dims(C.Structure):
    _fields_ = [
        ("layer_size", C.c_int32),
        ("stack_size", C.c_int32),
        ("input_channels", C.c_int32),
        ("residual_channels", C.c_int32),
        ("skip_channels", C.c_int32),
    ]


_PP = C.POINTER(C.c_void_p)


class Params(C.Structure):
    _fields_ = [
        ("causal_w", C.c_void_p),
        ("filter_w", _PP), ("gate_w", _PP),
        ("residual_w", _PP), ("residual_b", _PP),
        ("skip_w", _PP), ("skip_b", _PP),
        ("ctx_filter_w", _PP), ("ctx_filter_b", _PP),
        ("ctx_gate_w", _PP), ("ctx_gate_b", _PP),
        ("head1_w", C.c_void_p), ("head1_b", C.c_void_p),
        ("head2_w", C.c_void_p), ("head2_b", C.c_void_p),
    ]


_FP = C.POINTER(C.c_void_p)


class FwdBuffers(C.Structure):
    _fields_ = [("acts", C.c_void_p), ("th", C.c_void_p), ("sg", C.c_void_p), ("z", C.c_void_p),
                ("skip", C.c_void_p), ("a1", C.c_void_p), ("ctx", C.c_void_p), ("ctx_ld", C.c_int32),
                ("dense_audio", C.c_void_p), ("dense_ld", C.c_int32)]


class ParamGrads(C.Structure):
    _fields_ = [
        ("causal_w", C.c_void_p),
        ("filter_w", _PP), ("gate_w", _PP),
        ("residual_w", _PP), ("residual_b", _PP),
        ("skip_w", _PP), ("skip_b", _PP),
        ("head1_w", C.c_void_p), ("head1_b", C.c_void_p),
        ("head2_w", C.c_void_p), ("head2_b", C.c_void_p),
        ("ctx_filter_w", _PP), ("ctx_filter_b", _PP),
        ("ctx_gate_w", _PP), ("ctx_gate_b", _PP),
    ]


class BwdBuffers(C.Structure):
    _fields_ = [("dx_a", C.c_void_p), ("dx_b", C.c_void_p), ("dfg", C.c_void_p),
                ("dskip", C.c_void_p), ("da1", C.c_void_p), ("dlogit", C.c_void_p),
                ("dctx", C.c_void_p)]


class SeqSampling(C.Structure):
    """mvn_seq_sampling: the sampling settings of one sequence of a mvn_generate_seq launch (24 bytes)."""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("row", C.c_uint32),
                ("seed", C.c_uint64)]


class BlockTensor(C.Structure):
    """mvn_block_tensor: (batch, channels, len) behind ``p``, row stride ``ld`` floats, batch stride channels * ld."""
    _fields_ = [("p", C.c_void_p), ("ld", C.c_int32), ("len", C.c_int32)]


class BlockGatedParams(C.Structure):  # also used for mvn_block_gated_grads (same layout)
    _fields_ = [(n, C.c_void_p) for n in (
        "filter_w", "filter_b", "gate_w", "gate_b", "ctx_filter_w", "ctx_filter_b", "ctx_gate_w", "ctx_gate_b",
        "residual_w", "residual_b", "skip_w", "skip_b")]


_BT = C.POINTER(BlockTensor)
_BG = C.POINTER(BlockGatedParams)


class VideoParams(C.Structure):  # also used for mvn_video_grads (same layout)
    _fields_ = [("conv_w", C.c_void_p), ("conv_b", C.c_void_p),
                ("up_w", C.c_void_p * 3), ("up_b", C.c_void_p * 3)]


# name -> (restype, argtypes); tests/test_capi.py checks the header against this
SIGNATURES = {
    "mvn_abi_version": (C.c_int, []),
    "mvn_reload_switches": (C.c_int, []),
    "mvn_last_error": (C.c_char_p, []),
    "mvn_receptive_fields": (C.c_int, [C.POINTER(Dims)]),
    "mvn_output_size": (C.c_int, [C.POINTER(Dims), C.c_int]),
    "mvn_gen_variant": (C.c_int, [C.POINTER(Dims), C.c_int, C.c_int]),
    "mvn_gen_launch_pipelines": (C.c_int, [C.POINTER(Dims), C.c_int, C.c_int]),
    "mvn_gen_launch_is_cooperative": (C.c_int, []),
    "mvn_gen_weights_floats": (C.c_size_t, [C.POINTER(Dims), C.c_int]),
    "mvn_gen_state_floats": (C.c_size_t, [C.POINTER(Dims), C.c_int]),
    "mvn_gen_status_offset": (C.c_size_t, [C.POINTER(Dims), C.c_int]),
    "mvn_gen_pack_weights": (C.c_int, [C.POINTER(Dims), C.c_int, C.POINTER(Params), C.c_void_p,
                                       C.c_void_p]),
    "mvn_generate": (C.c_int, [C.POINTER(Dims), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                               C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvn_generate_ex": (C.c_int, [C.POINTER(Dims), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                  C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "mvn_generate_trunc": (C.c_int, [C.POINTER(Dims), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                     C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                     C.c_float, C.c_void_p]),
    "mvn_seq_sampling_check": (C.c_int, [C.POINTER(SeqSampling), C.c_int, C.c_int]),
    "mvn_generate_seq": (C.c_int, [C.POINTER(Dims), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "mvn_gen_guided_max_pairs": (C.c_int, [C.POINTER(Dims), C.c_int]),
    "mvn_generate_guided": (C.c_int, [C.POINTER(Dims), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "mvn_transpose_context": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p]),
    "mvn_padded_len": (C.c_int, [C.c_int]),
    "mvn_forward": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.c_void_p, C.c_int, C.c_int,
                              C.c_int, C.POINTER(FwdBuffers), C.c_void_p, C.c_int, C.c_int,
                              C.c_int, C.c_void_p]),
    "mvn_forward_f16": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.c_void_p, C.c_int, C.c_int,
                                  C.c_int, C.POINTER(FwdBuffers), C.c_void_p, C.c_int, C.c_int,
                                  C.c_int, C.c_void_p]),
    "mvn_backward": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.POINTER(ParamGrads),
                               C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FwdBuffers),
                               C.POINTER(BwdBuffers), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                               C.c_void_p]),
    "mvn_forward_bf16": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.c_void_p, C.c_int, C.c_int,
                                   C.c_int, C.POINTER(FwdBuffers), C.c_void_p, C.c_int, C.c_int,
                                   C.c_int, C.c_void_p]),
    "mvn_backward_bf16": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.POINTER(ParamGrads),
                                    C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FwdBuffers),
                                    C.POINTER(BwdBuffers), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_void_p]),
    "mvn_last_backward_form": (C.c_int, []),
    "mvn_last_embed_form": (C.c_int, []),
    "mvn_context_add_global": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mvn_global_fast_path": (C.c_int, [C.POINTER(Dims), C.c_int, C.c_int]),
    "mvn_global_bias": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvn_forward_global": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.POINTER(FwdBuffers), C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p, C.c_void_p]),
    "mvn_backward_global": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.POINTER(ParamGrads),
                                      C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FwdBuffers),
                                      C.POINTER(BwdBuffers), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mvn_backward_scratch": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.POINTER(ParamGrads),
                                       C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FwdBuffers),
                                       C.POINTER(BwdBuffers), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "mvn_global_scratch_floats": (C.c_size_t, [C.POINTER(Dims), C.c_int, C.c_int]),
    "mvn_global_bias_backward": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.POINTER(ParamGrads), C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvn_global_bf16_path": (C.c_int, [C.POINTER(Dims), C.c_int, C.c_int]),
    "mvn_global_bf16_scratch_floats": (C.c_size_t, [C.POINTER(Dims), C.c_int, C.c_int]),
    "mvn_forward_bf16_global": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.POINTER(FwdBuffers), C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_void_p, C.c_void_p]),
    "mvn_backward_bf16_global": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.POINTER(ParamGrads),
                                           C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FwdBuffers),
                                           C.POINTER(BwdBuffers), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mvn_bf16_ctx_path": (C.c_int, [C.POINTER(Dims), C.c_int, C.c_int]),
    "mvn_bf16_ctx_scratch_floats": (C.c_size_t, [C.POINTER(Dims), C.c_int, C.c_int]),
    "mvn_forward_bf16_ctx": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.POINTER(FwdBuffers), C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p]),
    "mvn_backward_bf16_ctx": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.POINTER(ParamGrads),
                                        C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FwdBuffers),
                                        C.POINTER(BwdBuffers), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "mvn_upsample_video": (C.c_int, [C.POINTER(Dims), C.POINTER(VideoParams), C.c_void_p, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_void_p]),
    "mvn_upsample_video_scratch_floats": (C.c_size_t, [C.POINTER(Dims), C.c_int, C.c_int]),
    "mvn_upsample_video_backward": (C.c_int, [C.POINTER(Dims), C.POINTER(VideoParams),
                                              C.POINTER(VideoParams), C.c_void_p, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mvn_gen_prime_from_forward": (C.c_int, [C.POINTER(Dims), C.POINTER(FwdBuffers), C.c_int,
                                             C.c_int, C.c_void_p, C.c_void_p]),
    "mvn_ce_parts": (C.c_int, [C.c_int, C.c_int]),
    "mvn_ce_on_probs_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "mvn_ce_on_probs_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvn_softmax_ce_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "mvn_softmax_ce_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p]),
    "mvn_softmax_ce_forward_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p]),
    "mvn_softmax_ce_backward_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                             C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_void_p]),
    # (the _ex pair and mvn_score_columns with a DEVICE array of per-sequence column counts before the stream)
    "mvn_softmax_ce_forward_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvn_softmax_ce_backward_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                              C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p, C.c_void_p]),
    "mvn_score_columns_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_void_p]),
    "mvn_score_scratch_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "mvn_score_columns": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.c_void_p]),
    "mvn_adamw_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float,
                                 C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                                 C.POINTER(C.c_size_t), C.c_int, C.c_void_p]),
    "mvn_adamw_ema_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                                     C.c_float, C.POINTER(C.c_size_t), C.c_int, C.c_void_p]),
    "mvn_mu_law_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "mvn_mu_law_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "mvn_pcm16_chunk": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                  C.c_void_p]),
    "mvn_pcm16_deemph_chunk": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mvn_onehot_to_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p]),
    "mvn_index_to_onehot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p]),
    "mvn_audio_frontend_scratch_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "mvn_audio_frontend": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvn_audio_frontend_var_scratch_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "mvn_audio_frontend_var": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvn_audio_frontend_window_scratch_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "mvn_audio_frontend_window": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # (form -- AUDIO_FORM_* below -- in front, the coefficient behind `normalize`, the emphasised waveform behind `index`)
    "mvn_audio_frontend_emph": (C.c_int, [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "mvn_video_frontend": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "mvn_publish_words": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_void_p]),
    # the five building blocks (csrc/blocks.hip)
    "mvn_block_last_form": (C.c_int, []),
    "mvn_block_conv_scratch_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvn_block_causal_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _BT, _BT, C.c_int, C.c_void_p]),
    "mvn_block_causal_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _BT, _BT, _BT, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mvn_block_dilated_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _BT, _BT, C.c_int, C.c_void_p]),
    "mvn_block_dilated_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _BT, _BT, _BT, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mvn_block_gated_scratch_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvn_block_gated_forward": (C.c_int, [_BG, C.c_int, C.c_int, C.c_int, _BT, _BT, _BT, _BT, _BT, _BT, C.c_int,
                                          C.c_void_p, C.c_size_t, C.c_void_p]),
    "mvn_block_gated_backward": (C.c_int, [_BG, _BG, C.c_int, C.c_int, C.c_int, _BT, _BT, _BT, _BT, _BT, _BT, _BT, _BT,
                                           C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mvn_block_dense_scratch_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvn_block_dense_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, _BT, _BT,
                                          _BT, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mvn_block_dense_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _BT, _BT, _BT, _BT, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                           C.c_void_p]),
    # local conditioning on log-mel frames (csrc/features.hip)
    "mvn_logmel_scratch_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvn_logmel_frontend": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "mvn_upsample_features_scratch_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mvn_upsample_features": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "mvn_upsample_features_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    # distance between two feature tensors (csrc/metrics.hip)
    "mvn_feature_distance_scratch_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "mvn_feature_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load (once) and return the library; raises NativeLibraryError loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: build it with `python -m movenet_amd.csrc.build` "
            "(or __graft_entry__.build()).  movenet_amd has no CPU/PyTorch fallback."
        )
    try:
        handle = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the box
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if handle.mvn_abi_version() != 2:
        raise NativeLibraryError("libmovenet_hip.so ABI version mismatch")
    _lib = handle
    return handle


def last_error() -> str:
    return lib().mvn_last_error().decode(errors="replace")


def check(rc: int, what: str) -> int:
    """Map a negative status to the exception type the reference would raise."""
    if rc >= 0:
        return rc
    msg = f"{what}: {last_error()} (status {rc})"
    if rc == MVN_ERR_TOO_SHORT:
        raise ValueError(last_error())  # movenet/wavenet.py:141-146
    if rc in (MVN_ERR_BAD_DIMS, MVN_ERR_BAD_ARG, MVN_ERR_UNSUPPORTED):
        raise ValueError(msg)
    raise RuntimeError(msg)


def sampling_rule(value) -> int:
    """"reference" / "model" -> MVN_SAMPLE_*; ValueError for anything else."""
    if not isinstance(value, str) or value not in SAMPLING_RULES:
        raise ValueError(f"sampling must be 'reference' or 'model', got {value!r}")
    return SAMPLING_RULES[value]


def loss_rule(value) -> int:
    """"reference" / "model" -> MVN_LOSS_*; ValueError for anything else."""
    if not isinstance(value, str) or value not in LOSS_RULES:
        raise ValueError(f"loss_rule must be 'reference' or 'model', got {value!r}")
    return LOSS_RULES[value]


def truncation(top_k, top_p):
    """(top_k, top_p) of mvn_generate_trunc as (int, float); ValueError unless top_k is an integer >= 0 (0: off) and
    top_p a number in (0, 1] (1: off; NaN refused)."""
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0 (0: off), got {top_k!r}")
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must lie in (0, 1] (1: off), got {top_p!r}")
    return int(top_k), float(top_p)


AUDIO_FORM_CLIP, AUDIO_FORM_VAR, AUDIO_FORM_WINDOW = 0, 1, 2  # MVN_AUDIO_FORM_* of mvn_audio_frontend_emph


def emphasis(value, name: str = "preemphasis") -> float:
    """The pre- / de-emphasis coefficient as the float32 value the kernels take; ValueError unless it is a number in
    [0, 1) (0: off; NaN refused)."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 <= value < 1.0 \
            or not C.c_float(value).value < 1.0:  # (a double just below 1 that rounds to 1.0f)
        raise ValueError(f"{name} must lie in [0, 1) (0: off), got {value!r}")
    return float(C.c_float(value).value)


def _per_sequence(value) -> bool:
    """True for what the generators take as one value per sequence: a list, tuple, numpy array or tensor that is
    not 0-dimensional."""
    if isinstance(value, (list, tuple)):
        return True
    return hasattr(value, "__len__") and hasattr(value, "tolist") and getattr(value, "ndim", 1) != 0


def any_per_sequence(*values) -> bool:
    return any(_per_sequence(v) for v in values)


def seq_sampling_array(batch: int, classes: int, temperature, top_k, top_p, seed, rows=None):
    """The checked HOST array of mvn_generate_seq, (SeqSampling * batch): ``temperature``, ``top_k``, ``top_p`` and
    ``seed`` each a scalar (the same for every sequence) or a 1-D sequence / tensor of length ``batch``; ``rows``
    (default: 0 .. batch - 1) the sequences' second Philox counter words.  ValueError for a wrong length or a value
    mvn_seq_sampling_check refuses (top_k < 0, top_p outside (0, 1]; the message names the row); every top_k >=
    ``classes`` comes back as 0.  Allocates nothing on a device."""
    batch = int(batch)

    def column(value, name, conv):
        if _per_sequence(value):
            value = value.tolist() if hasattr(value, "tolist") else list(value)
            if not isinstance(value, list) or any(isinstance(v, (list, tuple)) for v in value):
                raise ValueError(f"{name} must be a scalar or a 1-D sequence of length {batch}")
            if len(value) != batch:
                raise ValueError(f"{name} has {len(value)} entries for a batch of {batch}")
        else:
            value = [value] * batch
        out = []
        for b, v in enumerate(value):
            try:
                if isinstance(v, bool):
                    raise TypeError
                out.append(conv(v))
            except (TypeError, ValueError):
                raise ValueError(f"{name} of row {b} is {v!r}") from None
        return out

    def whole(v):
        if isinstance(v, float) and not v.is_integer():
            raise ValueError
        return int(v)

    cols = (column(temperature, "temperature", float), column(top_k, "top_k", whole), column(top_p, "top_p", float),
            column(seed, "seed", whole), column(list(range(batch)) if rows is None else rows, "rows", whole))
    for b, (k, r) in enumerate(zip(cols[1], cols[4])):
        if not -2 ** 31 <= k < 2 ** 31:
            raise ValueError(f"top_k of row {b} is {k!r}")
        if not 0 <= r < 2 ** 32:
            raise ValueError(f"rows: row {b} is {r!r}, not a 32-bit counter word")
    arr = (SeqSampling * max(batch, 1))()
    for b, (t, k, p, s, r) in enumerate(zip(*cols)):
        arr[b] = SeqSampling(t, k, p, r, s & (2 ** 64 - 1))
    rc = lib().mvn_seq_sampling_check(arr, batch, int(classes))
    if rc != MVN_OK:
        raise ValueError(last_error())
    return arr


def guidance_scales(batch: int, guidance):
    """The classifier-free guidance scales of ``batch`` sequences as a list of floats: ``guidance`` a number (the same
    for every sequence) or a 1-D sequence / tensor of ``batch`` numbers.  ValueError for a wrong length or a value that
    is not a finite number.  Allocates nothing on a device."""
    batch = int(batch)
    if _per_sequence(guidance):
        values = guidance.tolist() if hasattr(guidance, "tolist") else list(guidance)
        if not isinstance(values, list) or any(isinstance(v, (list, tuple)) for v in values):
            raise ValueError(f"guidance must be a number or a 1-D sequence of length {batch}")
        if len(values) != batch:
            raise ValueError(f"guidance has {len(values)} entries for a batch of {batch}")
    else:
        values = [guidance] * batch
    out = []
    for b, v in enumerate(values):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
            raise ValueError(f"guidance of row {b} is {v!r}, not a finite number")
        out.append(float(v))
    return out


def guided_max_pairs(dims, variant: int) -> int:
    """mvn_gen_guided_max_pairs: the pairs one guided launch of ``variant`` takes for ``dims`` (0: no guided form)."""
    return check(lib().mvn_gen_guided_max_pairs(dims, int(variant)), "mvn_gen_guided_max_pairs")


def make_dims(layer_size: int, stack_size: int, input_channels: int, residual_channels: int,
              skip_channels: int) -> Dims:
    return Dims(layer_size, stack_size, input_channels, residual_channels, skip_channels)


def ptr_array(ptrs: Sequence[int]):
    arr = (C.c_void_p * len(ptrs))(*ptrs)
    return arr, C.cast(arr, _PP)
