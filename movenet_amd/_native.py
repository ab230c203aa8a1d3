"""ctypes binding of libmovenet_hip.so, READ from the C ABI's header include/movenet_hip.h at import: every
``mvn_*`` prototype becomes a row of ``SIGNATURES`` and every ``#define MVN_* <integer>`` a module attribute.  Only
the struct layouts below are written out by hand (tests/test_abi_layout_host.py pins them to the header with a
compiler).  Importing this module needs the header, not the library and not a GPU.

There is deliberately NO fallback: if the library is missing or fails to load,
every entry point raises ``NativeLibraryError`` -- the product never routes
through PyTorch ops or the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional, Sequence

# MOVENET_HIP_LIB selects another build of the SAME library (the diagnostic twin with
# in-kernel stamps); it is not a fallback mechanism.
LIB_PATH = os.environ.get("MOVENET_HIP_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "lib", "libmovenet_hip.so")
# The contract; csrc/build.py compiles against this same file.
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "movenet_hip.h")


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


class VideoParams(C.Structure):  # also used for mvn_video_grads (same layout)
    _fields_ = [("conv_w", C.c_void_p), ("conv_b", C.c_void_p),
                ("up_w", C.c_void_p * 3), ("up_b", C.c_void_p * 3)]


# ---- the header reader: C declarations -> ctypes.  What it does not know it refuses; it never guesses. ----
_SCALARS = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "long long": C.c_longlong,
            "int32_t": C.c_int32, "uint64_t": C.c_uint64, "unsigned long long": C.c_uint64}
# `T *` for a T that Python fills in HOST memory is POINTER(its class); every other pointer -- device memory, the
# stream, the device-side descriptor arrays -- is a c_void_p.
_HOST_POINTEES = {"mvn_dims": Dims, "mvn_params": Params, "mvn_param_grads": ParamGrads, "mvn_fwd_buffers": FwdBuffers,
                  "mvn_bwd_buffers": BwdBuffers, "mvn_video_params": VideoParams, "mvn_video_grads": VideoParams,
                  "mvn_block_tensor": BlockTensor, "mvn_block_gated_params": BlockGatedParams,
                  "mvn_block_gated_grads": BlockGatedParams, "mvn_seq_sampling": SeqSampling,
                  "size_t": C.c_size_t}  # (mvn_adamw_step's skip_ranges)
# The exceptions to that rule, by (function, parameter name): these three take a DEVICE array of mvn_seq_sampling
# (only mvn_seq_sampling_check takes the host array), and one call takes a double by value (no rule for the type: a
# `double` anywhere else is still refused).
_OVERRIDES = {("mvn_generate_seq", "per_seq"): C.c_void_p, ("mvn_generate_guided", "per_seq"): C.c_void_p,
              ("mvn_generate_windowed", "per_seq"): C.c_void_p, ("mvn_pitch_distance", "gross_ratio"): C.c_double}


def _ctype(function: str, decl: str, position: Optional[int] = None):
    """The ctypes type of one declaration of ``function``: its parameter number ``position``, else its return type."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    stars, name = words.count("*"), ""
    if position is not None and len(words) > 1 and words[-1].isidentifier() and (
            stars or " ".join(words) not in _SCALARS):  # (the name is optional: `long long` has none)
        name = words.pop()
    base, kind = " ".join(words[:len(words) - stars]), None
    if base and words[len(words) - stars:] == ["*"] * stars:
        if position is None:
            kind = C.c_char_p if (base, stars) == ("char", 1) else None if stars else _SCALARS.get(base)
        elif (function, name) in _OVERRIDES:
            kind = _OVERRIDES[function, name]
        elif not stars:
            kind = _SCALARS.get(base)
        else:
            kind = C.POINTER(_HOST_POINTEES[base]) if stars == 1 and base in _HOST_POINTEES else C.c_void_p
    if kind is None:
        what = "the return type" if position is None else f"parameter {name!r}" if name else f"parameter {position}"
        raise NativeLibraryError(f"{function}: {what} is declared `{' '.join(decl.split())}`, which the header reader "
                                 "does not know (movenet_amd/_native.py)")
    return kind


def read_header(text: str):
    """A header's text as (constants, signatures): every ``#define MVN_NAME <integer>`` (the integer may stand in
    parentheses; a ``MVN_*`` macro of any other shape is refused) as {"MVN_NAME": value}, and every prototype
    ``<ret> mvn_name(<params>);`` as name -> (restype, [argtypes])."""
    lines = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).replace("\\\n", " ").split("\n")  # (no comments)
    constants, signatures, code = {}, {}, []
    for line in lines:
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        words = line.strip()[1:].split(None, 2)
        if words[:1] == ["define"] and len(words) > 1 and words[1].startswith("MVN_"):
            value = words[2].strip() if len(words) > 2 and words[1].isidentifier() else ""  # (no macro with arguments)
            if value.startswith("(") and value.endswith(")"):
                value = value[1:-1]
            try:
                constants[words[1]] = int(value)
            except ValueError:
                raise NativeLibraryError(f"`{line.strip()}` is not an integer constant") from None
    # (a statement runs from the last `;`, `{` or `}`: whatever stands in front of the name is the return type)
    for ret, name, params in re.findall(r"(?<![^;{}])([^;{}()]*)\b(mvn_\w+)\s*\(([^()]*)\)\s*;", "\n".join(code)):
        if name in signatures:
            raise NativeLibraryError(f"{name} is declared twice")
        params = [] if params.strip() in ("", "void") else params.split(",")
        signatures[name] = (_ctype(name, ret), [_ctype(name, p, i) for i, p in enumerate(params)])
    return constants, signatures


def _read_header_file():
    try:
        with open(HEADER_PATH, encoding="utf-8") as f:
            return read_header(f.read())
    except OSError as e:
        raise NativeLibraryError(f"cannot read the C ABI's header {HEADER_PATH}: {e}") from e


# SIGNATURES: name -> (restype, argtypes), one row per prototype of the header -- a new entry point needs no line here
_CONSTANTS, SIGNATURES = _read_header_file()
# MVN_OK and MVN_ERR_* under their own names, every other constant without the prefix: GEN_FOLD, BWD_FORM_BF16_CTX,
# EMBED_FORM_TABLES, SAMPLE_MODEL, LOSS_MODEL, BLOCK_FORM_FUSED64, AUDIO_FORM_WINDOW, ABI_VERSION, ...
globals().update((k if k == "MVN_OK" or k.startswith("MVN_ERR_") else k[len("MVN_"):], v)
                 for k, v in _CONSTANTS.items())
SAMPLING_RULES = {"reference": SAMPLE_REFERENCE, "model": SAMPLE_MODEL}  # noqa: F821
LOSS_RULES = {"reference": LOSS_REFERENCE, "model": LOSS_MODEL}  # noqa: F821
PIPE_VARIANTS = (GEN_PIPE, GEN_PIPE_F16, GEN_FOLD)  # noqa: F821  variants with a hand-off status word

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
    if handle.mvn_abi_version() != ABI_VERSION:  # noqa: F821
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
    if rc == MVN_ERR_TOO_SHORT:  # noqa: F821
        raise ValueError(last_error())  # movenet/wavenet.py:141-146
    if rc in (MVN_ERR_BAD_DIMS, MVN_ERR_BAD_ARG, MVN_ERR_UNSUPPORTED):  # noqa: F821
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
    if rc != MVN_OK:  # noqa: F821
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
