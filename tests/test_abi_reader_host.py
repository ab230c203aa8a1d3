"""CPU: the reader that derives the ctypes binding from include/movenet_hip.h (movenet_amd/_native.py: read_header),
fed short header texts of its own: what it must take, and what it must refuse instead of guessing."""
import ctypes as C

import pytest

from movenet_amd import _native as N


def _signatures(text):
    return N.read_header(text)[1]


def test_prototype_over_several_lines_with_comments_between_parameters():
    sigs = _signatures("""
        /* leading comment with a decoy: int mvn_not_this(int x); */
        int mvn_three_lines(const mvn_dims *dims, /* the dims */
                            float *out,  // device
                            size_t n, void *stream);
        size_t mvn_sizing(int batch, int t_len); /* trailing */
    """)
    assert list(sigs) == ["mvn_three_lines", "mvn_sizing"]
    assert sigs["mvn_three_lines"] == (C.c_int, [C.POINTER(N.Dims), C.c_void_p, C.c_size_t, C.c_void_p])
    assert sigs["mvn_sizing"] == (C.c_size_t, [C.c_int, C.c_int])


def test_void_and_empty_parameter_lists():
    sigs = _signatures("int mvn_a(void);\nconst char *mvn_b();\nint mvn_c( void );")
    assert sigs == {"mvn_a": (C.c_int, []), "mvn_b": (C.c_char_p, []), "mvn_c": (C.c_int, [])}


def test_unnamed_parameters_and_every_scalar():
    sigs = _signatures("int mvn_u(int, float, size_t, long long, int32_t, uint64_t, unsigned long long, float *,"
                       " const mvn_params *, const long long *);")
    assert sigs["mvn_u"][1] == [C.c_int, C.c_float, C.c_size_t, C.c_longlong, C.c_int32, C.c_uint64, C.c_uint64,
                                C.c_void_p, C.POINTER(N.Params), C.c_void_p]
    named = _signatures("int mvn_u(int a, float b, size_t c, long long d, int32_t e, uint64_t f, unsigned long long g,"
                        " float *h, const mvn_params *i, const long long *j);")
    assert named == sigs


def test_const_on_either_side_of_the_type():
    sigs = _signatures("int mvn_k(const float *a, float const *b, const float *const *c, int const n,"
                       " mvn_block_tensor const *t, const size_t *ranges);")
    assert sigs["mvn_k"][1] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(N.BlockTensor),
                                C.POINTER(C.c_size_t)]


def test_structs_and_preprocessor_lines_hold_no_prototypes():
    sigs = _signatures("""
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define OTHER_CALL(x) mvn_macro(x);
        typedef struct mvn_thing { int32_t a; float *p; } mvn_thing;
        typedef struct { int64_t offset; int32_t height, width; } mvn_clip;
        int mvn_after(const mvn_clip *clips, const mvn_thing *thing);
        #ifdef __cplusplus
        }
        #endif
    """)
    assert sigs == {"mvn_after": (C.c_int, [C.c_void_p, C.c_void_p])}


def test_device_array_overrides_go_by_function_and_parameter_name():
    text = ("int mvn_seq_sampling_check(mvn_seq_sampling *host, int batch, int classes);\n"
            "int mvn_generate_seq(const mvn_seq_sampling *per_seq, const mvn_seq_sampling *other);\n"
            "int mvn_generate_guided(int pairs, const mvn_seq_sampling *per_seq);\n"
            "int mvn_elsewhere(const mvn_seq_sampling *per_seq);")
    sigs = _signatures(text)
    host = C.POINTER(N.SeqSampling)
    assert sigs["mvn_seq_sampling_check"][1] == [host, C.c_int, C.c_int]
    assert sigs["mvn_generate_seq"][1] == [C.c_void_p, host]      # by name, not by position or type
    assert sigs["mvn_generate_guided"][1] == [C.c_int, C.c_void_p]
    assert sigs["mvn_elsewhere"][1] == [host]                     # and by function


def test_defines():
    constants, sigs = N.read_header("""
        #define MVN_PLAIN 7
        #define MVN_TRAILING 3 /* a trailing comment */
        #define MVN_SLASHES 4 // another
        #define MVN_NEGATIVE (-5)   /* a comment that
                                       runs on */
        #define MVN_BARE_NEGATIVE -6
        #  define MVN_SPACED ( -1 )
        #define OTHER_PREFIX 9
        #define MOVENET_HIP_H
        /* #define MVN_COMMENTED_OUT 1 */
        int mvn_f(void);
    """)
    assert constants == {"MVN_PLAIN": 7, "MVN_TRAILING": 3, "MVN_SLASHES": 4, "MVN_NEGATIVE": -5,
                         "MVN_BARE_NEGATIVE": -6, "MVN_SPACED": -1}
    assert list(sigs) == ["mvn_f"]


@pytest.mark.parametrize("line", ["#define MVN_EXPR (1 << 4)", "#define MVN_FLOAT 0.5", "#define MVN_EMPTY",
                                  "#define MVN_MACRO(x) 3", "#define MVN_NAME MVN_OTHER"])
def test_a_define_that_is_no_integer_is_refused(line):
    with pytest.raises(N.NativeLibraryError, match="MVN_"):
        N.read_header(line + "\n")


@pytest.mark.parametrize("text, function, parameter", [
    ("int mvn_bad(int a, long n, void *stream);", "mvn_bad", "'n'"),                # a scalar it has no rule for
    ("int mvn_bad2(int a, double, void *stream);", "mvn_bad2", "parameter 1"),      # ... unnamed: by position
    ("int mvn_arr(float x[3]);", "mvn_arr", "parameter 0"),                         # an array declarator
    ("int mvn_fn(mvn_dims dims);", "mvn_fn", "'dims'"),                             # a struct by value
    ("long mvn_ret(int a);", "mvn_ret", "return type"),
    ("float *mvn_retp(int a);", "mvn_retp", "return type"),
    ("typedef int mvn_t(int a);", "mvn_t", "return type"),
])
def test_an_unknown_type_is_refused_with_function_and_parameter_named(text, function, parameter):
    with pytest.raises(N.NativeLibraryError) as e:
        N.read_header("int mvn_fine(int a);\n" + text)
    assert function + ":" in str(e.value) and parameter in str(e.value)


def test_a_name_declared_twice_is_refused():
    with pytest.raises(N.NativeLibraryError, match="mvn_twice is declared twice"):
        N.read_header("int mvn_twice(int a);\nint mvn_twice(int a, int b);")


def test_a_prototype_the_library_does_not_export_reaches_libs_own_error(monkeypatch):
    real = N.lib()  # (loaded before the table is swapped, so that the module's cached handle can be put back)
    sigs = _signatures("int mvn_abi_version(void);\nint mvn_declared_but_never_written(const mvn_dims *dims);")
    monkeypatch.setattr(N, "SIGNATURES", sigs)
    monkeypatch.setattr(N, "_lib", None)
    with pytest.raises(N.NativeLibraryError, match="does not export mvn_declared_but_never_written"):
        N.lib()
    monkeypatch.undo()
    assert N.lib() is real


def test_a_missing_header_is_an_error_with_its_path(monkeypatch, tmp_path):
    missing = str(tmp_path / "include" / "movenet_hip.h")
    monkeypatch.setattr(N, "HEADER_PATH", missing)
    with pytest.raises(N.NativeLibraryError) as e:
        N._read_header_file()
    assert missing in str(e.value)


def test_the_modules_constants_and_table_are_the_headers():
    with open(N.HEADER_PATH) as f:
        constants, sigs = N.read_header(f.read())
    assert sigs == N.SIGNATURES and len(sigs) >= 96
    for name, value in constants.items():
        python_name = name if name == "MVN_OK" or name.startswith("MVN_ERR_") else name[len("MVN_"):]
        assert getattr(N, python_name) == value, name
    assert N.ABI_VERSION == constants["MVN_ABI_VERSION"] == N.lib().mvn_abi_version()
    assert (N.MVN_OK, N.MVN_ERR_TOO_SHORT, N.GEN_FOLD, N.BWD_FORM_BF16_CTX, N.EMBED_FORM_TABLES, N.SAMPLE_MODEL,
            N.LOSS_MODEL, N.BLOCK_FORM_FUSED64, N.AUDIO_FORM_WINDOW) == (0, -3, 5, 7, 4, 1, 1, 2, 2)
