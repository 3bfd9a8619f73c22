"""The ctypes binding takes its signatures from include/tagrec.h (tagrec_amd._lib.parse_header) and checks tensors at the
boundary (the Ptr classes' from_param).  Host tests on a header written here and on CPU tensors; one GPU test that a
wrong-dtype tensor is refused before anything is launched."""
import ctypes
from ctypes import byref, c_char_p, c_float, c_int, c_int64, c_uint64, c_void_p

import pytest
import torch

import tagrec_amd as T

L = T._lib

HEADER = """
/* a header in the forms include/tagrec.h uses */
#ifndef X_H
#define X_H
#define TAGREC_OK 0   /* tagrec_not_a_function( */
typedef struct tagrec_graph tagrec_graph;
int tagrec_abi_version(void);
const char* tagrec_last_error(void);
int tagrec_device_info(int* n_cu, int* wave_size, char* arch, int arch_len);
int tagrec_graph_create(tagrec_graph** out, int64_t n_rows,
                        const int64_t* rowptr, const int32_t* colidx, const float* vals,
                        void* stream);   // multi-line
int64_t tagrec_graph_workspace(int64_t nnz);
int tagrec_spmm_axpy_sparse_f32(const tagrec_graph* g, const float* G_in, const uint8_t* in_flags /* may be NULL */,
                                const unsigned* in_count, float b_scale, int D, void* stream);
int tagrec_sum_n_f32(float* out, const float* const* srcs, int n_src, int64_t n, void* stream);
int tagrec_dropout_f32(const float* x, float* out, int64_t n, float p, uint64_t seed, void* stream);
int tagrec_cor_fwd_f32(const float* x, double* rowsum, uint64_t* seeds3, int32_t k);
#endif
"""


def test_parser_reads_every_prototype_form_of_the_header():
    P = L.parse_header(HEADER)
    assert list(P) == ["tagrec_abi_version", "tagrec_last_error", "tagrec_device_info", "tagrec_graph_create",
                       "tagrec_graph_workspace", "tagrec_spmm_axpy_sparse_f32", "tagrec_sum_n_f32", "tagrec_dropout_f32",
                       "tagrec_cor_fwd_f32"]
    assert P["tagrec_abi_version"] == (c_int, [])
    assert P["tagrec_last_error"] == (c_char_p, [])
    assert P["tagrec_device_info"] == (c_int, [L.I32Ptr, L.I32Ptr, L.Ptr, c_int])
    assert P["tagrec_graph_create"] == (c_int, [L.Ptr, c_int64, L.I64Ptr, L.I32Ptr, L.F32Ptr, L.Ptr])
    assert P["tagrec_graph_workspace"] == (c_int64, [c_int64])
    assert P["tagrec_spmm_axpy_sparse_f32"] == (c_int, [L.Ptr, L.F32Ptr, L.U8Ptr, L.U32Ptr, c_float, c_int, L.Ptr])
    assert P["tagrec_sum_n_f32"] == (c_int, [L.F32Ptr, L.Ptr, c_int, c_int64, L.Ptr])
    assert P["tagrec_dropout_f32"] == (c_int, [L.F32Ptr, L.F32Ptr, c_int64, c_float, c_uint64, L.Ptr])
    assert P["tagrec_cor_fwd_f32"] == (c_int, [L.F32Ptr, L.F64Ptr, L.U64Ptr, ctypes.c_int32])


@pytest.mark.parametrize("decl, names", [
    ("int tagrec_bad_f32(const float* x, size_t n, void* stream);", ("tagrec_bad_f32", "size_t n")),          # unknown type
    ("int tagrec_bad_f32(const float* x, unsigned int n);", ("tagrec_bad_f32", "unsigned int n")),            # two-word type
    ("float* tagrec_bad_f32(int n);", ("tagrec_bad_f32", "float*")),                                          # pointer return
    ("int tagrec_foo (const float* x);", ("tagrec_foo", "const float* x")),                                   # pattern misses it
    ("int tagrec_foo(void (*cb)(int), void* stream);", ("tagrec_foo",)),                                      # nested parentheses
])
def test_parser_refuses_what_it_cannot_read(decl, names):
    with pytest.raises(T.TagrecError) as e:
        L.parse_header(HEADER.replace("#endif", decl + "\n#endif"))
    for n in names:
        assert n in str(e.value)


def test_real_header_is_what_load_binds():
    lib, P = L.load(), L._prototypes()
    assert len(P) >= 150 and sorted(P) == sorted(L.exported_symbols())
    for name, (restype, argtypes) in P.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert P["tagrec_row_flags_f32"] == (c_int, [L.F32Ptr, c_int64, c_int, L.U8Ptr, L.U32Ptr, L.Ptr])
    assert {n for n, (r, _) in P.items() if r is c_int64} == {n for n in P if n.endswith(("_workspace", "_result", "_floats"))}


TYPED = [(L.F32Ptr, torch.float32), (L.F64Ptr, torch.float64), (L.I64Ptr, torch.int64), (L.I32Ptr, torch.int32),
         (L.U8Ptr, torch.uint8), (L.U32Ptr, torch.int32), (L.U32Ptr, torch.uint32), (L.U64Ptr, torch.int64),
         (L.U64Ptr, torch.uint64)]


@pytest.mark.parametrize("cls, dtype", TYPED)
def test_typed_pointer_refuses_dtype_first_then_device(cls, dtype):
    wrong = torch.float64 if dtype != torch.float64 else torch.float32
    with pytest.raises(TypeError) as e:
        cls.from_param(torch.zeros(4, dtype=wrong))
    assert str(wrong) in str(e.value) and str(cls.dtypes[0]) in str(e.value)
    with pytest.raises(TypeError, match="GPU tensor"):
        cls.from_param(torch.zeros(4, dtype=dtype))


def test_typed_pointer_dtype_sets():
    assert L.U8Ptr.dtypes == (torch.uint8,) and L.I32Ptr.dtypes == (torch.int32,)       # no bool, no widening
    assert L.U32Ptr.dtypes == (torch.int32, torch.uint32) and L.U64Ptr.dtypes == (torch.int64, torch.uint64)
    with pytest.raises(TypeError, match="torch.bool"):
        L.U8Ptr.from_param(torch.zeros(4, dtype=torch.bool))


@pytest.mark.parametrize("cls", [L.Ptr, L.F32Ptr, L.I64Ptr, L.U8Ptr])
def test_pointer_classes_hand_ctypes_objects_through(cls):
    five, ref, arr = c_void_p(5), byref(c_int64()), (c_void_p * 2)()
    assert cls.from_param(five) is five and cls.from_param(ref) is ref and cls.from_param(arr) is arr
    assert cls.from_param(None) is None                                          # ctypes hands None over as NULL
    seven = cls.from_param(7)
    assert isinstance(seven, c_void_p) and seven.value == 7                      # a pointer-wide 7, not a C int
    llabs = ctypes.CDLL(None).llabs              # what arrives in C: |x| of a 64-bit argument, a fresh function object
    llabs.argtypes, llabs.restype = [cls], ctypes.c_longlong
    assert [llabs(None), llabs(7), llabs(1 << 40), llabs(five)] == [0, 7, 1 << 40, 5]
    for bad in (7.0, "x", b"x", [1], True):
        with pytest.raises(TypeError):
            cls.from_param(bad)


def test_untyped_pointer_stops_at_the_device_check():
    with pytest.raises(TypeError, match="GPU tensor"):
        L.Ptr.from_param(torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(TypeError, match="GPU tensor"):
        L.Ptr.from_param(torch.zeros(8, dtype=torch.float64))


def test_refusal_reaches_the_caller_as_argument_error():
    """Through the library: ctypes wraps what from_param raises and names the argument; nothing is called."""
    lib = L.load()
    with pytest.raises(ctypes.ArgumentError, match=r"argument 1: TypeError: expected a torch.float32 tensor, got torch.int32"):
        lib.tagrec_row_flags_f32(torch.zeros(4, 8, dtype=torch.int32), 4, 8, None, None, None)
    with pytest.raises(ctypes.ArgumentError, match=r"argument 4: TypeError: expected a GPU tensor"):
        lib.tagrec_row_flags_f32(None, 4, 8, torch.zeros(4, dtype=torch.uint8), None, None)


@pytest.mark.gpu
def test_wrong_dtype_is_refused_before_launch():
    """One wrong-dtype CUDA tensor among otherwise valid arguments: ctypes.ArgumentError, and the sentinel-filled outputs
    are untouched after a synchronize (the call never reached the library)."""
    dev = torch.device("cuda:0")
    lib, s = L.load(), L.stream_ptr
    g = T.Graph(torch.tensor([0, 1, 2, 3, 4], device=dev), torch.tensor([1, 0, 3, 2], dtype=torch.int32, device=dev),
                torch.ones(4, device=dev), (4, 4))
    flags = torch.full((4,), 7, dtype=torch.uint8, device=dev)
    count = torch.full((1,), 7, dtype=torch.int32, device=dev)
    with pytest.raises(ctypes.ArgumentError, match="torch.float32.*torch.int32"):
        lib.tagrec_row_flags_f32(torch.ones(4, 8, dtype=torch.int32, device=dev), 4, 8, flags, count, s())
    with pytest.raises(ctypes.ArgumentError, match="torch.int64.*torch.int32"):
        lib.tagrec_graph_mark_rows_u8(g.handle, torch.tensor([0, 2], dtype=torch.int32, device=dev), 2, flags, s())
    x, inv = torch.ones(4, 8, device=dev), torch.ones(4, device=dev)
    dx = torch.full((4, 8), 7.0, device=dev)
    with pytest.raises(ctypes.ArgumentError, match="torch.float32.*torch.float64"):
        lib.tagrec_rownorm_bwd_f32(x, inv, torch.ones(4, 8, dtype=torch.float64, device=dev), 8, 1.0, dx, 0, 4, 8, s())
    torch.cuda.synchronize()
    assert bool((flags == 7).all()) and int(count) == 7 and bool((dx == 7.0).all())
    # the same three calls with the right dtypes run
    T._lib.check(lib.tagrec_row_flags_f32(torch.ones(4, 8, device=dev), 4, 8, flags, count, s()), "row_flags")
    torch.cuda.synchronize()
    assert flags.tolist() == [1, 1, 1, 1] and int(count) == 4
