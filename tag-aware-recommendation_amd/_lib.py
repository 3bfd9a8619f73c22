"""ctypes binding of libtagrec_hip.so (the C ABI declared in include/tagrec.h).

The library is built in-tree by `__graft_entry__.build()` (hipcc, gfx950).  There
is deliberately no fallback: if the shared object is missing, or a call fails,
`TagrecError` is raised -- nothing here computes on the CPU.

include/tagrec.h is the only statement of the signatures: `load()` parses its prototypes and sets every function's
argtypes and restype from them, so a new entry point is declared in the header and wrapped where it is used, nothing
else.  A pointer parameter's argtype is one of a handful of classes (`Ptr` and its per-dtype subclasses) whose
`from_param` takes the tensor itself: a tensor whose dtype is not the header's pointee type, or one that is not on a
GPU, is refused with `ctypes.ArgumentError` before anything is launched.  Contiguity is not checked (strided slot views
with an `ld` argument are deliberate).  `ptr()` stays for raw callers and for the few deliberate reinterpretations.
"""
import ctypes
import os
import re
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtagrec_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "tagrec.h")       # where csrc/common.h includes it from
ABI_VERSION = 2

LOSS_SOFTPLUS = 0
LOSS_LOGSIGMOID = 1
LOSS_SOFTMAX = 2          # the multi-negative kernels (tagrec_rank_*) only


class TagrecError(RuntimeError):
    pass


def refuse_deterministic(config, model, not_covered):
    """Models without a fixed-order step refuse config["deterministic"] = True loudly instead of ignoring it."""
    if config.get("deterministic", False):
        raise TagrecError(f"{model}: deterministic=True is not covered (only the LightGCN and NGCF steps are): {not_covered}")


def refuse_ultragcn(config, what):
    """Every model but UltraGCN refuses the ug_* keys (and the "ultragcn" configuration) instead of ignoring them."""
    if config.get("model") == "ultragcn":
        raise TagrecError(f"{what}: the \"ultragcn\" configuration is not covered (weighted pointwise BCE on plain tables: "
                          "tagrec_amd.UltraGCN and BPR_training_data only)")
    keys = sorted(k for k in config if isinstance(k, str) and k.startswith("ug_"))
    if keys:
        raise TagrecError(f"{what}: {', '.join(keys)} belong to UltraGCN (get_config(\"ultragcn\")); this model does not read them")


def refuse_multi_negative(config, what):
    """Models and producers that consume (user, positive, one negative) triplets refuse n_negatives != 1, the "softmax"
    loss and negatives="in_batch" loudly instead of training on the first negative (only the LightGCN and NGCF steps and
    BPR_training_data are covered)."""
    if config.get("model") == "directau":
        raise TagrecError(f"{what}: the \"directau\" configuration is not covered (alignment / uniformity loss: tagrec_amd.DirectAU "
                          "and BPR_training_data only)")
    over = config.get("softmax_over", "negatives")
    if over != "negatives":
        raise TagrecError(f"{what}: softmax_over={over!r} is not covered (the softmax over the catalogue: the LightGCN and NGCF "
                          "steps and BPR_training_data only); it takes softmax_over=\"negatives\"")
    mask = config.get("catalogue_mask", "none")
    if mask != "none":
        raise TagrecError(f"{what}: catalogue_mask={mask!r} is not covered (it masks the softmax over the catalogue of the "
                          "LightGCN and NGCF steps); it takes catalogue_mask=\"none\"")
    neg = config.get("negatives", "sampled")
    if neg != "sampled":
        raise TagrecError(f"{what}: negatives={neg!r} is not covered (in-batch negatives: the LightGCN and NGCF steps and "
                          "BPR_training_data only); it takes negatives=\"sampled\"")
    k, loss = config.get("n_negatives", 1), config.get("mul_loss_func")
    if k != 1 or loss == "softmax":
        raise TagrecError(f"{what}: n_negatives={k!r} / mul_loss_func={loss!r} is not covered (multi-negative losses: the "
                          "LightGCN and NGCF steps and BPR_training_data only); it takes n_negatives=1 and softplus / logsigmoid")


class Ptr:
    """argtype of an untyped pointer parameter (void*, char*, a handle, a pointer to pointers): a GPU tensor of any
    dtype, None (NULL), an address as a plain int, or a ctypes object (c_void_p, byref(...), an array) as it is."""
    dtypes = None
    _ctypes = (ctypes._SimpleCData, ctypes.Array, ctypes._Pointer, type(ctypes.byref(c_int())))

    @classmethod
    def from_param(cls, v):
        if isinstance(v, torch.Tensor):
            if cls.dtypes is not None and v.dtype not in cls.dtypes:
                raise TypeError(f"expected a {' / '.join(map(str, cls.dtypes))} tensor, got {v.dtype}")
            if not v.is_cuda:
                raise TypeError(f"expected a GPU tensor (tagrec_amd has no CPU path), got one on {v.device}")
            return c_void_p(v.data_ptr())       # never the bare int: ctypes would pass it as a C int
        if v is None or isinstance(v, cls._ctypes):
            return v                            # ctypes passes None as NULL
        if type(v) is int:
            return c_void_p(v)
        raise TypeError(f"expected a tensor, None, an address or a ctypes object, got {type(v).__name__}")


class F32Ptr(Ptr):
    dtypes = (torch.float32,)


class F64Ptr(Ptr):
    dtypes = (torch.float64,)


class I64Ptr(Ptr):
    dtypes = (torch.int64,)


class I32Ptr(Ptr):
    dtypes = (torch.int32,)


class U8Ptr(Ptr):                       # no torch.bool: no caller passes one
    dtypes = (torch.uint8,)


class U32Ptr(Ptr):                      # counters are allocated as int32
    dtypes = (torch.int32, torch.uint32)


class U64Ptr(Ptr):
    dtypes = (torch.int64, torch.uint64)


# C type of include/tagrec.h (const dropped, the stars joined to the base type) -> argtype
_CTYPES = {"int": c_int, "int32_t": ctypes.c_int32, "int64_t": c_int64, "uint64_t": ctypes.c_uint64, "float": c_float,
           "double": ctypes.c_double,
           "float*": F32Ptr, "double*": F64Ptr, "int64_t*": I64Ptr, "int32_t*": I32Ptr, "int*": I32Ptr, "uint8_t*": U8Ptr,
           "unsigned*": U32Ptr, "uint64_t*": U64Ptr, "void*": Ptr, "char*": Ptr, "tagrec_graph*": Ptr,
           "float**": Ptr, "int32_t**": Ptr, "int64_t**": Ptr, "tagrec_graph**": Ptr}


def parse_header(text):
    """{name: (restype, argtypes)} of every `ret tagrec_name(args);` in the text of a header.  Not a C parser: a type is
    [const] word [const] stars, and whatever does not fit -- or a tagrec_ name the pattern did not reach -- is refused."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)            # comments, then preprocessor lines
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def ctype(decl, fn, ret=False):
        m = re.fullmatch(r"\s*(\w+)\s*((?:\*\s*)*)(\w+)?\s*", re.sub(r"\bconst\b", " ", decl))
        key = m and m.group(1) + "*" * m.group(2).count("*")
        if ret and key == "char*":                      # the one pointer the library returns: tagrec_last_error's text
            return c_char_p
        if key not in _CTYPES or (ret and issubclass(_CTYPES[key], Ptr)):
            raise TagrecError(f"include/tagrec.h: {fn}: no ctypes mapping for {' '.join(decl.split())!r}")
        return _CTYPES[key]

    protos = {}
    for ret, fn, args in re.findall(r"([\w\s*]+?)\b(tagrec_\w+)\(([^()]*)\)\s*;", text):
        protos[fn] = (ctype(ret, fn, True), [] if args.strip() == "void" else [ctype(a, fn) for a in args.split(",")])
    known = set(protos) | {k.rstrip("*") for k in _CTYPES}
    for m in re.finditer(r"\btagrec_\w+", text):
        if m.group() not in known:
            raise TagrecError(f"include/tagrec.h: {m.group()}: not a prototype this binding can read: "
                              f"{' '.join(text[m.start():m.start() + 200].split(';')[0].split())!r}")
    return protos


_protos = None


def _prototypes():
    global _protos
    if _protos is None:
        if not os.path.exists(HEADER_PATH):
            raise TagrecError(f"{HEADER_PATH} not found: the binding takes every signature from it")
        with open(HEADER_PATH) as f:
            _protos = parse_header(f.read())
    return _protos


_lib = None


def load():
    """Load the shared library once; raise TagrecError if it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TagrecError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  tagrec_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _prototypes().items():
        fn = getattr(lib, name)       # AttributeError here = header and library disagree
        fn.argtypes, fn.restype = argtypes, restype
    if lib.tagrec_abi_version() != ABI_VERSION:
        raise TagrecError(f"ABI mismatch: library {lib.tagrec_abi_version()}, host {ABI_VERSION}")
    _lib = lib
    return lib


def exported_symbols():
    return list(_prototypes())


def check(rc, what=""):
    if rc != 0:
        msg = load().tagrec_last_error().decode("utf-8", "replace")
        raise TagrecError(f"{what or 'tagrec call'} failed ({rc}): {msg}")


def stream_ptr():
    """torch's current HIP stream as the void* the ABI takes."""
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL), unchecked: for raw callers (tests, tools) and for the few places that
    hand a buffer to a parameter of another pointee type on purpose.  The package otherwise passes the tensor itself."""
    return c_void_p(0 if t is None else t.data_ptr())


def require_gpu_tensor(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TagrecError(f"{name}: expected a GPU tensor (tagrec_amd has no CPU path), got {type(t).__name__}"
                          f"{'' if not isinstance(t, torch.Tensor) else ' on ' + str(t.device)}")
    if t.dtype != dtype:
        raise TagrecError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise TagrecError(f"{name}: must be contiguous")
    return t
