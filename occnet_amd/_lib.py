"""ctypes binding of the C ABI in include/occnet_amd.h (and the headers of EXTENSION_HEADERS).

The product path has no CPU fallback: if libocc_amd.so is missing or an entry point is absent this
module raises at import/use time.  torch is imported first so the HIP runtime already loaded by
PyTorch-ROCm is the one our library binds to (same process, same streams).
"""
import ctypes
import os
import re

import torch  # noqa: F401  (loads libamdhip64 before our library)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libocc_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "occnet_amd.h")
# headers whose prototypes lib() binds besides the main one's: extensions of the C ABI that leave occnet_amd.h as it is
EXTRA_HEADERS = (os.path.join(os.path.dirname(_HERE), "include", "occnet_amd_visibility.h"),)
INPUT_HEADER = os.path.join(os.path.dirname(_HERE), "include", "occnet_amd_input.h")
DVR_HEADER = os.path.join(os.path.dirname(_HERE), "include", "occnet_amd_dvr.h")
EXTENSION_HEADERS = EXTRA_HEADERS + (INPUT_HEADER, DVR_HEADER)      # all of them; EXTRA_HEADERS stays the visibility header alone


class OccAmdError(RuntimeError):
    """Raised when a C-ABI entry point reports failure (mirror of TORCH_CHECK exceptions)."""


class OccAmdUnsupported(OccAmdError):
    """The shape has no fused kernel; the caller must take the unfused HIP path."""


def declared_symbols(header=HEADER_PATH):
    """Names of every function declared in the public header."""
    with open(header) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(occ_[a-z0-9_]+)\s*\(", src)))


# every scalar type of the header; anything with a '*' is a pointer, any other type is refused (prototypes)
_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "unsigned": ctypes.c_uint,
            "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}


class DevicePtr(ctypes.c_void_p):
    """argtypes entry of every pointer parameter: whatever c_void_p takes (None, an int, a c_void_p, a ctypes array,
    byref(...)), and a torch.Tensor, passed as its data_ptr()."""

    @classmethod
    def from_param(cls, v):
        if isinstance(v, torch.Tensor):
            return ctypes.c_void_p(v.data_ptr())
        return ctypes.c_void_p.from_param(v)


def prototypes(src=None):
    """{name: (restype, [(ctype, parameter name), ...])} of every function the header text `src` declares (None: the public
    header).  The header is the single source of the binding's types: a type this table does not know raises OccAmdError
    naming the prototype, so that a new one gets a deliberate mapping."""
    if src is None:
        with open(HEADER_PATH) as f:
            src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)

    def ctype(name, text, what):
        words = [w for w in text.replace("*", " * ").split() if w != "const"]
        if "*" in words:
            return ctypes.c_char_p if what == "return value" and words == ["char", "*"] else DevicePtr
        if " ".join(words) not in _SCALARS:
            raise OccAmdError(f"{name}: no ctypes mapping for the type {text.strip()!r} of its {what} (see _lib._SCALARS)")
        return _SCALARS[" ".join(words)]

    out = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(occ_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        args = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            m = re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", p, flags=re.S)
            if m is None:
                raise OccAmdError(f"{name}: cannot read the parameter {p.strip()!r}")
            args.append((ctype(name, m.group(1), f"parameter {m.group(2)!r}"), m.group(2)))
        out[name] = (ctype(name, ret, "return value"), args)
    return out


_lib = None
ABI = 3     # include/occnet_amd.h: bumped whenever a signature changes (2: range scales of the fp16 value rows; 3: their weight terms in device memory)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OccAmdError(
                f"{LIB_PATH} not found: build it with `python -m occnet_amd.build` "
                "(the MI355X path has no CPU fallback)")
        _lib = ctypes.CDLL(LIB_PATH)
        protos = prototypes()
        for header in EXTENSION_HEADERS:
            with open(header) as f:
                protos.update(prototypes(f.read()))
        for name, (restype, args) in protos.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = restype, [t for t, _ in args]
        if _lib.occ_abi_version() != ABI:
            got, _lib = _lib.occ_abi_version(), None
            raise OccAmdError(f"{LIB_PATH} has C ABI {got}, this package binds ABI {ABI}: rebuild it "
                              "(`python -m occnet_amd.build`)")
    return _lib


def check(rc, what):
    if rc == 0:
        return
    msg = lib().occ_last_error().decode()
    if rc == -3:
        raise OccAmdUnsupported(f"{what}: {msg}")
    raise OccAmdError(f"{what} failed (code {rc}): {msg}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


i32 = ctypes.c_int
i64 = ctypes.c_int64
f32 = ctypes.c_float
