"""ctypes binding of libnunerf.so (the C-ABI drop-in boundary, include/nu_nerf.h).

The product path has no CPU fallback: if the HIP library is missing or a GPU is absent, the ops
raise.  `import torch` happens first so that the library binds to the HIP runtime torch already
loaded (one runtime => torch's hipStream_t handles are valid inside the library).

Every `nu_*` entry the header declares gets its argtypes / restype from the header when the library
loads, and an errcheck that raises NuNerfLibraryError on a negative (NU_ERR_*) result: call sites pass
plain values (device addresses as ints, None for NULL) and never check return codes themselves.
"""
import ctypes
import os
import re

import torch  # noqa: F401  (must precede CDLL: see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# NU_NERF_LIB: another build of the same C ABI (development A/B runs of two kernel generations in one call); default: the in-tree library
_LIB_PATH = os.environ.get("NU_NERF_LIB") or os.path.join(_HERE, "libnunerf.so")
_HEADER = os.path.join(_HERE, "..", "include", "nu_nerf.h")
_lib = None

c_int = ctypes.c_int
c_ll = ctypes.c_longlong
c_f = ctypes.c_float
c_p = ctypes.c_void_p


class NuNerfLibraryError(RuntimeError):
    pass


def lib_path():
    return _LIB_PATH


# the only scalar types the header's signatures use; every pointer and hipStream_t is a c_void_p
_SCALARS = {"int": c_int, "long long": c_ll, "float": c_f, "double": ctypes.c_double}
_RESTYPES = ("int", "long long")


def _param_type(fn, decl):
    """ctypes type of one parameter declaration of `fn` ("const float* A", "long long workspace_bytes", "int")."""
    if "*" in decl:
        return c_p
    words = [w for w in decl.split() if w != "const"]
    for spelling in (" ".join(words), " ".join(words[:-1])):       # unnamed, then named
        if spelling == "hipStream_t":
            return c_p
        if spelling in _SCALARS:
            return _SCALARS[spelling]
    raise NuNerfLibraryError(f"{fn}: parameter {decl.strip()!r} has a type the binding does not map")


def _signatures():
    """(name, restype, argtypes) of every nu_* function the header declares."""
    with open(_HEADER) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).replace("\\\n", " ")
    # object-like macros stand for parameter lists (NU_RM_ARGS); every other preprocessor line goes
    macros = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(.*)$", text, flags=re.M))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r"\b\w+\b", lambda m: macros.get(m.group(0), m.group(0)), text)
    out = []
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(nu_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = " ".join(ret.split())
        if ret not in _RESTYPES:
            raise NuNerfLibraryError(f"{name}: return type {ret!r} is not one the binding maps")
        decls = [] if params.strip() in ("", "void") else params.split(",")
        out.append((name, _SCALARS[ret], [_param_type(name, d) for d in decls]))
    return out


def _errcheck(rc, fn, args):
    if rc < 0:
        raise NuNerfLibraryError(f"{fn.__name__} failed with code {rc}")
    return rc


def load():
    """Load libnunerf.so and bind every entry of include/nu_nerf.h; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise NuNerfLibraryError(
                f"{_LIB_PATH} not found: build it with `python -m nu_nerf_amd.build` "
                "(there is no CPU fallback for the product path)")
        lib = ctypes.CDLL(_LIB_PATH)
        for name, restype, argtypes in _signatures():
            if not hasattr(lib, name):
                raise NuNerfLibraryError(f"{_LIB_PATH} does not export {name}, which include/nu_nerf.h declares")
            fn = getattr(lib, name)
            fn.restype, fn.argtypes, fn.errcheck = restype, argtypes, _errcheck
        _lib = lib
    return _lib


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return c_p(0)
    return c_p(t.data_ptr())


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream(device_index=None):
    """The current HIP stream of torch as a void* (what every launch of the library takes).  `torch.cuda.current_stream()` builds
    a Python Stream object per call (~6 us, hundreds of calls per step); the raw getter returns the same handle in ~0.3 us."""
    if _raw_stream is not None:
        return c_p(_raw_stream(torch.cuda.current_device() if device_index is None else device_index))
    return c_p(torch.cuda.current_stream(device_index).cuda_stream)


def check(rc, what):
    if rc != 0:
        raise NuNerfLibraryError(f"{what} failed with code {rc}")


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NuNerfLibraryError("nu_nerf_amd ops need CUDA(HIP) tensors: there is no CPU fallback")
