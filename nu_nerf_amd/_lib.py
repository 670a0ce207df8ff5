"""ctypes binding of libnunerf.so (the C-ABI drop-in boundary, include/nu_nerf.h).

The product path has no CPU fallback: if the HIP library is missing or a GPU is absent, the ops
raise.  `import torch` happens first so that the library binds to the HIP runtime torch already
loaded (one runtime => torch's hipStream_t handles are valid inside the library).

include/nu_nerf.h is the one description of the ABI; nothing of it is written a second time in Python:
  - every `typedef struct NuX { ... } NuX;` becomes the ctypes.Structure `X` of this module (NuGemmNT -> GemmNT), fields in header
    order; every enumerator and every integer `#define` becomes a module constant under its C name (NU_EPI_* also as EPI_*).
    This happens at import and needs neither the built library nor a GPU;
  - every `nu_*` entry gets its argtypes / restype when the library loads, and an errcheck that raises NuNerfLibraryError on a
    negative (NU_ERR_*) result: call sites pass plain values (device addresses as ints, None for NULL) and never check return codes;
  - load() compares ctypes.sizeof of every generated struct with the `nu_<name>_size()` the library was compiled with.
A construct of the header the reader does not map is an error (NuNerfLibraryError), never skipped.
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


# the only scalar types the header uses; every pointer and hipStream_t is a c_void_p
_SCALARS = {"int": c_int, "long long": c_ll, "unsigned long long": ctypes.c_ulonglong, "float": c_f, "double": ctypes.c_double}
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


def _read_header():
    """(declarations, object-like macros) of the header: comments, line continuations and preprocessor lines removed."""
    with open(_HEADER) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).replace("\\\n", " ")
    macros = {k: v.strip() for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(.*)$", text, flags=re.M)}
    return re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M), macros


def _constants(text, macros):
    """name -> value of every integer `#define` and every enumerator."""
    out = {k: int(v.strip("()")) for k, v in macros.items() if re.fullmatch(r"\(?-?\d+\)?", v)}
    for body in re.findall(r"\benum\s+\w*\s*\{([^{}]*)\}", text):
        value = -1
        for item in filter(None, (i.strip() for i in body.split(","))):
            m = re.fullmatch(r"(\w+)(?:\s*=\s*(-?\d+))?", item)
            if m is None:
                raise NuNerfLibraryError(f"enumerator {item!r} is not of the form NAME or NAME = integer")
            value = value + 1 if m.group(2) is None else int(m.group(2))
            out[m.group(1)] = value
    return out


def _structs(text, constants):
    """short name -> ctypes.Structure of every `typedef struct NuX { ... } NuX;` of `text`, in order (a struct may hold earlier ones).
    Per declarator as in C: a `*` makes a c_void_p, `[n]` an array (n a literal or a name in `constants`)."""
    out = {}
    for cname, body, alias in re.findall(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        if cname != alias or not cname.startswith("Nu"):
            raise NuNerfLibraryError(f"struct {cname}: expected `typedef struct NuX {{ ... }} NuX;`, found the typedef name {alias}")
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *rest = decl.split(",")
            m = re.fullmatch(r"(?:const\s+)?([\w\s]+?)\s*(\**\s*\w+\s*(?:\[.*\])?)", first.strip())
            if m is None:
                raise NuNerfLibraryError(f"struct {cname}: field declaration {decl!r} has a shape the binding does not map")
            base = " ".join(m.group(1).split())
            for declarator in [m.group(2)] + rest:
                d = re.fullmatch(r"(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?", declarator.strip())
                if d is None:
                    raise NuNerfLibraryError(f"struct {cname}: declarator {declarator.strip()!r} has a shape the binding does not map")
                stars, field, bound = d.groups()
                if stars:
                    ctype = c_p
                elif base in _SCALARS:
                    ctype = _SCALARS[base]
                elif base.startswith("Nu") and base[2:] in out:
                    ctype = out[base[2:]]
                else:
                    raise NuNerfLibraryError(f"struct {cname}: field {field} has the type {base!r}, which the binding does not map")
                if bound is not None:
                    n = int(bound) if bound.isdigit() else constants.get(bound, 0)
                    if n <= 0:
                        raise NuNerfLibraryError(f"struct {cname}: field {field} has the array bound {bound}, which is no positive "
                                                 "integer literal or #define of the header")
                    ctype = ctype * n
                fields.append((field, ctype))
        out[cname[2:]] = type(cname[2:], (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{cname} of include/nu_nerf.h."})
    opened = re.findall(r"\b(?:struct|union)\s*(\w*)\s*\{", text)
    if len(opened) != len(out):
        raise NuNerfLibraryError(f"struct / union bodies {opened}: only {['Nu' + k for k in out]} have the form the binding maps")
    return out


def _signatures():
    """(name, restype, argtypes) of every nu_* function the header declares."""
    # object-like macros stand for parameter lists (NU_RM_ARGS)
    text = re.sub(r"\b\w+\b", lambda m: _MACROS.get(m.group(0), m.group(0)), _TEXT)
    out = []
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(nu_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = " ".join(ret.split())
        if ret not in _RESTYPES:
            raise NuNerfLibraryError(f"{name}: return type {ret!r} is not one the binding maps")
        decls = [] if params.strip() in ("", "void") else params.split(",")
        out.append((name, _SCALARS[ret], [_param_type(name, d) for d in decls]))
    return out


_TEXT, _MACROS = _read_header()
CONSTANTS = _constants(_TEXT, _MACROS)
STRUCTS = _structs(_TEXT, CONSTANTS)
globals().update(CONSTANTS)
globals().update({k[3:]: v for k, v in CONSTANTS.items() if k.startswith("NU_EPI_")})
globals().update(STRUCTS)
_NO_SIZE_ENTRY = ("Lin",)        # never crosses the boundary on its own: checked through NuSdfNet


def _abi_key(name):
    """What pairs a struct with its size entry: NuGemmNT <-> nu_gemm_nt_size, both "gemmnt"."""
    return name.lower().replace("_", "").removeprefix("nu").removesuffix("size")


def _errcheck(rc, fn, args):
    if rc < 0:
        raise NuNerfLibraryError(f"{fn.__name__} failed with code {rc}")
    return rc


def load():
    """Load libnunerf.so, bind every entry of include/nu_nerf.h and check every struct's compiled size; raise loudly when it has
    not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise NuNerfLibraryError(
                f"{_LIB_PATH} not found: build it with `python -m nu_nerf_amd.build` "
                "(there is no CPU fallback for the product path)")
        lib = ctypes.CDLL(_LIB_PATH)
        size_entries = {}
        for name, restype, argtypes in _signatures():
            if not hasattr(lib, name):
                raise NuNerfLibraryError(f"{_LIB_PATH} does not export {name}, which include/nu_nerf.h declares")
            fn = getattr(lib, name)
            fn.restype, fn.argtypes, fn.errcheck = restype, argtypes, _errcheck
            if name.endswith("_size"):
                size_entries[_abi_key(name)] = fn
        for short, cls in STRUCTS.items():
            fn = size_entries.pop(_abi_key("Nu" + short), None)
            if fn is None and short not in _NO_SIZE_ENTRY:
                raise NuNerfLibraryError(f"include/nu_nerf.h declares no nu_*_size entry for struct Nu{short}")
            if fn is not None and fn() != ctypes.sizeof(cls):
                raise NuNerfLibraryError(f"struct Nu{short}: {fn.__name__}() = {fn()} bytes as compiled into {_LIB_PATH}, "
                                         f"{ctypes.sizeof(cls)} as read from include/nu_nerf.h")
        if size_entries:
            raise NuNerfLibraryError(f"size entries that match no struct of include/nu_nerf.h: {sorted(size_entries)}")
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
