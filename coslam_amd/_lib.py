"""ctypes loader of libcoslam_hip.so.  Fails loudly when the HIP library is missing: there is no
CPU fallback anywhere in this package (the oracle under oracle/ is test infrastructure only).

include/coslam_hip.h is the only declaration of the C interface: lib() reads it and sets restype and argtypes
of every function from it, so a call with the wrong number or kind of arguments is a Python exception before
the call and a device pointer goes across at full width without a wrapper at the call site."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# COSLAM_HIP_LIB: another build of the same library (A/B runs of two kernel variants on one GPU box)
LIB_PATH = os.environ.get("COSLAM_HIP_LIB") or os.path.join(_HERE, "lib", "libcoslam_hip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "coslam_hip.h")

_lib = None

# the scalar kinds of the header; everything with a '*' or a '[' in it, and the one function-pointer typedef, is a c_void_p:
# POINTER(struct) types would refuse the bare addresses (tensor.data_ptr()) and byref() objects that callers pass
_SCALARS = {"int": ctypes.c_int, "double": ctypes.c_double, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
            "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong}
_POINTER_TYPEDEFS = ("cs_ba_followup_fn",)


class CoslamHipError(RuntimeError):
    pass


def header_text():
    """include/coslam_hip.h without its comments and preprocessor lines"""
    if not os.path.exists(HEADER_PATH):
        raise CoslamHipError(f"{os.path.normpath(HEADER_PATH)} is missing: it is the declaration of the library's C interface")
    with open(HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    return re.sub(r"^\s*#.*$", "", txt, flags=re.M)


def _ctype(decl, fn, is_result=False):
    """the ctypes type of one parameter declaration (its name included) or of a result type"""
    if "*" in decl or "[" in decl:
        return ctypes.c_char_p if is_result and re.fullmatch(r"const\s+char\s*\*", decl) else ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if is_result and words == ["void"]:
        return None
    if words and words[0] in _POINTER_TYPEDEFS:
        return ctypes.c_void_p
    for kind in (" ".join(words), " ".join(words[:-1])):   # without and with a parameter name
        if kind in _SCALARS:
            return _SCALARS[kind]
    raise CoslamHipError(f"{fn}: no ctypes mapping for '{decl}' in {os.path.normpath(HEADER_PATH)}")


def declarations():
    """{name: (restype, [argtypes])} of every function include/coslam_hip.h declares"""
    txt = re.sub(r"\{[^{}]*\}", "", header_text().replace('extern "C" {', ""))   # struct and enum bodies (all flat)
    out = {}
    for stmt in txt.split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(cs_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if not m or stmt.lstrip().startswith("typedef"):
            continue
        res, fn, params = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        out[fn] = (_ctype(res, fn, is_result=True), [] if params == "void" else [_ctype(p.strip(), fn) for p in params.split(",")])
    return out


def lib():
    """Return the loaded CDLL.  PyTorch (when importable) is imported first so that this library and
    torch share one HIP runtime (same SONAME libamdhip64.so.7) and therefore one set of streams/devices."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CoslamHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  coslam_amd has no CPU fallback."
        )
    decls = declarations()
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64 first)
    except Exception:
        pass
    cdll = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for fn, (restype, argtypes) in decls.items():
        try:
            f = getattr(cdll, fn)
        except AttributeError:   # an older build given by COSLAM_HIP_LIB; tests/test_abi.py holds the tree's own library to the header
            continue
        f.restype, f.argtypes = restype, argtypes
    _lib = cdll
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().cs_last_error().decode("utf-8", "replace")
        raise CoslamHipError(f"{what} failed with code {rc}: {msg}")
