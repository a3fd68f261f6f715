"""ctypes binding of libbbmap_amd.so (the C ABI declared in include/bbmap_amd.h).

There is no fallback: if the shared library is missing, loading raises; if no gfx950 device is
present, bbmsa_create() returns BBMAP_E_NODEVICE and the wrappers raise.
"""
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(HERE, "libbbmap_amd.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "bbmap_amd.h")


class BBMapAmdError(RuntimeError):
    pass


# The header is the one declaration of every entry point: load() reads its prototypes and types each function from them.
_BY_VALUE = {"int32_t": C.c_int32, "int": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32}
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "void": None, "const char *": C.c_char_p}


def parse_prototypes(text):
    """{name: (restype, argtypes)} of the bb*_ prototypes in header text.  A prototype reader for include/bbmap_amd.h, not a C parser:
    comments, preprocessor lines and struct / enum bodies go, and what is left is split at its semicolons.  Every pointer parameter is
    a c_void_p; a parameter or return type outside the two tables above raises and names the function."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r"\{[^{}]*\}", "", text)
    protos = {}
    for stmt in text.split(";"):
        m = re.fullmatch(r"(.*?)\b(bb[a-z]+_\w+)\s*\((.*)\)", stmt.strip(), re.S)
        if not m:
            continue
        ret, name, params = " ".join(m.group(1).replace("*", " * ").split()), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise BBMapAmdError("%s: no ctypes type for the return type %r" % (name, ret))
        argtypes = []
        for p in ([] if params == "void" else params.split(",")):
            words = [w for w in p.split() if w != "const"]
            kind = " ".join(words[:-1] if len(words) > 1 else words)         # (the last word is the parameter's name)
            if "*" in p or "[" in p:
                argtypes.append(C.c_void_p)
            elif kind in _BY_VALUE:
                argtypes.append(_BY_VALUE[kind])
            else:
                raise BBMapAmdError("%s: no ctypes type for the parameter %r" % (name, " ".join(p.split())))
        protos[name] = (_RETURNS[ret], argtypes)
    return protos


with open(HEADER) as _f:
    PROTOTYPES = parse_prototypes(_f.read())
EXPORTS = sorted(PROTOTYPES)          # every symbol include/bbmap_amd.h declares


class bbmsa_job(C.Structure):
    _fields_ = [("read_off", C.c_int64), ("ref_off", C.c_int64),
                ("read_len", C.c_int32), ("ref_len", C.c_int32),
                ("refStartLoc", C.c_int32), ("refEndLoc", C.c_int32),
                ("minScore", C.c_int32), ("flags", C.c_int32)]


class bbmsa_result(C.Structure):
    _fields_ = [("result", C.c_int32 * 5), ("status", C.c_int32), ("iterations", C.c_int64),
                ("score", C.c_int32 * 8), ("score_len", C.c_int32), ("match_len", C.c_int32),
                ("fill_kind", C.c_int32), ("columns", C.c_int32)]


class bbmsa_config(C.Structure):
    _fields_ = [("device", C.c_int32), ("maxRows", C.c_int32), ("maxColumns", C.c_int32),
                ("bandwidth", C.c_int32), ("bandwidthRatio", C.c_float), ("reserved", C.c_int32 * 3)]


class bbband_job(C.Structure):
    _fields_ = [("query_off", C.c_int64), ("ref_off", C.c_int64), ("query_len", C.c_int32), ("ref_len", C.c_int32),
                ("qstart", C.c_int32), ("rstart", C.c_int32), ("maxEdits", C.c_int32), ("flags", C.c_int32)]


class bbband_result(C.Structure):
    _fields_ = [("edits", C.c_int32), ("lastQueryLoc", C.c_int32), ("lastRefLoc", C.c_int32), ("lastRow", C.c_int32),
                ("lastEdits", C.c_int32), ("lastOffset", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


class bbband_config(C.Structure):
    _fields_ = [("device", C.c_int32), ("width", C.c_int32), ("semantics", C.c_int32), ("reserved", C.c_int32)]


_lib = None


def load():
    """Loads the HIP library and types every entry point from the header; raises if the library has not been built or lacks one."""
    global _lib
    if _lib is not None:
        return _lib
    so_path = os.environ.get("BBMAP_AMD_SO") or SO_PATH          # (experiments: a variant build, scripts/build_variant.py)
    if not os.path.exists(so_path):
        raise BBMapAmdError(
            "libbbmap_amd.so is missing (%s). Build it with `python -m bbmap_amd.build`; "
            "there is no CPU fallback." % so_path)
    L = C.CDLL(so_path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise BBMapAmdError("%s does not export %s, which include/bbmap_amd.h declares" % (so_path, name)) from None
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        raise BBMapAmdError("%s failed (%d): %s" % (what, rc, load().bbmap_last_error().decode()))
