"""CPU-side checks of the C ABI: the library builds/loads and exports every declared symbol."""
import ctypes as C
import os
import re
import threading

import pytest

from bbmap_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "bbmap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(bb(?:map|msa|band|idx|pipe|keys)_[a-z0-9_]+)\s*\(", hdr)))


def test_library_builds_and_exports_every_declared_symbol():
    build.build()
    L = C.CDLL(_lib.SO_PATH)
    syms = declared_symbols()
    assert syms, "no symbols parsed from include/bbmap_amd.h"
    for s in syms:
        assert hasattr(L, s), "missing export: " + s
    assert sorted(_lib.EXPORTS) == syms


def test_struct_layouts_match_header():
    assert C.sizeof(_lib.bbmsa_job) == 40
    assert C.sizeof(_lib.bbmsa_result) == 80
    assert _lib.bbmsa_result.iterations.offset == 24
    assert _lib.bbmsa_result.score.offset == 32


def test_abi_version():
    assert _lib.load().bbmap_abi_version() == 6


class _idx_params(C.Structure):
    _fields_ = [("i", C.c_int32 * 20), ("pointsPerSite", C.c_int64), ("profile", C.c_int32), ("reserved", C.c_int32)]


class _idx_desc(C.Structure):
    _fields_ = [("params", _idx_params), ("nblocks", C.c_int32), ("nchroms", C.c_int32), ("ptrs", C.c_void_p * 8)]


def _raw():
    """The library without the argtypes of _lib.load(): every argument below is an explicit ctypes value."""
    build.build()
    L = C.CDLL(_lib.SO_PATH)
    L.bbmap_last_error.restype = C.c_char_p
    L.bbkeys_device_workspace_bytes.restype = C.c_int64
    return L


def _msa_cfg(maxRows, maxColumns, scheme):
    return _lib.bbmsa_config(0, maxRows, maxColumns, 0, 0.0, (C.c_int32 * 3)(0, 0, scheme))


def _idx_desc_k(k):
    d = _idx_desc()
    d.params.i[0] = k
    d.nblocks = d.nchroms = 1
    return d


NULL, I32, I64 = None, C.c_int32, C.c_int64
OUT = lambda: C.byref(C.c_void_p())         # noqa: E731

# (entry point, arguments, return code, bbmap_last_error()): every one is refused before the first HIP call, so the same holds
# with and without a device.  At least one per host file of the library.
REJECTED = [
    ("bbmsa_align_batch", lambda: (NULL, I64(1), NULL, NULL, I64(0), NULL, I64(0), NULL, NULL, I32(0)), -2, b"bbmsa_align_batch: null context"),
    ("bbmsa_align_gapped_batch", lambda: (NULL, I64(1), NULL, NULL, NULL, I64(0), NULL, I64(0), NULL, NULL, I32(0)), -2,
     b"bbmsa_align_gapped_batch: null context"),
    ("bbband_align_batch", lambda: (NULL, I64(1), NULL, NULL, I64(0), NULL), -2, b"bbband_align_batch: null context"),
    ("bbidx_find_batch", lambda: (NULL, I64(1), NULL, NULL, NULL, I64(0), NULL, I64(0), NULL, I32(1), NULL), -2, b"bbidx_find_batch: null context"),
    ("bbidx_last_stats", lambda: (NULL, NULL, NULL), -2, b"bbidx_last_stats: null context"),
    ("bbidx_set_kernel", lambda: (NULL, I32(0)), -2, b"bbidx_set_kernel: bad argument"),
    ("bbidx_get_params", lambda: (NULL, NULL), -2, b"bbidx_get_params: null argument"),
    ("bbidx_build_profile", lambda: (I32(0), I32(0), I32(13), I32(-1), I32(1), NULL, NULL, NULL), -2, b"bbidx_build: null argument"),
    ("bbmsa_create", lambda: (NULL, NULL), -2, b"bbmsa_create: null argument"),
    ("bbmsa_create", lambda: (C.byref(_msa_cfg(0, 100, 0)), OUT()), -2, b"bbmsa_create: maxRows must be 1..640 and maxColumns 1..4096"),
    ("bbmsa_create", lambda: (C.byref(_msa_cfg(100, 100, 7)), OUT()), -2, b"bbmsa_create: unknown scoring scheme"),
    ("bbband_create", lambda: (C.byref(_lib.bbband_config(0, 0, 0, 0)), OUT()), -2, b"bbband_create: width must be 1..1023"),
    ("bbidx_create", lambda: (I32(0), C.byref(_idx_desc_k(7)), OUT()), -2, b"bbidx_create: bad index geometry (k must be 8..15)"),
    ("bbpipe_revcomp_device", lambda: (NULL, I64(-1), NULL, NULL, NULL), -2, b"bbpipe_revcomp_device: bad size"),
    ("bbpipe_run_stats_device", lambda: (NULL, I64(-1), I32(0), I32(0), I32(0), NULL, NULL, NULL, NULL, NULL, I32(1), NULL, NULL, NULL), -2,
     b"bbpipe_run_stats_device: bad argument"),
    ("bbmsa_fill_submit", lambda: (NULL, NULL, I32(0), NULL, I32(0), I32(0), I32(0), I32(0), I32(0), NULL, NULL, NULL), -2,
     b"bbmsa_fill_submit: null argument"),
    ("bbmsa_align_batch_device_indirect", lambda: (NULL, NULL, NULL, I64(1), NULL, NULL, NULL, NULL, NULL, I32(0)), -2,
     b"bbmsa_align_batch_device_indirect: null counter"),
    ("bbidx_set_scaffolds", lambda: (NULL, I32(1), NULL, NULL, NULL, I32(0)), -2, b"bbidx_set_scaffolds: null context"),
    ("bbkeys_default_config", lambda: (I32(9), NULL), -2, b"bbkeys_default_config: bad argument"),
    ("bbkeys_device_workspace_bytes", lambda: (NULL, I64(1), I64(1)), -2, b"bbkeys_device_workspace_bytes: bad argument"),
    ("bbmap_create", lambda: (NULL, NULL, NULL), -2, b"bbmap_create: null argument"),
    ("bbmap_get_output", lambda: (NULL, NULL), -2, b"bbmap_get_output: null argument"),
]


@pytest.mark.parametrize("case", range(len(REJECTED)), ids=["%02d-%s" % (i, c[0]) for i, c in enumerate(REJECTED)])
def test_rejected_arguments_keep_their_code_and_message(case):
    name, args, rc, msg = REJECTED[case]
    L = _raw()
    assert getattr(L, name)(*args()) == rc
    assert L.bbmap_last_error() == msg


def test_last_error_is_per_thread():
    L = _raw()
    assert L.bbidx_set_kernel(None, C.c_int32(0)) == -2
    seen = []
    t = threading.Thread(target=lambda: seen.append(L.bbmap_last_error()))
    t.start()
    t.join()
    assert seen == [b""]                                            # a thread that has made no call sees no message
    assert L.bbmap_last_error() == b"bbidx_set_kernel: bad argument"   # and this thread's own is still there
