"""CPU-side checks of the C ABI: the library builds/loads and exports every declared symbol."""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from bbmap_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "bbmap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(bb[a-z]+_[a-z0-9_]+)\s*\(", hdr)))


def test_library_builds_and_exports_every_declared_symbol():
    build.build()
    L = C.CDLL(_lib.SO_PATH)
    syms = declared_symbols()
    assert len(syms) >= 111, "include/bbmap_amd.h declared 111 functions when this test was written; the regex finds %d" % len(syms)
    for s in ("bbmsa_align_batch", "bbband_align_batch", "bbidx_find_batch", "bbmap_map_batch_device", "bbpipe_revcomp_device", "bbtrim_batch"):
        assert s in syms, "not found in the header: " + s
    for s in syms:
        assert hasattr(L, s), "missing export: " + s
    assert _lib.EXPORTS == syms                 # the loader's prototype reader and this regex find the same names


VP, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
# (restype, argtypes) as the binding declared them by hand before the loader read the header, every POINTER(x) written as c_void_p
PINNED = {
    "bbmap_get_sam": (C.c_int, [VP, I64, I32, VP, VP, I64, VP]),                                     # an int64_t count between pointers
    "bbidx_export_block": (C.c_int, [VP, I32, VP, VP, I64, VP, VP]),                                 # an int32_t between pointers
    "bbpipe_sam_records_device": (C.c_int, [VP, I64, I32, VP, I32] + [VP] * 7 + [I32] + [VP] * 5 + [I64, VP, VP, I64]),      # a long mixed tail
    "bbkeys_device_workspace_bytes": (I64, [VP, I64, I64]),                                          # an int64_t return
    "bbpipe_sam_records_workspace_bytes": (I64, [I64, I32]),                                         # no pointer at all
    "bbmap_destroy": (None, [VP]),                                                                   # a void return
    "bbmap_last_error": (C.c_char_p, []),                                                            # const char *, and (void)
    "bbmap_abi_version": (C.c_int, []),                                                              # (void)
    "bbmsa_align_batch": (C.c_int, [VP, I64, VP, VP, I64, VP, I64, VP, VP, I32]),                    # four header lines
    "bbidx_build_profile": (C.c_int, [I32] * 5 + [VP] * 3),                                          # values first; `const T *const *`
    "bbmsa_fill_submit": (C.c_int, [VP, VP, I32, VP, I32, I32, I32, I32, I32, VP, VP, VP]),
    "bbtrim_batch_device": (C.c_int, [VP, VP, I64, VP, VP, VP, VP, VP]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_derived_signature_equals_the_hand_written_one(name):
    assert _lib.PROTOTYPES[name] == PINNED[name]
    fn = getattr(_lib.load(), name)
    assert (fn.restype, list(fn.argtypes)) == PINNED[name]


def test_load_types_every_declared_function():
    L = _lib.load()
    for s in declared_symbols():
        fn = getattr(L, s)
        assert fn.argtypes is not None and (fn.restype, list(fn.argtypes)) == _lib.PROTOTYPES[s], s


@pytest.mark.parametrize("proto, word", [("int bbmap_new_call(bbmap_ctx *ctx, float ratio);", "float ratio"),
                                         ("int bbmap_new_call(bbmap_ctx *ctx, bbmap_config cfg);", "bbmap_config cfg"),
                                         ("double bbmap_new_call(bbmap_ctx *ctx);", "double"),
                                         ("bbmap_ctx *bbmap_new_call(void);", "bbmap_ctx *")])
def test_a_type_outside_the_table_is_refused_by_name(proto, word):
    good = "/* c */\ntypedef struct bbx { int32_t a; } bbx;\nint bbmap_ok(const bbx *x,\n             int64_t n);\n"
    assert _lib.parse_prototypes(good) == {"bbmap_ok": (C.c_int, [VP, I64])}
    with pytest.raises(_lib.BBMapAmdError) as e:
        _lib.parse_prototypes(good + proto)
    assert "bbmap_new_call" in str(e.value) and word in str(e.value)


def test_struct_layouts_match_header():
    assert C.sizeof(_lib.bbmsa_job) == 40
    assert C.sizeof(_lib.bbmsa_result) == 80
    assert _lib.bbmsa_result.iterations.offset == 24
    assert _lib.bbmsa_result.score.offset == 32


def _mirrors():
    """(struct name in the header, its Python mirror: a ctypes.Structure or a numpy dtype), every record the binding declares"""
    from bbmap_amd import banded, coverage, index, keys, mapper, msa, readstats, refsplit, rescue, runstats, trim
    return [("bbmsa_job", _lib.bbmsa_job), ("bbmsa_result", _lib.bbmsa_result), ("bbmsa_config", _lib.bbmsa_config),
            ("bbband_job", _lib.bbband_job), ("bbband_result", _lib.bbband_result), ("bbband_config", _lib.bbband_config),
            ("bbmsa_job", msa.JOB_DTYPE), ("bbmsa_result", msa.RESULT_DTYPE), ("bbmsa_gaps", msa.GAPS_DTYPE), ("bbmsa_ticket", msa.bbmsa_ticket),
            ("bbband_job", banded.JOB_DTYPE), ("bbband_result", banded.RESULT_DTYPE), ("bbband_pair", banded.PAIR_DTYPE),
            ("bbidx_params", index.bbidx_params), ("bbidx_index_desc", index.bbidx_index_desc), ("bbidx_read", index.READ_DTYPE),
            ("bbidx_site", index.SITE_DTYPE), ("bbkeys_config", keys.bbkeys_config), ("bbtrim_config", trim.bbtrim_config),
            ("bbtrim_rec", trim.TRIM_DTYPE), ("bbresc_job", rescue.JOB_DTYPE), ("bbresc_result", rescue.RESULT_DTYPE),
            ("bbmap_msite", mapper.MSITE_DTYPE), ("bbmap_jobinfo", mapper.JOBINFO_DTYPE), ("bbmap_final", mapper.FINAL_DTYPE),
            ("bbmap_scafrec", mapper.SCAFREC_DTYPE), ("bbmap_samrec", mapper.SAMREC_DTYPE), ("bbmap_samtags", mapper.SAMTAGS_DTYPE),
            ("bbmap_config", mapper.bbmap_config), ("bbmap_sam_config", mapper.bbmap_sam_config), ("bbmap_output", mapper.bbmap_output),
            ("bbmap_stats", mapper.bbmap_stats), ("bbmap_overflow_output", mapper.bbmap_overflow_output),
            ("bbmap_runstats", runstats.RUNSTATS_DTYPE), ("bbmap_truth", runstats.TRUTH_DTYPE),
            ("bbmap_covstrand", coverage.COVSTRAND_DTYPE), ("bbmap_covrec", coverage.COVREC_DTYPE), ("bbmap_covtotals", coverage.COVTOTALS_DTYPE),
            ("bbmap_cov_view", coverage.bbmap_cov_view), ("bbmap_readhist_view", readstats.bbmap_readhist_view),
            ("bbmap_split_config", refsplit.bbmap_split_config), ("bbmap_splitrec", refsplit.SPLITREC_DTYPE)]


def _layout(mirror):
    """(size, {field: offset}) of a ctypes.Structure or a numpy dtype"""
    if isinstance(mirror, np.dtype):
        return mirror.itemsize, {n: mirror.fields[n][1] for n in mirror.names}
    return C.sizeof(mirror), {n: getattr(mirror, n).offset for n, *_ in mirror._fields_}


def test_every_mirrored_record_has_the_compiler_s_layout(tmp_path):
    """sizeof and every mirrored field's offsetof, as the host C compiler lays the header's structs out, against the Python mirrors:
    a mirror field the header lacks does not compile, a missing or reordered one shifts an offset or the size."""
    mirrors = _mirrors()
    assert len(mirrors) >= 42
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "bbmap_amd.h"', "int main(void) {"]
    for i, (name, mirror) in enumerate(mirrors):
        src.append('    printf("%d sizeof %%zu\\n", sizeof(%s));' % (i, name))
        for f in _layout(mirror)[1]:
            # (a trailing underscore keeps a mirror's field clear of a Python keyword: bbmap_readhist_view.del_)
            src.append('    printf("%d %s %%zu\\n", offsetof(%s, %s));' % (i, f, name, f.rstrip("_")))
    src += ["    return 0;", "}", ""]
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe], check=True)
    got = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        i, f, v = line.split()
        got.setdefault(int(i), {})[f] = int(v)
    for i, (name, mirror) in enumerate(mirrors):
        size, offsets = _layout(mirror)
        assert dict(offsets, sizeof=size) == got[i], "%s (%s)" % (name, mirror.__name__ if isinstance(mirror, type) else "dtype")


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


NULL = None
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
