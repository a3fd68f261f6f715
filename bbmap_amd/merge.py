"""Binding of bbmerge_*: merging overlapping read pairs -- BBMerge's ratio-mode overlap search (BBMerge.mateByOverlap_ratioMode,
current/jgi/BBMerge.java:1615-1639, over the natives mateByOverlapRatioJNI and mateByOverlapRatioJNI_WithQualities) and the overlapped
branch of Read.joinRead (current/stream/Read.java:2804-2840).  A pair is two (bases_off, len) records into one blob; mate 2 is handed
over as it was sequenced and both stages reverse-complement it while they read it.  overlap_batch / join_batch run the host forms over
numpy arrays, overlap_batch_device / join_batch_device the kernels over torch tensors; both give the same output on every input.
merge_pairs packs lists of sequences and runs both device stages.
verdict_batch / verdict_batch_device give BBMerge's verdict per pair (bbmerge_verdict_batch: the entropy-derived minOverlap, ratio and
normal mode under BBMerge.mateByOverlap's composition, efilter / pfilter, the return code, counters); verdict_from_flags builds its
configuration from BBMerge's flags and the strict / vstrict / ustrict / xstrict / fast presets, and merge_pairs(verdict=...) joins what
that verdict accepts."""
import ctypes as C

import numpy as np

from . import _lib
from .index import READ_DTYPE
from .trim import _parse_boolean

MAX_READ_LEN = 512                                      # BBMERGE_MAX_READ_LEN
INFO_QUALITY, INFO_FLAT, INFO_SKIPPED = 1, 2, 256       # BBMERGE_INFO_*
REC_DTYPE = np.dtype([("insert", "<i4"), ("bad", "<i4"), ("ambig", "<i4"), ("info", "<i4")])


class bbmerge_config(C.Structure):
    _fields_ = [("minOverlap0", C.c_int32), ("minOverlap", C.c_int32), ("minInsert0", C.c_int32), ("minInsert", C.c_int32),
                ("maxRatio", C.c_float), ("ratioMargin", C.c_float), ("ratioOffset", C.c_float), ("gIncr", C.c_float), ("bIncr", C.c_float),
                ("useQuality", C.c_int32), ("withoutQuality", C.c_int32), ("maxMergeQuality", C.c_int32)]


def default_config(**kw):
    """BBMerge's defaults (minOverlap0 5, minOverlap 8, minInsert0 26, minInsert 35, maxRatio .09, ratioMargin 5.5, ratioOffset .55,
    both increments .95, the flat form only, maxMergeQuality 41); kw sets fields."""
    L = _lib.load()
    cfg = bbmerge_config()
    _lib.check(L.bbmerge_default_config(C.byref(cfg)), "bbmerge_default_config")
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError("bbmerge_config has no field %r" % (k,))
        setattr(cfg, k, v)
    return cfg


def from_flags(minoverlap=None, minoverlap0=None, ratiominoverlapreduction=None, mininsert=None, mininsert0=None, maxratio=None,
               ratiomargin=None, ratiooffset=None, maxq=None, usequality=None, overlapusingquality=None, overlapwithoutquality=None):
    """The bbmerge_config BBMerge's command line gives (BBMerge.java:366-391, :472-480).  A flag that is None was not given.
    minoverlap= / minoverlap0= set MIN_OVERLAPPING_BASES (11) / MIN_OVERLAPPING_BASES_0 (8), ratiominoverlapreduction= (3) comes off
    both for the natives (:1617-1618); mininsert= (35) is raised to MIN_OVERLAPPING_BASES, and a mininsert0= below 1 (the default, -1)
    becomes min(35, max((int)(minInsert * 0.75), 5, MIN_OVERLAPPING_BASES_0)); at the end minInsert0 is at most minInsert (:605-611,
    without the `loose` preset).  usequality= is this binding's name for overlapusingquality=; giving both is an error."""
    if usequality is not None and overlapusingquality is not None:
        raise ValueError("usequality and overlapusingquality are one flag")
    uq = usequality if usequality is not None else overlapusingquality
    cfg = default_config()
    min_overlapping_bases = 11 if minoverlap is None else int(minoverlap)
    min_overlapping_bases_0 = 8 if minoverlap0 is None else int(minoverlap0)
    reduction = 3 if ratiominoverlapreduction is None else int(ratiominoverlapreduction)
    min_insert = 35 if mininsert is None else int(mininsert)
    min_insert_0 = -1 if mininsert0 is None else int(mininsert0)
    min_insert = max(min_insert, min_overlapping_bases)
    if min_insert_0 < 1:
        min_insert_0 = min(35, max(int(min_insert * 0.75), 5, min_overlapping_bases_0))
    min_insert_0 = min(min_insert, min_insert_0)
    cfg.minOverlap0, cfg.minOverlap = min_overlapping_bases_0 - reduction, min_overlapping_bases - reduction
    cfg.minInsert0, cfg.minInsert = min_insert_0, min_insert
    if maxratio is not None:
        cfg.maxRatio = float(maxratio)
    if ratiomargin is not None:
        cfg.ratioMargin = float(ratiomargin)
    if ratiooffset is not None:
        cfg.ratioOffset = float(ratiooffset)
    if maxq is not None:
        cfg.maxMergeQuality = int(maxq)
    if uq is not None:
        cfg.useQuality = int(_parse_boolean(uq))
    if overlapwithoutquality is not None:
        cfg.withoutQuality = int(_parse_boolean(overlapwithoutquality))
    return cfg


INFO_RATIO, INFO_NORMAL, INFO_EFILTER, INFO_PFILTER = 4, 8, 16, 32                      # BBMERGE_INFO_*
RET_NO_SOLUTION, RET_AMBIG, RET_SHORT, RET_LONG = -1, -2, -4, -5                       # BBMERGE_RET_*
HIST_LEN = 2000                                                                         # BBMERGE_HIST_LEN
VERDICT_DTYPE = np.dtype([("code", "<i4"), ("minOverlap", "<i4"), ("insertRM", "<i4"), ("badRM", "<i4"), ("ambigRM", "<i4"),
                          ("insertNM", "<i4"), ("badNM", "<i4"), ("ambigNM", "<i4"), ("bad", "<i4"), ("expected", "<f4"),
                          ("probability", "<f4"), ("info", "<i4")])
STATS_DTYPE = np.dtype([(k, "<i8") for k in ("pairs", "merged", "ambiguous", "tooShort", "tooLong", "noSolution", "skipped", "insertSum",
                                             "insertMin", "insertMax")] + [("hist", "<i8", (HIST_LEN,))])


class bbmerge_verdict_config(C.Structure):
    _fields_ = [("ratio", bbmerge_config), ("useEntropy", C.c_int32), ("entropyK", C.c_int32), ("minEntropyScore", C.c_int32),
                ("minOverlapBases", C.c_int32), ("minOverlapBases0", C.c_int32), ("ratioReduction", C.c_int32),
                ("useRatioMode", C.c_int32), ("useNormalMode", C.c_int32), ("requireRatioMatch", C.c_int32), ("maxMismatchesR", C.c_int32),
                ("margin", C.c_int32), ("maxMismatches", C.c_int32), ("maxMismatches0", C.c_int32), ("minQuality", C.c_int32),
                ("qualIters", C.c_int32), ("useQuality", C.c_int32), ("useEfilter", C.c_int32), ("efilterRatio", C.c_float),
                ("efilterOffset", C.c_float), ("pfilterRatio", C.c_float), ("maxLength", C.c_int32), ("reserved", C.c_int32)]


def default_verdict_config(**kw):
    """bbmerge_default_verdict_config: BBMerge's defaults for the verdict (include/bbmap_amd.h lists them).  kw sets fields; a name
    that is a field of the embedded bbmerge_config (maxRatio, minInsert, ...) sets it there, `useQuality` names the verdict's own
    field (BBMerge.useQuality) and `overlapUsingQuality` the embedded one."""
    L = _lib.load()
    cfg = bbmerge_verdict_config()
    _lib.check(L.bbmerge_default_verdict_config(C.byref(cfg)), "bbmerge_default_verdict_config")
    own = {f[0] for f in bbmerge_verdict_config._fields_} - {"ratio"}
    for k, v in kw.items():
        if k in own:
            setattr(cfg, k, v)
        elif k == "overlapUsingQuality":
            cfg.ratio.useQuality = v
        elif hasattr(cfg.ratio, k):
            setattr(cfg.ratio, k, v)
        else:
            raise AttributeError("bbmerge_verdict_config has no field %r" % (k,))
    return cfg


def new_stats():
    """A bbmerge_stats record as a caller starts it: zeros, insertMin 999999999."""
    s = np.zeros(1, STATS_DTYPE)
    s["insertMin"] = 999999999
    return s


_STRICT = [("maxbad", "4"), ("margin", "3"), ("minqo", "8"), ("qualiters", "2")]
_BOTH_MODES = [("ratiomode", "t"), ("normalmode", "t"), ("requireratiomatch", "t")]
# the flags a preset puts in front of the command line (BBMerge.java:122-193, :258-267)
PRESETS = {
    "strict": _STRICT + [("ratiomode", "t"), ("normalmode", "f"), ("minentropy", "42"), ("minoverlap0", "7"), ("minoverlap", "11"),
                         ("maxratio", "0.075"), ("ratiomargin", "7.5"), ("ratiooffset", "0.55"), ("ratiominoverlapreduction", "4"),
                         ("efilter", "4"), ("pfilter", "0.0008"), ("minsecondratio", "0.12")],
    "vstrict": _STRICT + [("ratiomode", "t"), ("normalmode", "f"), ("minentropy", "52"), ("minoverlap", "12"), ("minoverlap0", "4"),
                          ("maxratio", "0.05"), ("ratiomargin", "12"), ("ratiooffset", "0.5"), ("ratiominoverlapreduction", "4"),
                          ("efilter", "2"), ("pfilter", "0.008"), ("minsecondratio", "0.16")],
    "ustrict": _STRICT + _BOTH_MODES + [("minentropy", "56"), ("minoverlap", "14"), ("minoverlap0", "3"), ("maxratio", "0.045"),
                                        ("ratiomargin", "12"), ("ratiooffset", "0.5"), ("ratiominoverlapreduction", "4"), ("efilter", "2"),
                                        ("pfilter", "0.03"), ("minsecondratio", "0.20")],
    "xstrict": _STRICT + _BOTH_MODES + [("minentropy", "56"), ("minoverlap", "14"), ("minoverlap0", "3"), ("maxratio", "0.055"),
                                        ("ratiomargin", "12"), ("ratiooffset", "0.65"), ("ratiominoverlapreduction", "4"), ("efilter", "2"),
                                        ("pfilter", "0.25"), ("minsecondratio", "0.24")],
    "fast": [("maxratio", "0.08"), ("ratiomargin", "2.5"), ("ratiominoverlapreduction", "3"), ("pfilter", "0.0002"), ("efilter", "8"),
             ("minentropy", "39"), ("mininsert0", "50"), ("minsecondratio", "0.08")],
}
_LOOSE = ("loose", "vloose", "veryloose", "uloose", "ultraloose", "xloose", "hloose", "hyperloose", "maxloose")      # BBMerge.java:91-106
_PRESET_NAMES = {"verystrict": "vstrict", "ultrastrict": "ustrict"}                                                    # :75-79
_ALIASES = {"useratio": "ratiomode", "ratio": "ratiomode", "usenormalmode": "normalmode", "rrm": "requireratiomatch", "entropy": "minentropy",
            "minoverlappingbases": "minoverlap", "minoverlapbases": "minoverlap", "minoverlappingbases0": "minoverlap0",
            "minoverlapbases0": "minoverlap0", "minq": "minqo", "maxbadbases": "maxbad", "mismatches": "maxbad", "maxbadbases0": "maxbad0",
            "mismatches0": "maxbad0", "ouq": "overlapusingquality", "owq": "overlapwithoutquality", "maxlen": "maxlength"}


def _byte(x):
    """Java's (byte) cast of an int"""
    return (int(x) + 128) % 256 - 128


def verdict_from_flags(preset=None, **flags):
    """The bbmerge_verdict_config BBMerge's command line gives.  preset: None, 'strict', 'vstrict', 'ustrict', 'xstrict' or 'fast'; its
    flags come first and the given ones override them, as in the argv BBMerge rewrites (BBMerge.java:122-193, :258-272).  flags:
    BBMerge's names and aliases (:360-400, :490-517) with their values as on the command line (strings, or Python values):
    ratiomode, normalmode, requireratiomatch / rrm, maxratio, ratiomargin, ratiooffset, ratiominoverlapreduction, minentropy / entropy
    (a value whose first character is a digit sets the score, anything else is read as a boolean that switches entropy, so "-5" is
    refused as Java's isDigit rule refuses it), minoverlap, minoverlap0, minqo / minq, maxq, qualiters (at least 1),
    maxbad / mismatches, maxbad0 / mismatches0, margin, efilter (a number, or a boolean: false gives ratio -1 and switches it off),
    pfilter (a number, or false for 0), efilteroffset, usequality, ignorequality, overlapusingquality / ouq, overlapwithoutquality /
    owq, mininsert, mininsert0, maxlength.  After parsing (:605-616, :653-664): minInsert and minInsert0 as from_flags; with neither
    mode on the normal mode is used; mismatches0 follows mismatches unless it was set and is raised to it; margin is capped at
    mismatches.  minsecondratio is accepted and ignored: only the Java ratio forms read it, and this project follows the natives
    (usejni=t).  The loose family (loose, vloose / veryloose, uloose / ultraloose, xloose / hloose / hyperloose / maxloose) is refused as a
    preset and as a flag set to true: its two `loose` branches (:1664-1672, :1699-1704) are not built.  Set to false such a flag is
    accepted and changes nothing."""
    preset = _PRESET_NAMES.get(preset, preset)
    if preset in _LOOSE:
        raise ValueError("%s: the loose presets need the `loose` branches of mateByOverlap_normalMode and calcMinOverlapFromEntropy, "
                         "which are not built" % preset)
    if preset is not None and preset not in PRESETS:
        raise ValueError("unknown preset %r" % (preset,))
    argv = list(PRESETS.get(preset, [])) + [(k, v) for k, v in flags.items() if v is not None]
    st = dict(ratiomode=True, normalmode=False, rrm=False, maxratio=None, ratiomargin=None, ratiooffset=None, reduction=3, minentropy=39,
              useentropy=True, minoverlap=11, minoverlap0=8, minq=10, maxq=None, qualiters=3, maxbad=3, maxbad0=3, mm0set=False, margin=2,
              efilter=6.0, useefilter=True, pfilter=0.00004, efilteroffset=0.05, usequality=True, ouq=None, owq=None, mininsert=35,
              mininsert0=-1, maxlength=-1)
    for name, b in argv:
        a = _ALIASES.get(name.lower(), name.lower())
        if a in _LOOSE:
            if _parse_boolean(b):
                raise ValueError("%s: the loose presets need the `loose` branches of mateByOverlap_normalMode and calcMinOverlapFromEntropy, "
                                 "which are not built" % a)
            continue                    # (loose=f: the preset stays off)
        s = b if isinstance(b, str) else ("t" if b is True else "f" if b is False else repr(b))
        if a == "ratiomode":
            st["ratiomode"] = _parse_boolean(s)
        elif a == "normalmode":
            st["normalmode"] = _parse_boolean(s)
        elif a == "requireratiomatch":
            st["rrm"] = _parse_boolean(s)
        elif a in ("maxratio", "ratiomargin", "ratiooffset", "efilteroffset"):
            st[a] = float(s)
        elif a == "ratiominoverlapreduction":
            st["reduction"] = int(s)
        elif a == "minentropy":
            if s[:1].isdigit():
                st["minentropy"] = int(s)
            else:
                st["useentropy"] = _parse_boolean(s)
        elif a in ("minoverlap", "minoverlap0", "maxbad", "margin", "mininsert", "mininsert0", "maxlength"):
            st[a] = int(s)
        elif a == "minqo":
            st["minq"] = _byte(int(s))
        elif a == "maxq":
            st["maxq"] = _byte(int(s))
        elif a == "qualiters":
            st["qualiters"] = max(1, int(s))
        elif a == "maxbad0":
            st["maxbad0"], st["mm0set"] = int(s), True
        elif a == "efilter":
            if s[:1].isalpha():
                if not _parse_boolean(s):
                    st["efilter"] = -1.0
            else:
                st["efilter"] = float(s)
            st["useefilter"] = st["efilter"] >= 0
        elif a == "pfilter":
            if s[:1].isalpha():
                if not _parse_boolean(s):
                    st["pfilter"] = 0.0
            else:
                st["pfilter"] = float(s)
        elif a == "usequality":
            st["usequality"] = _parse_boolean(s)
        elif a == "ignorequality":
            st["usequality"] = not _parse_boolean(s)
        elif a == "overlapusingquality":
            st["ouq"] = _parse_boolean(s)
        elif a == "overlapwithoutquality":
            st["owq"] = _parse_boolean(s)
        elif a == "minsecondratio":
            float(s)                    # (read by the Java ratio forms only; the natives have no such argument)
        elif a in PRESETS:
            raise ValueError("%s is a preset: pass it as preset=" % a)
        else:
            raise ValueError("verdict_from_flags: unknown flag %r" % (name,))
    min_insert = max(st["mininsert"], st["minoverlap"])
    min_insert_0 = st["mininsert0"]
    if min_insert_0 < 1:
        min_insert_0 = min(35, max(int(min_insert * 0.75), 5, st["minoverlap0"]))
    min_insert_0 = min(min_insert, min_insert_0)
    if not st["normalmode"] and not st["ratiomode"]:
        st["normalmode"] = True
    if not st["mm0set"] or st["maxbad0"] < st["maxbad"]:
        st["maxbad0"] = st["maxbad"]
    st["margin"] = min(st["margin"], st["maxbad"])
    cfg = default_verdict_config()
    r = cfg.ratio
    r.minOverlap0, r.minOverlap = st["minoverlap0"] - st["reduction"], st["minoverlap"] - st["reduction"]     # (not read by the verdict)
    r.minInsert0, r.minInsert = min_insert_0, min_insert
    for field, key in (("maxRatio", "maxratio"), ("ratioMargin", "ratiomargin"), ("ratioOffset", "ratiooffset"), ("maxMergeQuality", "maxq")):
        if st[key] is not None:
            setattr(r, field, st[key])
    if st["ouq"] is not None:
        r.useQuality = int(st["ouq"])
    if st["owq"] is not None:
        r.withoutQuality = int(st["owq"])
    cfg.useEntropy, cfg.minEntropyScore = int(st["useentropy"]), st["minentropy"]
    cfg.minOverlapBases, cfg.minOverlapBases0, cfg.ratioReduction = st["minoverlap"], st["minoverlap0"], st["reduction"]
    cfg.useRatioMode, cfg.useNormalMode, cfg.requireRatioMatch = int(st["ratiomode"]), int(st["normalmode"]), int(st["rrm"])
    cfg.margin, cfg.maxMismatches, cfg.maxMismatches0 = st["margin"], st["maxbad"], st["maxbad0"]
    cfg.minQuality, cfg.qualIters = st["minq"], st["qualiters"]
    cfg.useQuality, cfg.useEfilter = int(st["usequality"]), int(st["useefilter"])
    cfg.efilterRatio, cfg.efilterOffset, cfg.pfilterRatio = st["efilter"], st["efilteroffset"], st["pfilter"]
    cfg.maxLength = 0 if st["maxlength"] < 0 else st["maxlength"]
    return cfg


def verdict_batch(reads1, reads2, bases, quality=None, cfg=None, stats=None):
    """bbmerge_verdict_batch, the host form: BBMerge's verdict per pair.  Arguments as overlap_batch; cfg a bbmerge_verdict_config
    (the defaults when None); stats None or a STATS_DTYPE[1] array (new_stats()) that the call adds to.  Returns VERDICT_DTYPE[n]."""
    L = _lib.load()
    cfg = cfg or default_verdict_config()
    r1, r2 = np.ascontiguousarray(reads1, READ_DTYPE), np.ascontiguousarray(reads2, READ_DTYPE)
    assert len(r1) == len(r2)
    assert stats is None or (stats.dtype == STATS_DTYPE and stats.size == 1 and stats.flags.c_contiguous)
    b, q = _host_blobs(bases, quality)
    recs = np.zeros(len(r1), VERDICT_DTYPE)
    _lib.check(L.bbmerge_verdict_batch(C.byref(cfg), len(r1), r1.ctypes.data, r2.ctypes.data, b.ctypes.data, None if q is None else q.ctypes.data,
                                       recs.ctypes.data, None if stats is None else stats.ctypes.data), "bbmerge_verdict_batch")
    return recs


def _host_blobs(bases, quality):
    b = np.ascontiguousarray(bases, np.uint8).reshape(-1)
    q = None if quality is None else np.ascontiguousarray(quality, np.uint8).reshape(-1)
    assert q is None or q.size >= b.size
    if b.size == 0:
        b = np.zeros(1, np.uint8)
    return b, q


def overlap_batch(reads1, reads2, bases, quality=None, cfg=None):
    """bbmerge_overlap_batch, the host form.  reads1 / reads2: READ_DTYPE (bases_off, len) of the two mates, bases / quality: uint8 blobs
    (quality numeric phred at the same offsets, or None).  Returns REC_DTYPE[n]."""
    L = _lib.load()
    cfg = cfg or default_config()
    r1, r2 = np.ascontiguousarray(reads1, READ_DTYPE), np.ascontiguousarray(reads2, READ_DTYPE)
    assert len(r1) == len(r2)
    b, q = _host_blobs(bases, quality)
    recs = np.zeros(len(r1), REC_DTYPE)
    _lib.check(L.bbmerge_overlap_batch(C.byref(cfg), len(r1), r1.ctypes.data, r2.ctypes.data, b.ctypes.data, None if q is None else q.ctypes.data,
                                       recs.ctypes.data), "bbmerge_overlap_batch")
    return recs


def usual_inserts(recs):
    """The insert to join per pair by the usual rule: rec.insert where it is positive and the pair is not ambiguous, else 0."""
    recs = np.asarray(recs)
    return np.where((recs["insert"] > 0) & (recs["ambig"] == 0), recs["insert"], 0).astype(np.int32)


def slots_for(reads1, reads2):
    """(READ_DTYPE records whose bases_off name consecutive slots of alen + blen bytes, the bytes all slots take)"""
    need = np.maximum(reads1["len"], 0).astype(np.int64) + np.maximum(reads2["len"], 0)
    merged = np.zeros(len(need), READ_DTYPE)
    merged["bases_off"] = np.cumsum(need) - need
    return merged, int(need.sum())


def join_batch(reads1, reads2, bases, quality, insert, merged=None, out_bases=None, out_quality=None, cfg=None):
    """bbmerge_join_batch, the host form.  insert: int32 per pair (0: do not join).  merged / out_bases / out_quality: the slots and the
    buffers to write into (slots_for's and zeros when None).  Returns (merged with len set, out_bases, out_quality or None)."""
    L = _lib.load()
    cfg = cfg or default_config()
    r1, r2 = np.ascontiguousarray(reads1, READ_DTYPE), np.ascontiguousarray(reads2, READ_DTYPE)
    ins = np.ascontiguousarray(insert, np.int32)
    assert len(r1) == len(r2) == len(ins)
    b, q = _host_blobs(bases, quality)
    if merged is None:
        merged, total = slots_for(r1, r2)
        out_bases = np.zeros(max(1, total), np.uint8)
        out_quality = None if q is None else np.zeros(max(1, total), np.uint8)
    assert merged.dtype == READ_DTYPE and merged.flags.c_contiguous and out_bases.dtype == np.uint8 and out_bases.flags.c_contiguous
    assert q is None or (out_quality.dtype == np.uint8 and out_quality.flags.c_contiguous)
    _lib.check(L.bbmerge_join_batch(C.byref(cfg), len(r1), r1.ctypes.data, r2.ctypes.data, b.ctypes.data, None if q is None else q.ctypes.data,
                                    ins.ctypes.data, merged.ctypes.data, out_bases.ctypes.data,
                                    None if q is None else out_quality.ctypes.data), "bbmerge_join_batch")
    return merged, out_bases, out_quality if q is not None else None


def _device_args(torch, reads1, reads2, bases, quality):
    dev = bases.device
    for r in (reads1, reads2):
        assert r.dtype == torch.uint8 and r.is_contiguous() and r.numel() % READ_DTYPE.itemsize == 0 and r.device == dev
    assert reads1.numel() == reads2.numel()
    assert bases.dtype == torch.uint8 and bases.is_contiguous()
    assert quality is None or (quality.dtype == torch.uint8 and quality.is_contiguous() and quality.device == dev and quality.numel() >= bases.numel())
    if bases.numel() == 0:          # (an empty tensor has no address)
        bases = torch.zeros(1, dtype=torch.uint8, device=dev)
    return dev, reads1.numel() // READ_DTYPE.itemsize, bases


def overlap_batch_device(reads1, reads2, bases, quality=None, cfg=None):
    """bbmerge_overlap_batch_device over device tensors: reads1 / reads2 = uint8 views of READ_DTYPE, bases / quality uint8 (quality
    None: pairs without qualities).  Returns a new uint8 tensor viewing REC_DTYPE.  Enqueues on the current stream and does not wait.
    As with the mapper, torch must have been imported before the library is first loaded."""
    import torch
    L = _lib.load()
    cfg = cfg or default_config()
    dev, n, bases = _device_args(torch, reads1, reads2, bases, quality)
    recs = torch.zeros(max(1, n) * REC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = L.bbmerge_overlap_batch_device(C.byref(cfg), C.c_void_p(stream), n, reads1.data_ptr() if n else None, reads2.data_ptr() if n else None,
                                            bases.data_ptr(), None if quality is None else quality.data_ptr(), recs.data_ptr())
    _lib.check(rc, "bbmerge_overlap_batch_device")
    return recs[: n * REC_DTYPE.itemsize]


def new_stats_device(device):
    """new_stats() on the device: a uint8 tensor viewing STATS_DTYPE[1]"""
    import torch
    return torch.from_numpy(new_stats().view(np.uint8).copy()).to(device)


def verdict_batch_device(reads1, reads2, bases, quality=None, cfg=None, stats=None):
    """bbmerge_verdict_batch_device over device tensors, as overlap_batch_device.  stats: None, or a uint8 tensor viewing STATS_DTYPE[1]
    (new_stats_device()) that the kernels add to.  Returns a new uint8 tensor viewing VERDICT_DTYPE.  Enqueues on the current stream
    and does not wait."""
    import torch
    L = _lib.load()
    cfg = cfg or default_verdict_config()
    dev, n, bases = _device_args(torch, reads1, reads2, bases, quality)
    assert stats is None or (stats.dtype == torch.uint8 and stats.is_contiguous() and stats.numel() == STATS_DTYPE.itemsize and stats.device == dev)
    recs = torch.zeros(max(1, n) * VERDICT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = L.bbmerge_verdict_batch_device(C.byref(cfg), C.c_void_p(stream), n, reads1.data_ptr() if n else None, reads2.data_ptr() if n else None,
                                            bases.data_ptr(), None if quality is None else quality.data_ptr(), recs.data_ptr(),
                                            None if stats is None else stats.data_ptr())
    _lib.check(rc, "bbmerge_verdict_batch_device")
    return recs[: n * VERDICT_DTYPE.itemsize]


def join_batch_device(reads1, reads2, bases, quality, insert, merged, out_bases, out_quality=None, cfg=None):
    """bbmerge_join_batch_device over device tensors: insert int32[n], merged a uint8 view of READ_DTYPE whose bases_off name the slots
    (its len fields are written), out_bases / out_quality uint8 (out_quality may be None when quality is).  Writes in place, enqueues on
    the current stream and does not wait."""
    import torch
    L = _lib.load()
    cfg = cfg or default_config()
    dev, n, bases = _device_args(torch, reads1, reads2, bases, quality)
    assert insert.dtype == torch.int32 and insert.is_contiguous() and insert.numel() == n and insert.device == dev
    assert merged.dtype == torch.uint8 and merged.is_contiguous() and merged.numel() == n * READ_DTYPE.itemsize and merged.device == dev
    assert out_bases.dtype == torch.uint8 and out_bases.is_contiguous() and out_bases.device == dev
    assert quality is None or (out_quality is not None and out_quality.dtype == torch.uint8 and out_quality.is_contiguous() and out_quality.device == dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = L.bbmerge_join_batch_device(C.byref(cfg), C.c_void_p(stream), n, reads1.data_ptr() if n else None, reads2.data_ptr() if n else None,
                                         bases.data_ptr(), None if quality is None else quality.data_ptr(), insert.data_ptr() if n else None,
                                         merged.data_ptr() if n else None, out_bases.data_ptr() if out_bases.numel() else None,
                                         None if quality is None else out_quality.data_ptr())
    _lib.check(rc, "bbmerge_join_batch_device")


def pack_pairs(seqs1, seqs2, quals1=None, quals2=None):
    """(reads1, reads2, bases, quality or None) for lists of byte strings: one blob, mate 1s first.  Qualities are numeric phred values
    (bytes or uint8 arrays), given for both mates or for neither."""
    assert len(seqs1) == len(seqs2) and (quals1 is None) == (quals2 is None)
    seqs = [bytes(s) for s in seqs1] + [bytes(s) for s in seqs2]
    lens = np.array([len(s) for s in seqs], np.int64)
    reads = np.zeros(len(seqs), READ_DTYPE)
    reads["bases_off"], reads["len"] = np.cumsum(lens) - lens, lens
    bases = np.frombuffer(b"".join(seqs), np.uint8).copy()
    quality = None
    if quals1 is not None:
        quals = [np.asarray(bytearray(q) if isinstance(q, (bytes, bytearray)) else q, np.uint8) for q in list(quals1) + list(quals2)]
        assert [len(q) for q in quals] == lens.tolist()
        quality = np.concatenate(quals) if quals else np.zeros(0, np.uint8)
    n = len(seqs1)
    return reads[:n].copy(), reads[n:].copy(), bases, quality


def merge_pairs(seqs1, seqs2, quals1=None, quals2=None, cfg=None, device="cuda", verdict=None):
    """Both device stages over lists of sequences: packs the pairs, finds the overlaps, joins every pair the usual rule accepts
    (insert > 0, not ambiguous) and waits.  Returns (REC_DTYPE[n], a list with (bases, quality) per merged pair -- bytes, and a uint8
    array or None without qualities -- and None for a pair that was not merged).
    verdict: a bbmerge_verdict_config.  Then BBMerge's verdict decides (verdict_batch_device): the pairs joined are those with a
    positive `code`, at that insert, with verdict.ratio.maxMergeQuality, and the records returned are VERDICT_DTYPE[n]; cfg is not
    used."""
    import torch
    cfg = cfg or default_config()
    r1, r2, bases, quality = pack_pairs(seqs1, seqs2, quals1, quals2)
    n = len(r1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(device)    # noqa: E731
    d1, d2, db = up(r1), up(r2), up(bases)
    dq = None if quality is None else up(quality)
    merged, total = slots_for(r1, r2)
    dm = up(merged)
    if verdict is not None:
        cfg, rec_dtype = verdict.ratio, VERDICT_DTYPE
        drecs = verdict_batch_device(d1, d2, db, dq, verdict)
        code = drecs.view(torch.int32).view(-1, VERDICT_DTYPE.itemsize // 4)[:, 0] if n else torch.zeros(0, dtype=torch.int32, device=device)
        dins = torch.where(code > 0, code, torch.zeros_like(code)).contiguous()
    else:
        rec_dtype = REC_DTYPE
        drecs = overlap_batch_device(d1, d2, db, dq, cfg)
        rv = drecs.view(torch.int32).view(-1, 4) if n else torch.zeros((0, 4), dtype=torch.int32, device=device)
        dins = torch.where((rv[:, 0] > 0) & (rv[:, 2] == 0), rv[:, 0], torch.zeros_like(rv[:, 0])).contiguous()      # usual_inserts
    out_b = torch.zeros(max(1, total), dtype=torch.uint8, device=device)
    out_q = None if quality is None else torch.zeros(max(1, total), dtype=torch.uint8, device=device)
    join_batch_device(d1, d2, db, dq, dins, dm, out_b, out_q, cfg)
    recs = drecs.cpu().numpy().view(rec_dtype).copy()
    merged = dm.cpu().numpy().view(READ_DTYPE)
    hb = out_b.cpu().numpy()
    hq = None if out_q is None else out_q.cpu().numpy()
    out = []
    for i in range(n):
        off, ln = int(merged["bases_off"][i]), int(merged["len"][i])
        out.append(None if ln == 0 else (hb[off:off + ln].tobytes(), None if hq is None else hq[off:off + ln].copy()))
    return recs, out
