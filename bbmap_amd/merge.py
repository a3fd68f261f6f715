"""Binding of bbmerge_*: merging overlapping read pairs -- BBMerge's ratio-mode overlap search (BBMerge.mateByOverlap_ratioMode,
current/jgi/BBMerge.java:1615-1639, over the natives mateByOverlapRatioJNI and mateByOverlapRatioJNI_WithQualities) and the overlapped
branch of Read.joinRead (current/stream/Read.java:2804-2840).  A pair is two (bases_off, len) records into one blob; mate 2 is handed
over as it was sequenced and both stages reverse-complement it while they read it.  overlap_batch / join_batch run the host forms over
numpy arrays, overlap_batch_device / join_batch_device the kernels over torch tensors; both give the same output on every input.
merge_pairs packs lists of sequences and runs both device stages."""
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


def merge_pairs(seqs1, seqs2, quals1=None, quals2=None, cfg=None, device="cuda"):
    """Both device stages over lists of sequences: packs the pairs, finds the overlaps, joins every pair the usual rule accepts
    (insert > 0, not ambiguous) and waits.  Returns (REC_DTYPE[n], a list with (bases, quality) per merged pair -- bytes, and a uint8
    array or None without qualities -- and None for a pair that was not merged)."""
    import torch
    cfg = cfg or default_config()
    r1, r2, bases, quality = pack_pairs(seqs1, seqs2, quals1, quals2)
    n = len(r1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(device)    # noqa: E731
    d1, d2, db = up(r1), up(r2), up(bases)
    dq = None if quality is None else up(quality)
    drecs = overlap_batch_device(d1, d2, db, dq, cfg)
    merged, total = slots_for(r1, r2)
    dm = up(merged)
    rv = drecs.view(torch.int32).view(-1, 4) if n else torch.zeros((0, 4), dtype=torch.int32, device=device)
    dins = torch.where((rv[:, 0] > 0) & (rv[:, 2] == 0), rv[:, 0], torch.zeros_like(rv[:, 0])).contiguous()      # usual_inserts
    out_b = torch.zeros(max(1, total), dtype=torch.uint8, device=device)
    out_q = None if quality is None else torch.zeros(max(1, total), dtype=torch.uint8, device=device)
    join_batch_device(d1, d2, db, dq, dins, dm, out_b, out_q, cfg)
    recs = drecs.cpu().numpy().view(REC_DTYPE).copy()
    merged = dm.cpu().numpy().view(READ_DTYPE)
    hb = out_b.cpu().numpy()
    hq = None if out_q is None else out_q.cpu().numpy()
    out = []
    for i in range(n):
        off, ln = int(merged["bases_off"][i]), int(merged["len"][i])
        out.append(None if ln == 0 else (hb[off:off + ln].tobytes(), None if hq is None else hq[off:off + ln].copy()))
    return recs, out
