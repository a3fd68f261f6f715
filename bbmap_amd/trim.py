"""Binding of bbtrim_*: quality trimming before mapping -- align2.TrimRead.trim as the mapping thread applies it
(current/align2/AbstractMapThread.java:484-487).  A read is (bases_off, len) into a blob, so trimming writes a second read array and
the (left, right) pairs that Mapper.untrim() takes back; no base moves.  trim_batch runs the host form over numpy arrays,
trim_batch_device the device form over torch tensors; both give byte for byte the same output."""
import ctypes as C

import numpy as np

from . import _lib
from .index import READ_DTYPE

MODE_OPTIMAL, MODE_WINDOW, MODE_INTERVAL = 0, 1, 2
TRIM_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4")])


class bbtrim_config(C.Structure):
    _fields_ = [("mode", C.c_int32), ("trimLeft", C.c_int32), ("trimRight", C.c_int32), ("trimq", C.c_int32), ("minLength", C.c_int32),
                ("windowLength", C.c_int32), ("minGoodInterval", C.c_int32), ("optimalBias", C.c_float)]


def default_config(**kw):
    """BBMap's defaults (optimal mode, both sides off, trimq 6, minLength 60, window 4, interval 2, no bias); kw sets fields."""
    L = _lib.load()
    cfg = bbtrim_config()
    _lib.check(L.bbtrim_default_config(C.byref(cfg)), "bbtrim_default_config")
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _parse_boolean(b):
    """Tools.parseBoolean"""
    if b is None or isinstance(b, bool):
        return True if b is None else b
    s = str(b).lower()
    if s in ("t", "true", "1", "yes", ""):
        return True
    if s in ("f", "false", "0", "no"):
        return False
    raise ValueError("not a boolean: %r" % (b,))


def from_flags(qtrim=None, trimq=None, minlength=None, optitrim=None, trimgoodinterval=None):
    """The bbtrim_config BBMap's command line gives: Parser.parseQTrim (current/dna/Parser.java:156-189) for qtrim= (l / left, r / right,
    rl / lr / both, w / window[,N], a leading digit: trimq and the right side, or a boolean), optitrim= (a boolean, or a bias in [0, 1)),
    trimgoodinterval= and trimq=; minlength= is AbstractMapper's TRIM_MIN_LENGTH.  The flags are applied in this order: qtrim, optitrim,
    trimgoodinterval, trimq.  A flag that is None was not given.  One difference: `qtrim=window` without a length keeps the window of
    4 (Parser.java:168 reads split[1], which does not exist there)."""
    cfg = default_config()
    optimal, window = True, False
    if qtrim is not None:
        b = qtrim
        s = "" if isinstance(b, bool) else str(b)
        low = s.lower()
        if isinstance(b, bool):
            cfg.trimLeft = cfg.trimRight = int(b)
        elif s == "":
            cfg.trimLeft = cfg.trimRight = 1
        elif low in ("left", "l"):
            cfg.trimLeft, cfg.trimRight = 1, 0
        elif low in ("right", "r"):
            cfg.trimLeft, cfg.trimRight = 0, 1
        elif low in ("both", "rl", "lr"):
            cfg.trimLeft = cfg.trimRight = 1
        elif low in ("window", "w") or s.startswith("window,") or s.startswith("w,"):
            cfg.trimLeft, cfg.trimRight = 0, 1
            window, optimal = True, False
            parts = s.split(",")
            if len(parts) > 1:
                cfg.windowLength = int(parts[1])
        elif s[0].isdigit():
            cfg.trimq = int(s)
            cfg.trimRight = 1
        else:
            cfg.trimLeft = cfg.trimRight = int(_parse_boolean(s))
    if optitrim is not None:
        s = str(optitrim)
        if not isinstance(optitrim, bool) and s and (s[0] == "." or s[0].isdigit()):
            optimal = True
            cfg.optimalBias = float(s)
            if not 0 <= cfg.optimalBias < 1:
                raise ValueError("optitrim: the bias must be in [0, 1)")
        else:
            optimal = _parse_boolean(optitrim)
    if trimgoodinterval is not None:
        cfg.minGoodInterval = int(trimgoodinterval)
    if trimq is not None:
        cfg.trimq = int(trimq)
    if minlength is not None:
        cfg.minLength = int(minlength)
    cfg.mode = MODE_OPTIMAL if optimal else MODE_WINDOW if window else MODE_INTERVAL      # TrimRead.java:51-61 tests them in this order
    return cfg


def trim_batch(recs, bases, quality=None, cfg=None):
    """bbtrim_batch, the host form.  recs: READ_DTYPE (bases_off, len), bases / quality: uint8 blobs (quality numeric phred at the same
    offsets, or None).  Returns (trimmed READ_DTYPE records: bases_off moved, keys_off = nkeys = 0, TRIM_DTYPE[n])."""
    L = _lib.load()
    cfg = cfg or default_config()
    recs = np.ascontiguousarray(recs, READ_DTYPE)
    b = np.ascontiguousarray(bases, np.uint8).reshape(-1)
    q = None if quality is None else np.ascontiguousarray(quality, np.uint8).reshape(-1)
    assert q is None or q.size >= b.size
    n = len(recs)
    if b.size == 0:
        b = np.zeros(1, np.uint8)
    out, trims = np.zeros(n, READ_DTYPE), np.zeros(n, TRIM_DTYPE)
    _lib.check(L.bbtrim_batch(C.byref(cfg), n, recs.ctypes.data, b.ctypes.data, None if q is None else q.ctypes.data, out.ctypes.data,
                              trims.ctypes.data), "bbtrim_batch")
    return out, trims


def trim_batch_device(recs, bases, quality=None, cfg=None):
    """bbtrim_batch_device over device tensors: recs = the uint8 view of READ_DTYPE as Mapper.reads holds it, bases / quality uint8
    (quality None: reads without qualities).  Returns (trimmed records, trims): new uint8 tensors viewing READ_DTYPE / TRIM_DTYPE;
    recs is not written.  Enqueues on the current stream and does not wait.  As with the mapper, torch must have been imported
    before the library is first loaded."""
    import torch
    L = _lib.load()
    cfg = cfg or default_config()
    dev = bases.device
    assert recs.dtype == torch.uint8 and recs.is_contiguous() and recs.numel() % READ_DTYPE.itemsize == 0 and recs.device == dev
    assert bases.dtype == torch.uint8 and bases.is_contiguous()
    assert quality is None or (quality.dtype == torch.uint8 and quality.is_contiguous() and quality.device == dev and quality.numel() >= bases.numel())
    n = recs.numel() // READ_DTYPE.itemsize
    out = torch.zeros(max(1, n) * READ_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    trims = torch.zeros(max(1, n) * TRIM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    if bases.numel() == 0:          # (an empty tensor has no address)
        bases = torch.zeros(1, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = L.bbtrim_batch_device(C.byref(cfg), C.c_void_p(stream), n, recs.data_ptr() if n else None, bases.data_ptr(),
                                   None if quality is None else quality.data_ptr(), out.data_ptr(), trims.data_ptr())
    _lib.check(rc, "bbtrim_batch_device")
    return out[: n * READ_DTYPE.itemsize], trims[: n * TRIM_DTYPE.itemsize]
