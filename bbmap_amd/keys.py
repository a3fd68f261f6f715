"""Binding of bbkeys_*: the probe's per-read inputs (key offsets, key scores, base scores) -- AbstractMapThread.quickMap up to its
findAdvanced call (current/align2/AbstractMapThread.java:642-728).  make_keys / make_batch run the host form over numpy arrays,
make_batch_device the device form over torch tensors; both give byte for byte the same output."""
import ctypes as C

import numpy as np

from . import _lib
from .index import READ_DTYPE, read_lens

PROFILE_BBMAP, PROFILE_PACBIO = 0, 1


class bbkeys_config(C.Structure):
    _fields_ = [("k", C.c_int32), ("keyDensity", C.c_float), ("maxKeyDensity", C.c_float), ("minKeyDensity", C.c_float),
                ("maxDesiredKeys", C.c_int32), ("minApproxHitsToKeep", C.c_int32), ("semiperfectMode", C.c_int32), ("reserved", C.c_int32)]


def default_config(profile=PROFILE_BBMAP, **kw):
    L = _lib.load()
    cfg = bbkeys_config()
    _lib.check(L.bbkeys_default_config(profile, C.byref(cfg)), "bbkeys_default_config")
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def make_keys(bases, quality=None, cfg=None):
    """One read: returns (offsets, keyScores, baseScores); offsets is empty when quickMap would not probe the read.
    quality: numeric phred values (bytes / uint8 array) or None."""
    L = _lib.load()
    cfg = cfg or default_config()
    b = np.frombuffer(bytes(bases), np.uint8).copy() if not isinstance(bases, np.ndarray) else np.ascontiguousarray(bases, np.uint8)
    n = len(b)
    q = None if quality is None else np.ascontiguousarray(np.frombuffer(bytes(quality), np.uint8) if not isinstance(quality, np.ndarray) else quality, np.uint8)
    cap = max(1, n)
    offs, ks, bs = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(max(1, n), np.int8)
    m = L.bbkeys_make(C.byref(cfg), b.ctypes.data, None if q is None else q.ctypes.data, n, offs.ctypes.data, ks.ctypes.data, cap, bs.ctypes.data)
    if m < 0:
        _lib.check(m, "bbkeys_make")
    return offs[:m].tolist(), ks[:m].tolist(), bs[:n]


def make_batch(reads, qualities=None, cfg=None):
    """reads: list of uint8 arrays / bytes (any lengths); qualities: None or a list of the same shapes (numeric phred).
    Returns (recs [READ_DTYPE], bases blob, baseScores blob, keyinfo) laid out as bbmap_map_batch_device / bbidx_find_batch take them."""
    L = _lib.load()
    cfg = cfg or default_config()
    arrs = [np.frombuffer(bytes(r), np.uint8) if not isinstance(r, np.ndarray) else np.ascontiguousarray(r, np.uint8) for r in reads]
    lens = np.array([len(a) for a in arrs], np.int32)
    offs = np.zeros(len(arrs), np.int64)
    if len(arrs) > 1:
        offs[1:] = np.cumsum(lens[:-1].astype(np.int64))
    blob = np.concatenate(arrs) if arrs else np.zeros(1, np.uint8)
    qblob = None
    if qualities is not None:
        qblob = np.concatenate([np.frombuffer(bytes(q), np.uint8) if not isinstance(q, np.ndarray) else np.ascontiguousarray(q, np.uint8) for q in qualities])
        assert len(qblob) == len(blob)
    recs = np.zeros(len(arrs), READ_DTYPE)
    cap = int(2 * lens.astype(np.int64).sum()) + 2
    keyinfo = np.zeros(cap, np.int32)
    bs = np.zeros(max(1, len(blob)), np.int8)
    used = C.c_int64(0)
    _lib.check(L.bbkeys_make_batch(C.byref(cfg), len(arrs), offs.ctypes.data, lens.ctypes.data, blob.ctypes.data,
                                   None if qblob is None else qblob.ctypes.data, recs.ctypes.data, keyinfo.ctypes.data, cap, bs.ctypes.data,
                                   C.byref(used)), "bbkeys_make_batch")
    return recs, blob, bs, keyinfo[:max(1, used.value)].copy()


_workspace = {}          # torch device -> the uint8 tensor make_batch_device hands to the library, grown on demand


def workspace_bytes(cfg, n_reads, total_bases):
    L = _lib.load()
    nb = L.bbkeys_device_workspace_bytes(C.byref(cfg), n_reads, total_bases)
    if nb < 0:
        _lib.check(int(nb), "bbkeys_device_workspace_bytes")
    return int(nb)


def keyinfo_bound(cfg, n_reads, total_bases):
    """Ints of keyinfo that hold the keys of any n_reads reads with total_bases bases in all: a read gets at most
    max(2, ceil(len * keyDensity / k)) keys (KeyRing.desiredKeysFromDensity), and never more than len."""
    per_base = float(cfg.keyDensity) / cfg.k
    return 2 * min(total_bases, 3 * n_reads + int(np.ceil(total_bases * per_base * 1.001)) + 1)


def make_batch_device(recs, bases, quality=None, cfg=None, keyinfo_cap=None):
    """bbkeys_make_batch_device: the key stage over a batch that is already in device memory.  recs: the uint8 view of READ_DTYPE as
    Mapper.reads holds it (bases_off and len filled in), bases / quality: uint8 device tensors (quality numeric phred, or None).
    Fills recs' keys_off / nkeys in place and returns (recs, keyinfo[:used], base_scores), device tensors; keyinfo_cap: ints of
    keyinfo to allocate (default: enough for any qualities).  Runs on the current stream and waits for it.  As with the mapper, torch
    must have been imported before the library is first loaded (bbmap_amd.mapper imports it at its top), so that both use one HIP
    runtime."""
    import torch
    L = _lib.load()
    cfg = cfg or default_config()
    dev = bases.device
    assert recs.dtype == torch.uint8 and recs.is_contiguous() and recs.numel() % READ_DTYPE.itemsize == 0 and recs.device == dev
    assert bases.dtype == torch.uint8 and bases.is_contiguous()
    assert quality is None or (quality.dtype == torch.uint8 and quality.is_contiguous() and quality.device == dev and quality.numel() >= bases.numel())
    n = recs.numel() // READ_DTYPE.itemsize
    total = int(read_lens(recs).clamp(min=0).sum(dtype=torch.int64).item()) if n else 0
    cap = keyinfo_bound(cfg, n, total) if keyinfo_cap is None else int(keyinfo_cap)
    keyinfo = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
    base_scores = torch.zeros(max(1, bases.numel()), dtype=torch.int8, device=dev)
    need = workspace_bytes(cfg, n, total)
    ws = _workspace.get(dev)
    if ws is None or ws.numel() < need:
        _workspace[dev] = ws = torch.empty(need + need // 8 + 256, dtype=torch.uint8, device=dev)
    used = C.c_int64(0)
    if bases.numel() == 0:          # (an empty tensor has no address; the library wants one even for reads without bases)
        bases = torch.zeros(1, dtype=torch.uint8, device=dev)
        quality = None if quality is None else bases
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = L.bbkeys_make_batch_device(C.byref(cfg), C.c_void_p(stream), n, recs.data_ptr(), bases.data_ptr(),
                                        None if quality is None else quality.data_ptr(), keyinfo.data_ptr(), cap, base_scores.data_ptr(),
                                        ws.data_ptr(), ws.numel(), C.byref(used))
    _lib.check(rc, "bbkeys_make_batch_device")
    return recs, keyinfo[:used.value], base_scores
