"""Python binding of the device-resident mapper (bbmap_* in include/bbmap_amd.h): probe -> pairing / trimming -> ungapped
scores -> scoreSlow in rounds -> rescue, everything in HBM.  Used by bench.py and the tests; needs torch for device buffers."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import msa as M
from .index import READ_DTYPE, read_lens

MSITE_DTYPE = np.dtype([("chrom", "<i4"), ("strand", "<i4"), ("start", "<i4"), ("stop", "<i4"), ("hits", "<i4"),
                        ("quickScore", "<i4"), ("score", "<i4"), ("slowScore", "<i4"), ("pairedScore", "<i4"),
                        ("perfect", "<i4"), ("semiperfect", "<i4"), ("rescued", "<i4"), ("ngaps", "<i4"),
                        ("gaps", "<i4", (16,)), ("match_job", "<i4"), ("reserved", "<i4", (2,))])
JOBINFO_DTYPE = np.dtype([("read", "<i4"), ("seq", "<i4"), ("kind", "<i4"), ("site", "<i4")])
# bbmap_final: what BBMap prints for a read (the final alignment stage)
FINAL_DTYPE = np.dtype([("mapped", "<i4"), ("chrom", "<i4"), ("strand", "<i4"), ("start", "<i4"), ("stop", "<i4"), ("mapScore", "<i4"),
                        ("paired", "<i4"), ("ambiguous", "<i4"), ("perfect", "<i4"), ("rescued", "<i4"), ("match_len", "<i4"),
                        ("nsites", "<i4"), ("match_off", "<i8"), ("reserved", "<i4", (2,))])
# bbmap_scafrec: SamLine's scaffold coordinates of a final record (bbmap_get_scaffold_records); flags = SCAF_* bits
SCAFREC_DTYPE = np.dtype([("scaffold", "<i4"), ("start", "<i4"), ("stop", "<i4"), ("pos", "<i4"), ("end", "<i4"), ("scaflen", "<i4"),
                          ("flags", "<i4"), ("reserved", "<i4")])
SCAF_MAPPED, SCAF_PAIRED, SCAF_INBOUNDS, SCAF_SAME_SCAFFOLD = 1, 2, 4, 8
# bbmap_samrec: the fields of a SAM line (bbmap_get_sam_records); rname / rnext = global scaffold numbers (-1 `*`, rnext -2 `=`),
# nm / am -1 = no tag, cigar_len / md_len 0 = none, offsets into the text blob
SAMREC_DTYPE = np.dtype([("flag", "<i4"), ("mapq", "<i4"), ("rname", "<i4"), ("rnext", "<i4"), ("pos", "<i4"), ("pnext", "<i4"),
                         ("tlen", "<i4"), ("nm", "<i4"), ("am", "<i4"), ("tags", "<i4"), ("cigar_off", "<i8"), ("cigar_len", "<i4"),
                         ("md_len", "<i4"), ("md_off", "<i8")])
SAM_CIGAR13, SAM_MD = 1, 2
SAM_TAG_XT = 1
# bbmap_samtags: the further optional tags of a SAM line as values (bbmap_get_sam_records_cfg); `present` = SAM_MAKE_* bits
SAMTAGS_DTYPE = np.dtype([(n, "<i4") for n in ("present", "xs", "nh", "sm", "xm", "ys", "yl_query", "yl_ref", "yi_good", "yi_bad",
                                               "yi_perfect", "yr", "x8", "xb", "introns", "splices")])
# bbmap_sam_config.tags: which optional tags are made (BBMAP_SAM_MAKE_*; one Python copy of the bits, in bbmap_amd.sam)
from .sam import (MAKE_AM as SAM_MAKE_AM, MAKE_BOUNDS as SAM_MAKE_BOUNDS, MAKE_IDENTITY as SAM_MAKE_IDENTITY,  # noqa: E402
                  MAKE_INSERT as SAM_MAKE_INSERT, MAKE_LENGTH as SAM_MAKE_LENGTH, MAKE_NH as SAM_MAKE_NH, MAKE_NM as SAM_MAKE_NM,
                  MAKE_SCORE as SAM_MAKE_SCORE, MAKE_SM as SAM_MAKE_SM, MAKE_STOP as SAM_MAKE_STOP, MAKE_XM as SAM_MAKE_XM,
                  MAKE_XS as SAM_MAKE_XS, NO_TAGS as SAM_NO_TAGS, XS_SECONDSTRAND as SAM_XS_SECONDSTRAND)
SAM_DEFAULT_TAGS = SAM_MAKE_NM | SAM_MAKE_AM
SAM_ALL_TAGS = (SAM_DEFAULT_TAGS | SAM_MAKE_SM | SAM_MAKE_XM | SAM_MAKE_XS | SAM_MAKE_NH | SAM_MAKE_STOP | SAM_MAKE_LENGTH |
                SAM_MAKE_IDENTITY | SAM_MAKE_SCORE | SAM_MAKE_INSERT | SAM_MAKE_BOUNDS)
SAM_NO_INTRON_LIMIT = 2 ** 31 - 1
GAPPED_BIT = 1 << 30


class bbmap_config(C.Structure):
    _fields_ = [("device", C.c_int32), ("paired", C.c_int32), ("max_reads", C.c_int32), ("max_read_len", C.c_int32),
                ("max_sites", C.c_int32), ("minRatio", C.c_float)] + [(n, C.c_int32) for n in (
                    "slowAlignPadding", "slowRescuePadding", "extraPadding", "tipSearchDist", "maxPairDist", "averagePairDist",
                    "maxRescueDist", "maxRescueMismatches", "maxTrimSitesToRetain", "trimList", "doRescue", "alignColumns",
                    "clearzone3", "msaMaxColumns", "fastCols", "jobsPerRead", "finalStage")] + [("reserved", C.c_int32 * 4)]


class bbmap_sam_config(C.Structure):
    _fields_ = [("flags", C.c_int32), ("intronLimit", C.c_int32), ("tags", C.c_int32), ("reserved", C.c_int32 * 5)]


def sam_config(flags=0, intron_limit=None, tags=None):
    """bbmap_sam_default_config with the given fields replaced (None = the default: no limit, NM and AM)."""
    return bbmap_sam_config(int(flags), SAM_NO_INTRON_LIMIT if intron_limit is None else int(intron_limit),
                            SAM_DEFAULT_TAGS if tags is None else int(tags))


class bbmap_output(C.Structure):
    _fields_ = [("sites", C.c_void_p), ("nsites", C.c_void_p), ("cap", C.c_int32), ("match_stride", C.c_int32),
                ("gmatch_stride", C.c_int32), ("reserved", C.c_int32), ("n_jobs", C.c_int64), ("n_gapped_jobs", C.c_int64),
                ("jobs", C.c_void_p), ("results", C.c_void_p), ("jobinfo", C.c_void_p), ("match", C.c_void_p),
                ("gjobs", C.c_void_p), ("gresults", C.c_void_p), ("gjobinfo", C.c_void_p), ("gmatch", C.c_void_p),
                ("ggaps", C.c_void_p), ("final", C.c_void_p), ("final_match", C.c_void_p), ("final_match_bytes", C.c_int64),
                ("n_final_fills", C.c_int64)]


class bbmap_stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("reads", "reads_overflowed", "reads_without_site", "fills", "gapped_fills", "refills",
                                         "rescue_scans", "rescue_fills", "rounds", "fills_dropped")] + \
               [(n, C.c_float) for n in ("ms_probe", "ms_begin", "ms_score", "ms_slow", "ms_finish", "ms_rescue", "ms_total",
                                         "ms_dp_narrow", "ms_dp_wave", "ms_dp_generic", "ms_dp_gapped", "ms_quick_rescue")] + \
               [("probe_stats", C.c_int64 * 5), ("reads_reprobed", C.c_int64), ("ms_overflow", C.c_float), ("log_growths", C.c_float),
                ("ms_dp_wave_max", C.c_float), ("ms_final", C.c_float), ("final_fills", C.c_int64), ("final_rounds", C.c_int64),
                ("final_local", C.c_int64), ("dp_narrow_launches", C.c_int64), ("dp_sorted_launches", C.c_int64),
                ("sites_cross_scaffold", C.c_int64)]


class bbmap_overflow_output(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("read_ids", C.c_void_p), ("out", bbmap_output)]


NSITES_OVERFLOW, NSITES_MATE_OVERFLOW, NSITES_IN_TIER = -1, -2, -3


def sam_workspace_bytes(n_reads, max_read_len):
    """bbpipe_sam_records_workspace_bytes"""
    L = _lib.load()
    b = L.bbpipe_sam_records_workspace_bytes(int(n_reads), int(max_read_len))
    if b < 0:
        _lib.check(int(b), "bbpipe_sam_records_workspace_bytes")
    return int(b)


def sam_records_device(reads, bases, finals, pool, scaf, recs, text, text_bytes, workspace, paired=False, flags=0, intron_limit=None,
                       tags=None, tagrecs=None, sites=None, nsites=None, cap=0, chrom_arr=None, chrom_arr_len=None, max_read_len=600):
    """bbpipe_sam_records_device over torch device tensors the caller owns: uint8 views of READ_DTYPE / FINAL_DTYPE / SCAFREC_DTYPE
    records, the bases and the match-string pool (uint8); outputs recs (uint8, n x 64 bytes), tagrecs (uint8, n x 64 bytes, or None: the
    tag records are not made), text (uint8: its length is the blob's capacity), text_bytes (int64[1]: the bytes the blob needs);
    workspace: uint8, sam_workspace_bytes(n, max_read_len) long.  sites (uint8 view of MSITE_DTYPE[n, cap]) / nsites (int32) for XM;
    chrom_arr (int64: device addresses by chromosome number) / chrom_arr_len (int32) for MD.  Enqueues on the current stream and does
    not wait."""
    L = _lib.load()
    n = reads.numel() // READ_DTYPE.itemsize
    cfg = sam_config(flags, intron_limit, tags)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.bbpipe_sam_records_device(C.c_void_p(stream), n, int(bool(paired)), C.byref(cfg), int(max_read_len), ptr(reads), ptr(bases),
                                           ptr(finals), ptr(pool), ptr(scaf), ptr(sites), ptr(nsites), int(cap), ptr(chrom_arr),
                                           ptr(chrom_arr_len), ptr(recs), ptr(tagrecs), ptr(text), int(text.numel()), ptr(text_bytes),
                                           ptr(workspace), int(workspace.numel())), "bbpipe_sam_records_device")


def _copy(ptr, nbytes, dev=None):
    """device memory -> numpy bytes (bbmap_copy_to_host)"""
    out = np.empty(max(nbytes, 0), np.uint8)
    if nbytes > 0:
        L = _lib.load()
        _lib.check(L.bbmap_copy_to_host(out.ctypes.data, C.c_void_p(ptr), nbytes), "bbmap_copy_to_host")
    return out


class Mapper:
    """One bbmap_ctx over a DeviceIndex.  Mapper(...) is the fixed-length form: reads of one length, all with the same key offsets /
    key scores.  from_records / from_reads take reads of any lengths with keys of their own; in paired mode the mates of a pair may
    differ in length (each stage uses the length of the mate it works on, as BBMapThread.processReadPair does)."""

    def _open(self, di, n, read_len, paired, device, max_sites, cfg_kw, profile=None):
        """What the three entry points share: the default bbmap_config (profile None: Mapper(...)'s, bbmap.sh's defaults with the
        read length as given and always announced to the index; otherwise the profile's, a length of at least 1, announced for
        profile 0 only), the five sizing fields, cfg_kw on top, and the context."""
        self.L = _lib.load()
        self.di, self.n, self.read_len, self.paired = di, n, read_len, paired
        self.dev = torch.device("cuda", device)
        cfg = bbmap_config()
        if profile is None:
            max_len = read_len
            _lib.check(self.L.bbmap_default_config(C.byref(cfg)), "bbmap_default_config")
        else:
            max_len = max(1, read_len)
            _lib.check(self.L.bbmap_default_config_profile(profile, C.byref(cfg)), "bbmap_default_config_profile")
        if not profile:
            di.set_max_read_len(max_len)
        cfg.device, cfg.paired, cfg.max_reads, cfg.max_read_len, cfg.max_sites = device, int(paired), n, max_len, max_sites
        for k, v in cfg_kw.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        h = C.c_void_p()
        _lib.check(self.L.bbmap_create(di.h, C.byref(cfg), C.byref(h)), "bbmap_create")
        self.h = h

    def _upload_bases(self, blob):
        """A fresh doubled buffer with the blob in its first half: plus strands, then the reverse complements a step writes."""
        self.total_bytes = int(blob.size)
        self.bases = torch.zeros(2 * self.total_bytes, dtype=torch.uint8, device=self.dev)
        self.bases[: self.total_bytes].copy_(torch.from_numpy(blob))

    def __init__(self, di, n_reads, read_len, offsets, key_scores, paired=False, device=0, max_sites=32, **cfg_kw):
        self._open(di, n_reads, read_len, paired, device, max_sites, cfg_kw)
        self.total_bytes = n_reads * read_len
        self.bases = torch.zeros(2 * self.total_bytes, dtype=torch.uint8, device=self.dev)       # plus strands, then reverse complements
        self.base_scores = torch.zeros(self.total_bytes, dtype=torch.int8, device=self.dev)
        recs = np.zeros(n_reads, READ_DTYPE)
        recs["bases_off"] = np.arange(n_reads, dtype=np.int64) * read_len
        recs["keys_off"] = 0
        recs["len"] = read_len
        recs["nkeys"] = len(offsets)
        self.reads = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(self.dev)
        self.keyinfo = torch.tensor(list(offsets) + list(key_scores), dtype=torch.int32, device=self.dev)

    @classmethod
    def from_records(cls, di, recs, bases, base_scores, keyinfo, paired=False, device=0, max_sites=32, profile=0, **cfg_kw):
        """The general form: reads of any lengths with their own keys, as bbkeys_make_batch (bbmap_amd.keys.make_batch) lays them
        out -- recs (READ_DTYPE), the bases blob, base scores at the same offsets, keyinfo.  profile: 0 = bbmap.sh's classes,
        1 = mapPacBio.sh's (BBIDX_PROFILE_*; must be the index's).  cfg_kw sets bbmap_config fields, e.g. finalStage = 1 for
        mapPacBio's final records (off by default for that profile; 2 = BBMapThread's tail, for parity tests)."""
        self = cls.__new__(cls)
        recs = np.ascontiguousarray(recs, READ_DTYPE)
        self._open(di, len(recs), int(recs["len"].max()) if len(recs) else 0, paired, device, max_sites, cfg_kw, profile)
        self._upload_bases(np.ascontiguousarray(bases, np.uint8))
        self.base_scores = torch.from_numpy(np.ascontiguousarray(base_scores, np.int8)).to(self.dev)
        assert self.base_scores.numel() >= self.total_bytes
        self.reads = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(self.dev)
        self.keyinfo = torch.from_numpy(np.ascontiguousarray(keyinfo, np.int32)).to(self.dev)
        return self

    @classmethod
    def from_reads(cls, di, lens, bases, quality=None, kcfg=None, paired=False, device=0, max_sites=32, profile=0, trim=None, untrim=False,
                   **cfg_kw):
        """from_records for reads that have no keys yet: lens (one per read) and the bases blob the reads lie in back to back, with
        their numeric phred qualities at the same offsets or None.  Uploads them and runs quickMap's key stage on the device
        (bbmap_amd.keys.make_batch_device), so reads, keyinfo and base_scores exist in device memory only.  kcfg: a bbkeys_config
        (default: keys.default_config(profile)); profile and cfg_kw as in from_records.
        trim: a bbtrim_config (bbmap_amd.trim.from_flags / default_config): the trim stage (qtrim= / trimq=) runs on the device in
        front of the key stage and the mapper maps the trimmed records; self.reads_untrimmed and self.trims keep what untrim() needs.
        untrim only stores the intent (self.untrim_wanted): step() does not call untrim(), because add_run_stats() has to come before
        it and that order is the caller's."""
        from . import keys as K
        self = cls.__new__(cls)
        lens = np.ascontiguousarray(lens, np.int32)
        n = len(lens)
        recs = np.zeros(n, READ_DTYPE)
        recs["len"] = lens
        if n > 1:
            recs["bases_off"][1:] = np.cumsum(lens[:-1].astype(np.int64))
        blob = np.ascontiguousarray(bases, np.uint8).reshape(-1)
        assert blob.size >= int(lens.astype(np.int64).sum())
        self._open(di, n, int(lens.max()) if n else 0, paired, device, max_sites, cfg_kw, profile)
        self._upload_bases(blob)
        q = None
        if quality is not None:
            qblob = np.ascontiguousarray(quality, np.uint8).reshape(-1)
            assert qblob.size == blob.size
            q = torch.from_numpy(qblob).to(self.dev)
        self.quality = q                    # add_read_hist()'s default
        self.reads = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(self.dev)
        self.reads_untrimmed = self.trims = None
        self.untrim_wanted = bool(untrim)
        if trim is not None:
            from . import trim as T
            self.reads_untrimmed = self.reads
            self.reads, self.trims = T.trim_batch_device(self.reads_untrimmed, self.bases[: self.total_bytes], q, trim)
            if n and int(read_lens(self.reads).min().item()) <= 0:
                raise ValueError("Mapper.from_reads: trimming left a read without bases (possible with minLength <= 0 only); "
                                 "the mapper takes no zero-length read")
        _, keyinfo, self.base_scores = K.make_batch_device(self.reads, self.bases[: self.total_bytes], q, kcfg or K.default_config(profile))
        self.keyinfo = keyinfo if keyinfo.numel() else torch.zeros(1, dtype=torch.int32, device=self.dev)
        return self

    def close(self):
        if getattr(self, "h", None):
            self.L.bbmap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_reads(self, reads_u8):
        """reads_u8: n_reads x read_len bases; paired mode: mates interleaved (read 2p, 2p+1)."""
        assert reads_u8.size == self.total_bytes
        self.quality = None                 # (the qualities from_reads uploaded belong to the reads it was given)
        self.bases[: self.total_bytes].copy_(torch.from_numpy(np.ascontiguousarray(reads_u8).reshape(-1)))

    def load_records(self, recs, bases, base_scores, keyinfo):
        """Another batch for a context made by from_records, laid out the same way: no more reads than the context was made for and
        none longer than its longest."""
        recs = np.ascontiguousarray(recs, READ_DTYPE)
        assert 0 < len(recs) <= self.cfg.max_reads and int(recs["len"].max()) <= self.cfg.max_read_len
        blob = np.ascontiguousarray(bases, np.uint8)
        self.n = len(recs)
        self.quality = None                 # (the qualities from_reads uploaded belong to the reads it was given)
        self.reads_untrimmed = self.trims = None            # (and so do its trims)
        self._upload_bases(blob)
        self.base_scores = torch.from_numpy(np.ascontiguousarray(base_scores, np.int8)).to(self.dev)
        assert self.base_scores.numel() >= self.total_bytes
        self.reads = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(self.dev)
        self.keyinfo = torch.from_numpy(np.ascontiguousarray(keyinfo, np.int32)).to(self.dev)

    def step(self, bases=None):
        """Maps the resident batch; returns when it is done (bbmap_map_batch_device waits for its stream).  bases: another
        device buffer of 2 * n_reads * read_len bytes holding the batch's plus strands in its first half (a host that streams
        batches uploads the next one while this one is mapped)."""
        stream = torch.cuda.current_stream().cuda_stream
        b = self.bases if bases is None else bases
        self._stepped_own_bases = b is self.bases
        assert b.numel() == 2 * self.total_bytes and b.dtype == torch.uint8
        _lib.check(self.L.bbmap_map_batch_device(self.h, C.c_void_p(stream), self.n, self.reads.data_ptr(), b.data_ptr(),
                                                 self.total_bytes, self.base_scores.data_ptr(), self.keyinfo.data_ptr()),
                   "bbmap_map_batch_device")

    def map_batch_host(self, recs, bases, base_scores, keyinfo, sites_cap):
        """bbmap_map_batch: host buffers in, packed site lists out (what the JNI glue calls).  Returns (nsites int32[n],
        offsets int64[n + 1], records MSITE_DTYPE[min(total, sites_cap)], total)."""
        recs = np.ascontiguousarray(recs, READ_DTYPE)
        bases = np.ascontiguousarray(bases, np.uint8)
        base_scores = np.ascontiguousarray(base_scores, np.int8)
        keyinfo = np.ascontiguousarray(keyinfo, np.int32)
        n = len(recs)
        ns = np.zeros(n, np.int32)
        offs = np.zeros(n + 1, np.int64)
        sites = np.zeros(max(1, sites_cap), MSITE_DTYPE)
        total = C.c_int64(0)
        _lib.check(self.L.bbmap_map_batch(self.h, n, recs.ctypes.data, bases.ctypes.data, bases.size, base_scores.ctypes.data,
                                          keyinfo.ctypes.data, keyinfo.size, ns.ctypes.data, offs.ctypes.data, sites.ctypes.data,
                                          sites_cap, C.byref(total)), "bbmap_map_batch")
        return ns, offs, sites[:min(total.value, sites_cap)], total.value

    def untrim(self):
        """bbmap_untrim_batch_device: TrimRead.untrim over the last step of a context made by from_reads(trim=...): the final records,
        site lists and match strings get the trimmed ends back as soft clips, and everything called afterwards (final, fetch,
        sam_records, add_coverage, add_read_hist) works on the full reads.  add_run_stats() must come first (calcStatistics runs on
        the trimmed read); a second call for one step raises."""
        if getattr(self, "trims", None) is None:
            raise ValueError("Mapper.untrim: the context was not made by from_reads(trim=...)")
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.L.bbmap_untrim_batch_device(self.h, C.c_void_p(stream), self.reads_untrimmed.data_ptr(), self.trims.data_ptr()),
                   "bbmap_untrim_batch_device")

    def final(self, with_match=True):
        """bbmap_get_final: (records FINAL_DTYPE[n], match blob uint8[]) of the last step, overflow tier included; read r's match
        string is blob[match_off : match_off + match_len]."""
        fin = np.zeros(self.n, FINAL_DTYPE)
        nb = C.c_int64(0)
        _lib.check(self.L.bbmap_get_final(self.h, self.n, fin.ctypes.data, None, 0, C.byref(nb)), "bbmap_get_final")
        blob = np.zeros(max(1, nb.value), np.uint8)
        if with_match and nb.value:
            _lib.check(self.L.bbmap_get_final(self.h, self.n, fin.ctypes.data, blob.ctypes.data, blob.size, C.byref(nb)), "bbmap_get_final")
        return fin, blob

    def final_only(self, sites, nsites):
        """bbmap_final_batch_device: the final alignment stage alone over the given site lists (MSITE_DTYPE[n, cap], int32[n]); the
        reverse complements must be in place (a step() wrote them)."""
        st = np.ascontiguousarray(sites, MSITE_DTYPE)
        assert st.shape == (self.n, self.cfg.max_sites)
        d_sites = torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).to(self.dev)
        d_ns = torch.from_numpy(np.ascontiguousarray(nsites, np.int32)).to(self.dev)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.L.bbmap_final_batch_device(self.h, C.c_void_p(stream), self.n, self.reads.data_ptr(), self.bases.data_ptr(),
                                                   self.total_bytes, d_sites.data_ptr(), d_ns.data_ptr()), "bbmap_final_batch_device")

    def scaffold_records(self):
        """bbmap_get_scaffold_records: SamLine's scaffold coordinates of the last step's final records, overflow tier included.
        Returns (SCAFREC_DTYPE[n], names): names[i] = the name of scaffold i (global number) as the index's table was set from
        DeviceIndex.set_scaffolds (None when the table was set without names)."""
        p = C.c_void_p()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.L.bbmap_get_scaffold_records(self.h, C.c_void_p(stream), C.byref(p)), "bbmap_get_scaffold_records")
        torch.cuda.current_stream().synchronize()
        recs = _copy(p.value, self.n * SCAFREC_DTYPE.itemsize, self.dev).view(SCAFREC_DTYPE)
        return recs, getattr(self.di, "scaffold_names", None)

    def sam_records(self, flags=0, intron_limit=None, tags=None):
        """bbmap_get_sam_records: SamLine's fields for the last step's final records, overflow tier included, built on the device.
        flags: SAM_CIGAR13 | SAM_MD.  Returns (SAMREC_DTYPE[n], text uint8[]): read r's CIGAR is text[cigar_off : + cigar_len], its MD
        value text[md_off : + md_len] (bbmap_amd.sam formats lines from them).
        With intron_limit (SamLine.INTRON_LIMIT, `intronlen=`) or tags (SAM_MAKE_* bits) given: bbmap_get_sam_records_cfg, and the return
        value is (SAMREC_DTYPE[n], SAMTAGS_DTYPE[n], text)."""
        p, t, nb = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        stream = torch.cuda.current_stream().cuda_stream
        if intron_limit is not None or tags is not None:
            g, cfg = C.c_void_p(), sam_config(flags, intron_limit, tags)
            _lib.check(self.L.bbmap_get_sam_records_cfg(self.h, C.c_void_p(stream), C.byref(cfg), C.byref(p), C.byref(g), C.byref(t), C.byref(nb)),
                       "bbmap_get_sam_records_cfg")
            torch.cuda.current_stream().synchronize()
            return (_copy(p.value, self.n * SAMREC_DTYPE.itemsize, self.dev).view(SAMREC_DTYPE),
                    _copy(g.value, self.n * SAMTAGS_DTYPE.itemsize, self.dev).view(SAMTAGS_DTYPE), _copy(t.value, nb.value, self.dev))
        _lib.check(self.L.bbmap_get_sam_records(self.h, C.c_void_p(stream), int(flags), C.byref(p), C.byref(t), C.byref(nb)),
                   "bbmap_get_sam_records")
        torch.cuda.current_stream().synchronize()
        recs = _copy(p.value, self.n * SAMREC_DTYPE.itemsize, self.dev).view(SAMREC_DTYPE)
        return recs, _copy(t.value, nb.value, self.dev)

    def sam_records_host(self, flags=0, intron_limit=None, tags=None):
        """bbmap_get_sam: the same through the host-buffer form (records first, then the blob once its size is known); with
        intron_limit or tags given bbmap_get_sam_cfg, returning (recs, tags, text)."""
        recs = np.zeros(self.n, SAMREC_DTYPE)
        nb = C.c_int64(0)
        if intron_limit is not None or tags is not None:
            cfg, tg = sam_config(flags, intron_limit, tags), np.zeros(self.n, SAMTAGS_DTYPE)
            _lib.check(self.L.bbmap_get_sam_cfg(self.h, self.n, C.byref(cfg), recs.ctypes.data, tg.ctypes.data, None, 0, C.byref(nb)), "bbmap_get_sam_cfg")
            text = np.zeros(max(1, nb.value), np.uint8)
            _lib.check(self.L.bbmap_get_sam_cfg(self.h, self.n, C.byref(cfg), recs.ctypes.data, tg.ctypes.data, text.ctypes.data, text.size,
                                                C.byref(nb)), "bbmap_get_sam_cfg")
            return recs, tg, text[:nb.value]
        _lib.check(self.L.bbmap_get_sam(self.h, self.n, int(flags), recs.ctypes.data, None, 0, C.byref(nb)), "bbmap_get_sam")
        text = np.zeros(max(1, nb.value), np.uint8)
        _lib.check(self.L.bbmap_get_sam(self.h, self.n, int(flags), recs.ctypes.data, text.ctypes.data, text.size, C.byref(nb)), "bbmap_get_sam")
        return recs, text[:nb.value]

    def set_average_pair_dist(self, v):
        _lib.check(self.L.bbmap_set_average_pair_dist(self.h, int(v)), "bbmap_set_average_pair_dist")

    def _truth_tensor(self, truth):
        from .runstats import TRUTH_DTYPE
        t = np.ascontiguousarray(truth, TRUTH_DTYPE)
        assert len(t) == self.n
        return torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def add_run_stats(self, truth=None):
        """bbmap_add_run_stats: adds the last step, overflow tier included, to the context's running counters and insert-size
        histogram.  truth: TRUTH_DTYPE[n] (chrom < 0 = none for that read) or None.  A second call for one step raises."""
        d = None if truth is None else self._truth_tensor(truth)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.L.bbmap_add_run_stats(self.h, C.c_void_p(stream), None if d is None else C.c_void_p(d.data_ptr())),
                   "bbmap_add_run_stats")
        torch.cuda.current_stream().synchronize()          # (the truth tensor may go now)

    def run_stats(self, with_hist=True):
        """bbmap_get_run_stats: (RUNSTATS_DTYPE scalar, int64[INSERT_HIST_BINS] or None)."""
        from .runstats import RUNSTATS_DTYPE, INSERT_HIST_BINS
        rs = np.zeros(1, RUNSTATS_DTYPE)
        hist = np.zeros(INSERT_HIST_BINS, np.int64) if with_hist else None
        _lib.check(self.L.bbmap_get_run_stats(self.h, rs.ctypes.data, None if hist is None else hist.ctypes.data), "bbmap_get_run_stats")
        return rs[0], hist

    def reset_run_stats(self):
        _lib.check(self.L.bbmap_reset_run_stats(self.h), "bbmap_reset_run_stats")

    def set_adaptive(self, flags):
        """bbmap_set_adaptive: ADAPT_INSERT_LENGTH | ADAPT_RESCUE_SKIP (bbmap_amd.runstats); step() then counts each batch itself."""
        _lib.check(self.L.bbmap_set_adaptive(self.h, int(flags)), "bbmap_set_adaptive")

    def set_truth(self, truth):
        """bbmap_set_truth: truth records for the next step's own accumulation (adaptive contexts); None clears."""
        self._truth = None if truth is None else self._truth_tensor(truth)      # kept alive until the next step has used it
        _lib.check(self.L.bbmap_set_truth(self.h, None if self._truth is None else C.c_void_p(self._truth.data_ptr())), "bbmap_set_truth")

    def adaptive_state(self):
        """bbmap_get_adaptive_state: (averagePairDist, rescueSkipped)."""
        a, r = C.c_int32(0), C.c_int32(0)
        _lib.check(self.L.bbmap_get_adaptive_state(self.h, C.byref(a), C.byref(r)), "bbmap_get_adaptive_state")
        return a.value, r.value

    def enable_coverage(self, flags=0):
        """bbmap_cov_enable: allocates the coverage state for the index's scaffold table (flags: bbmap_amd.coverage.COV_*)."""
        _lib.check(self.L.bbmap_cov_enable(self.h, int(flags)), "bbmap_cov_enable")

    def add_coverage(self):
        """bbmap_add_coverage: adds the last step, overflow tier included.  A second call for one step raises."""
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.L.bbmap_add_coverage(self.h, C.c_void_p(stream)), "bbmap_add_coverage")

    def coverage(self, binsize=1000):
        """bbmap_cov_finalize: a snapshot of everything added so far as a bbmap_amd.coverage.Coverage (numpy arrays)."""
        from . import coverage as V
        w = V.bbmap_cov_view()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.L.bbmap_cov_finalize(self.h, C.c_void_p(stream), int(binsize), C.byref(w)), "bbmap_cov_finalize")
        torch.cuda.current_stream().synchronize()
        strands = 2 if w.flags & V.COV_STRANDED else 1
        ddt = np.int32 if w.depth_bytes == 4 else np.uint16
        arr = lambda p, count, dt: _copy(p, count * np.dtype(dt).itemsize, self.dev).view(dt)
        return V.Coverage(w.flags, arr(w.recs, w.nscaf, V.COVREC_DTYPE), arr(w.totals, 1, V.COVTOTALS_DTYPE)[0], arr(w.covoff, w.nscaf + 1, np.int64),
                          [arr(w.depth[t], w.slots, ddt) for t in range(strands)], [arr(w.hist[t], w.hist_bins, np.int64) for t in range(strands)],
                          int(binsize), arr(w.binoff, w.nscaf + 1, np.int64) if binsize > 0 else None,
                          [arr(w.bins[t], w.nbins, np.int64) for t in range(strands)] if binsize > 0 else None,
                          getattr(self.di, "scaffold_names", None))

    def coverage_host(self, binsize=1000):
        """bbmap_get_coverage, the host-buffer form: sizes first, then everything into buffers that hold it.  Returns a Coverage
        without covoff-independent extras (covoff and binoff are bbmap_amd.coverage.layout's)."""
        from . import coverage as V
        nscaf = len(self.di.scaffold_names)
        recs, totals, w = np.zeros(nscaf, V.COVREC_DTYPE), np.zeros(1, V.COVTOTALS_DTYPE), V.bbmap_cov_view()
        _lib.check(self.L.bbmap_get_coverage(self.h, int(binsize), recs.ctypes.data, nscaf, totals.ctypes.data, None, 0, None, 0, None, 0,
                                             C.byref(w)), "bbmap_get_coverage")
        strands = 2 if w.flags & V.COV_STRANDED else 1
        hist = np.zeros((strands, w.hist_bins), np.int64)
        depth = np.zeros((strands, w.slots), np.int32 if w.depth_bytes == 4 else np.uint16)
        bins = np.zeros((strands, max(1, w.nbins)), np.int64)
        _lib.check(self.L.bbmap_get_coverage(self.h, int(binsize), recs.ctypes.data, nscaf, totals.ctypes.data, hist.ctypes.data, hist.shape[1],
                                             depth.ctypes.data, depth.shape[1] * depth.itemsize, bins.ctypes.data, bins.shape[1], C.byref(w)),
                   "bbmap_get_coverage")
        covoff, binoff = V.layout(recs["length"].astype(np.int32), binsize)
        return V.Coverage(w.flags, recs, totals[0], covoff, list(depth), list(hist), int(binsize), binoff,
                          [b[:w.nbins] for b in bins] if binsize > 0 else None, self.di.scaffold_names)

    def reset_coverage(self):
        _lib.check(self.L.bbmap_reset_coverage(self.h), "bbmap_reset_coverage")

    def pack_sites(self, counts, offsets, packed):
        """The last step's site lists without their empty slots (bbmap_pack_sites_device), enqueued on the current stream:
        counts int32[n+1], offsets int64[n+1], packed uint8[cap_records * MSITE_DTYPE.itemsize] -- device tensors of the caller's."""
        stream = torch.cuda.current_stream().cuda_stream
        assert counts.numel() == self.n + 1 and offsets.numel() == self.n + 1 and packed.numel() % MSITE_DTYPE.itemsize == 0
        _lib.check(self.L.bbmap_pack_sites_device(self.h, C.c_void_p(stream), self.n, counts.data_ptr(), offsets.data_ptr(),
                                                  packed.data_ptr(), packed.numel() // MSITE_DTYPE.itemsize), "bbmap_pack_sites_device")

    def output_pointers(self):
        """(bbmap_output of the last step) -- device pointers and counts, for callers that move the logs themselves."""
        o = bbmap_output()
        _lib.check(self.L.bbmap_get_output(self.h, C.byref(o)), "bbmap_get_output")
        return o

    def stats(self):
        st = bbmap_stats()
        _lib.check(self.L.bbmap_last_stats(self.h, C.byref(st)), "bbmap_last_stats")
        d = {n: getattr(st, n) for n, _ in bbmap_stats._fields_ if n not in ("probe_stats",)}
        d["probe_stats"] = list(st.probe_stats)
        return d

    def _fetch_output(self, o, n, with_match, rows=None):
        """Host copies of one bbmap_output over n reads (rows: only the site lists of reads [0, rows))."""
        cap = o.cap
        out = dict(cap=cap)
        ns = n if rows is None else min(rows, n)
        rec = lambda p, count, dt: _copy(p, count * dt.itemsize, self.dev).view(dt)
        out["sites"] = rec(o.sites, ns * cap, MSITE_DTYPE).reshape(ns, cap)
        out["nsites"] = _copy(o.nsites, n * 4, self.dev).view(np.int32)
        nj, ng = int(o.n_jobs), int(o.n_gapped_jobs)
        out["jobs"] = rec(o.jobs, nj, M.JOB_DTYPE)
        out["results"] = rec(o.results, nj, M.RESULT_DTYPE)
        out["jobinfo"] = rec(o.jobinfo, nj, JOBINFO_DTYPE)
        out["gjobs"] = rec(o.gjobs, ng, M.JOB_DTYPE)
        out["gresults"] = rec(o.gresults, ng, M.RESULT_DTYPE)
        out["gjobinfo"] = rec(o.gjobinfo, ng, JOBINFO_DTYPE)
        out["ggaps"] = rec(o.ggaps, ng, M.GAPS_DTYPE)
        out["match_stride"], out["gmatch_stride"] = o.match_stride, o.gmatch_stride
        if with_match:
            out["match"] = _copy(o.match, nj * o.match_stride, self.dev).reshape(nj, o.match_stride)
            out["gmatch"] = _copy(o.gmatch, ng * o.gmatch_stride, self.dev).reshape(ng, o.gmatch_stride)
        return out

    def fetch(self, with_match=True, rows=None):
        """Host copies of a step's results: sites (n x cap, MSITE_DTYPE), nsites, and the two fill logs; out["overflow"] holds
        the same for the reads the overflow tier mapped (nsites == NSITES_IN_TIER in the main list), plus their read_ids."""
        o = bbmap_output()
        _lib.check(self.L.bbmap_get_output(self.h, C.byref(o)), "bbmap_get_output")
        out = self._fetch_output(o, self.n, with_match, rows)
        ov = bbmap_overflow_output()
        _lib.check(self.L.bbmap_get_overflow_output(self.h, C.byref(ov)), "bbmap_get_overflow_output")
        if ov.n_reads > 0:
            t = self._fetch_output(ov.out, int(ov.n_reads), with_match)
            t["read_ids"] = _copy(ov.read_ids, int(ov.n_reads) * 4, self.dev).view(np.int32)
            out["overflow"] = t
        if self.cfg.finalStage and rows is None:
            out["final"], out["final_match"] = self.final(with_match)
        return out

    def enable_read_hist(self, flags=None):
        """bbmap_hist_enable: allocates the zeroed histogram state (flags: bbmap_amd.readstats.RH_*, default all groups)."""
        from . import readstats as R
        _lib.check(self.L.bbmap_hist_enable(self.h, int(R.RH_ALL if flags is None else flags)), "bbmap_hist_enable")

    def add_read_hist(self, quality=None):
        """bbmap_add_read_hist: adds the last step, overflow tier included.  quality: a device uint8 tensor laid out like the
        batch's bases (numeric phred); default: the one from_reads uploaded, as long as the batch is still the one it was uploaded
        with (load_reads / load_records forget it, a step over another bases buffer does not use it), else none: the
        quality-dependent histograms then do not move.  A second call for one step raises."""
        if quality is None and getattr(self, "_stepped_own_bases", True):
            quality = getattr(self, "quality", None)        # (cleared by load_reads / load_records; not used for step(bases=other))
        assert quality is None or (quality.dtype == torch.uint8 and quality.numel() >= self.total_bytes)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.L.bbmap_add_read_hist(self.h, C.c_void_p(stream), None if quality is None else C.c_void_p(quality.data_ptr())),
                   "bbmap_add_read_hist")

    def read_hist(self):
        """bbmap_get_read_hist: a host copy of everything added so far as a bbmap_amd.readstats.ReadHist."""
        from . import readstats as R
        w = R.bbmap_readhist_view()
        _lib.check(self.L.bbmap_get_read_hist(self.h, None, 0, C.byref(w)), "bbmap_get_read_hist")
        block = np.zeros(w.words, np.int64)
        _lib.check(self.L.bbmap_get_read_hist(self.h, block.ctypes.data, block.size, C.byref(w)), "bbmap_get_read_hist")
        return R.ReadHist(w.flags, block)

    def reset_read_hist(self):
        _lib.check(self.L.bbmap_reset_read_hist(self.h), "bbmap_reset_read_hist")

    def enable_split(self, tables, flags=None, ambiguous2=0, clearzone=0, max_sites=0):
        """bbmap_split_enable: reference-set binning over the index's scaffold table.  tables: bbmap_amd.refsplit.tables(...) of the
        reference's scaffold names; clearzone / max_sites 0 = the context's CLEARZONE1 and the profile's MAX_SITESCORES_TO_PRINT."""
        from . import refsplit as S
        cfg = S.config(S.SPLIT_ALL if flags is None else flags, ambiguous2, clearzone, max_sites, tables.nsets, tables.nkeys)
        sets, keys = np.ascontiguousarray(tables.scaf_sets, np.uint64), np.ascontiguousarray(tables.scaf_key, np.int32)
        _lib.check(self.L.bbmap_split_enable(self.h, C.byref(cfg), sets.ctypes.data, keys.ctypes.data), "bbmap_split_enable")
        self._split_tables = tables

    def add_split(self):
        """bbmap_add_split: adds the last step, overflow tier included.  A second call for one step raises."""
        _lib.check(self.L.bbmap_add_split(self.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "bbmap_add_split")

    def split_records(self):
        """Host copy of the last added step's per-read records (refsplit.SPLITREC_DTYPE)."""
        from . import refsplit as S
        p = C.c_void_p()
        _lib.check(self.L.bbmap_get_split_records(self.h, C.byref(p)), "bbmap_get_split_records")
        torch.cuda.current_stream().synchronize()
        return _copy(p.value, self.n * S.SPLITREC_DTYPE.itemsize, self.dev).view(S.SPLITREC_DTYPE)

    def split_lists(self):
        """bbmap_get_split_lists: (set_off int64[2 nsets + 1], units int32[total]) of the last added step, on the host; rows 0 .. nsets - 1
        are the sets' streams, the rest their ambiguous streams (refsplit.lists_of splits them)."""
        torch.cuda.current_stream().synchronize()
        set_off = np.zeros(2 * self._split_tables.nsets + 1, np.int64)
        total = C.c_int64()
        _lib.check(self.L.bbmap_get_split_lists(self.h, set_off.ctypes.data, None, 0, C.byref(total)), "bbmap_get_split_lists")
        units = np.zeros(total.value, np.int32)
        if total.value:
            _lib.check(self.L.bbmap_get_split_lists(self.h, set_off.ctypes.data, units.ctypes.data, units.size, C.byref(total)), "bbmap_get_split_lists")
        return set_off, units

    def split_stats(self):
        """bbmap_get_split_stats: everything added so far as a refsplit.SplitStats."""
        from . import refsplit as S
        t = self._split_tables
        words = np.zeros(S.STATE_HEAD + 4 * (t.nkeys + t.nsets), np.int64)
        _lib.check(self.L.bbmap_get_split_stats(self.h, words.ctypes.data, words.size), "bbmap_get_split_stats")
        return S.SplitStats.from_words(words, t.nkeys, t.nsets, t.key_names, t.set_names)

    def reset_split(self):
        _lib.check(self.L.bbmap_reset_split(self.h), "bbmap_reset_split")
