"""Reference-set binning (bbmap_split_* / bbpipe_refsplit_* in include/bbmap_amd.h): scafstats= / refstats= and the stream lists of
bbsplit.sh.  The device works on integers; names are turned into them here (`tables`) and back into BBSplitter.printCounts' text
(`scafstats_lines` / `refstats_lines`, current/align2/BBSplitter.java:1157-1189).  The raw form over device arrays of the caller's is
`DeviceSplit`; the context form is Mapper.enable_split / add_split / split_records / split_lists / split_stats / reset_split."""
import ctypes as C
import math

import numpy as np

from . import _lib as LL
from .coverage import jfmt
from .index import READ_DTYPE

SPLIT_SCAF_STATS, SPLIT_SET_STATS, SPLIT_RECORDS, SPLIT_LISTS, SPLIT_ALL = 1, 2, 4, 8, 15
AMBIG2_UNSET, AMBIG2_FIRST, AMBIG2_SPLIT, AMBIG2_TOSS, AMBIG2_RANDOM, AMBIG2_ALL = 0, 1, 2, 3, 4, 5       # BBSplitter.java:1203-1208
MAX_SETS = 64
LDS_SLOTS, MAX_PROBES, CHUNK_READS, MAX_BLOCKS, LIST_BLOCK = 1024, 8, 4096, 1024, 256
STATE_HEAD = 4
REC_AMBIG_SETS, REC_AMBIG_READ, REC_MAPPED = 1, 2, 4
SPLITREC_DTYPE = np.dtype([("primary_mask", "<u8"), ("ambig_mask", "<u8"), ("flags", "<i4"), ("key", "<i4"), ("stats_mask", "<u8")])
HEADER = "#name\t%unambiguousReads\tunambiguousMB\t%ambiguousReads\tambiguousMB\tunambiguousReads\tambiguousReads"      # :1170


class bbmap_split_config(C.Structure):
    _fields_ = [("flags", C.c_int32), ("ambiguous2", C.c_int32), ("clearzone", C.c_int32), ("maxSites", C.c_int32), ("nsets", C.c_int32),
                ("nkeys", C.c_int32), ("reserved", C.c_int32 * 2)]


def slot_of(key):
    """The LDS table's slot of a key (the top 10 bits of a multiplicative hash; bbmap_amd.h)."""
    return ((int(key) * 2654435761) & 0xffffffff) >> 22


class Tables:
    """set_names (first-seen order), key_names (first-seen order), scaf_sets uint64[nscaf], scaf_key int32[nscaf]"""

    def __init__(self, set_names, key_names, scaf_sets, scaf_key):
        self.set_names, self.key_names, self.scaf_sets, self.scaf_key = set_names, key_names, scaf_sets, scaf_key

    @property
    def nsets(self):
        return len(self.set_names)

    @property
    def nkeys(self):
        return len(self.key_names)


def tables(packed, prefixes=True):
    """Scaffold names -> Tables.  packed: a reference.Packed, or the list of scaffold names by global number.  With prefixes
    (Data.scaffoldPrefixes, set by BBSplit, BBSplitter.java:43) a name is `sets$name`: the sets are the part before the first `$`,
    split at commas (toListNames, :1033-1048), the key is the part behind it (getScaffolds, :882-887); a name without `$` has no set
    and is its own key.  Without prefixes every name is its own key and there are no sets.  More than 64 sets raise."""
    names = packed.scaffold_names() if hasattr(packed, "scaffold_names") else list(packed)
    set_ix, key_ix = {}, {}
    sets, keys = np.zeros(len(names), np.uint64), np.zeros(len(names), np.int32)
    for g, name in enumerate(names):
        name = "" if name is None else name
        x = name.find("$") if prefixes else -1
        mask = 0
        if x >= 0:
            parts = name[:x].split(",")
            while len(parts) > 1 and parts[-1] == "":           # String.split drops trailing empty strings
                parts.pop()
            for s in parts:
                mask |= 1 << set_ix.setdefault(s, len(set_ix))
        keys[g] = key_ix.setdefault(name[x + 1:] if x >= 0 else name, len(key_ix))
        if len(set_ix) > MAX_SETS:
            raise ValueError("more than %d reference sets" % MAX_SETS)
        sets[g] = mask
    return Tables(list(set_ix), list(key_ix), sets, keys)


class SplitStats:
    """Host copy of the counter state: total_reads, keys int64[nkeys][4], sets int64[nsets][4] (unambiguous reads, unambiguous bases,
    ambiguous reads, ambiguous bases).  Adds with `+` (the ranks of bbmap_amd.dist are summed on the host)."""

    def __init__(self, total_reads, keys, sets, key_names=None, set_names=None):
        self.total_reads = int(total_reads)
        self.keys, self.sets = np.asarray(keys, np.int64).reshape(-1, 4), np.asarray(sets, np.int64).reshape(-1, 4)
        self.key_names, self.set_names = key_names, set_names      # for the text; not part of the comparison

    @classmethod
    def from_words(cls, words, nkeys, nsets, key_names=None, set_names=None):
        w = np.asarray(words, np.int64)
        assert w.size >= STATE_HEAD + 4 * (nkeys + nsets)
        return cls(w[0], w[STATE_HEAD:STATE_HEAD + 4 * nkeys], w[STATE_HEAD + 4 * nkeys:STATE_HEAD + 4 * (nkeys + nsets)], key_names, set_names)

    def __add__(self, o):
        assert self.keys.shape == o.keys.shape and self.sets.shape == o.sets.shape
        return SplitStats(self.total_reads + o.total_reads, self.keys + o.keys, self.sets + o.sets, self.key_names or o.key_names,
                          self.set_names or o.set_names)

    def __eq__(self, o):
        return self.total_reads == o.total_reads and np.array_equal(self.keys, o.keys) and np.array_equal(self.sets, o.sets)


def _jdouble(x, places=5):
    """String.format("%.5f", x) for any double"""
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    return jfmt(x, places)


def count_lines(names, counts, total_reads, header=True, nzo=True, sort=True):
    """printCounts (:1157-1189): rows of (name, mappedReads, mappedBases, ambiguousReads, ambiguousBases) in map order, or sorted by
    SetCount.compareTo (:1139-1143: mappedReads, ambiguousReads, name) and reversed."""
    rows = [(n, int(c[0]), int(c[1]), int(c[2]), int(c[3])) for n, c in zip(names, counts)]
    if sort:
        rows.sort(key=lambda r: (r[1], r[3], r[0]), reverse=True)
    divR = 100.0 / total_reads if total_reads else math.inf
    divB = 1.0 / 1000000
    out = [HEADER] if header else []
    for name, mr, mb, ar, ab in rows:
        if nzo and mr <= 0 and ar <= 0:
            continue
        with np.errstate(invalid="ignore"):
            cols = [float(np.float64(mr) * np.float64(divR)), mb * divB, float(np.float64(ar) * np.float64(divR)), ab * divB]
        out.append("\t".join([name] + [_jdouble(v) for v in cols] + [str(mr), str(ar)]))
    return out


def scafstats_lines(stats, key_names=None, header=True, nzo=True, sort=True):
    """scafstats= from a SplitStats (key_names: default the ones the stats carry, as Mapper.split_stats gives them)"""
    return count_lines(stats.key_names if key_names is None else key_names, stats.keys, stats.total_reads, header, nzo, sort)


def refstats_lines(stats, set_names=None, header=True, nzo=True, sort=True):
    """refstats= from a SplitStats"""
    return count_lines(stats.set_names if set_names is None else set_names, stats.sets, stats.total_reads, header, nzo, sort)


def lists_of(set_off, units, nsets):
    """The CSR arrays as two lists of per-set arrays: (streams, ambiguous streams)."""
    rows = [np.asarray(units[int(set_off[i]):int(set_off[i + 1])]) for i in range(2 * nsets)]
    return rows[:nsets], rows[nsets:]


def config(flags=SPLIT_ALL, ambiguous2=AMBIG2_UNSET, clearzone=0, max_sites=0, nsets=0, nkeys=0):
    return bbmap_split_config(int(flags), int(ambiguous2), int(clearzone), int(max_sites), int(nsets), int(nkeys), (C.c_int32 * 2)(0, 0))


def state_words(nkeys, nsets):
    b = LL.load().bbpipe_refsplit_state_bytes(int(nkeys), int(nsets))
    if b < 0:
        LL.check(int(b), "bbpipe_refsplit_state_bytes")
    return int(b) // 8


class DeviceSplit:
    """The raw form (bbpipe_refsplit_*): a zeroed state on the device for one configuration and one set of scaffold tables.
    scaf_off int32[nchroms + 2], scaf_loc int32[nscaf] as bbidx_set_scaffolds lays them out; scaf_sets / scaf_key by global number."""

    def __init__(self, cfg, nchroms, scaf_off, scaf_loc, pad, scaf_sets, scaf_key, device="cuda"):
        import torch
        self.torch, self.dev, self.cfg, self.nchroms, self.pad = torch, device, cfg, int(nchroms), int(pad)
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t).view(np.uint8).reshape(-1).copy()).to(device)      # noqa: E731
        pad1 = lambda a, t: np.concatenate([np.asarray(a, t), np.zeros(1, t)])       # noqa: E731  (never an empty device array)
        self.scaf_off, self.scaf_loc = up(scaf_off, np.int32), up(pad1(scaf_loc, np.int32), np.int32)
        self.scaf_sets, self.scaf_key = up(pad1(scaf_sets, np.uint64), np.uint64), up(pad1(scaf_key, np.int32), np.int32)
        self.state = torch.zeros(state_words(cfg.nkeys, cfg.nsets), dtype=torch.int64, device=device)
        self.records = None
        self.n, self.paired = 0, False

    def reset(self):
        self.state.zero_()

    def add(self, reads, finals, sites, nsites, cap, paired):
        """reads / finals / sites: uint8 device tensors of READ_DTYPE / FINAL_DTYPE / MSITE_DTYPE records (sites n x cap), nsites int32"""
        L, torch = LL.load(), self.torch
        n = reads.numel() // READ_DTYPE.itemsize
        self.records = torch.zeros(max(n, 1) * SPLITREC_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self.n, self.paired = n, bool(paired)
        stream = torch.cuda.current_stream().cuda_stream
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())        # noqa: E731
        LL.check(L.bbpipe_refsplit_add_device(C.c_void_p(stream), n, int(paired), C.byref(self.cfg), ptr(reads), ptr(finals), ptr(sites),
                                              ptr(nsites), int(cap), self.nchroms, ptr(self.scaf_off), ptr(self.scaf_loc), self.pad,
                                              ptr(self.scaf_sets), ptr(self.scaf_key), ptr(self.state), ptr(self.records)),
                 "bbpipe_refsplit_add_device")

    def stats(self):
        return SplitStats.from_words(self.state.cpu().numpy(), self.cfg.nkeys, self.cfg.nsets)

    def host_records(self):
        return self.records.cpu().numpy().view(SPLITREC_DTYPE)[:self.n]

    def lists(self):
        """(set_off int64[2 nsets + 1], units int32[total]) of the last add, on the host"""
        L, torch = LL.load(), self.torch
        nsets = self.cfg.nsets
        need = L.bbpipe_refsplit_lists_workspace_bytes(self.n, int(self.paired), nsets)
        if need < 0:
            LL.check(int(need), "bbpipe_refsplit_lists_workspace_bytes")
        ws = torch.zeros(int(need) + 8, dtype=torch.uint8, device=self.dev)
        set_off = torch.zeros(2 * nsets + 1, dtype=torch.int64, device=self.dev)
        stream = torch.cuda.current_stream().cuda_stream
        units = None
        for _ in range(2):          # the sizing call, then the one that places
            cap = 0 if units is None else units.numel()
            LL.check(L.bbpipe_refsplit_lists_device(C.c_void_p(stream), self.n, int(self.paired), nsets, C.c_void_p(self.records.data_ptr()),
                                                    C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(set_off.data_ptr()),
                                                    None if units is None else C.c_void_p(units.data_ptr()), cap),
                     "bbpipe_refsplit_lists_device")
            total = int(set_off[-1].item())
            if units is not None or total == 0:
                break
            units = torch.zeros(total, dtype=torch.int32, device=self.dev)
        return set_off.cpu().numpy(), (units.cpu().numpy() if units is not None else np.zeros(0, np.int32))
