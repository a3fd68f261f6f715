"""Reference-set binning on the device (bbmap_split_* / bbpipe_refsplit_*) against the sequential restatement of BBSplitter.printReads
(tests/refsplit_check.py, which works on sets of name strings): counters, per-read records and stream lists are equal exactly (all
state is 64-bit integers and the lists are a stable partition, so nothing depends on the order of the work).  Raw form over planted
records first, then contention and table shapes, the lists, then the context form over the PhiX fixture's reads."""
import ctypes as C

import numpy as np
import pytest
import torch

from bbmap_amd import _lib
from bbmap_amd import reference as REFM
from bbmap_amd import refsplit as S
from bbmap_amd.index import DeviceIndex, READ_DTYPE
from bbmap_amd.mapper import FINAL_DTYPE, MSITE_DTYPE, Mapper
from tests import refsplit_check as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = [K.UNSET, K.SPLIT, K.ALL, K.TOSS]
CLEARZONE, PAD = 200, 300


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


class World:
    """A scaffold table with its names: per-chromosome locs / lengths / names, the restatement's Reference and the device's tables"""

    def __init__(self, locs, lengths, names, prefixes=True):
        self.locs, self.lengths, self.names, self.prefixes = locs, lengths, names, prefixes
        self.ref = K.Reference(locs, names, PAD)
        self.tab = S.tables([n for ns in names for n in ns], prefixes)
        self.off = np.cumsum([0, 0] + [len(a) for a in locs]).astype(np.int32)
        self.loc = np.concatenate([np.asarray(a, np.int32) for a in locs])
        self.nchroms = len(locs)
        self.flat = [(c + 1, i) for c in range(self.nchroms) for i in range(len(locs[c]))]

    def device(self, flags=S.SPLIT_ALL, mode=K.UNSET, max_sites=5, clearzone=CLEARZONE):
        cfg = S.config(flags, mode, clearzone, max_sites, self.tab.nsets, self.tab.nkeys)
        return S.DeviceSplit(cfg, self.nchroms, self.off, self.loc, PAD, self.tab.scaf_sets, self.tab.scaf_key, DEV)

    def splitter(self, mode=K.UNSET, max_sites=5, clearzone=CLEARZONE):
        return K.Splitter(self.ref, self.tab.key_names, self.tab.set_names, self.prefixes, mode, clearzone, max_sites)


def _world(rng, per_chrom=(15, 24, 1), nsets=5, shared_every=6, twin_every=7):
    """3 chromosomes / 40 scaffolds / 5 sets: every `shared_every`-th scaffold is shared by two sets under a comma prefix, every
    `twin_every`-th repeats an earlier scaffold's tail under another set (two scaffolds, one key)"""
    locs, lengths, names, g = [], [], [], 0
    for n in per_chrom:
        lo, le, na, at = [], [], [], 8000
        for _ in range(n):
            ln = int(rng.integers(400, 2500))
            lo.append(at); le.append(ln)
            s = "S%d" % (g % nsets)
            if g % shared_every == shared_every - 1:
                s += ",S%d" % ((g + 2) % nsets)
            tail = "k%d" % (g - 3) if g % twin_every == twin_every - 1 else "k%d" % g
            na.append(s + "$" + tail)
            at += ln + PAD
            g += 1
        locs.append(lo); lengths.append(le); names.append(na)
    return World(locs, lengths, names)


def _site(rng, w, g=None):
    """(chrom, start, stop, -) of a site on global scaffold g: mostly inside it, sometimes hanging into the padding on either side"""
    chrom, i = w.flat[int(rng.integers(0, len(w.flat))) if g is None else g]
    a, ln = w.locs[chrom - 1][i], w.lengths[chrom - 1][i]
    n = int(rng.integers(50, 151))
    start = a + int(rng.integers(-PAD, ln + PAD - n)) if rng.random() < 0.25 else a + int(rng.integers(0, max(1, ln - n)))
    return chrom, start, start + n - 1


DROPS = [0, 0, 0, 1, 50, 199, 200, 201, 201, 400]


def _planted(rng, w, n, cap, ngroup=3):
    """n reads as the restatement's dicts plus the flag the device sees in nsites (None = the count).  Sites of one read come from a
    small group of scaffolds so that equal and different sets both occur; scores step down by DROPS (the clearzone's edge is 200)."""
    nscaf = len(w.loc)
    reads, flags = [], []
    for r in range(n):
        u = rng.random()
        length = int(rng.integers(50, 151))
        if u < 0.12:
            reads.append(dict(mapped=False, ambiguous=False, chrom=-1, start=-1, stop=-1, mapScore=0, length=length, sites=[]))
            flags.append(None if rng.random() < 0.7 else int(rng.choice([-1, -2, -3])))
            continue
        group = rng.integers(0, nscaf, ngroup)
        ns = int(rng.integers(1, cap + 1)) if u > 0.17 else 0
        score, sites = int(rng.choice([900, 1000, 1000, 1100])), []
        for j in range(ns):
            if j:
                score -= int(rng.choice(DROPS))
            g = int(group[0] if rng.random() < 0.5 else group[int(rng.integers(0, ngroup))])
            sites.append(_site(rng, w, g) + (score,))
        own = sites[0][:3] if sites and rng.random() < 0.9 else _site(rng, w)
        flag = None
        if sites and rng.random() < 0.03:
            flag = int(rng.choice([-1, -2]))                # a record that says mapped under an overflow flag: not mapped
        reads.append(dict(mapped=True, ambiguous=bool(rng.random() < 0.35), chrom=own[0], start=own[1], stop=own[2],
                          mapScore=int(rng.choice([500, 500, 600, 700])), length=length, sites=sites))
        flags.append(flag)
    return reads, flags


def _upload(reads, flags, cap):
    n = len(reads)
    fin, rd = np.zeros(n, FINAL_DTYPE), np.zeros(n, READ_DTYPE)
    sites, ns = np.zeros((max(n, 1), cap), MSITE_DTYPE), np.zeros(max(n, 1), np.int32)
    for r, x in enumerate(reads):
        f = fin[r]
        f["mapped"], f["ambiguous"], f["chrom"], f["start"], f["stop"], f["mapScore"] = x["mapped"], x["ambiguous"], x["chrom"], x["start"], x["stop"], x["mapScore"]
        rd[r]["len"] = x["length"]
        assert len(x["sites"]) <= cap
        for j, (c, a, b, sc) in enumerate(x["sites"]):
            s = sites[r, j]
            s["chrom"], s["start"], s["stop"], s["score"] = c, a, b, sc
        ns[r] = len(x["sites"]) if flags[r] is None else flags[r]
    return _dev(rd), _dev(fin), _dev(sites), _dev(ns)


def _seen(reads, flags):
    """the reads as the stage sees them: an overflow flag unmaps a read"""
    return [dict(x, mapped=False) if f in (-1, -2) else x for x, f in zip(reads, flags)]


def _mask(names, tab):
    return sum(1 << tab.set_names.index(s) for s in (names or ()))


def _want_records(w, reads, verdicts, paired):
    out = np.zeros(len(reads), S.SPLITREC_DTYPE)
    step = 2 if paired else 1
    for r, x in enumerate(reads):
        primary, ambig, amb, stat = verdicts[r // step]
        o = out[r]
        o["primary_mask"], o["ambig_mask"], o["stats_mask"] = _mask(primary, w.tab), _mask(ambig, w.tab), _mask(stat, w.tab)
        o["flags"] = (S.REC_AMBIG_SETS if amb else 0) | (S.REC_AMBIG_READ if x["mapped"] and x["ambiguous"] else 0) | (S.REC_MAPPED if x["mapped"] else 0)
        o["key"] = w.tab.key_names.index(K.key_of(w.ref.scaffold_name(x["chrom"], x["start"], x["stop"]), w.prefixes)) if x["mapped"] else -1
    return out


def _want_stats(w, k):
    keys = np.array([k.scaf[n] for n in w.tab.key_names], np.int64).reshape(-1, 4)
    sets = np.array([k.sets[n] for n in w.tab.set_names], np.int64).reshape(-1, 4)
    return S.SplitStats(k.total_reads, keys, sets)


def _want_lists(w, table, tableA):
    rows = [table.get(s, []) for s in w.tab.set_names] + [tableA.get(s, []) for s in w.tab.set_names]
    off = np.cumsum([0] + [len(x) for x in rows]).astype(np.int64)
    return off, np.array([u for x in rows for u in x], np.int32)


def _check_lists(got, want, nsets):
    (goff, gun), (woff, wun) = got, want
    assert np.array_equal(goff, woff), (goff, woff)
    assert np.array_equal(gun, wun)
    for i in range(2 * nsets):
        row = gun[goff[i]:goff[i + 1]]
        assert np.all(np.diff(row) > 0)                     # strictly ascending


_CACHE = {}


def _set():
    """(world, reads, flags, seen, cap) of the planted set: built once and left unchanged"""
    if "w" not in _CACHE:
        rng = np.random.default_rng(5)
        w = _world(rng)
        assert w.nchroms == 3 and len(w.loc) == 40 and w.tab.nsets == 5 and w.tab.nkeys < 40
        reads, flags = _planted(rng, w, 3000, 8)
        _CACHE["w"] = (w, reads, flags, _seen(reads, flags), 8)
    return _CACHE["w"]


def _restated(paired, mode):
    key = ("r", paired, mode)
    if key not in _CACHE:
        w, _, _, seen, _ = _set()
        k = w.splitter(mode)
        _CACHE[key] = (k,) + k.print_reads(seen, paired)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ the raw form, planted records
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("paired", [False, True])
def test_planted_records(paired, mode):
    w, reads, flags, seen, cap = _set()
    k, verdicts, table, tableA = _restated(paired, mode)
    d = w.device(mode=mode)
    d.add(*_upload(reads, flags, cap), cap, paired)
    assert d.stats() == _want_stats(w, k), (d.stats().keys - _want_stats(w, k).keys, d.stats().sets - _want_stats(w, k).sets)
    got, want = d.host_records(), _want_records(w, seen, verdicts, paired)
    for f in S.SPLITREC_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (f, np.argwhere(got[f] != want[f])[:8].ravel())
    _check_lists(d.lists(), _want_lists(w, table, tableA), w.tab.nsets)
    assert d.stats().total_reads == len(reads)
    # the text from the device's state is the restatement's
    assert S.scafstats_lines(d.stats(), w.tab.key_names) == K.print_counts(k.scaf, k.total_reads)
    assert S.refstats_lines(d.stats(), w.tab.set_names, nzo=False, sort=False) == K.print_counts(k.sets, k.total_reads, nzo=False, sort=False)


def test_planted_set_takes_every_branch():
    """from the restatement's own tallies: every rule of the issue's list occurs in the planted set"""
    _, reads, flags, seen, _ = _set()
    single, pair = _restated(False, K.UNSET)[0].tally, _restated(True, K.UNSET)[0].tally
    for name in ("s1_not_in_p1", "clearzone_break", "clearzone_edge_kept", "cap_hides_site", "shared_unambiguous", "ambiguous", "unambiguous"):
        assert single[name] > 0, name
    for name in ("p1_ne_p2", "s1_not_in_p1", "s2_not_in_p2", "single_mapped_mate", "mapscore_r1", "mapscore_r2", "mapscore_tie", "ambiguous",
                 "unambiguous"):
        assert pair[name] > 0, name
    assert any(x["mapped"] and x["ambiguous"] and not x["sites"] for x in seen)        # mapped, ambiguous, empty list: no key, no fault
    assert any(f in (-1, -2) and x["mapped"] for x, f in zip(reads, flags)) and any(f == -3 for f in flags)
    k = _restated(True, K.SPLIT)
    assert k[3] and k[2]                                     # SPLIT fills both tables


@pytest.mark.parametrize("flag", [S.SPLIT_SCAF_STATS, S.SPLIT_SET_STATS, S.SPLIT_RECORDS, S.SPLIT_LISTS])
def test_every_flag_alone(flag):
    w, reads, flags, seen, cap = _set()
    k, verdicts, table, tableA = _restated(True, K.SPLIT)
    want = _want_stats(w, k)
    d = w.device(flags=flag, mode=K.SPLIT)
    d.add(*_upload(reads, flags, cap), cap, True)
    got = d.stats()
    assert np.array_equal(got.keys, want.keys if flag == S.SPLIT_SCAF_STATS else 0 * want.keys)
    assert np.array_equal(got.sets, want.sets if flag == S.SPLIT_SET_STATS else 0 * want.sets)
    if flag in (S.SPLIT_RECORDS, S.SPLIT_LISTS):
        assert d.host_records().tobytes() == _want_records(w, seen, verdicts, True).tobytes()
        _check_lists(d.lists(), _want_lists(w, table, tableA), w.tab.nsets)
    else:
        assert not d.host_records().view(np.uint8).any()


def test_site_cap_and_clearzone_are_parameters():
    w, reads, flags, seen, cap = _set()
    for max_sites, cz in ((1, 200), (8, 200), (5, 0), (5, 1000)):
        k = w.splitter(K.ALL, max_sites, cz)
        verdicts, _, _ = k.print_reads(seen, False)
        d = w.device(mode=K.ALL, max_sites=max_sites, clearzone=cz)
        d.add(*_upload(reads, flags, cap), cap, False)
        assert d.stats() == _want_stats(w, k)
        assert d.host_records().tobytes() == _want_records(w, seen, verdicts, False).tobytes()


def test_names_without_prefixes_have_keys_and_no_sets():
    w0, reads, flags, seen, cap = _set()
    # (plain bbmap.sh names: toListNames would find sets behind a `$` whatever Data.scaffoldPrefixes says)
    w = World(w0.locs, w0.lengths, [[n.replace("$", "_") for n in ns] for ns in w0.names], prefixes=False)
    assert w.tab.nsets == 0 and w.tab.nkeys == 40
    k = w.splitter()
    verdicts, table, tableA = k.print_reads(seen, True)
    d = w.device()
    d.add(*_upload(reads, flags, cap), cap, True)
    assert d.stats() == _want_stats(w, k) and d.stats().keys.any()
    assert d.host_records().tobytes() == _want_records(w, seen, verdicts, True).tobytes()
    off, units = d.lists()
    assert off.tolist() == [0] and units.size == 0


# ------------------------------------------------------------------------------------------------ contention and table shapes
def _uniform(w, gs, length=100, ambiguous=False):
    """reads with one site each on the global scaffolds gs (an int array; -1 = unmapped), uploaded without Python loops"""
    gs = np.asarray(gs)
    n = len(gs)
    ok = gs >= 0
    chrom_of = np.repeat(np.arange(1, w.nchroms + 1), [len(a) for a in w.locs])
    g = np.where(ok, gs, 0)
    fin, rd = np.zeros(n, FINAL_DTYPE), np.zeros(n, READ_DTYPE)
    sites = np.zeros((n, 1), MSITE_DTYPE)
    fin["mapped"], fin["ambiguous"], fin["mapScore"] = ok, ambiguous, 500
    for rec in (fin, sites[:, 0]):
        rec["chrom"], rec["start"], rec["stop"] = chrom_of[g], w.loc[g] + 10, w.loc[g] + 10 + length - 1
    sites["score"] = 1000
    rd["len"] = length
    return _dev(rd), _dev(fin), _dev(sites), _dev(ok.astype(np.int32))


def test_one_key_and_one_set_under_contention():
    """200,000 identical records: 49 chunks on 49 workgroups, every lane of every wavefront on the same slot and the same set"""
    n = 200000
    w = World([[8000, 9000]], [[500, 500]], [["S0$a", "S1$b"]])
    for paired in (False, True):
        d = w.device()
        d.add(*_uniform(w, np.ones(n, np.int64)), 1, paired)
        st = d.stats()
        assert st.total_reads == n and st.keys.tolist() == [[0, 0, 0, 0], [n, 100 * n, 0, 0]] and st.sets.tolist() == [[0, 0, 0, 0], [n, 100 * n, 0, 0]]
        off, units = d.lists()
        step = 2 if paired else 1
        assert off.tolist() == [0, 0, n // step, n // step, n // step] and np.array_equal(units, np.arange(0, n, step))


def test_two_keys_that_collide_in_the_table():
    """the same count alternating between two keys of one slot: the second one lives in the next slot (linear probing)"""
    k1 = 3
    k2 = next(k for k in range(k1 + 1, 100000) if S.slot_of(k) == S.slot_of(k1))
    n = 200000
    names = ["S0$k%d" % i for i in range(k2 + 1)]
    w = World([[8000 + 400 * i for i in range(k2 + 1)]], [[100] * (k2 + 1)], [names])
    assert w.tab.scaf_key[k2] == k2
    d = w.device(flags=S.SPLIT_SCAF_STATS)
    d.add(*_uniform(w, np.where(np.arange(n) & 1, k2, k1), length=70, ambiguous=True), 1, False)
    st = d.stats()
    assert st.keys[k1].tolist() == [0, 0, n // 2, 35 * n] and st.keys[k2].tolist() == [0, 0, n // 2, 35 * n] and int(st.keys.sum()) == n + 70 * n


def _many_keys(nk):
    return World([[8000 + 400 * i for i in range(nk)]], [[100] * nk], [["S%d$k%d" % (i % 7, i) for i in range(nk)]])


def test_a_key_table_larger_than_the_lds_table():
    """100,000 keys, 150,000 reads: every key once, every fourth key a second time, the rest unmapped.  A chunk of 4096 reads holds
    4096 distinct keys, four times the table's slots: most adds go to the state directly."""
    nk = 100000
    w = _many_keys(nk)
    gs = np.concatenate([np.arange(nk), np.arange(0, nk, 4), np.full(25000, -1)])
    assert len(gs) == 150000
    d = w.device(flags=S.SPLIT_SCAF_STATS | S.SPLIT_SET_STATS)
    d.add(*_uniform(w, gs, length=90), 1, False)
    st = d.stats()
    hits = np.bincount(gs[gs >= 0], minlength=nk)
    assert hits.max() == 2 and int(hits.sum()) == 125000
    assert np.array_equal(st.keys[:, 0], hits) and np.array_equal(st.keys[:, 1], 90 * hits) and not st.keys[:, 2:].any()
    per_set = np.bincount(np.arange(nk) % 7, weights=hits, minlength=7).astype(np.int64)
    assert np.array_equal(st.sets[:, 0], per_set) and np.array_equal(st.sets[:, 1], 90 * per_set) and st.total_reads == 150000


def test_the_lds_table_overflows_inside_one_chunk():
    """one workgroup, one chunk (4000 reads), 3000 distinct keys on 1024 slots, ambiguous reads with several keys each: restatement"""
    rng = np.random.default_rng(9)
    w = _many_keys(3000)
    reads, flags = _planted(rng, w, 4000, 6, ngroup=6)
    assert len({s[:3] for x in reads for s in x["sites"]}) > S.LDS_SLOTS
    seen = _seen(reads, flags)
    k = w.splitter(K.UNSET, 6)
    k.print_reads(seen, False)
    assert sum(1 for c in k.scaf.values() if any(c)) > S.LDS_SLOTS
    d = w.device(max_sites=6)
    d.add(*_upload(reads, flags, 6), 6, False)
    assert d.stats() == _want_stats(w, k)


# ------------------------------------------------------------------------------------------------ the lists
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("units", [1, 63, 64, 65, 1000])
def test_lists_are_a_stable_partition(units, paired):
    """64 sets of which only 0, 5, 62 and 63 own scaffolds (shared ones included): rows of sets nothing goes to stay empty, set 63
    is the mask's top bit; 1000 units span four workgroups of the list passes"""
    names = ["S%d$x%d" % (i, i) for i in range(64)]
    order = [0, 5, 62, 63]
    own = ["S0$a", "S5$b", "S62$c", "S63$d", "S63,S0$e", "S5,S62,S63$f"]
    # sets are numbered in first-seen order: name all 64 first, on scaffolds no read ever touches
    all_names = names + own
    nscaf = len(all_names)
    w = World([[8000 + 400 * i for i in range(nscaf)]], [[100] * nscaf], [all_names])
    assert w.tab.nsets == 64 and w.tab.set_names[63] == "S63"
    rng = np.random.default_rng(units)
    n = units * (2 if paired else 1)
    reads, flags = [], []
    for r in range(n):
        sites, score = [], 1000
        for j in range(int(rng.integers(0, 4))):
            score -= int(rng.choice([0, 100, 300]))
            sites.append(_site(rng, w, 64 + int(rng.integers(0, len(own)))) + (score,))
        own_rec = sites[0][:3] if sites else (-1, -1, -1)
        reads.append(dict(mapped=bool(sites), ambiguous=False, chrom=own_rec[0], start=own_rec[1], stop=own_rec[2],
                          mapScore=int(rng.choice([500, 600])), length=100, sites=sites))
        flags.append(None)
    for mode in (K.SPLIT, K.ALL):
        k = w.splitter(mode)
        _, table, tableA = k.print_reads(reads, paired)
        d = w.device(flags=S.SPLIT_LISTS, mode=mode)
        d.add(*_upload(reads, flags, 4), 4, paired)
        off, un = d.lists()
        _check_lists((off, un), _want_lists(w, table, tableA), 64)
        used = {i for i in range(128) if off[i + 1] > off[i]}
        assert used <= set(order) | {64 + i for i in order}
        if units >= 63:
            assert 63 in used and 0 in used and (mode != K.SPLIT or 64 + 63 in used)


# ------------------------------------------------------------------------------------------------ state over batches, refusals
def test_two_batches_add_up_and_reset_zeroes():
    w, reads, flags, seen, cap = _set()
    k = w.splitter(K.ALL)
    k.print_reads(seen[:1000], True)
    k.print_reads(seen[1000:], True)
    d = w.device(mode=K.ALL)
    d.add(*_upload(reads[:1000], flags[:1000], cap), cap, True)
    d.add(*_upload(reads[1000:], flags[1000:], cap), cap, True)
    assert d.stats() == _want_stats(w, k)
    d.reset()
    d.add(*_upload(reads[:10], flags[:10], cap), cap, True)
    assert d.stats().total_reads == 10


def test_raw_refusals_and_a_call_on_nothing():
    L = _lib.load()
    err = lambda: L.bbmap_last_error()         # noqa: E731
    args = lambda cfg, off=None: (None, 2, 0, C.byref(cfg), None, None, None, None, 0, 1, off, None, PAD, None, None, None, None)        # noqa: E731
    assert L.bbpipe_refsplit_add_device(*args(S.config(nsets=65))) == -2 and err() == b"bbpipe_refsplit_add_device: at most 64 reference sets are supported"
    assert L.bbpipe_refsplit_add_device(*args(S.config(ambiguous2=S.AMBIG2_RANDOM, max_sites=5))) == -2
    assert err() == b"bbpipe_refsplit_add_device: AMBIGUOUS2_RANDOM is not implemented (the reference throws)"
    assert L.bbpipe_refsplit_add_device(*args(S.config(max_sites=5, nsets=2))) == -2 and err() == b"bbpipe_refsplit_add_device: no scaffold table"
    assert L.bbpipe_refsplit_add_device(*args(S.config(flags=16, max_sites=5))) == -2 and err() == b"bbpipe_refsplit_add_device: unknown flag bits"
    assert L.bbpipe_refsplit_add_device(*args(S.config(max_sites=0))) == -2
    assert L.bbpipe_refsplit_state_bytes(3, 65) == -2 and L.bbpipe_refsplit_state_bytes(3, 2) == 8 * (4 + 12 + 8)
    zero = (None, 0, 0, C.byref(S.config(max_sites=5, nsets=2)), None, None, None, None, 0, 1, None, None, PAD, None, None, None, None)
    assert L.bbpipe_refsplit_add_device(*zero) == 0
    w, _, _, _, cap = _set()
    d = w.device()
    d.add(*_upload([], [], cap), cap, False)
    assert d.stats() == S.SplitStats(0, np.zeros((w.tab.nkeys, 4)), np.zeros((5, 4)))
    off, units = d.lists()
    assert not off.any() and off.size == 11 and units.size == 0


# ------------------------------------------------------------------------------------------------ through the mapper
CLEAN = (2500, 3300)       # the stretch of the second genome that is left identical to the first


def _two_genomes():
    """PhiX cut in two: bases [0, 4000) are genome G1, a copy of them with a substitution every 40 bases (none inside CLEAN) is
    genome G2, and the rest is a record both genomes share under a comma prefix"""
    from tests.golden_phix import START_PAD, phix_reference
    ref = phix_reference()
    body = ref[START_PAD:len(ref) - START_PAD]
    g1 = body[:4000].copy()
    g2 = g1.copy()
    sub = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A"), ord("N"): ord("N")}
    for i in range(17, 4000, 40):
        if not CLEAN[0] <= i < CLEAN[1]:
            g2[i] = sub[int(g2[i])]
    return REFM.pack([("G1$phix_a", g1), ("G2$phix_b", g2), ("G1,G2$phix_tail", body[4000:].copy())])


def _mapper(mode, **kw):
    from tests.golden_phix import fixture_inputs
    reads, quals, paired = fixture_inputs(mode, True)
    p = _two_genomes()
    di = DeviceIndex.build(p.chroms, k=13)
    di.set_scaffolds(p)
    mp = Mapper.from_reads(di, [len(r) for r in reads], np.concatenate(reads), np.concatenate(quals), paired=paired, **kw)
    return p, di, mp, reads, paired


def _restate_mapper(p, mp, reads, paired, k):
    """feeds the final records and site lists fetched from the device (the overflow tier's in place of the reads it mapped) to the
    restatement"""
    from tests.test_runstats_gpu import _restate
    fin, _, lists, lens = _restate(mp, reads, paired, None)
    ns = mp.fetch(with_match=False)["nsites"]
    seen = []
    for r in range(len(fin)):
        f = fin[r]
        sites = [(int(s["chrom"]), int(s["start"]), int(s["stop"]), int(s["score"])) for s in lists[r]]
        seen.append(dict(mapped=bool(f["mapped"]) and int(ns[r]) not in (-1, -2), ambiguous=bool(f["ambiguous"]), chrom=int(f["chrom"]),
                         start=int(f["start"]), stop=int(f["stop"]), mapScore=int(f["mapScore"]), length=lens[r], sites=sites))
    return seen, k.print_reads(seen, paired)


@pytest.mark.parametrize("mode", ["pe", "se1"])
def test_phix_reads_against_two_genomes(mode):
    p, di, mp, reads, paired = _mapper(mode, max_sites=32)
    try:
        tab = S.tables(p)
        assert tab.set_names == ["G1", "G2"] and tab.key_names == ["phix_a", "phix_b", "phix_tail"] and tab.scaf_sets.tolist() == [1, 2, 3]
        w = World(p.locs, p.lengths, p.names)
        mp.enable_split(tab, ambiguous2=S.AMBIG2_SPLIT)
        assert mp.L.bbmap_add_split(mp.h, None) == -2 and mp.L.bbmap_last_error() == b"bbmap_add_split: no batch has been mapped yet"
        mp.step()
        mp.add_split()
        assert mp.L.bbmap_add_split(mp.h, None) == -2 and mp.L.bbmap_last_error() == b"bbmap_add_split: the last batch has been added already"
        k = K.Splitter(w.ref, tab.key_names, tab.set_names, True, K.SPLIT, 200, 5)
        seen, (verdicts, table, tableA) = _restate_mapper(p, mp, reads, paired, k)
        got, want = mp.split_records(), _want_records(w, seen, verdicts, paired)
        for f in S.SPLITREC_DTYPE.names:
            assert np.array_equal(got[f], want[f]), (f, np.argwhere(got[f] != want[f])[:8].ravel())
        st = mp.split_stats()
        assert st == _want_stats(w, k) and st.total_reads == len(reads)
        _check_lists(mp.split_lists(), _want_lists(w, table, tableA), 2)
        # reads from the stretch the two genomes share letter for letter are ambiguous between them, the others are not
        assert k.tally["ambiguous"] > 0 and k.tally["unambiguous"] > 0 and k.tally["shared_unambiguous"] > 0
        assert int(np.count_nonzero(got["flags"] & S.REC_MAPPED)) > 0.9 * len(reads)
        # the text from the device's state is the restatement's
        assert S.scafstats_lines(st, tab.key_names) == K.print_counts(k.scaf, k.total_reads)
        assert S.refstats_lines(st) == K.print_counts(k.sets, k.total_reads)
        assert S.refstats_lines(st, tab.set_names, nzo=False, sort=False) == K.print_counts(k.sets, k.total_reads, nzo=False, sort=False)
        # a second step adds to the first; a reset zeroes; the batch the context holds may then be added again
        mp.step()
        mp.add_split()
        assert mp.split_stats() == st + st
        mp.reset_split()
        assert mp.split_stats() == S.SplitStats(0, 0 * st.keys, 0 * st.sets)
        mp.add_split()
        assert mp.split_stats() == st
        mp.enable_split(tab, ambiguous2=S.AMBIG2_SPLIT)       # the same configuration again: nothing changes
        assert mp.split_stats() == st
    finally:
        mp.close()
        di.close()


def test_phix_overflow_tier_lists_are_used():
    """max_sites = 1: most pairs are mapped by the overflow tier, whose records and lists the stage takes"""
    p, di, mp, reads, paired = _mapper("pe", max_sites=1, reserved=(C.c_int32 * 4)(0, 4096, 256, 0))
    try:
        tab = S.tables(p)
        w = World(p.locs, p.lengths, p.names)
        mp.enable_split(tab, ambiguous2=S.AMBIG2_ALL)
        mp.step()
        assert mp.stats()["reads_reprobed"] > 0
        mp.add_split()
        k = K.Splitter(w.ref, tab.key_names, tab.set_names, True, K.ALL, 200, 5)
        seen, (verdicts, table, tableA) = _restate_mapper(p, mp, reads, paired, k)
        assert mp.split_records().tobytes() == _want_records(w, seen, verdicts, paired).tobytes()
        assert mp.split_stats() == _want_stats(w, k)
        _check_lists(mp.split_lists(), _want_lists(w, table, tableA), 2)
        assert k.tally["ambiguous"] > 0 and k.tally["unambiguous"] > 0
    finally:
        mp.close()
        di.close()


def test_context_refusals():
    from tests.golden_phix import fixture_inputs
    reads, quals, paired = fixture_inputs("se1", True)
    p = _two_genomes()
    tab = S.tables(p)
    sets, keys = np.ascontiguousarray(tab.scaf_sets), np.ascontiguousarray(tab.scaf_key)
    di = DeviceIndex.build(p.chroms, k=13)
    try:
        def enable(mp, **kw):
            cfg = S.config(**dict(dict(nsets=tab.nsets, nkeys=tab.nkeys), **kw))
            return mp.L.bbmap_split_enable(mp.h, C.byref(cfg), sets.ctypes.data, keys.ctypes.data), mp.L.bbmap_last_error()
        mp = Mapper.from_reads(di, [len(r) for r in reads], np.concatenate(reads), np.concatenate(quals), paired=paired, max_sites=32)
        try:
            assert enable(mp) == (-2, b"bbmap_split_enable: the index has no scaffold table (bbidx_set_scaffolds)")
            di.set_scaffolds(p)
            assert enable(mp, nsets=65) == (-2, b"bbmap_split_enable: at most 64 reference sets are supported")
            assert enable(mp, ambiguous2=S.AMBIG2_RANDOM) == (-2, b"bbmap_split_enable: AMBIGUOUS2_RANDOM is not implemented (the reference throws)")
            assert mp.L.bbmap_add_split(mp.h, None) == -2 and mp.L.bbmap_last_error() == b"bbmap_add_split: the stage is not enabled (bbmap_split_enable)"
            assert mp.L.bbmap_reset_split(mp.h) == 0        # nothing to reset
            assert enable(mp, flags=S.SPLIT_SCAF_STATS)[0] == 0
            assert enable(mp, flags=S.SPLIT_ALL) == (-2, b"bbmap_split_enable: the stage is enabled already with another configuration")
            mp.step()
            mp._split_tables = tab
            mp.add_split()
            assert mp.split_stats().keys.any() and not mp.split_stats().sets.any()
            assert mp.L.bbmap_get_split_records(mp.h, C.byref(C.c_void_p())) == -2
            assert mp.L.bbmap_last_error() == b"bbmap_get_split_records: the stage keeps no records (BBMAP_SPLIT_RECORDS)"
        finally:
            mp.close()
        mp = Mapper.from_reads(di, [len(r) for r in reads], np.concatenate(reads), np.concatenate(quals), paired=paired, max_sites=32, finalStage=0)
        try:
            assert enable(mp) == (-2, b"bbmap_split_enable: the context runs without the final stage (bbmap_config.finalStage)")
        finally:
            mp.close()
    finally:
        di.close()
