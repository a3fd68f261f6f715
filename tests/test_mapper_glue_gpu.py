"""GPU tests of the mapper's per-read kernels (begin / score / scoreSlow round / final begin / final round) around the three things
that change how they run but not what they compute: the first rounds' class order (BBMAP_CLASS_ORDER), Dev read in the
kernel-argument segment (BBMAP_KERNARG_DEV) and the byte loops' chunked loads (BBMAP_CHUNK_LOADS).  Every batch is mapped with all
three on and with all three off; each run is compared with the CPU oracle record by record (tests/mapper_check.py: site lists, every
fill's window / minScore / scores / traceback string, final records and match strings), and the two runs with each other field by
field, log and pool positions apart.

The oracle call is oracle.map_reads, the general form oracle.map_batch wraps (map_batch takes one length and one key set per batch;
the length-10 batch is shorter than k and has no keys).  The class-list batches, all of one length, go through map_batch itself.

Sites that really leave the chromosome array (start < 0, stop >= reflen) cannot come out of the probe -- removeOutOfBounds drops
them, in the reference as here -- so they are planted: the final stage runs alone over one-site lists that hang over either end of
a reference without N pads, at every edge length, and the oracle's lists are asserted to still hold such sites; a whole-flow batch
on the same reference has reads with an insertion next to either end, whose fill windows reach past the array.

"A read on the wrong list is still processed correctly" is checked by BBMAP_CLASS_ORDER=2, which sends EVERY read to the other
list (all reads with imperfect sites to the short-path list and back): the results must not move."""
import numpy as np
import pytest

from bbmap_amd import workload as W
from bbmap_amd.index import DeviceIndex
from bbmap_amd.mapper import Mapper
from oracle import oracle as O
from tests import pair_problems as PP
from tests.mapper_check import FINAL_FIELDS, SITE_FIELDS, compare, gpu_fills

pytestmark = pytest.mark.gpu

K = PP.K_TEST
SWITCHES = ("BBMAP_CLASS_ORDER", "BBMAP_KERNARG_DEV", "BBMAP_CHUNK_LOADS")
EDGE_LENS = (10, 31, 32, 33, 63, 64, 65, 127, 128, 129, 149, 150, 151)
PAD = 40                    # N pad of the test reference: short, so that reads reach over both ends of the chromosome
REF_N = (5000, 5001, 9000, 12000, 12033)          # undefined bases inside the reference
_cache = {}


def _ref():
    if "ref" not in _cache:
        ref = W.make_reference(40000, seed=77, pad=PAD, repeat_frac=0.1, families=20)
        for p in REF_N:
            ref[PAD + p] = ord("N")
        _cache["ref"] = ref
    return _cache["ref"]


def _device_index():
    if "di" not in _cache:
        _cache["di"] = DeviceIndex.build([_ref()], k=K)
    return _cache["di"]


def _sub(b):
    return b"CATG"[b"ACGT".index(bytes([b]))] if b in b"ACGT" else ord("A")


def _edge_read(ref, rng, L, i):
    """Read i of a chunk-edge batch: a window of the reference with the variant i % 10, on the strand (i // 10) % 2."""
    body = len(ref) - 2 * PAD
    v = i % 10
    pos = PAD + int(rng.integers(200, body - 2 * L - 700))
    if v == 5:                                       # over an undefined reference base
        pos = PAD + REF_N[(i // 10) % len(REF_N)] - int(rng.integers(0, L))
    if v == 8:                                       # hangs over the chromosome's start / end
        pos = PAD - 3 if (i // 20) % 2 == 0 else PAD + body - L + 3
    r = ref[pos:pos + L].copy()
    if v == 8:
        r[r == ord("N")] = ord("A")                   # the overhang is read as bases, not as N
    if v == 1:
        r[0] = _sub(r[0])
    elif v == 2:
        r[L - 1] = _sub(r[L - 1])
    elif v == 3:                                     # last base of a 32-byte chunk and of a 4-byte word, first of the next
        for p in (3, 31, 32, 63, 127):
            if p < L:
                r[p] = _sub(r[p])
    elif v == 4:
        r[min(L - 1, 3 + (i // 10) % 5)] = ord("N")
    elif v == 6 and L >= 60:                         # a deletion: the read needs a fill
        cut = L // 2
        r = np.concatenate([ref[pos:pos + cut], ref[pos + cut + 7:pos + L + 7]])
    elif v == 7 and L >= 60:                         # an insertion and two substitutions
        cut = L // 3
        r = np.concatenate([ref[pos:pos + cut], np.frombuffer(b"GATTA", np.uint8), ref[pos + cut:pos + L - 5]])
        r[L - 9] = _sub(r[L - 9])
        r[L - 2] = _sub(r[L - 2])
    elif v == 9:                                     # a run of substitutions at the 3' tip (tip search, clipping)
        for p in range(max(0, L - 7), L, 2):
            r[p] = _sub(r[p])
    r = np.ascontiguousarray(r[:L])
    assert len(r) == L
    if (i // 10) % 2:
        r = W.revcomp_rows(r.reshape(1, L)).reshape(L)
    return r


def _edge_batch(L, paired):
    rng = np.random.Generator(np.random.PCG64(1000 + L + (500 if paired else 0)))
    ref = _ref()
    n = 80
    reads = [_edge_read(ref, rng, L, i) for i in range(n)]
    if paired:                                       # mate 2: the window one insert further on, other strand, its own variant
        body = len(ref) - 2 * PAD
        out = []
        for i, r in enumerate(reads):
            pos = PAD + int(rng.integers(200, body - 3 * L - 900))
            a = ref[pos:pos + L].copy()
            b = W.revcomp_rows(ref[pos + L + 60:pos + 2 * L + 60].copy().reshape(1, L)).reshape(L)
            if i % 4 == 1:
                b[L - 1] = _sub(b[L - 1])
            if i % 4 == 2:
                a, b = r, b                            # a variant read with a mate from elsewhere
            if i % 4 == 3:
                a = r
                b = W.revcomp_rows(_edge_read(ref, rng, L, i + 3).reshape(1, L)).reshape(L)
            out += [a, b]
        reads = out
    return reads


def _set(monkeypatch, value):
    for s in SWITCHES:
        monkeypatch.setenv(s, value)


def _map_records(records, paired, max_sites=32, **kw):
    mp = Mapper.from_records(_device_index(), *records, paired=paired, max_sites=max_sites, **kw)
    try:
        mp.step()
        return mp.fetch(), mp.stats()
    finally:
        mp.close()


def _site_rows(out):
    ns = out["nsites"]
    keep = np.arange(out["sites"].shape[1])[None, :] < np.maximum(ns, 0)[:, None]
    return {f: np.where(keep, out["sites"][f], 0) for f in SITE_FIELDS}


def _same(a, b):
    """Differences between two device runs, positions in the logs and in the pool apart."""
    bad = []
    if not np.array_equal(a["nsites"], b["nsites"]):
        return ["nsites differ"]
    ra, rb = _site_rows(a), _site_rows(b)
    bad += ["site field %s differs" % f for f in SITE_FIELDS if not np.array_equal(ra[f], rb[f])]
    fa, fb = gpu_fills(a), gpu_fills(b)
    if set(fa) != set(fb):
        bad.append("fill sets differ")
    for k_ in set(fa) & set(fb):
        for f in ("kind", "refStartLoc", "refEndLoc", "minScore", "score", "iterations", "match_len", "match"):
            if f in fa[k_] and not np.array_equal(fa[k_][f], fb[k_][f]):
                bad.append("fill %r field %s differs" % (k_, f))
    if "final" in a:
        for f in FINAL_FIELDS:
            if not np.array_equal(a["final"][f], b["final"][f]):
                bad.append("final field %s differs" % f)
        for r in range(len(a["final"])):
            x, y = a["final"][r], b["final"][r]
            ma = a["final_match"][int(x["match_off"]):int(x["match_off"]) + int(x["match_len"])]
            mb = b["final_match"][int(y["match_off"]):int(y["match_off"]) + int(y["match_len"])]
            if not np.array_equal(ma, mb):
                bad.append("read %d match string differs" % r)
    return bad


def _on_off(monkeypatch, run, orc, n, paired):
    outs = {}
    for value in ("1", "0"):
        _set(monkeypatch, value)
        out, st = run()
        bad = compare(out, orc, n, paired=paired)
        assert not bad, "switches %s: %d differences\n" % (value, len(bad)) + "\n".join(bad[:20])
        outs[value] = (out, st)
    bad = _same(outs["1"][0], outs["0"][0])
    assert not bad, "\n".join(bad[:20])
    return outs["1"]


@pytest.mark.parametrize("paired", (False, True))
@pytest.mark.parametrize("L", EDGE_LENS)
def test_chunk_edges_match_oracle(monkeypatch, L, paired):
    reads = _edge_batch(L, paired)
    records = PP.make_records(reads)
    orc = PP.oracle_map(_ref(), *records, paired=paired)
    out, st = _on_off(monkeypatch, lambda: _map_records(records, paired), orc, len(reads), paired)
    if L >= 63:
        assert st["fills"] + st["gapped_fills"] > 0 and int((out["nsites"] > 0).sum()) > len(reads) // 2


# ---------------------------------------------------------------------------------------------- sites that leave the chromosome array
# The edge batches above stay inside the array (its N pads belong to it).  Here the reference has NO pad, so that the array's ends
# are the sequence's, and sites really reach past them: `start < 0`, `stop >= reflen` -- set_perfect's clamped form and Words::next8's clamp
# to the last word of the array.
def _ref0():
    if "ref0" not in _cache:
        _cache["ref0"] = W.make_reference(40000, seed=78, pad=0, repeat_frac=0.1, families=20)
    return _cache["ref0"]


def _device_index0():
    if "di0" not in _cache:
        _cache["di0"] = DeviceIndex.build([_ref0()], k=K)
    return _cache["di0"]


def _hanging(L, n, seed):
    """n reads of L bases that hang h = 1 .. min(29, L // 3) bases over the start (even reads) or the end (odd reads) of the array, on
    either strand, with two substitutions; and the site that says so: [-h, L - h - 1] or [reflen - (L - h), reflen + h - 1]."""
    ref = _ref0()
    R = len(ref)
    rng = np.random.default_rng(seed)
    reads, sites = [], np.zeros((n, 32), O.MSITE_DTYPE)
    for i in range(n):
        h = int(rng.integers(1, max(1, min(29, L // 3)) + 1))
        over = W.BASES[rng.integers(0, 4, h)]
        if i % 2 == 0:
            r, a, b = np.concatenate([over, ref[:L - h]]), -h, L - h - 1
        else:
            r, a, b = np.concatenate([ref[R - (L - h):], over]), R - (L - h), R + h - 1
        r = r.copy()
        if L > 12:
            r[rng.integers(h, L - h, 2)] = ord("A")
        strand = (i // 2) % 2
        if strand:
            r = W.revcomp_rows(r.reshape(1, L)).reshape(L)
        reads.append(np.ascontiguousarray(r))
        t = sites[i, 0]
        t["chrom"], t["strand"], t["start"], t["stop"], t["hits"] = 1, strand, a, b, 5
        t["quickScore"] = t["score"] = t["slowScore"] = (70 + 100 * (L - 1)) * 6 // 10
        t["match_job"] = -1
    return reads, sites, np.ones(n, np.int32)


def _final_only(records, sites, nsites, paired):
    mp = Mapper.from_records(_device_index0(), *records, paired=paired, max_sites=32)
    try:
        mp.step()                                    # (writes the reverse complements the stage reads)
        mp.final_only(sites, nsites)
        return mp.fetch(), mp.stats()
    finally:
        mp.close()


@pytest.mark.parametrize("paired", (False, True))
@pytest.mark.parametrize("L", EDGE_LENS)
def test_sites_over_both_array_ends_final_stage(monkeypatch, L, paired):
    """The final stage over one-site lists that reach past the array: fixXY / clipTipIndels / setPerfect on sites with start < 0 and
    stop >= reflen, and the lists that come out still hold such sites."""
    n = 48
    reads, sites, nsites = _hanging(L, n, seed=200 + L)
    records = PP.make_records(reads)
    ref = _ref0()
    oi = O.OracleIndex([ref], k=K)
    oi.s.p.quitAfterTwoPerfects = 0 if paired else 1
    orc = O.final_reads(oi, records[0], records[1], sites, nsites, paired=paired)
    # A site that ends past the array has no ungapped string (scoreNoIndelsAndMakeMatchString returns at once and leaves its array as
    # it was), and when its fill fails as well the reference goes on with that unwritten array: Java has zeros there, the oracle
    # whatever malloc returned, the device whatever the pool held.  Reads (pairs) with a failed fill are taken out of the batch.
    failed = {int(r) for r in orc["log"]["read"][orc["log"]["score_len"] == 0]}
    if paired:
        failed |= {r ^ 1 for r in failed}
    if failed:
        keep = [r for r in range(n) if r not in failed]
        reads, sites, nsites, n = [reads[r] for r in keep], sites[keep], nsites[keep], len(keep)
        records = PP.make_records(reads)
        orc = O.final_reads(oi, records[0], records[1], sites, nsites, paired=paired)
        assert not (orc["log"]["score_len"] == 0).any()
    top = orc["sites"][:, 0]
    have = orc["nsites"] > 0
    assert int((have & (top["start"] < 0)).sum()) >= 3 and int((have & (top["stop"] >= len(ref))).sum()) >= 3, \
        (int((have & (top["start"] < 0)).sum()), int((have & (top["stop"] >= len(ref))).sum()))
    _on_off(monkeypatch, lambda: _final_only(records, sites, nsites, paired), orc, n, paired)


@pytest.mark.parametrize("L", (64, 100, 150))
def test_reads_at_both_array_ends_whole_flow(monkeypatch, L):
    """Reads with an insertion 1 .. 40 bases inside either end of the array, both strands: the probe's sites are shorter than the
    read and lie within a few bases of the array's ends, and their fills' windows reach past both ends.  (A site the probe itself
    places past an end does not survive removeOutOfBounds: such reads have no list, here and in the reference.)"""
    ref = _ref0()
    R = len(ref)
    rng = np.random.default_rng(300 + L)
    reads = []
    for ins in (3, 5, 9):
        for s_ in (1, 2, 4, 8, 16, 40):
            j = W.BASES[rng.integers(0, 4, ins)]
            a = np.concatenate([ref[s_:s_ + 40], j, ref[s_ + 40:s_ + L - ins]])
            b = np.concatenate([ref[R - s_ - (L - ins):R - s_ - 40], j, ref[R - s_ - 40:R - s_]])
            for r in (a, b):
                reads += [np.ascontiguousarray(r), W.revcomp_rows(r.reshape(1, L)).reshape(L)]
    records = PP.make_records(reads)
    orc = PP.oracle_map(ref, *records, paired=False)
    log = orc["log"]
    assert int((log["refStartLoc"] < 0).sum()) >= 4 and int((log["refEndLoc"] >= R).sum()) >= 2
    assert int((orc["nsites"] > 0).sum()) >= len(reads) // 2

    def run():
        mp = Mapper.from_records(_device_index0(), *records, paired=False, max_sites=32)
        try:
            mp.step()
            return mp.fetch(), mp.stats()
        finally:
            mp.close()
    _on_off(monkeypatch, run, orc, len(reads), False)


# ---------------------------------------------------------------------------------------------- class lists
L_CLASS = 100


def _class_reads(kind, n_units, paired, seed):
    """n_units reads (pairs) of L_CLASS bases: kind 'perfect' = exact copies, 'imperfect' = every read with substitutions or an
    indel, 'alternate' = the two in turn, 'nosite' = every fourth pair's mate 2 is random sequence (no site)."""
    ref = _ref()
    rng = np.random.Generator(np.random.PCG64(seed))
    body = len(ref) - 2 * PAD
    L = L_CLASS
    rows = []
    for u in range(n_units):
        pos = PAD + int(rng.integers(200, body - 3 * L - 600))
        mates = [ref[pos:pos + L].copy()]
        if paired:
            mates.append(W.revcomp_rows(ref[pos + L + 80:pos + 2 * L + 80].copy().reshape(1, L)).reshape(L))
        for w, r in enumerate(mates):
            damaged = kind == "imperfect" or (kind in ("alternate", "nosite") and (u + w) % 2 == 1)
            if damaged:
                if u % 3 == 0:                      # a deletion
                    cut = 30 + u % 40
                    src = mates[w] if w == 0 else W.revcomp_rows(mates[w].reshape(1, L)).reshape(L)
                    src = np.concatenate([src[:cut], src[cut + 4:], np.frombuffer(b"ACGT", np.uint8)])
                    r = src if w == 0 else W.revcomp_rows(src.reshape(1, L)).reshape(L)
                else:
                    for p in (5 + u % 7, 50, L - 1 - u % 5):
                        r[p] = _sub(r[p])
            if kind == "nosite" and w == 1 and u % 4 == 0:
                r = W.BASES[rng.integers(0, 4, size=L, dtype=np.uint8)]
            rows.append(np.ascontiguousarray(r))
    return np.stack(rows)


def _map_uniform(reads, paired, max_sites=32, di=None, **kw):
    L = reads.shape[1]
    offs = O.make_offsets(L, K, 1.9)
    ks = [100 * K] * len(offs)
    mp = Mapper(di or _device_index(), len(reads), L, offs, ks, paired=paired, max_sites=max_sites, **kw)
    try:
        mp.load_reads(reads)
        mp.step()
        return mp.fetch(), mp.stats()
    finally:
        mp.close()


def _oracle_uniform(ref, reads, paired, cap=64):
    L = reads.shape[1]
    offs = O.make_offsets(L, K, 1.9)
    ks = [100 * K] * len(offs)
    oi = O.OracleIndex([ref], k=K)
    oi.s.p.quitAfterTwoPerfects = 0 if paired else 1
    if paired:
        return O.map_batch(oi, reads[0::2].copy(), reads[1::2].copy(), L, offs, ks, cap=cap)
    return O.map_batch(oi, reads, None, L, offs, ks, cap=cap)


@pytest.mark.parametrize("kind,paired", [(k_, p) for k_ in ("perfect", "imperfect", "alternate") for p in (False, True)] + [("nosite", True)])
def test_class_lists_by_mix(monkeypatch, kind, paired):
    reads = _class_reads(kind, 150, paired, seed=31)
    orc = _oracle_uniform(_ref(), reads, paired)
    out, st = _on_off(monkeypatch, lambda: _map_uniform(reads, paired), orc, len(reads), paired)
    if kind == "perfect":                            # (a repeat copy beside the exact site may still ask for a fill)
        mapped = out["nsites"] > 0
        defined = (reads != ord("N")).all(axis=1)     # (a copy of an undefined reference base is not a match)
        assert mapped.mean() > 0.9 and (out["sites"][:, 0]["perfect"][mapped & defined] != 0).all()
    if kind in ("imperfect", "alternate"):
        assert st["fills"] + st["gapped_fills"] > 20
    if kind == "nosite":
        assert int((out["nsites"][1::2] == 0).sum()) > 10


@pytest.mark.parametrize("paired", (False, True))
@pytest.mark.parametrize("n_units", (1, 63, 64, 65, 127, 128, 129))
def test_class_lists_by_batch_size(monkeypatch, n_units, paired):
    reads = _class_reads("alternate", n_units, paired, seed=40 + n_units)
    orc = _oracle_uniform(_ref(), reads, paired)
    _on_off(monkeypatch, lambda: _map_uniform(reads, paired), orc, len(reads), paired)


@pytest.mark.parametrize("paired", (False, True))
def test_swapped_class_lists_change_nothing(monkeypatch, paired):
    """Every read on the wrong list: the reads that need fills on the short-path list, the perfect ones on the long-path list."""
    reads = _class_reads("alternate", 150, paired, seed=52)
    orc = _oracle_uniform(_ref(), reads, paired)
    _set(monkeypatch, "1")
    monkeypatch.setenv("BBMAP_CLASS_ORDER", "2")
    out, st = _map_uniform(reads, paired)
    bad = compare(out, orc, len(reads), paired=paired)
    assert not bad, "\n".join(bad[:20])
    assert st["fills"] + st["gapped_fills"] > 20
    _set(monkeypatch, "1")
    bad = _same(out, _map_uniform(reads, paired)[0])
    assert not bad, "\n".join(bad[:20])


def test_class_lists_with_overflowed_mates(monkeypatch):
    """max_sites = 4 on a repeat-rich reference: pairs of which a mate's list overflows are on neither list and go to the tier."""
    ref = W.make_reference(200000, seed=11, pad=2000, repeat_frac=0.6, families=3)
    reads, _ = W.make_pairs(ref, 300, read_len=L_CLASS, seed=8, pad=2000, hard_frac=0.08)
    reads = reads.reshape(-1, L_CLASS)
    orc = _oracle_uniform(ref, reads, True, cap=1024)
    di = DeviceIndex.build([ref], k=K)
    try:
        out, st = _on_off(monkeypatch, lambda: _map_uniform(reads, True, max_sites=4, di=di), orc, len(reads), True)
    finally:
        di.close()
    assert st["reads_reprobed"] > 20 and int((out["nsites"] == -3).sum()) == st["reads_reprobed"]


def test_logs_and_pool_grow_in_class_order(monkeypatch):
    """Fill logs and match-string pool far too small: the reads that found no room repeat their step after the host has grown them."""
    monkeypatch.setenv("BBMAP_FINAL_POOL_UNITS", "4096")
    reads = _class_reads("alternate", 600, False, seed=61)
    orc = _oracle_uniform(_ref(), reads, False)
    out, st = _on_off(monkeypatch, lambda: _map_uniform(reads, False, jobsPerRead=-64), orc, len(reads), False)
    assert st["log_growths"] >= 1 and len(out["final_match"]) > 4 * 4096
