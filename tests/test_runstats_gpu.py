"""Run statistics on the device (run_stats.hip: bbpipe_run_stats_device, bbmap_add_run_stats) and the adaptive state they drive.

Every counter and every histogram bin must equal tests/runstats_check.py (the sequential restatement, pinned by hand in
tests/test_runstats_cpu.py) exactly.  Independent of the restatement, on the mapped runs: matchCountM + S + I + N = the summed lengths of
mapped reads that have a string, the histogram's total = mate-1 paired reads with a positive insert, firstSiteCorrect* +
firstSiteIncorrect = mappedRetained."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from bbmap_amd import keys as K
from bbmap_amd import reference as R
from bbmap_amd import runstats as RS
from bbmap_amd.index import DeviceIndex, PROFILE_PACBIO, READ_DTYPE
from bbmap_amd.mapper import FINAL_DTYPE, MSITE_DTYPE, Mapper
from tests import runstats_check as RC
from tests.test_scaffolds_gpu import ACGT, KL, _mutate, _rc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SYMS = np.frombuffer(b"mmmmmmmmmmmmSSDIXYNC", np.uint8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


# ------------------------------------------------------------------------------------------------ the raw form, synthetic records
def _synthetic(rng, n, paired, cap, scheme, str_lens=None, list_sizes=None):
    """n reads with random final records, strings and site lists: ties in the scores, truth that is a site's place exactly, nearly, or
    nowhere, or absent; pairs that are paired, unpaired or half mapped."""
    lens = rng.integers(30, 400, n).astype(np.int32)
    fin = np.zeros(n, FINAL_DTYPE)
    sites = np.zeros((n, cap), MSITE_DTYPE)
    nsites = np.zeros(n, np.int32)
    truth = np.zeros(n, RS.TRUTH_DTYPE)
    strings, off = [], 0
    for r in range(n):
        k = int(list_sizes[r]) if list_sizes is not None else (0 if rng.random() < 0.15 else int(rng.integers(1, cap + 1)))
        nsites[r] = k if k > 0 else int(rng.choice([0, -1, -2]))
        f = fin[r]
        f["chrom"], f["start"], f["stop"] = -1, -1, -1
        truth[r]["chrom"] = -1
        if k <= 0:
            continue
        s = sites[r][:k]
        s["score"] = np.sort(rng.integers(1, max(2, k // 2 + 2), k))[::-1] * 100          # ties: groups of more than one site
        s["chrom"] = rng.integers(1, 3, k); s["strand"] = rng.integers(0, 2, k)
        s["start"] = rng.integers(0, 100000, k); s["stop"] = s["start"] + lens[r] - 1
        s["perfect"] = rng.random(k) < 0.1; s["semiperfect"] = s["perfect"] | (rng.random(k) < 0.1)
        s["slowScore"] = rng.integers(0, 1000, k)
        if rng.random() < 0.3:
            s["slowScore"][0] = RC.max_quality(int(rng.integers(0, 2)), int(lens[r]))       # one scheme's maxQuality, not the other's
        f["mapped"] = rng.random() < 0.95
        f["chrom"], f["strand"], f["start"], f["stop"] = s[0]["chrom"], s[0]["strand"], s[0]["start"], s[0]["stop"]
        f["ambiguous"], f["perfect"], f["rescued"] = rng.random() < 0.2, rng.random() < 0.2, rng.random() < 0.2
        how = rng.integers(0, 5)
        if how < 4:
            j = 0 if how == 0 else int(rng.integers(0, k))
            da, db = [(0, 0), (0, 0), (3, 4), (15, 30)][how]                               # exact, exact, within thresh 5, loose only
            truth[r] = (s[j]["chrom"], s[j]["strand"], s[j]["start"] - da, s[j]["stop"] - db)
        ml = int(str_lens[r]) if str_lens is not None else (0 if rng.random() < 0.1 else int(rng.integers(1, 700)))
        if ml > 0:
            strings.append(SYMS[rng.integers(0, len(SYMS), ml)])
            f["match_len"], f["match_off"] = ml, off
            off += ml + int(rng.integers(0, 5))
            strings.append(np.zeros(off - int(f["match_off"]) - ml, np.uint8))
    if paired:
        for p in range(0, n - 1, 2):
            a, b = fin[p], fin[p + 1]
            if a["mapped"] and b["mapped"] and nsites[p] > 0 and nsites[p + 1] > 0:
                how = rng.integers(0, 4)
                if how < 3:                                                             # near each other; paired unless how == 2
                    b["chrom"] = a["chrom"]
                    b["start"] = a["start"] + int(rng.integers(-600, 45000 if how == 1 else 600)); b["stop"] = b["start"] + lens[p + 1] - 1
                    if rng.random() < 0.1:
                        b["stop"] = b["start"]
                    a["paired"] = b["paired"] = how != 2
    fin["nsites"] = nsites
    pool = np.concatenate(strings + [np.zeros(8, np.uint8)])
    return dict(lens=lens, fin=fin, sites=sites, nsites=nsites, truth=truth, pool=pool, cap=cap, paired=paired, scheme=scheme)


def _check_raw(d, thresh=0, with_truth=True, with_hist=True):
    n = len(d["fin"])
    recs = np.zeros(n, READ_DTYPE)
    recs["len"] = d["lens"]
    hist = torch.zeros(RS.INSERT_HIST_BINS, dtype=torch.int64, device=DEV) if with_hist else None
    got, _ = RS.run_stats_device(_dev(recs), _dev(d["fin"]), _dev(d["pool"]), _dev(d["sites"]), _dev(d["nsites"]), d["cap"], d["paired"],
                                 d["scheme"], thresh, _dev(d["truth"]) if with_truth else None, None, hist)
    matches = [d["pool"][int(f["match_off"]): int(f["match_off"]) + int(f["match_len"])].tobytes() if int(f["match_len"]) > 0 else None
               for f in d["fin"]]
    lists = [d["sites"][r][:max(0, int(d["nsites"][r]))] for r in range(n)]
    want, whist = RC.run_stats(d["fin"], matches, lists, d["lens"], d["paired"], d["truth"] if with_truth else None, d["scheme"], thresh)
    assert not RC.differences(got, want), RC.differences(got, want)
    if with_hist:
        assert np.array_equal(hist.cpu().numpy(), whist)
    return want, whist


@pytest.mark.parametrize("paired", [False, True])
def test_string_lengths_and_step_borders(paired):
    """strings of 1, 63, 64, 65, 128, 129 symbols and one longer than 65,535 bytes; a D run and an I run across the 64-symbol border"""
    rng = np.random.default_rng(5 + paired)
    sl = [1, 63, 64, 65, 128, 129, 70001, 200, 200, 64]
    d = _synthetic(rng, len(sl), paired, 4, 0, str_lens=sl, list_sizes=[1, 2, 3, 4, 1, 2, 3, 4, 1, 2])
    for r, run in ((7, b"D"), (8, b"I")):                     # 'm' x 60, the run x 10 (columns 60..69), 'm' to the end
        o = int(d["fin"][r]["match_off"])
        d["pool"][o: o + 200] = np.frombuffer(b"m" * 60 + run * 10 + b"m" * 130, np.uint8)
    want, _ = _check_raw(d)
    assert want["matchCountD1"] + want["matchCountD2"] >= 10 and want["matchCountI1"] + want["matchCountI2"] >= 10
    _check_raw(d, thresh=5, with_truth=True, with_hist=False)


def test_site_list_sizes_and_chunk_carries():
    """lists of 1, 63, 64, 65, 130 and 4,096 sites; a score change exactly at a chunk border, the first correct site in the second
    chunk, the loose-only hit at site 0"""
    rng = np.random.default_rng(9)
    sizes = [1, 63, 64, 65, 130, 4096, 130, 130, 1]
    d = _synthetic(rng, len(sizes), False, 4096, 0, list_sizes=sizes)
    s = d["sites"][6]                                          # one score for sites 0..63, the next from site 64 on; truth = site 70
    s["score"][:64] = 900; s["score"][64:130] = 800
    s["start"][:130] = np.arange(130) * 1000; s["stop"][:130] = s["start"][:130] + 99
    s["chrom"][:130] = 1; s["strand"][:130] = 0
    d["truth"][6] = (1, 0, 70000, 70099)
    s = d["sites"][7]                                          # every site its own group; truth = site 64, the second chunk's first
    s["score"][:130] = 10000 - np.arange(130); s["start"][:130] = np.arange(130) * 1000; s["stop"][:130] = s["start"][:130] + 99
    s["chrom"][:130] = 2; s["strand"][:130] = 1
    d["truth"][7] = (2, 1, 64000, 64099)
    s = d["sites"][8]
    s["chrom"][0], s["strand"][0], s["start"][0], s["stop"][0] = 1, 0, 515, 640
    d["truth"][8] = (1, 0, 500, 599)                           # start 15 off, stop 41 off: loose only
    want, _ = _check_raw(d)
    assert want["correctLowHit1"] >= 2 and want["firstSiteCorrectLoose1"] > want["firstSiteCorrectP1"] + want["firstSiteCorrectM1"]
    _check_raw(d, thresh=5)
    _check_raw(d, with_truth=False, with_hist=False)


@pytest.mark.parametrize("n,paired", [(1, False), (2, True), (2 * RS.RUNSTATS_MAX_WAVES + 1, False), (2 * RS.RUNSTATS_MAX_WAVES + 2, True)])
def test_read_counts_and_the_persistent_loop(n, paired):
    """1 read, one pair, and more reads than twice the grid's wavefronts (an odd read left alone in single-ended mode)"""
    rng = np.random.default_rng(n)
    d = _synthetic(rng, n, paired, 3, 0)
    want, whist = _check_raw(d)
    assert want["readsUsed1"] + want["readsUsed2"] == n
    if paired and n > 2:
        assert whist.sum() > 0 and whist[RS.INSERT_HIST_BINS - 1] > 0 and want["badPairs"] > 0 and want["numMated"] > 0


@pytest.mark.parametrize("scheme", [0, 1])
def test_both_schemes_and_thresholds(scheme):
    rng = np.random.default_rng(20 + scheme)
    d = _synthetic(rng, 400, True, 70, scheme)
    a, _ = _check_raw(d, thresh=0)
    b, _ = _check_raw(d, thresh=5)
    assert a["perfectMatch1"] > 0 and b["firstSiteCorrectP1"] + b["firstSiteCorrectM1"] > a["firstSiteCorrectP1"] + a["firstSiteCorrectM1"]
    _check_raw(dict(d, scheme=1 - scheme))                    # the other scheme's maxQuality over the same records


# ------------------------------------------------------------------------------------------------ mapped batches
@functools.lru_cache(maxsize=None)
def genome():
    """Ten seeded scaffolds on two chromosomes; scaffold 3 carries a copy of 800 bases of scaffold 1 (a repeat), scaffold 0 is 40 kb
    long (room for mates further apart than maxPairDist)."""
    rng = np.random.default_rng(77)
    lens = [40000, 6000, 3000, 7000, 5000, 9000, 4000, 8000, 3500, 6500]
    bodies = [ACGT[rng.integers(0, 4, n)] for n in lens]
    bodies[3][2000:2800] = bodies[1][1000:1800]
    recs = [("s%d" % i, b) for i, b in enumerate(bodies)]
    p = R.pack(recs, max_length=60000)
    assert p.nchroms >= 2
    return p


def _pairs(n_pairs, seed):
    """(reads: list of uint8 arrays, mates interleaved; truth TRUTH_DTYPE per read)"""
    p = genome()
    rng = np.random.default_rng(seed)
    sb = p.scaffold_bases()
    reads, truth = [], []

    def seg(g, o, n):
        c, a, _ = sb[g]
        return p.chroms[c - 1][a + o: a + o + n].copy()

    def put(rd, t=None):
        reads.append(np.asarray(rd, np.uint8))
        truth.append(t if t is not None else (-1, 0, 0, 0))

    for i in range(n_pairs):
        kind = i % 10
        l1, l2 = int(rng.integers(100, 151)), int(rng.integers(100, 151))
        g = int(rng.integers(1, len(sb)))
        c, a, n = sb[g]
        o = int(rng.integers(0, n - 700))
        gap = int(rng.integers(250, 350))
        t1, t2 = (c, 0, a + o, a + o + l1 - 1), (c, 1, a + o + gap, a + o + gap + l2 - 1)
        m1, m2 = _mutate(rng, seg(g, o, l1), 2), _rc(_mutate(rng, seg(g, o + gap, l2), 2))
        if kind < 4:
            put(m1, t1); put(m2, t2)
        elif kind == 4:                                         # an insertion and a deletion in mate 1, Ns in mate 2
            m1 = np.concatenate([seg(g, o, 50), ACGT[rng.integers(0, 4, 2)], seg(g, o + 50, 30), seg(g, o + 83, l1 - 82)])
            m2 = m2.copy(); m2[rng.choice(l2, 3, replace=False)] = ord("N")
            put(m1); put(m2)
        elif kind == 5:                                         # maps nowhere
            put(ACGT[rng.integers(0, 4, l1)]); put(ACGT[rng.integers(0, 4, l2)])
        elif kind == 6:                                         # the mate lies on another scaffold
            g2 = 1 + (g % (len(sb) - 1))
            put(m1, t1); put(_rc(seg(g2, 300, l2)))
        elif kind == 7:                                         # a substitution every 10 bases: no key survives, only rescue finds it
            m2 = seg(g, o + gap, l2)
            for j in range(4, l2, 10):
                m2[j] = ACGT[(int(np.searchsorted(ACGT, m2[j])) + 1) % 4]
            put(m1, t1); put(_rc(m2))
        elif kind == 8:                                         # both mates inside the repeat
            put(seg(1, 1020, l1)); put(_rc(seg(1, 1020 + 300, l2)))
        else:                                                   # further apart than maxPairDist
            o = int(rng.integers(0, 3000))
            put(seg(0, o, l1)); put(_rc(seg(0, o + 33500, l2)))
    return reads, np.array(truth, RS.TRUTH_DTYPE)


_restate, _check_mapped = RC.restate, RC.check_mapped           # (other test modules take them from tests/runstats_check.py)


def _mapper(reads, paired, profile=0, **kw):
    p = genome()
    di = DeviceIndex.build(p.chroms, k=KL if profile == 0 else None, profile=profile)
    di.set_scaffolds(p)
    recs, blob, bs, ki = K.make_batch([r for r in reads], None, K.default_config(profile))
    mp = Mapper.from_records(di, recs, blob, bs, ki, paired=paired, profile=profile, **kw)
    return di, mp


def test_mapped_pairs_every_counter():
    reads, truth = _pairs(300, 1)
    di, mp = _mapper(reads, True, max_sites=64)
    try:
        mp.step()
        got, want = _check_mapped(mp, reads, True, truth)
        print({k: int(want[k]) for k in want if want[k]})
        two = lambda k: int(want[k + "1"]) + int(want[k + "2"])
        assert want["badPairs"] > 0 and want["bothUnmapped"] > 0 and want["numMated"] > 0
        assert two("rescuedP") + two("rescuedM") > 0
        assert two("ambiguousBestAlignment") > 0
        assert two("readCountI") > 0 and two("readCountD") > 0 and two("readCountN") > 0
        assert two("topSiteSum") > two("uniqueHit") and two("topSiteSum") > two("mappedRetained")       # a top group of more than one site
        assert two("semiperfectMatch") > 0
        assert want["numMatedBases"] != want["insertSizeSum"] - want["innerLengthSum"]               # unequal mates: :1481
        # ---- accumulation: another batch sums to the restatement over both; a second count of one batch is refused and changes
        # nothing; reset gives zeros
        _, whist = RC.run_stats(*_restate(mp, reads, True, truth), True, truth, 0, 0, mp.cfg.maxPairDist)
        reads2, truth2 = _pairs(300, 11)
        _load(mp, reads2)
        mp.step()
        mp.add_run_stats(truth2)
        twice, hist2 = mp.run_stats()
        both, bhist = RC.run_stats(*_restate(mp, reads2, True, truth2), True, truth2, 0, 0, mp.cfg.maxPairDist, stats=dict(want), hist=whist.copy())
        assert both["readsUsed1"] == 600 and both["numMated"] > want["numMated"] and any(both[k] != 2 * want[k] for k in both)
        assert not RC.differences(twice, both), RC.differences(twice, both)
        assert np.array_equal(hist2, bhist)
        assert mp.L.bbmap_add_run_stats(mp.h, None, None) == -2
        again, hist3 = mp.run_stats()
        assert again.tobytes() == twice.tobytes() and np.array_equal(hist2, hist3)
        mp.reset_run_stats()
        zero, hist0 = mp.run_stats()
        assert not any(int(zero[k]) for k in RS.RUNSTATS_DTYPE.names) and hist0.sum() == 0
    finally:
        mp.close()
        di.close()


def _load(mp, reads, profile=0):
    """another batch into the same context"""
    mp.load_records(*K.make_batch([r for r in reads], None, K.default_config(profile)))


def test_mapped_single_ended():
    reads, truth = _pairs(300, 2)
    di, mp = _mapper(reads, False, max_sites=64)
    try:
        mp.step()
        got, want = _check_mapped(mp, reads, False, truth)
        assert want["readsUsed2"] == 0 and want["numMated"] == 0 and want["bothUnmapped"] > 0 and want["mappedRetained1"] > 400
    finally:
        mp.close()
        di.close()


def test_overflow_tier_reads_take_the_tiers_lists():
    reads, truth = _pairs(300, 3)
    di, mp = _mapper(reads, True, max_sites=1, reserved=(C.c_int32 * 4)(0, 4096, 256, 0))
    try:
        mp.step()
        assert mp.stats()["reads_reprobed"] > 0
        _check_mapped(mp, reads, True, truth)
    finally:
        mp.close()
        di.close()


def test_pacbio_profile_final_stage():
    reads, truth = _pairs(60, 4)
    di, mp = _mapper(reads, False, profile=PROFILE_PACBIO, max_sites=64, finalStage=1)
    try:
        mp.step()
        got, want = _check_mapped(mp, reads, False, truth, scheme=1)
        assert want["mappedRetained1"] > 30
    finally:
        mp.close()
        di.close()


def test_context_without_final_stage_is_refused():
    reads, truth = _pairs(20, 5)
    di, mp = _mapper(reads, True, max_sites=64, finalStage=0)
    try:
        assert mp.L.bbmap_add_run_stats(mp.h, None, None) == -2          # no batch yet, no final stage
        mp.step()
        assert mp.L.bbmap_add_run_stats(mp.h, None, None) == -2
        assert mp.L.bbmap_set_adaptive(mp.h, 1) == -2 and mp.L.bbmap_set_adaptive(mp.h, 4) == -2
    finally:
        mp.close()
        di.close()


# ------------------------------------------------------------------------------------------------ adaptive state
def _short_pairs(n_pairs, seed, split, hard=0):
    """100-base pairs with an inner distance near 300 (split = False), or whose mates lie on different scaffolds (split = True); hard:
    every hard-th pair's mate 2 has a substitution every 10 bases, so that no key survives and only rescue finds it"""
    p = genome()
    rng = np.random.default_rng(seed)
    sb = p.scaffold_bases()
    reads = []
    for i in range(n_pairs):
        g = int(rng.integers(1, len(sb)))
        c, a, n = sb[g]
        o = int(rng.integers(0, n - 700))
        reads.append(_mutate(rng, p.chroms[c - 1][a + o: a + o + 100], 1))
        if split:
            others = [x for x in range(len(sb)) if sb[x][0] != c]               # another chromosome: such mates never pair
            c2, a2, n2 = sb[others[int(rng.integers(0, len(others)))]]
            o2 = int(rng.integers(0, n2 - 200))
            reads.append(_rc(p.chroms[c2 - 1][a2 + o2: a2 + o2 + 100]))
        else:
            gap = 100 + int(rng.integers(290, 311))
            m2 = _mutate(rng, p.chroms[c - 1][a + o + gap: a + o + gap + 100], 1)
            if hard and i % hard == 0:
                m2 = p.chroms[c - 1][a + o + gap: a + o + gap + 100].copy()
                for j in range(4, 100, 10):
                    m2[j] = ACGT[(int(np.searchsorted(ACGT, m2[j])) + 1) % 4]
            reads.append(_rc(m2))
    return reads


def _lists_equal(a, b):
    """final records, match strings and site lists of two contexts' last batches; left out: where a string lies in its pool and which
    fill-log entry a site refers to (both follow the order in which the batch's wavefronts took their slots)"""
    fa, ba = a.final()
    fb, bb = b.final()
    oa, ob = a.fetch(with_match=False), b.fetch(with_match=False)
    names = [k for k in FINAL_DTYPE.names if k not in ("match_off", "reserved")]
    if not (all(np.array_equal(fa[k], fb[k]) for k in names) and ba.tobytes() == bb.tobytes() and np.array_equal(oa["nsites"], ob["nsites"])):
        return False                                       # (bbmap_get_final packs the strings in read order)
    snames = [k for k in MSITE_DTYPE.names if k not in ("match_job", "reserved")]
    return all(np.array_equal(oa["sites"][r][:max(0, n)][k], ob["sites"][r][:max(0, n)][k]) for r, n in enumerate(oa["nsites"]) for k in snames)


def test_adaptive_insert_length():
    reads = _short_pairs(1100, 6, False)
    di, mp = _mapper(reads, True, max_sites=16)
    plain = Mapper.from_records(di, *K.make_batch(reads, None, K.default_config(0)), paired=True, max_sites=16)
    try:
        assert mp.adaptive_state() == (100, 0)
        plain.step()
        mp.set_adaptive(RS.ADAPT_INSERT_LENGTH)
        mp.step()                                              # batch 1: still with 100
        assert _lists_equal(mp, plain)                         # flags move nothing inside a batch: equals a context with flags 0
        assert mp.L.bbmap_add_run_stats(mp.h, None, None) == -2                  # counted by the step itself
        st, _ = mp.run_stats()
        fin, matches, lists, lens = _restate(mp, reads, True, None)
        want, _ = RC.run_stats(fin, matches, lists, lens, True)
        assert not RC.differences(st, want)
        assert want["numMated"] > 1000
        apd = RC.insert_length_rule(want, True, 100)
        assert apd != 100 and 280 <= apd <= 320
        assert mp.adaptive_state() == (apd, 0)
        assert plain.adaptive_state() == (100, 0)              # flags 0: stays
        plain.step()
        assert plain.adaptive_state() == (100, 0) and _lists_equal(mp, plain)
        reads2 = _short_pairs(1100, 16, False)                 # batch 2, other pairs, with the new value
        _load(mp, reads2)
        _load(plain, reads2)
        mp.step()
        plain.set_average_pair_dist(apd)
        plain.step()
        assert _lists_equal(mp, plain)
        st2, _ = mp.run_stats()                                # the running counters hold both batches; the value moved with them
        both, _ = RC.run_stats(*_restate(mp, reads2, True, None), True, stats=dict(want))
        assert not RC.differences(st2, both), RC.differences(st2, both)
        assert mp.adaptive_state() == (RC.insert_length_rule(both, True, apd), 0)
    finally:
        plain.close()
        mp.close()
        di.close()


def test_adaptive_rescue_skip():
    reads = _short_pairs(1100, 7, True)
    di, mp = _mapper(reads, True, max_sites=16)
    plain = Mapper.from_records(di, *K.make_batch(reads, None, K.default_config(0)), paired=True, max_sites=16)
    try:
        mp.set_adaptive(RS.ADAPT_RESCUE_SKIP)
        mp.step()
        plain.step()
        assert mp.stats()["rescue_scans"] > 0 and mp.stats()["rescue_scans"] == plain.stats()["rescue_scans"]
        st, _ = mp.run_stats()
        assert RC.rescue_skip_rule(st) and mp.adaptive_state()[1] == 1 and plain.adaptive_state()[1] == 0
        mp.step()                                              # batch 2 starts with rescue skipped
        plain.step()
        assert mp.stats()["rescue_scans"] == 0 and plain.stats()["rescue_scans"] > 0
        mp.reset_run_stats()                                   # the counters no longer satisfy the rule: rescue resumes
        assert mp.adaptive_state()[1] == 0
        reads3 = _short_pairs(1100, 8, False, hard=5)          # batch 3: well-paired reads, a fifth of the mates for rescue to find
        _load(mp, reads3)
        _load(plain, reads3)
        mp.step()
        plain.step()
        assert mp.stats()["rescue_scans"] == plain.stats()["rescue_scans"] > 0 and _lists_equal(mp, plain)
        st3, _ = mp.run_stats()
        assert st3["numMated"] * 20 >= st3["mappedRetained2"] > 0 and st3["rescuedP2"] + st3["rescuedM2"] > 0
        assert not RC.rescue_skip_rule(st3) and mp.adaptive_state()[1] == 0
    finally:
        plain.close()
        mp.close()
        di.close()


# ------------------------------------------------------------------------------------------------ the PhiX fixture
def test_phix_fixture_with_truth_from_the_read_names():
    """The six runs of tests/test_golden_phix.py with calcCorrectness' `original` taken from the read names: every counter equals the
    restatement, and mappedRetained, firstSiteCorrectP + M and firstSiteCorrectLoose of each sample are at least FLOORS_FINAL's
    (mapped, strict, loose), the floors that file holds for the records BBMap prints.  Coordinates: the names carry start and stop in
    BBMap's padded chromosome space (chromosome 1 = 8,000 N + PhiX + 8,000 N, tests/golden_phix.py), which is the space of
    phix_reference() that the index is built from and of the mapper's sites and final records; test_golden_phix.py compares the same
    fields the same way."""
    from tests.golden_phix import fixture_inputs, fixture_runs, phix_reference, sample_reads
    from tests.test_golden_phix import FLOORS_FINAL
    di = DeviceIndex.build([phix_reference()], k=13)
    try:
        for name, r in fixture_runs().items():
            recs, blob, bs, ki, paired = r["inputs"]
            reads, _, _ = fixture_inputs(name.split("_")[0], name.endswith("_qual"))
            samples = (1, 2) if paired else (int(name[2]),)
            truth = np.zeros(len(recs), RS.TRUTH_DTYPE)
            for which in samples:
                _, t = sample_reads(which)
                v = truth[which - 1::2] if paired else truth
                v["chrom"], v["strand"], v["start"], v["stop"] = 1, t["strand"], t["start"], t["stop"]
            mp = Mapper.from_records(di, recs, blob, bs, ki, paired=paired, max_sites=32)
            try:
                mp.step()
                assert mp.stats()["reads_overflowed"] == 0
                got, want = _check_mapped(mp, reads, paired, truth)
            finally:
                mp.close()
            for which in samples:
                m = str(which) if paired else "1"
                triple = (int(got["mappedRetained" + m]), int(got["firstSiteCorrectP" + m]) + int(got["firstSiteCorrectM" + m]),
                          int(got["firstSiteCorrectLoose" + m]))
                floor = FLOORS_FINAL[(name[:2], which)]
                print(name, which, triple, floor)
                assert triple == (int(want["mappedRetained" + m]), int(want["firstSiteCorrectP" + m]) + int(want["firstSiteCorrectM" + m]),
                                  int(want["firstSiteCorrectLoose" + m]))
                assert all(g >= f for g, f in zip(triple, floor)), (name, which, triple, floor)
    finally:
        di.close()
