"""CPU tests of the mapper restatement on pairs whose mates differ in length (oracle/mapper_oracle.c: process_pair with len1 and
len2, BBMapThread.java:943-1098).  The restatement is what the device is compared with (tests/test_mixed_lengths_gpu.py), so what can
be pinned without the device is pinned here: equal mates give what the uniform entry gives, every bound belongs to the mate it is
applied to, planted mates come back where they were drawn, and the batch reaches the paths the GPU tests rely on.

The batch (tests/pair_problems.py: pair_batch): 1,760 pairs on a 300 kb reference, 110 of each class and 220 of (150,100),
(100,150), (151,149), (64,65), (128,127) -- at 600 pairs over the eleven classes alone the oracle fills only 7 rescues of a longer
mate from a shorter anchor.  What the oracle does with it (the device must do the same, and the GPU tests assert that it does):

    rescue fills  len(anchor) > len(loose) 134,  len(anchor) < len(loose) 26,  equal 6
    rescued sites len(anchor) > len(loose) 107,  len(anchor) < len(loose) 35,  equal 6
    class      pairs  reads with a site  top sites paired / unpaired  reads with a rescued site  (of them the shorter mate)
    (150,150)   110         220                 196 /  24                      6
    (150,100)   220         440                 388 /  52                     11                       7
    (100,150)   220         440                 388 /  52                     11                       8
    (150,36)    110         219                 192 /  27                      7                       6
    (40,150)    110         219                 190 /  29                      6                       6
    (151,149)   220         440                 390 /  50                     21                       8
    (64,65)     220         440                 384 /  56                      7                       2
    (128,127)   220         439                 388 /  51                     18                       9
    (150,12)    110         216                 190 /  26                      3                       3
    (150,11)    110         168                 110 /  58                     58                      58
    (9,150)     110         110                   0 / 110                      0                       0
"""
import math

import numpy as np

from oracle import oracle as O
from tests import pair_problems as PP
from tests.mapper_check import FINAL_FIELDS, SITE_FIELDS
from tests.problems import max_quality

INDEL = frozenset(b"ID")


def test_equal_mates_give_what_the_uniform_entry_gives():
    """map_reads over per-read records (every read with keys of its own) against map_batch, the uniform special case whose
    signature and callers did not change: site lists, final records, match strings and the fill log, field by field."""
    reads, _ = PP.equal_batch()
    n, L = reads.shape
    offs = O.make_offsets(L, PP.K_TEST, 1.9)
    ks = [100 * PP.K_TEST] * len(offs)
    recs = np.zeros(n, O.READ_DTYPE)
    recs["bases_off"] = np.arange(n, dtype=np.int64) * L
    recs["keys_off"] = np.arange(n, dtype=np.int64) * 2 * len(offs)
    recs["len"], recs["nkeys"] = L, len(offs)
    keyinfo = np.tile(np.array(list(offs) + ks, np.int32), n)
    ref = PP.reference()
    a = O.map_reads(PP.oracle_index(ref), recs, reads.reshape(-1), keyinfo, paired=True, cap=64, match_stride=4200, jobs_per_read=12)
    b = O.map_batch(PP.oracle_index(ref), reads[0::2].copy(), reads[1::2].copy(), L, offs, ks, cap=64, match_stride=4200)
    for w in (0, 1):
        ns, sites, fin, fm = a["nsites"][w::2], a["sites"][w::2], a["final"][w::2], a["fmatch"][w::2]
        assert np.array_equal(ns, b["nsites%d" % (w + 1)])
        assert sites.tobytes() == b["sites%d" % (w + 1)].tobytes()
        assert fin.tobytes() == b["final%d" % (w + 1)].tobytes() and np.array_equal(fm, b["fmatch%d" % (w + 1)])
    assert a["log"].tobytes() == b["log"].tobytes() and np.array_equal(a["match"], b["match"])       # (one thread: one order)
    assert a["stats"] == b["stats"] and a["stats"][2] > 50 and (a["log"]["kind"] == 2).sum() > 10
    assert set(SITE_FIELDS) <= set(sites.dtype.names) and set(FINAL_FIELDS) <= set(fin.dtype.names)


def _match_of(orc, job):
    ml = int(orc["log"]["match_len"][job])
    return orc["match"][job, :ml].tobytes()


def test_every_bound_is_the_own_mates():
    """A perfect site spans its own mate's length and scores its own mate's maxQuality (maxSwScore1 / 2, BBMapThread.java:983-986);
    a rescued site without an insertion or deletion spans the loose mate's length, and a rescue fill's traceback string has one
    symbol per base of the loose mate (slowRescue over `bases`, AbstractMapThread.java:1199-1210).  An oracle that used the other
    mate's length anywhere on these paths fails here."""
    b, orc = PP.pair_batch(), PP.pair_oracle()
    lens = b["truth"]["len"]
    perfect = plain_rescued = filled_rescued = 0
    unequal_perfect = 0
    for r, s in enumerate(PP.oracle_lists(orc)):
        L = int(lens[r])
        for x in s:
            span = int(x["stop"]) - int(x["start"]) + 1
            if int(x["perfect"]) == 1:
                assert span == L and int(x["slowScore"]) == max_quality(L), (r, L, x)
                perfect += 1
                unequal_perfect += int(lens[r ^ 1]) != L
            if int(x["rescued"]) and int(x["ngaps"]) == 0:
                job = int(x["match_job"])
                m = _match_of(orc, job) if job >= 0 else b""
                if job >= 0 and m:
                    assert int(orc["log"]["read"][job]) == r
                    assert sum(1 for ch in m if ch != ord("D")) == L, (r, L, m)
                    assert span == sum(1 for ch in m if ch != ord("I")), (r, L, m, x)
                    filled_rescued += 1
                if not (INDEL & set(m)):
                    assert span == L, (r, L, x, m)
                    plain_rescued += 1
    assert perfect > 1000 and unequal_perfect > 700 and plain_rescued > 60 and filled_rescued > 60, (perfect, unequal_perfect, plain_rescued, filled_rescued)


# class -> (share measured on this batch, drop against the control class (150,150), which reaches 1.0000).  The bound asserted is the
# control's share in the same run minus the drop, rounded down to a whole percent.
TRUTH = {(150, 150): (1.0000, 0.0), (150, 100): (1.0000, 0.0), (100, 150): (1.0000, 0.0), (150, 36): (0.9955, 0.0045),
         (40, 150): (0.9955, 0.0045), (151, 149): (0.9977, 0.0023), (64, 65): (1.0000, 0.0), (128, 127): (0.9977, 0.0023)}


def test_planted_mates_come_back_at_the_adjusted_truth():
    b, orc = PP.pair_batch(), PP.pair_oracle()
    share = PP.truth_shares(PP.oracle_lists(orc), b["truth"], b["cls"])
    print({c: round(v, 4) for c, v in share.items()})
    control = share[(150, 150)]
    assert [c for c in PP.CLASSES if min(c) >= 36] == list(TRUTH)
    for c, (_, drop) in TRUTH.items():
        bound = math.floor((control - drop) * 100 + 1e-9) / 100
        assert share[c] >= bound, (c, share[c], bound)
    # (the classes below 36 bases: the short mate is found by rescue alone or not at all; printed, not bounded)


def test_the_batch_reaches_what_the_gpu_tests_rely_on():
    b, orc = PP.pair_batch(), PP.pair_oracle()
    cov = PP.coverage(PP.oracle_lists(orc), PP.oracle_rescue_reads(orc), b["truth"]["len"], b["cls"])
    print({k: v for k, v in cov.items() if k != "classes"})
    for c, d in cov["classes"].items():
        print(c, d)
    assert not PP.check_coverage(cov), PP.check_coverage(cov)
    assert set(cov["classes"]) == set(PP.CLASSES) and (orc["nsites"] >= 0).all()
    # sub-k mates: no key in the records, so no site unless rescue put it there
    recs = b["records"][0]
    for p, c in enumerate(b["cls"]):
        for r in (2 * p, 2 * p + 1):
            if int(recs["len"][r]) < PP.K_TEST:
                assert int(recs["nkeys"][r]) == 0
                s = orc["sites"][r, :int(orc["nsites"][r])]
                assert s["rescued"].all()
    assert (recs["nkeys"][recs["len"] == 12] == 1).all()
    # fills are numbered per read without holes, rescue fills included
    log = orc["log"]
    order = np.lexsort((log["seq"], log["read"]))
    rd, sq = log["read"][order], log["seq"][order]
    first = np.concatenate([[True], rd[1:] != rd[:-1]])
    assert (sq[first] == 0).all() and (np.diff(sq)[~first[1:]] == 1).all()
