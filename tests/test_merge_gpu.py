"""The merge stage on the device: bbmerge_overlap_batch_device against the oracle's restatement of BBMerge's natives
(tests/merge_problems.py), bbmerge_join_batch_device against the host form and the restatement of Read.joinRead
(tests/merge_check.py), and merge_pairs on error-free fragments.  Records and bytes are compared as whole arrays, with no tolerance."""
import itertools

import numpy as np
import pytest
import torch

from bbmap_amd import merge as M
from bbmap_amd.index import READ_DTYPE
from tests import merge_problems as P
from tests.test_merge_cpu import (HAND, HAND_JOINS, HAND_JOINS_NOQ, check_fragments, check_joins, fragments, hand_join_inputs, hand_join_inputs_noq,
                                  join_inserts, slot)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def device_overlap(r1, r2, bases, quality, cfg):
    recs = M.overlap_batch_device(_dev(r1), _dev(r2), _dev(bases), None if quality is None else _dev(quality), cfg)
    return recs.cpu().numpy().view(M.REC_DTYPE)


def assert_records(got, exp):
    diff = np.flatnonzero(got != exp)
    assert got.shape == exp.shape and diff.size == 0, (diff[:5], got[diff[:5]], exp[diff[:5]])


# ------------------------------------------------------------------------------------------------ overlap
@pytest.mark.parametrize("name", sorted(P.CONFIGS))
def test_device_overlap_equals_the_oracle(name):
    pairs, (r1, r2, bases, quality) = P.problem_set()
    assert all(c > 0 for c in P.classes(P.expected_for(name)))
    assert_records(device_overlap(r1, r2, bases, quality, P.config(P.CONFIGS[name])), P.expected_for(name))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 0])
def test_pair_counts(n):
    pairs, (r1, r2, bases, quality) = P.problem_set()
    got = device_overlap(r1[:n], r2[:n], bases, quality, P.config(P.CONFIGS["quality-then-flat"]))
    assert_records(got, P.expected_for("quality-then-flat")[:n])


LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 511, 512)


def border_pairs():
    """every pair of LENGTHS (the 512 / 5 pair both ways round among them): b continues a's tail where both are long enough, with one
    substitution in every third pair; then the special contents"""
    rng = np.random.default_rng(77)
    out = []
    for t, (alen, blen) in enumerate(itertools.product(LENGTHS, LENGTHS)):
        a, b = P.ACGT[rng.integers(0, 4, alen)].copy(), P.ACGT[rng.integers(0, 4, blen)].copy()
        if min(alen, blen) >= 3:
            ov = int(rng.integers(3, min(alen, blen) + 1))
            b[:ov] = a[alen - ov:]
            if t % 3 == 0:
                b[int(rng.integers(0, ov))] = P.ACGT[int(rng.integers(0, 4))]
        out.append((a.tobytes(), b.tobytes(), rng.integers(2, 42, alen).astype(np.uint8), rng.integers(2, 42, blen).astype(np.uint8)))
    q = lambda n, v=30: np.full(n, v, np.uint8)       # noqa: E731
    out += [(b"ACGTACGTAC", b"GTACGTACGT", q(10), q(10)),                        # 20 - 5 < 26: no insert to test
            (b"N" * 90, b"N" * 70, q(90, 2), q(70, 2)), (b"N" * 40, b"ACGT" * 10, q(40), q(40)),          # all-N mates
            (b"A" * 100, b"A" * 100, q(100), q(100)), (b"A" * 7, b"A" * 150, q(7), q(150)), (b"C" * 40, b"C" * 33, q(40, 12), q(33, 9)),
            (b"AC" * 60, b"AC" * 50, q(120), q(100)),                             # homopolymers and a dinucleotide repeat
            (b"T" * 30 + b"A" * 6, b"A" * 6 + b"G" * 30, q(36), q(36)),           # a clean overlap of 6: good between the two minima
            (b"T" * 30 + b"A" * 7, b"A" * 7 + b"G" * 30, q(37), q(37))]
    body = P.ACGT[rng.integers(0, 4, 130)].tobytes()
    for v in (0, 70, 1, 69):                                                     # qualities at the ends of probCorrect
        out.append((b"GG" + body, body + b"TT", q(132, v), q(132, 41)))
        out.append((b"GG" + body, body + b"TT", np.where(np.arange(132) % 2, v, 70 - v).astype(np.uint8), q(132, v)))
    # The homopolymers above leave findBestRatio through `bad == 0 && good > minOverlap0 && good < minOverlap` at its first insert
    # (8 columns, good 7.6).  For the main loop's copy of that return findBestRatio has to succeed first: a mate against itself
    # (insert = its length) whose last 6 or 7 bases equal its first, so that the main loop meets a clean overlap of 6 or 7 columns
    # (good 5.7 or 6.65) among its first inserts, which findBestRatio never tests.
    for end in (b"ACGTCA", b"ACGTCAG"):
        whole = end + P.ACGT[rng.integers(0, 4, 88)].tobytes() + end
        out.append((whole, whole, q(len(whole), 38), q(len(whole), 38)))
    return out


@pytest.mark.parametrize("name", ["defaults", "quality-only", "quality-then-flat"])
def test_borders(name):
    pairs = border_pairs()
    r1, r2, bases, quality = M.pack_pairs(*P.hand_over(pairs))
    exp = P.expected_records(pairs, P.CONFIGS[name])
    got = device_overlap(r1, r2, bases, quality, P.config(P.CONFIGS[name]))
    assert_records(got, exp)
    assert_records(M.overlap_batch(r1, r2, bases, quality, P.config(P.CONFIGS[name])), exp)
    assert (exp["insert"] > 0).sum() > 30 and ((exp["ambig"] == 1) & (exp["insert"] < 0)).sum() >= 3
    info = int(exp["info"][-1])
    assert exp[-2:].tolist() == [(-1, 100, 1, info), (-1, 102, 1, info)]     # the main loop's early return, bestBad still min(alen, blen)


@pytest.mark.parametrize("use_quality", [0, 1])
def test_known_answers_derived_by_hand(use_quality):
    a, bs = b"AAAACGGCAC", [b"CGGCACTTTT", b"CGTCACTTTT", b"TTTTTTTTTT"]
    q40 = np.full(10, 40, np.uint8)
    r1, r2, bases, quality = M.pack_pairs([a] * 3, [P.revcomp(b) for b in bs], [q40] * 3, [q40] * 3)
    got = device_overlap(r1, r2, bases, quality, P.config(HAND + (use_quality, 0)))
    info = M.INFO_QUALITY if use_quality else M.INFO_FLAT
    assert got.tolist() == [(14, 0, 0, info), (14, 1, 0, info), (-1, 10, 0, info)]


def test_a_pair_outside_the_limits_is_reported_and_its_neighbours_are_not_disturbed():
    pairs = P.make_pairs(4, 3)
    s1, s2, q1, q2 = P.hand_over(pairs)
    s1b, q1b = [s1[0], b"ACGT" * 128 + b"A", s1[1], s1[2], s1[3]], [q1[0], np.full(513, 30, np.uint8), q1[1], q1[2].copy(), q1[3]]
    s2b, q2b = [s2[0], s2[0], s2[1], s2[2], s2[3]], [q2[0], q2[0], q2[1], q2[2], q2[3]]
    q1b[3][5] = 71
    packed = M.pack_pairs(s1b, s2b, q1b, q2b)
    got = device_overlap(*packed, P.config(P.CONFIGS["quality-then-flat"]))
    exp = P.expected_records(pairs, P.CONFIGS["quality-then-flat"])
    assert got[[0, 2, 4]].tolist() == exp[[0, 1, 3]].tolist()
    assert got[[1, 3]].tolist() == [(-1, 0, 0, M.INFO_SKIPPED)] * 2
    assert_records(got, M.overlap_batch(*packed, P.config(P.CONFIGS["quality-then-flat"])))
    assert_records(device_overlap(*packed, P.config(P.CONFIGS["defaults"])), M.overlap_batch(*packed, P.config(P.CONFIGS["defaults"])))


def test_without_qualities_the_flat_form_runs_whatever_the_flags():
    pairs, (r1, r2, bases, quality) = P.problem_set()
    got = device_overlap(r1[:300], r2[:300], bases, None, P.config(P.CONFIGS["quality-only"]))
    assert_records(got, P.expected_for("defaults")[:300])


def test_on_a_stream_of_its_own():
    pairs, (r1, r2, bases, quality) = P.problem_set()
    d = [_dev(x) for x in (r1[:500], r2[:500], bases, quality)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        recs = M.overlap_batch_device(*d, P.config(P.CONFIGS["quality-then-flat"]))
    s.synchronize()
    assert_records(recs.cpu().numpy().view(M.REC_DTYPE), P.expected_for("quality-then-flat")[:500])


# ------------------------------------------------------------------------------------------------ join
def device_join(r1, r2, bases, quality, ins, cfg=None):
    """(merged, out_bases, out_quality, bytes written outside the joined ranges): the buffers start as a sentinel"""
    merged, total = M.slots_for(r1, r2)
    dm = _dev(merged)
    ob = torch.full((max(1, total),), 0xA5, dtype=torch.uint8, device=DEV)
    oq = None if quality is None else torch.full((max(1, total),), 0xA5, dtype=torch.uint8, device=DEV)
    M.join_batch_device(_dev(r1), _dev(r2), _dev(bases), None if quality is None else _dev(quality), torch.from_numpy(ins).to(DEV), dm, ob, oq, cfg)
    merged = dm.cpu().numpy().view(READ_DTYPE)
    ob, oq = ob.cpu().numpy(), None if oq is None else oq.cpu().numpy()
    written = np.zeros(len(ob), bool)
    for off, ln in zip(merged["bases_off"], merged["len"]):
        written[off:off + ln] = True
    stray = int((ob[~written] != 0xA5).sum()) + (0 if oq is None else int((oq[~written] != 0xA5).sum()))
    return merged, ob, oq, stray


@pytest.mark.parametrize("with_quality, maxq", [(True, 41), (True, 30), (False, 41)])
def test_device_join_equals_the_host_join_and_the_restatement(with_quality, maxq):
    n = 1200
    pairs, ins = join_inserts(n)
    r1, r2, bases, quality = P.problem_set()[1]
    quality = quality if with_quality else None
    cfg = M.default_config(maxMergeQuality=maxq)
    merged, ob, oq, stray = device_join(r1[:n], r2[:n], bases, quality, ins, cfg)
    assert stray == 0
    hm, hb, hq = M.join_batch(r1[:n], r2[:n], bases, quality, ins, cfg=cfg)
    assert (merged == hm).all()
    for i in range(n):
        assert (slot(merged, ob, i) == slot(hm, hb, i)).all() and (not with_quality or (slot(merged, oq, i) == slot(hm, hq, i)).all()), i
    check_joins(pairs, ins, with_quality, merged, ob, oq, maxq)


def test_device_join_of_pairs_written_out_by_hand():
    """the pairs of tests/test_merge_cpu.py::test_host_join_of_pairs_written_out_by_hand, whose docstring derives them"""
    (r1, r2, bases, quality), ins = hand_join_inputs()
    merged, ob, oq, stray = device_join(r1, r2, bases, quality, ins)
    assert stray == 0
    for i, (a, b, qa, qb, insert, eb, eq) in enumerate(HAND_JOINS):
        assert slot(merged, ob, i).tobytes() == eb and slot(merged, oq, i).tolist() == eq, i
    (r1, r2, bases, _), ins = hand_join_inputs_noq()
    merged, ob, oq, stray = device_join(r1, r2, bases, None, ins)
    assert stray == 0 and oq is None
    for i, (a, b, insert, eb) in enumerate(HAND_JOINS_NOQ):
        assert slot(merged, ob, i).tobytes() == eb, i


@pytest.mark.parametrize("n", [0, 1, 5])
def test_device_join_of_few_pairs(n):
    pairs, ins = join_inserts(40)
    r1, r2, bases, quality = P.problem_set()[1]
    merged, ob, oq, stray = device_join(r1[:n], r2[:n], bases, quality, ins[:n])
    assert stray == 0
    check_joins(pairs[:n], ins[:n], True, merged, ob, oq)


# ------------------------------------------------------------------------------------------------ both stages, no oracle
def test_error_free_fragments_come_back_whole():
    """500 fragments of 40..280 bases of a random sequence, read to 100 and to 150 from both ends without errors, qualities 35:
    merge_pairs gives the fragment back for every unambiguous pair that can overlap (tests/test_merge_cpu.py::check_fragments says
    which those are and why), and at least 95 % are unambiguous -- on the host, with records equal to the oracle's, all 500 are
    (test_error_free_fragments_merge_unambiguously_on_the_host)."""
    frs = fragments(500, 8)
    q = [np.full(len(f[1]), 35, np.uint8) for f in frs]
    recs, out = M.merge_pairs([f[1] for f in frs], [f[2] for f in frs], q, q)
    assert (recs["ambig"] == 0).mean() >= 0.95
    check_fragments(frs, recs, [None if o is None else o[0] for o in out])
    for (frag, m1, m2), o in zip(frs, out):
        if o is not None:
            # columns both mates cover carry min(35 + 35 / 4, 41) = 41, the others their read's 35
            both = np.zeros(len(frag), bool)
            both[len(frag) - len(m2):len(m1)] = True
            assert (o[1] == np.where(both, 41, 35)).all()
    # without qualities the same bases come back and no quality array
    recs2, out2 = M.merge_pairs([f[1] for f in frs[:100]], [f[2] for f in frs[:100]])
    assert (recs2 == recs[:100]).all() and [None if o is None else o[0] for o in out2] == [None if o is None else o[0] for o in out[:100]]
    assert all(o is None or o[1] is None for o in out2)
