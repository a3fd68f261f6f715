"""GPU parity test: the rescue-scan kernel (bbpipe_quick_rescue_device) against the CPU oracle."""
import functools

import numpy as np
import pytest

from bbmap_amd.rescue import RESULT_DTYPE, quick_rescue_batch
from oracle.oracle import quick_rescue
from tests.rescue_check import first_divergence
from tests.rescue_problems import make_full_set, make_problems, scanned

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("affine", [True, False])
def test_quick_rescue_matches_oracle(affine):
    ref, probs = make_problems(11, 1500)
    got = quick_rescue_batch(probs, [ref], min_index=[300], use_affine=affine)
    found = 0
    for p, g in zip(probs, got):
        exp = quick_rescue(p[0], ref, 300, p[2], p[3], p[4], p[5], p[6], useAffine=affine)
        assert g == exp, (p[1:], g, exp)
        found += exp is not None
    assert found > 600


# ---------------------------------------------------------------------------------------------------------------
# The edge sets (tests/rescue_problems.py: edge jobs, planted families, degenerate jobs over six chromosomes) through the raw
# bbresc_result records.  Every comparison is exact equality.  Each step launches the kernel once.
#
# What these can and cannot see.  A replay of the survivors out of search order, a stale cap taken for the current one, "<=" in
# the absdif tie, a skipped byte tail and read N = reference N counted as a match each change records of this set (the old set
# of make_problems showed only the last two).  The kernel's `finished` exit is different: once a perfect hit has narrowed the
# range the best score is the read length and the cap is 0, so a start beyond the narrowed bound can only tie on score with a
# larger absdif and is never taken.  Leaving the exit out costs time and changes no record, here or in the Java.
SEED, N_EDGE = 1, 3000                      # the set whose coverage tests/test_oracle_rescue.py counts
FIELDS = RESULT_DTYPE.names
SCORES = {True: dict(points_match=53, points_match2=91, base_hit_score=37),      # keyed by use_affine; none is a default
          False: dict(points_match=61, points_match2=83, base_hit_score=29)}


@functools.lru_cache(maxsize=None)
def _edge_set(affine):
    """(chroms, min_index, probs, families, expected bbresc_result records from the oracle)"""
    chroms, min_index, probs, fams = make_full_set(SEED, N_EDGE)
    exp = np.zeros(len(probs), RESULT_DTYPE)
    for i, p in enumerate(probs):
        b, ch, loc, sd, right, ideal, mam = p
        if len(b) > 600:
            exp[i]["found"] = -2                # declined: longer than the kernel's read buffer
        elif scanned(p):
            s = SCORES[affine]
            r = quick_rescue(b, chroms[ch - 1], min_index[ch - 1], loc, sd, right, ideal, mam, pointsMatch=s["points_match"],
                             pointsMatch2=s["points_match2"], useAffine=affine, baseHitScore=s["base_hit_score"])
            if r is not None:
                exp[i] = (1, r["start"], r["stop"], r["score"], r["mismatches"], r["perfect"], r["semiperfect"], r["contig"])
    return chroms, min_index, probs, fams, exp


def _explain(chroms, min_index, probs, fams, got, exp, order=None):
    """Failure text: the first differing record, with the tracer's account of that job."""
    bad = np.flatnonzero(got != exp)
    i = int(bad[0])
    j = i if order is None else int(order[i])
    b, ch, loc, sd, right, ideal, mam = probs[j]
    g = dict(zip(("start", "stop", "score", "mismatches", "perfect", "semiperfect", "contig"), [int(x) for x in got[i].tolist()[1:]]))
    msg = "%d of %d records differ; first at position %d: job %d, family %s, len %d, %r\ngot %r\nexp %r\n" % (
        len(bad), len(exp), i, j, fams[j], len(b), probs[j][1:], got[i], exp[i])
    if scanned(probs[j]):
        msg += first_divergence(b, chroms[ch - 1], min_index[ch - 1], loc, sd, right, ideal, mam, g if got[i]["found"] == 1 else None)
    return msg


@pytest.mark.parametrize("affine", [True, False])
def test_edge_set_equals_oracle_in_every_field(affine):
    chroms, min_index, probs, fams, exp = _edge_set(affine)
    got = quick_rescue_batch(probs, chroms, min_index=min_index, use_affine=affine, raw=True, prefill=0xA5, **SCORES[affine])
    assert len(got) == len(probs) > 3500 and int((exp["found"] == 1).sum()) > 2000
    assert (got == exp).all(), _explain(chroms, min_index, probs, fams, got, exp)
    for f in FIELDS:                                                       # field by field as well: == on records is all-or-nothing
        assert (got[f] == exp[f]).all(), f


def test_raw_codes_and_untouched_bytes():
    chroms, min_index, probs, fams, exp = _edge_set(True)
    got = quick_rescue_batch(probs, chroms, min_index=min_index, raw=True, prefill=0xA5, spare_records=5, **SCORES[True])
    assert len(got) == len(probs) + 5
    tail, got = got[len(probs):], got[:len(probs)]
    assert (tail.view(np.uint8) == 0xA5).all()                             # nothing is written after record n - 1
    assert set(np.unique(got["found"]).tolist()) == {1, 0, -2}
    too_long = np.array([len(p[0]) > 600 for p in probs])
    assert too_long.sum() >= 4 and ((got["found"] == -2) == too_long).all()
    degenerate = np.array([f == "D" for f in fams])
    assert degenerate.sum() == 16
    for f in FIELDS[1:]:                                                   # written, and as zero: the prefill is gone
        assert (got[f][degenerate] == 0).all(), f
        assert (got[f][got["found"] != 1] == 0).all(), f
    assert (got == exp).all(), _explain(chroms, min_index, probs, fams, got, exp)
    # the dict form keeps hiding the code: both "declined" and "nothing found" are None
    dicts = quick_rescue_batch(probs[:40], chroms, min_index=min_index, **SCORES[True])
    assert [d is not None for d in dicts] == (exp["found"][:40] == 1).tolist()


def test_small_batches_one_to_nine_jobs():
    """n = 1..9: partly filled workgroups of four waves, starting at a stretch that holds degenerate jobs among live ones."""
    chroms, min_index, probs, fams, exp = _edge_set(True)
    at = fams.index("D") - 3
    assert "D" in fams[at:at + 9] and (exp["found"][at:at + 9] == 1).any()
    for n in range(1, 10):
        got = quick_rescue_batch(probs[at:at + n], chroms, min_index=min_index, raw=True, prefill=0xA5, spare_records=2, **SCORES[True])
        assert (got[n:].view(np.uint8) == 0xA5).all(), n
        assert (got[:n] == exp[at:at + n]).all(), (n, _explain(chroms, min_index, probs[at:at + n], fams[at:at + n], got[:n], exp[at:at + n]))


def test_large_shuffled_batch_is_position_independent():
    """The whole set ten times over, each copy at shuffled positions: about 37,000 jobs in one launch.  A job's record must not
    depend on where it stands or on which jobs share its workgroup.  The oracle runs once per distinct job."""
    chroms, min_index, probs, fams, exp = _edge_set(True)
    rng = np.random.default_rng(7)
    order = np.concatenate([rng.permutation(len(probs)) for _ in range(10)])
    got = quick_rescue_batch([probs[i] for i in order], chroms, min_index=min_index, raw=True, prefill=0xA5, **SCORES[True])
    assert len(got) == 10 * len(probs) > 35000
    assert (got == exp[order]).all(), _explain(chroms, min_index, probs, fams, got, exp[order], order)


def test_read_offsets_of_every_residue():
    """The read is copied to LDS byte by byte from reads + read_off: every residue of read_off mod 16 must behave like an aligned one."""
    chroms, min_index, probs, fams, exp = _edge_set(True)
    probs, fams, exp = probs[:1600], fams[:1600], exp[:1600]
    for aligned in (True, False):
        gaps, pos = [], 0
        for i, p in enumerate(probs):
            want = 0 if aligned else (1 + i + i // 16) % 16             # every residue, in every position of the workgroup
            gaps.append((want - pos) % 16)
            pos += gaps[-1] + len(p[0])
        offs = np.cumsum([g + len(p[0]) for g, p in zip(gaps, probs)]) - [len(p[0]) for p in probs]
        assert set((offs % 16).tolist()) == ({0} if aligned else set(range(16)))
        got = quick_rescue_batch(probs, chroms, min_index=min_index, raw=True, prefill=0xA5, read_gaps=gaps, **SCORES[True])
        assert (got == exp).all(), (aligned, _explain(chroms, min_index, probs, fams, got, exp))
