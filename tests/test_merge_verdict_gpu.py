"""BBMerge's verdict on the device: bbmerge_verdict_batch_device against the host form on the whole problem set under every
configuration (tests/test_merge_verdict_cpu.py holds the host form against the restatement on the same set), against the restatement
itself on a slice of every class and on the border cases, the counters, and merge_pairs(verdict=) on error-free fragments.  Whole
records are compared, the filters' floats by their bits."""
import itertools

import numpy as np
import pytest
import torch

from bbmap_amd import merge as M
from tests import merge_problems as P
from tests import merge_verdict_check as K
from tests import merge_verdict_problems as V
from tests.test_merge_cpu import fragments
from tests.test_merge_verdict_cpu import HOST_CONFIGS

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def device_verdict(r1, r2, bases, quality, cfg, stats=None):
    recs = M.verdict_batch_device(_dev(r1), _dev(r2), _dev(bases), None if quality is None else _dev(quality), cfg, stats)
    return recs.cpu().numpy().view(M.VERDICT_DTYPE)


def assert_records(got, exp):
    diff = K.differing(got, exp)
    assert diff.size == 0, (diff[:5], got[diff[:5]], exp[diff[:5]])


SLICE = 600          # 30 pairs of each of the 20 classes


@pytest.mark.parametrize("name", HOST_CONFIGS)
def test_device_equals_host_equals_restatement(name):
    batch, cfg = V.batch(name), V.config(name)
    got = device_verdict(*batch, cfg)
    assert_records(got, M.verdict_batch(*batch, cfg=cfg))
    assert_records(got[:SLICE], K.verdicts(V.problem_set()[0][:SLICE], cfg, with_quality=V.CONFIGS[name][1]))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 0])
def test_pair_counts(n):
    """around the wavefront's width, and none"""
    r1, r2, bases, quality = V.batch("xstrict")
    cfg = V.config("xstrict")
    stats = M.new_stats_device(DEV)
    got = device_verdict(r1[:n], r2[:n], bases, quality, cfg, stats)
    exp = M.verdict_batch(r1[:n], r2[:n], bases, quality, cfg=cfg)
    assert got.shape == (n,)
    assert_records(got, exp)
    assert stats.cpu().numpy().tobytes() == K.recount(exp).tobytes()


# ------------------------------------------------------------------------------------------------ borders
LENGTHS = (0, 1, 2, 3, 11, 12, 191, 192, 193, 512)
BORDER_CONFIGS = {
    "defaults": lambda: M.default_verdict_config(),
    "xstrict": lambda: M.verdict_from_flags("xstrict"),
    "both-modes-qualiters-4-margin-0": lambda: M.default_verdict_config(useNormalMode=1, qualIters=4, margin=0),
    "normal-only-qualiters-1": lambda: M.verdict_from_flags(ratiomode="f", normalmode="t", qualiters=1),
    "usequality=f-both-modes": lambda: M.default_verdict_config(useQuality=0, useNormalMode=1),
    "quality-forms-no-filters": lambda: M.default_verdict_config(useEfilter=0, pfilterRatio=0.0, useNormalMode=1, overlapUsingQuality=1),
    "k5-score-200": lambda: M.default_verdict_config(entropyK=5, minEntropyScore=200, useNormalMode=1),
}


def border_pairs():
    """Every combination of LENGTHS (around entropyK, around minOverlap, around the 192 of the short kernel class, the limit): b
    continues a's tail where both are long enough, with a few substitutions in every third pair; a 513-base mate between ordinary
    pairs; then the special contents."""
    rng = np.random.default_rng(78)
    q = lambda n, v=30: np.full(n, v, np.uint8)       # noqa: E731
    out = []
    for t, (alen, blen) in enumerate(itertools.product(LENGTHS, LENGTHS)):
        a, b = P.ACGT[rng.integers(0, 4, alen)].copy(), P.ACGT[rng.integers(0, 4, blen)].copy()
        if min(alen, blen) >= 3:
            ov = int(rng.integers(3, min(alen, blen) + 1))
            b[:ov] = a[alen - ov:]
            if t % 3 == 0:
                for _ in range(int(rng.integers(1, 4))):
                    b[int(rng.integers(0, ov))] = P.ACGT[int(rng.integers(0, 4))]
        out.append((a.tobytes(), b.tobytes(), rng.integers(2, 42, alen).astype(np.uint8), rng.integers(2, 42, blen).astype(np.uint8)))
        if t % 25 == 7:
            out.append((P.ACGT[rng.integers(0, 4, 513)].tobytes(), b.tobytes(), q(513), q(blen)))          # skipped
    # entropy: the score reached exactly at the last base, and one base short of it (never reached: len + 1), for each scan
    whole = P.ACGT[rng.integers(0, 4, 150)].tobytes()
    other = whole[-40:] + P.ACGT[rng.integers(0, 4, 110)].tobytes()
    # (over two letters, so that the score comes late and this scan's answer is the pair's minOverlap)
    low = np.frombuffer(b"AG", np.uint8)[rng.integers(0, 2, 150)].tobytes()
    at_b = K.calc_min_overlap_by_entropy_head(low, 3, 39)
    at_a = K.calc_min_overlap_by_entropy_tail(low, 3, 39)
    assert 16 < at_b < 149 and 16 < at_a < 149
    for a, b in ((whole, low[:at_b + 1]), (whole, low[:at_b]), (low[-(at_a + 1):], other), (low[-at_a:], other)):
        out.append((a, b, q(len(a)), q(len(b))))
    out += [(b"N" * 90, b"N" * 70, q(90, 2), q(70, 2)), (b"N" * 40, b"ACGT" * 10, q(40), q(40)),          # all-N mates
            (b"A" * 100, b"A" * 100, q(100), q(100)), (b"AC" * 60, b"AC" * 50, q(120), q(100)),
            (whole[:60] + b"N" * 30 + whole[90:], other[:20] + b"NN" + other[22:], q(150), q(150))]        # N runs reset the k-mer
    body = P.ACGT[rng.integers(0, 4, 130)].tobytes()
    wrong = bytearray(body)
    wrong[40], wrong[90] = wrong[41], wrong[91]
    for v in (0, 1, 2, 59, 60, 70):                  # at or below minprob; the ends of probCorrect2 and of probCorrect
        out.append((b"GG" + body, body + b"TT", q(132, v), q(132, 41)))
        out.append((b"GG" + body, bytes(wrong) + b"TT", np.where(np.arange(132) % 2, v, 41).astype(np.uint8), q(132, v)))
    big = P.ACGT[rng.integers(0, 4, 994)].tobytes()                              # the largest inserts 512-base mates give
    out.append((big[:512], big[-512:], q(512, 35), q(512, 35)))
    return out


def expected_borders(pairs, cfg, with_quality=True):
    """the restatement's records, and the skipped record where the documented rule skips a pair (include/bbmap_amd.h)"""
    have_quality = bool(cfg.useQuality) and with_quality
    prob_read = have_quality and ((cfg.useRatioMode and cfg.ratio.useQuality) or cfg.useNormalMode)
    filtered = have_quality and (cfg.useEfilter or cfg.pfilterRatio > 0)
    out = np.zeros(len(pairs), M.VERDICT_DTYPE)
    for i, (a, b, qa, qb) in enumerate(pairs):
        top = max([0] + list(qa) + list(qb))
        if max(len(a), len(b)) > M.MAX_READ_LEN or (prob_read and top > 70) or (filtered and top > 59):
            out[i] = (-1, 0, -1, 0, 0, -1, 99999, 0, 0, 0.0, 0.0, M.INFO_SKIPPED)
        else:
            out[i] = K.verdicts([(a, b, qa, qb)], cfg, with_quality=with_quality)[0]
    return out


@pytest.mark.parametrize("name", sorted(BORDER_CONFIGS))
def test_borders(name):
    pairs = border_pairs()
    cfg = BORDER_CONFIGS[name]()
    r1, r2, bases, quality = M.pack_pairs(*P.hand_over(pairs))
    exp = expected_borders(pairs, cfg)
    got = device_verdict(r1, r2, bases, quality, cfg)
    assert_records(got, exp)
    assert_records(M.verdict_batch(r1, r2, bases, quality, cfg=cfg), exp)
    skipped = (exp["info"] & M.INFO_SKIPPED) != 0
    n513 = sum(len(p[0]) == 513 for p in pairs)
    if name == "defaults":
        assert n513 == 4 and skipped.sum() == n513 + 4                      # and the four pairs with a quality of 60 or 70
        k = len(pairs) - 12 - 1 - 5 - 4                                     # the four entropy pairs
        lens = [(len(p[0]), len(p[1])) for p in pairs[k:k + 4]]
        assert exp["minOverlap"][k:k + 4].tolist() == [lens[0][1] - 1, lens[1][1] + 1, lens[2][0] - 1, lens[3][0] + 1]
        assert exp["code"][-1] == 994 and (exp["code"] > 0).sum() > 20
    else:
        assert skipped.sum() == n513 + (0 if name in ("usequality=f-both-modes", "quality-forms-no-filters") else 4)
    if name == "quality-forms-no-filters":                                  # 60 and 70 are evaluated through probCorrect
        assert (exp["info"][-13:-1] & M.INFO_QUALITY != 0).all()


def test_borders_without_a_quality_array_and_on_another_stream():
    pairs = border_pairs()
    cfg = M.default_verdict_config(useNormalMode=1)
    r1, r2, bases, _ = M.pack_pairs(*P.hand_over(pairs))
    exp = expected_borders(pairs, cfg, with_quality=False)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = M.verdict_batch_device(_dev(r1), _dev(r2), _dev(bases), None, cfg)
    stream.synchronize()
    assert_records(got.cpu().numpy().view(M.VERDICT_DTYPE), exp)


# ------------------------------------------------------------------------------------------------ counters
def test_stats_accumulate_over_two_calls_and_null_stats_is_allowed():
    """hist[1999] takes every insert of 1999 or more, but with BBMERGE_MAX_READ_LEN = 512 no insert can exceed 512 + 512 - 4, so that
    slot is unreachable and stays 0; the largest inserts the limit allows (994 here) land in their own slot."""
    pairs = border_pairs()
    cfg = M.default_verdict_config()
    border = M.pack_pairs(*P.hand_over(pairs))
    stats = M.new_stats_device(DEV)
    first = device_verdict(*V.batch("defaults"), cfg, stats)
    second = device_verdict(*border, cfg, stats)
    got = stats.cpu().numpy().view(M.STATS_DTYPE)
    exp = K.recount(np.concatenate([first, second]))
    assert got.tobytes() == exp.tobytes()
    assert got["hist"][0][994] == 1 and got["hist"][0][1999] == 0 and got["insertMax"][0] == 994 and got["skipped"][0] == 8
    assert got["pairs"][0] == len(first) + len(second) == sum(got[k][0] for k in ("merged", "ambiguous", "tooShort", "tooLong", "noSolution", "skipped"))
    assert_records(device_verdict(*border, cfg, None), second)


# ------------------------------------------------------------------------------------------------ merge_pairs
def test_merge_pairs_with_a_verdict_returns_error_free_fragments():
    """An error-free pair has bad = 0, passes efilter and has probability 1.  It merges where the overlap has at least the pair's
    own minOverlap columns (then 0.95 * columns >= minOverlap - 3) and the fragment has minInsert (35) bases or more."""
    frs = fragments(300, 9)
    q = [np.full(len(f[1]), 35, np.uint8) for f in frs]
    recs, out = M.merge_pairs([f[1] for f in frs], [f[2] for f in frs], q, q, verdict=M.default_verdict_config())
    assert recs.dtype == M.VERDICT_DTYPE
    eligible = 0
    for i, (frag, m1, m2) in enumerate(frs):
        if len(m1) + len(m2) - len(frag) >= recs["minOverlap"][i] and len(frag) >= 35:
            eligible += 1
            assert recs["code"][i] == len(frag) and out[i] is not None and out[i][0] == frag, i
        assert (out[i] is None) == (recs["code"][i] <= 0), i
        if out[i] is not None:
            assert out[i][0] == frag and len(out[i][1]) == len(frag), i
    assert eligible >= 200 and eligible < len(frs)
    # the default rule and its records are what they were
    recs0, out0 = M.merge_pairs([f[1] for f in frs], [f[2] for f in frs], q, q)
    assert recs0.dtype == M.REC_DTYPE and sum(o is not None for o in out0) >= eligible
