"""Shared inputs of the verdict tests (tests/test_merge_verdict_cpu.py, tests/test_merge_verdict_gpu.py) and their expected records.

3,000 pairs, seeded, made in overlap orientation like tests/merge_problems.py (mate 2 is handed over as revcomp(b)).  Pair t is of
class t % 20:
  0-5   a fragment read from both ends, mates 60..160 (0-2: the same length, 3: mate 2 the shorter by up to 90, 4: mate 1 the
        shorter, 5: 100..250 each), with sequencing errors drawn from REALISTIC qualities (38 falling to about 12 along the read, an
        error where 10^(-q/10) says so) and 0..6 further substitutions in the overlap at a random place;
  6     the same with HOSTILE qualities: every base 36..41, and 1..4 substitutions in the overlap (efilter's case: the expected
        number of mismatches is far below the count);
  7     flat qualities 17..22 and 4..8 substitutions in an overlap of 100..150 (pfilter's case: efilter expects that many, the
        product of their probabilities is tiny);
  8     too short.  findBestRatio only looks at inserts of minInsert (35) and more, so an insert below it is returned only where a
        longer one has a ratio within maxRatio, and unambiguously only where 5.5 times its own ratio lies below that one.  The one
        solution: insert 34 without a mismatch (0.55 / 34 = 0.01618, times 5.5 = 0.08897) beside insert 38 with three (3.4 / 38 =
        0.08947 < 0.09), mates of 68 or more (margin2 = 6.05 / minLength below 0.08947).  Built as a 34-base fragment of period 4 with
        one substitution inside and one near its end, so that the shifts by 4 (inserts 38, 30, 26) all carry the three mismatches;
  9-10  unrelated mates (no solution);
  11    both mates a repeat of one unit of 1..3 bases (ambiguous; the entropy scan never reaches the score: len + 1);
  12-14 a fragment whose overlap lies in low-complexity sequence: the last 45..80 bases of mate 1 and the first of b are random over
        two letters (eight 3-mers: the score of 39 needs all of them once and seven twice, some 30..45 bases), overlap 12..40, no
        errors.  The alignment is unique, so the pair merges with minOverlap 11, and where the entropy result exceeds the overlap it
        does not (a verdict that useEntropy=0 turns);
  15    as 0 with a run of 3..30 N in each mate (the N resets the k-mer);
  16    mates of 300..420 with an overlap of at least 260, qualities 14..19 and 23..30 substitutions (more than maxMismatchesR bad
        at a ratio the search accepts; the long kernel class);
  17    as 0 with 2..4 substitutions at good quality in a long overlap (the ratio mode accepts, the strict normal mode does not);
  18    as 0, fragments longer than 200 from mates of 120..160 (too long once maxLength is 200);
  19    short mates of 12..40 with a planted overlap of 8..len.
Expected records come from tests/merge_verdict_check.py."""
import functools

import numpy as np

from bbmap_amd import merge as M
from tests import merge_problems as P
from tests import merge_verdict_check as K

ACGT = P.ACGT
N_PAIRS = 3000
SEED = 20261021


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _realistic(rng, n):
    """qualities that start near 38 and fall towards the end, with noise, 2..41"""
    slope = rng.uniform(0.05, 0.25)
    q = 38 - slope * np.arange(n) * (150.0 / max(n, 150)) + rng.normal(0, 3, n)
    q[rng.random(n) < 0.03] = 2
    return np.clip(np.rint(q), 2, 41).astype(np.uint8)


def _mutate(rng, s, at):
    s[at] = ACGT[(int(np.flatnonzero(ACGT == s[at])[0]) + int(rng.integers(1, 4))) % 4] if s[at] in ACGT else ACGT[0]


def _sequencing_errors(rng, s, q):
    for i in np.flatnonzero(rng.random(len(s)) < 10.0 ** (-q.astype(np.float64) / 10)):
        _mutate(rng, s, int(i))


def _fragment(rng, alen, blen, insert):
    """(a, b) in overlap orientation: the two ends of a random fragment of `insert` bases, read alen and blen deep (into random
    sequence past the fragment's end where a mate is longer than it)"""
    frag = _rand(rng, insert)
    a = np.concatenate([frag, _rand(rng, max(0, alen - insert))])[:alen]
    b = np.concatenate([_rand(rng, max(0, blen - insert)), frag])[-blen:]
    return a, b


def _overlap_columns(alen, blen, insert):
    """(i in a, j in b) of the columns of the overlap for an insert"""
    istart, jstart = max(0, insert - blen), max(0, blen - insert)
    n = min(alen - istart, blen - jstart, insert)
    return istart, jstart, n


def _substitute_in_overlap(rng, a, b, insert, count):
    istart, jstart, n = _overlap_columns(len(a), len(b), insert)
    for c in rng.choice(n, size=min(count, n), replace=False):
        _mutate(rng, b, jstart + int(c))


def make_pair(rng, t):
    kind = t % 20
    if kind in (0, 1, 2, 3, 4, 5, 15, 17, 18):
        if kind == 5:
            alen, blen = int(rng.integers(100, 251)), int(rng.integers(100, 251))
        elif kind == 18:
            alen, blen = int(rng.integers(120, 161)), int(rng.integers(120, 161))
        else:
            alen = int(rng.integers(60, 161))
            blen = alen
            if kind == 3:
                blen = max(30, alen - int(rng.integers(1, 91)))
            if kind == 4:
                alen, blen = max(30, alen - int(rng.integers(1, 91))), alen
        lo, hi = 36, alen + blen - 6
        if kind == 18:
            lo = 201
        if kind == 17:
            hi = max(lo, alen + blen - 80)
        insert = int(rng.integers(lo, hi + 1))
        a, b = _fragment(rng, alen, blen, insert)
        qa, qb = _realistic(rng, alen), _realistic(rng, blen)[::-1].copy()
        if kind == 17:
            istart, jstart, n = _overlap_columns(alen, blen, insert)
            qa[istart:istart + n] = np.maximum(qa[istart:istart + n], 25)
            qb[jstart:jstart + n] = np.maximum(qb[jstart:jstart + n], 25)
            _substitute_in_overlap(rng, a, b, insert, int(rng.integers(2, 5)))
        else:
            _sequencing_errors(rng, a, qa)
            _sequencing_errors(rng, b, qb)
            _substitute_in_overlap(rng, a, b, insert, int(rng.integers(0, 7)) if rng.random() < 0.4 else 0)
        if kind == 15:
            for s in (a, b):
                n = int(rng.integers(3, 31))
                at = int(rng.integers(0, len(s) - n + 1))
                s[at:at + n] = ord("N")
    elif kind == 6:
        alen = blen = int(rng.integers(60, 161))
        insert = int(rng.integers(40, alen + blen - 20))
        a, b = _fragment(rng, alen, blen, insert)
        qa, qb = rng.integers(36, 42, alen).astype(np.uint8), rng.integers(36, 42, blen).astype(np.uint8)
        _substitute_in_overlap(rng, a, b, insert, int(rng.integers(1, 5)))
    elif kind == 7:
        alen = blen = int(rng.integers(120, 161))
        insert = alen + blen - int(rng.integers(100, min(alen, 150) + 1))
        a, b = _fragment(rng, alen, blen, insert)
        qa, qb = rng.integers(17, 23, alen).astype(np.uint8), rng.integers(17, 23, blen).astype(np.uint8)
        _substitute_in_overlap(rng, a, b, insert, int(rng.integers(4, 9)))
    elif kind == 8:
        alen, blen = int(rng.integers(68, 101)), int(rng.integers(68, 101))
        unit = ACGT[rng.permutation(4)]
        w = np.resize(unit, 38).copy()
        p1 = int(rng.integers(12, 30))
        p2 = int(rng.choice([p for p in range(34, 38) if p % 4 != p1 % 4]))
        _mutate(rng, w, p1)
        _mutate(rng, w, p2)
        a = np.concatenate([w[4:], w[34:], _rand(rng, alen - 38)])
        b = np.concatenate([_rand(rng, blen - 38), w])
        qa, qb = rng.integers(30, 41, alen).astype(np.uint8), rng.integers(30, 41, blen).astype(np.uint8)
    elif kind in (9, 10):
        alen, blen = int(rng.integers(40, 161)), int(rng.integers(40, 161))
        a, b = _rand(rng, alen), _rand(rng, blen)
        qa, qb = _realistic(rng, alen), _realistic(rng, blen)[::-1].copy()
    elif kind == 11:
        alen, blen = int(rng.integers(40, 161)), int(rng.integers(40, 161))
        unit = _rand(rng, int(rng.integers(1, 4)))
        a, b = np.resize(unit, alen).copy(), np.resize(unit, blen).copy()
        qa, qb = _realistic(rng, alen), _realistic(rng, blen)[::-1].copy()
    elif kind in (12, 13, 14):
        alen = blen = int(rng.integers(90, 161))
        ov = int(rng.integers(12, 41))
        insert = alen + blen - ov
        a, b = _fragment(rng, alen, blen, insert)
        run = int(rng.integers(45, 81))
        two = ACGT[rng.permutation(4)[:2]]
        a[alen - run:] = two[rng.integers(0, 2, run)]
        b[:run] = two[rng.integers(0, 2, run)]
        b[:ov] = a[alen - ov:]
        qa, qb = rng.integers(30, 41, alen).astype(np.uint8), rng.integers(30, 41, blen).astype(np.uint8)
    elif kind == 16:
        alen, blen = int(rng.integers(300, 421)), int(rng.integers(300, 421))
        ov = int(rng.integers(260, min(alen, blen) + 1))
        insert = alen + blen - ov
        a, b = _fragment(rng, alen, blen, insert)
        qa, qb = rng.integers(14, 20, alen).astype(np.uint8), rng.integers(14, 20, blen).astype(np.uint8)
        _substitute_in_overlap(rng, a, b, insert, int(rng.integers(23, 31)))
    else:
        alen, blen = int(rng.integers(12, 41)), int(rng.integers(12, 41))
        ov = int(rng.integers(8, min(alen, blen) + 1))
        a, b = _fragment(rng, alen, blen, alen + blen - ov)
        qa, qb = _realistic(rng, alen), _realistic(rng, blen)[::-1].copy()
    return a.tobytes(), b.tobytes(), qa, qb


def make_pairs(n, seed):
    rng = np.random.default_rng(seed)
    return [make_pair(rng, t) for t in range(n)]


@functools.lru_cache(maxsize=None)
def problem_set():
    """(pairs in overlap orientation, pack_pairs' output for them as handed over)"""
    pairs = make_pairs(N_PAIRS, SEED)
    return pairs, M.pack_pairs(*P.hand_over(pairs))


# name -> (the configuration, whether the batch has a quality array)
CONFIGS = {
    "defaults": (lambda: M.default_verdict_config(), True),
    "strict": (lambda: M.verdict_from_flags("strict"), True),
    "xstrict": (lambda: M.verdict_from_flags("xstrict"), True),
    "ustrict": (lambda: M.verdict_from_flags("ustrict"), True),
    "fast": (lambda: M.verdict_from_flags("fast"), True),
    "usequality=f": (lambda: M.default_verdict_config(useQuality=0), True),
    "no-quality-array": (lambda: M.default_verdict_config(), False),
    "entropy=f": (lambda: M.default_verdict_config(useEntropy=0), True),
    "normal-mode-only": (lambda: M.verdict_from_flags(ratiomode="f", normalmode="t"), True),
    "normal-mode-only-no-quality": (lambda: M.verdict_from_flags(ratiomode="f", normalmode="t"), False),
    "efilter=f": (lambda: M.default_verdict_config(useEfilter=0), True),
    "pfilter=f": (lambda: M.default_verdict_config(pfilterRatio=0.0), True),
    "maxmismatchesr=1000000": (lambda: M.default_verdict_config(maxMismatchesR=1000000), True),
    "maxlength=200": (lambda: M.default_verdict_config(maxLength=200), True),
    "quality-forms": (lambda: M.default_verdict_config(overlapUsingQuality=1, useNormalMode=1), True),
}


def config(name):
    return CONFIGS[name][0]()


@functools.lru_cache(maxsize=None)
def expected_for(name):
    """the restatement's records of the problem set under CONFIGS[name], computed once"""
    out = K.verdicts(problem_set()[0], config(name), with_quality=CONFIGS[name][1])
    out.setflags(write=False)
    return out


def batch(name):
    """(reads1, reads2, bases, quality or None) of the problem set as CONFIGS[name] takes it"""
    r1, r2, bases, quality = problem_set()[1]
    return r1, r2, bases, quality if CONFIGS[name][1] else None
