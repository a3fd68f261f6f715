"""Shared inputs and expected overlap records of the merge tests (tests/test_merge_cpu.py, tests/test_merge_gpu.py).

Pairs: `a` and `b` are made in overlap orientation and mate 2 is handed over as revcomp(b).  Lengths are uniform in 20..160 for each
mate, independently.  Of every 6 pairs, 4 have b[:ov] = a[alen-ov:] with ov uniform in 4..min(alen, blen) and up to 0, 2, 7 and 19
random substitutions inside the overlap (one limit each), 1 is a pair of repeats of a random unit of 1..4 bases (the ambiguous
class), 1 is unrelated random sequence.  Every seventh pair has one N in each mate.  Qualities are uniform in 2..41.

Expected records come from the oracle (oracle/bbmerge_oracle.c: orc_bbmerge_mate_by_overlap_ratio and _ratio_q) under the composition
of BBMerge.mateByOverlap_ratioMode (current/jgi/BBMerge.java:1615-1639), written out in expected_records()."""
import ctypes as C
import functools

import numpy as np

from bbmap_amd import merge as M

ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = np.zeros(256, np.uint8)
for _x, _y in zip(b"ACGTN", b"TGCAN"):
    _COMP[_x] = _y
N_PAIRS = 4000
SUB_LIMITS = (0, 2, 7, 19)

# (minOverlap0, minOverlap, minInsert0, minInsert, maxRatio, ratioMargin, ratioOffset, gIncr, bIncr, useQuality, withoutQuality)
CONFIGS = {
    "defaults": (5, 8, 26, 35, 0.09, 5.5, 0.55, 0.95, 0.95, 0, 1),
    "quality-only": (5, 8, 26, 35, 0.09, 5.5, 0.55, 0.95, 0.95, 1, 0),
    "quality-then-flat": (5, 8, 26, 35, 0.09, 5.5, 0.55, 0.95, 0.95, 1, 1),
    "shim-numbers": (8, 12, 35, 35, 0.075, 2.0, 0.55, 0.65, 0.95, 0, 1),
}


def config(values, **kw):
    names = ("minOverlap0", "minOverlap", "minInsert0", "minInsert", "maxRatio", "ratioMargin", "ratioOffset", "gIncr", "bIncr", "useQuality",
             "withoutQuality")
    return M.default_config(**dict(zip(names, values), **kw))


def revcomp(s):
    return _COMP[np.frombuffer(bytes(s), np.uint8)][::-1].tobytes()


def make_pairs(n, seed):
    """[(a, b, qa, qb)]: bytes in overlap orientation and uint8 qualities, by the recipe above"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        alen, blen = int(rng.integers(20, 161)), int(rng.integers(20, 161))
        kind = t % 6
        if kind == 4:
            unit = ACGT[rng.integers(0, 4, int(rng.integers(1, 5)))]
            a = np.resize(unit, alen).copy()
            b = np.resize(unit, blen).copy()
        else:
            a, b = ACGT[rng.integers(0, 4, alen)].copy(), ACGT[rng.integers(0, 4, blen)].copy()
            if kind < 4:
                ov = int(rng.integers(4, min(alen, blen) + 1))
                b[:ov] = a[alen - ov:]
                for _ in range(int(rng.integers(0, SUB_LIMITS[kind] + 1))):
                    b[int(rng.integers(0, ov))] = ACGT[int(rng.integers(0, 4))]
        if t % 7 == 0:
            a[int(rng.integers(0, alen))] = ord("N")
            b[int(rng.integers(0, blen))] = ord("N")
        out.append((a.tobytes(), b.tobytes(), rng.integers(2, 42, alen).astype(np.uint8), rng.integers(2, 42, blen).astype(np.uint8)))
    return out


def hand_over(pairs):
    """(seqs1, seqs2, quals1, quals2) as a caller holds them: mate 2 as it was sequenced, its qualities in that order"""
    return ([p[0] for p in pairs], [revcomp(p[1]) for p in pairs], [p[2] for p in pairs], [p[3][::-1].copy() for p in pairs])


@functools.lru_cache(maxsize=None)
def problem_set():
    """The 4,000 pairs, made once: (pairs in overlap orientation, pack_pairs' output for them as handed over)"""
    pairs = make_pairs(N_PAIRS, 20261020)
    return pairs, M.pack_pairs(*hand_over(pairs))


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import lib
    O = lib()
    i8, f32, i32 = C.POINTER(C.c_int8), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    O.orc_bbmerge_mate_by_overlap_ratio.argtypes = [i8, C.c_int, i8, C.c_int, i32, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_float] * 5
    O.orc_bbmerge_mate_by_overlap_ratio_q.argtypes = [i8, C.c_int, i8, C.c_int, i8, i8, f32, f32, i32, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_float] * 3
    return O, i8, f32, i32


def oracle_flat(a, b, values):
    """(x, rvector[2], rvector[4]) of the flat native for a, b in overlap orientation"""
    O, i8, f32, i32 = _oracle()
    mo0, mo, mi0, mi, maxr, margin, off, g, bd = values[:9]
    aa, bb = np.frombuffer(a + b"\0", np.int8).copy(), np.frombuffer(b + b"\0", np.int8).copy()
    rv = np.zeros(5, np.int32)
    x = O.orc_bbmerge_mate_by_overlap_ratio(aa.ctypes.data_as(i8), len(a), bb.ctypes.data_as(i8), len(b), rv.ctypes.data_as(i32), mo0, mo, mi0, mi,
                                            maxr, margin, off, g, bd)
    return x, int(rv[2]), int(rv[4])


def oracle_quality(a, b, qa, qb, values):
    O, i8, f32, i32 = _oracle()
    mo0, mo, mi0, mi, maxr, margin, off = values[:7]
    aa, bb = np.frombuffer(a + b"\0", np.int8).copy(), np.frombuffer(b + b"\0", np.int8).copy()
    qa, qb = np.append(qa, 0).astype(np.int8), np.append(qb, 0).astype(np.int8)
    ap, bp = np.zeros(len(a) + 1, np.float32), np.zeros(len(b) + 1, np.float32)
    rv = np.zeros(5, np.int32)
    x = O.orc_bbmerge_mate_by_overlap_ratio_q(aa.ctypes.data_as(i8), len(a), bb.ctypes.data_as(i8), len(b), qa.ctypes.data_as(i8), qb.ctypes.data_as(i8),
                                              ap.ctypes.data_as(f32), bp.ctypes.data_as(f32), rv.ctypes.data_as(i32), mo0, mo, mi0, mi, maxr, margin, off)
    return x, int(rv[2]), int(rv[4])


def expected_record(a, b, qa, qb, values):
    """BBMerge.mateByOverlap_ratioMode (BBMerge.java:1619-1638) around the oracle's two natives; qa is None for a pair without qualities"""
    use_quality, without_quality = values[9], values[10]
    x, bad, ambig, info = -1, 0, 0, 0                                  # int x=-1; rvector[4]=0
    overlapped = False
    if use_quality and qa is not None and qb is not None:
        overlapped = True
        x, bad, ambig = oracle_quality(a, b, qa, qb, values)
        info |= M.INFO_QUALITY
    if not overlapped or (without_quality and (x < 0 or ambig == 1)):
        x, bad, ambig = oracle_flat(a, b, values)
        info |= M.INFO_FLAT
    return x, bad, ambig, info


def expected_records(pairs, values, with_quality=True):
    out = np.zeros(len(pairs), M.REC_DTYPE)
    for i, (a, b, qa, qb) in enumerate(pairs):
        out[i] = expected_record(a, b, qa if with_quality else None, qb if with_quality else None, values)
    return out


@functools.lru_cache(maxsize=None)
def expected_for(name):
    """the oracle's records of the problem set under CONFIGS[name], computed once"""
    out = expected_records(problem_set()[0], CONFIGS[name])
    out.setflags(write=False)
    return out


def classes(recs):
    """(merged unambiguous, merged ambiguous, none unambiguous, none ambiguous) counts of a record array"""
    merged, ambig = recs["insert"] > 0, recs["ambig"] == 1
    return int((merged & ~ambig).sum()), int((merged & ambig).sum()), int((~merged & ~ambig).sum()), int((~merged & ambig).sum())
