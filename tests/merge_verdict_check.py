"""TEST INFRASTRUCTURE ONLY.  BBMerge's verdict for one pair restated statement by statement, with the reference's line numbers at
the right (BBMerge.java = current/jgi/BBMerge.java, Overlapper = current/jgi/BBMergeOverlapper.java): the two entropy scans, the
qualIters loop of mateByOverlap_normalMode, mateByOverlap's composition, both filters and processReadPair_inner's return code.
Nothing of the library's arithmetic is used.  The normal mode's search, with its inner early exit, is tests/merge_verdict_check.cpp
(plain Python is too slow for it); the ratio mode's natives are the oracle's (oracle/bbmerge_oracle.c), called with the pair's own
minOverlap.  `a`, `b` are bytes in overlap orientation (b = mate 2 reverse-complemented), qa / qb uint8 arrays or None; cfg is a
bbmerge_verdict_config, read field by field.  Filters use numpy float32 scalars and a double square root, as the Java does."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

from bbmap_amd import merge as M
from tests import merge_problems as P

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32

RET_NO_SOLUTION, RET_AMBIG, RET_SHORT, RET_LONG = -1, -2, -4, -5                        # BBMerge.java: RET_*

PROB_CORRECT2 = np.array([                                                              # Overlapper:951-956
    0.0000, 0.2501, 0.3690, 0.4988, 0.6019, 0.6838, 0.7488, 0.8005, 0.8415, 0.8741, 0.9000, 0.9206, 0.9369, 0.9499,
    0.9602, 0.9684, 0.9749, 0.9800, 0.9842, 0.9874, 0.9900, 0.9921, 0.9937, 0.9950, 0.9960, 0.9968, 0.9975, 0.9980,
    0.9984, 0.9987, 0.9990, 0.9992, 0.9994, 0.9995, 0.9996, 0.9997, 0.9997, 0.9998, 0.9998, 0.9999, 0.9999, 0.9999,
    0.9999, 0.9999, 0.9999, 0.9999, 0.9999, 0.9999, 0.9999, 0.9999, 0.9999, 0.9999, 0.9999, 0.9999, 0.9999, 0.9999,
    0.9999, 0.9999, 0.9999, 0.9999], np.float32)
assert PROB_CORRECT2.size == 60
BASE_TO_NUMBER = {ord(c): n for n, cs in enumerate(("Aa", "Cc", "Gg", "TtUu")) for c in cs}     # Dedupe.java:5804-5808


@functools.lru_cache(maxsize=None)
def _normal_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="merge_verdict_check_"), "libmerge_verdict_check.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-shared", "-fPIC", "-ffp-contract=off", os.path.join(HERE, "merge_verdict_check.cpp"),
                           "-o", out])
    L = C.CDLL(out)
    i8, f32, i32 = C.POINTER(C.c_int8), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    L.chk_mate_by_overlap_java.argtypes = [i8, C.c_int, i8, C.c_int, i8, i8, f32, f32, i32] + [C.c_int] * 7 + [C.POINTER(C.c_int64)]
    L.chk_mate_by_overlap_java.restype = C.c_int32
    return L, i8, f32, i32


def calc_min_overlap_by_entropy_tail(bases, k, minscore):                               # Overlapper:860
    bits = 2 * k                                                                        # :861
    mask = ~((-1) << bits)                                                              # :862
    kmer = length = ones = twos = 0                                                     # :863
    counts = [0] * (1 << bits)                                                          # :868, :873
    i, j = 0, len(bases) - 1
    while i < len(bases):                                                               # :875
        b = bases[j]                                                                    # :877
        if b not in BASE_TO_NUMBER:                                                     # :878
            length = 0                                                                  # :879
            kmer = 0                                                                    # :880
        else:
            length += 1                                                                 # :882
            n = BASE_TO_NUMBER[b]                                                       # :883
            kmer = ((kmer << 2) | n) & mask                                             # :884
            if length >= k:                                                             # :886
                counts[kmer] += 1                                                       # :887
                if counts[kmer] == 1:                                                   # :888
                    ones += 1
                elif counts[kmer] == 2:                                                 # :889
                    twos += 1
                if ones * 4 + twos >= minscore:                                         # :890
                    return i
        i, j = i + 1, j - 1
    return len(bases) + 1                                                               # :895


def calc_min_overlap_by_entropy_head(bases, k, minscore):                               # Overlapper:898
    bits = 2 * k                                                                        # :899
    mask = ~((-1) << bits)                                                              # :900
    kmer = length = ones = twos = 0                                                     # :901
    counts = [0] * (1 << bits)                                                          # :906, :911
    for i in range(len(bases)):                                                         # :913
        b = bases[i]                                                                    # :915
        if b not in BASE_TO_NUMBER:                                                     # :916
            length = 0                                                                  # :917
            kmer = 0                                                                    # :918
        else:
            length += 1                                                                 # :920
            n = BASE_TO_NUMBER[b]                                                       # :921
            kmer = ((kmer << 2) | n) & mask                                             # :922
            if length >= k:                                                             # :924
                counts[kmer] += 1                                                       # :925
                if counts[kmer] == 1:                                                   # :926
                    ones += 1
                elif counts[kmer] == 2:                                                 # :927
                    twos += 1
                if ones * 4 + twos >= minscore:                                         # :928
                    return i
    return len(bases) + 1                                                               # :933


def calc_min_overlap_from_entropy(a, b, cfg):                                           # BBMerge.java:1696
    if not cfg.useEntropy:                                                              # :1697
        return cfg.minOverlapBases
    x = calc_min_overlap_by_entropy_tail(a, cfg.entropyK, cfg.minEntropyScore)          # :1706
    y = calc_min_overlap_by_entropy_head(b, cfg.entropyK, cfg.minEntropyScore)          # :1707
    return max(cfg.minOverlapBases, max(x, y))                                          # :1708


def _java_byte(x):
    return (int(x) + 128) % 256 - 128


def mate_by_overlap_java(a, b, qa, qb, min_overlap0, min_overlap, min_insert0, margin, max_mismatches0, max_mismatches, minq, columns=None):
    """(x, rvector[2], rvector[4]) of mateByOverlapJava_unrolled, through tests/merge_verdict_check.cpp"""
    L, i8, f32, i32 = _normal_lib()
    aa, bb = np.frombuffer(a + b"\0", np.int8).copy(), np.frombuffer(b + b"\0", np.int8).copy()
    n = max(len(a), len(b)) + 1
    ap, bp = np.zeros(n, np.float32), np.zeros(n, np.float32)
    rv = np.zeros(5, np.int32)
    if qa is None or qb is None:
        pa = pb = None
    else:
        ka, kb = np.append(qa, 0).astype(np.int8), np.append(qb, 0).astype(np.int8)
        pa, pb = ka.ctypes.data_as(i8), kb.ctypes.data_as(i8)
    cols = C.c_int64(0)
    x = L.chk_mate_by_overlap_java(aa.ctypes.data_as(i8), len(a), bb.ctypes.data_as(i8), len(b), pa, pb, ap.ctypes.data_as(f32), bp.ctypes.data_as(f32),
                                   rv.ctypes.data_as(i32), min_overlap0, min_overlap, min_insert0, margin, max_mismatches0, max_mismatches, minq,
                                   C.byref(cols))
    if columns is not None:
        columns.append(cols.value)
    return x, int(rv[2]), int(rv[4])


def mate_by_overlap_normal_mode(a, b, qa, qb, cfg, min_overlap, columns=None):          # BBMerge.java:1641
    ambig_nm = False                                                                    # :1643
    best_insert_nm = -1                                                                 # :1644
    best_bad_nm = 999999                                                                # :1645
    assert cfg.qualIters > 0                                                            # :1647
    max_qual_iters = 1 if qa is None or qb is None else cfg.qualIters                   # :1648
    i = 0
    while i < max_qual_iters and best_insert_nm < 0:                                    # :1651
        x, rv2, rv4 = mate_by_overlap_java(a, b, qa, qb, cfg.minOverlapBases0 - i, min_overlap + i, cfg.ratio.minInsert0, cfg.margin,
                                           cfg.maxMismatches0, cfg.maxMismatches, _java_byte(cfg.minQuality - 2 * i), columns)      # :1653-1654
        if x > -1:                                                                      # :1655
            best_insert_nm = x                                                          # :1656
            best_bad_nm = rv2                                                           # :1657
            ambig_nm = rv4 == 1                                                         # :1658
            break                                                                       # :1659
        i += 1
    # (:1664-1672 `loose` and :1674-1687 trim-on-failure are not built)
    return best_insert_nm, best_bad_nm, 1 if ambig_nm else 0                            # :1690-1693: rvector[0], [2], [4]


def mate_by_overlap_ratio_mode(a, b, qa, qb, cfg, min_overlap):                         # BBMerge.java:1615
    min0 = cfg.minOverlapBases0 - cfg.ratioReduction                                    # :1617
    mn = min_overlap - cfg.ratioReduction                                               # :1618
    r = cfg.ratio
    values = (min0, mn, r.minInsert0, r.minInsert, r.maxRatio, r.ratioMargin, r.ratioOffset, 0.95, 0.95, r.useQuality, r.withoutQuality)
    x, rv2, rv4, info = -1, 0, 0, 0                                                     # :1619-1620 (rvector[2] is set by every native)
    overlapped = False                                                                  # :1626
    if r.useQuality and qa is not None and qb is not None:                              # :1627
        overlapped = True
        x, rv2, rv4 = P.oracle_quality(a, b, qa, qb, values)                            # :1629
        info |= M.INFO_QUALITY
    if not overlapped or (r.withoutQuality and (x < 0 or rv4 == 1)):                    # :1633
        x, rv2, rv4 = P.oracle_flat(a, b, values)                                       # :1634
        info |= M.INFO_FLAT
    return x, rv2, rv4, info


@functools.lru_cache(maxsize=None)
def _filters(a, b, qa, qb, insert):
    """(expectedMismatches, probability) of a pair at an insert; qa, qb as bytes so that the answers are kept per pair and insert"""
    return expected_mismatches(a, b, np.frombuffer(qa, np.uint8), np.frombuffer(qb, np.uint8), insert), \
        probability(a, b, np.frombuffer(qa, np.uint8), np.frombuffer(qb, np.uint8), insert)


def expected_mismatches(a, b, qa, qb, overlap):                                         # Overlapper:667
    alen, blen = len(a), len(b)                                                         # :670
    istart = 0 if overlap <= blen else overlap - blen                                   # :671
    jstart = alen - overlap if overlap <= alen else 0                                   # :672
    expected = F(0)                                                                     # :674
    if qa is None or qb is None:                                                        # :677
        return F((overlap + 0) // 16)
    i, j = istart, jstart
    while i < overlap and i < alen and j < blen:                                        # :699
        ca, cb = a[i], b[j]                                                             # :700
        q1, q2 = qa[i], qb[j]                                                           # :701
        if ca == ord("N") or cb == ord("N"):                                            # :703
            pass
        else:
            prob_c = F(PROB_CORRECT2[q1] * PROB_CORRECT2[q2])                           # :708
            prob_e = F(F(1) - prob_c)                                                   # :709
            expected = F(expected + prob_e)                                             # :711
        i, j = i + 1, j + 1
    return expected                                                                     # :723


def probability(a, b, qa, qb, insert):                                                  # Overlapper:728
    alen, blen = len(a), len(b)                                                         # :730
    istart = 0 if insert <= blen else insert - blen                                     # :731
    jstart = 0 if insert >= blen else blen - insert                                     # :732
    if qa is None or qb is None:                                                        # :734
        return F(1)
    prob_actual = F(1)                                                                  # :736
    prob_common = F(1)                                                                  # :737
    i, j = istart, jstart
    while i < insert and i < alen and j < blen:                                         # :745
        ca, cb = a[i], b[j]                                                             # :746
        q1, q2 = qa[i], qb[j]                                                           # :747
        if ca == ord("N") or cb == ord("N"):                                            # :749
            pass
        else:
            prob_c = F(PROB_CORRECT2[q1] * PROB_CORRECT2[q2])                           # :757
            prob_m = F(prob_c + F(F(F(1) - prob_c) * F(0.25)))                          # :758
            prob_e = F(F(1) - prob_m)                                                   # :759
            prob_common = F(prob_common * max(prob_m, prob_e))                          # :764
            prob_actual = F(prob_actual * (prob_m if ca == cb else prob_e))             # :765
        i, j = i + 1, j + 1
    with np.errstate(all="ignore"):
        q = F(prob_actual / prob_common)                                                # :784, the quotient in float
        r = F(np.sqrt(np.float64(q)))                                                   # Math.sqrt in double, then (float)
    return F(np.nan) if np.isnan(r) else r                                              # (Java has one NaN)


def verdict(a, b, qa, qb, cfg, columns=None):
    """The verdict record of one pair as a dict with VERDICT_DTYPE's fields: BBMerge.mateByOverlap (BBMerge.java:1741-1837) inside
    processReadPair_inner (:2044-2068), after processReadPair has stripped the qualities for useQuality=f (:1913-1916)."""
    if not cfg.useQuality:                                                              # :1914
        qa = qb = None                                                                  # :1915
    info = 0
    expected, prob = F(0), F(0)
    min_overlap = calc_min_overlap_from_entropy(a, b, cfg)                              # :1744
    if cfg.useRatioMode:                                                                # :1767
        best_insert_rm, rv2, rv4, rinfo = mate_by_overlap_ratio_mode(a, b, qa, qb, cfg, min_overlap)      # :1768
        best_bad_rm = rv2                                                               # :1769
        ambig_rm = (rv4 == 1) if best_insert_rm > -1 else False                         # :1770
        info |= rinfo | M.INFO_RATIO
    else:
        best_insert_rm, best_bad_rm, ambig_rm = -1, 0, False                            # :1772-1774
    rrm = bool(cfg.requireRatioMatch)
    if cfg.useNormalMode and ((not rrm and (best_insert_rm < 0 or ambig_rm)) or (rrm and (best_insert_rm > 0 and not ambig_rm))):      # :1779
        best_insert_nm, rv2, rv4 = mate_by_overlap_normal_mode(a, b, qa, qb, cfg, min_overlap, columns)  # :1780
        best_bad_nm = rv2                                                               # :1781
        ambig_nm = (rv4 == 1) if best_insert_nm > -1 else False                         # :1782
        info |= M.INFO_NORMAL
    else:
        ambig_nm, best_insert_nm, best_bad_nm = False, -1, 99999                        # :1784-1786
    if rrm and cfg.useNormalMode and cfg.useRatioMode:                                  # :1791
        ambig = ambig_rm or ambig_nm                                                    # :1792
        best_bad = best_bad_rm                                                          # :1793
        best_insert = best_insert_nm if best_insert_nm == best_insert_rm else -1        # :1794
    elif cfg.useRatioMode and best_insert_rm > -1 and not ambig_rm:                     # :1797
        ambig, best_bad, best_insert = ambig_rm, best_bad_rm, best_insert_rm            # :1798-1800
    else:
        ambig, best_bad, best_insert = ambig_nm, best_bad_nm, best_insert_nm            # :1802-1804
    if best_bad > cfg.maxMismatchesR:                                                   # :1809
        ambig = True
    rec = dict(minOverlap=min_overlap, insertRM=best_insert_rm, badRM=best_bad_rm, ambigRM=int(ambig_rm), insertNM=best_insert_nm,
               badNM=best_bad_nm, ambigNM=int(ambig_nm), bad=best_bad)

    def mate_by_overlap_returns():
        nonlocal ambig, best_insert, expected, prob, info
        if ambig:                                                                       # :1812
            return RET_AMBIG
        elif best_insert < 0:                                                           # :1813
            return RET_NO_SOLUTION
        if cfg.useQuality and qa is not None and qb is not None:                        # :1817
            fe, fp = None, None
            if cfg.useEfilter and best_insert > 0 and not ambig:                        # :1818
                fe, fp = _filters(a, b, qa.tobytes(), qb.tobytes(), best_insert)
                best_expected = fe                                                      # :1819
                if F(F(best_expected + F(cfg.efilterOffset)) * F(cfg.efilterRatio)) < F(best_bad):      # :1820
                    ambig = True
                expected = best_expected
                info |= M.INFO_EFILTER
            if cfg.pfilterRatio > 0 and best_insert > 0 and not ambig:                  # :1826
                if fp is None:
                    fe, fp = _filters(a, b, qa.tobytes(), qb.tobytes(), best_insert)
                prob = fp                                                               # :1827
                if prob < F(cfg.pfilterRatio):                                          # :1828
                    best_insert = -1
                info |= M.INFO_PFILTER
        if ambig:                                                                       # :1834
            return RET_AMBIG
        return best_insert if best_insert > 0 else RET_NO_SOLUTION                      # :1836

    best = mate_by_overlap_returns()                                                    # :2053
    ambig2 = best == RET_AMBIG                                                          # :2054
    max_read_length = cfg.maxLength if cfg.maxLength > 0 else 2 ** 31 - 1               # :634
    if ambig2:                                                                          # :2061
        code = RET_AMBIG
    elif best > 0:                                                                      # :2062
        if best < cfg.ratio.minInsert:                                                  # :2063
            code = RET_SHORT
        elif best > max_read_length:                                                    # :2064
            code = RET_LONG
        else:
            code = best                                                                 # :2065
    else:
        code = RET_NO_SOLUTION                                                          # :2067
    rec.update(code=code, expected=expected, probability=prob, info=info)
    return rec


def verdicts(pairs, cfg, with_quality=True, columns=None):
    """VERDICT_DTYPE[n] for [(a, b, qa, qb)]"""
    out = np.zeros(len(pairs), M.VERDICT_DTYPE)
    for i, (a, b, qa, qb) in enumerate(pairs):
        rec = verdict(a, b, qa if with_quality else None, qb if with_quality else None, cfg, columns)
        for k, v in rec.items():
            out[k][i] = v
    return out


def recount(recs):
    """bbmerge_stats from records (BBMerge.java:1402-1422): a STATS_DTYPE[1] array"""
    s = M.new_stats()
    recs = np.asarray(recs)
    skipped = (recs["info"] & M.INFO_SKIPPED) != 0
    code = recs["code"]
    merged = ~skipped & (code > 0)
    s["pairs"], s["skipped"], s["merged"] = len(recs), skipped.sum(), merged.sum()
    s["ambiguous"] = (~skipped & (code == RET_AMBIG)).sum()
    s["tooShort"] = (~skipped & (code == RET_SHORT)).sum()
    s["tooLong"] = (~skipped & (code == RET_LONG)).sum()
    s["noSolution"] = (~skipped & (code == RET_NO_SOLUTION)).sum()
    if merged.any():
        ins = code[merged].astype(np.int64)
        s["insertSum"], s["insertMin"], s["insertMax"] = ins.sum(), ins.min(), ins.max()
        s["hist"][0] = np.bincount(np.minimum(ins, M.HIST_LEN - 1), minlength=M.HIST_LEN)
    return s


def differing(got, exp):
    """indices where two VERDICT_DTYPE arrays differ in any field, the floats compared by their bits"""
    assert got.dtype == exp.dtype == M.VERDICT_DTYPE and len(got) == len(exp)
    words = lambda r: np.ascontiguousarray(r).view("<i4").reshape(len(r), M.VERDICT_DTYPE.itemsize // 4)          # noqa: E731
    return np.flatnonzero((words(got) != words(exp)).any(axis=1))
