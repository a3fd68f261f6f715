"""Oracle answer of one bbmsa job and the field-by-field check of a kernel's record against it (shared by the GPU parity
tests of the DP: tests/test_msa_gpu.py, tests/test_msa_routes_gpu.py, tests/test_msa_rows_per_lane_gpu.py), and the check of
one per-call fill's planes and limits against the oracle's `packed` matrix."""
import ctypes as C

import numpy as np

from bbmap_amd import msa as M
from oracle.oracle import OracleMSA


def oracle_align(om, read, ref, a, b, ms, flags):
    """What the reference would produce for one job with these flags (oracle restatement)."""
    mode = flags & 7
    out = {"score": None, "match": None, "status": 0}
    if flags & M.CLAMP_WINDOW:
        a = max(0, a)
        b = min(len(ref) - 1, b)
    it_l0, it_u0 = om.iterationsLimited, om.iterationsUnlimited
    if mode == M.FILL_LIMITED_RAW:
        res, _ = om.fill_limited_raw(read, ref, a, b, ms)
        om.s.rows, om.s.columns = len(read), b - a + 1
        null = res[4] == 1
    elif mode == M.FILL_UNLIMITED_RAW:
        res, _ = om.fill_unlimited_raw(read, ref, a, b)
        res = res + [0]
        om.s.rows, om.s.columns = len(read), b - a + 1
        null = False
    else:
        r4 = om.fillLimited(read, ref, a, b, ms)
        null = r4 is None
        res = None if null else r4 + [0]
        if null:
            out["status"] = 1
    out["iterations"] = (om.iterationsLimited - it_l0) + (om.iterationsUnlimited - it_u0)
    out["fill_kind"] = 1 if om.iterationsUnlimited != it_u0 else 0
    out["result"] = res
    if not null:
        if flags & M.DO_SCORE:
            out["score"] = om.score(read, ref, a, b, res[0], res[1], res[2])
        if flags & M.DO_TRACEBACK:
            out["match"] = om.traceback(read, ref, a, b, res[0], res[1], res[2])
    return out


def oracle_align_gapped(om, read, ref, a, b, ms, gaps, flags):
    """What the reference would produce for one job of the gapped entries (bbmsa_align_gapped_batch*): without a gap array the
    plain job; with one, MSA.fillAndScoreLimited(read, ref, a, b, minScore, gaps) -- or fillUnlimited(read, ref, a, b, gaps) for
    BBMSA_FILL_UNLIMITED_RAW -- on the clamped window, then score(..., gapped) always and traceback(..., gapped) on request.
    Beside oracle_align's fields: refused (the gapped reference does not fit maxColumns: the device answers BBMSA_ST_BAD_SHAPE),
    kept (the string before its '-' are expanded) and gref = (buffer, greflimit, greflimit2, grefRefOrigin)."""
    if gaps is None:
        out = oracle_align(om, read, ref, a, b, ms, flags)
        out.update(refused=False, kept=out["match"], gref=None)
        return out
    a, b = max(0, a), min(len(ref) - 1, b)
    out = {"score": None, "match": None, "kept": None, "status": 0, "refused": False, "gref": None, "result": None,
           "iterations": 0, "fill_kind": 0}
    lim = om.makeGref(ref, gaps, a, b)
    if lim is None or lim + 1 > om.maxColumns:
        out["refused"] = True
        out["status"] = M.ST_BAD_SHAPE
        assert om.fillLimited(read, ref, a, b, ms, gaps) is None and om.fillUnlimited(read, ref, a, b, gaps) is None
        return out
    it_l0, it_u0 = om.iterationsLimited, om.iterationsUnlimited
    if flags & 7 == M.FILL_UNLIMITED_RAW:
        r4 = om.fillUnlimited(read, ref, a, b, gaps)
    else:
        r4 = om.fillLimited(read, ref, a, b, ms, gaps)
    out["iterations"] = (om.iterationsLimited - it_l0) + (om.iterationsUnlimited - it_u0)
    out["fill_kind"] = 1 if om.iterationsUnlimited != it_u0 else 0
    out["gref"] = om.gref()
    if r4 is None:
        out["status"] = M.ST_NULL
        return out
    out["result"] = r4 + [0]
    out["score"] = om.score(read, ref, a, b, r4[0], r4[1], r4[2], gapped=True)
    if flags & M.DO_TRACEBACK:
        out["match"] = om.traceback(read, ref, a, b, r4[0], r4[1], r4[2], gapped=True)
        out["kept"] = om.traceback(read, ref, a, b, r4[0], r4[1], r4[2], gapped=True, keep_gaps=True)
    return out


_GAPPED = {}


def gapped_set(scheme, name):
    """One set of tests/gapped_problems.py, built once: (problems, flags, kinds)."""
    from tests import gapped_problems as G
    key = ("set", scheme, name)
    if key not in _GAPPED:
        _GAPPED[key] = G.SETS[name](scheme)
    return _GAPPED[key]


def gapped_expected(scheme, name, band=(0, 0.0), maxColumns=None, problems=None, flags=None, kinds=None):
    """The oracle's answers for a set of tests/gapped_problems.py (or for the jobs given), computed once per context shape and
    shared by the tests; None for the arrays of the `refused` class, which the reference's contract does not cover."""
    from tests import gapped_problems as G
    key = ("exp", scheme, name, band, maxColumns)
    if key not in _GAPPED:
        if problems is None:
            problems, flags, kinds = gapped_set(scheme, name)
        sh = G.SHAPES[scheme]
        om = OracleMSA(sh["maxRows"], maxColumns or sh["maxColumns"], band[0], band[1], scheme=scheme)
        _GAPPED[key] = [None if G.is_refused(k) else oracle_align_gapped(om, p[0], p[1], p[2], p[3], p[4], G.gaps_of(p), f)
                        for p, f, k in zip(problems, flags, kinds)]
    return _GAPPED[key]


def check_gapped_job(g, exp, flags, ctx):
    """g: one raw record (test_msa_routes_gpu.record) of a job of the gapped entries; exp: oracle_align_gapped's answer.  Status,
    score[0..score_len), result[0..4] and match_len always; the string where DO_TRACEBACK asked for one (KEEP_GAPS: with its '-');
    iterations unless BBMSA_NO_ITERATIONS."""
    if exp["refused"]:
        assert g["status"] == M.ST_BAD_SHAPE and g["match_len"] == 0 and g["score"] is None, ctx
        return
    assert g["status"] == exp["status"], ctx
    if exp["result"] is not None:
        assert g["result"] == exp["result"], ctx
    assert g["score"] == exp["score"], ctx
    assert g["fill_kind"] == exp["fill_kind"], ctx
    if not flags & M.NO_ITERATIONS:
        assert g["iterations"] == exp["iterations"], ctx
    want = exp["kept"] if flags & M.TRACE_KEEP_GAPS else exp["match"]
    if flags & M.DO_TRACEBACK and want is not None:
        assert g["match_len"] == len(want), ctx
        assert g["match"] == want, ctx
    else:
        assert g["match_len"] == 0 and g["match"] is None, ctx


def check_job(g, exp, ctx):
    """g: one record as MultiStateAligner11ts.align returns it; exp: oracle_align's answer for the same job."""
    if exp["result"] is not None:
        assert g["result"] == exp["result"], ctx
    else:
        assert g["status"] == M.ST_NULL, ctx
    assert g["status"] == exp["status"], ctx
    assert g["iterations"] == exp["iterations"], ctx
    assert g["fill_kind"] == exp["fill_kind"], ctx
    assert g["score"] == exp["score"], ctx
    assert g["match"] == exp["match"], ctx


MARK = 0x5a5a5a5a                                   # what the oracle's planes hold where its fill wrote nothing


def check_packed_fill(maxRows, maxCols, band, rd, ref, a, b, ms, limited, fill, packed=None):
    """One per-call fill (bbmsa_fill_submit / _collect) against a fresh oracle of the same shape.  `fill(packed)` gets the flat
    3 x (maxRows + 1) x (maxCols + 1) int32 array in the Java layout, holding what the constructor leaves there, puts the device's
    planes into it and returns (result5, iterations, vertLimit, horizLimit).  Three checks: (1) every cell the oracle's
    restatement of the native fill WROTE holds the same int on our side (score, time bits and the subfloor of visited-but-bad
    cells), and nothing outside rows x columns changed; (2) vertLimit / horizLimit come back as the native code leaves them;
    (3) score2 / traceback2 (the oracle's restatement of the Java walkers, which read `packed`) run on OUR matrix and give what they
    give on the oracle's own.  Returns whether the walkers ran (False: a limited fill below minScore, nothing to walk).
    `packed`: an array to reuse."""
    om = OracleMSA(maxRows, maxCols, bandwidth=band[0], bandwidthRatio=band[1])
    view = np.ctypeslib.as_array(om.s.packed, shape=(3, maxRows + 1, maxCols + 1))
    pristine = view.copy()                              # row 0 / column 0 as the constructor leaves them
    view[:, 1:, 1:] = MARK
    if limited:
        exp, exp_it = om.fill_limited_raw(rd, ref, a, b, ms)
    else:
        exp, exp_it = om.fill_unlimited_raw(rd, ref, a, b)
        exp = exp + [0]
    if packed is None:
        packed = np.empty(pristine.size, np.int32)
    packed[:] = pristine.reshape(-1)
    got, it, vl, hl = fill(packed)
    assert got[:4] == exp[:4] and (not limited or got[4] == exp[4]) and it == exp_it
    rows, cols = len(rd), b - a + 1
    ours = packed.reshape(3, maxRows + 1, maxCols + 1)
    o, g = view[:, 1:rows + 1, 1:cols + 1], ours[:, 1:rows + 1, 1:cols + 1]
    wrote = o != MARK
    assert wrote.sum() > rows                           # (the oracle did fill something)
    # "not a score": subfloor (pruned, below the limit, or a row-end sentinel) and the BADoff the native fill spreads over the last
    # row first (:398-403).  Nothing reads the time bits of such a cell, and the native code itself strips them wherever a
    # sentinel lands on a computed cell; we keep subfloor there.  Every other cell -- every real score and its time -- is exact.
    maxGain = (rows - 1) * 100 + 70
    subfloor = ((ms << 11) - (maxGain << 11) - 5 * (100 << 11)) if limited else -2 * (maxGain << 11)
    badoff = (-(1 << 20) + 2000) << 11
    dead = wrote & (((o & ~2047) == subfloor) | (o == badoff))
    live = wrote & ~dead
    assert live.sum() > rows
    assert (g[live] == o[live]).all()
    assert (((g[dead] & ~2047) == subfloor) | (g[dead] == badoff)).all()
    assert (ours[:, 0, :] == pristine[:, 0, :]).all() and (ours[:, :, 0] == pristine[:, :, 0]).all()
    assert (ours[:, rows + 1:, :] == pristine[:, rows + 1:, :]).all() and (ours[:, 1:, cols + 1:] == pristine[:, 1:, cols + 1:]).all()
    if limited:
        assert list(vl) == np.ctypeslib.as_array(om.s.vertLimit, shape=(maxRows + 1,))[:rows + 1].tolist()
        assert list(hl) == np.ctypeslib.as_array(om.s.horizLimit, shape=(maxCols + 1,))[:cols + 1].tolist()
    if limited and exp[4] == 1:
        return False
    want_score = om.score(rd, ref, a, b, exp[0], exp[1], exp[2])
    want_tb = om.traceback(rd, ref, a, b, exp[0], exp[1], exp[2])
    # same walkers, our matrix: overwrite the oracle's packed with the planes the GPU produced
    C.memmove(om.s.packed, packed.ctypes.data, packed.size * 4)
    assert om.score(rd, ref, a, b, got[0], got[1], got[2]) == want_score
    assert om.traceback(rd, ref, a, b, got[0], got[1], got[2]) == want_tb
    return True
