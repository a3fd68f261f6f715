"""The band kernel (msa_fill_band.hip: a job over 8 lanes, 32 diagonals in registers, in front of the first pass) against the oracle.

Every job of every set is compared with OracleMSA field by field as tests/msa_check.py does -- status, result[5], score vector,
iterations, match string -- whichever kernel finished it: the band kernel hands a job on the moment its window touches the band's
edge.  bbmsa_last_counts says how many jobs it finished and how many of its candidates it handed on; the candidate rule is
restated here (is_candidate), so `finished + handed on == candidates` pins that every candidate went one way or the other."""
import random

import numpy as np
import pytest

from bbmap_amd import msa as M
from bbmap_amd import workload as W
from bbmap_amd.index import DeviceIndex
from bbmap_amd.mapper import Mapper
from oracle import oracle as O
from oracle.oracle import OracleMSA
from tests.mapper_check import compare, set_route
from tests.msa_check import check_job, oracle_align
from tests.problems import max_quality, rand_seq
from tests.test_msa_routes_gpu import Dev, make_ctx, record, run

pytestmark = pytest.mark.gpu

MAXR, MAXC, FAST = 160, 1024, 320
ALL = M.FILL_AND_SCORE_LIMITED | M.DO_TRACEBACK
RAW = M.FILL_LIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
KEEP_GAPS = 1 << 7
B = 32                                      # diagonals of the band
MAX_SLACK = 2000                            # BBMSA_NARROW_SLACK's default
BADOFF = (-(((1 << 20) - 1) - 2000) - 1) * 2048

_RNG = random.Random(5)
REF = rand_seq(_RNG, 30000)


def is_candidate(p, fl, max_slack=MAX_SLACK):
    """The band kernel's candidate rule (msa_fill_band.hip; its predecessor's, unchanged)."""
    read, ref, a, b, ms = p
    if fl & M.CLAMP_WINDOW:
        a, b = max(0, a), min(len(ref) - 1, b)
    rows, cols, mode = len(read), b - a + 1, fl & 7
    if not (16 <= rows <= MAXR and rows <= cols <= MAXC) or mode == M.FILL_UNLIMITED_RAW:
        return False
    if mode == M.FILL_LIMITED:
        if ms < 1 or cols + rows < 90 or cols > rows + min(170, rows + 20):
            return False
        ms -= 120
    return max_quality(rows) - ms <= max_slack


def launch(monkeypatch, probs, flags, stride=None, env=None, count=None, cap=None):
    jobs, reads, refs = M.pack_problems(probs, flags)
    if stride is None:
        stride = (max(len(p[0]) + (p[3] - p[2] + 1) + 8 for p in probs) + 15) & ~15
    ctx = make_ctx(monkeypatch, env or {}, 32, maxRows=MAXR, maxColumns=MAXC, fast_cols=FAST)
    rec, mat = run(ctx, Dev(jobs, reads, refs, cap=cap), stride, count=count)
    r, c = ctx.last_route(), ctx.last_counts()
    ctx.close()
    return rec, mat, r, c


def check_set(probs, flags, rec, mat, tag, skip_match=()):
    om = OracleMSA(MAXR, MAXC)
    for k, (p, fl) in enumerate(zip(probs, flags)):
        exp = oracle_align(om, p[0], p[1], p[2], p[3], p[4], fl)
        g = record(rec, mat, k)
        if k in skip_match:
            g["match"] = exp["match"]
        check_job(g, exp, "%s: job %d rows %d window [%d, %d] minScore %d flags %#x" % (tag, k, len(p[0]), p[2], p[3], p[4], fl))


def centred(ref, st, L, cols):
    """the window of `cols` columns in which ref[st:st+L] lies on the band's middle diagonal"""
    a = st - (cols - L) // 2
    return a, a + cols - 1


def substitute(rng, rd, n, lo=0, hi=None):
    rd = bytearray(rd)
    hi = len(rd) if hi is None else hi
    for _ in range(n):
        i = rng.randrange(lo, hi)
        rd[i] = rng.choice([c for c in b"ACGT" if c != rd[i]])
    return bytes(rd)


# ------------------------------------------------------------------------------------------------ shapes
def test_shapes_and_both_parities(monkeypatch):
    rng = random.Random(11)
    probs, flags = [], []
    for L in (16, 17, 31, 32, 33, 64, 149, 150, 151, 160):
        for cols in (L, L + 1, L + 8, L + 12, L + 13, L + 60, 256):
            for v in range(5):
                st = rng.randrange(2000, len(REF) - 2000)
                rd = substitute(rng, REF[st:st + L], v % 3)
                ref = REF
                if v == 3:                                             # an N in the read
                    rd = bytearray(rd); rd[rng.randrange(L)] = ord("N"); rd = bytes(rd)
                a, b = centred(REF, st, L, cols)
                if v == 4:                                             # an N in the window: handed on
                    x = bytearray(REF[a - 50:b + 50]); x[50 + rng.randrange(cols)] = ord("N"); ref = bytes(x); a, b = 50, 50 + cols - 1
                ms = max_quality(L) - rng.choice([0, 200, 700, 1500, 1800])
                for fl in (ALL, RAW):
                    probs.append((rd, ref, a, b, ms, )); flags.append(fl)
    # windows clamped at the reference's start and at its end
    short = rand_seq(rng, 170)
    for L, st in ((150, 3), (150, 15), (100, 60), (64, 100)):
        for ms_off in (0, 600):
            probs.append((substitute(rng, short[st:st + L], 1), short, st - 9, st + L + 8, max_quality(L) - ms_off)); flags.append(ALL)
    rec, mat, r, c = launch(monkeypatch, probs, flags)
    check_set(probs, flags, rec, mat, "shapes")
    cand = sum(is_candidate(p, f) for p, f in zip(probs, flags))
    print("shapes: %d jobs, %d candidates, band finished %d, handed on %d" % (len(probs), cand, c["narrow"], c["narrow_left"]))
    assert r["narrow"] and c["narrow"] + c["narrow_left"] == cand, (r, c, cand)
    assert c["narrow"] > 0 and c["narrow_left"] > 0, c                # (every candidate with an N in its window is handed on)


# ------------------------------------------------------------------------------------------------ band edges
def _indel_set(rng):
    """150-base reads with ONE deletion or ONE insertion of d bases near either end, in windows padded by 6 columns on both sides
    as realign_new pads them, minScore = the score the oracle finds (RAW: 50 points below it).  Row 1 is good over the whole
    free shift of the window, columns - rows + 1 = d + 13 columns with a deletion, and the path itself crosses d diagonals: at
    about half the band the fill touches an edge and is handed on.  Insertions of more than 11 bases cost more than the
    candidate rule's 2,000 points of slack and never enter the kernel."""
    om = OracleMSA(MAXR, MAXC)
    probs, flags = [], []
    L = 150
    for d in range(8, 21):
        for where in (20, L - 24):
            for ins in (False, True):
                st = rng.randrange(2000, len(REF) - 2000)
                if ins:
                    rd = REF[st:st + where] + rand_seq(rng, d) + REF[st + where:st + L - d]
                    a, b = st - 6, st + L + 5
                else:
                    rd = REF[st:st + where] + REF[st + where + d:st + L + d]
                    a, b = st - 6, st + L + d + 5
                sv, _ = om.fillAndScoreLimited(rd, REF, a, b, 1)
                probs.append((rd, REF, a, b, sv[0])); flags.append(ALL)
                probs.append((rd, REF, a, b, sv[0] - 50)); flags.append(RAW)
    return probs, flags


def test_band_edges_one_indel_of_growing_length(monkeypatch):
    probs, flags = _indel_set(random.Random(12))
    rec, mat, r, c = launch(monkeypatch, probs, flags)
    check_set(probs, flags, rec, mat, "band edges")
    cand = sum(is_candidate(p, f) for p, f in zip(probs, flags))
    nonnull = sum(int(rec[k]["status"]) == M.ST_OK and int(rec[k]["result"][4]) == 0 for k in range(len(probs)))
    print("band edges: %d jobs, %d candidates, %d non-null, band finished %d, handed on %d" % (len(probs), cand, nonnull, c["narrow"], c["narrow_left"]))
    assert cand >= len(probs) // 2 and nonnull > len(probs) // 2      # every deletion is a candidate; minScore is the fill's own score
    assert c["narrow"] > 0 and c["narrow_left"] > 0 and c["narrow"] + c["narrow_left"] == cand, c


# ------------------------------------------------------------------------------------------------ must finish
def _visited_diagonals(om, view, p):
    """min and max of col - row over the cells the reference's limited fill writes in rows 2 .. rows-1 (the marked-matrix method of
    scripts/exp_band_width.py), or None when it writes none"""
    MARK = 0x5A5A5A5A
    read, ref, a, b, ms = p
    L, cols = len(read), b - a + 1
    view[:, 1:, 1:] = MARK
    om.fill_limited_raw(read, ref, a, b, ms - 120)
    wrote = (view[:, 2:L, 1:cols + 1] != MARK).any(axis=0)
    rows_i, cols_i = np.nonzero(wrote)
    if len(rows_i) == 0:
        return None
    d = (cols_i + 1) - (rows_i + 2)
    return int(d.min()), int(d.max())


def test_tight_fills_in_padded_windows_all_finish_in_the_band(monkeypatch):
    """What realign_new's first fill is for most reads: 0-3 substitutions, a window of rows + 12 columns, minScore = the ungapped
    score.  Checked on the CPU first: the reference's visited cells stay within the middle B - 4 diagonals of the band."""
    rng = random.Random(13)
    probs = []
    om = OracleMSA(MAXR, MAXC)
    view = np.ctypeslib.as_array(om.s.packed, shape=(3, MAXR + 1, MAXC + 1))
    for i in range(512):
        L = (150, 150, 100, 151)[i % 4]
        st = rng.randrange(2000, len(REF) - 2000)
        rd = substitute(rng, REF[st:st + L], i % 4, 3, L - 3)
        sv, _ = om.fillAndScoreLimited(rd, REF, st, st + L - 1, 1)       # the ungapped placement's score
        a, b = st - 6, st + L + 5
        probs.append((rd, REF, a, b, sv[0]))
        ext = _visited_diagonals(om, view, probs[-1])
        D0 = (12 // 2) - B // 2                                          # band position i of row r is column r + D0 + i
        assert ext is not None and ext[0] >= D0 + 2 and ext[1] <= D0 + B - 3, (i, ext)
    flags = [ALL] * len(probs)
    rec, mat, r, c = launch(monkeypatch, probs, flags)
    check_set(probs, flags, rec, mat, "must finish")
    assert c["narrow"] == len(probs) and c["narrow_left"] == 0, c


# ------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("entry", ["direct", "indirect"])
def test_job_counts_around_a_wave_of_sixteen(monkeypatch, entry):
    """16 jobs share a wavefront, two a lane group: rows 36 and 150 alternate, so every group steps a short and a long job."""
    rng = random.Random(14)
    probs = []
    for i in range(16 * 9 + 1):
        L = 36 if i % 2 else 150
        st = rng.randrange(2000, len(REF) - 2000)
        rd = substitute(rng, REF[st:st + L], i % 3)
        a, b = centred(REF, st, L, L + 20)
        probs.append((rd, REF, a, b, max_quality(L) - 150 * (i % 4)))
    om = OracleMSA(MAXR, MAXC)
    exp = [oracle_align(om, p[0], p[1], p[2], p[3], p[4], ALL) for p in probs]
    stride = 208
    for n in (1, 2, 15, 16, 17, len(probs)):
        sub, fl = probs[:n], [ALL] * n
        if entry == "direct":
            rec, mat, r, c = launch(monkeypatch, sub, fl, stride)
        else:
            rec, mat, r, c = launch(monkeypatch, probs, [ALL] * len(probs), stride, count=n, cap=len(probs) + 5)
            assert (rec[n:].view(np.uint8) == 0xA5).all(), n             # nothing past the count was touched
        for k in range(n):
            check_job(record(rec, mat, k), exp[k], "%s n=%d job %d" % (entry, n, k))
        assert r["narrow"] and r["indirect"] == (entry == "indirect") and c["narrow"] + c["narrow_left"] == n, (n, r, c)
        assert c["narrow"] > 0, (n, c)


# ------------------------------------------------------------------------------------------------ nulls and limits
def test_null_fills_slack_limit_and_short_match_slots(monkeypatch):
    rng = random.Random(15)
    L = 150
    probs, flags = [], []
    for where in (40, 75, 110, 140, 146):                              # a burst of substitutions: the fill stops in that row (BADoff) or gets through
        for nsub in (1, 2, 3, 5, 8):
            for slack in (0, 150, 400, 900, 1500):
                st = rng.randrange(2000, len(REF) - 2000)
                rd = substitute(rng, REF[st:st + L], nsub, where, min(L, where + 4))
                a, b = centred(REF, st, L, L + 12)
                probs.append((rd, REF, a, b, max_quality(L) - slack)); flags.append(RAW)
                probs.append((rd, REF, a, b, max_quality(L) - slack)); flags.append(ALL)
    for slack in (0, 100, 200):                                        # the last base alone differs: the last row is entered and has no good cell
        for i in range(8):
            st = rng.randrange(2000, len(REF) - 2000)
            rd = substitute(rng, REF[st:st + L], 1, L - 1, L)
            a, b = centred(REF, st, L, L + 12)
            probs.append((rd, REF, a, b, max_quality(L) - slack)); flags.append(RAW if i % 2 else ALL)
    rec, mat, r, c = launch(monkeypatch, probs, flags)
    check_set(probs, flags, rec, mat, "nulls")
    raw = [k for k in range(len(probs)) if flags[k] == RAW]
    res = rec["result"]
    bad_off = sum(int(res[k][4]) == 1 and int(res[k][3]) == BADOFF for k in raw)
    subfloor = {k: (probs[k][4] - max_quality(L) - 500) * 2048 for k in raw}          # minScore - maxGain - 5 * MATCH2, in offset points
    no_good = sum(int(res[k][4]) == 1 and int(res[k][3]) == subfloor[k] for k in raw)
    # (the third null case, a good cell in the last row with the best score below minScore, cannot happen in a limited fill: the
    # last row's vertLimit is minScore itself)
    print("nulls: BADoff %d, no good cell in the last row %d; band finished %d, handed on %d" % (bad_off, no_good, c["narrow"], c["narrow_left"]))
    assert bad_off > 0 and no_good > 0, (bad_off, no_good)
    assert c["narrow"] + c["narrow_left"] == len(probs) and c["narrow"] > 0, c

    # slack exactly at the limit is a candidate, one point more is not
    st = 5000
    a, b = centred(REF, st, L, L + 12)
    for slack, want in ((MAX_SLACK, 40), (MAX_SLACK + 1, 0)):
        pr = [(REF[st + i:st + i + L], REF, a + i, b + i, max_quality(L) - slack) for i in range(40)]
        rec, mat, r, c = launch(monkeypatch, pr, [RAW] * 40)
        check_set(pr, [RAW] * 40, rec, mat, "slack %d" % slack)
        assert r["narrow"] and c["narrow"] + c["narrow_left"] == want, (slack, c)

    # a match slot shorter than some tracebacks: the strings with a deletion need rows + d bytes
    pr, need = [], []
    for i in range(64):
        d = (0, 0, 3, 9)[i % 4]
        st = rng.randrange(2000, len(REF) - 2000)
        rd = REF[st:st + 70] + REF[st + 70 + d:st + L + d]
        a, b = centred(REF, st, L, L + 12 + d)
        pr.append((rd, REF, a, b, max_quality(L) - 900)); need.append(L + d)
    stride = L + 4
    rec, mat, r, c = launch(monkeypatch, pr, [ALL] * 64, stride)
    over = {k for k in range(64) if need[k] > stride}
    check_set(pr, [ALL] * 64, rec, mat, "short slots", skip_match=over)
    assert all(int(rec[k]["match_len"]) == (-1 if k in over else need[k]) for k in range(64)), rec["match_len"]
    assert len(over) == 16 and c["narrow"] > 0, c


# ------------------------------------------------------------------------------------------------ flow
def test_mapper_throughput_route_with_and_without_the_final_stage(monkeypatch):
    set_route(monkeypatch, "throughput")
    L, k = 150, 12
    ref = W.make_reference(300000, seed=6, pad=2000, repeat_frac=0.15)
    reads, _ = W.make_pairs(ref, 2000, read_len=L, seed=4, pad=2000, hard_frac=0.08)
    offs = O.make_offsets(L, k, 1.9)
    ks = [100 * k] * len(offs)
    n = reads.size // L
    oi = O.OracleIndex([ref], k=k)
    oi.s.p.quitAfterTwoPerfects = 0
    r = reads.reshape(-1, L)
    launches = {}
    for stage in (0, 1):
        di = DeviceIndex.build([ref], k=k)
        mp = Mapper(di, n, L, offs, ks, paired=True, max_sites=32, finalStage=stage)
        mp.load_reads(reads)
        mp.step()
        out, st = mp.fetch(), mp.stats()
        mp.close()
        di.close()
        orc = O.map_batch(oi, r[0::2].copy(), r[1::2].copy(), L, offs, ks, params=O.map_default_params(finalStage=stage), cap=64, match_stride=4200)
        bad = compare(out, orc, n, paired=True)
        assert not bad, "\n".join(bad[:20])
        launches[stage] = st["dp_narrow_launches"]
    print("band kernel launches: %d without the final stage, %d with it" % (launches[0], launches[1]))
    assert launches[1] > launches[0] > 0, launches
