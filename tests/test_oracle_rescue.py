"""CPU tests of the rescue-scan oracle (AbstractMapThread.quickRescue restated): hand-derived cases."""
import collections
import functools

from oracle.oracle import quick_rescue
from tests.rescue_check import first_divergence, quick_rescue_literal, trace_quick_rescue
from tests.rescue_problems import make_full_set, make_problems, scanned


def test_quick_rescue_known_cases():
    ref = b"N" * 20 + b"ACGTTGCAAGCTTAGGCTTAACGGATCCGATTACAGGCTAAGCTTCGATCGGATATCGGCTAGCTAGGCTTAAGG" * 3 + b"N" * 20
    read = ref[60:100]
    r = quick_rescue(read, ref, 20, 30, 200, True, 58, 10)
    # exact copy at 60; the unit repeats every 75 bases, so 135 also matches: the scan stops at idealStart + |60 - 58|
    assert r == dict(start=60, stop=99, score=70 + 100 * 39, mismatches=0, perfect=1, semiperfect=1, contig=0)
    r = quick_rescue(read, ref, 20, 200, 200, False, 140, 10)      # searching left from 200: 135 comes first and is nearer
    assert r["start"] == 135 and r["perfect"] == 1
    bad = bytearray(read); bad[10] = ord("N"); bad[30] = ord("A") if bad[30] != ord("A") else ord("C")
    r = quick_rescue(bytes(bad), ref, 20, 30, 200, True, 58, 10)
    # two mismatches (the N and the substitution); runs of 10 and 19 complete before a mismatch, the trailing 9 do not count
    assert (r["start"], r["mismatches"], r["contig"], r["perfect"], r["semiperfect"]) == (60, 2, 19, 0, 0)
    assert r["score"] == 70 + 100 * (40 - 1 - 2)
    # the reference starts with minMismatches = maxAllowedMismatches + 1 and accepts "<=": one more than "allowed" passes
    assert quick_rescue(bytes(bad), ref, 20, 30, 200, True, 58, 1)["mismatches"] == 2
    assert quick_rescue(bytes(bad), ref, 20, 30, 200, True, 58, 0) is None
    assert quick_rescue(read[:9], ref, 20, 30, 200, True, 58, 3) is None            # reads shorter than 10 are not rescued


def test_quick_rescue_generated_set_is_consistent():
    ref, probs = make_problems(3, 200)
    found = 0
    for b, ch, loc, sd, right, ideal, mam in probs:
        r = quick_rescue(b, ref, 0, loc, sd, right, ideal, mam)
        if r is None:
            continue
        found += 1
        mm = sum(1 for j in range(len(b)) if b[j] != ref[r["start"] + j] or b[j] == ord("N"))
        assert mm == r["mismatches"] <= mam + 1
        lo = max(0, loc) if right else max(0, loc - sd)
        hi = min(len(ref) - len(b), loc + sd) if right else min(len(ref) - len(b), loc)
        assert lo <= r["start"] <= hi
    assert found > 80


# ---------------------------------------------------------------------------------------------------------------
# The edge sets of tests/rescue_problems.py: the sequential tracer (tests/rescue_check.py, written from the Java) against the
# C oracle, and counts of what those inputs exercise.  SEED and N_EDGE are the set the GPU test runs.
SEED, N_EDGE = 1, 3000
FLOOR_PER_DIRECTION = ("narrow_in_block", "narrow_stops_later_block", "stale_cap", "improve", "tie_win", "tie_lose", "tie_equal_absdif")


@functools.lru_cache(maxsize=None)
def _traced(seed):
    chroms, min_index, probs, fams = make_full_set(seed, N_EDGE)
    out = []
    for p in probs:
        b, ch, loc, sd, right, ideal, mam = p
        out.append(trace_quick_rescue(b, chroms[ch - 1], min_index[ch - 1], loc, sd, right, ideal, mam) if scanned(p) else (None, None))
    return chroms, min_index, probs, fams, out


def test_tracer_shortcut_equals_the_literal_loops():
    """trace_quick_rescue walks mismatch positions found by numpy; the base-by-base Java loops must give the same on short jobs."""
    chroms, min_index, probs, fams, traced = _traced(SEED)
    n = 0
    for p, (res, rec) in zip(probs, traced):
        b, ch, loc, sd, right, ideal, mam = p
        if scanned(p) and len(b) <= 65 and sd <= 200 and n < 400:
            n += 1
            for kw in (dict(), dict(pointsMatch=53, pointsMatch2=91, useAffine=False, baseHitScore=37)):
                lit = quick_rescue_literal(b, chroms[ch - 1], min_index[ch - 1], loc, sd, right, ideal, mam, **kw)
                got = trace_quick_rescue(b, chroms[ch - 1], min_index[ch - 1], loc, sd, right, ideal, mam, **kw)[0]
                assert got == lit, (p[1:], got, lit)
    assert n == 400


def test_tracer_equals_oracle_on_the_edge_sets():
    """Field for field, on every scanned job of make_full_set(seed, 3000) for seeds 1, 2 and 3: 3 x 3000 edge jobs (B), all
    planted jobs (C, 3 x 680) and the scanned degenerate ones, about 11,000 jobs, under both score formulas.  Measured on the
    CPU: 6.0 s for this test (oracle 0.5 s, tracer the rest); the slowest CPU test before it took 7.5 s."""
    diffs = []
    for seed in (SEED, 2, 3):
        chroms, min_index, probs, fams, traced = _traced(seed)
        for p, f, (res, rec) in zip(probs, fams, traced):
            if not scanned(p):
                continue
            b, ch, loc, sd, right, ideal, mam = p
            args = (b, chroms[ch - 1], min_index[ch - 1], loc, sd, right, ideal, mam)
            exp = quick_rescue(*args)
            if res != exp:
                diffs.append((seed, f, p[1:], res, exp))
            kw = dict(pointsMatch=53, pointsMatch2=91, useAffine=False, baseHitScore=37)
            res2, exp2 = trace_quick_rescue(*args, **kw)[0], quick_rescue(*args, **kw)
            if res2 != exp2:
                diffs.append((seed, f, p[1:], res2, exp2))
    assert not diffs, "%d differences, first:\n%r\n%s" % (len(diffs), diffs[0], first_divergence(
        *[(p[0], c[p[1] - 1], m[p[1] - 1]) + p[2:] for c, m, ps, _, _ in [_traced(diffs[0][0])] for p in ps if p[1:] == diffs[0][2]][0],
        got=diffs[0][4]))


def test_edge_set_reaches_the_branches_it_is_for():
    """Counts the inputs of the committed seed: nothing is measured.  A job counts once however often it takes a branch."""
    chroms, min_index, probs, fams, traced = _traced(SEED)
    jobs = collections.Counter()
    for p, (res, rec) in zip(probs, traced):
        if rec is None:
            continue
        d = "right" if p[4] else "left"
        for k in FLOOR_PER_DIRECTION:
            jobs[k, d] += rec[k] > 0
        jobs["tail_bytes", rec["tail_bytes"]] += 1
        jobs["len", len(p[0])] += 1
        jobs["sp_exit_chunk", rec["sp_exit_chunk"]] += 1
        jobs["sp_n_over_limit"] += rec["sp_n_over_limit"]
        jobs["semiperfect_not_perfect"] += res is not None and res["semiperfect"] == 1 and res["perfect"] == 0
        jobs["clipped_both_ends"] += rec["clip_low"] and rec["clip_high"]
        jobs["chrom", p[1]] += 1
    print(sorted(jobs.items(), key=str))
    for k in FLOOR_PER_DIRECTION:
        for d in ("right", "left"):
            assert jobs[k, d] >= 50, (k, d, jobs[k, d])
    for t in range(4):
        assert jobs["tail_bytes", t] >= 20, t
    for n in (10, 11, 12, 13, 597, 598, 599, 600):
        assert jobs["len", n] >= 20, n
    for c in range(1, 10):
        assert jobs["sp_exit_chunk", c] >= 20, c
    assert jobs["sp_n_over_limit"] >= 20
    assert jobs["semiperfect_not_perfect"] >= 20
    assert jobs["clipped_both_ends"] >= 20
    assert all(jobs["chrom", c] >= 20 for c in range(1, len(chroms) + 1))
    # chromosome numbers are mixed inside the 4-job workgroups
    assert sum(len({p[1] for p in probs[i:i + 4]}) > 1 for i in range(0, len(probs) - 3, 4)) > len(probs) // 8


def test_planted_families_do_what_they_were_built_for():
    chroms, min_index, probs, fams, traced = _traced(SEED)
    seen = collections.Counter()
    for p, f, (res, rec) in zip(probs, fams, traced):
        b, ch, loc, sd, right, ideal, mam = p
        seen[f.split(":")[0]] += 1
        if f in ("i:few", "i:half") and len(b) >= 41:
            assert res is not None and (res["perfect"], res["semiperfect"]) == (0, 1) and not rec["sp_n_over_limit"], (f, p[1:], res)
            assert res["mismatches"] == (len(b) // 2 if f == "i:half" else res["mismatches"]) > 0
        elif f == "i:over" and len(b) >= 41:
            assert res is not None and res["semiperfect"] == 0 and rec["sp_n_over_limit"] and res["mismatches"] == len(b) // 2 + 1
        elif f.startswith("ii:"):
            assert res is not None and rec["sp_exit_chunk"] == int(f[3:]) and not rec["sp_n_over_limit"], (f, p[1:], res, rec)
        elif f == "iii" and mam == -1:
            d = [x for x in (1, 31, 32, 33, 63, 64, 65) if res is not None and abs(res["start"] - ideal) == x]
            assert d and rec["tie_equal_absdif"] == 1 and res["perfect"] == 1, (p[1:], res, rec)
            assert res["start"] == (ideal - d[0] if right else ideal + d[0])          # the copy met first keeps the site
        elif f == "iv":
            assert rec["stale_cap"] >= 1 and rec["improve"] >= 1, (p[1:], res, rec)
        elif f == "v":
            assert (res is not None) == (mam + 1 >= len(b)), (p[1:], res)
            assert res is None or (res["mismatches"], res["contig"], res["semiperfect"]) == (len(b), 0, 0)
        elif f == "vi":
            assert res is None or res["mismatches"] > 0, (p[1:], res)
        elif f == "D":
            assert res is None
    assert seen["i"] == 96 and seen["ii"] == 216 and seen["iii"] == 168 and seen["iv"] == 120 and seen["v"] == 24 and seen["vi"] == 24
    assert seen["D"] == 16
