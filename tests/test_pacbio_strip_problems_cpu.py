"""Census of the planted job sets of tests/pacbio_strip_problems.py, by the oracle alone (no GPU): the GPU tests of the strip kernel
(tests/test_pacbio_strip_edges_gpu.py) are only as good as what the sets contain, so every plant is held to the oracle's answer
here -- the insertion run lies on the rows it was planted on, the fill dies in the row it was meant to die in, the read hangs over
the window's end by as many bases as planned.  A plant that does not take fails here, on the CPU, and is re-seeded."""
import collections

import pytest

from bbmap_amd import msa as M
from tests import pacbio_strip_problems as P
from tests.pacbio_strip_problems import ALL, LIM, UNL, MAX_COLS, MAX_ROWS, STRIP, kind_args

BADOFF = (-(((1 << 22) - 1) - 2000) - 1) * 512      # MultiStateAligner9PacBio.BADoff (:2434)


def subfloor(rows, ms):
    """What a limited fill reports when its last row holds no good cell (:216-219 of the Java: floor - 5 * MATCH2)."""
    return (ms - ((rows - 1) * 100 + 90) - 500) * 512


def null_branch(p, fl, e):
    """Which of fillLimitedX's three "no result" exits a raw limited fill took (None: it has a result, or is not a raw limited fill)."""
    if fl & 7 != M.FILL_LIMITED_RAW or e["result"][4] != 1:
        return None
    return "middle" if e["result"][3] == BADOFF else "last" if e["result"][3] == subfloor(len(p[0]), p[4]) else "low"


def is_null(fl, e):
    return e["result"] is None if fl & 7 == M.FILL_LIMITED else (fl & 7 == M.FILL_LIMITED_RAW and e["result"][4] == 1)


def runs(p, fl, e):
    """The oracle's match string as runs [(symbol class, length, row, column)]: row / column (1-based, column of the window) of the
    cell the run starts at; 'M' stands for m / S / N.  An insertion run keeps its column, a deletion run its row (the row the
    diagonal goes on at)."""
    a = max(0, p[2]) if fl & M.CLAMP_WINDOW else p[2]
    row, col = 1, e["score"][1] - a + 1
    out = []
    for ch in e["match"].decode():
        cls = "M" if ch in "mSN" else ch
        if out and out[-1][0] == cls:
            out[-1][1] += 1
        else:
            out.append([cls, 1, row, col])
        row += cls != "D"
        col += cls in "MD"
    return [tuple(r) for r in out]


def by_kind(name):
    probs, flags, kinds, exp = P.answers(name)
    for k in range(len(probs)):
        kn, args = kind_args(kinds[k])
        yield k, kn, args, probs[k], flags[k], exp[k]


def test_set_shapes_and_modes():
    """Every set fits its context, uses the three modes, and its size is what the GPU tests were sized for."""
    sizes = {}
    for name, (gen, maxRows, maxColumns, band) in P.SETS.items():
        probs, flags, kinds = gen()
        assert (probs, flags, kinds) == gen()                                        # fixed seeds
        sizes[name] = len(probs)
        for p, f, k in zip(probs, flags, kinds):
            if not k.startswith("bad_"):
                assert 1 <= len(p[0]) <= maxRows and 1 <= P.columns_of(p, f, maxColumns) <= maxColumns, (name, k)
        if name != "death":
            assert set(flags) == {ALL, LIM, UNL}, name
    print("jobs per set:", sizes)
    assert all(n <= 250 for k, n in sizes.items() if k != "mixed") and 256 < sizes["mixed"] < 512
    assert (MAX_ROWS + STRIP - 1) // STRIP == 3 and MAX_COLS % 8 and MAX_COLS >= MAX_ROWS + 170


def test_rows_and_death_take_every_reachable_null_branch():
    """Three exits of a limited fill give no result: a row was never entered (BADoff), the last row holds no good cell (subfloor),
    the best score of the last row is below minScore.  The first two are planted.  The third cannot happen, in this scheme or in
    11ts: a good cell of the last row is >= max(vertLimit[rows], horizLimit[col]), vertLimit[rows] is minScore itself (no base is
    left to gain from), so a last row with a good cell has a best score >= minScore.  It is counted, and must stay 0."""
    seen = collections.Counter()
    lengths = collections.defaultdict(set)
    for name in ("rows", "death"):
        for k, kn, args, p, fl, e in by_kind(name):
            br = null_branch(p, fl, e)
            seen[(name, br)] += 1
            lengths[kn].add(len(p[0]))
            if kn == "last_row":
                assert br == "last", (k, args)
            if kn == "death":
                assert br == "middle", (k, args)
            if kn == "unreachable" and len(p[0]) >= 2 and fl == LIM:
                assert br == "middle", (k, args)
            if kn in ("perfect", "subs", "refn"):
                assert not is_null(fl, e), (k, kn, args)
    print("null branches:", dict(seen))
    assert seen[("rows", "middle")] >= 5 and seen[("rows", "last")] == len(P.ROW_LENGTHS) - 1 and seen[("death", "middle")] == 24
    assert seen[("rows", "low")] == 0 and seen[("death", "low")] == 0
    for kn in ("perfect", "subs", "refn", "lower", "wrong_site", "unreachable"):
        assert lengths[kn] == set(P.ROW_LENGTHS), kn
    assert lengths["del"] == lengths["ins"] == {r for r in P.ROW_LENGTHS if r >= 7}
    ns = sorted((args["rows"], args["q"]) for k, kn, args, p, fl, e in by_kind("rows") if kn == "n" and "q" in args)
    assert ns == sorted((r, q) for r in P.ROW_LENGTHS if r >= 511 for q in (510, 511, 512, 513) if q < r)
    for k, kn, args, p, fl, e in by_kind("rows"):
        if kn == "n" and "q" in args:
            assert p[0][args["q"]] == ord("N") and p[0].count(b"N") == 1


def test_death_walks_the_first_row_not_entered_across_the_border():
    """One more row is entered per step of q, so the visited cells strictly increase -- through q = 510, 511, 512 where the last
    row entered is 511, 512 (the strip's last) and 513 (the next strip's first)."""
    its = collections.defaultdict(list)
    for k, kn, args, p, fl, e in by_kind("death"):
        assert e["result"][3] == BADOFF and e["result"][4] == 1 and e["fill_kind"] == 0
        its[args["rows"]].append((args["q"], e["iterations"]))
    assert sorted(its) == sorted(P.DEATH_ROWS)
    for rows, v in its.items():
        assert [q for q, _ in v] == list(P.DEATH_Q) and P.DEATH_Q[0] < STRIP - 1 and P.DEATH_Q[-1] > STRIP + 1
        assert all(x[1] < y[1] for x, y in zip(v, v[1:])), (rows, v)
        print("death rows %d: iterations %s" % (rows, [i for _, i in v]))


def test_cols_sit_on_the_block_and_dword_edges():
    seen64, seen8, kinds = set(), set(), collections.Counter()
    for k, kn, args, p, fl, e in by_kind("cols"):
        cols = P.columns_of(p, fl)
        kinds[kn] += 1
        if kn == "width":
            assert cols == args["cols"] and cols >= args["rows"] + 8
            seen64.add((args["rows"], cols % 64))
            seen8.add((args["rows"], (cols + 63) & 7))
        if kn == "max_columns":
            assert cols == MAX_COLS
        if kn == "narrow":
            assert cols == len(p[0]) - args["short"]
        if kn.startswith("clamped"):
            assert fl == ALL and (p[2] < 0 or p[3] >= len(p[1]))
        assert not is_null(fl, e), (k, kn, args)
    assert seen64 == {(r, m) for r in (513, 600) for m in (62, 63, 0, 1, 2)}
    assert seen8 >= {(r, m) for r in (513, 600) for m in (6, 7, 0)}
    assert kinds["max_columns"] == 6 and kinds["narrow"] == 12 and kinds["clamped_left"] == kinds["clamped_right"] == kinds["clamped_both"] == 2
    narrow = {args["short"] for k, kn, args, p, fl, e in by_kind("cols") if kn == "narrow"}
    assert narrow == {0, 3, 40}


def test_walk_plants_took():
    seen = collections.Counter()
    for k, kn, args, p, fl, e in by_kind("walk"):
        where = (k, kn, args, e["match"])
        assert not is_null(fl, e), where
        rs = runs(p, fl, e)
        rows = len(p[0])
        if kn in ("ins", "longins"):                                                 # (a), (d): one I run of exactly n on the planted rows
            assert [r for r in rs if r[0] != "M"] == [("I", args["n"], args["row"], r[3]) for r in rs if r[0] == "I"], where
            assert sum(r[0] == "I" for r in rs) == 1, where
            seen[(kn, args["n"])] += 1
            if kn == "longins":
                assert args["n"] > 511 and args["row"] <= STRIP < args["row"] + args["n"] - 1
        elif kn in ("del", "longdel"):                                               # (b), (c): one D run of exactly n at the planted column
            assert [r for r in rs if r[0] != "M"] == [("D", args["n"], args["row"], args["col"])], where
            seen[(kn, args["n"])] += 1
            if kn == "longdel":
                assert args["n"] > 511
        elif kn.startswith("overhang"):                                              # (e)
            m, kk = e["match"], args["k"]
            assert len(e["score"]) == 8, where
            if kn == "overhang_left":
                assert m.startswith(b"X" * kk) and m[kk:kk + 1] != b"X" and e["score"][6] == kk, where
            else:
                assert m.endswith(b"Y" * kk) and m[-kk - 1:-kk] != b"Y" and e["score"][7] == kk, where
            seen[(kn, kk, rows)] += 1
        else:                                                                        # (f): every '-' on the path stands for 128 D
            g = args["gaps"]
            assert p[1].count(b"-") == g and kn.startswith("gap")
            steps = rows + g                                                         # one step per read base and one per '-'
            assert len(e["match"]) == steps - g + 128 * g and e["match"].count(b"D") == 128 * g, where
            assert b"-" not in e["match"]
            seen[kn] += 1
    for n in P.INS_N:
        assert seen[("ins", n)] == len(P.ins_rows(n))
    for n in P.DEL_N:
        assert seen[("del", n)] == 3
    assert seen[("longdel", 520)] == seen[("longdel", 600)] == 2 and seen[("longins", 520)] == 1
    for kk in (1, 5, 70):
        assert seen[("overhang_left", kk, MAX_ROWS)] == seen[("overhang_right", kk, MAX_ROWS)] == 1
    assert seen[("overhang_right", 70, 530)] == 1                                    # begins in strip 0 (row 461), ends in strip 1
    assert seen[("overhang_right", 5, STRIP)] == 2                                   # rows 508..512: the strip's last lane, in the last column
    assert seen["gap64"] == seen["gap65"] == seen["gap64_65"] == seen["gap65_600"] == 1
    # the insertion runs touch the border from both sides and straddle it
    ends = {(args["row"] + args["n"] - 1) for k, kn, args, p, fl, e in by_kind("walk") if kn == "ins"}
    starts = {args["row"] for k, kn, args, p, fl, e in by_kind("walk") if kn == "ins"}
    assert {STRIP - 1, STRIP} <= ends and STRIP + 1 in starts
    for n in P.INS_N[1:]:
        r = P.ins_rows(n)["straddle"]
        assert r <= STRIP and r + n - 1 >= STRIP + 1
    for c in (64, 65):
        assert any(p[1][c - 1:c] == b"-" and p[2] == 0 for k, kn, args, p, fl, e in by_kind("walk") if kn.startswith("gap"))


def test_mixed_launch_holds_what_it_claims():
    probs, flags, kinds, exp = P.answers("mixed")
    names = collections.Counter(kind_args(k)[0] for k in kinds)
    assert names["tall"] == 12 and names["small"] >= 300 and names["overflow"] == 1
    assert names["bad_rows"] == names["bad_columns"] == names["bad_columns_zero"] == 1
    tall = [k for k, kd in enumerate(kinds) if kd.startswith("tall")]
    assert tall[0] == 0 and tall[-1] >= len(kinds) - 2 and all(513 <= len(probs[k][0]) <= MAX_ROWS for k in tall)
    for k, kd in enumerate(kinds):
        p, fl = probs[k], flags[k]
        if kd == "bad_rows":
            assert len(p[0]) == MAX_ROWS + 1
        elif kd == "bad_columns":
            assert P.columns_of(p, fl) == MAX_COLS + 1 and not fl & M.CLAMP_WINDOW
        elif kd == "bad_columns_zero":
            assert P.columns_of(p, fl) == 0
        elif kd.startswith("overflow"):
            assert len(exp[k]["match"]) > P.MIXED_STRIDE                             # the one string that does not fit
        elif exp[k]["match"] is not None:
            assert len(exp[k]["match"]) <= P.MIXED_STRIDE
    assert 0 < sum(is_null(f, e) for f, e in zip(flags, exp) if e is not None) < len(probs) // 2


def test_one_wave_launch_alternates_shapes_and_outcomes():
    probs, flags, kinds, exp = P.answers("one_wave")
    out = collections.Counter()
    for k, (p, fl, kd, e) in enumerate(zip(probs, flags, kinds, exp)):
        kn, args = kind_args(kd)
        assert (len(p[0]), P.columns_of(p, fl)) == (args["rows"], args["cols"])
        if k:
            assert len(p[0]) != len(probs[k - 1][0])                                 # no two neighbours of one shape
        dead = null_branch(p, fl, e) == "middle"
        if kn == "dies" and args["rows"] > 3:
            assert dead, (k, kd)
        out[(args["rows"] > 3, "dead" if dead else "null" if is_null(fl, e) else "unlimited" if e["fill_kind"] else "limited")] += 1
    print("one wave:", dict(out))
    assert len(probs) == 42 and out[(True, "dead")] >= 8 and out[(True, "limited")] >= 8 and out[(True, "unlimited")] >= 8
    assert {(len(p[0]), P.columns_of(p, f)) for p, f in zip(probs, flags)} == {(1030, 1200), (3, 20), (513, 530), (600, 664)}


@pytest.mark.parametrize("name", ["banded_ratio", "banded_width"])
def test_banded_launch_has_limited_and_unlimited_fills(name):
    probs, flags, kinds, exp = P.answers(name)
    limited = sum(e["fill_kind"] == 0 for e in exp)
    nulls = sum(is_null(f, e) for f, e in zip(flags, exp))
    print("%s: %d jobs, %d limited (banded), %d without a result" % (name, len(probs), limited, nulls))
    assert len(probs) == 60 and all(60 <= len(p[0]) <= 600 for p in probs)
    assert limited >= 30 and len(probs) - limited >= 15 and 0 < nulls < limited
