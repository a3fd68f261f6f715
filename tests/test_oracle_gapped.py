"""The job sets of tests/gapped_problems.py against the oracle alone (no GPU): every set holds what it was planted for, so the
device tests (tests/test_msa_gapped_edges_gpu.py) cannot pass by missing their targets; the reference's own assertions about its
coordinate translation (MultiStateAligner11tsJNI.java:510-522) hold on every answered job; and the oracle answers "does not fit"
instead of writing past its planes where a gapped reference has more columns than the aligner (the guard in orc_fill_limited /
orc_fill_unlimited)."""
import random

import pytest

from oracle.oracle import OracleMSA
from tests import gapped_problems as G
from tests.msa_check import gapped_expected, gapped_set, oracle_align_gapped

SCHEMES = ("11ts", "9pacbio")
GAPC = ord("-")


def answered(scheme, name):
    probs, flags, kinds = gapped_set(scheme, name)
    return [(p, f, k, e) for p, f, k, e in zip(probs, flags, kinds, gapped_expected(scheme, name)) if e is not None]


def from_gapped(gref, point):
    """translateFromGappedCoordinate (:759-779), restated here a second time."""
    buf, lim, lim2, origin = gref
    if point <= 0:
        return origin + point
    j = origin
    for i in range(lim2):
        if i == point:
            return j
        j += 128 if buf[i] == GAPC else 1
    return None


def to_gapped(gref, point):
    """translateToGappedCoordinate (:781-801)."""
    buf, lim, lim2, origin = gref
    if point <= origin:
        return point - origin
    j = origin
    for i in range(lim2):
        if j == point:
            return i
        j += 128 if buf[i] == GAPC else 1
    return None


@pytest.mark.parametrize("scheme", SCHEMES)
def test_every_class_has_answered_members(scheme):
    for name in G.SETS:
        rows = answered(scheme, name)
        assert any(e["score"] is not None for _, _, _, e in rows), name
        assert all(k.split(":")[0] == name for _, _, k, _ in rows), name
    for name in ("gap_steps", "lane_sweep", "blocks"):
        rows = answered(scheme, name)
        assert sum(e["score"] is not None for _, _, _, e in rows) >= 0.9 * len(rows), name
        assert not any(e["refused"] for _, _, _, e in rows), name
    assert len(gapped_set(scheme, "lane_sweep")[0]) <= 2000
    assert all(len(gapped_set(scheme, name)[0]) <= 700 for name in G.SETS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_gap_steps_hold_every_size_and_symbol_count(scheme):
    rows = answered(scheme, "gap_steps")
    seen = {}
    for p, f, k, e in rows:
        gap = p[5][2] - p[5][1] - 1
        buf, lim, lim2, origin = e["gref"]
        seen.setdefault(gap, set()).add(buf[:lim].count(b"-"))
    assert sorted(seen) == sorted(G.GAP_STEPS)
    assert seen[256] == {1} and seen[383] == {1} and seen[384] == {2} and seen[511] == {2} and seen[512] == {3}
    assert seen[8319] == {63} and seen[8320] == {64} and seen[8321] == {64} and seen[8447] == {64} and seen[8448] == {65} and seen[16000] == {124} and seen[16383] == {126}
    for p, f, k, e in rows:                                                        # the symbols of one gap are one run
        buf, lim = e["gref"][0], e["gref"][1]
        n = buf[:lim].count(b"-")
        assert b"-" * n in buf[:lim]
    assert any("del_beside" in k and e["score"] is not None for _, _, k, e in rows)
    assert any("ins_beside" in k and e["score"] is not None for _, _, k, e in rows)
    assert {e["fill_kind"] for _, _, _, e in rows} == {0, 1}                       # both fills behind the Java gate


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lane_sweep_covers_every_residue(scheme):
    rows = answered(scheme, "lane_sweep")
    lims, firsts, stops, lims_behind, firsts_behind, stops_behind = set(), set(), set(), set(), set(), set()
    longest = 0
    for p, f, k, e in rows:
        gref = e["gref"]
        buf, lim, lim2, origin = gref
        b = min(len(p[1]) - 1, p[3])
        gstop = to_gapped(gref, b)
        assert gstop is not None and gstop == lim - 1
        # the read runs past the window: the record carries a pad hint, which is what shows the device's index of b
        assert e["score"] is not None and len(e["score"]) == 8 and e["score"][7] > 0, k
        run = buf.index(b"-")
        n = 0
        while buf[run + n] == GAPC:
            n += 1
        longest = max(longest, n)
        if "behind" in k:
            lims_behind.add(lim % 64)
            assert n >= 65 and gstop > run + n                                     # b lies behind a run that fills a whole chunk
            second = buf.index(b"-", run + n)
            firsts_behind.add(second % 64)
            stops_behind.add(gstop % 64)
        else:
            lims.add(lim % 64)
            firsts.add(run % 64)
            stops.add(gstop % 64)
    full = set(range(64))
    assert lims == full and firsts == full and stops == full
    assert lims_behind == full and firsts_behind == full and stops_behind == full
    assert longest >= 65


@pytest.mark.parametrize("scheme", SCHEMES)
def test_blocks_hold_every_even_ngaps(scheme):
    rows = answered(scheme, "blocks")
    assert {len(p[5]) for p, _, _, _ in rows} == {4, 6, 8, 10, 12, 14, 16}
    for p, f, k, e in rows:
        assert all(p[5][i + 1] - p[5][i] - 1 >= 256 for i in range(1, len(p[5]) - 1, 2)), k
        assert e["gref"][1] == G.gref_columns(p[5], max(0, p[2]), min(len(p[1]) - 1, p[3])), k
    assert max(e["gref"][1] for _, _, _, e in rows) > G.SHAPES[scheme]["maxColumns"] * 0.7


@pytest.mark.parametrize("scheme", SCHEMES)
def test_array_ends_clip_and_fill_the_cushion(scheme):
    rows = answered(scheme, "array_ends")
    left = [(p, e) for p, _, k, e in rows if ":left" in k or ":both" in k]
    right = [(p, e) for p, _, k, e in rows if ":right" in k or ":both" in k]
    assert left and all(p[2] < 0 and p[5][0] == 0 and e["gref"][3] == 0 for p, e in left)
    assert any(e["score"] is not None and e["score"][1] == 0 for p, e in left)
    assert right and all(p[3] >= len(p[1]) and p[5][-1] == len(p[1]) - 1 for p, e in right)
    assert any(e["score"] is not None and e["score"][2] == len(p[1]) - 1 for p, e in right)
    for p, e in right:                                                             # nothing behind the site: the cushion is 'N'
        buf, lim, lim2, origin = e["gref"]
        assert lim2 == lim + 127 and buf[lim:lim2 + 1] == b"N" * 128
    tails, tight = set(), 0
    for p, f, k, e in rows:
        if ":tail=" in k:
            buf, lim, lim2, origin = e["gref"]
            tails.add(len(p[1]) - 1 - p[5][-1])
            b = min(len(p[1]) - 1, p[3])                                           # the cushion starts behind the clamped window
            assert buf[lim:lim2 + 1] == p[1][b + 1:] + b"N" * (128 - (len(p[1]) - 1 - b)), k
            tight += b == p[5][-1]
    assert min(tails) == 1 and max(tails) == 127 and len(tails) >= 6 and tight >= 6


@pytest.mark.parametrize("scheme", SCHEMES)
def test_overhang_holds_pad_hints_and_starts_left_of_the_origin(scheme):
    rows = [r for r in answered(scheme, "overhang") if r[3]["score"] is not None]
    pad_left = [e for _, _, _, e in rows if len(e["score"]) == 8 and e["score"][6] > 0]
    pad_right = [e for _, _, _, e in rows if len(e["score"]) == 8 and e["score"][7] > 0]
    assert len(pad_left) >= 10 and len(pad_right) >= 10
    assert any(e["score"][6] >= 10 for e in pad_left)
    assert any(e["score"][1] < e["gref"][3] for _, _, _, e in rows)                # translated start left of grefRefOrigin
    # bestRefStop == gstop in an insertion state: the pad hint is the state's time
    ins = [(p, e) for p, _, _, e in rows if e["score"][5] == 2 and e["score"][2] == min(len(p[1]) - 1, p[3])]
    assert any(len(e["score"]) == 8 and e["score"][7] > 1 for p, e in ins)
    # fewer columns than rows - 2: the kernels that take windows narrower than the read
    deep = [(p, e) for p, _, k, e in answered(scheme, "overhang") if ":deep" in k]
    assert deep and all(e["gref"][1] + 1 < len(p[0]) - 2 for p, e in deep)
    assert any(e["score"] is not None for p, e in deep)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_modes_hold_every_mode_and_the_null_fill(scheme):
    rows = answered(scheme, "modes")
    assert {f for _, f, _, _ in rows} == set(G.MODES)
    null = [e for _, _, k, e in rows if k.endswith(":null")]
    assert sum(e["status"] == 1 for e in null) >= 4                                # the limited fill, out of reach
    assert any(e["status"] == 0 and e["fill_kind"] == 1 for e in null)             # too wide for it: fillUnlimited never returns null
    for fl in G.MODES:
        mine = [e for _, f, k, e in rows if f == fl and not k.endswith((":null", ":tight"))]
        assert all(e["score"] is not None for e in mine)
        assert all((e["match"] is not None) == bool(fl & 32) for e in mine)
        if fl & 7 == 1:
            assert all(e["fill_kind"] == 1 for e in mine)
        else:
            assert {e["fill_kind"] for e in mine} == {0, 1}
    tight = [e for _, _, k, e in rows if k.endswith(":tight")]
    assert any(e["score"] is not None and e["fill_kind"] == 0 for e in tight)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_the_references_own_assertions_hold(scheme):
    """:510-522: from(to(a)) == a, from(to(b)) == b, to(a) == 0, score[1] and score[2] survive the round trip; and the string
    :481-493 expand is the kept string with every '-' as 128 'D' (127 bytes longer per symbol)."""
    checked = strings = 0
    for name in G.SETS:
        for p, f, k, e in answered(scheme, name):
            if e["gref"] is None or e["score"] is None:
                continue
            gref = e["gref"]
            a, b = max(0, p[2]), min(len(p[1]) - 1, p[3])
            ga, gb = to_gapped(gref, a), to_gapped(gref, b)
            assert ga == 0 and gb is not None, k
            assert from_gapped(gref, ga) == a and from_gapped(gref, gb) == b, k
            for w in (1, 2):
                point = to_gapped(gref, e["score"][w])
                assert point is not None and from_gapped(gref, point) == e["score"][w], k
            checked += 1
            if e["match"] is not None:
                n = e["kept"].count(b"-")
                assert e["match"] == e["kept"].replace(b"-", b"D" * 128), k
                assert len(e["match"]) - len(e["kept"]) == 127 * n and e["match"].count(b"D") - e["kept"].count(b"D") == 128 * n, k
                assert b"-" not in e["match"], k
                strings += n > 0
    assert checked > 550 and strings > 500


def test_fit_contexts_refuse_below_greflimit_plus_one_columns():
    for scheme in SCHEMES:
        probs, flags, kinds, lim = G.fit(scheme)
        sh = G.SHAPES[scheme]
        for delta in G.FIT_DELTAS + (G.FIT_SMALL - lim,):
            maxColumns = lim + delta
            om = OracleMSA(sh["maxRows"], maxColumns, scheme=scheme)
            for p, f, k in zip(probs, flags, kinds):
                e = oracle_align_gapped(om, p[0], p[1], p[2], p[3], p[4], G.gaps_of(p), f)
                if k == "fit:plain":
                    assert not e["refused"] and e["score"] is not None, (delta, k)
                    continue
                assert e["refused"] == (delta < 1), (scheme, delta, k)
                if delta >= 1:
                    buf, glim, lim2, origin = e["gref"]
                    assert glim == lim and lim2 == maxColumns + 1 and e["score"] is not None      # a cushion of 1 or 2 bytes
                made = om.makeGref(p[1], p[5], max(0, p[2]), p[3])
                assert (made is None) == (lim > maxColumns + 2), (scheme, delta)                    # makeGref itself: only past its buffer


def test_oracle_answers_where_the_gapped_reference_is_one_column_over():
    """The job of the issue this guard came from: greflimit 331 needs 332 columns; OracleMSA(224, 331) ran 332 columns over planes
    of 331 and took the process down."""
    rng = random.Random(1)
    ref = bytes(rng.choice(b"ACGT") for _ in range(4000))
    st, L, cut, dl = 1000, 150, 70, 300
    rd = ref[st:st + cut] + ref[st + cut + dl:st + dl + L]
    g = [st, st + cut - 1, st + cut + dl, st + dl + L - 1]
    args = (rd, ref, st - 4, g[-1] + 4, 5000, g)
    assert OracleMSA(224, 1600).makeGref(ref, g, st - 4, g[-1] + 4) == 331
    sv, mx = OracleMSA(224, 332).fillAndScoreLimited(*args)
    assert sv is not None and sv == OracleMSA(224, 1600).fillAndScoreLimited(*args)[0]
    om = OracleMSA(224, 331)
    assert om.fillAndScoreLimited(*args) == (None, None)
    assert om.fillLimited(rd, ref, st - 4, g[-1] + 4, 5000, g) is None
    assert om.fillUnlimited(rd, ref, st - 4, g[-1] + 4, g) is None
    assert om.fillLimited(rd[:100], ref, st - 4, st + 103, 3000) is not None       # and goes on answering


def test_traceback_returns_the_string_of_a_16_kb_gap():
    rng = random.Random(2)
    ref = bytes(rng.choice(b"ACGT") for _ in range(20000))
    st, L, cut, dl = 1000, 150, 70, 16000
    rd = ref[st:st + cut] + ref[st + cut + dl:st + dl + L]
    g = [st, st + cut - 1, st + cut + dl, st + dl + L - 1]
    om = OracleMSA(224, 1600)
    sv, mx = om.fillAndScoreLimited(rd, ref, st - 4, g[-1] + 4, 5000, g)
    assert sv is not None and sv[1] == st and sv[2] == g[-1]
    tb = om.traceback(rd, ref, st - 4, g[-1] + 4, mx[0], mx[1], mx[2], gapped=True)
    kept = om.traceback(rd, ref, st - 4, g[-1] + 4, mx[0], mx[1], mx[2], gapped=True, keep_gaps=True)
    assert kept.count(b"-") == 124 and tb == kept.replace(b"-", b"D" * 128)
    assert tb.count(b"m") == L and tb.count(b"D") == dl                            # the whole deletion, base for base


def test_refused_set_holds_every_refusal():
    probs, flags, kinds = gapped_set("11ts", "refused")
    names = {k.split(":")[1] for k in kinds if G.is_refused(k)}
    assert names == {"ngaps1", "ngaps3", "ngaps17", "descending", "descending_last", "negative", "past_end", "past_end_inner",
                     "gap127", "gap0", "window_reversed"}
    recs = G.gap_records(probs)
    by = {k.split(":")[1]: (p, r) for p, k, r in zip(probs, kinds, recs) if G.is_refused(k)}
    assert [by[n][1]["ngaps"] for n in ("ngaps1", "ngaps3", "ngaps17")] == [1, 3, 17]
    p, r = by["gap127"]
    assert r["gaps"][2] - r["gaps"][1] - 1 == 127
    p, r = by["past_end"]
    assert r["gaps"][3] == len(p[1])
    p, r = by["negative"]
    assert r["gaps"][0] < 0
    p, r = by["window_reversed"]
    assert p[3] < p[2]
    # each stands between two good jobs, and the plain jobs with ngaps 0 / -1 are there
    for i, k in enumerate(kinds):
        if G.is_refused(k):
            assert kinds[i - 1] == "refused:neighbour" and not G.is_refused(kinds[i + 1])
    assert sorted(int(r["ngaps"]) for k, r in zip(kinds, recs) if k.startswith("refused:pass")) == [-1, 0]
    exp = gapped_expected("11ts", "refused")
    assert all(e is not None and e["score"] is not None for k, e in zip(kinds, exp) if not G.is_refused(k))
