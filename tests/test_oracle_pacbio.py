"""CPU checks of the PacBio variant of the DP restatement (oracle/liboracle_pacbio.so): the constants and the
hand-derivable values of current/align2/MultiStateAligner9PacBio.java."""
import numpy as np
import pytest

from oracle.oracle import OracleMSA, lib_pacbio


def test_pacbio_tables_and_offsets():
    L = lib_pacbio()
    # calcDelScoreOffset / calcInsScoreOffset (:2254-2310), 9 score-offset bits
    assert L.orc_calc_del_score_offset(1) == -292 * 512
    assert L.orc_calc_del_score_offset(5) == (-292 - 4 * 37) * 512
    assert L.orc_calc_del_score_offset(30) == (-292 - 4 * 37 - 15 * 17 - 10 * 2) * 512
    assert L.orc_calc_del_score_offset(90) == (-292 - 4 * 37 - 15 * 17 - 60 * 2 - ((90 - 80 + 3) // 4) * 1) * 512
    assert L.orc_calc_ins_score_offset(1) == -205 * 512
    assert L.orc_calc_ins_score_offset(25) == (-205 - 4 * 42 - 15 * 23 - 5 * 8) * 512


def test_pacbio_column_zero_follows_the_constructor():
    om = OracleMSA(40, 50, scheme="9pacbio")
    W = 51
    col0 = np.ctypeslib.as_array(om.s.packed, shape=(3 * 41 * W,))[:41 * W:W] // 512
    exp = [0, -205]
    for i in range(2, 41):
        exp.append(exp[-1] + (-42 if i < 5 else (-23 if i < 20 else -8)))     # :91-98, tiers by `i<LIMIT`
    assert col0.tolist() == exp


def test_pacbio_perfect_and_one_substitution():
    om = OracleMSA(120, 160, scheme="9pacbio")
    rng = np.random.default_rng(4)
    g = bytes(rng.choice(list(b"ACGT"), 300).astype(np.uint8))
    rd = g[100:200]
    r = om.fillUnlimited(rd, g, 90, 215)
    assert r == [100, 110, 0, 90 + 99 * 100]
    assert om.traceback(rd, g, 90, 215, r[0], r[1], r[2]) == b"m" * 100
    bad = bytearray(rd)
    bad[50] = ord("A") if bad[50] != ord("A") else ord("C")
    r = om.fillUnlimited(bytes(bad), g, 90, 215)
    # 50 matches (90 + 49*100), SUB after a streak > 1 (-137), then match restarts at 90 and 48 more at 100
    assert r[3] == (90 + 49 * 100) - 137 + 90 + 48 * 100


def _unlimited(om, rd, g, a, b):
    """fillUnlimited, and the rows / columns fields as MultiStateAligner9PacBio.fillUnlimited leaves them (:622-623) for the walkers
    ('Y' where col >= columns); the restatement's entry follows the 11ts JNI class, which does not set them (final stage)."""
    r = om.fillUnlimited(rd, g, a, b)
    om.s.rows, om.s.columns = len(rd), b - a + 1
    return r


def _flanked(seed):
    """1200 random bases and the two 100-base flanks cut from them; the bases next to the cut are chosen so that the indel cannot
    slide (a slide would be an equally good alignment somewhere else)."""
    rng = np.random.default_rng(seed)
    return bytearray(bytes(rng.choice(list(b"ACGT"), 1200).astype(np.uint8))), rng


FLANKS = (90 + 99 * 100) + (90 + 99 * 100)      # each flank: MATCH for its first base, MATCH2 for the other 99 (:327-329: after an
#                                                 indel the match plane is entered with scoreD / scoreI + POINTS_MATCH, not MATCH2)


@pytest.mark.parametrize("n,penalty", [
    # calcInsScore's tiers as the fill charges them (:499-501): INS, then INS2 while the streak is < 5, INS3 while < 20, INS4 after
    (4, -205 - 3 * 42), (5, -205 - 4 * 42), (6, -205 - 4 * 42 - 23),
    (19, -205 - 4 * 42 - 14 * 23), (20, -205 - 4 * 42 - 15 * 23), (21, -205 - 4 * 42 - 15 * 23 - 8)])
def test_pacbio_insertion_tiers(n, penalty):
    g, rng = _flanked(10 + n)
    ins = bytearray(bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8)))
    ins[0] = next(x for x in b"ACGT" if x != g[400])                       # (cannot slide right)
    ins[-1] = next(x for x in b"ACGT" if x != g[399] and (n > 1 or x != g[400]))   # (nor left)
    rd = bytes(g[300:400] + ins + g[400:500])
    g = bytes(g)
    om = OracleMSA(260, 320, scheme="9pacbio")
    r = _unlimited(om, rd, g, 290, 515)
    assert r[3] == FLANKS + penalty
    assert om.traceback(rd, g, 290, 515, r[0], r[1], r[2]) == b"m" * 100 + b"I" * n + b"m" * 100


@pytest.mark.parametrize("n,penalty", [
    # :431-435: DEL, then DEL2 while the streak is < 5, DEL3 while < 20, DEL4 while < 80, then DEL5 on every streak that is a
    # multiple of 4 (80: one for a run of 81..84) and nothing in between
    (4, -292 - 3 * 37), (5, -292 - 4 * 37), (6, -292 - 4 * 37 - 17),
    (19, -292 - 4 * 37 - 14 * 17), (20, -292 - 4 * 37 - 15 * 17), (21, -292 - 4 * 37 - 15 * 17 - 2),
    (80, -292 - 4 * 37 - 15 * 17 - 60 * 2), (84, -292 - 4 * 37 - 15 * 17 - 60 * 2 - 1)])
def test_pacbio_deletion_tiers(n, penalty):
    g, rng = _flanked(40 + n)
    g[400 + n] = next(x for x in b"ACGT" if x != g[400])                   # (the run cannot slide right)
    g[400 + n - 1] = next(x for x in b"ACGT" if x != g[399])               # (nor left)
    g = bytes(g)
    rd = g[300:400] + g[400 + n:500 + n]
    om = OracleMSA(220, 320, scheme="9pacbio")
    r = _unlimited(om, rd, g, 290, 515 + n)
    assert r[3] == FLANKS + penalty
    assert om.traceback(rd, g, 290, 515 + n, r[0], r[1], r[2]) == b"m" * 100 + b"D" * n + b"m" * 100


def test_pacbio_deletion_of_520_wraps_the_time_field():
    """The deletion plane's streak lives in 9 bits.  :480: `if(time>MAX_TIME){time=MAX_TIME-MASK5;}`: the 512th cell of the run stores
    508, not 512, and the run goes on 509, 510, 511, 508, ...  The cell of run length L is charged by the streak of the cell before
    it (:431-435), DEL5 where that streak is >= 80 and a multiple of 4:
      L = 81..511 : streak L - 1 = 80..510, multiples of 4: 80, 84, .., 508                      -> 108 x DEL5
      L = 512..520: streaks 511, 508, 509, 510, 511, 508, 509, 510, 511 (wrapped), two are 508   ->   2 x DEL5
    The wrap keeps the streak's phase (512 = 508 mod 4), so the sum equals the unwrapped one; a field clamped at 511 would charge
    nothing after L = 511 (-923 in all), a field that overflowed into 0 would open a new deletion (-292) at L = 513."""
    n = 520
    penalty = -292 - 4 * 37 - 15 * 17 - 60 * 2 - 108 - 2
    assert penalty == -925
    g, rng = _flanked(77)
    g[400 + n] = next(x for x in b"ACGT" if x != g[400])
    g[400 + n - 1] = next(x for x in b"ACGT" if x != g[399])
    g = bytes(g)
    rd = g[300:400] + g[400 + n:500 + n]
    om = OracleMSA(220, 800, scheme="9pacbio")
    r = _unlimited(om, rd, g, 290, 515 + n)
    assert r[3] == FLANKS + penalty
    assert om.traceback(rd, g, 290, 515 + n, r[0], r[1], r[2]) == b"m" * 100 + b"D" * n + b"m" * 100
    W = 801                                                                # the stored times along the run (row 100, deletion plane)
    dplane = np.ctypeslib.as_array(om.s.packed, shape=(3, 221, W))[1]
    times = (dplane[100, 110 + 1:110 + n + 1] & 511).tolist()             # row 100 ends the first flank at column 110
    assert times[:511] == list(range(1, 512)) and times[511:] == [508, 509, 510, 511, 508, 509, 510, 511, 508]


def _column_zero_after_a_fill_of_max_columns(scheme, perfect):
    om = OracleMSA(40, 60, scheme=scheme)
    col0 = np.ctypeslib.as_array(om.s.packed, shape=(3, 41, 61))[:, :, 0].copy()
    rng = np.random.default_rng(8)
    g = bytes(rng.choice(list(b"ACGT"), 200).astype(np.uint8))
    res, _ = om.fill_limited_raw(g[70:110], g, 60, 119, 1500)                # 40 rows, 60 columns: the widest window of this object
    assert res[4] == 0 and res[3] == perfect
    return col0, np.ctypeslib.as_array(om.s.packed, shape=(3, 41, 61))[:, :, 0].copy()      # (the object goes with this frame)


def test_limited_fill_of_max_columns_keeps_column_zero():
    """The row-end sentinel of fillLimitedX goes to packed[..][row-1][col+1] (:553-559).  With columns == maxColumns that is one past
    the row: Java's int[][][] has no such element.  The restatement's planes are flat, where the write landed on column 0 of the
    next row, and every later fill on the same object started from a spoilt seed column (found as a 4-cell difference in
    `iterations` two jobs later).  The PacBio build leaves the write out."""
    before, after = _column_zero_after_a_fill_of_max_columns("9pacbio", 90 + 39 * 100)
    assert (after == before).all()


def test_11ts_restatement_keeps_the_jni_write_onto_column_zero():
    """The 11ts class fills through its JNI C, whose planes are flat as well: jni/MultiStateAligner11tsJNI.c:660-667 does write
    (row-1) * (maxColumns+1) + col + 1, column 0 of `row`.  That is the reference's behaviour, and the 11ts build restates it."""
    before, after = _column_zero_after_a_fill_of_max_columns("11ts", 70 + 39 * 100)
    assert (after != before).any() and (after[:, 0] == before[:, 0]).all()
