"""Known answers for tests/sam_splice_check.py (the restatement the spliced-read GPU tests compare the device with) and for the optional
tags of bbmap_amd/sam.py, and the tie of that restatement to tests/sam_check.py (pinned by hand in tests/test_sam_cpu.py).

Every expected value in the hand cases was derived from the Java text, not from running any code (c = count, r = refloc; the MD
chromosome is "ACGT" x 10 with the scaffold at [0, 40) and refstart 4, as in test_sam_cpu.py):

toCigar14 (current/stream/SamLine.java:679-750) with INTRON_LIMIT
  4 m, 12 D, 4 m at readStart 10: "4=" at the first D; at the next m `lastMode=='D' && count>INTRON_LIMIT`: 12 > 10 -> "12N", 12 > 12 is
      false -> "12D"; final "4=".
  4 m, 11 D, the string ends: the final append (:737-742) tests `mode=='D' && count>INTRON_LIMIT` -> "4=11N" at limit 10.
  3 m, 11 D at readStart 87, reflen 100: r 87..89 '='; D at r 90..99 are ten columns of mode D; the eleventh D stands at r 100: clipped,
      mode S, "10D" is appended (10 > 10 is false: the clipped column is not counted, so limit + 1 columns print D) and sfdflag keeps the
      new count 0; final "0S" -> "3=10D0S".  With 2 m behind it: both clipped -> "3=10D2S".
  2 m, 11 D, 4 m at readStart -5: m m clipped (c 2, r -3); D at r -3, -2, -1 clipped, not counted (c 2, r 0); eight D at r 0..7 ->
      "2S", c 8; m -> "8D" at limit 10, "8N" at limit 7 (8 > 7); final "4=".
NM (:1514-1535): delsCurrent <= INTRON_LIMIT is added at the first non-D column and reset either way: 12 D at limit 10 -> 0, at limit
  12 -> 12.  2 m, 12 D, 2 m, 2 D, 2 m at limit 10: the first run is dropped and reset, the second adds 2.
makeMdTag (:1361-1445): at the flush `dels<=INTRON_LIMIT` fails for 12 > 10: nothing is appended, count is not reset and dels is not
  reset.  4 m, 12 D, 4 m -> count runs to 8 -> "8"; at limit 12 the flush prints "4" "^" ref[8..20) = ACGTACGTACGT, then "4".
  2 m, 12 D, 2 m, 2 D, 2 m: at the second flush dels is 12 + 2 = 14 > 10 again -> dropped as well, count runs to 6 -> "6".
Read.identityFlat (current/stream/Read.java:1529-1596): a D run is bad when `current<INTRON_LIMIT`: 12 < 10 no, 12 < 12 no, 12 < 13
  yes -> bad 0, 0, 12; good 8.  Read.countErrors (:2189-2240): splice++ when the streak of D equals max(minSplice, 1): 12 reaches 10 and
  12, not 13 -> 1, 1, 0.
makeIdentityTag (:1326-1330): good 1, bad 31: f = 1/32 exactly, 100*f = 3.125 exactly; Java's %.2f rounds HALF_UP -> "3.13" (Python's
  own % gives 3.12).  good 13, bad 19: 40.625 -> "40.63".
makeXSTag (:1346-1359): plus = strand==PLUS; inverted for pairnum 1; inverted for XS_SECONDSTRAND.
makeStopTag / makeLengthTag (:1316-1324) on "2S8D4=" of a 6-base read at POS 1: calcCigarLength with soft clips 2 + 8 + 4 = 14 -> YS =
  1 + 14 - 1 = 14; YL = 6 - 2 = 4 and 8 + 4 = 12.  On "4=12N4=" of an 8-base read at POS 11: N counts as reference length, 20 -> YS 30,
  YL 8,20."""
import numpy as np

from bbmap_amd import reference as R
from bbmap_amd import sam as SAM
from tests import sam_check as SK
from tests import sam_splice_check as SP
from tests import scaffold_check as SC

CHROM = np.frombuffer(b"ACGT" * 10, np.uint8)
FIN = np.dtype([("mapped", "<i4"), ("chrom", "<i4"), ("strand", "<i4"), ("start", "<i4"), ("stop", "<i4"), ("mapScore", "<i4"),
                ("paired", "<i4"), ("ambiguous", "<i4"), ("perfect", "<i4")])
M12 = b"mmmm" + b"D" * 12 + b"mmmm"
CARRY = b"mm" + b"D" * 12 + b"mm" + b"DD" + b"mm"


def _md(m, limit):
    return SP.make_md_tag(CHROM, 4, m, np.frombuffer(b"A" * 16, np.uint8), 0, 40, limit)


def test_three_thresholds_on_one_run_derived_by_hand():
    assert SP.to_cigar(M12, 10, 29, 1000, False, 10) == "4=12N4="
    assert SP.to_cigar(M12, 10, 29, 1000, True, 10) == "4M12N4M"
    assert SP.calc_nm(M12, "4=12N4=", 8, 10) == 0
    assert _md(M12, 10) == "8"
    assert SP.identity_counts(M12, 10) == (8, 0) and SP.count_splices(M12, 10) == 1
    assert SP.to_cigar(M12, 10, 29, 1000, False, 12) == "4=12D4="
    assert SP.calc_nm(M12, "4=12D4=", 8, 12) == 12
    assert _md(M12, 12) == "4^ACGTACGTACGT4"
    assert SP.identity_counts(M12, 12) == (8, 0) and SP.count_splices(M12, 12) == 1        # 12 < 12 is false
    assert SP.identity_counts(M12, 13) == (8, 12) and SP.count_splices(M12, 13) == 0


def test_md_carry_over_derived_by_hand():
    assert SP.to_cigar(CARRY, 10, 29, 1000, False, 10) == "2=12N2=2D2="
    assert SP.calc_nm(CARRY, "2=12N2=2D2=", 6, 10) == 2
    assert _md(CARRY, 10) == "6"
    assert _md(CARRY, 12) == "2^GTACGTACGTAC2^AC2"          # (both printed: ref[6..18), ref[20..22))


def test_final_append_and_clipped_columns_derived_by_hand():
    assert SP.to_cigar(b"mmmm" + b"D" * 11, 10, 24, 1000, False, 10) == "4=11N"
    assert SP.to_cigar(b"mmmm" + b"D" * 11, 10, 24, 1000, True, 10) == "4M11N"
    assert SP.to_cigar(b"mmm" + b"D" * 11, 87, 100, 100, False, 10) == "3=10D0S"
    assert SP.to_cigar(b"mmm" + b"D" * 11 + b"mm", 87, 102, 100, False, 10) == "3=10D2S"
    assert SP.to_cigar(b"mmm" + b"D" * 11 + b"mm", 87, 102, 100, False, 9) == "3=10N2S"
    assert SP.to_cigar(b"mm" + b"D" * 11 + b"mmmm", -5, 11, 100, False, 10) == "2S8D4="
    assert SP.to_cigar(b"mm" + b"D" * 11 + b"mmmm", -5, 11, 100, False, 7) == "2S8N4="


def test_cigar_lengths_and_identity_text_derived_by_hand():
    assert SP.calc_cigar_length("2S8D4=", True) == 14 and SP.calc_cigar_length("2S8D4=", False) == 12
    assert SP.count_leading_clip_cigar("2S8D4=") == 2 and SP.count_leading_clip_cigar("4=2S") == 0
    assert SP.calc_cigar_length("4=12N4=", False) == 20
    m = b"m" + b"S" * 31
    assert SP.identity_counts(m, SP.INT_MAX) == (1, 31)
    assert SP.identity_text(1, 31, False) == "YI:f:3.13" and "%.2f" % 3.125 == "3.12"
    assert SP.identity_text(13, 19, False) == "YI:f:40.63"
    assert SP.identity_text(8, 0, False) == "YI:f:100.00" and SP.identity_text(0, 0, True) == "YI:f:100"
    assert SAM.identity_tag(1, 31, False) == "YI:f:3.13" and SAM.identity_tag(13, 19, False) == "YI:f:40.63"
    assert SAM.identity_tag(0, 0, True) == "YI:f:100"
    assert SP.identity_counts(b"mmNNNNNmmCC", SP.INT_MAX) == (4 + 2, 6)          # n = (5 + 3) / 4 = 2: good += 2, bad += 6; C is skipped


def _scaf(rows):
    s = np.zeros(len(rows), SC.SCAFREC_DTYPE)
    for i, row in enumerate(rows):
        for k, v in row.items():
            s[i][k] = v
    return s


def _fin(rows):
    f = np.zeros(len(rows), FIN)
    for i, row in enumerate(rows):
        for k, v in row.items():
            f[i][k] = v
    return f


HIT = dict(mapped=1, chrom=1, strand=0, start=14, stop=33, mapScore=700)
ON = dict(scaffold=0, start=10, stop=29, pos=11, end=30, scaflen=36, flags=SC.MAPPED | SC.INBOUNDS)
CALL = np.frombuffer(b"A" * 8, np.uint8)


def test_whole_line_with_every_tag_derived_by_hand():
    fin, scaf = _fin([HIT]), _scaf([ON])
    recs, tg, text, strings = SP.sam_records(None, fin, [M12], [8], [CALL], [CHROM], False, SP.MD, 10, SP.ALL_TAGS, scaf=scaf)
    assert strings == [("4=12N4=", "8")] and text == b"4=12N4=8"
    t = tg[0]
    assert int(recs[0]["nm"]) == 0 and int(t["xs"]) == 1 and int(t["introns"]) == 1 and int(t["splices"]) == 1
    assert (int(t["ys"]), int(t["yl_query"]), int(t["yl_ref"])) == (30, 8, 20)
    assert (int(t["yi_good"]), int(t["yi_bad"]), int(t["yi_perfect"])) == (8, 0, 0)
    assert int(t["nh"]) == 1 and int(t["yr"]) == 700 and int(t["xm"]) == 1 and int(t["xb"]) == ord("I")
    assert int(t["present"]) == SP.ALL_TAGS & ~(SP.NM | SP.AM | SP.INSERT)              # no X8 without a mate
    mapq = int(recs[0]["mapq"])
    line = SAM.lines(recs, np.frombuffer(text, np.uint8), ["r"], [CALL], None, ["s0"], False, tags=tg)[0].split("\t")
    assert line[:9] == ["r", "0", "s0", "11", str(mapq), "4=12N4=", "*", "0", "0"]
    assert line[11:] == ["NM:i:0", "SM:i:%d" % mapq, "AM:i:%d" % mapq, "XM:i:1", "XS:A:+", "MD:Z:8", "NH:i:1", "YS:i:30", "YL:Z:8,20",
                         "YI:f:100.00", "YR:i:700", "XB:Z:I"]
    # the same line at limit 12: no N, no XS, the run back in NM and MD
    recs, tg, text, strings = SP.sam_records(None, fin, [M12], [8], [CALL], [CHROM], False, SP.MD, 12, SP.ALL_TAGS, scaf=scaf)
    assert strings == [("4=12D4=", "4^GTACGTACGTAC4")]       # (refstart 14: ref[18..30))
    assert int(recs[0]["nm"]) == 12 and not int(tg[0]["present"]) & SP.XS and int(tg[0]["introns"]) == 0 and int(tg[0]["splices"]) == 1
    # NO_TAGS: nothing, XT and MD included; an unmapped line: nothing either
    recs, tg, text, strings = SP.sam_records(None, _fin([dict(HIT, ambiguous=1)]), [M12], [8], [CALL], [CHROM], False, SP.MD, 10,
                                             SP.ALL_TAGS | SP.NO_TAGS, scaf=scaf)
    assert strings == [("4=12N4=", None)] and int(recs[0]["nm"]) == -1 and int(recs[0]["am"]) == -1 and int(recs[0]["tags"]) == 0
    assert int(tg[0]["present"]) == 0 and int(tg[0]["introns"]) == 1
    miss = _fin([dict(mapped=0, chrom=-1, start=-1, stop=-1)])
    recs, tg, text, _ = SP.sam_records(None, miss, [None], [8], [CALL], [CHROM], False, SP.MD, 10, SP.ALL_TAGS, scaf=_scaf([dict(scaffold=-1)]))
    assert text == b"" and int(tg[0]["present"]) == 0 and int(recs[0]["nm"]) == -1


def test_xs_for_every_strand_and_mate_derived_by_hand():
    want = {(0, 0): 1, (1, 0): -1, (0, 1): -1, (1, 1): 1}            # (strand, pairnum) -> XS
    for (strand, pairnum), xs in want.items():
        rows = [dict(HIT, strand=strand), dict(HIT, strand=strand)]
        for tags, sign in ((SP.ALL_TAGS, 1), (SP.ALL_TAGS | SP.XS_SECONDSTRAND, -1)):
            _, tg, _, strings = SP.sam_records(None, _fin(rows), [M12, M12], [8, 8], [CALL, CALL], [CHROM], True, 0, 10, tags,
                                               scaf=_scaf([dict(ON, flags=ON["flags"] | SC.SAME_SCAFFOLD)] * 2))
            assert strings[pairnum][0] == "4=12N4=" and int(tg[pairnum]["xs"]) == xs * sign, (strand, pairnum, tags)
    for strand, xs in ((0, 1), (1, -1)):                             # without a mate pairnum is 0
        _, tg, _, _ = SP.sam_records(None, _fin([dict(HIT, strand=strand)]), [M12], [8], [CALL], [CHROM], False, 0, 10, SP.ALL_TAGS, scaf=_scaf([ON]))
        assert int(tg[0]["xs"]) == xs
    _, tg, _, _ = SP.sam_records(None, _fin([HIT]), [M12], [8], [CALL], [CHROM], False, 0, 12, SP.ALL_TAGS, scaf=_scaf([ON]))
    assert int(tg[0]["xs"]) == 0 and not int(tg[0]["present"]) & SP.XS   # no N, no XS


def test_pair_tags_and_splice_counts_derived_by_hand():
    # mates of 8 bases at 14..33 (plus) and 50..57 (minus) on one chromosome: PlusLeft, mid = 50 - 33 - 1 = 16 -> 16 + 8 + 8 = 32;
    # the mate unmapped (start = stop = -1 comes first and start == stop) -> 0.  XB: I + the mate's letter.
    mate = dict(mapped=1, chrom=1, strand=1, start=50, stop=57, mapScore=300)
    on2 = dict(scaffold=0, start=46, stop=53, pos=47, end=54, scaflen=36, flags=SC.MAPPED)          # b1 53 >= scaflen: out of bounds
    _, tg, _, _ = SP.sam_records(None, _fin([HIT, mate]), [M12, b"m" * 8], [8, 8], [CALL, CALL], [CHROM], True, 0, 10, SP.ALL_TAGS,
                                 scaf=_scaf([ON, on2]))
    assert [int(t["x8"]) for t in tg] == [32, 32]
    assert [int(t["xb"]) for t in tg] == [ord("I") | ord("O") << 8, ord("O") | ord("I") << 8]
    assert SAM.splice_counts(tg, True) == (1, 0) and SAM.splice_counts(tg, False) == (1, 0)
    miss = dict(mapped=0, chrom=-1, start=-1, stop=-1)
    recs, tg, _, _ = SP.sam_records(None, _fin([HIT, miss]), [M12, None], [8, 8], [CALL, CALL], [CHROM], True, 0, 10, SP.ALL_TAGS,
                                    scaf=_scaf([ON, dict(scaffold=-1)]))
    assert int(tg[0]["x8"]) == 0 and int(tg[0]["xb"]) == ord("I") | ord("U") << 8 and int(tg[1]["present"]) == 0
    assert int(recs[0]["am"]) == 0
    # XM: the top site's score twice more in the list -> 3; an ambiguous read with a list of one -> 2
    _, tg, _, _ = SP.sam_records(None, _fin([HIT, dict(HIT, ambiguous=1)]), [M12, M12], [8, 8], [CALL, CALL], [CHROM], False, 0, 10, SP.ALL_TAGS,
                                 site_scores=[[700, 700, 650, 700], [700]], scaf=_scaf([ON, ON]))
    assert [int(t["xm"]) for t in tg] == [3, 2]


# ------------------------------------------------------------------------------------------------ the tie to tests/sam_check.py
SYMS = np.frombuffer(b"mmmmmmmmSSNDDDIXYsB", np.uint8)


def _random_match(rng):
    n = int(rng.integers(1, 90))
    body = SYMS[rng.integers(0, len(SYMS), n)].copy()
    for _ in range(int(rng.integers(0, 3))):                # runs, so that D / I stretches of some length occur
        a = int(rng.integers(0, n))
        body[a: a + int(rng.integers(1, 30))] = rng.choice(np.frombuffer(b"DImS", np.uint8))
    lead, tail = (int(rng.integers(0, 6)) if rng.random() < 0.3 else 0 for _ in range(2))
    if not (lead or tail or (body != ord("D")).any()):      # (a read has at least one base)
        body[int(rng.integers(0, n))] = ord("m")
    return b"C" * lead + body.tobytes() + b"C" * tail


def test_unlimited_default_tags_equal_the_pinned_restatement():
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGTN", np.uint8)
    p = R.pack([("sA", acgt[rng.integers(0, 4, 200)]), ("sB", acgt[rng.integers(0, 4, 200)])], start_pad=20, mid_pad=30, end_pad=20)
    table = SC.table_of(p)
    total = 0
    for batch in range(400):
        paired = bool(batch & 1)
        n = 8
        matches, fin, calls = [], np.zeros(n, FIN), []
        for r in range(n):
            m = _random_match(rng)
            reflen = sum(1 for b in m if chr(b) not in "IXY")
            start = int(rng.choice([20, 250])) + int(rng.integers(-12, 205))
            mapped = rng.random() < 0.9
            fin[r] = (1, 1, int(rng.integers(0, 2)), start, start + reflen - 1, int(rng.integers(0, 9000)), int(rng.integers(0, 2)),
                      int(rng.random() < 0.2), int(rng.random() < 0.1)) if mapped else (0, -1, 0, -1, -1, 0, 0, 0, 0)
            matches.append(m if mapped and rng.random() < 0.95 else None)
            calls.append(acgt[rng.integers(0, 5, sum(1 for b in m if b != ord("D")))])
        lens = [len(c) for c in calls]
        flags = batch >> 1 & 3
        want, wtext, wstrings = SK.sam_records(table, fin, matches, lens, calls, p.chroms, paired, flags)
        got, tg, text, strings = SP.sam_records(table, fin, matches, lens, calls, p.chroms, paired, flags)
        for f in SK.SAMREC_DTYPE.names:
            assert np.array_equal(got[f], want[f]), (batch, f)
        assert text == wtext and strings == wstrings, batch
        assert not tg["present"].any() and not tg["introns"].any() and not tg["splices"].any()
        total += sum(1 for s in strings if s[0])
    assert total > 2000


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_new_entry_points_refuse_bad_arguments_before_any_device_call():
    import ctypes as C

    from bbmap_amd import _lib, build

    class bbmap_sam_config(C.Structure):
        _fields_ = [("flags", C.c_int32), ("intronLimit", C.c_int32), ("tags", C.c_int32), ("reserved", C.c_int32 * 5)]

    SAM_DEFAULT_TAGS, SAM_NO_INTRON_LIMIT = SP.NM | SP.AM, SP.INT_MAX
    build.build()
    L = C.CDLL(_lib.SO_PATH)
    L.bbmap_last_error.restype = C.c_char_p
    L.bbpipe_sam_records_workspace_bytes.restype = C.c_int64
    cfg = bbmap_sam_config()
    assert L.bbmap_sam_default_config(C.byref(cfg)) == 0
    assert (cfg.flags, cfg.intronLimit, cfg.tags, list(cfg.reserved)) == (0, SAM_NO_INTRON_LIMIT, SAM_DEFAULT_TAGS, [0] * 5)
    assert C.sizeof(cfg) == 32
    assert L.bbmap_sam_default_config(None) == -2 and L.bbmap_last_error() == b"bbmap_sam_default_config: null argument"
    assert L.bbpipe_sam_records_workspace_bytes(C.c_int64(-1), C.c_int32(100)) == -2
    assert L.bbpipe_sam_records_workspace_bytes(C.c_int64(10), C.c_int32(7000)) == -2
    raw = lambda n, cfgp: L.bbpipe_sam_records_device(None, C.c_int64(n), C.c_int32(1), cfgp, C.c_int32(150), *([None] * 7), C.c_int32(0),
                                                      *([None] * 5), C.c_int64(0), None, None, C.c_int64(0))
    assert raw(3, C.byref(cfg)) == -2 and L.bbmap_last_error() == b"bbpipe_sam_records_device: bad argument"      # an odd count of mates
    assert raw(2, None) == -2 and L.bbmap_last_error() == b"bbpipe_sam_records_device: null argument"
    cfg.intronLimit = -1
    assert raw(2, C.byref(cfg)) == -2 and L.bbmap_last_error() == b"bbpipe_sam_records_device: negative intron limit"
    cfg.intronLimit, cfg.tags = 10, 1 << 14
    assert raw(2, C.byref(cfg)) == -2 and L.bbmap_last_error() == b"bbpipe_sam_records_device: unknown tag bits"
    cfg.tags = SAM_DEFAULT_TAGS
    assert raw(2, C.byref(cfg)) == -2 and L.bbmap_last_error() == b"bbpipe_sam_records_device: null buffer"         # no device word for the size
    assert L.bbmap_get_sam_records_cfg(None, None, C.byref(cfg), None, None, None, None) == -2
    assert L.bbmap_get_sam_cfg(None, C.c_int64(0), C.byref(cfg), None, None, None, C.c_int64(0), None) == -2
