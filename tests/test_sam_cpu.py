"""Known answers for tests/sam_check.py (the restatement the GPU test compares the device with) and for bbmap_amd/sam.py.

Every expected value below was derived by hand from the Java text of current/stream/SamLine.java, not from running any code.  The
derivations (c = count, r = refloc / rpos, chromosome of the MD cases = "ACGT" x 10 with the scaffold at [0, 40), refstart 4):

toCigar14 / toCigar13 (:679-750 / :600-663)
  "mmmSmmDDmmImm", readStart 10, reflen 1000: three '=' (c 3); S -> mode X: append "3="; m -> "1X"; two '='; D -> "2="; two D; m -> "2D";
      two '='; I -> "2="; m -> "1I"; two '=' and the final append "2=".  1.3: m m m S m m are all M -> "6M", then "2D" "2M" "1I" "2M".
  "CCmmmmCC": C is mode S and moves refloc -> "2S4=2S".
  eight m at readStart -3: r = -3, -2, -1 are clipped (S, c 3), r = 0.. are '=' -> "3S5=".  At readStart 96, reflen 100: r 96..99 '=',
      r 100.. clipped -> "4=4S".
  "mDDmmmmm" at readStart -4: m clipped (c 1, r -3); D clipped: r -2, sfdflag takes the count back (c 1); D: r -1 (c 1); m at r -1
      clipped (c 2, r 0); m at r 0 is '=' -> "2S", then "4=".
  "mmmDD" at readStart 97, reflen 100: r 97..99 '=' (c 3); D at r 100 is clipped: mode S, "3=" appended, c = 0, and sfdflag keeps it 0;
      the same for the second D; the unconditional final append prints "0S" -> "3=0S".
  "mmXX" at readStart 98, reflen 100: two '=' (r 100), X clipped (a clipped column moves refloc unless it is I) -> "2=2S"; in bounds
      (readStart 10) X is mode I -> "2=2I".  "XXmm" at readStart -1: X clipped (S, r 0); X at r 0 is I and does not move r: "1S"; m: "1I";
      -> "1S1I2=".
  "mmNmm": N is mode M in 1.4 -> "2=1M2="; in 1.3 everything is M -> "5M".
  the first symbol's mode differs from the initial lastMode '=' with c 0: nothing is appended for the empty run ("Smm" -> "1X2=").
makeMdTag (:1361-1445)
  "mmmSmmDDmmImm": r 4..6 c 3; S at r 7 (T): "3" "T"; r 8, 9 c 2; D D (r 10, 11, dels 2); m: flush "2" "^" ref[10..12) = "GT"; m m (c 2);
      I; m m (c 4); final "4" -> "3T2^GT4".
  "CCmSmmCC": clipped columns only move r: m at r 6 (c 1); S at r 7: "1T"; c 2; -> "1T2".
  "mSSm": "1" "C" (r 5); second S: c 0 and prevSub -> no count, "G"; final "1" -> "1CG1".  "SSm": c 0 and !prevSub -> "0A", then "C" -> "0AC1".
  "mmDSm": c 2; D at r 6; S: flush "2^G", then c 0 and !prevSub -> "0T"; final "1" -> "2^G0T1".  "SmDSm": "0A"; c 1; flush "1^G"; S with
      prevSub set and c 0 -> "T" alone -> "0A1^GT1".
  "mmNmm" with call "ACGTA": N at r 6 (G) and call[2] = G: a match, "5"; with call "ACNTA": a substitution, "2G2".
NM (:1514-1535): "mmmSmmDDmmImm", no clips: S + I + two D = 4.  "CCmSmmCC" with "2S1=1X2=2S": from 2, to 6: the S at cpos 3 -> 1.
toMapq (:1709-1721): length 100, score 9970: score2 = 5970 * 1.6f = 9552, max = 1.5f * 6.643856 + 36 = 45.96578, 9552 * 45.96578 / 10000
  = 43.9 -> 44.  score 4400: 640 * 45.96578 / 10000 = 2.94 -> 3 -> max(4, .) = 4.  Ambiguous: 9970 * 3 / 10000 = 2.99 -> 3; score 5000:
  1.5 -> Math.round gives 2; score 1000: 0.3 -> 0 -> max(1, .) = 1.  Unmapped: 0.
The constructor (:115-354) on two scaffolds sA at [20, 220) and sB at [250, 450) of chromosome 1, reads of 50 'm':
  mates at 30..79 (plus) and 120..169 (minus), paired: a1 10, b1 59 -> pos 11, end 60; a2 100 -> 101, 150; sameScaf; tlen = 1 + 150 - 11
      = 140, minus sign for the second line (its start is the larger); flags 0x1 + 0x2 + 0x40 + 0x20 = 99 and 0x1 + 0x2 + 0x80 + 0x10 =
      147; RNEXT '='.  Both at 30..79: tlen 1 + 60 - 11 = 50, the tie goes to pairnum 0: +50 / -50.
  mates on sA and sB: tlen 0, RNEXT = the mate's scaffold, no 0x2.  Only the first mapped: POS = PNEXT = 11 on both lines, RNAME sA on
      both, RNEXT '='; flags 0x1 + 0x40 + 0x8 = 73 and 0x1 + 0x80 + 0x4 = 133.  Neither: 0, 0, `*`, `*`, 77 and 141."""
import numpy as np

from bbmap_amd import reference as R
from bbmap_amd import sam as SAM
from tests import sam_check as SK
from tests import scaffold_check as SC

CHROM = np.frombuffer(b"ACGT" * 10, np.uint8)
FIN = np.dtype([("mapped", "<i4"), ("chrom", "<i4"), ("strand", "<i4"), ("start", "<i4"), ("stop", "<i4"), ("mapScore", "<i4"),
                ("paired", "<i4"), ("ambiguous", "<i4"), ("perfect", "<i4")])


def test_cigar_known_answers_derived_by_hand():
    m = b"mmmSmmDDmmImm"
    assert SK.to_cigar14(m, 10, 21, 1000) == "3=1X2=2D2=1I2="
    assert SK.to_cigar13(m, 10, 21, 1000) == "6M2D2M1I2M"
    assert SK.to_cigar14(b"CCmmmmCC", 5, 12, 1000) == "2S4=2S"
    assert SK.to_cigar14(b"m" * 8, -3, 4, 100) == "3S5="
    assert SK.to_cigar14(b"m" * 8, 96, 103, 100) == "4=4S"
    assert SK.to_cigar14(b"mDDmmmmm", -4, 3, 100) == "2S4="
    assert SK.to_cigar14(b"mmmDD", 97, 101, 100) == "3=0S"             # the unconditional final append
    assert SK.to_cigar13(b"mmmDD", 97, 101, 100) == "3M0S"
    assert SK.to_cigar14(b"mmXX", 98, 99, 100) == "2=2S"
    assert SK.to_cigar14(b"mmXX", 10, 11, 100) == "2=2I"
    assert SK.to_cigar14(b"XXmm", -1, 0, 100) == "1S1I2="
    assert SK.to_cigar14(b"mmNmm", 10, 14, 100) == "2=1M2="
    assert SK.to_cigar13(b"mmNmm", 10, 14, 100) == "5M"
    assert SK.to_cigar14(b"Smm", 10, 12, 100) == "1X2="                 # initial lastMode '=' with count 0: no empty run
    assert SK.to_cigar14(b"mmm", 7, 7, 100) is None and SK.to_cigar14(None, 1, 2, 100) is None


def test_md_and_nm_known_answers_derived_by_hand():
    md = lambda m, call=b"A" * 16: SK.make_md_tag(CHROM, 4, m, np.frombuffer(call, np.uint8), 0, 40)
    assert md(b"mmmSmmDDmmImm") == "3T2^GT4"
    assert md(b"CCmSmmCC") == "1T2"
    assert md(b"mSSm") == "1CG1"
    assert md(b"SSm") == "0AC1"
    assert md(b"mmDSm") == "2^G0T1"
    assert md(b"SmDSm") == "0A1^GT1"
    assert md(b"mmNmm", b"ACGTA") == "5"
    assert md(b"mmNmm", b"ACNTA") == "2G2"
    assert SK.calc_nm(b"mmmSmmDDmmImm", "3=1X2=2D2=1I2=", 11) == 4
    assert SK.calc_nm(b"CCmSmmCC", "2S1=1X2=2S", 8) == 1
    assert SK.calc_left_clip("2S4=") == 2 and SK.calc_left_clip("4=2S") == 0 and SK.calc_right_clip("4=2S") == 2
    assert SK.calc_right_clip("3=0S") == 0 and SK.calc_right_clip("2S4=") == 0


def test_mapq_known_answers_derived_by_hand():
    assert SK.to_mapq(9970, 100, True, False) == 44
    assert SK.to_mapq(4400, 100, True, False) == 4
    assert SK.to_mapq(3000, 100, True, False) == 4
    assert SK.to_mapq(9970, 100, True, True) == 3
    assert SK.to_mapq(5000, 100, True, True) == 2
    assert SK.to_mapq(1000, 100, True, True) == 1
    assert SK.to_mapq(9970, 100, False, False) == 0 and SK.to_mapq(9970, 0, True, False) == 0


def _packed():
    rng = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    p = R.pack([("sA", acgt[rng.integers(0, 4, 200)]), ("sB", acgt[rng.integers(0, 4, 200)])], start_pad=20, mid_pad=30, end_pad=20)
    assert [list(a) for a in p.locs] == [[20, 250]] and [list(a) for a in p.lengths] == [[200, 200]]
    return p


def _line(p, rows, paired, flags=0, matches=None, calls=None, length=50):
    fin = np.zeros(len(rows), FIN)
    for i, row in enumerate(rows):
        for k, v in row.items():
            fin[i][k] = v
    matches = matches or [b"m" * length if int(f["mapped"]) else None for f in fin]
    calls = calls or [np.frombuffer(b"A" * length, np.uint8)] * len(rows)
    return SK.sam_records(SC.table_of(p), fin, matches, [len(c) for c in calls], calls, p.chroms, paired, flags)


def _hit(start, strand=0, paired=1, **kw):
    return dict(mapped=1, chrom=1, strand=strand, start=start, stop=start + 49, mapScore=4920, paired=paired, perfect=1, **kw)


MISS = dict(mapped=0, chrom=-1, strand=0, start=-1, stop=-1)


def test_pos_pnext_tlen_table_flags_and_names_derived_by_hand():
    p = _packed()
    recs, text, strings = _line(p, [_hit(30), _hit(120, strand=1)], True)
    assert [tuple(int(r[k]) for k in ("flag", "rname", "pos", "rnext", "pnext", "tlen")) for r in recs] == \
        [(99, 0, 11, -2, 101, 140), (147, 0, 101, -2, 11, -140)]
    assert strings == [("50=", None), ("50=", None)] and text == b"50=50="
    assert [int(r["nm"]) for r in recs] == [0, 0]
    recs, _, _ = _line(p, [_hit(30), _hit(30, strand=1)], True)
    assert [int(r["tlen"]) for r in recs] == [50, -50]                  # start1 == start2: pairnum 0 keeps the plus sign
    recs, _, _ = _line(p, [_hit(30, paired=0), _hit(260, strand=1, paired=0)], True)
    assert [tuple(int(r[k]) for k in ("flag", "rname", "pos", "rnext", "pnext", "tlen")) for r in recs] == \
        [(0x1 | 0x40 | 0x20, 0, 11, 1, 11, 0), (0x1 | 0x80 | 0x10, 1, 11, 0, 11, 0)]
    recs, _, strings = _line(p, [_hit(30, paired=0), MISS], True)
    assert [tuple(int(r[k]) for k in ("flag", "rname", "pos", "rnext", "pnext", "tlen")) for r in recs] == \
        [(73, 0, 11, -2, 11, 0), (133, 0, 11, -2, 11, 0)]
    assert strings[1] == (None, None) and int(recs[1]["nm"]) == -1 and int(recs[1]["am"]) == -1 and int(recs[1]["mapq"]) == 0
    assert int(recs[0]["am"]) == 0                                      # min(mapq, 0): the mate is not mapped
    recs, _, _ = _line(p, [MISS, _hit(30, paired=0)], True)
    assert [tuple(int(r[k]) for k in ("flag", "rname", "pos", "rnext", "pnext")) for r in recs] == [(69, 0, 11, -2, 11), (137, 0, 11, -2, 11)]
    recs, _, _ = _line(p, [MISS, MISS], True)
    assert [tuple(int(r[k]) for k in ("flag", "rname", "pos", "rnext", "pnext", "tlen")) for r in recs] == [(77, -1, 0, -1, 0, 0), (141, -1, 0, -1, 0, 0)]
    recs, _, _ = _line(p, [_hit(30, strand=1, paired=0)], False)
    assert tuple(int(recs[0][k]) for k in ("flag", "rname", "pos", "rnext", "pnext", "tlen")) == (16, 0, 11, -1, 0, 0)
    assert int(recs[0]["am"]) == int(recs[0]["mapq"])                   # single-ended: AM = MAPQ


def test_md_reads_the_read_as_it_came_in_on_the_minus_strand():
    """scaffold sA = chromosome [20, 220).  A 5-base minus-strand read "mNmmm" at start s: makeMdTag gets r.bases, which the mapping
    threads never reverse (see sam_records.hip), so the N column compares ref[s + 1] with call[1] of the read AS IT CAME IN.  s is chosen
    so that this base equals the reference base while the aligned strand holds an N there: the reference's tag is "5", not "1x3"."""
    p = _packed()
    comp = {65: 84, 67: 71, 71: 67, 84: 65}
    ref = p.chroms[0]
    s = next(i for i in range(40, 200) if comp[int(ref[i + 3])] == int(ref[i + 1]))
    aligned = ref[s: s + 5].copy()
    aligned[1] = ord("N")
    came_in = np.array([78 if b == 78 else comp[int(b)] for b in aligned[::-1]], np.uint8)
    assert came_in[1] == ref[s + 1] and came_in[3] == ord("N")
    row = dict(mapped=1, chrom=1, strand=1, start=s, stop=s + 4, mapScore=300, paired=0, perfect=0)
    _, _, strings = _line(p, [row], False, SK.MD, matches=[b"mNmmm"], calls=[came_in])
    assert strings[0] == ("1=1M3=", "5")


def test_sam_text_formatting_on_hand_made_records():
    p = _packed()
    assert SAM.header(p) == ["@HD\tVN:1.4\tSO:unsorted", "@SQ\tSN:sA\tLN:200", "@SQ\tSN:sB\tLN:200"]
    assert SAM.header(p, cigar13=True)[0] == "@HD\tVN:1.3\tSO:unsorted"
    assert SAM.qname("r1/1", True) == "r1" and SAM.qname("r1 2", True) == "r1" and SAM.qname("r1/1", False) == "r1/1"
    assert SAM.qname("a\tb/3", True) == "a_b/3" and SAM.qname("/1", True) == "/1"
    recs = np.zeros(3, SK.SAMREC_DTYPE)
    text = np.frombuffer(b"2=1X1=3T03S1=", np.uint8)
    recs[0] = (99, 44, 0, -2, 11, 101, 140, 1, 40, 1, 0, 6, 3, 6)
    recs[1] = (147, 30, 0, -2, 101, 11, -140, -1, 30, 0, 9, 4, 0, 13)
    recs[2] = (77, 0, -1, -1, 0, 0, 0, -1, -1, 0, 13, 0, 0, 13)
    reads = [b"ACGT", b"AACG", b"TTTT"]
    quals = [[0, 1, 2, 3], [10, 11, 12, 13], None]
    out = SAM.lines(recs, text, ["x/1", "x/2", "y"], reads, quals, ["sA", "sB"], True)
    assert out[0] == "x\t99\tsA\t11\t44\t2=1X1=\t=\t101\t140\tACGT\t!\"#$\tXT:A:R\tNM:i:1\tAM:i:40\tMD:Z:3T0"
    assert out[1] == "x\t147\tsA\t101\t30\t3S1=\t=\t11\t-140\tCGTT\t.-,+\tAM:i:30"       # minus strand: SEQ reverse-complemented, QUAL reversed
    assert out[2] == "y\t77\t*\t0\t0\t*\t*\t0\t0\tTTTT\t*"


def test_the_binding_declares_the_header_s_record():
    from bbmap_amd import mapper
    assert mapper.SAMREC_DTYPE == SK.SAMREC_DTYPE and mapper.SAMREC_DTYPE.itemsize == 64
