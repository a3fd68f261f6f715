"""CPU tests of the FASTA reader and packer (bbmap_amd/reference.py, FastaToChromArrays2.makeNextChrom) and of the test-local
restatement of Data.isSingleScaffold / scaffoldIndex / SamLine's coordinate block (tests/scaffold_check.py) on hand-derived cases."""
import gzip
import os

import numpy as np

from bbmap_amd import reference as R
from tests import golden_phix
from tests import scaffold_check as SC

N = ord("N")


def _write(tmp_path, text, name="ref.fa", gz=False):
    p = os.path.join(str(tmp_path), name)
    data = text.encode()
    if gz:
        with gzip.open(p, "wb") as f:
            f.write(data)
    else:
        with open(p, "wb") as f:
            f.write(data)
    return p


def _s(a):
    return bytes(np.asarray(a, np.uint8))


def test_one_scaffold(tmp_path):
    recs = R.read_fasta(_write(tmp_path, ">chr1 some description\nACGT\nAC\n"))
    assert [(n, _s(b)) for n, b in recs] == [("chr1 some description", b"ACGTAC")]
    p = R.pack(recs)
    assert p.nchroms == 1 and p.inter_scaffold_padding == 300
    c = p.chroms[0]
    assert len(c) == 8000 + 6 + 8001                          # terminalN <= END_PADDING: 8001 trailing N, not 8000
    assert _s(c[:8000]) == b"N" * 8000 and _s(c[8000:8006]) == b"ACGTAC" and _s(c[8006:]) == b"N" * 8001
    assert p.locs[0].tolist() == [8000] and p.lengths[0].tolist() == [6] and p.names[0] == ["chr1 some description"]


def test_trimmed_names(tmp_path):
    recs = R.read_fasta(_write(tmp_path, ">chr1 some description\nACGT\n>chr2\tx\nGG\n"), trim_names=True)
    assert [n for n, _ in recs] == ["chr1", "chr2"]


def test_three_merged_scaffolds(tmp_path):
    text = ">a\n" + "A" * 10 + "\n>b\n" + "C" * 7 + "\n" + "G" * 5 + "\n>c\n" + "T" * 3 + "\n"
    p = R.pack(R.read_fasta(_write(tmp_path, text)))
    assert p.nchroms == 1
    L1, L2, L3 = 10, 12, 3
    assert p.locs[0].tolist() == [8000, 8000 + L1 + 300, 8000 + L1 + 300 + L2 + 300]
    assert p.lengths[0].tolist() == [L1, L2, L3] and p.names[0] == ["a", "b", "c"]
    c = _s(p.chroms[0])
    assert c == b"N" * 8000 + b"A" * 10 + b"N" * 300 + b"C" * 7 + b"G" * 5 + b"N" * 300 + b"T" * 3 + b"N" * 8001


def test_short_scaffold_skipped_but_mid_pad_added(tmp_path):
    text = ">a\nAAAA\n>short\nCC\n>c\nGGGG\n"
    p = R.pack(R.read_fasta(_write(tmp_path, text)), min_scaffold=3)
    # the skipped record still gets its MID_PADDING (`if(scaffolds>0)` comes before the MIN_SCAFFOLD test): two pads in a row
    assert _s(p.chroms[0]) == b"N" * 8000 + b"AAAA" + b"N" * 600 + b"GGGG" + b"N" * 8001
    assert p.locs[0].tolist() == [8000, 8000 + 4 + 600] and p.names[0] == ["a", "c"]
    # skipped as the first record of a chromosome: no pad at all
    p = R.pack(R.read_fasta(_write(tmp_path, ">short\nCC\n>c\nGGGG\n", "b.fa")), min_scaffold=3)
    assert _s(p.chroms[0]) == b"N" * 8000 + b"GGGG" + b"N" * 8001 and p.locs[0].tolist() == [8000]


def test_split_into_several_chromosomes(tmp_path):
    recs = [("s%d" % i, b"ACGT" * 25) for i in range(5)]      # five 100-base records
    # a record fits while len + MID_PADDING + END_PADDING + maxIndex <= max_length; maxIndex = 7999 on an empty chromosome
    # first fit: 100 + 300 + 8000 + 7999 = 16399; second: 100 + 300 + 8000 + 8099 = 16499; third: 16899
    p = R.pack(recs, max_length=16500)
    assert [len(l) for l in p.locs] == [2, 2, 1]
    assert [l.tolist() for l in p.locs] == [[8000, 8400], [8000, 8400], [8000]]
    assert [n for ns in p.names for n in ns] == ["s0", "s1", "s2", "s3", "s4"]
    # END_PADDING is added only while maxIndex < MAX_LENGTH - 1: 8500 + 8001 > 16500, so chromosome 1 stops at 16500 bases
    assert len(p.chroms[0]) == 16500 and len(p.chroms[1]) == 16500 and len(p.chroms[2]) == 8100 + 8001
    p = R.pack(recs, max_length=16450)                        # the second record no longer fits: 16499 > 16450
    assert [len(l) for l in p.locs] == [1, 1, 1, 1, 1]
    assert all(len(c) == 8100 + 8001 for c in p.chroms)
    # merge=False: one scaffold per chromosome
    p = R.pack(recs, merge=False)
    assert [len(l) for l in p.locs] == [1] * 5
    assert p.scaffold_bases() == [(c, 8000, 100) for c in range(1, 6)]


def test_input_ending_in_n(tmp_path):
    p = R.pack([("a", b"ACGT" + b"N" * 5)])
    # five terminal N count towards END_PADDING: 8001 - 5 are added
    assert len(p.chroms[0]) == 8000 + 9 + 7996 and p.lengths[0].tolist() == [9]
    p = R.pack([("a", b"ACGT" + b"N" * 9000)])
    assert len(p.chroms[0]) == 8000 + 9004 + 1                # terminalN stops counting at END_PADDING: one more N
    p = R.pack([("a", b"ACGT")], end_pad=0)
    assert len(p.chroms[0]) == 8004


def test_lower_case_and_iupac(tmp_path):
    recs = R.read_fasta(_write(tmp_path, ">x\nacgtnACGTN\nRYKMSWBDHVuU-.*X\n"))
    assert _s(recs[0][1]) == b"ACGTNACGTN" + b"NNNNNNNNNN" + b"TT" + b"NNNN"


def test_gzip_input_and_lines_before_a_header(tmp_path):
    recs = R.read_fasta(_write(tmp_path, ">a\r\nAC\r\nGT\r\n>b\n\nTT\n", "r.fa.gz", gz=True))
    assert [(n, _s(b)) for n, b in recs] == [("a", b"ACGT"), ("b", b"TT")]
    recs = R.read_fasta(_write(tmp_path, "AC\n>b\nTT\n", "s.fa"))
    assert [(n, _s(b)) for n, b in recs] == [(None, b"AC"), ("b", b"TT")]


def test_phix_packs_like_the_golden_reference():
    recs = R.read_fasta(os.path.join(golden_phix.HERE, "phix174_ill.ref.fa.gz"))
    assert len(recs) == 1
    p = R.pack(recs)
    ref = golden_phix.phix_reference()                       # 8000 N + body + 8000 N
    body = len(ref) - 16000
    c = p.chroms[0]
    assert _s(c[:8000 + body]) == _s(ref[:8000 + body])
    assert len(c) == 8000 + body + 8001 and _s(c[8000 + body:]) == b"N" * 8001
    assert p.locs[0].tolist() == [8000] and p.lengths[0].tolist() == [body]


def test_single_scaffold_boundaries():
    pad = 300
    locs = [None, [8000, 8400, 9000], [8000]]
    # loc1 + pad exactly on a start: binarySearch hits it
    assert SC.scaffold_index(locs, pad, 1, 8400 - pad // 2) == 1
    assert SC.is_single_scaffold(locs, pad, 1, 8400 - pad, 8450)          # loc1 + pad == 8400: scaffold 1, bounds [8100, 9000)
    assert not SC.is_single_scaffold(locs, pad, 1, 8400 - pad - 1, 8450)  # scaffold 0 then: loc2 >= its upper bound 8400
    # inside scaffold 0, up to the next start
    assert SC.is_single_scaffold(locs, pad, 1, 8000, 8399)
    assert not SC.is_single_scaffold(locs, pad, 1, 8000, 8400)
    # a site inside the pad before scaffold 1 belongs to scaffold 1 once loc1 + pad reaches its start
    assert SC.is_single_scaffold(locs, pad, 1, 8150, 8300)
    # the last scaffold: always single
    assert SC.is_single_scaffold(locs, pad, 1, 8800, 20000)
    # before the first scaffold (start padding): scaffold 0, single while loc2 < the next start
    assert SC.is_single_scaffold(locs, pad, 1, 10, 8399)
    assert not SC.is_single_scaffold(locs, pad, 1, 10, 8400)
    # one-scaffold chromosomes and no table
    assert SC.is_single_scaffold(locs, pad, 2, 0, 10 ** 6)
    assert SC.is_single_scaffold(None, pad, 1, 8000, 9500)
    assert SC.scaffold_index(locs, pad, 2, 123456) == 0
    # scaffoldIndex puts a point in the pad on the closer scaffold
    assert SC.scaffold_index(locs, pad, 1, 8400 - 151) == 0 and SC.scaffold_index(locs, pad, 1, 8400 - 150) == 1
    assert SC.scaffold_index(locs, pad, 1, 5) == 0 and SC.scaffold_index(locs, pad, 1, 10 ** 6) == 2


def test_samline_block_on_hand_built_records():
    from bbmap_amd.mapper import FINAL_DTYPE
    table = ([None, [8000, 8400]], [None, [100, 500]], 300, [0, 0])
    f = np.zeros(6, FINAL_DTYPE)
    f["mapped"] = 1
    f["chrom"] = 1
    f["paired"] = 1
    f["start"][:] = [8010, 8405, 7995, 8090, 8500, 8420]
    f["stop"][:] = [8019, 8414, 8004, 8410, 8509, 8429]
    m = [b"m" * 10, b"CCm" + b"m" * 5 + b"CC", b"CmDmImmmmmm", b"m" * 21, b"m" * 10, None]
    out = SC.scaffold_records(table, f, m, paired=True)
    # pair 0: both on their own scaffolds (0 and 1): paired, not sameScaf
    assert out["scaffold"][:2].tolist() == [0, 1] and out["pos"][:2].tolist() == [11, 6 + 2] and out["end"][:2].tolist() == [20, 15 - 2]
    assert out["flags"][:2].tolist() == [SC.MAPPED | SC.PAIRED | SC.INBOUNDS] * 2
    # pair 1: mate 1 starts 5 bases before its scaffold (a1 = -5): leading clip 1, then C m D m I m: rloc reaches 0 after
    # C m D m m (the I does not move it) -> dels 1, ins 1 -> pos = -5 + 1 + 1 + 0 = -3 -> clamped to 1; not inbounds.
    # Mate 2 spans the boundary at 8400: unmapped, and mate 1 unpaired.
    assert out["scaffold"][2] == 0 and out["start"][2] == -5 and out["pos"][2] == 1 and out["end"][2] == 5
    assert out["flags"][2] == SC.MAPPED and out["flags"][3] == 0 and out["scaffold"][3] == -1
    # pair 2: both on scaffold 1: sameScaf; end clamped to scaflen never needed here
    assert out["flags"][4] == out["flags"][5] == SC.MAPPED | SC.PAIRED | SC.INBOUNDS | SC.SAME_SCAFFOLD
    assert SC.count_leading_indels(-3, b"mIIDm") == 1 - 2
    assert SC.count_leading_clip(b"C3m") == 3 and SC.count_trailing_clip(b"mmCC") == 2
