"""SAM for spliced reads on the device: the intron limit (the `N` operator, the runs NM and MD leave out, XS) and the optional tags of
bbmap_get_sam_records_cfg / bbpipe_sam_records_device.

Device output must equal tests/sam_splice_check.py (a sequential restatement, pinned by hand in tests/test_sam_splice_cpu.py and tied
there to tests/sam_check.py) field for field and byte for byte.  The raw form is driven with hand-made records whose shapes are chosen
for the kernels' 64-symbol step -- among them the strings the mapper never produces (one that ends in a deletion run, `0S`); the mapper
tests plant reads with a deletion of known length and add checks that do not go through the restatement."""
import ctypes as C
import re

import numpy as np
import pytest

from bbmap_amd import keys as K
from bbmap_amd import reference as R
from bbmap_amd import sam as SAM
from bbmap_amd.index import READ_DTYPE, DeviceIndex
from bbmap_amd.mapper import (FINAL_DTYPE, MSITE_DTYPE, SAM_ALL_TAGS, SAM_CIGAR13, SAM_MAKE_XS, SAM_MD, SAM_NO_INTRON_LIMIT, SAM_NO_TAGS,
                              SAM_XS_SECONDSTRAND, SAMREC_DTYPE, SAMTAGS_DTYPE, SCAFREC_DTYPE, Mapper, sam_config, sam_records_device,
                              sam_workspace_bytes)
from tests import sam_splice_check as SP
from tests import scaffold_check as SC

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    COMP[_a] = _b
OPS = re.compile(r"(\d+)([=XIDSMN])")
LIMITS = (1, 10, SAM_NO_INTRON_LIMIT)
FLAGS = (0, SAM_CIGAR13, SAM_MD, SAM_CIGAR13 | SAM_MD)
assert (SP.ALL_TAGS, SP.NO_TAGS, SP.XS_SECONDSTRAND, SP.CIGAR13, SP.MD) == (SAM_ALL_TAGS, SAM_NO_TAGS, SAM_XS_SECONDSTRAND, SAM_CIGAR13, SAM_MD)
assert SP.SAMTAGS_DTYPE == SAMTAGS_DTYPE
assert (SP.NM, SP.AM, SP.SM, SP.XM, SP.XS, SP.XS_SECONDSTRAND, SP.NH, SP.STOP, SP.LENGTH, SP.IDENTITY, SP.SCORE, SP.INSERT, SP.BOUNDS,
        SP.NO_TAGS) == (SAM.MAKE_NM, SAM.MAKE_AM, SAM.MAKE_SM, SAM.MAKE_XM, SAM.MAKE_XS, SAM.XS_SECONDSTRAND, SAM.MAKE_NH, SAM.MAKE_STOP,
                        SAM.MAKE_LENGTH, SAM.MAKE_IDENTITY, SAM.MAKE_SCORE, SAM.MAKE_INSERT, SAM.MAKE_BOUNDS, SAM.NO_TAGS)


def _rc(a):
    return COMP[np.asarray(a, np.uint8)[::-1]]


def _equal(got, want, what):
    recs, tg, text, need = got
    wrecs, wtg, wtext, strings = want
    assert need == len(wtext), (what, need, len(wtext))
    for f in SAMREC_DTYPE.names:
        bad = [r for r in range(len(wrecs)) if recs[r][f] != wrecs[r][f]]
        assert not bad, (what, f, [(r, recs[r], wrecs[r], strings[r]) for r in bad[:3]])
    for f in SAMTAGS_DTYPE.names if tg is not None else ():
        bad = [r for r in range(len(wtg)) if tg[r][f] != wtg[r][f]]
        assert not bad, (what, f, [(r, tg[r], wtg[r], strings[r]) for r in bad[:3]])
    assert text[:need].tobytes() == wtext, what


# ------------------------------------------------------------------------------------------------ the raw form, hand-made records
SCAFLOC, CAP = 300, 4
CHROM = ACGT[np.random.default_rng(5).integers(0, 4, 1400)]


def _case(match, a1=20, scaflen=700, scaffold=0, **fin):
    return dict(match=match, a1=a1, scaflen=scaflen, scaffold=scaffold, fin=fin)


def _batch(cases, paired, seed):
    """the arrays of bbpipe_sam_records_device for hand-made cases (None = an unmapped read of 30 bases); the scaffold records are
    written as SamLine's coordinate block would (tests/scaffold_check.py's formulas), with every case's own scaflen"""
    rng = np.random.default_rng(seed)
    n = len(cases)
    reads, fin, scaf = np.zeros(n, READ_DTYPE), np.zeros(n, FINAL_DTYPE), np.zeros(n, SCAFREC_DTYPE)
    sites, nsites = np.zeros((n, CAP), MSITE_DTYPE), np.zeros(n, np.int32)
    pool, bases, matches, calls = bytearray(), [], [], []
    for r, c in enumerate(cases):
        m = c["match"] if c else None
        ln = sum(1 for b in m if b != ord("D")) if c else 30
        call = ACGT[rng.integers(0, 4, ln)].copy()
        if ln > 4 and r % 3 == 0:
            call[rng.integers(0, ln, 2)] = ord("N")
        reads[r]["bases_off"], reads[r]["len"] = sum(len(b) for b in bases), ln
        bases.append(call); calls.append(call); matches.append(m)
        f = fin[r]
        if not c:
            f["chrom"], f["start"], f["stop"], scaf[r]["scaffold"] = -1, -1, -1, -1
            continue
        span = sum(1 for b in m if chr(b) not in "IXY")
        a1, b1 = c["a1"], c["a1"] + span - 1
        f["mapped"], f["chrom"], f["start"], f["stop"], f["mapScore"] = 1, 1, SCAFLOC + a1, SCAFLOC + b1, int(rng.integers(40, 95)) * ln
        f["match_len"], f["match_off"] = len(m), len(pool)
        for k, v in c["fin"].items():
            f[k] = v
        pool += m + b"\0" * (-len(m) % 4)
        s = scaf[r]
        s["scaffold"], s["start"], s["stop"], s["scaflen"] = c["scaffold"], a1, b1, c["scaflen"]
        s["pos"] = max(1, a1 + 1 + SC.count_leading_clip(m) + SC.count_leading_indels(a1, m))
        s["end"] = min(c["scaflen"], b1 + 1 - SC.count_trailing_clip(m))
        s["flags"] = SC.MAPPED | (SC.INBOUNDS if a1 >= 0 and b1 < c["scaflen"] else 0) | (SC.PAIRED if int(f["paired"]) else 0)
        nsites[r] = int(rng.integers(0, CAP + 1))
        sites[r]["score"] = rng.choice([500, 600], CAP)
    if paired:
        for r in range(0, n, 2):
            if cases[r] and cases[r + 1] and cases[r]["scaffold"] == cases[r + 1]["scaffold"]:
                scaf[r]["flags"] |= SC.SAME_SCAFFOLD; scaf[r + 1]["flags"] |= SC.SAME_SCAFFOLD
    scores = [[int(x) for x in sites[r]["score"][:nsites[r]]] for r in range(n)]
    return dict(reads=reads, bases=np.concatenate(bases), fin=fin, pool=np.frombuffer(bytes(pool), np.uint8), scaf=scaf, sites=sites,
                nsites=nsites, matches=matches, calls=calls, lens=[int(x) for x in reads["len"]], scores=scores, paired=paired)


GUARD = 64


def _device(b, flags, limit, tags, text_cap=None, want_tags=True, **over):
    """one bbpipe_sam_records_device call over uploaded copies of the batch.  text_cap: None = a buffer that surely fits; else the
    blob's capacity in bytes, and GUARD bytes of 0xEE lie behind it, so that a write behind the capacity shows.  Returns
    (SAMREC_DTYPE[n], SAMTAGS_DTYPE[n] or None, the text buffer with its guard, the bytes the blob needs)."""
    import torch
    dev = torch.device("cuda")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).view(np.uint8).reshape(-1).copy()).to(dev)
    pad = lambda a: np.concatenate([np.asarray(a, np.uint8).reshape(-1), np.zeros(64, np.uint8)])
    n = len(b["reads"])
    d_chrom = up(pad(CHROM), np.uint8)
    carr = torch.tensor([0, d_chrom.data_ptr()], dtype=torch.int64, device=dev)            # (chromosome numbers start at 1)
    clen = torch.tensor([0, len(CHROM)], dtype=torch.int32, device=dev)
    guard = 0 if text_cap is None else GUARD
    if text_cap is None:
        text_cap = 24 * sum(len(m) for m in b["matches"] if m) + 32 * n + 64
    buf = torch.full((text_cap + guard + 1,), 0xEE, dtype=torch.uint8, device=dev)
    recs = torch.zeros(n * SAMREC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    tagrecs = torch.zeros(n * SAMTAGS_DTYPE.itemsize, dtype=torch.uint8, device=dev) if want_tags else None
    need = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.zeros(sam_workspace_bytes(n, 600), dtype=torch.uint8, device=dev)
    kw = dict(paired=b["paired"], flags=flags, intron_limit=limit, tags=tags, tagrecs=tagrecs, sites=up(b["sites"], MSITE_DTYPE),
              nsites=up(b["nsites"], np.int32), cap=CAP, chrom_arr=carr, chrom_arr_len=clen, max_read_len=600)
    kw.update(over)
    sam_records_device(up(b["reads"], READ_DTYPE), up(pad(b["bases"]), np.uint8), up(b["fin"], FINAL_DTYPE), up(pad(b["pool"]), np.uint8),
                       up(b["scaf"], SCAFREC_DTYPE), recs, buf[:text_cap], need, ws, **kw)
    torch.cuda.current_stream().synchronize()
    return (recs.cpu().numpy().view(SAMREC_DTYPE), tagrecs.cpu().numpy().view(SAMTAGS_DTYPE) if want_tags else None,
            buf.cpu().numpy()[:text_cap + guard], int(need.item()))


def _restated(b, flags, limit, tags):
    return SP.sam_records(None, b["fin"], b["matches"], b["lens"], b["calls"], [CHROM], b["paired"], flags, limit, tags, b["scores"], b["scaf"])


def _every_setting(b):
    seen = set()
    for limit in LIMITS:
        for flags in FLAGS:
            want = _restated(b, flags, limit, SAM_ALL_TAGS)
            _equal(_device(b, flags, limit, SAM_ALL_TAGS), want, (limit, flags))
            seen.update(c for c, _ in want[3] if c)
    return seen


m, D = b"m", b"D"
SINGLE = [
    _case(m * 60 + D * 11 + m * 30),                        # a run over the step border (columns 60-70)
    _case(m * 10 + D * 200 + m * 20),                       # head in step 0, tail in step 3
    _case(m * 5 + D * 1 + m * 5), _case(m * 5 + D * 2 + m * 5),                       # limit 1: exactly limit, limit + 1
    _case(m * 5 + D * 9 + m * 5), _case(m * 5 + D * 10 + m * 5), _case(m * 5 + D * 11 + m * 5),       # limit 10: - 1, exactly, + 1
    _case(m * 50 + D * 14 + m * 10),                        # ends exactly at column 63
    _case(m * 64 + D * 12 + m * 8),                         # starts at column 64
    _case(m * 20 + D * 15 + m * 19 + b"S" + m * 20 + D * 15 + m * 20),          # two long runs, in different steps
    _case(m * 20 + D * 15 + m * 19 + b"S" + m * 20 + D * 3 + b"S" + m * 20, strand=1),       # long, then short: the MD carry-over
    _case(m * 30 + D * 3 + m * 40 + D * 15 + m * 10 + D * 2 + m * 5),           # short, long, short
    _case(m * 30 + D * 15),                                 # ends in a long run: the final append
    _case(D * 40),                                          # one step, only D (a read without bases)
    _case(m * 10 + b"X" + m * 5 + D * 20 + m * 10, a1=675),                     # a long run over the scaffold's end, X in the step
    _case(m * 5 + b"Y" + m * 5 + D * 20 + m * 30, a1=-20),                      # over its start (negative refloc), Y in the step
    _case(m * 3 + D * 11, a1=687, scaflen=700),             # limit + 1 columns of which one is clipped: 10D0S
    _case(m * 3 + D * 2, a1=697, scaflen=700),              # 3=0S
    _case(b"S"), _case(m * 31 + b"S" + m * 31), _case(m * 32 + b"S" + m * 31), _case(m * 32 + b"S" + m * 32), _case(m * 64 + b"S" + m * 64),
    _case(m * 64, perfect=1), _case(m * 65, perfect=1, strand=1),               # the shortcut CIGAR
    _case(m * 10 + b"NNN" + m * 10 + b"IIII" + m * 10 + b"s" + m * 10, ambiguous=1),
    _case(b"CC" + m * 20 + D * 12 + m * 20 + b"CCC", strand=1),
    _case(m + b"S" * 31),                                   # the YI tie: 3.125
    None,                                                   # unmapped: no tags
    _case(m * 70 + D * 100 + b"S" + m * 21 + D * 64 + m * 2),                   # a run that is exactly one whole step (columns 192-255)
]


def test_raw_form_single_reads_every_limit_flag_and_tag():
    b = _batch(SINGLE, False, 1)
    seen = _every_setting(b)
    for cigar in ("60=11N30=", "10=200N20=", "5=1D5=", "5=2N5=", "5=10D5=", "5=11N5=", "30=15N", "40N", "40D", "3=10D0S", "3=0S", "64=", "65M",
                  "60M11N30M", "30M15N"):
        assert cigar in seen, (cigar, sorted(seen))
    assert "11S11N30=" in seen and "10=1I5=10D10S" in seen                       # the runs over the scaffold's start and end
    # SAM text with every tag, and the YI tie through the formatter
    recs, tg, text, need = _device(b, SAM_MD, 10, SAM_ALL_TAGS)
    lines = SAM.lines(recs, text[:need], ["r%d" % i for i in range(len(recs))], b["calls"], None, ["s0", "s1"], False, tags=tg)
    tie = lines[len(SINGLE) - 3].split("\t")
    assert "YI:f:3.13" in tie and "XB:Z:I" in tie and not any(x.startswith("XS") for x in tie)
    first = lines[0].split("\t")
    assert first[5] == "60=11N30=" and first[11] == "NM:i:0" and "XS:A:+" in first and "NH:i:1" in first and "YL:Z:90,101" in first
    assert len(lines[len(SINGLE) - 2].split("\t")) == 11                        # the unmapped line carries no tag
    assert SAM.splice_counts(tg, False)[0] == int((tg["splices"] > 0).sum()) > 5


def test_raw_form_second_strand_no_tags_and_default_tags():
    b = _batch(SINGLE, False, 2)
    for tags in (SAM_ALL_TAGS | SAM_XS_SECONDSTRAND, SAM_ALL_TAGS | SAM_NO_TAGS, None, SAM_MAKE_XS):
        want = _restated(b, SAM_MD, 10, SP.NM | SP.AM if tags is None else tags)
        got = _device(b, SAM_MD, 10, tags)
        _equal(got, want, tags)
    recs, tg, _, _ = got = _device(b, SAM_MD, 10, SAM_ALL_TAGS | SAM_NO_TAGS)
    assert not tg["present"].any() and (recs["nm"] == -1).all() and (recs["md_len"] == 0).all() and (recs["tags"] == 0).all()
    assert tg["introns"].sum() > 5                          # (the CIGAR keeps its N)
    _, tg2, _, _ = _device(b, 0, 10, SAM_ALL_TAGS | SAM_XS_SECONDSTRAND)
    _, tg1, _, _ = _device(b, 0, 10, SAM_ALL_TAGS)
    assert (tg1["xs"] == -tg2["xs"]).all() and (tg1["xs"] != 0).sum() > 5


def _pairs():
    long1, plain = m * 40 + D * 30 + m * 40, m * 39 + b"S" + m * 40
    return [
        _case(long1, a1=50, paired=1), _case(plain, a1=300, strand=1, paired=1),              # a proper pair
        _case(plain, a1=50, paired=1), _case(long1, a1=300, strand=1, paired=1),              # the minus-strand mate 2 carries the N
        _case(long1, a1=50, strand=1), None,                                                  # the mate unmapped
        None, _case(long1, a1=50),
        _case(long1, a1=50), _case(plain, a1=80, scaffold=1, strand=1),                       # on another scaffold
        _case(long1, a1=50), _case(plain, a1=660, strand=1),                                  # the mate out of bounds
        _case(plain, a1=-10), _case(long1, a1=200),                                           # this read out of bounds, same strands
        None, None,
        _case(long1, a1=400, paired=1), _case(plain, a1=100, strand=1, paired=1),             # plus read to the right of the minus read
        _case(long1, a1=100, paired=1, ambiguous=1), _case(long1, a1=100, strand=1, paired=1),
    ]


def test_raw_form_pairs_am_x8_xb():
    b = _batch(_pairs(), True, 3)
    _every_setting(b)
    recs, tg, text, need = _device(b, 0, 10, SAM_ALL_TAGS)
    letters = {(chr(int(x) & 0xff), chr(int(x) >> 8)) for x in tg["xb"] if x}
    assert letters >= {("I", "I"), ("I", "U"), ("I", "O"), ("O", "I")}, letters
    assert int(tg[3]["xs"]) == 1 and int(tg[0]["xs"]) == 1 and int(tg[4]["xs"]) == -1       # minus mate 2: +; plus mate 1: +; minus mate 1: -
    # mate 1 at [50, 159] plus, mate 2 from 300 minus, 80 bases each: PlusLeft, mid = 300 - 159 - 1 = 140 -> 140 + 80 + 80
    assert int(tg[0]["x8"]) == 300 and int(tg[1]["x8"]) == 300 and int(tg[4]["x8"]) == 0
    lines = SAM.lines(recs, text[:need], ["p%d/%d" % (i // 2, i % 2 + 1) for i in range(len(recs))], b["calls"], None, ["s0", "s1"], True, tags=tg)
    assert "XB:Z:IU" in lines[4].split("\t") and "X8:Z:300" in lines[0].split("\t") and len(lines[5].split("\t")) == 11


def test_raw_form_text_capacity_one_byte_short_and_rejections():
    b = _batch(SINGLE, False, 4)
    want = _restated(b, SAM_MD, 10, SAM_ALL_TAGS)
    full = _device(b, SAM_MD, 10, SAM_ALL_TAGS)
    _equal(full, want, "fits")
    need = full[3]
    recs, tg, text, need2 = _device(b, SAM_MD, 10, SAM_ALL_TAGS, text_cap=need - 1)
    assert need2 == need and len(text) == need - 1 + GUARD
    assert np.array_equal(recs, full[0]) and np.array_equal(tg, full[1])                    # the records keep the true lengths and offsets
    assert text[:need - 1].tobytes() == want[2][:need - 1] and (text[need - 1:] == 0xEE).all()
    recs, tg, text, need3 = _device(b, SAM_MD, 10, SAM_ALL_TAGS, text_cap=0)
    assert need3 == need and (text == 0xEE).all() and np.array_equal(recs, full[0])
    for flags, limit, tags, kw in ((0, -1, SAM_ALL_TAGS, {}), (0, 10, 1 << 20, {}), (4, 10, SAM_ALL_TAGS, {}), (0, 10, SAM_ALL_TAGS, dict(sites=None))):
        with pytest.raises(Exception, match="bbpipe_sam_records_device"):
            _device(b, flags, limit, tags, **kw)


def test_raw_form_without_tag_records_under_a_limit():
    """the plain instantiation of the sizing kernel (no tag records wanted) at finite limits: the N letter, NM without the long runs
    and MD's dropped runs equal the restatement's records and text; no site list is needed then"""
    for cases, paired, seed in ((SINGLE, False, 6), (_pairs(), True, 7)):
        b = _batch(cases, paired, seed)
        for limit in (1, 10):
            for flags in FLAGS:
                for tags in (SAM_ALL_TAGS, None):
                    want = _restated(b, flags, limit, SP.NM | SP.AM if tags is None else tags)
                    got = _device(b, flags, limit, tags, want_tags=False, sites=None, nsites=None, cap=0)
                    assert got[1] is None
                    _equal(got, want, (limit, flags, tags))
        want = _restated(b, SAM_MD, 10, SAM_ALL_TAGS)
        assert any("N" in c for c, _ in want[3] if c) and (want[0]["nm"] == 0).any()


# ------------------------------------------------------------------------------------------------ through the mapper
DELS, HEADS = (9, 10, 11, 40, 300), (40, 60, 75)


def _reference():
    rng = np.random.default_rng(21)
    return R.pack([("g%d" % i, ACGT[rng.integers(0, 4, n)]) for i, n in enumerate((3000, 1800, 2600, 900, 2200))])


def _spliced(p, rng, d, h):
    """ref[a : a + h] + ref[a + h + d : ...] of 100..150 bases inside one scaffold, and the scaffold segment 200 bases further down"""
    sb = [s for s in p.scaffold_bases() if s[2] >= 1500]
    c, start, n = sb[int(rng.integers(0, len(sb)))]
    ln = int(rng.integers(100, 151))
    a = start + int(rng.integers(20, n - ln - d - 420))
    ch = p.chroms[c - 1]
    rd = np.concatenate([ch[a: a + h], ch[a + h + d: a + d + ln]])
    assert len(rd) == ln
    mate_ln = int(rng.integers(100, 151))
    return rd, ch[a + d + ln + 200: a + d + ln + 200 + mate_ln].copy()


def _planted(p, paired, seed):
    rng = np.random.default_rng(seed)
    reads, plan = [], []
    for rep in range(4):
        for d in DELS:
            for h in HEADS:
                rd, down = _spliced(p, rng, d, h)
                minus = bool((rep + d + h) & 1)
                if not paired:
                    reads.append(_rc(rd) if minus else rd); plan.append((d, h))
                elif minus:                                 # mate 2 carries the deletion, on the minus strand
                    reads += list(_mirror(p, rng, d, h)); plan += [None, (d, h)]
                else:
                    reads += [rd, _rc(down)]; plan += [(d, h), None]
    return reads, plan


def _mirror(p, rng, d, h):
    """a pair whose mate 1 is a plain plus-strand read and whose mate 2, further down and on the minus strand, carries the deletion"""
    sb = [s for s in p.scaffold_bases() if s[2] >= 1500]
    c, start, n = sb[int(rng.integers(0, len(sb)))]
    ch = p.chroms[c - 1]
    l1, ln = int(rng.integers(100, 151)), int(rng.integers(100, 151))
    a = start + int(rng.integers(20, n - l1 - 200 - ln - d - 20))
    b = a + l1 + 200
    return ch[a: a + l1].copy(), _rc(np.concatenate([ch[b: b + h], ch[b + h + d: b + d + ln]]))


def _ops(cigar):
    ops = [(int(n), o) for n, o in OPS.findall(cigar)]
    assert "".join("%d%s" % x for x in ops) == cigar, cigar
    return ops


@pytest.mark.parametrize("paired", [False, True])
def test_mapper_planted_deletions_at_limit_10(paired):
    p = _reference()
    reads, plan = _planted(p, paired, 30 + paired)
    di = DeviceIndex.build(p.chroms, k=13)
    mp = None
    try:
        di.set_scaffolds(p)
        recs_in, blob, bs, ki = K.make_batch(reads)
        mp = Mapper.from_records(di, recs_in, blob, bs, ki, paired=paired, max_sites=64)
        mp.step()
        st = mp.stats()
        assert st["reads_overflowed"] == 0 and st["reads_reprobed"] == 0
        before = {fl: mp.sam_records(fl) for fl in FLAGS}                        # the default call, first
        fin, mblob = mp.final()
        matches = [mblob[int(f["match_off"]): int(f["match_off"]) + int(f["match_len"])].tobytes() if int(f["match_len"]) > 0 else None for f in fin]
        out = mp.fetch(with_match=False)
        scores = [[int(x) for x in out["sites"][r, :max(0, int(out["nsites"][r]))]["score"]] for r in range(len(reads))]
        lens = [len(r) for r in reads]
        tab = SC.table_of(p)
        scaf, _ = mp.scaffold_records()
        for flags in FLAGS:
            recs, tg, text = mp.sam_records(flags, intron_limit=10, tags=SAM_ALL_TAGS)
            want = SP.sam_records(tab, fin, matches, lens, reads, p.chroms, paired, flags, 10, SAM_ALL_TAGS, scores)
            _equal((recs, tg, text, len(text)), want, flags)
            hrecs, htg, htext = mp.sam_records_host(flags, intron_limit=10, tags=SAM_ALL_TAGS)
            assert np.array_equal(hrecs, recs) and np.array_equal(htg, tg) and htext.tobytes() == text.tobytes()
            # at no limit the new path is the old call, byte for byte; and the old call still returns what it returned
            urecs, utg, utext = mp.sam_records(flags, intron_limit=SAM_NO_INTRON_LIMIT)
            after = mp.sam_records(flags)
            for x in (urecs, after[0]):
                assert np.array_equal(x, before[flags][0])
            assert utext.tobytes() == after[1].tobytes() == before[flags][1].tobytes()
            assert not utg["present"].any() and not utg["introns"].any() and not utg["splices"].any()
        # ---- independent of the restatement
        recs, tg, text = mp.sam_records(SAM_MD, intron_limit=10, tags=SAM_ALL_TAGS)
        hit = dict.fromkeys(["long_N", "d10_D", "d11_N", "minus_mate2_xs"], 0)
        hit["long"] = sum(1 for x in plan if x and x[0] > 10)            # every constructed read with d > 10, mapped or not
        for r, rec in enumerate(recs):
            if int(rec["flag"]) & 4 or int(rec["cigar_len"]) == 0:
                assert int(tg[r]["introns"]) == 0 and not int(tg[r]["present"]) & SAM_MAKE_XS
                continue
            cigar = text[int(rec["cigar_off"]): int(rec["cigar_off"]) + int(rec["cigar_len"])].tobytes().decode()
            ops = _ops(cigar)
            assert sum(n for n, o in ops if o in "M=XIS") == lens[r], (r, cigar)
            if int(scaf[r]["flags"]) & SC.INBOUNDS:
                assert sum(n for n, o in ops if o in "M=XDN") == int(scaf[r]["end"]) - int(scaf[r]["pos"]) + 1, (r, cigar)
            assert all(n > 10 for n, o in ops if o == "N") and all(n <= 10 for n, o in ops if o == "D"), cigar
            n_ops = sum(1 for _, o in ops if o == "N")
            assert int(tg[r]["introns"]) == n_ops and bool(int(tg[r]["present"]) & SAM_MAKE_XS) == (n_ops > 0)
            if n_ops and paired and r & 1 and int(rec["flag"]) & 0x10:
                hit["minus_mate2_xs"] += 1
                assert int(tg[r]["xs"]) == 1                 # minus, inverted for mate 2
            if plan[r]:
                d = plan[r][0]
                hit["long_N"] += d > 10 and n_ops > 0
                hit["d10_D"] += d == 10 and (10, "D") in ops; hit["d11_N"] += d == 11 and (11, "N") in ops
        print("planted:", hit, "splice counts:", SAM.splice_counts(tg, paired))
        assert 2 * hit["long_N"] >= hit["long"] > 0, hit
        assert hit["d10_D"] > 0 and hit["d11_N"] > 0, hit
        if paired:
            assert hit["minus_mate2_xs"] > 0, hit
        lines = SAM.lines(recs, text, ["q%d" % i for i in range(len(reads))], reads, None, di.scaffold_names, paired, tags=tg)
        assert sum("XS:A:" in ln for ln in lines) == int((tg["xs"] != 0).sum()) > 0
    finally:
        if mp is not None:
            mp.close()
        di.close()


def test_cfg_error_returns():
    p = _reference()
    reads, _ = _planted(p, False, 33)
    di = DeviceIndex.build(p.chroms, k=13)
    mp = None
    try:
        di.set_scaffolds(p)
        mp = Mapper.from_records(di, *K.make_batch(reads[:8]), paired=False, max_sites=64)
        a, g, t, nb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64(0)
        call = lambda cfg: mp.L.bbmap_get_sam_records_cfg(mp.h, None, C.byref(cfg), C.byref(a), C.byref(g), C.byref(t), C.byref(nb))
        assert call(sam_config()) == -2                     # no batch yet
        mp.step()
        assert call(sam_config()) == 0 and nb.value > 0
        assert call(sam_config(intron_limit=-1)) == -2 and mp.L.bbmap_last_error() == b"bbmap_get_sam_records_cfg: negative intron limit"
        assert call(sam_config(tags=1 << 14)) == -2 and call(sam_config(flags=4)) == -2
        assert call(sam_config(intron_limit=0, tags=SAM_ALL_TAGS)) == 0
        assert mp.L.bbmap_get_sam_records_cfg(mp.h, None, None, C.byref(a), C.byref(g), C.byref(t), C.byref(nb)) == -2
    finally:
        if mp is not None:
            mp.close()
        di.close()
