"""The final alignment stage for the mapPacBio profile (bbmap_config.finalStage on BBIDX_PROFILE_PACBIO).

finalStage = 1 runs BBMapThreadPacBio's tail (current/align2/BBMapThreadPacBio.java:497-670, :1088-1290) with MultiStateAligner9PacBio's
points; finalStage = 2 runs BBMapThread's tail with the same points.  The CPU oracle compiled with -DORC_PACBIO restates the second
(oracle/mapper_oracle.c:758), so the verification is split:
  * the SCHEME: device finalStage = 2 against the oracle, exactly -- records, match strings byte for byte, the lists after the stage and
    every fill -- on long pieces (the stage alone, the whole flow, pairs);
  * the POLICY: for each rule in which BBMapThreadPacBio's tail differs, site lists on which the two tails give different records;
    the finalStage = 1 record equals a short Python restatement of the cited Java lines and differs from the oracle's;
  * the fixture: the PhiX reads through the PacBio classes with finalStage = 1, judged by the truth in their names."""
import ctypes as C

import numpy as np
import pytest

from bbmap_amd import keys as K
from bbmap_amd import workload as W
from bbmap_amd.index import DeviceIndex, PROFILE_PACBIO
from bbmap_amd.mapper import MSITE_DTYPE, Mapper
from oracle import oracle as O
from tests.final_problems import perturb
from tests.mapper_check import compare

pytestmark = pytest.mark.gpu
PB = PROFILE_PACBIO
ACGT = np.frombuffer(b"ACGT", np.uint8)
FSTRIDE = 81920                     # the oracle's per-read match-string buffer: room for the > 64 KiB strings below


def max_sw(L):                      # MultiStateAligner9PacBio.maxQuality(numBases)
    return 90 + (L - 1) * 100


def _mutate(rng, seg, rate):
    """PacBio-like damage: deletions / substitutions / insertions 35 : 20 : 45 at `rate` per base"""
    out = []
    for b in seg:
        u = rng.random()
        if u < rate * 0.35:
            continue
        if u < rate * 0.55:
            out.append(ACGT[(int(np.searchsorted(ACGT, b)) + 1 + int(rng.integers(0, 3))) % 4])
            continue
        if u < rate:
            out.append(ACGT[int(rng.integers(0, 4))])
        out.append(b)
    return np.asarray(out, np.uint8)


def check_invariants(fin, blob, lens, sites=None, nsites=None):
    """every mapped record's string consumes exactly the read (m S N I X Y C) and spans exactly [start, stop] (m S N D X Y C); bit 31 of
    every returned site's reserved[1] is clear.  Returns the longest string."""
    longest = 0
    for r in range(len(fin)):
        f = fin[r]
        ml = int(f["match_len"])
        if f["mapped"] and ml:
            m = blob[int(f["match_off"]): int(f["match_off"]) + ml].tobytes()
            assert sum(m.count(c) for c in b"mSNIXYC") == int(lens[r]), r
            assert sum(m.count(c) for c in b"mSNDXYC") == int(f["stop"]) - int(f["start"]) + 1, r
            longest = max(longest, ml)
    if sites is not None:
        for r in range(len(nsites)):
            n = int(nsites[r])
            if n > 0:
                assert not (sites[r, :n]["reserved"][:, 1].astype(np.int64) & 0x80000000).any(), r
    return longest


def _mapper(di, recs, blob, bs, ki, stage, paired=False, max_sites=32, **kw):
    return Mapper.from_records(di, recs, blob, bs, ki, paired=paired, max_sites=max_sites, profile=PB, finalStage=stage, **kw)


def _lists(di, recs, blob, bs, ki, max_sites=32):
    """the site lists as scoreSlow leaves them (finalStage = 0), and the bases buffer with the reverse complements the step wrote"""
    mp = _mapper(di, recs, blob, bs, ki, 0, max_sites=max_sites)
    mp.step()
    out = mp.fetch()
    bases = mp.bases.clone()
    mp.close()
    s, ns = out["sites"].copy(), np.maximum(out["nsites"], 0).astype(np.int32)
    return s, ns, bases


def _stage(di, recs, blob, bs, ki, bases, s, ns, stage, paired=False, **kw):
    mp = _mapper(di, recs, blob, bs, ki, stage, paired=paired, max_sites=s.shape[1], **kw)
    mp.bases.copy_(bases)
    mp.final_only(s, ns)
    out, st = mp.fetch(), mp.stats()
    mp.close()
    return out, st


# ---------------------------------------------------------------------------------------------- 1. scheme parity (finalStage = 2)
@pytest.fixture(scope="module")
def long_problem():
    """a 420 kb reference; pieces of 4000-6000 and 1000-2000 bases (make_pacbio_pieces), and two reads across a 70 kb deletion whose
    gapped site gives match strings longer than 64 KiB"""
    ref = W.make_reference(420000, seed=91, pad=8000, repeat_frac=0.05, families=40)
    chroms = [ref]
    longp, _ = W.make_pacbio_pieces(chroms, 8, seed=11, min_len=4000, max_len=6000, pad=8000)
    shortp, _ = W.make_pacbio_pieces(chroms, 16, seed=12, min_len=1000, max_len=2000, pad=8000)
    rng = np.random.default_rng(13)
    gapped, gsites = [], []
    for a in (20000, 150000):
        d = 70000
        r = np.concatenate([ref[a:a + 2500], ref[a + 2500 + d:a + 5000 + d]]).copy()
        for q in rng.integers(0, len(r), 30):
            r[q] = ACGT[(int(np.searchsorted(ACGT, r[q])) + 1) % 4]
        gapped.append(r)
        gsites.append((a, a + 2499, a + 2500 + d, a + 4999 + d))
    pieces = longp + shortp + gapped
    recs, blob, bs, ki = K.make_batch(pieces, None, K.default_config(K.PROFILE_PACBIO))
    di = DeviceIndex.build(chroms, profile=PB)
    s, ns, bases = _lists(di, recs, blob, bs, ki)
    s, ns = perturb(s, ns, 17, len(ref))
    s["match_job"] = -1
    s["reserved"] = 0
    n0 = len(longp) + len(shortp)
    for q, g in enumerate(gsites):                       # the gapped sites, planted as the probe would report them (BBIndex gaps)
        r = n0 + q
        s[r] = np.zeros(1, MSITE_DTYPE)[0]
        t = s[r, 0].copy()
        t["chrom"], t["strand"], t["start"], t["stop"], t["hits"] = 1, 0, g[0], g[3], 20
        t["score"] = t["slowScore"] = t["quickScore"] = int(0.9 * max_sw(len(gapped[q])))
        t["ngaps"] = 4
        t["gaps"][:4] = g
        t["match_job"] = -1
        s[r, 0] = t
        ns[r] = 1
    yield dict(ref=ref, chroms=chroms, pieces=pieces, recs=recs, blob=blob, bs=bs, ki=ki, di=di, s=s, ns=ns, bases=bases, n_gapped=len(gapped))
    di.close()


def _check_gapped(out, P):
    """the reads across the 70 kb deletion: 2,500 + 2,500 aligned bases around one run of 70,000 'D's, at the planted coordinates"""
    fin, blob = out["final"], out["final_match"]
    n0 = len(P["pieces"]) - P["n_gapped"]
    for q in range(P["n_gapped"]):
        r = n0 + q
        f = fin[r]
        g = P["s"][r, 0]["gaps"][:4]
        m = blob[int(f["match_off"]): int(f["match_off"]) + int(f["match_len"])].tobytes()
        assert f["mapped"] and (int(f["start"]), int(f["stop"])) == (int(g[0]), int(g[3])), f
        assert len(m) == 75000 and m.count(b"D") == 70000 and b"D" * 70000 in m and m.count(b"S") <= 30, (len(m), m.count(b"D"))
        assert int(f["mapScore"]) > 0.97 * max_sw(5000)


def test_stage_alone_equals_the_oracle_on_long_pieces(long_problem):
    """every piece against the oracle; the two reads across the 70 kb deletion are checked by their known answer instead: their
    75,000-byte strings exceed the oracle's traceback buffer (rows + columns + 8,256 bytes, oracle/mapper_oracle.c:919), which then
    reports no string for the fill"""
    P = long_problem
    n = len(P["pieces"])
    n0 = n - P["n_gapped"]
    out, st = _stage(P["di"], P["recs"], P["blob"], P["bs"], P["ki"], P["bases"], P["s"], P["ns"], 2)
    oi = O.OracleIndex(P["chroms"], profile="pacbio")
    orc = O.final_reads(oi, P["recs"], P["blob"], P["s"], P["ns"], params=O.map_default_params("pacbio", finalStage=1), match_stride=FSTRIDE)
    bad = compare(out, orc, n, False, reads_range=range(n0))
    assert not bad, "\n".join(bad[:20])
    assert st["final_fills"] == len(orc["log"]) and st["final_fills"] > 20
    longest = check_invariants(out["final"], out["final_match"], P["recs"]["len"], out["sites"], out["nsites"])
    assert longest > 65535, longest                       # the reads across the 70 kb deletion: 70,000 'D's in one string
    _check_gapped(out, P)
    assert int(out["final"]["mapped"].sum()) >= n - 4
    # and the profile's own tail (finalStage = 1) keeps the invariants on the same lists
    out1, _ = _stage(P["di"], P["recs"], P["blob"], P["bs"], P["ki"], P["bases"], P["s"], P["ns"], 1)
    assert check_invariants(out1["final"], out1["final_match"], P["recs"]["len"], out1["sites"], out1["nsites"]) > 65535
    _check_gapped(out1, P)


def test_whole_flow_equals_the_oracle():
    ref = W.make_reference(300000, seed=93, pad=8000, repeat_frac=0.05, families=40)
    chroms = [ref]
    pieces, _ = W.make_pacbio_pieces(chroms, 3, seed=21, min_len=4000, max_len=6000, pad=8000)
    p2, _ = W.make_pacbio_pieces(chroms, 12, seed=22, min_len=1000, max_len=2000, pad=8000)
    pieces = pieces + p2
    recs, blob, bs, ki = K.make_batch(pieces, None, K.default_config(K.PROFILE_PACBIO))
    di = DeviceIndex.build(chroms, profile=PB)
    mp = _mapper(di, recs, blob, bs, ki, 2)
    mp.step()
    out, st = mp.fetch(), mp.stats()
    mp.close()
    di.close()
    oi = O.OracleIndex(chroms, profile="pacbio")
    orc = O.map_reads(oi, recs, blob, ki, base_scores=bs, paired=False, cap=64, threads=8,
                      params=O.map_default_params("pacbio", finalStage=1))
    bad = compare(out, orc, len(pieces), False)
    assert not bad, "\n".join(bad[:20])
    assert st["reads_overflowed"] == 0 and st["final_fills"] > 5
    check_invariants(out["final"], out["final_match"], recs["len"], out["sites"], out["nsites"])
    assert int(out["final"]["mapped"].sum()) >= len(pieces) - 2


def test_paired_stage_equals_the_oracle():
    """mates of 1000-1800 bases, 3-4 kb fragments: the paired tail (final pairing, canPair, genMatchString per mate)"""
    ref = W.make_reference(300000, seed=95, pad=8000, repeat_frac=0.05, families=40)
    rng = np.random.default_rng(31)
    reads = []
    for p in range(14):
        a = int(rng.integers(9000, len(ref) - 14000))
        frag = ref[a:a + int(rng.integers(3000, 4000))]
        m1 = _mutate(rng, frag[:int(rng.integers(1000, 1800))], 0.12)
        m2 = _mutate(rng, W.revcomp_rows(frag[-int(rng.integers(1000, 1800)):].reshape(1, -1))[0], 0.12)
        if p % 5 == 4:                                    # a mate from elsewhere: no pair
            b = int(rng.integers(9000, len(ref) - 14000))
            m2 = _mutate(rng, ref[b:b + 1200], 0.12)
        reads += [m1, m2]
    recs, blob, bs, ki = K.make_batch(reads, None, K.default_config(K.PROFILE_PACBIO))
    di = DeviceIndex.build([ref], profile=PB)
    s, ns, bases = _lists(di, recs, blob, bs, ki)
    s["match_job"] = -1
    s["reserved"] = 0
    out, st = _stage(di, recs, blob, bs, ki, bases, s, ns, 2, paired=True)
    di.close()
    oi = O.OracleIndex([ref], profile="pacbio")
    orc = O.final_reads(oi, recs, blob, s, ns, paired=True, params=O.map_default_params("pacbio", finalStage=1), match_stride=FSTRIDE)
    bad = compare(out, orc, len(reads), True)
    assert not bad, "\n".join(bad[:20])
    assert st["final_fills"] == len(orc["log"])
    check_invariants(out["final"], out["final_match"], recs["len"], out["sites"], out["nsites"])
    assert 0 < int(out["final"]["paired"].sum()) < len(reads)


# ---------------------------------------------------------------------------------------------- 2. policy: BBMapThreadPacBio's tail
CZ = dict(P=150, b1=220, b1b=280, b1c=480)               # (int)(CLEARZONE_RATIO* x POINTS_MATCH2), BBMapThreadPacBio.java:38-41, :112-115


def pacbio_clearzone(perfect, score, msw):
    """BBMapThreadPacBio.java:499-501 (single) and :1094-1096 (paired): the same step rule"""
    if perfect:
        return CZ["P"]
    if score >= int(np.float32(msw) * np.float32(0.92)):
        return CZ["b1"]
    if score >= int(np.float32(msw) * np.float32(0.82)):
        return CZ["b1b"]
    return CZ["b1c"]


def count_top_scores(lst, thresh):                       # Tools.countTopScores (Tools.java:913-930)
    count, limit = 1, int(lst[0]["score"]) - thresh
    for x in lst[1:]:
        if int(x["score"]) < limit:
            break
        if int(lst[0]["start"]) != int(x["start"]) and int(lst[0]["stop"]) != int(x["stop"]):
            count += 1
    return count


def apply_clearzone3(mapScore, slow, L, CZ3, INV):     # AbstractMapThread.applyClearzone3 (:1820-1870); slow: the list's slowScores
    f32 = np.float32
    mults = [0, 1, .75, 0.5, 0.25, 0.125, 0.0625]
    sub = f32(0)
    for i in range(1, min(7, len(slow))):
        if i > 2 and slow[i] < slow[i - 1]:
            break
        dif = slow[0] - slow[i]
        if dif >= CZ3:
            break
        g = f32(CZ3 - dif) * f32(INV)
        fr = g + f32(2) * (g * g) + f32(2) * (g * g) * g
        if fr <= 0:
            break
        sub = f32(sub + f32(fr * f32(mults[i])))
    if sub <= 0:
        return 0
    asym = f32(4) + f32(0.03) * f32(L)
    sub = f32(sub * f32(1.8))
    subi = int(f32(f32(CZ3) * f32(f32(asym * sub) / f32(sub + asym))) + f32(0.5))
    subi = min(subi, mapScore - 300)
    return max(subi, 0)


def tip_penalty(mapScore, match, bases, msw, tiplen=7):  # calcTipScorePenalty (AbstractMapThread.java:2499-2573)
    L = len(bases)
    points = 0
    for seq in (match, match[::-1]):
        prev, cpos = ord("m"), 0
        for b in seq:
            if cpos > tiplen:
                break
            if b == ord("m"):
                cpos += 1
            elif b == ord("D"):
                if prev != ord("D"):
                    points += 2 * (tiplen + 2 - cpos)
            elif b in (ord("N"), ord("C")):
                points += tiplen + 2 - cpos
                cpos += 1
            else:
                points += 2 * (tiplen + 2 - cpos)
                cpos += 1
            prev = b
    b = bases[0]
    if b != ord("N") and b == bases[1]:
        i = 2
        while i <= tiplen and bases[i] == b:
            points += 1
            i += 1
    b, last = bases[L - 1], L - 1
    if b != ord("N") and b == bases[last - 1]:
        i = last - 2
        while i >= last - tiplen and bases[i] == b:
            points += 1
            i -= 1
    if points < 1:
        return 0
    f32 = np.float32
    fr = f32(f32(80) * f32(points)) / f32(f32(points) + f32(80))
    pen = int(f32(fr * f32(0.0022)) * f32(msw))
    mx = mapScore - msw // 10
    return 0 if mx <= 0 else min(pen, mx)


def _site(chrom, strand, start, stop, score, perfect=0):
    t = np.zeros(1, MSITE_DTYPE)[0]
    t["chrom"], t["strand"], t["start"], t["stop"], t["hits"] = chrom, strand, start, stop, 10
    t["quickScore"] = t["score"] = t["slowScore"] = score
    t["perfect"] = t["semiperfect"] = perfect
    t["match_job"] = -1
    return t


@pytest.fixture(scope="module")
def policy_ref():
    ref = W.make_reference(400000, seed=97, pad=8000)
    di = DeviceIndex.build([ref], profile=PB)
    yield ref, di
    di.close()


def _policy_run(ref, di, reads, lists, paired=False, cap=128, **params):
    """device finalStage 1 and 2 and the oracle over the same hand-made lists; asserts device 2 == oracle exactly"""
    recs, blob, bs, ki = K.make_batch(reads, None, K.default_config(K.PROFILE_PACBIO))
    s = np.zeros((len(reads), cap), MSITE_DTYPE)
    ns = np.zeros(len(reads), np.int32)
    for r, lst in enumerate(lists):
        for i, t in enumerate(lst):
            s[r, i] = t
        ns[r] = len(lst)
    pre = _mapper(di, recs, blob, bs, ki, 0, paired=paired, max_sites=cap, **params)
    pre.step()                                            # (the reverse complements)
    bases = pre.bases.clone()
    pre.close()
    out1, _ = _stage(di, recs, blob, bs, ki, bases, s, ns, 1, paired=paired, **params)
    out2, _ = _stage(di, recs, blob, bs, ki, bases, s, ns, 2, paired=paired, **params)
    oi = O.OracleIndex([ref], profile="pacbio")
    op = O.map_default_params("pacbio", finalStage=1, **params)
    orc = O.final_reads(oi, recs, blob, s, ns, paired=paired, params=op, match_stride=FSTRIDE)
    bad = compare(out2, orc, len(reads), paired)
    assert not bad, "\n".join(bad[:20])
    for o in (out1, out2):
        check_invariants(o["final"], o["final_match"], recs["len"], o["sites"], o["nsites"])
    return out1, out2, orc


def test_single_clearzone_is_a_step_rule(policy_ref):
    """BBMapThreadPacBio.java:499-510 (cutoffs 0.92 / 0.82 of maxSwScore, :53-54) against BBMapThread's interpolation (:508-525): a second
    site 250 below a top site at 0.95 x maxSwScore lies outside CLEARZONE1 = 220 but inside BBMapThread's interpolated zone (~300)"""
    ref, di = policy_ref
    L, reads, lists = 1500, [], []
    for q in range(6):
        a = 20000 + 50000 * q
        reads.append(ref[a:a + L].copy())
        top = int(0.95 * max_sw(L)) + 40 * q
        lists.append([_site(1, 0, a, a + L - 1, top), _site(1, 0, a + 200000 - 7000 * q, a + 200000 - 7000 * q + L - 1, top - 250)])
    out1, _, orc = _policy_run(ref, di, reads, lists)
    for r, lst in enumerate(lists):
        want = int(count_top_scores(lst, pacbio_clearzone(False, int(lst[0]["score"]), max_sw(L))) > 1)
        assert int(out1["final"]["ambiguous"][r]) == want == 0
        assert int(orc["final"]["ambiguous"][r]) == 1      # discriminates: BBMapThread's zone takes the second site in


def test_no_clearzone1e_block(policy_ref):
    """BBMapThread counts sites within CLEARZONE1e (2 x 100 - 90 + 137 + 1 = 248 here) when the list is long (:517-525, CLEARZONE_LIMIT1e = 40: more than 81 of them
    make the read ambiguous); BBMapThreadPacBio has no such block (:505-510)"""
    ref, di = policy_ref
    L = 1200
    reads, lists = [], []
    for q in range(2):
        a = 30000 + 100000 * q
        reads.append(ref[a:a + L].copy())
        top = max_sw(L) - 100
        lst = [_site(1, 0, a, a + L - 1, top)]
        for k in range(90):
            b = 250000 + 1500 * k + 37 * q
            lst.append(_site(1, 0, b, b + L - 1, top - 230))
        lists.append(lst)
    out1, _, orc = _policy_run(ref, di, reads, lists)
    for r, lst in enumerate(lists):
        cz = pacbio_clearzone(False, int(lst[0]["score"]), max_sw(L))
        assert cz == 220 and count_top_scores(lst, cz) == 1 and count_top_scores(lst, 248) == 91
        assert int(out1["final"]["ambiguous"][r]) == 0
        assert int(orc["final"]["ambiguous"][r]) == 1


def test_fixed_clearzone3(policy_ref):
    """applyClearzone3(r, CLEARZONE3, INV_CLEARZONE3) (BBMapThreadPacBio.java:633-641) against BBMapThread's cz3v2 = CLEARZONE3 x
    min(1.25, maxSw / mapScore) (:668-682): a second site whose distance lies between 800 and cz3v2.  The restatement starts from the
    oracle-pinned finalStage = 2 intermediate of a run without clearzone3 (no applyClearzone3, no tip penalty)."""
    ref, di = policy_ref
    L = 1500
    rng = np.random.default_rng(41)
    reads, base = [], []
    for q in range(4):
        a = 40000 + 60000 * q
        r = ref[a:a + L].copy()
        for p in rng.choice(np.arange(20, L - 20), 70, replace=False):
            r[p] = ACGT[(int(np.searchsorted(ACGT, r[p])) + 1) % 4]
        reads.append(r)
        base.append(a)
    first = [[_site(1, 0, a, a + L - 1, int(0.85 * max_sw(L)))] for a in base]
    _, mid, _ = _policy_run(ref, di, reads, first, clearzone3=0)
    lists = []
    for r, a in enumerate(base):
        T = int(mid["final"]["mapScore"][r])
        q = np.float32(max_sw(L)) / np.float32(T)
        cz3v2 = int(np.float32(800) * min(np.float32(1.25), q))
        assert cz3v2 > 820, cz3v2
        gap = (800 + cz3v2) // 2
        lists.append([_site(1, 0, a, a + L - 1, T), _site(1, 0, a + 300000, a + 300000 + L - 1, T - gap)])
    mids = []
    for r in range(len(reads)):
        f = mid["final"][r]
        mids.append((int(f["mapScore"]), mid["final_match"][int(f["match_off"]): int(f["match_off"]) + int(f["match_len"])].copy()))
    out1, _, orc = _policy_run(ref, di, reads, lists)
    for r in range(len(reads)):
        T, m = mids[r]
        slow = [T, int(lists[r][1]["slowScore"])]
        sub = apply_clearzone3(T, slow, L, 800, np.float32(1) / np.float32(800))
        assert sub == 0                                      # outside the fixed zone
        want = T - sub
        want -= tip_penalty(want, m.tobytes(), reads[r].tobytes(), max_sw(L))
        assert int(out1["final"]["mapScore"][r]) == want, (r, int(out1["final"]["mapScore"][r]), want)
        assert int(orc["final"]["mapScore"][r]) < want       # BBMapThread's wider zone takes points off


def test_paired_clearzone_uses_plain_cutoffs(policy_ref):
    """BBMapThreadPacBio.java:1094-1096: CUTOFF x maxSw (CLEARZONE1 = 220) against BBMapThread's SCALE x maxSw - FLAT (:1158-1160,
    CLEARZONE1 = 200): a second site 210 below the top makes the PacBio read ambiguous and leaves BBMapThread's unique.  Both mates' sites
    lie on the plus strand, so the final pairing finds no pair and leaves the scores as given."""
    ref, di = policy_ref
    L = 1300
    reads, lists = [], []
    for q in range(3):
        a = 25000 + 80000 * q
        reads += [ref[a:a + L].copy(), ref[a + 5000:a + 5000 + L].copy()]
        top = max_sw(L) - 500
        lists.append([_site(1, 0, a, a + L - 1, top), _site(1, 0, a + 200000, a + 200000 + L - 1, top - 210)])
        lists.append([_site(1, 0, a + 5000, a + 5000 + L - 1, top)])
    out1, _, orc = _policy_run(ref, di, reads, lists, paired=True)
    for q in range(3):
        lst = lists[2 * q]
        want = int(count_top_scores(lst, pacbio_clearzone(False, int(lst[0]["score"]), max_sw(L))) > 1)
        assert int(out1["final"]["ambiguous"][2 * q]) == want == 1
        assert int(orc["final"]["ambiguous"][2 * q]) == 0


def test_no_xy_saving_changes_nothing_under_the_defaults(policy_ref):
    """processAmbiguous(.., save_xy = false) (BBMapThreadPacBio.java:507) returns true at once (AbstractMapThread.java:1424-1425);
    BBMapThread passes SAVE_AMBIGUOUS_XY, false under bbmap.sh's defaults, and its own comment says the call "never gets executed
    anymore, so always returns true" (BBMapThread.java:532).  No list can tell the two apart: this test pins the shared outcome -- a
    read whose top sites tie is ambiguous under both tails."""
    ref, di = policy_ref
    L = 1000
    a = 60000
    lists = [[_site(1, 0, a, a + L - 1, max_sw(L) - 1000), _site(1, 0, a + 100000, a + 100000 + L - 1, max_sw(L) - 1000)]]
    out1, out2, orc = _policy_run(ref, di, [ref[a:a + L].copy()], lists)
    assert int(out1["final"]["ambiguous"][0]) == int(out2["final"]["ambiguous"][0]) == int(orc["final"]["ambiguous"][0]) == 1


# ---------------------------------------------------------------------------------------------- 3. the PhiX fixture, finalStage = 1
# (mapped, strict, loose) of the FINAL records per sample, floors against the truth in the read names (the lists' are FLOORS_PACBIO,
# test_golden_phix.py).  Sample1's sit one read below the lists' in `mapped` and one in `strict`, for the two reads below, in both runs.
FLOORS_FINAL_PACBIO = {1: (99, 79, 99), 2: (98, 78, 97)}
FINAL_BELOW_LISTS = {1: {
    # its list's top site has slowScore 0, below (int)(maxSwScore x MINIMUM_ALIGNMENT_SCORE_RATIO 0.46) = 4,595: `r.sites=null`
    # (BBMapThreadPacBio.java:514-516), reported unmapped
    15: "unmapped",
    # a junk 14-base left tip and an 11-base insertion: genMatchStringForSite's realign_new (AbstractMapThread.java:968-1034,
    # TranslateColorspaceRead.java:229-653) aligns the tip as substitutions (SSmmSSNSSSSmmSSSS...IIIIIIIIIII...) and moves the start
    # 14 bases left of the truth; the stop stays (a loose hit).  The oracle's BBMapThread tail gives the same string.
    47: "start moved",
}, 2: {}}


def test_fixture_final_records():
    """the four PhiX runs through the PacBio classes with finalStage = 1: floors on the final records, a strict top site stays strict,
    every mapped read's string consumes the read and spans [start, stop], the reads reported unmapped are the low-scoring ones"""
    from tests.golden_phix import PACBIO_MSA, fixture_runs_pacbio, phix_reference, sample_reads
    from tests.test_golden_phix import _final_against_truth, _score_against_truth
    ref = phix_reference()
    di = DeviceIndex.build([ref], profile=PB)
    min_score = int(np.float32(0.46) * np.float32(max_sw(100)))
    got, lost = {}, {}
    for name, r in fixture_runs_pacbio().items():
        recs, blob, bs, ki, _ = r["inputs"]
        which = int(name[2])
        _, truth = sample_reads(which)
        lists = _mapper(di, recs, blob, bs, ki, 0, msaMaxColumns=PACBIO_MSA["msaMaxColumns"])
        lists.step()
        pre = lists.fetch()
        lists.close()
        mp = _mapper(di, recs, blob, bs, ki, 1, msaMaxColumns=PACBIO_MSA["msaMaxColumns"])
        mp.step()
        out = mp.fetch()
        mp.close()
        fin, blob_ = out["final"], out["final_match"]
        got[name] = _final_against_truth(fin, truth)
        print(name, "final", got[name], "lists", _score_against_truth(pre["sites"], pre["nsites"], truth))
        check_invariants(fin, blob_, recs["len"], out["sites"], out["nsites"])
        top = pre["sites"][:, 0]
        lost[name] = []
        for i in range(100):
            was_strict = pre["nsites"][i] > 0 and top["strand"][i] == truth["strand"][i] and top["start"][i] == truth["start"][i] and top["stop"][i] == truth["stop"][i]
            if fin["mapped"][i]:
                if was_strict and FINAL_BELOW_LISTS[which].get(i) != "start moved":
                    assert (fin["start"][i], fin["stop"][i]) == (truth["start"][i], truth["stop"][i]), (name, i)
                if FINAL_BELOW_LISTS[which].get(i) == "start moved":
                    assert fin["stop"][i] == truth["stop"][i] and fin["start"][i] == truth["start"][i] - 14, (name, i)
            elif pre["nsites"][i] > 0:
                assert FINAL_BELOW_LISTS[which].get(i) == "unmapped", (name, i)
                lost[name].append((i, int(top["slowScore"][i]), int(fin["mapScore"][i])))
                assert top["slowScore"][i] < min_score + 300, (name, i, int(top["slowScore"][i]))
        print(name, "mapped in the lists, unmapped in the final records (read, list slowScore, mapScore):", lost[name])
    di.close()
    for name, g in got.items():
        assert all(x >= f for x, f in zip(g, FLOORS_FINAL_PACBIO[int(name[2])])), (name, g)


# ---------------------------------------------------------------------------------------------- 5. creation, C ABI and JNI glue
def test_create_with_final_stage_returns_records():
    ref = W.make_reference(200000, seed=99, pad=8000)
    pieces, truth = W.make_pacbio_pieces([ref], 6, seed=5, min_len=800, max_len=1500, pad=8000)
    recs, blob, bs, ki = K.make_batch(pieces, None, K.default_config(K.PROFILE_PACBIO))
    di = DeviceIndex.build([ref], profile=PB)
    mp = Mapper.from_records(di, recs, blob, bs, ki, max_sites=32, profile=PB)
    assert mp.cfg.finalStage == 0                            # the profile's default is unchanged: the stage is opt-in
    mp.close()
    mp = _mapper(di, recs, blob, bs, ki, 1)
    mp.step()
    fin, m = mp.final()
    mp.close()
    assert int(fin["mapped"].sum()) >= 5 and int(fin["match_len"].sum()) == len(m)
    for r in range(len(pieces)):
        if fin["mapped"][r]:
            assert int(fin["strand"][r]) == int(truth[r][1]) and abs(int(fin["start"][r]) - int(truth[r][2])) < 200
    # the JNI glue: BBMapHIP(index, paired, maxReads, maxReadLen, maxSites, finalStage = 1) through a minimal JNIEnv
    _jni_glue(di, recs, blob, bs, ki, fin, m)
    di.close()


def _jni_glue(di, recs, blob, bs, ki, fin_c, match_c):
    import os
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bbmap_amd", "libbbmap_amd_jni.so"))

    class Buf(C.Structure):                               # the mock's jobject for a direct ByteBuffer
        _fields_ = [("addr", C.c_void_p), ("cap", C.c_int64)]
    thrown = []
    FIND = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_char_p)
    THROW = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_char_p)
    ADDR = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_void_p)
    CAP = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_void_p)
    cbs = [FIND(lambda e, n: 1), THROW(lambda e, c, m: thrown.append(m) or 0),
           ADDR(lambda e, b: Buf.from_address(b).addr if b else None), CAP(lambda e, b: Buf.from_address(b).cap if b else -1)]
    table = (C.c_void_p * 232)()
    for slot, f in zip((6, 14, 230, 231), cbs):
        table[slot] = C.cast(f, C.c_void_p)
    env = C.pointer(C.c_void_p(C.addressof(table)))

    def buf(a):
        return Buf(a.ctypes.data, a.nbytes)
    lib.Java_align2_BBMapHIP_create.restype = C.c_int64
    lib.Java_align2_BBMapHIP_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint8, C.c_int32, C.c_int32, C.c_int32]
    n = len(recs)
    ctx = lib.Java_align2_BBMapHIP_create(env, None, di.h.value if hasattr(di.h, "value") else di.h, PB | (2 << 8), 0, n, int(recs["len"].max()), 32)
    assert ctx and not thrown, thrown
    rc = np.ascontiguousarray(recs).view(np.uint8).copy()
    bl, bsc, kin = np.ascontiguousarray(blob, np.uint8), np.ascontiguousarray(bs, np.int8), np.ascontiguousarray(ki, np.int32)
    nsites, offs, sites = np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros(64 * n * 128, np.uint8)
    args = [buf(x) for x in (rc, bl, bsc, kin, nsites, offs, sites)]
    lib.Java_align2_BBMapHIP_mapBatch.restype = C.c_int64
    lib.Java_align2_BBMapHIP_mapBatch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32]
    total = lib.Java_align2_BBMapHIP_mapBatch(env, None, ctx, n, C.byref(args[0]), C.byref(args[1]), C.byref(args[2]), bl.size, C.byref(args[3]), kin.size,
                                              C.byref(args[4]), C.byref(args[5]), C.byref(args[6]), 64 * n)
    assert not thrown and total > 0, thrown
    fin = np.zeros(n * 64, np.uint8)
    mb = np.zeros(max(1, len(match_c)), np.uint8)
    fb, mbb = buf(fin), buf(mb)
    lib.Java_align2_BBMapHIP_getFinal.restype = C.c_int64
    lib.Java_align2_BBMapHIP_getFinal.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    got = lib.Java_align2_BBMapHIP_getFinal(env, None, ctx, n, C.byref(fb), C.byref(mbb), mb.size)
    lib.Java_align2_BBMapHIP_destroy.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.Java_align2_BBMapHIP_destroy(env, None, ctx)
    assert not thrown, thrown
    assert got == len(match_c) and fin.tobytes() == np.ascontiguousarray(fin_c).tobytes() and mb[:got].tobytes() == match_c[:got].tobytes()
