"""Quality trimming on the device: bbtrim_batch_device against the host form, Mapper.from_reads(trim=...) against a run over the same
reads trimmed on the host and packed back to back, and Mapper.untrim() (bbmap_untrim_batch_device) against the restatement of
TrimRead.untrim (tests/trim_check.py), followed by the SAM records, read histograms and coverage of the untrimmed batch against their
own checkers.  Everything is compared exactly.

Two runs of the mapper agree in everything but where a string lies in its pool and which fill-log entry a site refers to: both follow
the order in which the batch's wavefronts took their slots (tests/test_runstats_gpu.py::_lists_equal leaves them out for the same
reason), so match_off, reserved[0] and match_job are not compared; the strings themselves are, byte for byte."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest
import torch

from bbmap_amd import _lib
from bbmap_amd import reference as R
from bbmap_amd import trim as T
from bbmap_amd.index import DeviceIndex, READ_DTYPE
from bbmap_amd.mapper import FINAL_DTYPE, MSITE_DTYPE, Mapper, _copy, bbmap_overflow_output
from tests import trim_check as TC
from tests.test_trim_cpu import INT, OPT, WIN, SIDES, case_reads, cfg, lowered_phix, pack

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAGS = dict(qtrim="rl", trimq=10, minlength=30)
FIN_NAMES = [k for k in FINAL_DTYPE.names if k not in ("match_off", "reserved")]
SITE_NAMES = [k for k in MSITE_DTYPE.names if k not in ("match_job", "reserved")]
TIER = dict(max_sites=1, reserved=(C.c_int32 * 4)(0, 4096, 256, 0))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


# ------------------------------------------------------------------------------------------------ device against host
def _mixed(n, seed):
    """n reads of mixed lengths in one batch (their offsets fall on every alignment), drawn from the CPU test's case set"""
    cases = case_reads()
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(cases), n)
    # read 0 has something to trim in every mode, with its qualities (low at both ends) and without them (N at both ends), so that
    # no batch, the one of a single read included, passes on reads that are all left alone
    out = [(b"NN" + b"ACGT" * 10 + b"NAN", bytes([2, 2] + [30] * 40 + [2, 2, 2]))]
    for i in pick[1:]:
        b, q = cases[int(i)]
        cut = int(rng.integers(0, 8)) if len(b) > 8 else 0
        out.append((b[cut:], q[cut:]))
    return [x[0] for x in out], [x[1] for x in out]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 1000])
@pytest.mark.parametrize("with_quality", [True, False])
def test_device_equals_host(n, with_quality):
    reads, quals = _mixed(n, n)
    recs, blob, qblob = pack(reads, quals if with_quality else None)
    assert n < 8 or len({int(o) & 7 for o in recs["bases_off"]}) == 8
    d_recs, d_blob, d_q = _dev(recs), _dev(blob), (_dev(qblob) if with_quality else None)
    configs = [cfg(m, l, r, tq, ml) for m, (l, r), tq, ml in itertools.product((OPT, WIN, INT), SIDES[1:], (0, 1, 10, 41), (0, 60))]
    configs += [cfg(OPT, optimalBias=0.05), cfg(WIN, windowLength=7), cfg(WIN, windowLength=1), cfg(INT, minGoodInterval=3)]
    trimmed = 0
    for c in configs:
        want_recs, want_trims = T.trim_batch(recs, blob, qblob if with_quality else None, c)
        got_recs, got_trims = T.trim_batch_device(d_recs, d_blob, d_q, c)
        got_recs, got_trims = got_recs.cpu().numpy().view(READ_DTYPE), got_trims.cpu().numpy().view(T.TRIM_DTYPE)
        assert got_trims.tobytes() == want_trims.tobytes(), (c.mode, c.trimLeft, c.trimRight, c.trimq, c.minLength,
                                                             np.flatnonzero((got_trims != want_trims))[:5])
        assert got_recs.tobytes() == want_recs.tobytes()
        trimmed += int(np.count_nonzero(want_trims["left"] + want_trims["right"]))
    assert trimmed > 0
    assert d_recs.cpu().numpy().tobytes() == recs.tobytes()                 # the input records are not written


def test_device_on_nothing():
    recs, trims = T.trim_batch_device(torch.zeros(0, dtype=torch.uint8, device=DEV), torch.zeros(0, dtype=torch.uint8, device=DEV), None, cfg())
    assert recs.numel() == 0 and trims.numel() == 0
    d = _dev(np.zeros(1, READ_DTYPE))
    L = _lib.load()
    assert L.bbtrim_batch_device(C.byref(cfg()), None, 1, d.data_ptr(), d.data_ptr(), None, d.data_ptr(), d.data_ptr()) == -2
    assert L.bbmap_last_error() == b"bbtrim_batch_device: reads_out must not alias reads_in"


# ------------------------------------------------------------------------------------------------ through the mapper
def _packed():
    from tests.golden_phix import phix_reference
    ref = phix_reference()
    return ref, R.Packed([ref], [np.array([8000], np.int32)], [np.array([len(ref) - 16000], np.int32)], [["phix174"]], 300)


def _mapper(reads, quals, paired, trim=None, **kw):
    ref, packed = _packed()
    di = DeviceIndex.build([ref], k=13)
    di.set_scaffolds(packed)
    kw.setdefault("max_sites", 32)
    mp = Mapper.from_reads(di, [len(r) for r in reads], np.concatenate(reads), None if quals is None else np.concatenate(quals),
                           paired=paired, trim=trim, **kw)
    return di, mp, packed


def _grab(mp, o, n):
    """one bbmap_output as it is on the device: records, their strings, site lists, the sites' own strings"""
    cap = o.cap
    fin = _copy(o.final, n * FINAL_DTYPE.itemsize).view(FINAL_DTYPE)
    pool = _copy(o.final_match, int(o.final_match_bytes))
    sites = _copy(o.sites, n * cap * 128).view(MSITE_DTYPE).reshape(n, cap)
    nsites = _copy(o.nsites, n * 4).view(np.int32)

    def string(off, ln):
        assert 0 <= off and off + ln <= len(pool), (off, ln, len(pool))
        return pool[off: off + ln].tobytes()
    matches = [string(int(f["match_off"]), int(f["match_len"])) if int(f["match_len"]) > 0 else None for f in fin]
    smatches = [[string(4 * (int(s["reserved"][0]) - 1), int(s["reserved"][1]) & 0x7fffffff) if int(s["reserved"][0]) > 0 else None
                 for s in sites[r][:max(0, int(nsites[r]))]] for r in range(n)]
    return dict(fin=fin, matches=matches, sites=sites, nsites=nsites, smatches=smatches, pool_bytes=len(pool))


def _state(mp):
    """(main output, overflow tier's output or None, the tier's read numbers)"""
    main = _grab(mp, mp.output_pointers(), mp.n)
    ov = bbmap_overflow_output()
    assert mp.L.bbmap_get_overflow_output(mp.h, C.byref(ov)) == 0
    if ov.n_reads == 0:
        return main, None, None
    return main, _grab(mp, ov.out, int(ov.n_reads)), _copy(ov.read_ids, int(ov.n_reads) * 4).view(np.int32)


def _same(a, b, what):
    """two outputs field by field (see the module's docstring for what is left out)"""
    for k in FIN_NAMES:
        bad = np.flatnonzero(a["fin"][k] != b["fin"][k])
        assert not len(bad), (what, k, bad[:5], a["fin"][bad[:3]], b["fin"][bad[:3]])
    assert a["matches"] == b["matches"], (what, [i for i in range(len(a["matches"])) if a["matches"][i] != b["matches"][i]][:5])
    assert np.array_equal(a["nsites"], b["nsites"]), what
    for r, n in enumerate(a["nsites"]):
        n = max(0, int(n))
        for k in SITE_NAMES:
            assert np.array_equal(a["sites"][r][:n][k], b["sites"][r][:n][k]), (what, r, k, a["sites"][r][:n][k], b["sites"][r][:n][k])
        assert [int(x) & 0x7fffffff if m is not None else 0 for x, m in zip(a["sites"][r][:n]["reserved"][:, 1], a["smatches"][r])] == \
               [len(m) if m is not None else 0 for m in b["smatches"][r]], (what, r)
        assert a["smatches"][r] == b["smatches"][r], (what, r)


def _host_trimmed(reads, quals):
    recs, blob, qblob = pack([bytes(r) for r in reads], [bytes(q) for q in quals])
    _, trims = T.trim_batch(recs, blob, qblob, T.from_flags(**FLAGS))
    tr = [r[int(t["left"]): len(r) - int(t["right"])] for r, t in zip(reads, trims)]
    tq = [q[int(t["left"]): len(q) - int(t["right"])] for q, t in zip(quals, trims)]
    return tr, tq, trims


@pytest.mark.parametrize("mode", ["pe", "se1"])
def test_trimmed_records_are_mapped_as_trimmed_reads(mode):
    reads, quals, paired = lowered_phix(mode)
    tr, tq, trims = _host_trimmed(reads, quals)
    assert int(np.count_nonzero(trims["left"])) > 30 and int(np.count_nonzero(trims["right"])) > 30
    if paired:
        assert sum(1 for p in range(0, len(tr), 2) if len(tr[p]) != len(tr[p + 1])) > 30
    di, mp, _ = _mapper(reads, quals, paired, trim=T.from_flags(**FLAGS))
    di2, mp2, _ = _mapper(tr, tq, paired)
    try:
        assert mp.trims.cpu().numpy().view(T.TRIM_DTYPE).tobytes() == trims.tobytes()
        assert mp.reads_untrimmed is not None and not mp.untrim_wanted
        mp.step()
        mp2.step()
        a, ta, _ = _state(mp)
        b, tb, _ = _state(mp2)
        assert ta is None and tb is None
        _same(a, b, mode)
        # Not an empty comparison: 97 of 100 reads are PhiX reads of at least 30 bases after trimming (three have random bases), so
        # most of them map unless the moved records were addressed wrongly.  The exact count is the host-trimmed run's, above.
        assert int(np.count_nonzero(a["fin"]["mapped"])) > len(reads) // 2 and sum(m is not None for m in a["matches"]) > len(reads) // 2
        # run statistics are taken before untrim (calcStatistics runs inside processRead): those of the host-trimmed run
        mp.add_run_stats()
        mp2.add_run_stats()
        (rs, hist), (rs2, hist2) = mp.run_stats(), mp2.run_stats()
        assert rs.tobytes() == rs2.tobytes() and np.array_equal(hist, hist2) and int(rs["mappedRetained1"]) > 0
    finally:
        mp.close(); mp2.close(); di.close(); di2.close()


def _check_untrim(before, after, trims, ids, counts):
    fin, matches, sites, smatches = TC.untrim(before["fin"], before["matches"], before["sites"], before["nsites"], before["smatches"], trims, ids)
    _same(after, dict(fin=fin, matches=matches, sites=sites, nsites=before["nsites"], smatches=smatches), "untrim")
    # the new pool holds every string once, in 4-byte units
    units = sum((len(m) + 3) // 4 for m in after["matches"] if m is not None) + sum((len(m) + 3) // 4 for row in after["smatches"] for m in row if m is not None)
    assert after["pool_bytes"] == 4 * units
    for i, f in enumerate(before["fin"]):
        left, right = (int(x) for x in trims[i if ids is None else int(ids[i])])
        g = after["fin"][i]
        if left + right == 0:
            assert g.tobytes()[:48] == f.tobytes()[:48]                      # untouched but for where its string lies
            counts["mapped_untrimmed"] += int(f["mapped"]) != 0
            continue
        if not int(f["mapped"]):
            counts["unmapped"] += 1
            assert int(g["start"]) == int(g["stop"]) == -1
            continue
        counts["plus" if int(f["strand"]) == 0 else "minus"] += 1
        counts["minus_left_only"] += int(f["strand"]) == 1 and left > 0 and right == 0
        lt, rt = (left, right) if int(f["strand"]) == 0 else (right, left)
        assert int(g["start"]) == int(f["start"]) - lt and int(g["stop"]) == int(f["stop"]) + rt and int(g["perfect"]) == 0
        if after["matches"][i] is not None:
            m = after["matches"][i]
            assert m.startswith(b"C" * lt) and m.endswith(b"C" * rt) and len(m) == len(before["matches"][i]) + lt + rt
            counts["strings"] += 1
        counts["site_strings"] += sum(m is not None for m in after["smatches"][i])
        counts["sites"] += max(0, int(before["nsites"][i]))


def _counts():
    return dict.fromkeys(["plus", "minus", "unmapped", "mapped_untrimmed", "minus_left_only", "strings", "site_strings", "sites"], 0)


@pytest.mark.parametrize("mode", ["pe", "se1"])
def test_untrim_then_sam_histograms_and_coverage(mode):
    from bbmap_amd import coverage as V
    from tests import coverage_check as CK
    from tests import readstats_check as RK
    from tests import scaffold_check as SC
    from tests.test_coverage_gpu import _compare as cov_compare, _refcounts
    from tests.test_readstats_gpu import _compare as hist_compare
    from tests.test_sam_gpu import check_run
    reads, quals, paired = lowered_phix(mode)
    di, mp, packed = _mapper(reads, quals, paired, trim=T.from_flags(**FLAGS), untrim=True)
    try:
        assert mp.untrim_wanted
        mp.enable_read_hist()
        mp.enable_coverage(0)
        mp.step()
        trims = mp.trims.cpu().numpy().view(T.TRIM_DTYPE)
        before, tier, _ = _state(mp)
        assert tier is None
        pos_before = mp.sam_records(0)[0]["pos"].copy()
        mp.untrim()
        after, _, _ = _state(mp)
        counts = _counts()
        _check_untrim(before, after, trims, None, counts)
        assert counts["plus"] > 10 and counts["minus"] > 10 and counts["unmapped"] >= 2 and counts["mapped_untrimmed"] >= 5, counts
        assert counts["minus_left_only"] >= 1 and counts["strings"] > 50 and counts["sites"] > 50, counts
        # ---- SAM records of the untrimmed batch: the checker over the untrimmed records and the full reads
        got = check_run(mp, packed, reads, paired)
        recs, text, _ = got[0]
        assert np.array_equal(recs["pos"], pos_before)                       # POS does not move
        clipped = 0
        for r, (f, t) in enumerate(zip(after["fin"], trims)):
            if not int(f["mapped"]) or int(t["left"]) + int(t["right"]) == 0 or int(recs[r]["cigar_len"]) == 0:
                continue
            cigar = text[int(recs[r]["cigar_off"]): int(recs[r]["cigar_off"]) + int(recs[r]["cigar_len"])].tobytes().decode()
            lt, rt = (int(t["left"]), int(t["right"])) if int(f["strand"]) == 0 else (int(t["right"]), int(t["left"]))
            lead, trail = re.match(r"^(\d+)S", cigar), re.search(r"(\d+)S$", cigar)
            assert (lt == 0 or (lead and int(lead.group(1)) >= lt)) and (rt == 0 or (trail and int(trail.group(1)) >= rt)), (r, cigar, lt, rt)
            clipped += 1
        assert clipped > 50
        # ---- read histograms and coverage of the untrimmed batch: their checkers over the same inputs
        fin, blob = mp.final()
        matches = [blob[int(f["match_off"]): int(f["match_off"]) + int(f["match_len"])].tobytes() if int(f["match_len"]) > 0 else None for f in fin]
        assert matches == after["matches"]
        mp.add_read_hist()
        rs = RK.ReadStats()
        rs.add_batch([bytes(r) for r in reads], [bytes(q) for q in quals], fin, matches, paired)
        hist_compare(mp.read_hist(), rs)
        assert int(mp.read_hist().length[100]) == len(reads) and rs.match[5].any()      # full lengths; clipSum moved
        mp.add_coverage()
        p = CK.Pileup(SC.table_of(packed), 0, packed.scaffold_names(), _refcounts(packed))
        p.add_batch(fin, matches, [bytes(r) for r in reads], paired)
        cov_compare(mp.coverage(1000), p, 1000)
        # ---- refusals
        assert mp.L.bbmap_add_run_stats(mp.h, None, None) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_add_run_stats: the last batch has been untrimmed already (call it before bbmap_untrim_batch_device)"
        assert mp.L.bbmap_untrim_batch_device(mp.h, None, mp.reads_untrimmed.data_ptr(), mp.trims.data_ptr()) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_untrim_batch_device: the last batch has been untrimmed already"
        # the next step is a new batch: trimmed again, untrimmed again, the same result
        mp.step()
        mp.add_run_stats()
        mp.untrim()
        again, _, _ = _state(mp)
        _same(again, after, "second step")
    finally:
        mp.close(); di.close()


def test_untrim_overflow_tier():
    reads, quals, paired = lowered_phix("pe")
    di, mp, _ = _mapper(reads, quals, paired, trim=T.from_flags(**FLAGS), **TIER)
    try:
        mp.step()
        assert mp.stats()["reads_reprobed"] > 0
        trims = mp.trims.cpu().numpy().view(T.TRIM_DTYPE)
        before, tbefore, ids = _state(mp)
        assert tbefore is not None and len(ids) > 20
        mp.untrim()
        after, tafter, ids2 = _state(mp)
        assert np.array_equal(ids, ids2)
        _check_untrim(before, after, trims, None, _counts())
        counts = _counts()
        _check_untrim(tbefore, tafter, trims, ids, counts)
        assert counts["plus"] > 5 and counts["minus"] > 5 and counts["strings"] > 20 and counts["site_strings"] > 0 and counts["sites"] > 40, counts
        # bbmap_get_final puts the tier's untrimmed record in place of a main record that says so itself (its own nsites; the main
        # final stage runs before the tier's reads are marked in the main list, tests/test_readstats_gpu.py has the details)
        fin, blob = mp.final()
        for i, r in enumerate(ids):
            if int(after["fin"]["nsites"][int(r)]) == -3:
                f = fin[int(r)]
                assert all(f[k] == tafter["fin"][i][k] for k in FIN_NAMES)
                if int(f["match_len"]) > 0:
                    assert blob[int(f["match_off"]): int(f["match_off"]) + int(f["match_len"])].tobytes() == tafter["matches"][i]
    finally:
        mp.close(); di.close()


def test_refusals_and_zero_length():
    reads, quals, paired = lowered_phix("se1")
    di, mp, _ = _mapper(reads, quals, paired, trim=T.from_flags(**FLAGS), finalStage=0)
    try:
        assert mp.L.bbmap_untrim_batch_device(mp.h, None, mp.reads_untrimmed.data_ptr(), mp.trims.data_ptr()) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_untrim_batch_device: the context runs without the final stage (bbmap_config.finalStage)"
        mp.step()
        with pytest.raises(Exception, match="without the final stage"):
            mp.untrim()
    finally:
        mp.close(); di.close()
    di, mp, _ = _mapper(reads, quals, paired, trim=T.from_flags(**FLAGS))
    try:
        assert mp.L.bbmap_untrim_batch_device(mp.h, None, mp.reads_untrimmed.data_ptr(), mp.trims.data_ptr()) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_untrim_batch_device: no batch has been mapped yet"
    finally:
        mp.close(); di.close()
    di, mp, _ = _mapper(reads, quals, paired)
    try:
        with pytest.raises(ValueError, match="from_reads"):
            mp.untrim()
    finally:
        mp.close(); di.close()
    # minLength 0 lets the optimal mode trim a read away: the stage computes it, the mapper refuses the batch
    bad = [np.full(len(q), 2, np.uint8) if i == 4 else q for i, q in enumerate(quals)]
    ref, _ = _packed()
    di = DeviceIndex.build([ref], k=13)
    try:
        with pytest.raises(ValueError, match="without bases"):
            Mapper.from_reads(di, [len(r) for r in reads], np.concatenate(reads), np.concatenate(bad), trim=T.from_flags(qtrim="rl", trimq=10, minlength=0))
    finally:
        di.close()


def test_without_trim_nothing_changes():
    """a from_reads without trim, a second one, and one whose trim stage has both sides off (every trim 0, 0): the same records"""
    reads, quals, paired = lowered_phix("pe")
    runs = [_mapper(reads, quals, paired), _mapper(reads, quals, paired), _mapper(reads, quals, paired, trim=T.default_config())]
    try:
        states = []
        for _, mp, _ in runs:
            mp.step()
            states.append(_state(mp)[0])
        assert runs[0][1].trims is None and runs[0][1].reads_untrimmed is None
        assert not runs[2][1].trims.cpu().numpy().any()
        assert torch.equal(runs[2][1].reads.view(torch.int32).view(-1, 6)[:, [0, 1, 4]], runs[2][1].reads_untrimmed.view(torch.int32).view(-1, 6)[:, [0, 1, 4]])
        assert int(np.count_nonzero(states[0]["fin"]["mapped"])) > 0.9 * len(reads)
        _same(states[0], states[1], "untrimmed twice")
        _same(states[0], states[2], "trim stage with both sides off")
        # an untrim with nothing to take back moves the strings and changes nothing else
        runs[2][1].untrim()
        _same(_state(runs[2][1])[0], states[0], "untrim of nothing")
    finally:
        for di, mp, _ in runs:
            mp.close(); di.close()
