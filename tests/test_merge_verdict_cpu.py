"""BBMerge's verdict without a device: the host form bbmerge_verdict_batch against the statement-by-statement restatement
(tests/merge_verdict_check.py) on the pairs of tests/merge_verdict_problems.py, whole records including the filters' float bits; the
conditions those pairs must meet; the normal mode against the oracle's restatement of the native; the counters; the records'
layout; verdict_from_flags; every refusal; and the existing overlap search, unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bbmap_amd import _lib, build
from bbmap_amd import merge as M
from tests import merge_problems as P
from tests import merge_verdict_check as K
from tests import merge_verdict_problems as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


def turned(name, other):
    """pairs whose code under CONFIGS[name] differs from the one under CONFIGS[other]"""
    return V.expected_for(name)["code"] != V.expected_for(other)["code"]


# ------------------------------------------------------------------------------------------------ the inputs themselves
def test_problem_set_holds_every_class():
    """Conditions on the inputs, judged on the restatement's answers alone, so that no class can vanish silently."""
    d = V.expected_for("defaults")
    n = len(d)
    code = d["code"]
    shares = dict(merged=(code > 0).sum(), ambiguous=(code == K.RET_AMBIG).sum(), no_solution=(code == K.RET_NO_SOLUTION).sum(),
                  short=(code == K.RET_SHORT).sum())
    print(n, shares)
    assert n >= 3000 and all(v >= 0.02 * n for v in shares.values()), shares
    by_efilter = (code == K.RET_AMBIG) & turned("defaults", "efilter=f")
    by_pfilter = (code == K.RET_NO_SOLUTION) & ((d["info"] & M.INFO_PFILTER) != 0) & turned("defaults", "pfilter=f")
    # (a pair the ratio mode turned down has bad = minLength or 99999 and is ambiguous by the same rule; those are not meant)
    by_mismatches_r = (code == K.RET_AMBIG) & turned("defaults", "maxmismatchesr=1000000") & (d["insertRM"] > 0) & (d["ambigRM"] == 0)
    by_entropy = turned("defaults", "entropy=f")
    long_ = V.expected_for("maxlength=200")["code"] == K.RET_LONG
    u = V.expected_for("ustrict")
    by_rrm = (u["insertRM"] > 0) & (u["ambigRM"] == 0) & (u["insertNM"] != u["insertRM"]) & ((u["info"] & M.INFO_NORMAL) != 0)
    counts = dict(efilter=by_efilter.sum(), pfilter=by_pfilter.sum(), mismatches_r=by_mismatches_r.sum(), entropy=by_entropy.sum(), long=long_.sum(),
                  rrm=by_rrm.sum())
    print(counts)
    assert counts["efilter"] >= 20 and counts["pfilter"] >= 20 and counts["mismatches_r"] >= 20 and counts["entropy"] >= 50
    assert counts["long"] >= 20 and counts["rrm"] >= 20
    assert d["minOverlap"].min() == 11 and (d["minOverlap"] == np.array([max(len(p[0]), len(p[1])) for p in V.problem_set()[0]]) + 1).sum() >= 20
    # every stage's flag occurs, and both outcomes of each filter
    x = V.expected_for("xstrict")
    assert ((x["info"] & M.INFO_NORMAL) != 0).sum() >= 100 and (x["insertNM"] > 0).sum() >= 50 and (x["ambigNM"] == 1).sum() >= 1
    assert ((d["info"] & M.INFO_EFILTER) != 0).sum() > ((d["info"] & M.INFO_PFILTER) != 0).sum() > 100


def test_the_restatement_takes_the_inner_early_exit():
    """The library sums every column of every overlap; the restatement stops at `bad <= badlim` as the Java does.  The exit is
    taken on nearly every overlap of these pairs, so the equality below is a test of the exactness argument."""
    pairs = [p for p in V.problem_set()[0][:400] if len(p[0]) == len(p[1])]
    cfg = M.verdict_from_flags(ratiomode="f", normalmode="t", qualiters=1, entropy="f")
    columns = []
    recs = K.verdicts(pairs, cfg, columns=columns)
    assert len(columns) == len(pairs) and (recs["minOverlap"] == 11).all()
    full = 0                                                            # overlaps 8 .. alen + blen - max(11, 26) - 1, all their columns
    for a, b, _, _ in pairs:
        full += sum(min(o, 2 * len(a) - o) for o in range(8, 2 * len(a) - 26))
    print(sum(columns), full)
    assert sum(columns) < full / 3


# ------------------------------------------------------------------------------------------------ host form against the restatement
HOST_CONFIGS = ["defaults", "strict", "xstrict", "ustrict", "fast", "usequality=f", "no-quality-array", "entropy=f", "normal-mode-only",
                "normal-mode-only-no-quality", "quality-forms", "maxlength=200"]


@pytest.mark.parametrize("name", HOST_CONFIGS)
def test_host_verdict_equals_the_restatement(name):
    got = M.verdict_batch(*V.batch(name), cfg=V.config(name))
    exp = V.expected_for(name)
    diff = K.differing(got, exp)
    assert diff.size == 0, (diff[:5], got[diff[:5]], exp[diff[:5]])


def test_normal_mode_equals_the_oracles_native_where_every_probability_is_equal():
    """orc_bbmerge_mate_by_overlap restates jni/BBMergeOverlapper.c, which weighs a column by aprob[j] * bprob[j] where the Java has
    aprob[j] * bprob[i]; without qualities every probability is 0.98 and the two agree, so the native is a second witness -- where
    mate 1 is not the longer one: j runs over mate 1, and the native's bprob is filled for blen entries only."""
    from oracle.oracle import lib
    O = lib()
    i8, f32, i32 = C.POINTER(C.c_int8), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    O.orc_bbmerge_mate_by_overlap.argtypes = [i8, C.c_int, i8, C.c_int, i8, i8, f32, f32, i32] + [C.c_int] * 7
    O.orc_bbmerge_mate_by_overlap.restype = C.c_int32
    name = "normal-mode-only-no-quality"
    cfg = V.config(name)
    got = M.verdict_batch(*V.batch(name), cfg=cfg)
    pairs = [(i, p[0], p[1]) for i, p in enumerate(V.problem_set()[0]) if len(p[0]) <= len(p[1])]
    found = 0
    for i, a, b in pairs:
        aa, bb = np.frombuffer(a + b"\0", np.int8).copy(), np.frombuffer(b + b"\0", np.int8).copy()
        n = max(len(a), len(b)) + 1
        ap, bp, rv = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(5, np.int32)
        x = O.orc_bbmerge_mate_by_overlap(aa.ctypes.data_as(i8), len(a), bb.ctypes.data_as(i8), len(b), None, None, ap.ctypes.data_as(f32),
                                          bp.ctypes.data_as(f32), rv.ctypes.data_as(i32), cfg.minOverlapBases0, int(got["minOverlap"][i]),
                                          cfg.ratio.minInsert0, cfg.margin, cfg.maxMismatches0, cfg.maxMismatches, cfg.minQuality)
        exp = (x, int(rv[2]), int(rv[4])) if x > -1 else (-1, 999999, 0)               # BBMerge.java:1644-1645, :1655-1658, :1782
        assert (int(got["insertNM"][i]), int(got["badNM"][i]), int(got["ambigNM"][i])) == exp, i
        found += x > -1
    assert found >= 300 and len(pairs) >= 2000


# ------------------------------------------------------------------------------------------------ skipped pairs
def test_pairs_outside_the_limits_are_skipped_and_their_neighbours_are_not_disturbed():
    pairs = V.problem_set()[0][:5]
    s1, s2, q1, q2 = P.hand_over(pairs)
    q1 = [q.copy() for q in q1]
    long_ = b"ACGT" * 128 + b"A"                                        # 513 bases
    s1b, q1b = [s1[0], long_, s1[1], s1[2], s1[3], s1[4]], [q1[0], np.full(513, 30, np.uint8), q1[1], q1[2], q1[3], q1[4]]
    s2b, q2b = [s2[0], s2[0], s2[1], s2[2], s2[3], s2[4]], [q2[0], q2[0], q2[1], q2[2], q2[3], q2[4]]
    q1b[3][5] = 60                                                      # outside probCorrect2, inside probCorrect
    q1b[4][7] = 71                                                      # outside both
    batch = M.pack_pairs(s1b, s2b, q1b, q2b)
    skipped = np.zeros(1, M.VERDICT_DTYPE)
    skipped[0] = (-1, 0, -1, 0, 0, -1, 99999, 0, 0, 0.0, 0.0, M.INFO_SKIPPED)
    stats = M.new_stats()
    got = M.verdict_batch(*batch, stats=stats)
    exp = V.expected_for("defaults")
    assert K.differing(got[[0, 2, 5]], exp[[0, 1, 4]]).size == 0
    assert K.differing(got[[1, 3, 4]], np.repeat(skipped, 3)).size == 0
    assert stats["pairs"][0] == 6 and stats["skipped"][0] == 3 and stats["hist"].sum() == stats["merged"][0] == (got["code"] > 0).sum()
    # with the filters off 60 is read by nobody (the flat form runs alone) and neither is 71; with the normal mode on 71 is outside
    off = M.default_verdict_config(useEfilter=0, pfilterRatio=0.0)
    got = M.verdict_batch(*batch, cfg=off)
    assert (got["info"] & M.INFO_SKIPPED != 0).tolist() == [False, True, False, False, False, False]
    edited = [(a, b, qa.copy(), qb) for a, b, qa, qb in pairs]
    edited[2][2][5], edited[3][2][7] = 60, 71
    assert K.differing(got[[0, 2, 3, 4, 5]], K.verdicts(edited, off)).size == 0
    got = M.verdict_batch(*batch, cfg=M.default_verdict_config(useEfilter=0, pfilterRatio=0.0, useNormalMode=1))
    assert (got["info"] & M.INFO_SKIPPED != 0).tolist() == [False, True, False, False, True, False]
    # useQuality = 0: no quality is read at all
    got = M.verdict_batch(*batch, cfg=M.default_verdict_config(useQuality=0, useNormalMode=1))
    assert (got["info"] & M.INFO_SKIPPED != 0).tolist() == [False, True, False, False, False, False]
    assert K.differing(got[[0, 2, 3, 4, 5]], K.verdicts(edited, M.default_verdict_config(useQuality=0, useNormalMode=1))).size == 0


# ------------------------------------------------------------------------------------------------ counters
@pytest.mark.parametrize("name", ["defaults", "maxlength=200"])
def test_stats_equal_a_recount_and_a_second_call_adds(name):
    batch, cfg = V.batch(name), V.config(name)
    stats = M.new_stats()
    recs = M.verdict_batch(*batch, cfg=cfg, stats=stats)
    once = K.recount(recs)
    assert stats.tobytes() == once.tobytes()
    assert stats["pairs"][0] == sum(stats[k][0] for k in ("merged", "ambiguous", "tooShort", "tooLong", "noSolution", "skipped"))
    r1, r2, bases, quality = batch
    M.verdict_batch(r1[:700], r2[:700], bases, quality, cfg=cfg, stats=stats)
    both = K.recount(np.concatenate([recs, recs[:700]]))
    assert stats.tobytes() == both.tobytes()
    assert M.verdict_batch(r1[:0], r2[:0], bases, quality, cfg=cfg, stats=stats).size == 0 and stats.tobytes() == both.tobytes()


# ------------------------------------------------------------------------------------------------ layout
def test_struct_sizes_and_offsets(tmp_path):
    names = {"bbmerge_verdict_config": [f[0] for f in M.bbmerge_verdict_config._fields_], "bbmerge_verdict_rec": list(M.VERDICT_DTYPE.names),
             "bbmerge_stats": list(M.STATS_DTYPE.names)}
    src = ["#include <stddef.h>", "#include <stdio.h>", '#include "bbmap_amd.h"', "int main(void) {"]
    for s, fs in names.items():
        src.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        src += ['    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for f in fs]
    src += ['    printf("hist len %d\\n", BBMERGE_HIST_LEN);',
            '    printf("info bits %d\\n", BBMERGE_INFO_RATIO | BBMERGE_INFO_NORMAL << 8 | BBMERGE_INFO_EFILTER << 16 | BBMERGE_INFO_PFILTER << 24);',
            '    printf("ret codes %d\\n", -BBMERGE_RET_NO_SOLUTION | -BBMERGE_RET_AMBIG << 8 | -BBMERGE_RET_SHORT << 16 | -BBMERGE_RET_LONG << 24);',
            "    return 0;", "}", ""]
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe], check=True)
    got = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        s, f, v = line.split()
        got.setdefault(s, {})[f] = int(v)
    cfg = M.bbmerge_verdict_config
    assert got["bbmerge_verdict_config"] == dict({f[0]: getattr(cfg, f[0]).offset for f in cfg._fields_}, sizeof=C.sizeof(cfg))
    assert C.sizeof(cfg) == 136 and cfg.ratio.offset == 0 and cfg.useEntropy.offset == 48
    for s, dt in (("bbmerge_verdict_rec", M.VERDICT_DTYPE), ("bbmerge_stats", M.STATS_DTYPE)):
        assert got[s] == dict({k: dt.fields[k][1] for k in dt.names}, sizeof=dt.itemsize), s
    assert M.VERDICT_DTYPE.itemsize == 48 and M.STATS_DTYPE.itemsize == 16080
    assert got["hist"]["len"] == M.HIST_LEN
    assert got["info"]["bits"] == M.INFO_RATIO | M.INFO_NORMAL << 8 | M.INFO_EFILTER << 16 | M.INFO_PFILTER << 24
    assert got["ret"]["codes"] == -M.RET_NO_SOLUTION | -M.RET_AMBIG << 8 | -M.RET_SHORT << 16 | -M.RET_LONG << 24
    assert _lib.load().bbmap_abi_version() == 6                         # symbols were added, nothing changed


# ------------------------------------------------------------------------------------------------ flags
def verdict_fields(cfg):
    own = tuple(getattr(cfg, f[0]) for f in M.bbmerge_verdict_config._fields_[1:-1])
    return tuple(getattr(cfg.ratio, n) for n, _ in M.bbmerge_config._fields_), own


def f32(x):
    return float(np.float32(x))


def test_default_verdict_config():
    ratio, own = verdict_fields(M.default_verdict_config())
    assert ratio == (5, 8, 26, 35, f32(0.09), 5.5, f32(0.55), f32(0.95), f32(0.95), 0, 1, 41)
    #             entropy     overlaps    modes    R   margin mm mm0 minq iters uq ef  efilter  offset      pfilter      maxLength
    assert own == (1, 3, 39, 11, 8, 3, 1, 0, 0, 20, 2, 3, 3, 10, 3, 1, 1, 6.0, f32(0.05), f32(0.00004), 0)
    assert verdict_fields(M.verdict_from_flags()) == (ratio, own)
    L = _lib.load()
    assert L.bbmerge_default_verdict_config(None) == -2 and L.bbmap_last_error() == b"bbmerge_default_verdict_config: null argument"
    with pytest.raises(AttributeError):
        M.default_verdict_config(nosuchfield=1)


# preset -> (minOverlapBases0, minOverlapBases, reduction, minEntropy, normal, rrm, maxRatio, ratioMargin, ratioOffset, efilter, pfilter,
#            minInsert0): BBMerge.java:122-193, :258-267 by hand; every strict preset adds maxbad=4 margin=3 minqo=8 qualiters=2
PRESET_NUMBERS = {
    "strict": (7, 11, 4, 42, 0, 0, 0.075, 7.5, 0.55, 4, 0.0008, 26),
    "vstrict": (4, 12, 4, 52, 0, 0, 0.05, 12, 0.5, 2, 0.008, 26),
    "ustrict": (3, 14, 4, 56, 1, 1, 0.045, 12, 0.5, 2, 0.03, 26),
    "xstrict": (3, 14, 4, 56, 1, 1, 0.055, 12, 0.65, 2, 0.25, 26),
    "fast": (8, 11, 3, 39, 0, 0, 0.08, 2.5, 0.55, 8, 0.0002, 35),
}


@pytest.mark.parametrize("preset", sorted(PRESET_NUMBERS))
def test_verdict_from_flags_per_preset(preset):
    """minInsert0: mininsert0 is not given by a strict preset, so min(35, max((int)(35 * 0.75), 5, MIN_OVERLAPPING_BASES_0)) = 26 for
    every minoverlap0 <= 26; fast gives mininsert0=50 and min(minInsert, 50) = 35 remains (:605-611)."""
    mo0, mo, red, ent, normal, rrm, maxr, rmargin, roff, ef, pf, mi0 = PRESET_NUMBERS[preset]
    cfg = M.verdict_from_flags(preset)
    strict = preset != "fast"
    ratio, own = verdict_fields(cfg)
    assert ratio == (mo0 - red, mo - red, mi0, 35, f32(maxr), f32(rmargin), f32(roff), f32(0.95), f32(0.95), 0, 1, 41)
    mm, margin, minq, iters = (4, 3, 8, 2) if strict else (3, 2, 10, 3)
    assert own == (1, 3, ent, mo, mo0, red, 1, normal, rrm, 20, margin, mm, mm, minq, iters, 1, 1, f32(ef), f32(0.05), f32(pf), 0)
    # an explicit flag comes after the preset's and overrides it
    over = M.verdict_from_flags(preset, efilter="7", minentropy=33, maxratio="0.06", mismatches=5)
    assert (f32(over.efilterRatio), over.minEntropyScore, f32(over.ratio.maxRatio), over.maxMismatches, over.maxMismatches0) == (7.0, 33, f32(0.06), 5, 5)


def test_verdict_from_flags_parse_rules():
    v = M.verdict_from_flags
    assert (v(entropy="f").useEntropy, v(entropy="f").minEntropyScore) == (0, 39) and (v(minentropy=50).useEntropy, v(minentropy="50").minEntropyScore) == (1, 50)
    assert (v(efilter="f").useEfilter, v(efilter="f").efilterRatio) == (0, -1.0) and (v(efilter="t").useEfilter, v(efilter="t").efilterRatio) == (1, 6.0)
    assert (v(efilter="3.5").useEfilter, v(efilter=3.5).efilterRatio) == (1, 3.5) and v(efilter="-1").useEfilter == 0
    assert v(pfilter="f").pfilterRatio == 0.0 and v(pfilter="t").pfilterRatio == f32(0.00004) and v(pfilter="0.01").pfilterRatio == f32(0.01)
    assert v(efilteroffset="0.5").efilterOffset == 0.5
    assert v(usequality="f").useQuality == 0 and v(ignorequality="t").useQuality == 0 and v(usequality="f").ratio.useQuality == 0
    assert v(ouq="t").ratio.useQuality == 1 and v(owq="f").ratio.withoutQuality == 0
    assert (v(normalmode="t").useNormalMode, v(ratiomode="f").useRatioMode, v(ratiomode="f").useNormalMode) == (1, 0, 1)     # :613-616
    assert v(rrm="t").requireRatioMatch == 1 and v(requireratiomatch=True).requireRatioMatch == 1
    assert (v(margin=1).margin, v(margin=5).margin) == (1, 3)                                                                   # :662-664
    assert (v(mismatches=6).maxMismatches0, v(mismatches=6, mismatches0=4).maxMismatches0, v(mismatches=2, mismatches0=4).maxMismatches0) == (6, 6, 4)
    assert (v(minq=12).minQuality, v(minqo=300).minQuality, v(qualiters=0).qualIters, v(qualiters=5).qualIters) == (12, 44, 1, 5)
    assert (v(maxlength=300).maxLength, v().maxLength) == (300, 0)
    c = v(minoverlap=30, mininsert=12, minoverlap0=9, ratiominoverlapreduction=2)
    assert (c.minOverlapBases, c.minOverlapBases0, c.ratioReduction, c.ratio.minInsert, c.ratio.minInsert0) == (30, 9, 2, 30, 22)
    assert verdict_fields(v(minsecondratio="0.3")) == verdict_fields(v())          # accepted and ignored
    for loose in ("loose", "vloose", "uloose", "xloose"):
        with pytest.raises(ValueError, match="loose.*mateByOverlap_normalMode.*calcMinOverlapFromEntropy"):
            v(loose)
        with pytest.raises(ValueError, match="loose"):
            v(**{loose: "t"})
    for loose in ("veryloose", "ultraloose", "hloose", "hyperloose", "maxloose"):                          # BBMerge.java:95-103
        with pytest.raises(ValueError, match="loose"):
            v(**{loose: "t"})
    assert verdict_fields(v(loose="f", vloose="f", ultraloose=False)) == verdict_fields(v())          # switched off: nothing changes
    assert verdict_fields(v("verystrict")) == verdict_fields(v("vstrict")) and verdict_fields(v("ultrastrict")) == verdict_fields(v("ustrict"))
    with pytest.raises(ValueError):
        v(minentropy="-5")              # no digit in front: read as a boolean, as Java's isDigit rule does
    with pytest.raises(ValueError):
        v(nosuchflag=1)
    with pytest.raises(ValueError):
        v("nosuchpreset")


# ------------------------------------------------------------------------------------------------ refusals
VP = C.c_void_p
VERDICTS = ("bbmerge_verdict_batch", "bbmerge_verdict_batch_device")
BAD_RATIO = b": bad config (no NaN, ratioMargin >= 1, gIncr and bIncr >= 0, minInsert0 and minInsert >= 0, maxMergeQuality 0..127)"
BAD_VERDICT = b": bad config (entropyK 1..5, qualIters >= 1, 0 <= maxMismatches0 >= maxMismatches >= margin, a mode on, no NaN)"


def _call(name, cfg, n, nulls=()):
    """the entry point with every buffer a valid host address except those named in `nulls`: each refusal comes before the first HIP
    call and before any buffer is read, so the device form can be asked without a device"""
    L = _lib.load()
    buf = np.zeros(64, np.uint8)
    names = ["reads1", "reads2", "bases", "quality", "recs", "stats"]
    args = [None if cfg is None else C.byref(cfg)] + ([None] if name.endswith("_device") else []) + [n] + \
        [None if k in nulls else buf.ctypes.data for k in names]
    rc = getattr(L, name)(*args)
    return rc, L.bbmap_last_error()


@pytest.mark.parametrize("name", VERDICTS)
def test_rejected_arguments(name):
    who = name.encode()
    good = M.default_verdict_config()
    assert _call(name, None, 1) == (-2, who + b": null config")
    assert _call(name, good, -1) == (-2, who + b": bad pair count")
    for bad in (dict(maxRatio=float("nan")), dict(ratioOffset=float("nan")), dict(gIncr=float("nan")), dict(ratioMargin=0.99), dict(gIncr=-0.5),
                dict(bIncr=-1.0), dict(minInsert=-1), dict(minInsert0=-1), dict(maxMergeQuality=128), dict(maxMergeQuality=-1)):
        assert _call(name, M.default_verdict_config(**bad), 1) == (-2, who + BAD_RATIO), bad
    for bad in (dict(entropyK=0), dict(entropyK=6), dict(qualIters=0), dict(maxMismatches0=-1, maxMismatches=-2, margin=-3),
                dict(maxMismatches0=2, maxMismatches=3), dict(margin=4), dict(useRatioMode=0, useNormalMode=0), dict(efilterRatio=float("nan")),
                dict(efilterOffset=float("nan")), dict(pfilterRatio=float("nan"))):
        assert _call(name, M.default_verdict_config(**bad), 1) == (-2, who + BAD_VERDICT), bad
    for k in ("reads1", "reads2", "bases", "recs"):
        assert _call(name, good, 1, nulls={k}) == (-2, who + b": null buffer"), k
    assert _call(name, good, 0, nulls={"reads1", "reads2", "bases", "quality", "recs", "stats"})[0] == 0
    for ok in (dict(entropyK=1), dict(entropyK=5), dict(margin=3), dict(margin=-2), dict(maxMismatches0=0, maxMismatches=0, margin=0)):
        assert _call(name, M.default_verdict_config(**ok), 0)[0] == 0, ok


def test_entropy_k_from_one_to_five_and_other_scores():
    pairs = V.problem_set()[0][:400]
    batch = M.pack_pairs(*P.hand_over(pairs))
    for k, score in ((1, 10), (2, 39), (4, 60), (5, 200)):
        cfg = M.default_verdict_config(entropyK=k, minEntropyScore=score)
        assert K.differing(M.verdict_batch(*batch, cfg=cfg), K.verdicts(pairs, cfg)).size == 0, k


# ------------------------------------------------------------------------------------------------ the existing search, unchanged
@pytest.mark.parametrize("name", sorted(P.CONFIGS))
def test_the_overlap_search_still_equals_the_oracle(name):
    pairs, (r1, r2, bases, quality) = P.problem_set()
    got = M.overlap_batch(r1, r2, bases, quality, P.config(P.CONFIGS[name]))
    exp = P.expected_for(name)
    diff = np.flatnonzero(got != exp)
    assert diff.size == 0, (diff[:5], got[diff[:5]], exp[diff[:5]])
