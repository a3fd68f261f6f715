"""Inputs and the case table for the tests of the mapper under non-default settings (BBMap profile): the bbmap_config fields that
mirror BBMap's command-line flags (minratio= / minid=, padding=, pairlen=, rescuedist=, rescuemismatches=, maxsites2=, rescue=,
pambig=, tipsearch=, trimlist=; AbstractMapper.java:253-487), which every other mapper test leaves at the profile's default.

A case names a workload, a settings dict and the effects the setting must have on that workload.  tests/test_oracle_config.py
asserts the effects on the CPU oracle alone (so that no case can pass on the GPU without the setting having done anything);
tests/test_mapper_config_gpu.py runs the device and the oracle with the same dict and compares everything.  The dict goes to
bbmap_config and to the oracle's MapParams through device_settings / oracle_params, which refuse a key either side lacks: ctypes
would otherwise take a misspelt key as a new Python attribute and the run would silently be one at the defaults.

Every read is L = 150 bases with the keys of make_offsets(150, 12, 1.9); the workloads are 400-600 pairs or reads on references of
200-300 kb and built once per process."""
import collections

import numpy as np

from bbmap_amd import workload as W

L, K = 150, 12
PAD = 2000
BASES = W.BASES

# bbmap_config fields the oracle has no counterpart of (they shape buffers and launches, not results), and Mapper arguments
DEVICE_ONLY = ("fastCols", "jobsPerRead", "reserved", "max_sites")


def oracle_params(settings):
    """MapParams at the BBMap profile's defaults with `settings` applied: every key that is not device-only must be a MapParams
    field."""
    from oracle import oracle as O
    fields = {n for n, _ in O.MapParams._fields_}
    kw = {k_: v for k_, v in settings.items() if k_ not in DEVICE_ONLY}
    unknown = sorted(set(kw) - fields)
    if unknown:
        raise KeyError("not a field of the oracle's MapParams: %s" % ", ".join(unknown))
    return O.map_default_params(**kw)


def device_settings(settings):
    """The settings as Mapper(...) keywords: every key must be a bbmap_config field (max_sites is Mapper's own argument)."""
    from bbmap_amd.mapper import bbmap_config
    fields = {n for n, _ in bbmap_config._fields_}
    unknown = sorted(set(settings) - fields)
    if unknown:
        raise KeyError("not a field of bbmap_config: %s" % ", ".join(unknown))
    return dict(settings)


# ------------------------------------------------------------------------------------------------------------------ workloads
def _subst(rng, row, cols):
    old = row[cols]
    row[cols] = BASES[(np.searchsorted(BASES, old) + rng.integers(1, 4, size=len(cols))) % 4]


def _tip_indel_rows(ref, starts, rng):
    """One plus-strand read per start with a 5-13 base deletion or insertion 3-11 bases from a tip; read i is of kind i % 4:
    deletion at the left tip, deletion at the right tip, insertion at the left tip, insertion at the right tip."""
    rows = np.empty((len(starts), L), np.uint8)
    for i, s in enumerate(starts):
        s, d, t = int(s), int(rng.integers(5, 14)), int(rng.integers(3, 12))
        kind = i % 4
        if kind == 0:
            rows[i] = np.concatenate([ref[s:s + t], ref[s + t + d:s + d + L]])
        elif kind == 1:
            rows[i] = np.concatenate([ref[s:s + L - t], ref[s + L - t + d:s + L + d]])
        else:
            ins = BASES[rng.integers(0, 4, size=d, dtype=np.uint8)]
            cut = t if kind == 2 else L - t - d
            rows[i] = np.concatenate([ref[s:s + cut], ins, ref[s + cut:s + L - d]])
    return rows


def _tip_indel(n=400):
    ref = W.make_reference(300000, seed=31, pad=PAD, repeat_frac=0.05)
    rng = np.random.default_rng(32)
    starts = rng.integers(PAD + 100, len(ref) - PAD - L - 100, size=n)
    rows = _tip_indel_rows(ref, starts, rng)
    minus = rng.random(n) < 0.5
    rows[minus] = W.revcomp_rows(rows[minus])
    return dict(ref=ref, reads=rows.reshape(-1), paired=False)


def _tip_indel_pairs(n_pairs=400):
    """Pairs as make_pairs lays them out (mates on opposite strands, the unsequenced middle triangular on [-100, 100], half the
    fragments from the minus strand), both mates tip-indel reads."""
    ref = workload("tip_indel")["ref"]
    rng = np.random.default_rng(33)
    left = rng.integers(PAD + 100, len(ref) - PAD - 2 * L - 300, size=n_pairs)
    right = left + L + np.rint(rng.triangular(-100, 0, 100, size=n_pairs)).astype(np.int64)
    ra = _tip_indel_rows(ref, left, rng)
    rb = W.revcomp_rows(_tip_indel_rows(ref, right, rng))
    flip = rng.random(n_pairs) < 0.5
    reads = np.empty((2 * n_pairs, L), np.uint8)
    reads[0::2] = np.where(flip[:, None], rb, ra)
    reads[1::2] = np.where(flip[:, None], ra, rb)
    return dict(ref=ref, reads=reads.reshape(-1), paired=True)


def _near_copy(n=500):
    """Six segments of 400-800 bases, each planted four times on a uniform 250 kb reference, every copy with 2-4 substitutions per
    150 bases against the segment.  A read drawn from a copy has its second-best sites at the other copies, 4-8 substitutions
    away: more than CLEARZONE1 (200 points) and, for the nearer ones, less than CLEARZONE3 (800) below the best."""
    ref = W.make_reference(250000, seed=41, pad=PAD)
    rng = np.random.default_rng(42)
    slots = rng.permutation(np.arange(PAD + 2000, len(ref) - PAD - 3000, 9000))[:24]
    copies = []
    for f in range(6):
        n_ = int(rng.integers(400, 801))
        seg = BASES[rng.integers(0, 4, size=n_, dtype=np.uint8)]
        for c in range(4):
            cp = seg.copy()
            for lo in range(0, n_, 150):
                w = min(150, n_ - lo)
                _subst(rng, cp, lo + rng.choice(w, size=min(w, int(rng.integers(2, 5))), replace=False))
            pos = int(slots[4 * f + c])
            ref[pos:pos + n_] = cp
            copies.append((pos, n_))
    rows = np.empty((n, L), np.uint8)
    for i in range(n):
        pos, n_ = copies[int(rng.integers(0, len(copies)))]
        s = pos + int(rng.integers(0, n_ - L + 1))
        rows[i] = ref[s:s + L]
        ns = int(rng.integers(0, 3))
        if ns:
            _subst(rng, rows[i], rng.choice(L, size=ns, replace=False))
    minus = rng.random(n) < 0.5
    rows[minus] = W.revcomp_rows(rows[minus])
    return dict(ref=ref, reads=rows.reshape(-1), paired=False)


def _diverged(n=400):
    """Reads with 10-18 % substitutions (15-27 of 150 bases).  An isolated substitution costs 257 points (the lost match, the
    substitution, and the next match's streak bonus), so a read drops below 0.56 of the maximum (8383 of 14970) from 26 substitutions
    upward and stays above 0.30 up to 40: every other read gets 25-27, the rest 15-24, and the upper half maps at minRatio = 0.30
    where the probe finds it, and not at the default."""
    ref = W.make_reference(200000, seed=51, pad=PAD)
    rng = np.random.default_rng(52)
    starts = rng.integers(PAD + 100, len(ref) - PAD - L - 100, size=n)
    rows = np.empty((n, L), np.uint8)
    for i, s in enumerate(starts):
        rows[i] = ref[int(s):int(s) + L]
        _subst(rng, rows[i], rng.choice(L, size=int(rng.integers(25, 28) if i % 2 else rng.integers(15, 25)), replace=False))
    minus = rng.random(n) < 0.5
    rows[minus] = W.revcomp_rows(rows[minus])
    return dict(ref=ref, reads=rows.reshape(-1), paired=False)


def _pairs(n_pairs=600, **kw):
    ref = W.make_reference(300000, seed=6, pad=PAD, repeat_frac=0.15)
    reads, _ = W.make_pairs(ref, n_pairs, read_len=L, seed=4, pad=PAD, **dict(dict(hard_frac=0.08), **kw))
    return dict(ref=ref, reads=reads, paired=True)


def _repeat_pairs(n_pairs=400):
    ref = W.make_reference(200000, seed=11, pad=PAD, repeat_frac=0.6, families=3)
    reads, _ = W.make_pairs(ref, n_pairs, read_len=L, seed=2, pad=PAD, hard_frac=0.05)
    return dict(ref=ref, reads=reads, paired=True)


WORKLOADS = {
    "pairs": _pairs,                                                    # test_mapper_gpu.py's paired workload at 600 pairs
    "wide_pairs": lambda: _pairs(middle=(50, 900), hard_frac=0.4),      # inserts of 350-1200 bases, many mates only rescue finds
    "repeat_pairs": _repeat_pairs,                                      # long site lists: trimming and the overflow tier
    "tip_indel": _tip_indel,
    "tip_indel_pairs": _tip_indel_pairs,
    "near_copy": _near_copy,
    "diverged": _diverged,
}
_cache = {}


def workload(name):
    """dict ref, reads (uint8, n x L flat, mates interleaved), paired, n -- made once; nobody writes to it"""
    if name not in _cache:
        w = WORKLOADS[name]()
        w["n"] = w["reads"].size // L
        _cache[name] = w
    return _cache[name]


def keys():
    from oracle import oracle as O
    offs = O.make_offsets(L, K, 1.9)
    return offs, [100 * K] * len(offs)


def oracle_index(name):
    from oracle import oracle as O
    w = workload(name)
    oi = O.OracleIndex([w["ref"]], k=K)
    oi.s.p.quitAfterTwoPerfects = 0 if w["paired"] else 1            # BBMap.java:434
    return oi


ORACLE_CAP = {"repeat_pairs": 1024}             # (the oracle's lists have room for what the device's overflow tier holds)


def oracle_run(name, settings, oi=None):
    """oracle.map_batch over the workload under `settings` (strict: oracle_params).  Results are kept per (workload, settings); an
    index made here is kept per workload."""
    from oracle import oracle as O
    key = (name, tuple(sorted((k_, v) for k_, v in settings.items() if k_ not in DEVICE_ONLY)))
    if key not in _cache:
        w = workload(name)
        offs, ks = keys()
        cap = ORACLE_CAP.get(name, 64)
        if oi is None:
            if ("oi", name) not in _cache:
                _cache[("oi", name)] = oracle_index(name)
            oi = _cache[("oi", name)]
        r = w["reads"].reshape(-1, L)
        r1, r2 = (r[0::2].copy(), r[1::2].copy()) if w["paired"] else (r, None)
        _cache[key] = O.map_batch(oi, r1, r2, L, offs, ks, params=oracle_params(settings), cap=cap, match_stride=4200)
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------ what a run did
def finals(orc, paired):
    """FINAL_DTYPE per read, mates interleaved"""
    if not paired:
        return orc["final1"]
    out = np.empty(2 * len(orc["final1"]), orc["final1"].dtype)
    out[0::2], out[1::2] = orc["final1"], orc["final2"]
    return out


def site_lists(orc, paired):
    """one tuple of (chrom, strand, start, stop, slowScore, pairedScore, rescued) tuples per read, mates interleaved"""
    f = ("chrom", "strand", "start", "stop", "slowScore", "pairedScore", "rescued")
    per = []
    for w in ((1, 2) if paired else (1,)):
        s, ns = orc["sites%d" % w], orc["nsites%d" % w]
        per.append([tuple(tuple(int(x[g]) for g in f) for x in s[i, :max(0, int(ns[i]))]) for i in range(len(ns))])
    return per[0] if not paired else [x for pr in zip(*per) for x in pr]


def fills_by_key(orc):
    """{(read, seq): (kind, refStartLoc, refEndLoc, minScore)} of a run's fill log"""
    g = orc["log"]
    return {(int(g["read"][i]), int(g["seq"][i])): (int(g["kind"][i]), int(g["refStartLoc"][i]), int(g["refEndLoc"][i]), int(g["minScore"][i]))
            for i in range(len(g))}


def kind_counts(orc):
    return np.bincount(orc["log"]["kind"], minlength=7).tolist()


def measure(a, b, paired):
    """What differs between two oracle runs of one workload, as counts: the numbers the liveness conditions are stated in."""
    fa, fb = finals(a, paired), finals(b, paired)
    from tests.mapper_check import FINAL_FIELDS
    la, lb = site_lists(a, paired), site_lists(b, paired)
    ka, kb = fills_by_key(a), fills_by_key(b)
    both = sorted(set(ka) & set(kb))
    same_kind = [k_ for k_ in both if ka[k_][0] == kb[k_][0]]
    resc = lambda lst: tuple(x for x in lst if x[6])
    ca, cb = kind_counts(a), kind_counts(b)
    k1a = sorted(v[1:3] for v in ka.values() if v[0] == 1)
    k1b = sorted(v[1:3] for v in kb.values() if v[0] == 1)
    return dict(
        final=int(sum(any(int(fa[r][f]) != int(fb[r][f]) for f in FINAL_FIELDS) for r in range(len(fa)))),
        mapped=abs(int((fa["mapped"] > 0).sum()) - int((fb["mapped"] > 0).sum())),
        paired_flags=int((fa["paired"] != fb["paired"]).sum()),
        score_or_ambiguous=int(((fa["mapScore"] != fb["mapScore"]) | (fa["ambiguous"] != fb["ambiguous"])).sum()),
        site_lists=int(sum(x != y for x, y in zip(la, lb))),
        starts=int(sum(tuple(s[:4] for s in x) != tuple(s[:4] for s in y) for x, y in zip(la, lb))),
        rescued_sites=int(sum(resc(x) != resc(y) for x, y in zip(la, lb))),
        windows=int(sum(ka[k_][1:3] != kb[k_][1:3] for k_ in same_kind)),
        minscores=int(sum(ka[k_][3] != kb[k_][3] for k_ in same_kind)),
        fills=(len(ka), len(kb)), kind1=(ca[1], cb[1]), kind2=(ca[2], cb[2]), kind4=(ca[4], cb[4]),
        kind1_windows=int(len(k1a) != len(k1b) or sum(x != y for x, y in zip(k1a, k1b))),
        identical=bool(fa.tobytes() == fb.tobytes() and la == lb and ka == kb))


# ---------------------------------------------------------------------------------------------------------------- the cases
# effects: names of measure()'s counts that must reach FLOOR (the floor test_mapper_gpu.py uses for "rescue really ran"), or
#   "kind1_count"      the number of kind-1 fills (scoreSlow's wider refill) differs from the base run's
#   "refills>=10"      the run itself logs at least 10 kind-1 fills
#   "final>=1"         at least one final record differs (an effect found on one or two reads only; the case's other effects hold
#                      the floor)
#   "same_as_base"     nothing at all differs from the base run
#   "same_as:NAME"     nothing at all differs from the run of case NAME (which has effects of its own)
#   "final_same_as:NAME"  the final records equal those of case NAME's run ("defaults": the run at the profile's defaults)
# base: the settings of the run the case is compared with (default: the profile's defaults).
FLOOR = 5
Case = collections.namedtuple("Case", "name workload settings effects base mapper")


def _case(name, workload, settings, effects, base=None, **mapper):
    return Case(name, workload, settings, tuple(effects), base or {}, mapper)


PAD0, PAD1, PAD8, PAD12, PAD20 = (dict(slowAlignPadding=p, slowRescuePadding=p) for p in (0, 1, 8, 12, 20))
NO_TIP = dict(tipSearchDist=0)
CASES = [
    # both arms of ratioPaired / ratioPreRescue's max() (AbstractMapThread.java:106-107): 0.30 and 0.56 take the first arm of both,
    # 0.76 the second arm of both (0.608 < 0.664, 0.456 < 0.568), 0.90 likewise (0.72 < 0.86, 0.54 < 0.82)
    _case("minRatio_0.30_pairs", "pairs", dict(minRatio=0.30), ["minscores"]),
    _case("minRatio_0.30_diverged", "diverged", dict(minRatio=0.30), ["mapped", "final"]),
    _case("minRatio_0.76", "pairs", dict(minRatio=0.76), ["final"]),
    _case("minRatio_0.90", "pairs", dict(minRatio=0.90), ["final"]),
    _case("padding_0_single", "tip_indel", dict(PAD0, **NO_TIP), ["windows", "kind1_count"], base=NO_TIP),
    _case("padding_1_single", "tip_indel", dict(PAD1, **NO_TIP), ["windows"], base=NO_TIP),
    _case("padding_20_single", "tip_indel", dict(PAD20, **NO_TIP), ["windows"], base=NO_TIP),
    _case("padding_0_paired", "wide_pairs", PAD0, ["windows", "kind1_count"]),
    _case("padding_1_paired", "wide_pairs", PAD1, ["windows"]),
    _case("padding_20_paired", "wide_pairs", PAD20, ["windows"]),
    # at 20 / 20 the first fill is wide enough that no site asks for a refill; at 12 / 12 some still do, so a refill at a widened
    # slowAlignPadding runs (windows of 150 + 2 * 22 columns and the tip indel's length)
    _case("padding_12_refills", "tip_indel_pairs", dict(PAD12, **NO_TIP), ["windows", "kind1_count"], base=NO_TIP),
    _case("extraPadding_0", "tip_indel", dict(extraPadding=0, **NO_TIP), ["kind1_windows", "refills>=10"], base=NO_TIP),
    _case("extraPadding_30", "tip_indel", dict(extraPadding=30, **NO_TIP), ["kind1_windows", "refills>=10"], base=NO_TIP),
    # at slowAlignPadding = 2 the two refill widths differ in what the site adopts: one site of the 800 mates keeps another fill
    # (BBMapThread.java:322-335 keeps the wider fill unless it scores lower), and two final records move
    _case("extraPadding_0_padding_2", "tip_indel_pairs", dict(NO_TIP, slowAlignPadding=2, extraPadding=0),
          ["kind1_windows", "refills>=10", "final>=1"], base=dict(NO_TIP, slowAlignPadding=2, extraPadding=30)),
    _case("extraPadding_30_padding_2", "tip_indel_pairs", dict(NO_TIP, slowAlignPadding=2, extraPadding=30),
          ["kind1_windows", "refills>=10", "final>=1"], base=dict(NO_TIP, slowAlignPadding=2, extraPadding=0)),
    _case("tipSearchDist_0", "tip_indel", NO_TIP, ["kind1_count", "refills>=10"]),
    _case("tipSearchDist_15", "tip_indel", dict(tipSearchDist=15), ["windows", "site_lists"]),
    _case("refill_paired", "tip_indel_pairs", NO_TIP, ["kind1_count", "refills>=10"]),
    # logs that start at 64 entries: phase 0 meets NO_ROOM (more than 300 reads find no room in the first round).  The first growth
    # takes a log to what the round asked for, a quarter more and 1024 entries, which is more than these batches log in all, so no
    # refill of phase 1 waits for room here, and nothing in stats() would show it if one did
    _case("refill_small_logs", "tip_indel", NO_TIP, ["kind1_count", "refills>=10"], jobsPerRead=-64),
    _case("refill_paired_small_logs", "tip_indel_pairs", NO_TIP, ["kind1_count", "refills>=10"], jobsPerRead=-64),
    _case("maxPairDist_500", "wide_pairs", dict(maxPairDist=500), ["paired_flags"]),
    # a limit inside the mates' own spread of inner distances: pairing decides by the site lists' coordinates, the final stage then
    # realigns the tip indels, and three pairs keep their `paired` flag with a final inner distance of 19 or 22 bases -- the only
    # input found on which the run statistics' clamp at maxPairDist binds (tests/test_mapper_config_gpu.py)
    _case("maxPairDist_18_tip_indel", "tip_indel_pairs", dict(NO_TIP, maxPairDist=18), ["paired_flags"], base=NO_TIP),
    _case("doRescue_0", "pairs", dict(doRescue=0), ["final", "rescued_sites"]),
    _case("maxRescueDist_250", "pairs", dict(maxRescueDist=250), ["same_as:doRescue_0"]),
    # rescue is off when min(maxPairDist, 2 * averagePairDist + 100) > maxRescueDist = 1200 (AbstractMapThread.java:1146-1151): 1200 / 1202.
    # averagePairDist also enters the paired scores, so the two are compared with each other's neighbours: 550 with rescue on must
    # keep rescuing, 551 must equal 550 with rescue switched off
    _case("averagePairDist_550", "pairs", dict(averagePairDist=550), ["rescued_sites", "final_same_as:defaults"],
          base=dict(averagePairDist=550, doRescue=0)),
    _case("averagePairDist_551", "pairs", dict(averagePairDist=551), ["same_as_base", "final_same_as:doRescue_0"],
          base=dict(averagePairDist=551, doRescue=0)),
    _case("averagePairDist_400_wide", "wide_pairs", dict(averagePairDist=400), ["rescued_sites"]),
    _case("maxRescueMismatches_3", "pairs", dict(maxRescueMismatches=3), ["rescued_sites"]),
    _case("maxRescueMismatches_0", "pairs", dict(maxRescueMismatches=0), ["rescued_sites"]),
    _case("maxTrimSitesToRetain_2", "repeat_pairs", dict(maxTrimSitesToRetain=2), ["site_lists"]),
    _case("maxTrimSitesToRetain_8", "repeat_pairs", dict(maxTrimSitesToRetain=8), ["site_lists"]),
    _case("clearzone3_0_repeats", "repeat_pairs", dict(clearzone3=0), ["minscores"]),
    _case("clearzone3_0_near_copy", "near_copy", dict(clearzone3=0), ["score_or_ambiguous"]),
    _case("combined", "wide_pairs", dict(PAD8, minRatio=0.90, maxPairDist=500, clearzone3=0), ["final", "paired_flags", "windows"]),
    _case("overflow_tier", "repeat_pairs", dict(PAD8, minRatio=0.90), ["final", "windows"], max_sites=4),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def missed_effects(case):
    """Runs the oracle under the case's settings and under its base and returns (the list of effects the case misses -- empty: the
    setting is live on this input --, measure()'s counts)."""
    w = workload(case.workload)
    run = oracle_run(case.workload, case.settings)
    m = measure(oracle_run(case.workload, case.base), run, w["paired"])
    missed = []
    for e in case.effects:
        if e == "kind1_count":
            ok = m["kind1"][0] != m["kind1"][1]
        elif e == "refills>=10":
            ok = m["kind1"][1] >= 10
        elif e == "final>=1":
            ok = m["final"] >= 1
        elif e == "same_as_base":
            ok = m["identical"]
        elif e.startswith("same_as:") or e.startswith("final_same_as:"):
            how, other = e.split(":")
            o = BY_NAME.get(other)
            o_run = oracle_run(case.workload, o.settings if o else {})
            assert other == "defaults" or (o.workload == case.workload and not missed_effects(o)[0]), other
            d = measure(o_run, run, w["paired"])
            ok = d["identical"] if how == "same_as" else d["final"] == 0
        else:
            ok = m[e] >= FLOOR
        if not ok:
            missed.append(e)
    return missed, m
