"""Unlimited fills (fillUnlimited) on the wavefront kernel, record by record against the oracle.

A width-sorted launch gives the unlimited fills a list of their own and runs it through the kernel's build for them (no limits,
no prune tests, no good-column extents: msa_fill_fast.hip, UNL); every other route, the wide pass and BBMSA_UNLIMITED_LOOP=0 leave
them to the general build.  bbmsa_last_unlimited says which build ran how many, and how many wavefront steps they were.  Every
set below goes through the sorted route, the plain first pass, the latency route and the _indirect entry, each with the switch on
and off: every record is the oracle's, the bytes of on and off are the same, and the counters are what the set predicts.

The sets plant every way into the unlimited fill (the raw flag, minScore < 1, rows + columns < 90, the width clause on both sides
of its edge, the band clause on a banded context), reads of 1 to 6 rows (the barrier rows of both planes), windows of rows - 2
columns, windows clamped at both ends, perfect reads, substitutions, indels of 1-6 and of 200 bases, N in read and reference,
'-' runs with and without BBMSA_TRACE_KEEP_GAPS, and a 40-row read whose deletion streak passes the time field's 2,047.

One recorded deviation: at 64 lanes x 5 rows the general build's `iterations` of a few LIMITED fills is not the oracle's; those
jobs are compared with the numbers recorded in tests/golden/msa_64x5_limited_iterations.json (see KNOWN_ITERATIONS)."""
import json
import os
import random

import numpy as np
import pytest

from bbmap_amd import msa as M
from oracle.oracle import OracleMSA
from tests.msa_check import oracle_align
from tests.problems import max_quality, mutate, rand_seq
from tests.test_msa_routes_gpu import Dev, _gapped_set, check_against_oracle, record, run

pytestmark = pytest.mark.gpu

KEEP_GAPS = 1 << 7
ALL = M.FILL_AND_SCORE_LIMITED | M.DO_TRACEBACK
RAW_U = M.FILL_UNLIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
RAW_L = M.FILL_LIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
UNBANDED, BANDED = (0, 0.0), (40, 0.18)
ENV = ("BBMSA_NARROW", "BBMSA_SORT_BY_WIDTH", "BBMSA_LATENCY_JOBS", "BBMSA_LANES_PER_JOB", "BBMSA_UNLIMITED_LOOP", "BBMSA_UNLIMITED_STATS", "BBMSA_GENERIC_SCRATCH_MB")

# name: (maxRows, maxColumns, fast_cols, lanes, band, typical read length)
CONTEXTS = {
    "160x704_32x5": (160, 704, 384, 32, UNBANDED, 150),        # 32 lanes x 5 rows, two jobs per wave; wide pass 64 x 3
    "160x704_16x10": (160, 704, 384, 16, UNBANDED, 150),       # four jobs per wave
    "320x704_64x5": (320, 704, 704, 64, UNBANDED, 150),        # one job per wave, no wide pass; unlimited fills of 300 and 320 rows beside the 150-row mix
    "64x2304_clamp": (64, 2304, 2304, 32, UNBANDED, 40),       # windows of more than 2,047 columns in the first pass
    "160x704_banded": (160, 704, 384, 32, BANDED, 150),
}


def make_ctx(monkeypatch, name, env):
    maxR, maxC, fast, lanes, band, _ = CONTEXTS[name]
    return new_ctx(monkeypatch, env, maxR, maxC, fast, lanes, band)


def new_ctx(monkeypatch, env, maxR, maxC, fast, lanes, band=UNBANDED):
    """A context that counts for bbmsa_last_unlimited, created under `env`."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BBMSA_GENERIC_SCRATCH_MB", "256")
    monkeypatch.setenv("BBMSA_UNLIMITED_STATS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return M.MSAContext(maxR, maxC, band[0], band[1], lanes_per_job=lanes, fast_cols=fast)
    finally:
        for k in ENV:
            monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------ job sets
def _jobset(name, seed=11):
    """(problems, flags) for one context: the planted cases first, then a seeded mix of limited and unlimited fills, shuffled."""
    maxR, maxC, fast, lanes, band, L = CONTEXTS[name]
    rng = random.Random(seed)
    ref = bytearray(rand_seq(rng, 12000))
    n_at = [1000 + 700 * i for i in range(12)]
    for i in n_at:
        ref[i] = ord("N")
    ref = bytes(ref)
    short = rand_seq(rng, min(maxC - 8, 2 * L + 40))                    # windows clamped at both ends
    pieces, pos = [], 0                                                # '-' runs every few hundred bases
    while pos < 6000:
        step = rng.randrange(120, 400)
        pieces.append(ref[pos:pos + step])
        pieces.append(b"-" * rng.randint(1, 4))
        pos += step
    gref = b"".join(pieces)
    gap_at = [i for i in range(400, len(gref) - 1000) if gref[i] == ord("-") and gref[i - 1] != ord("-")]
    probs, flags = [], []

    def add(rd, G, a, b, ms, fl):
        assert 1 <= len(rd) <= maxR and len(rd) - 2 <= b - a + 1 and min(b, len(G) - 1) - max(a, 0) + 1 <= maxC, (name, len(rd), a, b)
        assert (fl & M.CLAMP_WINDOW) or (0 <= a and b < len(G)), (name, a, b)      # an unclamped window lies inside its array
        probs.append((bytes(rd), G, a, b, ms))
        flags.append(fl)

    def site(n, extra=0):
        return rng.randrange(800, len(ref) - n - extra - 3000)

    def window(st, n, width, left=None):
        left = rng.randrange(0, max(1, width - n)) if left is None else left
        return st - left, st - left + width - 1

    wide = min(maxC, 700)
    # -- every way into the unlimited fill
    for fl in (RAW_U, RAW_L):                                          # the raw modes at the same windows
        for width in (L + 8, L + 60, 330, fast, fast + 1, wide):
            if not L <= width <= maxC:
                continue
            st = site(L, width)
            a, b = window(st, L, width)
            add(mutate(rng, ref[st:st + L + 12], n_prob=0.05)[:L], ref, a, b, int(0.5 * max_quality(L)), fl)
    for ms in (0, -5, 1):                                              # minScore < 1 (1: limited)
        st = site(L, 40)
        add(mutate(rng, ref[st:st + L + 12], n_prob=0.0)[:L], ref, st - 6, st + L + 20, ms, ALL)
    for rows, cols in ((30, 40), (30, 59), (30, 60), (44, 45), (45, 45)):      # rows + columns < 90, and just not
        if rows <= maxR:
            st = site(rows, cols)
            add(ref[st:st + rows], ref, st - 3, st - 3 + cols - 1, int(0.4 * max_quality(rows)), ALL)
    for rows, cols in ((150, 320), (150, 321), (40, 100), (40, 101), (L, L + min(170, L + 20)), (L, L + min(170, L + 20) + 1)):
        if rows <= maxR and cols <= maxC:                              # the width clause on both sides of its edge
            st = site(rows, cols)
            a, b = window(st, rows, cols, left=(cols - rows) // 2)
            add(mutate(rng, ref[st:st + rows + 12], n_prob=0.0)[:rows], ref, a, b, int(0.4 * max_quality(rows)), ALL)
    if band != UNBANDED:                                               # the band clause: halfband * 3 > columns from 428 columns on at 150 rows
        for cols in range(418, 440, 2):
            st = site(150, cols)
            a, b = window(st, 150, cols, left=6)
            add(mutate(rng, ref[st:st + 162], n_prob=0.0)[:150], ref, a, b, int(0.4 * max_quality(150)), ALL)
    # -- content
    for rows in (1, 2, 3, 4, 5, 6):                                    # the barrier rows of both planes
        for cols in sorted({max(1, rows - 2), rows, rows + 3, 40, 330}):
            st = site(rows, cols)
            rd = bytearray(ref[st:st + rows])
            if rows > 2 and cols > rows:
                rd[rows // 2] = rng.choice(b"ACGT")
            a = st - min(2, max(0, cols - rows))
            for fl in (ALL, RAW_U):
                add(rd, ref, a, a + cols - 1, 0 if rows < 3 else 40, fl)
    for width in (L - 2, L - 1, L):                                    # windows of rows - 2 columns and up
        st = site(L)
        add(ref[st:st + L], ref, st + (L - width), st + L - 1, 0, rng.choice([ALL, RAW_U]))
    for k in (1, 17, 39):                                              # clamped at both ends
        rd = mutate(rng, short[20:20 + L + 10], n_prob=0.0)[:L]
        add(rd, short, -k, len(short) - 1 + k, 0, ALL)
        add(rd, short, -k, len(short) - 1 + k, 0, M.FILL_UNLIMITED_RAW | M.CLAMP_WINDOW | M.DO_SCORE | M.DO_TRACEBACK)
    for n in (1, 2, 3, 4, 5, 6):                                       # indels of 1-6 bases, perfect reads, substitutions
        st = site(L + 8, 340)
        p = rng.randrange(L // 3, L - L // 3)
        dele = ref[st:st + p] + ref[st + p + n:st + L + n]
        ins = (ref[st:st + p] + rand_seq(rng, n) + ref[st + p:st + L])[:L]
        sub = bytearray(ref[st:st + L])
        for _ in range(n):
            sub[rng.randrange(L)] = rng.choice(b"ACGT")
        for rd in (dele, ins, sub, ref[st:st + L]):
            a, b = window(st, L, max(330, L + 60) + rng.choice([0, 10]), left=rng.randrange(2, 40))
            add(rd, ref, a, b, int(0.4 * max_quality(L)), rng.choice([ALL, RAW_U]))
    if L + 200 + 12 <= maxC:                                           # a 200-base deletion (the window is wide enough to be unlimited)
        for _ in range(4):
            st = site(L, 260)
            p = rng.randrange(L // 3, L - L // 3)
            add(ref[st:st + p] + ref[st + p + 200:st + L + 200], ref, st - 6, st + L + 205, int(0.3 * max_quality(L)), ALL)
    if maxR >= 320:
        # reads that use (nearly) every lane of the 64 x 5 geometry, unlimited fills only: perfect, mutated, with a 200-base insertion
        for rows in (300, 320):
            for i in range(24):
                st = site(rows, 400)
                if i % 4 == 3:
                    rd = ref[st:st + 50] + rand_seq(rng, 200) + ref[st + 50:st + rows - 200]
                else:
                    rd = (mutate(rng, ref[st:st + rows + 12], n_prob=0.05) + ref[st + rows + 12:st + rows + 40])[:rows] if i % 4 else ref[st:st + rows]
                width = rng.choice([rows - 2, rows + 8, 400, rows + min(170, rows + 20) + 1, 640, 704])
                a, b = window(st, rows, width, left=rng.randrange(0, 8) if width > rows + 8 else 0)
                # the raw flag, minScore < 1, or (past rows + 170 columns) the width clause
                fl, ms = (RAW_U, 5000) if i % 3 == 0 else ((ALL, 0) if width <= rows + 170 or i % 3 == 1 else (ALL, int(0.3 * max_quality(rows))))
                add(rd, ref, a, b, ms, fl)
    for i in range(6):                                                 # N in the read and in the reference
        st = n_at[i] - rng.randrange(5, L - 5)
        rd = bytearray(ref[st:st + L])
        for _ in range(rng.randint(1, 3)):
            rd[rng.randrange(L)] = ord("N")
        add(rd, ref, st - 10, st + 330, int(0.3 * max_quality(L)), rng.choice([ALL, RAW_U]))
    for i in range(10):                                                # '-' runs, with and without KEEP_GAPS
        g = rng.choice(gap_at)
        st = g - rng.randrange(10, L - 10)
        rd = gref[st:st + L + 8].replace(b"-", b"")[:L]
        fl = (ALL, ALL | KEEP_GAPS, RAW_U, RAW_U | KEEP_GAPS)[i % 4]
        add(rd, gref, st - 4, st + rng.choice([L + 12, 335, 400]), int(0.3 * max_quality(len(rd))) if i % 2 else 0, fl)
    if maxC >= 2300:                                                   # a deletion streak past the time field's 2,047
        for dl in (2040, 2100, 2200):
            st = site(40, 2400)
            rd = ref[st:st + 20] + ref[st + 20 + dl:st + 40 + dl]
            for fl in (ALL, RAW_U):
                add(rd, ref, st - 20, st - 20 + 2299, int(0.3 * max_quality(40)), fl)
    # -- a seeded mix to fill the launch (the sort's floor is 256 jobs)
    while len(probs) < 330:
        width = rng.choice([L + 8, L + 30, L + 40, L + 55, L + 100, 322, 330, 380, fast, fast + 8, wide])
        width = max(min(width, maxC), L)
        st = site(L, width)
        a, b = window(st, L, width, left=rng.randrange(0, 20))
        add(mutate(rng, ref[st:st + L + 12], n_prob=0.05)[:L], ref, a, b, int(rng.choice([0.3, 0.5, 0.7]) * max_quality(L)),
            rng.choice([ALL, ALL, ALL | M.NO_ITERATIONS, RAW_U, RAW_L, M.FILL_LIMITED | M.CLAMP_WINDOW | M.DO_TRACEBACK]))
    order = list(range(len(probs)))
    rng.shuffle(order)
    return [probs[k] for k in order], [flags[k] for k in order]


_CACHE = {}


def jobset(name):
    """The set of a context, packed, with the oracle's answer per job: computed once and shared."""
    if name not in _CACHE:
        maxR, maxC, fast, lanes, band, L = CONTEXTS[name]
        probs, flags = _jobset(name)
        jobs, reads, refs = M.pack_problems(probs, flags)
        om = OracleMSA(maxR, maxC, band[0], band[1])
        exp = [oracle_align(om, p[0], p[1], p[2], p[3], p[4], f) for p, f in zip(probs, flags)]
        stride = (max(len(p[0]) + (p[3] - p[2] + 1) + 8 + 127 * bytes(p[1][max(0, p[2]):max(0, p[3] + 1)]).count(b"-") for p in probs) + 15) & ~15
        _CACHE[name] = (probs, flags, jobs, reads, refs, exp, stride)
    return _CACHE[name]


def columns_of(p, fl):
    a, b = p[2], p[3]
    if fl & M.CLAMP_WINDOW:
        a, b = max(0, a), min(len(p[1]) - 1, b)
    return b - a + 1


def predict(name, probs, flags, exp, geo, route, switch, jobs=None):
    """What bbmsa_last_unlimited must show: the unlimited build takes the unlimited fills of a sorted launch that fit the first
    pass; a fill counts (with columns + lanes in use - 1 steps) in the pass that ran it.  (A banded limited fill whose rows have a
    hole runs in the first pass, again in the wide pass and then on the one-thread kernel: see counters_match.)"""
    fast, R, wideR = geo["fast_cols"], geo["rows_per_lane"], geo["wide_rows_per_lane"]
    out = {"stripped": 0, "general": 0, "unlimited_steps": 0, "steps": 0}
    for k in (range(len(probs)) if jobs is None else jobs):
        rows, cols = len(probs[k][0]), columns_of(probs[k], flags[k])
        first = route != "latency" and cols <= fast
        steps = cols + (rows + (R if first else wideR) - 1) // (R if first else wideR) - 1
        out["steps"] += steps
        if exp[k]["fill_kind"] == 1:
            out["unlimited_steps"] += steps
            out["stripped" if (route == "sorted" and switch and first) else "general"] += 1
    return out


# In the 64-lane x 5-row context the general build's visited-cell count of a few LIMITED fills differs from the oracle's by a few
# cells, every other field equal: the limited loop's good-column bookkeeping, which the unlimited build does not have.  The fixture
# lists those jobs of the "320x704_64x5" set with the oracle's count and the kernel's, as the library of the commit before the
# unlimited build and this one both give it.  Exactly these jobs are compared with the recorded kernel count; every other job,
# limited or not, with the oracle's.  A fill that starts or stops deviating, or deviates by another amount, fails the test.
KNOWN_ITERATIONS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msa_64x5_limited_iterations.json")
KNOWN_CONTEXT = "320x704_64x5"


def known_iterations(exp):
    with open(KNOWN_ITERATIONS_FILE) as f:
        known = {int(r["job"]): r for r in json.load(f)["jobs"]}
    assert len(known) <= 12                                            # one limited fill in seven at the most: a list, not a waiver
    for k, r in known.items():
        assert exp[k]["fill_kind"] == 0 and exp[k]["iterations"] == r["oracle"] and 0 < abs(r["kernel"] - r["oracle"]) <= 9, (k, r)
    return {k: r["kernel"] for k, r in known.items()}


def expected(name, exp, picks=None):
    """The oracle's records, with the recorded kernel count in the listed jobs (picks: the set's job index of each record)."""
    if name != KNOWN_CONTEXT:
        return exp
    known = known_iterations(jobset(name)[5])
    picks = range(len(exp)) if picks is None else picks
    return [dict(e, iterations=known[j]) if j in known else e for j, e in zip(picks, exp)]


def counters_match(name, u, want):
    if CONTEXTS[name][4] == UNBANDED:
        return u == want
    return dict(u, steps=0) == dict(want, steps=0) and want["steps"] <= u["steps"] <= 2 * want["steps"]


ROUTES = {
    "sorted": {"BBMSA_NARROW": 0, "BBMSA_SORT_BY_WIDTH": 1},
    "first_pass": {"BBMSA_NARROW": 0},
    "latency": {"BBMSA_NARROW": 0, "BBMSA_LATENCY_JOBS": 1 << 20},
    "indirect": {"BBMSA_NARROW": 0, "BBMSA_SORT_BY_WIDTH": 1},
}


# ------------------------------------------------------------------------------------------------ every route, switch on and off
@pytest.mark.parametrize("name", sorted(CONTEXTS))
def test_unlimited_fills_match_the_oracle_on_every_route_with_the_switch_on_and_off(monkeypatch, name):
    probs, flags, jobs, reads, refs, exp, stride = jobset(name)
    bad = [False] * len(probs)
    n_unl = sum(e["fill_kind"] == 1 for e in exp)
    assert n_unl > 60 and len(probs) - n_unl > 40                      # both kinds, well mixed
    if name == "160x704_banded":                                       # the band clause decided both ways
        kinds = {e["fill_kind"] for p, f, e in zip(probs, flags, exp) if f == ALL and len(p[0]) == 150 and 418 <= p[3] - p[2] + 1 < 440 and p[4] > 0}
        assert kinds == {0, 1}
    if name == "64x2304_clamp":                                        # the deletion plane's time was clamped on the way
        assert sum(e["match"] is not None and b"D" * 2050 in e["match"] for e in exp) >= 4
    dev = Dev(jobs, reads, refs)
    first = None
    for route, env in ROUTES.items():
        for switch in (1, 0):
            ctx = make_ctx(monkeypatch, name, dict(env, BBMSA_UNLIMITED_LOOP=switch))
            geo = ctx.geometry()
            rec, mat = run(ctx, dev, stride, count=len(probs) if route == "indirect" else None)
            r, u = ctx.last_route(), ctx.last_unlimited()
            ctx.close()
            tag = "%s route %s switch %d" % (name, route, switch)
            assert r["sorted"] == (route == "sorted") and r["latency"] == (route == "latency") and r["indirect"] == (route == "indirect"), (tag, r)
            assert not r["narrow"], (tag, r)
            check_against_oracle(rec, mat, expected(name, exp), flags, bad, tag)
            assert counters_match(name, u, predict(name, probs, flags, exp, geo, route, switch)), (tag, u)
            if route == "sorted" and switch:
                assert u["stripped"] > 60, (tag, u)
            if first is None:
                first = (rec.copy(), mat.copy())
            else:                                                      # every route, on and off: the same bytes
                assert rec.tobytes() == first[0].tobytes(), tag
                assert mat.tobytes() == first[1].tobytes(), tag


# ------------------------------------------------------------------------------------------------ who shares a wavefront
PATTERNS = {2: ["UU", "UL", "LU", "LL"], 4: ["UUUU", "UULU", "LUUU", "LLLL", "ULLL"], 1: ["U", "L"]}


@pytest.mark.parametrize("name", ["160x704_32x5", "160x704_16x10", "320x704_64x5"])
def test_unlimited_and_limited_fills_side_by_side_in_a_wavefront(monkeypatch, name):
    """Unsorted, so that list position decides which jobs share a wavefront: every pattern of unlimited (U) and limited (L) fills
    within a wave, each pattern 40 (one job per wave: 140) times in a row and then an odd tail.  The general build runs all of them (it is exact for an
    unlimited fill beside a limited one); the sorted launch of the same list separates them."""
    probs, flags, jobs, reads, refs, exp, stride = jobset(name)
    per_wave = 64 // CONTEXTS[name][3]
    fast = CONTEXTS[name][2]
    pool = {"U": [k for k, e in enumerate(exp) if e["fill_kind"] == 1 and columns_of(probs[k], flags[k]) <= fast],
            "L": [k for k, e in enumerate(exp) if e["fill_kind"] == 0 and columns_of(probs[k], flags[k]) <= fast]}
    rng = random.Random(5)
    pick = []
    for pat in PATTERNS[per_wave]:
        for _ in range(40 if per_wave > 1 else 140):                   # (the sort's floor is 256 jobs)
            pick += [rng.choice(pool[c]) for c in pat]
    pick += [rng.choice(pool["U"]) for _ in range(per_wave + 1 if per_wave > 1 else 1)]     # an odd tail: the last wave has a padding job
    if per_wave > 1:
        assert len(pick) % per_wave == 1
    pj = jobs[pick]
    dev = Dev(pj, reads, refs)
    pexp, pflags, pprobs = [exp[k] for k in pick], [flags[k] for k in pick], [probs[k] for k in pick]
    first = None
    for route in ("first_pass", "sorted"):
        for switch in (1, 0):
            ctx = make_ctx(monkeypatch, name, dict(ROUTES[route], BBMSA_UNLIMITED_LOOP=switch))
            geo = ctx.geometry()
            rec, mat = run(ctx, dev, stride)
            r, u = ctx.last_route(), ctx.last_unlimited()
            ctx.close()
            tag = "%s patterns route %s switch %d" % (name, route, switch)
            assert r["sorted"] == (route == "sorted") and r["first_handed_on"] == 0, (tag, r)
            check_against_oracle(rec, mat, expected(name, pexp, pick), pflags, [False] * len(pick), tag)
            want = predict(name, pprobs, pflags, pexp, geo, route, switch)
            assert u == want, (tag, u, want)
            n_u = sum(e["fill_kind"] == 1 for e in pexp)
            assert (u["stripped"], u["general"]) == ((n_u, 0) if route == "sorted" and switch else (0, n_u)), (tag, u)
            if first is None:
                first = (rec.copy(), mat.copy())
            else:
                assert rec.tobytes() == first[0].tobytes() and mat.tobytes() == first[1].tobytes(), tag


@pytest.mark.parametrize("n", [256, 257, 259])
def test_sorted_launch_sizes_with_one_and_no_unlimited_fill(monkeypatch, n):
    """The sort's floor (256 jobs) and odd counts, with lists of unlimited fills of 0, 1, 3 and n entries."""
    name = "160x704_32x5"
    probs, flags, jobs, reads, refs, exp, stride = jobset(name)
    fast = CONTEXTS[name][2]
    U = [k for k, e in enumerate(exp) if e["fill_kind"] == 1 and columns_of(probs[k], flags[k]) <= fast]
    L = [k for k, e in enumerate(exp) if e["fill_kind"] == 0]
    ctx = make_ctx(monkeypatch, name, dict(ROUTES["sorted"]))
    geo = ctx.geometry()
    for n_u in (0, 1, 3, n):
        pick = [U[i % len(U)] for i in range(n_u)] + [L[i % len(L)] for i in range(n - n_u)]
        random.Random(n + n_u).shuffle(pick)
        rec, mat = run(ctx, Dev(jobs[pick], reads, refs), stride)
        r, u = ctx.last_route(), ctx.last_unlimited()
        tag = "n %d unlimited %d" % (n, n_u)
        assert r["sorted"], (tag, r)
        pexp, pflags, pprobs = [exp[k] for k in pick], [flags[k] for k in pick], [probs[k] for k in pick]
        check_against_oracle(rec, mat, pexp, pflags, [False] * n, tag)
        assert u == predict(name, pprobs, pflags, pexp, geo, "sorted", 1), (tag, u)
        assert u["stripped"] == n_u and u["general"] == 0, (tag, u)
    ctx.close()


# ------------------------------------------------------------------------------------------------ every rows-per-lane build
@pytest.mark.parametrize("R", range(1, 11))
def test_every_rows_per_lane_build_of_the_unlimited_kernel(monkeypatch, R):
    """The unlimited build is compiled for R = 1..10 rows per lane; R decides which lane owns a row, the lane and slot that keep the
    last row's maximum, where a traceback record lies, and the register budget.  A context of 32 R rows at 32 lanes launches
    build R over a sorted list of unlimited fills only: the row counts 1, 2, R, R + 1, 2R, M/2, M/2 + 1, 31R, 31R + 1, M - 1, M
    (M = 32 R) with perfect and mutated reads and N, in windows of rows - 2 columns up to the context's 704."""
    Mx, maxC = 32 * R, 704
    rng = random.Random(100 + R)
    ref = bytearray(rand_seq(rng, 3200))
    for i in range(900, 2900, 230):
        ref[i] = ord("N")
    ref = bytes(ref)
    row_counts = sorted({1, 2, R, R + 1, 2 * R, Mx // 2, Mx // 2 + 1, 31 * R, 31 * R + 1, Mx - 1, Mx})
    probs, flags = [], []
    while len(probs) < 264:
        rows = row_counts[len(probs) % len(row_counts)]
        width = rng.choice([max(1, rows - 2), rows, rows + 8, rows + 40, min(maxC, rows + 200), maxC])
        st = rng.randrange(800, 1300)
        rd = ref[st:st + rows] if len(probs) % 3 == 0 else (mutate(rng, ref[st:st + rows + 12], n_prob=0.1) + ref[st + rows + 12:st + rows + 40])[:rows]
        left = 0 if width <= rows else rng.randrange(0, min(8, width - rows) + 1)
        fl, ms = (RAW_U, 700) if len(probs) % 2 else (ALL, 0)           # the raw flag, or minScore < 1 through the gate
        probs.append((bytes(rd), ref, st - left, st - left + width - 1, ms))
        flags.append(fl)
    jobs, reads, refs = M.pack_problems(probs, flags)
    om = OracleMSA(Mx, maxC)
    exp = [oracle_align(om, p[0], p[1], p[2], p[3], p[4], f) for p, f in zip(probs, flags)]
    assert all(e["fill_kind"] == 1 for e in exp)
    stride = (Mx + maxC + 8 + 15) & ~15
    ctx = new_ctx(monkeypatch, ROUTES["sorted"], Mx, maxC, maxC, 32)
    geo = ctx.geometry()
    assert geo["lanes"] == 32 and geo["rows_per_lane"] == R, geo
    rec, mat = run(ctx, Dev(jobs, reads, refs), stride)
    r, u = ctx.last_route(), ctx.last_unlimited()
    ctx.close()
    assert r["sorted"] and r["first_handed_on"] == 0, r
    assert u["stripped"] == len(probs) and u["general"] == 0 and u["steps"] == u["unlimited_steps"], u
    check_against_oracle(rec, mat, exp, flags, [False] * len(probs), "unlimited build R = %d" % R)


# ------------------------------------------------------------------------------------------------ gapped references
def test_gapped_reference_fills_through_the_host_entry(monkeypatch):
    """bbmsa_align_gapped_batch: the gap arrays become '-' runs in wide windows, which the gate sends to fillUnlimited; sorted, those
    that fit the first pass run in the unlimited build.  On and off: the same bytes, and the oracle's scores and strings."""
    probs, glist = _gapped_set(31, 400)
    jobs, reads, refs = M.pack_problems(probs, ALL)
    gaps = np.zeros(len(probs), M.GAPS_DTYPE)
    for k, g in enumerate(glist):
        if g is not None:
            gaps[k]["ngaps"] = len(g)
            gaps[k]["gaps"][:len(g)] = g
    maxR, maxC = 160, 1600
    stride = ((maxR + maxC + 2 + 128 * 24 + 15) // 16) * 16
    om = OracleMSA(maxR, maxC)
    want = []
    for p, g in zip(probs, glist):
        sv, mx = om.fillAndScoreLimited(p[0], p[1], p[2], p[3], p[4], g)
        tb = None if sv is None else om.traceback(p[0], p[1], max(0, p[2]), min(len(p[1]) - 1, p[3]), mx[0], mx[1], mx[2], gapped=g is not None)
        want.append((sv, tb))
    assert sum(sv is not None for sv, _ in want) > 200
    got = {}
    for switch in (1, 0):
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in dict(ROUTES["sorted"], BBMSA_UNLIMITED_LOOP=switch, BBMSA_UNLIMITED_STATS=1, BBMSA_GENERIC_SCRATCH_MB=256).items():
            monkeypatch.setenv(k, str(v))
        ctx = M.MSAContext(maxR, maxC, lanes_per_job=32)
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        res, mat = ctx.align_gapped_batch(jobs, gaps, reads, refs, stride)
        r, u = ctx.last_route(), ctx.last_unlimited()
        ctx.close()
        assert r["sorted"], r
        unl = (res["fill_kind"] == 1) & (res["status"] != M.ST_BAD_SHAPE)
        fits = int((unl & (res["columns"] <= 640)).sum())              # (the default first pass holds 640 columns)
        print("gapped: %d unlimited fills, %d of them in the first pass; %s" % (int(unl.sum()), fits, u))
        assert fits >= 50 and u["stripped"] + u["general"] == int(unl.sum()), (switch, u, fits)
        assert u["stripped"] == (fits if switch else 0), (switch, u, fits)
        for k, (sv, tb) in enumerate(want):
            g = record(res, mat, k)
            assert g["status"] != M.ST_BAD_SHAPE and g["score"] == sv and g["match"] == tb, (switch, k)
        got[switch] = (res.tobytes(), mat.tobytes())
    assert got[1] == got[0]
