"""A launch that is width-sorted AND goes through the band kernel (bbmsa_sort_with_band), record by record against the oracle.

The sort's key is (class, columns / 8 descending) with three classes: unlimited fills, the band kernel's candidates (its own rule,
band_is_candidate: restated here as is_candidate), everything else.  The band kernel walks the candidates' list and appends what it
hands on behind the sorted general list.  Every job must be the oracle's -- result vector, status, iterations, score vector,
traceback string -- whichever kernel finished it, and the bytes must be those of the same launch with the switch off (band kernel
over every job, no sort).  bbmsa_debug_sorted_lists returns the three lists: together a permutation of the job indices, no class
mixed into another, buckets non-increasing inside each list.  The second context's shape (160 x 640, no band kernel) goes through
the same kernels and is held to the same properties.

The oracle's answer for a job comes from an aligner of its own (tests/msa_known.py: the reference's fill reads what the fill before
it left in its matrix; one limited fill of the planted set has a recorded `iterations` deviation, which the parent library shares).

bbmsa_last_counts on such a launch: finished by the band kernel + handed on by it + the sort's general and unlimited lists = jobs."""
import random

import numpy as np
import pytest

from bbmap_amd import msa as M
from tests.msa_check import check_job
from tests.msa_known import fresh_oracle, with_known
from tests.problems import max_quality, mutate, rand_seq
from tests.test_msa_routes_gpu import Dev, record, run

pytestmark = pytest.mark.gpu

ALL = M.FILL_AND_SCORE_LIMITED | M.DO_TRACEBACK
RAW_L = M.FILL_LIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
RAW_U = M.FILL_UNLIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
MAXR, PLAIN_COLS, SECOND_COLS = 160, 256, 640            # 32 lanes x 5 rows; the mapper's two shapes
MAX_SLACK = 2000                                         # BBMSA_NARROW_SLACK's default
ENV = ("BBMSA_NARROW", "BBMSA_SORT_BY_WIDTH", "BBMSA_SORT_WITH_BAND", "BBMSA_LATENCY_JOBS", "BBMSA_LANES_PER_JOB", "BBMSA_UNLIMITED_LOOP",
       "BBMSA_WIDE_UNLIMITED", "BBMSA_NARROW_SLACK")
SORTED_BAND = {"BBMSA_SORT_BY_WIDTH": 1, "BBMSA_SORT_WITH_BAND": 1}
BAND_ONLY = {"BBMSA_SORT_BY_WIDTH": 1}                    # (both on without the switch: the parent's route, band kernel and no sort)

_RNG = random.Random(20)
REF = rand_seq(_RNG, 30000)


def new_ctx(monkeypatch, env, maxC):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return M.MSAContext(MAXR, maxC, lanes_per_job=32)
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def window_of(p, fl):
    read, ref, a, b, ms = p
    if fl & M.CLAMP_WINDOW:
        a, b = max(0, a), min(len(ref) - 1, b)
    return len(read), b - a + 1


def is_candidate(p, fl, maxC):
    """The band kernel's candidate rule (band_is_candidate, msa_common.h)."""
    rows, cols = window_of(p, fl)
    ms, mode = p[4], fl & 7
    if not (16 <= rows <= MAXR and rows <= cols <= maxC) or mode == M.FILL_UNLIMITED_RAW:
        return False
    if mode == M.FILL_LIMITED:
        if ms < 1 or cols + rows < 90 or cols > rows + min(170, rows + 20):
            return False
        ms -= 120
    return max_quality(rows) - ms <= MAX_SLACK


def substitute(rng, rd, n):
    rd = bytearray(rd)
    for _ in range(n):
        i = rng.randrange(len(rd))
        rd[i] = rng.choice([c for c in b"ACGT" if c != rd[i]])
    return bytes(rd)


def centred(st, L, cols):
    a = st - (cols - L) // 2
    return a, a + cols - 1


# ------------------------------------------------------------------------------------------------ the planted set
def _planted():
    """(problems, flags, kinds): kinds[k] in {"band", "leave", "general", "unlimited"} says what the job was planted as."""
    rng = random.Random(7)
    probs, flags, kinds = [], [], []

    def add(rd, ref, a, b, ms, fl, kind):
        probs.append((bytes(rd), ref, a, b, ms))
        flags.append(fl)
        kinds.append(kind)

    def site(L, extra=0):
        return rng.randrange(2000, len(REF) - L - extra - 2000)

    for i in range(150):                                               # candidates that finish in the band
        L = rng.choice([100, 150, 150, 151])
        st = site(L)
        a, b = centred(st, L, L + rng.choice([8, 12, 13, 16]))
        add(substitute(rng, REF[st:st + L], i % 3), REF, a, b, max_quality(L) - rng.choice([0, 300, 900, 1500]), rng.choice([ALL, ALL, RAW_L]), "band")
    for i in range(60):                                                # candidates that must leave it
        L = 150
        st = site(L, 40)
        if i % 3 == 0:                                                 # an N in the window
            a, b = centred(st, L, L + 12)
            x = bytearray(REF[a - 50:b + 51])
            x[50 + rng.randrange(L + 12)] = ord("N")
            add(REF[st:st + L], bytes(x), 50, 50 + L + 11, max_quality(L) - 600, ALL, "leave")
        else:                                                          # a deletion / insertion that carries the path to position 0 or 31
            d = rng.choice([16, 17, 19, 22])
            p = rng.randrange(40, 110)
            if i % 3 == 1:
                rd = REF[st:st + p] + REF[st + p + d:st + L + d]       # deletion: the path moves d diagonals to the right
                a, b = centred(st, L, L + d + 12)
                b = a + L + d + 11
            else:
                rd = REF[st:st + p] + rand_seq(rng, d) + REF[st + p:st + L - d]      # insertion: d diagonals to the left
                a, b = centred(st, L, L + 12)
            add(rd, REF, a, b, max_quality(L) - 1900, RAW_L, "leave")
    widths = [158, 159, 160, 161, 166, 166, 166, 166, 167, 168, 169, 175, 176, 177, 183, 184, 185, 191, 192, 193, 199, 200, 201, 215, 216, 217,
              231, 232, 233, 247, 248, 249, 254, 255, 256, 256, 256]
    for i in range(296):                                               # non-candidates (slack past 2,000): ten and more buckets, many equal widths
        L = rng.choice([150, 150, 149, 100])
        width = widths[i % len(widths)]
        st = site(L, width)
        a = st - rng.randrange(0, max(1, width - L - 8))
        add(mutate(rng, REF[st:st + L + 12], n_prob=0.05)[:L], REF, a, a + width - 1, int(rng.choice([0.3, 0.5, 0.56]) * max_quality(L)),
            rng.choice([ALL, ALL, RAW_L, M.FILL_AND_SCORE_LIMITED]), "general")
    for i in range(95):                                                # unlimited fills: minScore < 1, rows + columns < 90, the raw mode
        if i % 3 == 0:
            L = 150
            width = rng.choice([158, 166, 167, 200, 256])
            st = site(L, width)
            add(mutate(rng, REF[st:st + L + 12], n_prob=0.0)[:L], REF, st - 4, st - 4 + width - 1, rng.choice([0, -5]), ALL, "unlimited")
        elif i % 3 == 1:
            rows, cols = rng.choice([(30, 40), (30, 59), (44, 45), (20, 30)])
            st = site(rows, cols)
            add(REF[st:st + rows], REF, st - 3, st - 3 + cols - 1, int(0.4 * max_quality(rows)), ALL, "unlimited")
        else:
            L = rng.choice([100, 150])
            width = rng.randrange(L + 4, 257)
            st = site(L, width)
            add(mutate(rng, REF[st:st + L + 12], n_prob=0.05)[:L], REF, st - 2, st - 2 + width - 1, 100, RAW_U, "unlimited")
    order = list(range(len(probs)))
    rng.shuffle(order)
    return [probs[k] for k in order], [flags[k] for k in order], [kinds[k] for k in order]


_CACHE = {}


def planted():
    """The set and its oracle answers (once; one limited fill's `iterations` is the recorded kernel count, tests/msa_known.py)."""
    if "set" not in _CACHE:
        probs, flags, kinds = _planted()
        assert len(probs) == 601                                       # odd
        exp = with_known("planted", fresh_oracle(MAXR, PLAIN_COLS, probs, flags))
        _CACHE["set"] = (probs, flags, kinds, exp)
    return _CACHE["set"]


def stride_of(probs):
    return (max(len(p[0]) + (p[3] - p[2] + 1) + 8 for p in probs) + 15) & ~15


def launch(monkeypatch, env, probs, flags, maxC=PLAIN_COLS, lists=False):
    jobs, reads, refs = M.pack_problems(probs, flags)
    ctx = new_ctx(monkeypatch, env, maxC)
    rec, mat = run(ctx, Dev(jobs, reads, refs), stride_of(probs))
    out = {"rec": rec, "mat": mat, "route": ctx.last_route(), "counts": ctx.last_counts()}
    if lists:
        out["lists"] = ctx.debug_sorted_lists(len(probs))
    ctx.close()
    return out


def check_oracle(out, probs, flags, exp, tag):
    for k in range(len(probs)):
        p = probs[k]
        check_job(record(out["rec"], out["mat"], k), exp[k],
                  "%s: job %d rows %d window [%d, %d] minScore %d flags %#x" % (tag, k, len(p[0]), p[2], p[3], p[4], flags[k]))


def check_lists(lists, probs, flags, exp, maxC, band, tag):
    """Permutation, classes, buckets non-increasing.  `band`: the launch ran the band kernel (else no job is a candidate)."""
    n = len(probs)
    allj = np.concatenate([lists["general"], lists["unlimited"], lists["candidates"]])
    assert len(allj) == n and (np.sort(allj) == np.arange(n)).all(), tag + ": the lists are not a permutation of the jobs"
    cand = np.array([band and is_candidate(p, f, maxC) for p, f in zip(probs, flags)])
    unl = np.array([e["fill_kind"] == 1 for e in exp]) & ~cand
    assert cand[lists["candidates"]].all(), tag + ": a non-candidate in the candidates' list"
    assert unl[lists["unlimited"]].all(), tag + ": a limited fill or a candidate in the unlimited list"
    assert not (cand | unl)[lists["general"]].any(), tag + ": a candidate or an unlimited fill in the general list"
    bucket = np.array([max(0, window_of(p, f)[1]) >> 3 for p, f in zip(probs, flags)])
    for name, lst in lists.items():
        assert (np.diff(bucket[lst]) <= 0).all(), "%s: buckets rise inside the %s list: %s" % (tag, name, bucket[lst].tolist())
    return int(cand.sum()), int(unl.sum())


def check_sorted_band(out, probs, flags, exp, tag):
    n = len(probs)
    r, c = out["route"], out["counts"]
    assert r["sorted"] and r["narrow"] and not r["latency"], (tag, r)
    ncand, nunl = check_lists(out["lists"], probs, flags, exp, PLAIN_COLS, True, tag)
    assert c["narrow"] + c["narrow_left"] == ncand, (tag, c, ncand)        # every candidate went one way or the other
    assert c["narrow"] + c["narrow_left"] + c["wave"] == n, (tag, c, n)
    assert r["narrow_finished"] == c["narrow"], (tag, r, c)
    return ncand, nunl


def one_width_set(kind):
    rng = random.Random(3)
    L, width = 150, 166
    probs, flags = [], []
    for i in range(600):
        st = rng.randrange(2000, len(REF) - 2500)
        a, b = centred(st, L, width)
        ms = max_quality(L) - rng.choice([200, 900]) if kind == "candidates" else int(0.5 * max_quality(L))
        probs.append((substitute(rng, REF[st:st + L], i % 4), REF, a, b, ms))
        flags.append(ALL)
    return probs, flags


def second_context_set():
    rng = random.Random(9)
    probs, flags = [], []
    for i in range(700):
        L = rng.choice([100, 150, 150])
        width = rng.choice([170, 199, 200, 201, 320, 321, 400, 639, 640, rng.randrange(170, 641)])
        st = rng.randrange(2000, len(REF) - 3000)
        a = st - rng.randrange(0, 20)
        fl, ms = rng.choice([(ALL, int(0.4 * max_quality(L))), (ALL, int(0.56 * max_quality(L))), (ALL, 0), (RAW_U, 100), (RAW_L, int(0.5 * max_quality(L)))])
        probs.append((mutate(rng, REF[st:st + L + 12], n_prob=0.0)[:L], REF, a, a + width - 1, ms))
        flags.append(fl)
    return probs, flags


# ------------------------------------------------------------------------------------------------ tests
def test_planted_set_sorted_with_band(monkeypatch):
    probs, flags, kinds, exp = planted()
    on = launch(monkeypatch, SORTED_BAND, probs, flags, lists=True)
    check_oracle(on, probs, flags, exp, "sorted with band")
    ncand, nunl = check_sorted_band(on, probs, flags, exp, "sorted with band")
    c = on["counts"]
    print("sorted with band: %d jobs, %d candidates, band finished %d, handed on %d, %d unlimited" % (len(probs), ncand, c["narrow"], c["narrow_left"], nunl))
    assert c["narrow"] > 0 and c["narrow_left"] > 0, c
    assert c["narrow_left"] >= sum(k == "leave" for k in kinds) // 3, c          # (at least every candidate with an N in its window)
    assert nunl >= 90 and len(set(on["lists"]["general"].tolist())) > 250
    widths = {window_of(p, f)[1] >> 3 for p, f, k in zip(probs, flags, kinds) if k == "general"}
    assert len(widths) >= 6
    # the same bytes with the switch off: the band kernel over every job, no sort
    off = launch(monkeypatch, BAND_ONLY, probs, flags)
    assert off["route"]["narrow"] and not off["route"]["sorted"], off["route"]
    assert off["counts"]["narrow"] == c["narrow"] and off["counts"]["narrow_left"] == c["narrow_left"], (off["counts"], c)
    assert on["rec"].tobytes() == off["rec"].tobytes()
    assert on["mat"].tobytes() == off["mat"].tobytes()


@pytest.mark.parametrize("case", ["no_candidate", "only_candidates", "exactly_256", "below_the_floor"])
def test_degenerate_launches(monkeypatch, case):
    probs, flags, kinds, exp = planted()
    if case == "no_candidate":
        keep = [k for k in range(len(probs)) if not is_candidate(probs[k], flags[k], PLAIN_COLS)]
    elif case == "only_candidates":
        keep = [k for k in range(len(probs)) if is_candidate(probs[k], flags[k], PLAIN_COLS)]
        keep = (keep * 2)[:max(len(keep), 257)]                        # (the sort's floor is 256 jobs)
    elif case == "exactly_256":
        keep = list(range(256))
    else:
        keep = list(range(255))
    P, F, E = [probs[k] for k in keep], [flags[k] for k in keep], [exp[k] for k in keep]
    if case == "below_the_floor":                                      # 255 jobs: the band kernel over every job, no sort
        out = launch(monkeypatch, SORTED_BAND, P, F)
        assert out["route"]["narrow"] and not out["route"]["sorted"], out["route"]
        check_oracle(out, P, F, E, case)
        return
    out = launch(monkeypatch, SORTED_BAND, P, F, lists=True)
    check_oracle(out, P, F, E, case)
    ncand, _ = check_sorted_band(out, P, F, E, case)
    if case == "no_candidate":
        assert ncand == 0 and out["counts"]["narrow"] == 0 and out["counts"]["narrow_left"] == 0 and out["counts"]["wave"] == len(P), out["counts"]
    if case == "only_candidates":
        assert ncand == len(P) and out["counts"]["wave"] == 0 and out["counts"]["narrow"] > 0, out["counts"]


@pytest.mark.parametrize("kind", ["general", "candidates"])
def test_600_jobs_of_one_width(monkeypatch, kind):
    """Every job in one bucket: the worst case of the aggregated atomics (one LDS word, one global word per block)."""
    probs, flags = one_width_set(kind)
    exp = fresh_oracle(MAXR, PLAIN_COLS, probs, flags)
    out = launch(monkeypatch, SORTED_BAND, probs, flags, lists=True)
    check_oracle(out, probs, flags, exp, "one width, " + kind)
    ncand, nunl = check_sorted_band(out, probs, flags, exp, "one width, " + kind)
    assert (ncand, nunl) == ((600, 0) if kind == "candidates" else (0, 0))


def test_second_context_shape_sorts_into_the_same_lists(monkeypatch):
    """160 x 640, no band kernel: unlimited fills and the rest, each in descending width, no candidates' list."""
    probs, flags = second_context_set()
    exp = fresh_oracle(MAXR, SECOND_COLS, probs, flags)
    out = launch(monkeypatch, {"BBMSA_NARROW": 0, "BBMSA_SORT_BY_WIDTH": 1}, probs, flags, maxC=SECOND_COLS, lists=True)
    assert out["route"]["sorted"] and not out["route"]["narrow"], out["route"]
    check_oracle(out, probs, flags, exp, "second context")
    ncand, nunl = check_lists(out["lists"], probs, flags, exp, SECOND_COLS, False, "second context")
    assert ncand == 0 and len(out["lists"]["candidates"]) == 0 and nunl > 100 and len(out["lists"]["general"]) > 100
    # with the unlimited build off the unlimited fills are general jobs: one list
    out = launch(monkeypatch, {"BBMSA_NARROW": 0, "BBMSA_SORT_BY_WIDTH": 1, "BBMSA_UNLIMITED_LOOP": 0}, probs, flags, maxC=SECOND_COLS, lists=True)
    assert len(out["lists"]["general"]) == len(probs) and len(out["lists"]["unlimited"]) == 0
    bucket = np.array([window_of(p, f)[1] >> 3 for p, f in zip(probs, flags)])
    assert (np.diff(bucket[out["lists"]["general"]]) <= 0).all()
    check_oracle(out, probs, flags, exp, "second context, one list")
