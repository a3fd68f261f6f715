"""The wavefront kernel's build with both step loops (msa_fill_fast.hip, UNL == 2; bbmsa_set_wide_unlimited) against the oracle.

The launches of the 64-lane geometry hold one job per wavefront, so one build can carry the general loop and the prune-free loop
of the unlimited fills and pick per job (fill_is_limited).  It is compiled for every rows-per-lane value of the wide geometry,
R = 1..10; a context of 64 R rows launches build R.  Both ways into that geometry are run: the latency route (BBMSA_LATENCY_JOBS:
every job of the launch) and the wide pass (windows past the first pass's column buffer).  Limited and unlimited fills alternate
in the list, so consecutive blocks take different loops; rows 1, 2, R, R + 1, 32 R, 64 R - 1, 64 R; windows of rows - 2 columns up
to the context's 704.  With the switch on and off every record is the oracle's and the bytes are the same; with it on
bbmsa_last_unlimited counts every unlimited fill under the prune-free loop, and no limited one.

The oracle's answer for a job comes from an aligner of its own; one limited fill (639 rows, 64 x 10) has a recorded `iterations`
deviation of the general build, which the parent library shares (tests/msa_known.py)."""
import random

import pytest

from bbmap_amd import msa as M
from tests.msa_check import check_job
from tests.msa_known import fresh_oracle, with_known
from tests.problems import max_quality, mutate, rand_seq
from tests.test_msa_routes_gpu import Dev, record, run

pytestmark = pytest.mark.gpu

ALL = M.FILL_AND_SCORE_LIMITED | M.DO_TRACEBACK
RAW_U = M.FILL_UNLIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
RAW_L = M.FILL_LIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
MAXC, FAST = 704, 384
ENV = ("BBMSA_NARROW", "BBMSA_SORT_BY_WIDTH", "BBMSA_SORT_WITH_BAND", "BBMSA_LATENCY_JOBS", "BBMSA_LANES_PER_JOB", "BBMSA_UNLIMITED_LOOP",
       "BBMSA_UNLIMITED_STATS", "BBMSA_WIDE_UNLIMITED", "BBMSA_GENERIC_SCRATCH_MB")
ROUTES = {"latency": {"BBMSA_NARROW": 0, "BBMSA_LATENCY_JOBS": 1 << 20}, "wide_pass": {"BBMSA_NARROW": 0}}


def new_ctx(monkeypatch, env, maxR):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BBMSA_GENERIC_SCRATCH_MB", "512")          # (one wavefront of 640 x 704 scratch matrices is 347 MB)
    monkeypatch.setenv("BBMSA_UNLIMITED_STATS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return M.MSAContext(maxR, MAXC, fast_cols=FAST)
    finally:
        for k in ENV:
            monkeypatch.delenv(k, raising=False)


def jobset(R, route):
    """Limited and unlimited fills in turn.  The wide pass's set holds windows past FAST columns only: every job reaches it."""
    Mx = 64 * R
    rng = random.Random(300 + R)
    ref = bytearray(rand_seq(rng, 4200))
    for i in range(900, 3900, 310):
        ref[i] = ord("N")
    ref = bytes(ref)
    row_counts = sorted({1, 2, R, R + 1, Mx // 2, Mx - 1, Mx})
    probs, flags = [], []
    for rows in row_counts:
        if route == "latency":
            widths = sorted({max(1, rows - 2), rows, rows + 8, min(MAXC, rows + 150), MAXC})
        else:
            widths = sorted({max(FAST + 1, rows - 2), max(FAST + 1, min(MAXC, rows + 9)), MAXC})
        for width in widths:
            for fl, frac in ((RAW_U, 0.5), (RAW_L, 0.5), (ALL, 0.0), (ALL, 0.4), (RAW_L, 0.9), (RAW_U, 0.5)):
                st = rng.randrange(800, 2400)
                rd = mutate(rng, ref[st:st + rows + 12], n_prob=0.05)[:rows] if rows > 20 else ref[st:st + rows]
                left = rng.randrange(0, max(1, min(40, width - len(rd))))
                probs.append((bytes(rd), ref, st - left, st - left + width - 1, int(frac * max_quality(len(rd)))))
                flags.append(fl)
    return probs, flags


@pytest.mark.parametrize("route", ["latency", "wide_pass"])
@pytest.mark.parametrize("R", range(1, 11))
def test_both_loops_build_matches_the_oracle(monkeypatch, R, route):
    maxR = 64 * R
    probs, flags = jobset(R, route)
    exp = with_known("wide_R%d_%s" % (R, route), fresh_oracle(maxR, MAXC, probs, flags))
    n_u = sum(e["fill_kind"] == 1 for e in exp)
    assert n_u >= len(probs) // 3 and len(probs) - n_u >= len(probs) // 4, (n_u, len(probs))
    jobs, reads, refs = M.pack_problems(probs, flags)
    stride = (max(len(p[0]) + (p[3] - p[2] + 1) + 8 for p in probs) + 15) & ~15
    dev = Dev(jobs, reads, refs)
    runs = {}
    for switch in (1, 0):
        ctx = new_ctx(monkeypatch, dict(ROUTES[route], BBMSA_WIDE_UNLIMITED=switch), maxR)
        assert ctx.geometry()["wide_rows_per_lane"] == R
        rec, mat = run(ctx, dev, stride)
        r, u = ctx.last_route(), ctx.last_unlimited()
        ctx.close()
        tag = "R %d route %s switch %d" % (R, route, switch)
        assert r["latency"] == (route == "latency") and r["wide_pass"] and not r["narrow"] and not r["sorted"], (tag, r)
        if route == "wide_pass":
            assert r["first_handed_on"] == len(probs), (tag, r)         # every window is past the first pass's buffer
        assert r["wide_handed_on"] == 0, (tag, r)
        for k, p in enumerate(probs):
            check_job(record(rec, mat, k), exp[k], "%s: job %d rows %d window [%d, %d] minScore %d flags %#x" % (tag, k, len(p[0]), p[2], p[3], p[4], flags[k]))
        assert (u["stripped"], u["general"]) == ((n_u, 0) if switch else (0, n_u)), (tag, u, n_u)
        runs[switch] = (rec, mat)
    assert runs[1][0].tobytes() == runs[0][0].tobytes()
    assert runs[1][1].tobytes() == runs[0][1].tobytes()
