"""Every launch route of the DP (bbmsa_align_impl) against the oracle, job by job.

A launch takes one of several routes through the kernels depending on the context's switches and on the launch size: the
narrow-window kernel in front of the first pass, the first pass alone, the width-sorted first pass, the latency route (no first
pass: the wide pass takes every job), and the _indirect entries whose job count is read on the device.  One seeded job set with
every kind of job mixed in one launch (narrow-fit windows, ordinary and wide windows, windows clamped at both ends, gap symbols in
the reference with and without BBMSA_TRACE_KEEP_GAPS, N and lower-case bases, null fills, the raw modes, 1 x 1 jobs, jobs
outside the context's shape, long deletions that break a band) goes through each route; every record must be the oracle's, and
the raw records of all routes must be the same bytes.  bbmsa_last_route shows that the route meant really ran.

Routes are picked with the environment switches bbmsa_create reads (BBMSA_NARROW, BBMSA_SORT_BY_WIDTH, BBMSA_LATENCY_JOBS)."""
import random

import numpy as np
import pytest

from bbmap_amd import msa as M
from oracle.oracle import OracleMSA
from tests.msa_check import check_job, oracle_align
from tests.problems import max_quality, mutate, rand_seq

pytestmark = pytest.mark.gpu

KEEP_GAPS = 1 << 7
ALL = M.FILL_AND_SCORE_LIMITED | M.DO_TRACEBACK
MAXR, MAXC, FAST = 160, 1024, 320          # 160 rows keep 16 lanes x 10 rows; windows past 320 columns take the wide pass
UNBANDED, BANDED = (0, 0.0), (40, 0.18)
N_JOBS = 5200
SENT = 0xA5                                # sentinel byte of untouched results / match slots
ROUTE_ENV = ("BBMSA_NARROW", "BBMSA_SORT_BY_WIDTH", "BBMSA_LATENCY_JOBS", "BBMSA_LANES_PER_JOB")


# ------------------------------------------------------------------------------------------------ job set
def _jobset(seed, n):
    """(problems, flags, bad): problems as pack_problems takes them; bad[k] = the job lies outside MAXR x MAXC (BAD_SHAPE)."""
    rng = random.Random(seed)
    ref = bytearray(rand_seq(rng, 40000))
    for _ in range(40):
        ref[rng.randrange(len(ref))] = ord("N")
    ref = bytes(ref)
    short = rand_seq(rng, 300)                                         # windows clamped at both ends
    pieces, pos = [], 0                                                # a gapped reference: runs of '-' every ~500 bases
    while pos < 20000:
        step = rng.randrange(300, 700)
        pieces.append(ref[pos:pos + step])
        pieces.append(b"-" * rng.randint(1, 4))
        pos += step
    gref = b"".join(pieces)
    gap_at = [i for i in range(200, len(gref) - 400) if gref[i] == ord("-") and gref[i - 1] != ord("-")]
    flag_mix = [ALL, ALL, M.FILL_AND_SCORE_LIMITED, M.FILL_LIMITED | M.CLAMP_WINDOW | M.DO_TRACEBACK, ALL | M.NO_ITERATIONS,
                M.FILL_LIMITED | M.CLAMP_WINDOW]
    probs, flags, bad = [], [], []

    def add(rd, G, a, b, ms, fl, is_bad=False):
        probs.append((bytes(rd), G, a, b, ms))
        flags.append(fl)
        bad.append(is_bad)

    def site(L, extra=0):
        return rng.randrange(500, len(ref) - L - extra - 500)

    for i in range(n):
        kind = i % 17
        L = rng.choice([100, 150, 150])
        if kind <= 2:                                                  # narrow-fit: read + 8 columns, high minScore
            st = site(L)
            rd = bytearray(ref[st:st + L])
            for _ in range(rng.randint(0, 2)):
                rd[rng.randrange(10, L - 10)] = rng.choice(b"ACGT")
            add(rd, ref, st - 4, st + L + 3, max_quality(L) - rng.randrange(150, 1800), rng.choice([ALL, ALL, M.FILL_AND_SCORE_LIMITED]))
        elif kind <= 7:                                                # ordinary (158..290) and wide (330..1000) windows
            width = rng.randrange(158, 291) if kind <= 6 else rng.randrange(330, 1001)
            st = site(L, width)
            rd = mutate(rng, ref[st:st + L + 12], n_prob=0.0)[:L]
            a = st - rng.randrange(0, max(1, width - L))
            add(rd, ref, a, a + width - 1, int(rng.choice([0.3, 0.5, 0.56, 0.7]) * max_quality(len(rd))), rng.choice(flag_mix))
        elif kind == 8:                                                # clamped at both ends
            rd = mutate(rng, short[60:220], n_prob=0.0)[:150]
            add(rd, short, -rng.randrange(1, 40), len(short) - 1 + rng.randrange(1, 40), int(0.4 * max_quality(len(rd))),
                rng.choice([ALL, M.FILL_LIMITED | M.CLAMP_WINDOW | M.DO_TRACEBACK]))
        elif kind == 9:                                                # '-' symbols in the window, with and without KEEP_GAPS
            g = rng.choice(gap_at)
            st = g - rng.randrange(30, L - 30)
            seg = gref[st:st + L + 8]
            rd = seg.replace(b"-", b"")[:L]
            add(rd, gref, st - 4, st + L + 12, int(0.3 * max_quality(len(rd))), rng.choice([ALL, ALL | KEEP_GAPS]))
        elif kind == 10:                                               # N and lower-case bases in the read
            st = site(L, 20)
            rd = bytearray(ref[st:st + L])
            for _ in range(rng.randint(1, 4)):
                rd[rng.randrange(L)] = ord("N")
            p, q = rng.randrange(0, L - 20), rng.randint(3, 20)
            rd[p:p + q] = bytes(rd[p:p + q]).lower()
            add(rd, ref, st - 8, st + L + 7, int(0.3 * max_quality(L)), rng.choice(flag_mix))
        elif kind == 11:                                               # null fill: minScore out of reach
            st = site(L, 20)
            rd = ref[st:st + L]
            add(rd, ref, st - 4, st + L + rng.randrange(3, 40), max_quality(L) + 121,
                rng.choice([ALL, M.FILL_LIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK]))
        elif kind in (12, 13):                                         # raw limited / raw unlimited
            width = rng.randrange(158, 400)
            st = site(L, width)
            rd = mutate(rng, ref[st:st + L + 12], n_prob=0.05)[:L]
            a = st - rng.randrange(0, 20)
            add(rd, ref, a, a + width - 1, int(0.5 * max_quality(len(rd))),
                (M.FILL_LIMITED_RAW if kind == 12 else M.FILL_UNLIMITED_RAW) | M.DO_SCORE | M.DO_TRACEBACK)
        elif kind == 14:                                               # 1 x 1
            st = site(1)
            add(ref[st:st + 1], ref, st, st, 0,
                rng.choice([ALL, M.FILL_LIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK, M.FILL_UNLIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK]))
        elif kind == 15:                                               # BAD_SHAPE: rows > maxRows, or columns > maxColumns unclamped
            if rng.random() < 0.5:
                st = site(MAXR + 10, 30)
                add(ref[st:st + MAXR + 10], ref, st - 4, st + MAXR + 20, 100, ALL, True)
            else:
                st = site(L, MAXC + 100)
                add(ref[st:st + L], ref, st, st + MAXC + rng.randrange(1, 80), 100, M.FILL_LIMITED | M.DO_SCORE | M.DO_TRACEBACK, True)
        else:                                                          # long deletion: rows with holes in a band
            d = rng.randrange(15, 60)
            p = rng.randrange(30, L - 30)
            st = site(L, d + 20)
            rd = ref[st:st + p] + ref[st + p + d:st + L + d]
            add(rd, ref, st - 6, st + L + d + 5, int(0.3 * max_quality(L)), rng.choice([ALL, ALL, M.FILL_LIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK]))
    order = list(range(n))
    rng.shuffle(order)
    return [probs[k] for k in order], [flags[k] for k in order], [bad[k] for k in order]


_CACHE = {}


def jobset():
    if "set" not in _CACHE:
        probs, flags, bad = _jobset(2025, N_JOBS)
        jobs, reads, refs = M.pack_problems(probs, flags)
        _CACHE["set"] = (probs, flags, bad, jobs, reads, refs)
    return _CACHE["set"]


def oracle(band, scheme="11ts"):
    """The oracle's answer for every job of the set, once per band (None for BAD_SHAPE jobs: nothing to compute)."""
    key = ("oracle", band)
    if key not in _CACHE:
        probs, flags, bad = jobset()[:3]
        om = OracleMSA(MAXR, MAXC, band[0], band[1])
        _CACHE[key] = [None if b else oracle_align(om, p[0], p[1], p[2], p[3], p[4], f) for p, f, b in zip(probs, flags, bad)]
    return _CACHE[key]


def match_need(e, fl, kept):
    """Bytes the slot needs for this job's string: expanded, or as the kernels wrote it with KEEP_GAPS (`kept`)."""
    if e is None or e["match"] is None:
        return 0
    return len(kept) if fl & KEEP_GAPS else len(e["match"])


def full_stride():
    probs = jobset()[0]
    s = max(len(p[0]) + (p[3] - p[2] + 1) + 8 + 127 * bytes(p[1][max(0, p[2]):max(0, p[3] + 1)]).count(b"-") for p in probs)
    return (s + 15) & ~15


# ------------------------------------------------------------------------------------------------ device runs
def _torch():
    import torch
    return torch


class Dev:
    """Device copies of a job set: `cap` job records (the tail beyond n repeats the set's first jobs: valid jobs, so a kernel that
    ran past its count would compute them and write their records, never read garbage)."""

    def __init__(self, jobs, reads, refs, cap=None, gaps=None):
        torch = _torch()
        n = len(jobs)
        cap = n if cap is None else cap
        idx = np.arange(cap) % n
        self.n, self.cap = n, cap
        self.jobs = torch.from_numpy(np.ascontiguousarray(jobs[idx]).view(np.uint8).copy()).cuda()
        self.gaps = None if gaps is None else torch.from_numpy(np.ascontiguousarray(gaps[idx]).view(np.uint8).copy()).cuda()
        self.reads = torch.from_numpy(np.ascontiguousarray(reads).copy()).cuda()
        self.refs = torch.from_numpy(np.ascontiguousarray(refs).copy()).cuda()


def run(ctx, dev, stride, n=None, count=None, res=None, match=None):
    """One launch.  count=None: the direct entry over n jobs; otherwise the _indirect entry with capacity dev.cap and the
    count written to device memory by a torch op on the launch's stream right in front of the call.  Returns (records, match)."""
    torch = _torch()
    cap = dev.cap
    if res is None:
        res = torch.full((cap * M.RESULT_DTYPE.itemsize,), SENT, dtype=torch.uint8, device="cuda")
        match = torch.full((cap * stride,), SENT, dtype=torch.uint8, device="cuda") if stride else None
    torch.cuda.synchronize()
    mp = match.data_ptr() if match is not None else 0
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        if count is None:
            nn = dev.n if n is None else n
            if dev.gaps is None:
                ctx.align_batch_device(nn, dev.jobs.data_ptr(), dev.reads.data_ptr(), dev.refs.data_ptr(), res.data_ptr(), mp, stride,
                                       stream=s.cuda_stream)
            else:
                ctx.align_gapped_batch_device(nn, dev.jobs.data_ptr(), dev.gaps.data_ptr(), dev.reads.data_ptr(), dev.refs.data_ptr(),
                                              res.data_ptr(), mp, stride, stream=s.cuda_stream)
        else:
            cnt = torch.empty(1, dtype=torch.int64, device="cuda")
            cnt.fill_(count)                                           # (little-endian: the low 4 bytes are the uint32 count)
            if dev.gaps is None:
                ctx.align_batch_device_indirect(cnt.data_ptr(), cap, dev.jobs.data_ptr(), dev.reads.data_ptr(), dev.refs.data_ptr(),
                                                res.data_ptr(), mp, stride, stream=s.cuda_stream)
            else:
                ctx.align_gapped_batch_device_indirect(cnt.data_ptr(), cap, dev.jobs.data_ptr(), dev.gaps.data_ptr(), dev.reads.data_ptr(),
                                                       dev.refs.data_ptr(), res.data_ptr(), mp, stride, stream=s.cuda_stream)
    s.synchronize()
    rec = res.cpu().numpy().view(M.RESULT_DTYPE)
    mat = match.cpu().numpy().reshape(cap, stride) if match is not None else None
    return rec, mat


def make_ctx(monkeypatch, env, lanes=0, band=UNBANDED, scheme=M.SCHEME_11TS, maxRows=MAXR, maxColumns=MAXC, fast_cols=FAST):
    for k in ROUTE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return M.MSAContext(maxRows, maxColumns, band[0], band[1], lanes_per_job=lanes, fast_cols=fast_cols, scheme=scheme)
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def record(rec, mat, k):
    """One raw record in the shape MultiStateAligner11ts.align returns (match: the string as written, '-' kept)."""
    r = rec[k]
    ml = int(r["match_len"])
    return {"result": r["result"].tolist(), "status": int(r["status"]), "iterations": int(r["iterations"]),
            "score": None if r["score_len"] == 0 else r["score"][:r["score_len"]].tolist(),
            "match": mat[k, :ml].tobytes() if (mat is not None and ml > 0) else None, "fill_kind": int(r["fill_kind"]),
            "match_len": ml}


def check_against_oracle(rec, mat, exp, flags, bad, tag, jobs=None):
    """Every job of `jobs` (default: all) field by field against the oracle; KEEP_GAPS strings are expanded as the caller
    would; the bytes of a slot past its string stay sentinel."""
    stride = mat.shape[1] if mat is not None else 0
    for k in (range(len(exp)) if jobs is None else jobs):
        g = record(rec, mat, k)
        ctx = "%s: job %d flags %#x" % (tag, k, flags[k])
        if bad[k]:
            assert g["status"] == M.ST_BAD_SHAPE and g["match_len"] == 0, ctx
            continue
        if g["match"] is not None and flags[k] & KEEP_GAPS:
            g["match"] = g["match"].replace(b"-", b"D" * 128)
        check_job(g, exp[k], ctx)
        if mat is not None:
            assert (mat[k, max(0, g["match_len"]):stride] == SENT).all(), ctx + ": bytes past the string were written"


ROUTES = {                                   # name: (environment, what bbmsa_last_route must show)
    "narrow": ({}, "narrow"),
    "first_pass": ({"BBMSA_NARROW": 0}, "first"),
    "sorted": ({"BBMSA_NARROW": 0, "BBMSA_SORT_BY_WIDTH": 1}, "sorted"),
    "latency": ({"BBMSA_NARROW": 0, "BBMSA_LATENCY_JOBS": N_JOBS}, "latency"),
    "latency_n_minus_1": ({"BBMSA_NARROW": 0, "BBMSA_LATENCY_JOBS": N_JOBS - 1}, "first"),
}


def assert_route(r, want, banded, indirect=False):
    assert r["indirect"] == indirect, r
    assert r["wide_pass"], r
    if want == "narrow" and not banded:                 # (a banded context has no narrow kernel: the first pass takes all)
        assert r["narrow"] and r["narrow_finished"] > 0 and not r["sorted"] and not r["latency"], r
    elif want == "sorted":
        assert r["sorted"] and not r["narrow"] and not r["latency"] and r["first_handed_on"] > 0, r
    elif want == "latency":
        assert r["latency"] and not r["narrow"] and not r["sorted"] and r["first_handed_on"] == 0, r
    else:
        assert not r["narrow"] and not r["sorted"] and not r["latency"] and r["first_handed_on"] > 0, r
    if banded:
        assert r["wide_handed_on"] > 0, r                # rows with holes: the generic kernel ran


# ------------------------------------------------------------------------------------------------ the route matrix
@pytest.mark.parametrize("band", [UNBANDED, BANDED], ids=["unbanded", "banded"])
@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_every_route_matches_the_oracle(monkeypatch, lanes, band):
    probs, flags, bad, jobs, reads, refs = jobset()
    exp = oracle(band)
    assert sum(bad) > 100 and sum(e is not None and e["status"] == M.ST_NULL for e in exp) > 100
    stride = full_stride()
    dev = Dev(jobs, reads, refs)
    first = None
    for name, (env, want) in ROUTES.items():
        ctx = make_ctx(monkeypatch, env, lanes, band)
        rec, mat = run(ctx, dev, stride)
        r = ctx.last_route()
        ctx.close()
        tag = "lanes %d band %s route %s" % (lanes, band, name)
        assert_route(r, want, band != UNBANDED)
        check_against_oracle(rec, mat, exp, flags, bad, tag)
        if first is None:
            first = (rec.copy(), mat.copy())
        else:                                                # every route: the same bytes, `columns` included
            assert rec.tobytes() == first[0].tobytes(), tag
            assert mat.tobytes() == first[1].tobytes(), tag


@pytest.mark.parametrize("lanes", [16, 64])
def test_launch_sizes_at_block_wave_sort_and_latency_edges(monkeypatch, lanes):
    """1, 63, 64, 65 (waves), 255, 256, 257 (the sort's floor), 4,097 (latency threshold 4,096 + 1) jobs on every route."""
    probs, flags, bad, jobs, reads, refs = jobset()
    exp = oracle(UNBANDED)
    stride = full_stride()
    dev = Dev(jobs, reads, refs)
    envs = {"narrow": {}, "first_pass": {"BBMSA_NARROW": 0}, "sorted": {"BBMSA_NARROW": 0, "BBMSA_SORT_BY_WIDTH": 1},
            "latency": {"BBMSA_NARROW": 0, "BBMSA_LATENCY_JOBS": 4096}}
    for name, env in envs.items():
        ctx = make_ctx(monkeypatch, env, lanes)
        for n in (1, 63, 64, 65, 255, 256, 257, 4097):
            rec, mat = run(ctx, dev, stride, n=n)
            r = ctx.last_route()
            tag = "lanes %d route %s n %d" % (lanes, name, n)
            assert r["narrow"] == (name == "narrow"), (tag, r)
            assert r["sorted"] == (name == "sorted" and n >= 256), (tag, r)
            assert r["latency"] == (name == "latency" and n <= 4096), (tag, r)
            check_against_oracle(rec, mat, exp, flags, bad, tag, jobs=range(n))
            assert (rec[n:].view(np.uint8) == SENT).all() and (mat[n:] == SENT).all(), tag + ": records past n_jobs written"
        ctx.close()


# ------------------------------------------------------------------------------------------------ indirect job counts
def _indirect_cases(ctx, dev, stride, direct_rec, direct_mat, tag, route_check=None):
    n, cap = dev.n, dev.cap
    for count in (n, 0, cap + 1000):
        rec, mat = run(ctx, dev, stride, count=count)
        r = ctx.last_route()
        assert r["indirect"] and not r["latency"] and not r["sorted"], (tag, count, r)
        if route_check:
            route_check(r, count)
        m = min(count, cap)
        idx = np.arange(m) % n                                 # (tail jobs repeat the set's first ones)
        assert rec[:m].tobytes() == direct_rec[idx].tobytes(), (tag, count)
        assert mat[:m].tobytes() == direct_mat[idx].tobytes(), (tag, count)
        assert (rec[m:].view(np.uint8) == SENT).all() and (mat[m:] == SENT).all(), (tag, count, "records past the count written")
    # a second launch on the same buffers with a smaller count: only its own records change
    torch = _torch()
    res = torch.full((cap * M.RESULT_DTYPE.itemsize,), SENT, dtype=torch.uint8, device="cuda")
    match = torch.full((cap * stride,), SENT, dtype=torch.uint8, device="cuda")
    run(ctx, dev, stride, count=n, res=res, match=match)
    res.fill_(SENT)
    match.fill_(SENT)
    small = n // 3 + 1
    rec, mat = run(ctx, dev, stride, count=small, res=res, match=match)
    assert rec[:small].tobytes() == direct_rec[:small].tobytes() and mat[:small].tobytes() == direct_mat[:small].tobytes(), tag
    assert (rec[small:].view(np.uint8) == SENT).all() and (mat[small:] == SENT).all(), tag + ": second launch wrote past its count"


@pytest.mark.parametrize("setting", ["narrow", "first_pass_sort_latency_set", "banded"])
def test_indirect_count_matches_the_direct_entry(monkeypatch, setting):
    """bbmsa_align_batch_device_indirect: min(*count, max_jobs) jobs run and nothing past them is written.  A device count
    disables the width sort and the latency route even where the context asks for them."""
    probs, flags, bad, jobs, reads, refs = jobset()
    band = BANDED if setting == "banded" else UNBANDED
    env = {"BBMSA_NARROW": 0, "BBMSA_SORT_BY_WIDTH": 1, "BBMSA_LATENCY_JOBS": 1 << 20} if setting.startswith("first") else {}
    stride = full_stride()
    ctx = make_ctx(monkeypatch, env, 32, band)
    direct_rec, direct_mat = run(ctx, Dev(jobs, reads, refs), stride)
    check_against_oracle(direct_rec, direct_mat, oracle(band), flags, bad, "direct " + setting)
    dev = Dev(jobs, reads, refs, cap=len(jobs) + 37)

    def route_check(r, count):
        assert r["narrow"] == (setting == "narrow"), r
        if setting == "narrow" and count:
            assert r["narrow_finished"] > 0, r
        if setting == "banded" and count:
            assert r["wide_handed_on"] > 0, r
    _indirect_cases(ctx, dev, stride, direct_rec, direct_mat, setting, route_check)
    ctx.close()


def _gapped_set(seed, n):
    """Ungapped jobs of the main set mixed with gap-array jobs (long deletions; BBIndex.makeGapArray's shape)."""
    rng = random.Random(seed)
    ref = rand_seq(rng, 8000)
    probs, gaps = [], []
    for i in range(n):
        L = rng.choice([100, 150])
        st = rng.randrange(200, 3000)
        cut = rng.randrange(30, L - 30)
        dl = rng.choice([300, 700, 1500])
        rd = bytearray(ref[st:st + cut] + ref[st + cut + dl:st + dl + L])
        for _ in range(rng.randint(0, 3)):
            rd[rng.randrange(L)] = rng.choice(b"ACGT")
        stop = st + dl + L - 1
        g = [st, st + cut - 1 + rng.randint(0, 3), st + cut + dl - rng.randint(0, 3), stop] if i % 3 else None
        if g is None:
            rd = ref[st:st + L]
            stop = st + L + rng.randrange(3, 60)
        probs.append((bytes(rd), ref, st - 4, stop + 4, int(rng.choice([0.3, 0.5]) * max_quality(len(rd)))))
        gaps.append(g)
    return probs, gaps


@pytest.mark.parametrize("setting", ["narrow", "first_pass", "banded"])
def test_gapped_indirect_count_matches_the_direct_entry(monkeypatch, setting):
    probs, glist = _gapped_set(31, 700)
    jobs, reads, refs = M.pack_problems(probs, ALL)
    gaps = np.zeros(len(probs), M.GAPS_DTYPE)
    for k, g in enumerate(glist):
        if g is not None:
            gaps[k]["ngaps"] = len(g)
            gaps[k]["gaps"][:len(g)] = g
    band = BANDED if setting == "banded" else UNBANDED
    maxR, maxC = 160, 1600
    stride = ((maxR + maxC + 2 + 128 * 24 + 15) // 16) * 16
    ctx = make_ctx(monkeypatch, {"BBMSA_NARROW": 0} if setting == "first_pass" else {}, 32, band, maxRows=maxR, maxColumns=maxC)
    direct_rec, direct_mat = run(ctx, Dev(jobs, reads, refs, gaps=gaps), stride)
    om = OracleMSA(maxR, maxC, band[0], band[1])
    nonnull = 0
    for k, (p, g) in enumerate(zip(probs, glist)):
        sv, mx = om.fillAndScoreLimited(p[0], p[1], p[2], p[3], p[4], g)
        got = record(direct_rec, direct_mat, k)
        assert got["status"] != M.ST_BAD_SHAPE and got["score"] == sv, (setting, k, got, sv)
        if sv is not None:
            nonnull += 1
            tb = om.traceback(p[0], p[1], max(0, p[2]), min(len(p[1]) - 1, p[3]), mx[0], mx[1], mx[2], gapped=g is not None)
            assert got["match"] == tb, (setting, k)
    assert nonnull > 300
    _indirect_cases(ctx, Dev(jobs, reads, refs, cap=len(jobs) + 37, gaps=gaps), stride, direct_rec, direct_mat, "gapped " + setting)
    ctx.close()


def _pacbio_set(seed, n):
    rng = random.Random(seed)
    ref = rand_seq(rng, 6000)
    probs = []
    for i in range(n):
        L = rng.choice([120, 400, 700, 1000])
        st = rng.randrange(300, 4500)
        rd = bytearray(ref[st:st + L])
        for pos in range(rng.randrange(10, 60), L - 20, rng.randrange(40, 90)):
            if rng.random() < 0.5:
                del rd[pos]
            else:
                rd[pos] = rng.choice(b"ACGT")
        width = min(1400, len(rd) + rng.choice([16, 40, 200, 380]))
        a = st - 8
        probs.append((bytes(rd), ref, a, a + width - 1, int(rng.choice([0.3, 0.5]) * (90 + 100 * (len(rd) - 1)))))
    return probs


@pytest.mark.parametrize("band", [UNBANDED, BANDED], ids=["strip", "banded_generic"])
def test_pacbio_indirect_count_matches_the_direct_entry(monkeypatch, band):
    """The 9PacBio scheme: the strip kernel in its sequential form (a device count never takes the pipelined one) and, banded,
    the generic kernel, with the count on the device."""
    monkeypatch.setenv("BBMSA_GENERIC_SCRATCH_MB", "4096")
    probs = _pacbio_set(7, 40)
    jobs, reads, refs = M.pack_problems(probs, ALL)
    maxR, maxC = 1000, 1400
    stride = ((maxR + maxC + 8 + 15) // 16) * 16
    ctx = make_ctx(monkeypatch, {}, 0, band, scheme=M.SCHEME_9PACBIO, maxRows=maxR, maxColumns=maxC, fast_cols=0)
    direct_rec, direct_mat = run(ctx, Dev(jobs, reads, refs), stride)
    om = OracleMSA(maxR, maxC, band[0], band[1], scheme="9pacbio")
    for k, p in enumerate(probs):
        exp = oracle_align(om, p[0], p[1], p[2], p[3], p[4], ALL)
        check_job(record(direct_rec, direct_mat, k), exp, "pacbio %s job %d" % (band, k))

    def route_check(r, count):
        assert not r["narrow"] and not r["wide_pass"], r
        if band != UNBANDED and count:
            assert r["first_handed_on"] > 0, r           # banded fills: the strip kernel hands them to the generic kernel
    _indirect_cases(ctx, Dev(jobs, reads, refs, cap=len(jobs) + 37), stride, direct_rec, direct_mat, "pacbio %s" % (band,), route_check)
    ctx.close()


# ------------------------------------------------------------------------------------------------ slots too small
@pytest.mark.parametrize("route", ["narrow", "first_pass", "sorted", "latency", "banded"])
def test_match_slots_shorter_than_some_tracebacks(monkeypatch, route):
    """match_len == -1 exactly where the string needs more than the stride; a job without DO_TRACEBACK leaves its slot as it was.
    (Not checked: what a slot reported -1 holds -- no route promises anything about it.)"""
    probs, flags, bad, jobs, reads, refs = jobset()
    band = BANDED if route == "banded" else UNBANDED
    exp = oracle(band)
    # the strings as the kernels write them (KEEP_GAPS: compact), from a run with room for all of them
    ctx = make_ctx(monkeypatch, {}, 32, band)
    full_rec, full_mat = run(ctx, Dev(jobs, reads, refs), full_stride())
    ctx.close()
    flags2 = [f & ~M.DO_TRACEBACK if k % 2 else f for k, f in enumerate(flags)]
    jobs2 = jobs.copy()
    jobs2["flags"] = flags2
    need = [match_need(exp[k], flags[k], record(full_rec, full_mat, k)["match"]) for k in range(len(flags))]
    traced = sorted(need[k] for k in range(0, len(need), 2) if need[k] > 0)
    stride = traced[len(traced) * 3 // 5] & ~3
    env = {"narrow": {}, "banded": {}, "first_pass": {"BBMSA_NARROW": 0}, "sorted": {"BBMSA_NARROW": 0, "BBMSA_SORT_BY_WIDTH": 1},
           "latency": {"BBMSA_NARROW": 0, "BBMSA_LATENCY_JOBS": N_JOBS}}[route]
    ctx = make_ctx(monkeypatch, env, 32, band)
    rec, mat = run(ctx, Dev(jobs2, reads, refs), stride)
    r = ctx.last_route()
    ctx.close()
    assert_route(r, {"banded": "first", "first_pass": "first"}.get(route, route), band != UNBANDED)
    over = 0
    for k in range(len(flags)):
        tag = "%s job %d need %d stride %d" % (route, k, need[k], stride)
        ml = int(rec[k]["match_len"])
        if k % 2 or need[k] == 0:
            assert ml == 0 and (mat[k] == SENT).all(), tag
            continue
        if need[k] > stride:
            assert ml == -1, tag
            over += 1
        else:
            assert ml == need[k], tag
            assert mat[k, :ml].tobytes() == full_mat[k, :ml].tobytes(), tag
            assert (mat[k, ml:] == SENT).all(), tag
        # every other field is what it is with room for the string
        a, b = rec[k].copy(), full_rec[k].copy()
        a["match_len"] = b["match_len"] = 0
        assert a.tobytes() == b.tobytes(), tag
    assert over > 100


# ------------------------------------------------------------------------------------------------ context reuse
@pytest.mark.parametrize("route", ["narrow", "sorted_latency"])
def test_context_reuse_across_sizes_equals_fresh_contexts(monkeypatch, route):
    """5,000 -> 3 -> 20,000 -> 300 jobs on one context: the list buffers grow (slowCap / fastCap), and with the sort and a latency
    threshold of 4,096 the route changes from launch to launch; every launch equals a fresh context's."""
    probs, flags, bad = _jobset(77, 20000)
    jobs, reads, refs = M.pack_problems(probs, flags)
    stride = (max(len(p[0]) + (p[3] - p[2] + 1) + 8 + 127 * bytes(p[1][max(0, p[2]):max(0, p[3] + 1)]).count(b"-") for p in probs) + 15) & ~15
    env = {} if route == "narrow" else {"BBMSA_NARROW": 0, "BBMSA_SORT_BY_WIDTH": 1, "BBMSA_LATENCY_JOBS": 4096}
    dev = Dev(jobs, reads, refs)
    ctx = make_ctx(monkeypatch, env, 32)
    exp_om = OracleMSA(MAXR, MAXC)
    for n in (5000, 3, 20000, 300):
        rec, mat = run(ctx, dev, stride, n=n)
        r = ctx.last_route()
        if route != "narrow":
            assert r["sorted"] == (n > 4096) and r["latency"] == (n <= 4096), (n, r)
        else:
            assert r["narrow"], (n, r)
        fresh = make_ctx(monkeypatch, env, 32)
        frec, fmat = run(fresh, dev, stride, n=n)
        fresh.close()
        assert rec[:n].tobytes() == frec[:n].tobytes() and mat[:n].tobytes() == fmat[:n].tobytes(), (route, n)
        assert (rec[n:].view(np.uint8) == SENT).all(), (route, n)
        for k in range(0, n, 97):                                  # and a sample against the oracle
            if not bad[k]:
                g = record(rec, mat, k)
                if g["match"] is not None and flags[k] & KEEP_GAPS:
                    g["match"] = g["match"].replace(b"-", b"D" * 128)
                check_job(g, oracle_align(exp_om, *probs[k], flags[k]), "reuse %s n %d job %d" % (route, n, k))
    ctx.close()
