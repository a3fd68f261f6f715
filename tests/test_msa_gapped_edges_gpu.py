"""The gapped-reference path of the DP against the oracle, field by field and byte by byte, at its segment, buffer and route edges.

A job with a gap array runs through three pieces: make_gref_kernel builds the gapped reference and derives an ordinary job that
points at it (bbmap_amd/csrc/msa_gapped.hip), a fill kernel runs it -- each has its own copy of the gapped tail, the pad-hint line
`bW = INTERNAL_GAPPED ? ref_len : b` and the '-' -> 128 x 'D' expansion --, and gref_post_kernel translates score[1..2] back.  The
sets of tests/gapped_problems.py (tests/test_oracle_gapped.py shows from the oracle that they hold what they claim) go through
every route that can carry a derived job; the route is forced with the switches bbmsa_create reads and proved by
bbmsa_last_route / bbmsa_last_counts.  Every launch here holds gap-array jobs only (the two plain jobs of the `refused` set
aside), so a kernel the counters show at work took gapped jobs.

Which kernels a derived job can reach, from the code:
  * the first pass / the wide pass of the wavefront kernel (msa_fill_fast.hip): every derived job whose gapped reference has at
    least rows - 2 columns; past fast_cols (320 here) columns the wide pass -- the 8-block and the 16 kb jobs;
  * the generic kernel (msa_fill_generic.hip): in a banded context the jobs whose rows have holes, and in any context a gapped
    reference with fewer than rows - 2 columns (the `overhang:deep` jobs).  A window "wider than the wide pass takes" cannot be
    arranged: where the wide pass exists its buffer is maxColumns wide, and make_gref_kernel refuses what exceeds maxColumns.
    The code has one more way -- setup_wide_pass (msa_host.hip) sets up no wide pass when its LDS need passes 160 KB, and
    bbmsa_align_impl then gives the first pass's hand-overs, wide derived jobs included, straight to the generic kernel -- but
    bbmsa_create takes at most 640 x 4,096, where that need is about 48 KB, so no context a caller can make gets there;
  * the band kernel (msa_fill_band.hip) does receive derived jobs: they are FILL_LIMITED jobs, and band_is_candidate (msa_common.h)
    takes one whose gapped reference has at most rows + min(170, rows + 20) columns and whose minScore lies within 2,000 of the
    best score -- one gap with gap % 128 + symbols + padding <= 41 (the `modes:*:tight` jobs).  A read that crosses the gap
    moves over at least 129 diagonals, more than the band's 32, so the band kernel tries such a job and hands it on; the test
    asserts that it tried exactly the jobs the rule names (finished + handed on), not that it finished one;
  * 9PacBio: the strip kernel (msa_fill_strip.hip) in its sequential and its pipelined form (plan_route picks the form from the
    job count and BBMSA_STRIP_PIPE_JOBS; no counter tells them apart, tests/test_msa_route_cpu.py holds the rule); it takes
    windows narrower than the read itself, so the generic kernel sees derived jobs in a banded context only.

Set x route: the seven launch sets (gap_steps, lane_sweep, blocks, array_ends, overhang, modes, refused) go through the four
unbanded routes, the banded context, 32 and 64 lanes and both forms of the strip kernel.  Left out, for reasons in the code:
16 lanes x blocks and x the four `overhang:deep` reads (16 lanes hold at most 10 rows each, so the context has at most 160 rows;
these reads have 200); `fit` and `slot` need contexts and strides of their own and run on the first pass (both schemes) only;
the entries and the shuffle run on the default route over the sets named in their tests.

The raw records of all routes of one context shape are the same bytes."""
import numpy as np
import pytest

from bbmap_amd import msa as M
from tests import gapped_problems as G
from tests.msa_check import check_gapped_job, gapped_expected, gapped_set
from tests.test_msa_routes_gpu import BANDED, SENT, UNBANDED, Dev, make_ctx, record, run

pytestmark = pytest.mark.gpu

FAST = 320                                   # first-pass column buffer: wider gapped references take the wide pass
ROUTES = {                                   # name: environment of bbmsa_create
    "first_pass": {"BBMSA_NARROW": 0},
    "narrow": {},
    "sorted": {"BBMSA_NARROW": 0, "BBMSA_SORT_BY_WIDTH": 1},
    "latency": {"BBMSA_NARROW": 0, "BBMSA_LATENCY_JOBS": 1 << 20},
}
SETS_11TS = ("gap_steps", "lane_sweep", "blocks", "array_ends", "overhang", "modes", "refused")
_PACKED = {}


def packed(scheme, name):
    key = (scheme, name)
    if key not in _PACKED:
        probs, flags, kinds = gapped_set(scheme, name)
        _PACKED[key] = G.pack(probs, flags)
    return _PACKED[key]


def context(monkeypatch, scheme="11ts", env=None, lanes=0, band=UNBANDED, maxRows=None, maxColumns=None):
    sh = G.SHAPES[scheme]
    if scheme == "9pacbio":
        monkeypatch.setenv("BBMSA_GENERIC_SCRATCH_MB", "4096")
    return make_ctx(monkeypatch, env or {}, lanes, band, scheme=M.SCHEME_11TS if scheme == "11ts" else M.SCHEME_9PACBIO,
                    maxRows=maxRows or sh["maxRows"], maxColumns=maxColumns or sh["maxColumns"], fast_cols=FAST if scheme == "11ts" else 0)


def stride_for(exp, flags):
    """Room for every string of the set as the kernels write it (KEEP_GAPS: with its '-'), a multiple of 16."""
    need = [len(e["kept"] if f & G.KEEP_GAPS else e["match"]) for e, f in zip(exp, flags) if e is not None and e["match"] is not None]
    return (max(need + [16]) + 15) & ~15


def check_records(rec, mat, exp, flags, tag, n=None):
    """Records 0 .. n-1 against the oracle (record k is job k % len(exp): a Dev repeats its set up to its capacity); an array the
    reference's contract does not cover (exp None) must be BBMSA_ST_BAD_SHAPE; bytes past a string stay as they were."""
    for k in range(len(exp) if n is None else n):
        e, f = exp[k % len(exp)], flags[k % len(exp)]
        g = record(rec, mat, k)
        ctx = "%s: job %d flags %#x" % (tag, k, f)
        if e is None:
            assert g["status"] == M.ST_BAD_SHAPE and g["match_len"] == 0 and g["score"] is None, ctx
        else:
            check_gapped_job(g, e, f, ctx)
        assert (mat[k, max(0, g["match_len"]):] == SENT).all(), ctx + ": bytes past the string were written"


def band_candidates(probs, exp):
    """Per job: does band_is_candidate (msa_common.h) take it?  Derived jobs are FILL_LIMITED over greflimit + 1 columns."""
    out = []
    for p, e in zip(probs, exp):
        if e is None or e["gref"] is None or e["refused"]:
            out.append(False)
            continue
        rows, cols, ms = len(p[0]), e["gref"][1] + 1, p[4]
        out.append(16 <= rows <= cols and ms >= 1 and cols + rows >= 90 and cols <= rows + min(170, rows + 20)
                   and (70 + 100 * (rows - 1)) - (ms - 120) <= 2000)
    return out


def launched(marks, n_launched):
    """How many marked jobs a launch of n_launched jobs holds when the set repeats up to the launch's size (Dev)."""
    reps, tail = divmod(n_launched, len(marks))
    return reps * sum(marks) + sum(marks[:tail])


def gref_columns(exp):
    return [e["gref"][1] + 1 if e is not None and e["gref"] is not None and not e["refused"] else None for e in exp]


def assert_route(ctx, name, probs, exp, n_launched):
    r, c = ctx.last_route(), ctx.last_counts()
    assert not r["indirect"] and r["wide_pass"], (name, r)
    assert r["narrow"] == (name == "narrow") and r["sorted"] == (name == "sorted") and r["latency"] == (name == "latency"), (name, r)
    cols = gref_columns(exp)
    n_wide = launched([w is not None and w > FAST for w in cols], n_launched)
    n_deep = launched([w is not None and w < len(p[0]) - 2 for p, w in zip(probs, cols)], n_launched)
    if name == "latency":
        assert r["first_handed_on"] == 0, (name, r)
    else:
        assert r["first_handed_on"] == n_wide + n_deep, (name, r, n_wide, n_deep)      # too wide or too narrow for the first pass
    assert r["wide_handed_on"] == n_deep and c["generic"] == n_deep, (name, r, c)      # narrower than the read: the generic kernel
    if name == "narrow":
        assert c["narrow"] + c["narrow_left"] == launched(band_candidates(probs, exp), n_launched), (name, c)


@pytest.mark.parametrize("name", SETS_11TS)
def test_every_route_matches_the_oracle(monkeypatch, name):
    probs, flags, kinds = gapped_set("11ts", name)
    exp = gapped_expected("11ts", name)
    jobs, gaps, reads, refs = packed("11ts", name)
    stride = stride_for(exp, flags)
    n = len(jobs)
    dev = Dev(jobs, reads, refs, cap=max(n, 256), gaps=gaps)             # (sorted: launches of 256 jobs and more)
    first = None
    for route, env in ROUTES.items():
        ctx = context(monkeypatch, env=env, lanes=32)
        rec, mat = run(ctx, dev, stride, n=dev.cap)
        assert_route(ctx, route, probs, exp, dev.cap)
        ctx.close()
        check_records(rec, mat, exp, flags, "%s route %s" % (name, route), n=dev.cap)
        if first is None:
            first = (rec.copy(), mat.copy())
        else:
            assert rec.tobytes() == first[0].tobytes() and mat.tobytes() == first[1].tobytes(), (name, route)
    if name == "modes":
        assert sum(band_candidates(probs, exp)) >= 6                          # the band kernel did get gapped jobs
    if name in ("gap_steps", "blocks"):
        assert sum(w > FAST for w in gref_columns(exp)) >= 20              # and the wide pass


@pytest.mark.parametrize("name", SETS_11TS)
def test_banded_context_matches_the_oracle(monkeypatch, name):
    """A band: the first pass redoes in the generic kernel what breaks its assumption about a row's good columns (a job whose rows
    have holes), beside the jobs narrower than the read."""
    probs, flags, kinds = gapped_set("11ts", name)
    exp = gapped_expected("11ts", name, BANDED)
    jobs, gaps, reads, refs = packed("11ts", name)
    ctx = context(monkeypatch, lanes=32, band=BANDED)
    rec, mat = run(ctx, Dev(jobs, reads, refs, gaps=gaps), stride_for(exp, flags))
    r, c = ctx.last_route(), ctx.last_counts()
    ctx.close()
    cols = gref_columns(exp)
    n_deep = sum(w is not None and w < len(p[0]) - 2 for p, w in zip(probs, cols))
    assert not r["narrow"] and r["wide_pass"] and not r["sorted"] and not r["latency"], r
    # a read across a gap keeps good cells on two diagonals at least 129 columns apart, so every set has rows with holes: the
    # generic kernel took more than the jobs narrower than the read
    assert r["wide_handed_on"] == c["generic"] and c["generic"] > n_deep, (r, c, n_deep)
    check_records(rec, mat, exp, flags, "banded " + name)


LANE_ROWS = {16: 160, 32: 224, 64: 224}      # 16 lanes hold at most 10 rows each (create_11ts doubles the group beyond that)


@pytest.mark.parametrize("name", SETS_11TS)
def test_lane_groups_of_16_32_and_64(monkeypatch, name):
    """Every set at 32 and 64 lanes per job; at 16 lanes, whose context cannot have more than 160 rows, the jobs of up to 160 rows:
    all of gap_steps, lane_sweep, array_ends, modes and refused, overhang without its 200-row `deep` jobs, and none of blocks
    (200-row reads), which therefore runs at 32 and 64 lanes only."""
    probs, flags, kinds = gapped_set("11ts", name)
    exp = gapped_expected("11ts", name)
    stride = stride_for(exp, flags)
    cols = gref_columns(exp)
    first = None
    for lanes in (32, 64, 16):
        idx = [k for k, p in enumerate(probs) if len(p[0]) <= LANE_ROWS[lanes]]
        if name == "blocks" and lanes == 16:
            assert not idx
            continue
        assert len(idx) >= len(probs) - 8
        jobs, gaps, reads, refs = G.pack([probs[k] for k in idx], [flags[k] for k in idx])
        ctx = context(monkeypatch, env=ROUTES["first_pass"], lanes=lanes, maxRows=LANE_ROWS[lanes])
        assert ctx.geometry()["lanes"] == lanes
        rec, mat = run(ctx, Dev(jobs, reads, refs, gaps=gaps), stride)
        r, c = ctx.last_route(), ctx.last_counts()
        ctx.close()
        n_wide = sum(cols[k] is not None and cols[k] > FAST for k in idx)
        n_deep = sum(cols[k] is not None and cols[k] < len(probs[k][0]) - 2 for k in idx)
        assert r["first_handed_on"] == n_wide + n_deep and c["generic"] == n_deep, (lanes, r, c)
        check_records(rec, mat, [exp[k] for k in idx], [flags[k] for k in idx], "%s lanes %d" % (name, lanes))
        if first is None:
            first = (rec.copy(), mat.copy())
        else:
            assert rec.tobytes() == first[0][idx].tobytes() and mat.tobytes() == first[1][idx].tobytes(), (name, lanes)


@pytest.mark.parametrize("form", ["sequential", "pipelined"])
@pytest.mark.parametrize("name", SETS_11TS)
def test_pacbio_strip_kernel_matches_the_oracle(monkeypatch, name, form):
    """The strip kernel answers every job itself in both forms (it takes windows narrower than the read too): nothing goes to the
    generic kernel -- no band, and no hand-shake of the pipelined form timed out."""
    probs, flags, kinds = gapped_set("9pacbio", name)
    exp = gapped_expected("9pacbio", name)
    jobs, gaps, reads, refs = packed("9pacbio", name)
    assert len(jobs) <= 512                                              # (the pipelined form takes launches of up to BBMSA_STRIP_PIPE_JOBS)
    monkeypatch.setenv("BBMSA_STRIP_PIPE_JOBS", "0" if form == "sequential" else "512")
    ctx = context(monkeypatch, "9pacbio")
    monkeypatch.delenv("BBMSA_STRIP_PIPE_JOBS")
    rec, mat = run(ctx, Dev(jobs, reads, refs, gaps=gaps), stride_for(exp, flags))
    r, c = ctx.last_route(), ctx.last_counts()
    ctx.close()
    assert not r["narrow"] and not r["wide_pass"] and not r["sorted"] and not r["latency"], r
    assert r["first_handed_on"] == 0 and c["generic"] == 0, (form, r, c)
    check_records(rec, mat, exp, flags, "9pacbio %s %s" % (form, name))


def test_pacbio_banded_context_takes_the_generic_kernel(monkeypatch):
    """9PacBio hands only banded fills to its generic kernel: the one way a derived job reaches that kernel's gapped tail there."""
    probs, flags, kinds = gapped_set("9pacbio", "gap_steps")
    exp = gapped_expected("9pacbio", "gap_steps", BANDED)
    jobs, gaps, reads, refs = packed("9pacbio", "gap_steps")
    ctx = context(monkeypatch, "9pacbio", band=BANDED)
    rec, mat = run(ctx, Dev(jobs, reads, refs, gaps=gaps), stride_for(exp, flags))
    r = ctx.last_route()
    ctx.close()
    assert r["first_handed_on"] > 0, r
    check_records(rec, mat, exp, flags, "9pacbio banded gap_steps")


@pytest.mark.parametrize("scheme", ["11ts", "9pacbio"])
def test_contexts_around_greflimit_columns(monkeypatch, scheme):
    """maxColumns = greflimit + 2, + 1 fit (the cushion is 2 and 1 bytes); + 0, - 1, - 2 (the copy exactly fills maxColumns + 2),
    - 3 and a far too small context are refused, and the plain jobs of the launch do not notice."""
    probs, flags, kinds, lim = G.fit(scheme)
    jobs, gaps, reads, refs = G.pack(probs, flags)
    dev = Dev(jobs, reads, refs, gaps=gaps)
    for delta in G.FIT_DELTAS + (G.FIT_SMALL - lim,):
        exp = gapped_expected(scheme, "fit", maxColumns=lim + delta, problems=probs, flags=flags, kinds=kinds)
        assert [e["refused"] for e, k in zip(exp, kinds) if k == "fit:gapped"] == [delta < 1] * kinds.count("fit:gapped")
        assert all(e["score"] is not None for e in exp if not e["refused"])
        ctx = context(monkeypatch, scheme, env=ROUTES["first_pass"], lanes=32, maxColumns=lim + delta)
        rec, mat = run(ctx, dev, stride_for(exp, flags) + 16)
        ctx.close()
        check_records(rec, mat, exp, flags, "%s fit maxColumns = greflimit %+d" % (scheme, delta))


def test_direct_indirect_and_host_entries(monkeypatch):
    """gap_steps and blocks in one launch through bbmsa_align_gapped_batch_device (1, 3, 4, 5 and 257 jobs: make_gref_kernel and
    gref_post_kernel take four jobs per block), its _indirect form (a count below the capacity: nothing past it is written) and
    bbmsa_align_gapped_batch."""
    probs, flags, exp = [], [], []
    for name in ("gap_steps", "blocks"):
        p, f, _ = gapped_set("11ts", name)
        probs, flags, exp = probs + p, flags + f, exp + gapped_expected("11ts", name)
    jobs, gaps, reads, refs = G.pack(probs, flags)
    n = len(jobs)
    stride = stride_for(exp, flags)
    ctx = context(monkeypatch, lanes=32)
    dev = Dev(jobs, reads, refs, cap=300, gaps=gaps)
    full = None
    for m in (257, 1, 3, 4, 5):
        rec, mat = run(ctx, dev, stride, n=m)
        check_records(rec, mat, exp, flags, "direct n = %d" % m, n=m)
        assert (rec[m:].view(np.uint8) == SENT).all() and (mat[m:] == SENT).all(), "direct n = %d: records past n_jobs written" % m
        if full is None:
            full = (rec.copy(), mat.copy())
        else:
            assert rec[:m].tobytes() == full[0][:m].tobytes() and mat[:m].tobytes() == full[1][:m].tobytes(), m
    for count in (n, 257, 5, 0, 1000):
        rec, mat = run(ctx, dev, stride, count=count)
        assert ctx.last_route()["indirect"]
        m = min(count, dev.cap)
        check_records(rec, mat, exp, flags, "indirect count = %d" % count, n=min(m, 257))
        assert rec[:min(m, 257)].tobytes() == full[0][:min(m, 257)].tobytes(), count
        assert (rec[m:].view(np.uint8) == SENT).all() and (mat[m:] == SENT).all(), "indirect count = %d: records past the count written" % count
    res, hmat = ctx.align_gapped_batch(jobs, gaps, reads, refs, stride)
    ctx.close()
    assert res.tobytes() == full[0][:n].tobytes()
    for k in range(n):
        ml = max(0, int(res[k]["match_len"]))
        assert hmat[k, :ml].tobytes() == full[1][k, :ml].tobytes(), k


@pytest.mark.parametrize("name", ["lane_sweep", "modes"])
def test_records_do_not_depend_on_position_or_on_the_scratch_buffer(monkeypatch, name):
    """The set, the same set shuffled, then the set again on one context: the gapped references land in other slots of the scratch
    buffer, over what the launch before left there."""
    import random
    probs, flags, kinds = gapped_set("11ts", name)
    exp = gapped_expected("11ts", name)
    stride = stride_for(exp, flags)
    ctx = context(monkeypatch, lanes=32)
    jobs, gaps, reads, refs = packed("11ts", name)
    dev = Dev(jobs, reads, refs, gaps=gaps)
    rec0, mat0 = run(ctx, dev, stride)
    check_records(rec0, mat0, exp, flags, name + " in order")
    order = list(range(len(probs)))
    random.Random(5).shuffle(order)
    j2, g2, r2, f2 = G.pack([probs[k] for k in order], [flags[k] for k in order])
    rec1, mat1 = run(ctx, Dev(j2, r2, f2, gaps=g2), stride)
    for pos, k in enumerate(order):
        assert rec1[pos].tobytes() == rec0[k].tobytes() and mat1[pos].tobytes() == mat0[k].tobytes(), (name, pos, k, kinds[k])
    rec2, mat2 = run(ctx, dev, stride)
    ctx.close()
    assert rec2.tobytes() == rec0.tobytes() and mat2.tobytes() == mat0.tobytes()


@pytest.mark.parametrize("scheme", ["11ts", "9pacbio"])
def test_string_slots_that_fit_exactly_and_miss_by_one(monkeypatch, scheme):
    """match_stride equal to a job's expanded length: its string is there; one below: match_len == -1 and the record otherwise
    intact.  The same with BBMSA_TRACE_KEEP_GAPS, whose strings are the short ones."""
    probs, flags, kinds = gapped_set(scheme, "slot")
    exp = gapped_expected(scheme, "slot")
    ctx = context(monkeypatch, scheme, lanes=32)
    for keep in (False, True):
        fl = [f | G.KEEP_GAPS if keep else f for f in flags]
        jobs, gaps, reads, refs = G.pack(probs, fl)
        dev = Dev(jobs, reads, refs, gaps=gaps)
        need = [len(e["kept"] if keep else e["match"]) for e in exp]
        assert len(set(need)) == len(need) and all(e["kept"].count(b"-") > 0 for e in exp)
        for k in range(len(probs)):
            for stride in (need[k], need[k] - 1):
                rec, mat = run(ctx, dev, stride)
                for q, e in enumerate(exp):
                    g = record(rec, mat, q)
                    tag = "%s keep %s stride %d job %d need %d" % (scheme, keep, stride, q, need[q])
                    if need[q] > stride:
                        assert g["match_len"] == -1, tag
                        g["match_len"], g["match"] = need[q], e["kept"] if keep else e["match"]        # every other field: as with room
                    else:
                        assert (mat[q, g["match_len"]:] == SENT).all(), tag
                    check_gapped_job(g, e, fl[q], tag)
                assert int(rec[k]["match_len"]) == (need[k] if stride == need[k] else -1)
    ctx.close()


@pytest.mark.parametrize("entry", ["device", "host"])
def test_refused_arrays_do_not_disturb_their_neighbours(monkeypatch, entry):
    """Odd ngaps, 1, 17, descending entries, a negative one, one at or past ref_len, a gap below 128 (127 and 0), a window that
    ends before it starts: BBMSA_ST_BAD_SHAPE, nothing computed.  ngaps 0 and -1 are plain jobs.  Every other job of the launch
    equals its record from a launch without the refused ones."""
    probs, flags, kinds = gapped_set("11ts", "refused")
    exp = gapped_expected("11ts", "refused")
    stride = stride_for(exp, flags)
    keep = [k for k, kind in enumerate(kinds) if not G.is_refused(kind)]
    assert len(keep) == len(kinds) - 11
    ctx = context(monkeypatch, lanes=32)

    def launch(idx):
        jobs, gaps, reads, refs = G.pack([probs[k] for k in idx], [flags[k] for k in idx])
        if entry == "host":
            res, mat = ctx.align_gapped_batch(jobs, gaps, reads, refs, stride)
            return res, np.where(np.arange(stride)[None, :] < np.maximum(res["match_len"], 0)[:, None], mat, SENT)
        return run(ctx, Dev(jobs, reads, refs, gaps=gaps), stride)

    rec, mat = launch(list(range(len(kinds))))
    check_records(rec, mat, exp, flags, "refused, " + entry)
    for k, kind in enumerate(kinds):
        if G.is_refused(kind):
            assert int(rec[k]["status"]) == M.ST_BAD_SHAPE and int(rec[k]["score_len"]) == 0 and int(rec[k]["match_len"]) == 0, kind
    clean_rec, clean_mat = launch(keep)
    ctx.close()
    for pos, k in enumerate(keep):
        assert rec[k].tobytes() == clean_rec[pos].tobytes() and mat[k].tobytes() == clean_mat[pos].tobytes(), (k, kinds[k])
