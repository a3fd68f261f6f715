"""Every rows-per-lane build of the wavefront DP kernel (msa_fill_fast_kernel<R, BANDED, MAT>) against the oracle, job by job.

The kernel is compiled for R = 1..10 rows per lane, with and without a band, in the batch form and in the matrix-materialising
form (MAT) of the per-call fills: 40 builds.  R decides which lane owns a row, the suffix sum behind vertLimit, which lane and slot
keep the last row's maximum, where a traceback record lies and where both walkers look for it, and (through the register budget
of its launch bounds) what spills.  A batch context runs R = ceil(maxRows / lanes), so a context of exactly lanes * R rows picks
the build; a MAT launch runs R = ceil(longest read of the launch / 64).  bbmsa_geometry says which build ran.

Batch form: for every (R, band) one context per lane group (16, 32, 64 lanes) with maxRows = lanes * R, and one launch of a
seeded job set whose row counts sit on every edge of the row ownership (1..4 for the barriers, R, R + 1, 2R, half the rows, the
last lane entered by one row, maxRows - 1, maxRows), whose windows sit on the edges of the kernel's shape (the narrowest window
it keeps, one column less, the first pass's buffer and one column more, a partial last record dword, windows clamped at either
end), with perfect reads, substitutions, indels, N on both sides, wrong sites, fills that die in a middle row and in the last
row, and the three fill modes mixed per job.  Every record is compared field by field.

MAT form: solo fills at both ends of every R's range of read lengths, and shared launches of many threads in which short reads
run at the rows per lane of a long one; planes, limits and the walkers' answers against the oracle's."""
import random
import threading

import numpy as np
import pytest

from bbmap_amd import msa as M
from oracle.oracle import OracleMSA
from tests.msa_check import check_job, check_packed_fill, oracle_align
from tests.problems import max_quality, rand_seq
from tests.test_msa_routes_gpu import SENT, Dev, make_ctx, record, run

pytestmark = pytest.mark.gpu

ALL = M.FILL_AND_SCORE_LIMITED | M.DO_TRACEBACK
LIM = M.FILL_LIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
UNL = M.FILL_UNLIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
MODES = (ALL, LIM, UNL)
UNBANDED, BANDED = (0, 0.0), (40, 0.18)
LANES = (16, 32, 64)
BADOFF = (-(1 << 20) + 2000) << 11             # what a limited fill that never reached the last row reports as its score


def shape(G, R):
    """(maxRows, maxColumns, fast_cols) of the context that runs R rows per lane on G lanes.  Ordinary windows (rows + 8..30
    columns) fit the first pass's buffer; the planted fast_cols + 1 and the window clamped at both ends do not."""
    return G * R, G * R + 128, G * R + 40


def row_counts(G, R):
    m = G * R
    return sorted({r for r in (1, 2, 3, 4, R, R + 1, 2 * R, m // 2, m // 2 + 1, (G - 1) * R, (G - 1) * R + 1, m - 1, m) if 1 <= r <= m})


def subfloor(rows, ms):
    """The limited fill's "not a score" (jni/MultiStateAligner11tsJNI.c:405-408), which it reports when the last row holds nothing good."""
    return (ms - ((rows - 1) * 100 + 70) - 500) << 11


# ------------------------------------------------------------------------------------------------ job set
def jobset(G, R):
    """(problems, flags, kinds) for the context shape(G, R); kinds[k] names what job k was planted for."""
    maxR, maxC, fast = shape(G, R)
    rng = random.Random(7919 * R + G)
    ref = rand_seq(rng, 4000)
    refn = bytearray(ref)                                              # the same reference with an N every 23 bases
    for i in range(11, len(refn), 23):
        refn[i] = ord("N")
    refn = bytes(refn)
    short = rand_seq(rng, maxR + 60)                                   # windows clamped at its ends
    probs, flags, kinds = [], [], []

    def add(kind, rd, rf, a, b, ms, fl):
        assert 1 <= len(rd) <= maxR and 1 <= min(b, len(rf) - 1) - max(a, 0) + 1 <= maxC, kind
        assert fl == ALL or (0 <= a and b < len(rf)), kind             # only the Java-level mode clamps
        probs.append((bytes(rd), rf, a, b, ms))
        flags.append(fl)
        kinds.append(kind)

    def site(span):
        return rng.randrange(300, len(ref) - span - 300)

    def window(st, span, rows):
        """An ordinary window of rows + 8..30 columns around the `span` reference bases the read was drawn from."""
        cols = rows + rng.randrange(8, 31)
        a = st - rng.randrange(0, cols - span + 1)
        return a, a + cols - 1

    def other(b, alphabet=b"ACGT"):
        return rng.choice([x for x in alphabet if x != b])

    def ratio_ms(rows):
        return int(rng.choice([0.3, 0.5, 0.7]) * max_quality(rows))

    turn = 0
    for rows in row_counts(G, R):
        variants = ("perfect", "subs", "n", "unreachable", "last_row") if rows <= 4 else \
            ("perfect", "subs", "del", "ins", "n", "wrong_site", "unreachable", "last_row")
        for v in variants:
            turn += 1
            fl = MODES[turn % 3]
            st = site(rows + 6)
            rd = bytearray(ref[st:st + rows])
            rf, span, ms = ref, rows, ratio_ms(rows)
            if v == "subs":
                for _ in range(rng.randint(1, 3)):
                    q = rng.randrange(rows)
                    rd[q] = other(rd[q])
            elif v == "del" and rows >= 8:                             # the read lacks 1-6 reference bases
                d, q = rng.randint(1, 6), rng.randrange(3, rows - 3)
                rd = bytearray(ref[st:st + q] + ref[st + q + d:st + rows + d])
                span = rows + d
            elif v == "ins" and rows >= 8:                             # the read holds 1-6 bases the reference lacks
                d = rng.randint(1, min(6, rows - 6))
                q = rng.randrange(3, rows - d - 2)
                rd = bytearray(ref[st:st + q] + rand_seq(rng, d) + ref[st + q:st + rows - d])
                span = rows - d
            elif v == "n":
                if turn % 2:
                    rd[rng.randrange(rows)] = ord("N")
                else:
                    rf = refn
            elif v == "unreachable":                                   # no cell of row 1 is good: a fill of two or more rows stops in its middle
                ms, fl = max_quality(rows) + 121, (ALL if turn % 2 else LIM)
            elif v == "last_row" and rows >= 2:                        # good down to the last row, where nothing reaches minScore
                rd[rows - 1] = other(rd[rows - 1])
                ms, fl = max_quality(rows), LIM
            a, b = window(st, span, rows)
            if v == "wrong_site":                                      # a window somewhere else: dies where its luck ends
                a, b = window(site(rows + 6), rows, rows)
                ms, fl = int(rng.choice([0.5, 0.7]) * max_quality(rows)), (ALL if turn % 2 else LIM)
            add(v, rd, rf, a, b, ms, fl)

    m = G * R
    rb = m // 2 + 1                                                    # (>= 9: a row count in the middle of the lanes)
    for k, rows in enumerate((m, rb)):                                 # the narrowest window the kernel keeps
        st = site(rows)
        add("cols_rows_minus_2", ref[st:st + rows], ref, st + 1, st + rows - 2, int(0.3 * max_quality(rows)), (UNL, LIM)[k])
    for k, rows in enumerate(sorted({m, rb, (G - 1) * R + 1})):        # one column less: the one-thread kernel's
        st = site(rows)
        add("cols_rows_minus_3", ref[st:st + rows], ref, st + 1, st + rows - 3, int(0.3 * max_quality(rows)), MODES[k % 3])
    for rows in (m, rb):                                               # the first pass's buffer, and one column more (the wide pass)
        for cols in (fast, fast + 1):
            st = site(cols)
            rd = bytearray(ref[st:st + rows])
            rd[rows // 2] = other(rd[rows // 2])
            a = st - rng.randrange(0, cols - rows + 1)
            add("cols_fast" if cols == fast else "cols_fast_plus_1", rd, ref, a, a + cols - 1, int(0.3 * max_quality(rows)), MODES[(rows + cols) % 3])
    nl = (rb + R - 1) // R                                             # last step = columns + nl - 1: a record dword ending at nibble 6, 7, 0
    c0 = next(c for c in range(rb + 8, rb + 16) if (c + nl - 1) & 7 == 6)
    for cols in (c0, c0 + 1, c0 + 2):
        st = site(cols)
        rd = bytearray(ref[st:st + rb])
        rd[rb - 2] = other(rd[rb - 2])
        add("last_dword_%d" % ((cols + nl - 1) & 7), rd, ref, st - (cols - rb), st + rb - 1, int(0.5 * max_quality(rb)), ALL)
    ls = len(short)
    add("clamped_left", short[3:3 + rb], short, -rng.randrange(1, 20), rb + 24, int(0.4 * max_quality(rb)), ALL)
    add("clamped_right", short[ls - rb - 2:ls - 2], short, ls - rb - 20, ls - 1 + rng.randrange(1, 20), int(0.4 * max_quality(rb)), ALL)
    add("clamped_both", short[30:30 + m], short, -5, ls + 5, int(0.4 * max_quality(m)), ALL)      # (maxRows + 60 columns: the wide pass)

    order = list(range(len(probs)))
    rng.shuffle(order)
    return [probs[k] for k in order], [flags[k] for k in order], [kinds[k] for k in order]


def columns_of(p, fl):
    a, b = (max(0, p[2]), min(len(p[1]) - 1, p[3])) if fl & M.CLAMP_WINDOW else (p[2], p[3])
    return b - a + 1


def is_null(e, fl):
    return e["result"] is None if fl & 7 == M.FILL_LIMITED else (fl & 7 == M.FILL_LIMITED_RAW and e["result"][4] == 1)


# ------------------------------------------------------------------------------------------------ batch form
@pytest.mark.parametrize("band", [UNBANDED, BANDED], ids=["unbanded", "banded"])
@pytest.mark.parametrize("R", range(1, 11))
def test_batch_build_matches_the_oracle_at_every_lane_group(monkeypatch, R, band):
    monkeypatch.setenv("BBMSA_GENERIC_SCRATCH_MB", "512")            # (read at create: 64 scratch matrices of 640 x 768 need 379 MB)
    banded = band != UNBANDED
    n_all = nulls = 0
    rows_seen, kinds_seen, modes_seen, deaths = set(), set(), set(), set()
    for G in LANES:
        maxR, maxC, fast = shape(G, R)
        probs, flags, kinds = jobset(G, R)
        n = len(probs)
        om = OracleMSA(maxR, maxC, band[0], band[1])
        exp = [oracle_align(om, p[0], p[1], p[2], p[3], p[4], f) for p, f in zip(probs, flags)]
        cols = [columns_of(p, f) for p, f in zip(probs, flags)]
        planted = sum(c < len(p[0]) - 2 for p, c in zip(probs, cols))                # windows the wavefront kernel does not keep
        wide = sum(c > fast for c in cols)
        assert planted == kinds.count("cols_rows_minus_3") >= 2 and wide == 3
        assert all(c >= len(p[0]) - 3 and c <= maxC for p, c in zip(probs, cols))
        for p, f, e in zip(probs, flags, exp):
            if f == LIM and e["result"][4] == 1:                                     # where the limited fill died
                deaths.add("middle" if e["result"][3] == BADOFF else "last" if e["result"][3] == subfloor(len(p[0]), p[4]) else "low")
        jobs, reads, refs = M.pack_problems(probs, flags)
        stride = (2 * maxR + 128 + 8 + 15) & ~15
        ctx = make_ctx(monkeypatch, {"BBMSA_NARROW": 0}, G, band, maxRows=maxR, maxColumns=maxC, fast_cols=fast)
        geo = ctx.geometry()
        assert (maxR + G - 1) // G == R                                              # the build under test, as created:
        assert geo == {"lanes": G, "rows_per_lane": R, "fast_cols": fast, "wide_rows_per_lane": (maxR + 63) // 64}, geo
        rec, mat = run(ctx, Dev(jobs, reads, refs), stride)
        route, counts = ctx.last_route(), ctx.last_counts()
        ctx.close()
        tag = "R %d band %s lanes %d" % (R, band, G)
        assert not route["narrow"] and not route["sorted"] and not route["latency"] and route["wide_pass"], (tag, route)
        for k in range(n):
            where = "%s: job %d (%s) rows %d columns %d flags %#x" % (tag, k, kinds[k], len(probs[k][0]), cols[k], flags[k])
            g = record(rec, mat, k)
            check_job(g, exp[k], where)
            assert (mat[k, max(0, g["match_len"]):] == SENT).all(), where + ": bytes past the string were written"
        extra = counts["generic"] - planted                                          # fills the one-thread kernel redid
        print("%s: %d jobs, %d null, first pass handed on %d, one-thread kernel %d (planted %d)"
              % (tag, n, sum(is_null(e, f) for e, f in zip(exp, flags)), route["first_handed_on"], counts["generic"], planted))
        if not banded:
            assert extra == 0 and route["first_handed_on"] == planted + wide, (tag, route, counts)
        else:                                                                        # rows with holes in their good columns, by design
            assert route["first_handed_on"] >= planted + wide and extra >= 0, (tag, route, counts)
            assert extra < n - planted, (tag, counts)
            if G == 64:
                assert 3 * extra <= n - planted, (tag, counts)
        n_all += n
        nulls += sum(is_null(e, f) for e, f in zip(exp, flags))
        rows_seen |= {(G, len(p[0])) for p in probs}
        kinds_seen |= set(kinds)
        modes_seen |= set(flags)
    assert 0 < nulls < n_all
    assert rows_seen >= {(G, r) for G in LANES for r in row_counts(G, R)}
    assert kinds_seen >= {"perfect", "subs", "del", "ins", "n", "wrong_site", "unreachable", "last_row", "cols_rows_minus_2", "cols_rows_minus_3",
                          "cols_fast", "cols_fast_plus_1", "last_dword_6", "last_dword_7", "last_dword_0", "clamped_left", "clamped_right",
                          "clamped_both"}
    assert modes_seen == set(MODES) and deaths >= {"middle", "last"}, (modes_seen, deaths)


# ------------------------------------------------------------------------------------------------ matrix-materialising form
MAT_ROWS, MAT_COLS = 640, 700                  # a `packed` array of 3 x 641 x 701 ints: 5.4 MB


def _mat_case(rng, ref, i, rows, narrow=False):
    """(read, a, b, limited, minScore): a read of `rows` bases from the right site -- plain, with an N and a substitution, or
    with a deletion of 1-6 bases -- in a window of rows + 13 columns, or (narrow) one six columns narrower than the read."""
    st = rng.randrange(50, len(ref) - rows - 80)
    rd = bytearray(ref[st:st + rows + 10])
    if i % 3 == 1:
        rd[rng.randrange(rows)] = ord("N")
        rd[rng.randrange(rows)] = rng.choice(b"ACGT")
    if i % 3 == 2:
        del rd[rows // 2:rows // 2 + rng.randint(1, 6)]
    a, b = st - 4, st + rows + 8
    if narrow:
        b = a + rows - 6
    return bytes(rd[:rows]), a, b, i % 4 != 3, int(0.5 * max_quality(rows))


@pytest.mark.parametrize("band", [UNBANDED, BANDED], ids=["unbanded", "banded"])
def test_solo_packed_fills_at_both_ends_of_every_rows_per_lane(band):
    """One fill per launch, so the launch runs ceil(rows / 64) rows per lane: reads of 64 (R - 1) + 1, 64 (R - 1) + 33 and 64 R
    bases for R = 4..10 (the 60 / 100 / 150-base fills of test_legacy_packed_matrix_feeds_the_java_walkers run R = 1..3)."""
    rng = random.Random(404)
    ctx = M.MSAContext(maxRows=MAT_ROWS, maxColumns=MAT_COLS, bandwidth=band[0], bandwidthRatio=band[1], legacy=True)
    ref = rand_seq(rng, 3000)
    packed = np.empty(3 * (MAT_ROWS + 1) * (MAT_COLS + 1), np.int32)
    lengths = [x for R in range(4, 11) for x in (64 * (R - 1) + 1, 64 * (R - 1) + 33, 64 * R)]
    calls = planted = walked = limited_n = 0
    for i, rows in enumerate(x for x in lengths for _ in range(2)):                  # every length twice: other content, other mode
        narrow = i % 11 == 7
        rd, a, b, limited, ms = _mat_case(rng, ref, i, rows, narrow)

        def fill(buf):
            return ctx.fill_packed(rd, ref, a, b, ms, limited, buf, limits=True)
        walked += check_packed_fill(MAT_ROWS, MAT_COLS, band, rd, ref, a, b, ms, limited, fill, packed)
        calls, planted, limited_n = calls + 1, planted + narrow, limited_n + limited
        st = ctx.legacy_stats()
        assert st["calls"] == calls and st["launches"] == calls                      # alone in its launch, so:
        assert ctx.geometry()["rows_per_lane"] == (rows + 63) // 64, (rows, ctx.geometry())
    st, geo = ctx.legacy_stats(), ctx.geometry()
    ctx.close()
    print("band %s: %d fills (%d limited), %d handed on (%d planted), rows per lane launched %s"
          % (band, calls, limited_n, st["handed_on"], planted, sorted(geo["launched"])))
    assert geo["launched"] == set(range(4, 11)) and planted >= 3 and 0 < limited_n < calls
    if band == UNBANDED:
        assert st["handed_on"] == planted
    else:
        assert planted <= st["handed_on"] and 3 * (st["handed_on"] - planted) <= calls - planted
    assert walked > calls // 2


@pytest.mark.parametrize("band", [UNBANDED, BANDED], ids=["unbanded", "banded"])
def test_shared_packed_launches_of_mixed_lengths_match_the_oracle(band):
    """12 threads on one context, reads of 40..640 bases: calls that arrive together share a launch, which runs every fill at the
    rows per lane of its longest read -- a 40-base read on 4 lanes of 10 rows beside a 640-base one.  Every thread keeps its
    results and the rows x columns crop of its planes; each is then held to the oracle, not to the same kernel's solo run."""
    rng = random.Random(505)
    ctx = M.MSAContext(maxRows=MAT_ROWS, maxColumns=MAT_COLS, bandwidth=band[0], bandwidthRatio=band[1], legacy=True)
    ref = rand_seq(rng, 3000)
    n_threads, per_thread = 12, 5
    lengths = [40, 64, 65, 100, 129, 150, 200, 257, 300, 385, 450, 513, 600, 640]
    cases = [_mat_case(rng, ref, i, lengths[(i * 5 + i // len(lengths)) % len(lengths)]) for i in range(n_threads * per_thread)]
    got = {}
    gate = threading.Barrier(n_threads)

    def work(t):
        packed = np.zeros(3 * (MAT_ROWS + 1) * (MAT_COLS + 1), np.int32)
        planes = packed.reshape(3, MAT_ROWS + 1, MAT_COLS + 1)
        gate.wait()
        for i in range(t, len(cases), n_threads):
            rd, a, b, limited, ms = cases[i]
            res, it, vl, hl = ctx.fill_packed(rd, ref, a, b, ms, limited, packed, limits=True)
            got[i] = (res, it, vl, hl, planes[:, 1:len(rd) + 1, 1:b - a + 2].copy())
    threads = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    st, geo = ctx.legacy_stats(), ctx.geometry()
    ctx.close()
    assert len(got) == len(cases) and st["calls"] == len(cases)
    assert st["launches"] < len(cases)                                               # some calls shared a launch (ctypes releases the GIL in the call)
    own = {(len(c[0]) + 63) // 64 for c in cases}                                    # and fewer builds ran than the lengths ask for alone:
    assert geo["launched"] <= set(range(1, 11)) and len(geo["launched"]) < len(own), (geo, own)      # some read ran at a longer one's rows per lane
    assert sum(g[4].nbytes for g in got.values()) < 200 << 20
    print("band %s: %d fills in %d launches, %d handed on, rows per lane launched %s"
          % (band, len(cases), st["launches"], st["handed_on"], sorted(geo["launched"])))
    packed = np.empty(3 * (MAT_ROWS + 1) * (MAT_COLS + 1), np.int32)
    walked = 0
    for i, (rd, a, b, limited, ms) in enumerate(cases):                              # (the oracle object stays on this thread)
        res, it, vl, hl, crop = got[i]

        def fill(buf):
            buf.reshape(3, MAT_ROWS + 1, MAT_COLS + 1)[:, 1:len(rd) + 1, 1:b - a + 2] = crop
            return res, it, vl, hl
        walked += check_packed_fill(MAT_ROWS, MAT_COLS, band, rd, ref, a, b, ms, limited, fill, packed)
    assert walked > len(cases) // 2
    if band == UNBANDED:
        assert st["handed_on"] == 0
    else:
        assert 3 * st["handed_on"] <= len(cases)
