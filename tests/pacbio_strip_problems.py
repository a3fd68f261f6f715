"""Planted job sets for the strip-tiled 9PacBio kernel (bbmap_amd/csrc/msa_fill_strip.hip): plain Python, fixed seeds, no GPU.

Every generator returns (problems, flags, kinds): problems[k] = (read, ref, refStartLoc, refEndLoc, minScore), flags[k] the job's
mode, kinds[k] what job k was planted for -- "name" or "name:key=value:key=value" (kind_args splits it; rows and columns are
1-based, as the kernel and the reference count them).  tests/test_pacbio_strip_problems_cpu.py holds every plant to the oracle
(did the insertion land on the rows it was planted on?), tests/test_pacbio_strip_edges_gpu.py holds the device to the oracle.

Sets:
  rows   read lengths on every edge of the row ownership (1, R, 2R, the strip's last lane, 512 | 513, 1024 | 1025, maxRows) x error kinds
  death  a limited fill whose first row not entered walks across the strip border one row at a time
  cols   window widths on the edges of the 64-column boundary blocks, of the record dwords, of maxColumns, of the read's length
  walk   tracebacks that cross the strip border inside an insertion / deletion run, runs at the penalty tiers and past the 9-bit time,
         reads hanging over either end of the window, references with '-' symbols
  mixed  one launch of tiny, tall, bad-shape and overflowing jobs (more jobs than pipelined slots)
and the launches of the one-resident-wave test and of the banded contexts."""
import random

from bbmap_amd import msa as M
from tests.problems import rand_seq

STRIP = 512                  # rows of a strip: 64 lanes x kStripR (= 8) rows per lane, bbmap_amd/csrc/msa_fill_strip.hip (`constexpr int kStripR`)
MAX_ROWS = 2 * STRIP + 6     # 1030: three strips (so three wavefronts per job in the pipelined form), six rows in the last one
MAX_COLS = 1203              # not a multiple of 8 (the LDS layout), >= rows + 170

ALL = M.FILL_AND_SCORE_LIMITED | M.DO_TRACEBACK
LIM = M.FILL_LIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
UNL = M.FILL_UNLIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
MODES = (ALL, LIM, UNL)

ROW_LENGTHS = (1, 2, 7, 8, 9, 16, 17, 504, 505, 511, 512, 513, 520, 521, 1023, 1024, 1025, 1030)
DEATH_ROWS, DEATH_Q = (1030, 700), tuple(range(506, 518))
INS_N = (1, 4, 5, 6, 19, 20, 21, 30)
DEL_N = (1, 4, 5, 6, 19, 20, 21, 79, 80, 81, 84, 130)
MIXED_STRIDE = 1104          # match_stride of the mixed launch: room for every string of it but the one with an expanded '-'


def max_q(rows):
    """MultiStateAligner9PacBio.maxQuality: MATCH for the first base, MATCH2 for every other."""
    return 90 + 100 * (rows - 1)


def tight_min_score(rows):
    """A minScore that a perfect read still reaches in a limited fill and a read with one substitution does not.  Not max_q:
    vertLimit counts the LAST base as the one that gains MATCH and every other as MATCH2 (:413-425 of the Java) while the fill gives
    MATCH to the FIRST, so with minScore = max_q row 1 (90) is below its limit (100); and the match plane is pruned where the
    diagonal is <= limit - MATCH2 (:314, not <), so max_q - 10 dies in row 2.  With max_q - 20 every row of a perfect read is good
    with 10 to spare, and a substitution (-137 - 100) leaves nothing good in its row."""
    return max_q(rows) - 20


def kind_args(kind):
    """'ins:n=4:row=508' -> ('ins', {'n': 4, 'row': 508})"""
    name, *rest = kind.split(":")
    return name, {k: int(v) for k, v in (x.split("=") for x in rest)}


def columns_of(p, fl, maxColumns=MAX_COLS):
    """The window's width as the kernel computes it (MSA.fillAndScoreLimited clamps, the raw modes do not)."""
    a, b = p[2], p[3]
    if fl & M.CLAMP_WINDOW:
        a, b = max(0, a), min(len(p[1]) - 1, b)
        if b - a >= maxColumns:
            b = min(len(p[1]) - 1, a + maxColumns - 1)
    return b - a + 1


def other(rng, b, alphabet=b"ACGT"):
    return rng.choice([x for x in alphabet if x != b])


class _Set:
    def __init__(self, maxRows=MAX_ROWS, maxColumns=MAX_COLS):
        self.maxRows, self.maxColumns = maxRows, maxColumns
        self.probs, self.flags, self.kinds = [], [], []

    def add(self, kind, rd, rf, a, b, ms, fl, check=True):
        if check:
            assert 1 <= len(rd) <= self.maxRows and 1 <= min(b, len(rf) - 1) - max(a, 0) + 1 <= self.maxColumns, kind
            assert fl == ALL or (0 <= a and b < len(rf)), kind             # only the Java-level mode clamps
        self.probs.append((bytes(rd), rf, a, b, ms))
        self.flags.append(fl)
        self.kinds.append(kind)

    def out(self):
        return self.probs, self.flags, self.kinds


def _window(rng, st, span, rows):
    """rows + 8..30 columns around the `span` reference bases the read was drawn from."""
    cols = max(rows, span) + rng.randrange(8, 31)
    a = st - rng.randrange(0, cols - span + 1)
    return a, a + cols - 1


def _foreign(rng, n, before, after):
    """n inserted bases that cannot slide: the first differs from the reference base after the run, the last from the one before."""
    f = bytearray(rand_seq(rng, n))
    f[0] = other(rng, after)
    f[-1] = rng.choice([x for x in b"ACGT" if x != before and (n > 1 or x != after)])
    return bytes(f)


def _del_site(rng, ref, lo, hi, q, n):
    """A site st such that deleting ref[st + q : st + q + n] can slide neither way (the bases at both ends of the run differ from
    the ones the slide would pair them with)."""
    for _ in range(1000):
        st = rng.randrange(lo, hi)
        if ref[st + q] != ref[st + q + n] and ref[st + q - 1] != ref[st + q + n - 1]:
            return st
    raise AssertionError("no site")


# ------------------------------------------------------------------------------------------------ rows
def rows_set():
    rng = random.Random(5120)
    ref = rand_seq(rng, 4000)
    refn = bytearray(ref)                                              # the same reference with an N every 23 bases
    for i in range(11, len(refn), 23):
        refn[i] = ord("N")
    refn = bytes(refn)
    S = _Set()

    def site(span):
        return rng.randrange(300, len(ref) - span - 300)

    turn = 0
    for rows in ROW_LENGTHS:
        variants = ["perfect", "subs", "del", "ins"] if rows >= 7 else ["perfect", "subs"]     # (1 and 2 rows cannot flank an indel)
        variants += ["n:q=%d" % q for q in (510, 511, 512, 513) if q < rows] if rows >= 511 else ["n"]
        variants += ["refn", "lower", "wrong_site", "unreachable"] + (["last_row"] if rows >= 2 else [])
        for v in variants:
            turn += 1
            fl = MODES[turn % 3]
            st = site(rows + 6)
            rd = bytearray(ref[st:st + rows])
            rf, span = ref, rows
            ms = int(rng.choice([0.3, 0.5, 0.7]) * max_q(rows))
            name = v.split(":")[0]
            if name == "subs":
                for _ in range(rng.randint(1, 3)):
                    q = rng.randrange(rows)
                    rd[q] = other(rng, rd[q])
            elif name == "del":                                        # the read lacks 1-6 reference bases
                d, q = rng.randint(1, 6), rng.randrange(3, rows - 3)
                rd = bytearray(ref[st:st + q] + ref[st + q + d:st + rows + d])
                span = rows + d
            elif name == "ins":                                        # the read holds 1-6 bases the reference lacks
                d = rng.randint(1, min(6, rows - 6))
                q = rng.randrange(3, rows - d - 2)
                rd = bytearray(ref[st:st + q] + rand_seq(rng, d) + ref[st + q:st + rows - d])
                span = rows - d
            elif name == "n":                                          # the bases whose MATCH / MATCH2 cost the suffix sum carries over the border
                q = kind_args(v)[1]["q"] if ":" in v else rng.randrange(rows)
                rd[q] = ord("N")
            elif name == "refn":
                rf = refn
            elif name == "lower":                                      # a lower-case stretch of the reference inside the window
                q, ln = rng.randrange(0, max(1, rows - 4)), rng.randint(1, 12)
                rf = ref[:st + q] + ref[st + q:st + q + ln].lower() + ref[st + q + ln:]
            elif name == "unreachable":                                # no cell of row 1 is good
                ms, fl = max_q(rows) + 121, (ALL if turn % 2 else LIM)
            elif name == "last_row":                                   # good down to the last row, where nothing reaches minScore
                rd[rows - 1] = other(rng, rd[rows - 1])
                ms, fl = tight_min_score(rows), LIM
            a, b = _window(rng, st, span, rows)
            if name == "wrong_site":                                   # a window somewhere else: dies where its luck ends
                a, b = _window(rng, site(rows + 6), rows, rows)
                ms, fl = int(rng.choice([0.5, 0.7]) * max_q(rows)), (ALL if turn % 2 else LIM)
            S.add("%s:rows=%d" % (v, rows), rd, rf, a, b, ms, fl)
    return S.out()


# ------------------------------------------------------------------------------------------------ death
def death_set():
    """minScore = the highest a perfect read reaches, and one substitution at base q: row q + 1 has no good cell, row q + 2 is the
    first one not entered."""
    rng = random.Random(5121)
    ref = rand_seq(rng, 3000)
    S = _Set()
    for rows in DEATH_ROWS:
        st = rng.randrange(300, 1200)
        a, b = st - 9, st + rows + 11                                  # one window per read length: the visited cells differ by q alone
        for q in DEATH_Q:
            rd = bytearray(ref[st:st + rows])
            rd[q] = other(rng, rd[q])
            S.add("death:rows=%d:q=%d" % (rows, q), rd, ref, a, b, tight_min_score(rows), LIM)
    return S.out()


# ------------------------------------------------------------------------------------------------ cols
def cols_widths(rows):
    """The smallest widths >= rows + 8 with columns mod 64 in {62, 63, 0, 1, 2}.  (columns + 63) & 7 follows from columns mod 64:
    these five give 5, 6, 7, 0, 1, so the record-dword residues 6, 7, 0 ride on 63, 0, 1; no other pairing exists.)"""
    return [next(c for c in range(rows + 8, rows + 8 + 64) if c % 64 == r) for r in (62, 63, 0, 1, 2)]


def cols_set():
    rng = random.Random(5122)
    ref = rand_seq(rng, 4000)
    S = _Set()
    turn = 0
    for rows in (513, 600):
        def read(v, st):
            rd = bytearray(ref[st:st + rows])
            if v == "subs":
                for _ in range(2):
                    q = rng.randrange(rows)
                    rd[q] = other(rng, rd[q])
                return rd, rows
            d, q = rng.randint(1, 6), rng.randrange(3, rows - 3)
            return bytearray(ref[st:st + q] + ref[st + q + d:st + rows + d]), rows + d
        for cols in cols_widths(rows):
            for v in ("subs", "del"):
                turn += 1
                st = rng.randrange(400, 2000)
                rd, span = read(v, st)
                a = st - rng.randrange(0, cols - span + 1)
                S.add("width:rows=%d:cols=%d:mod64=%d:dword=%d" % (rows, cols, cols % 64, (cols + 63) & 7), rd, ref, a, a + cols - 1,
                      int(0.5 * max_q(rows)), MODES[turn % 3])
        for fl in MODES:                                               # columns == maxColumns
            st = rng.randrange(700, 2000)
            rd, span = read("subs", st)
            a = st - rng.randrange(0, MAX_COLS - span + 1)
            S.add("max_columns:rows=%d:cols=%d" % (rows, MAX_COLS), rd, ref, a, a + MAX_COLS - 1, int(0.5 * max_q(rows)), fl)
        for k, short in enumerate((3, 40, 0)):                         # windows no wider than the read: columns = rows - short
            st = rng.randrange(400, 2000)
            nins = short + 5                                           # single inserted bases, spread: the read spans rows - nins reference bases
            rd = bytearray(ref[st:st + rows - nins])
            for i in range(nins):
                q = 5 + i * ((rows - 20) // nins)
                rd.insert(q, other(rng, rd[q]))
            cols = rows - short
            a = st - 2
            for fl in (MODES[k % 3], MODES[(k + 1) % 3]):
                S.add("narrow:rows=%d:cols=%d:short=%d" % (rows, cols, short), rd, ref, a, a + cols - 1, int(0.3 * max_q(rows)), fl)
        short_ref = rand_seq(rng, rows + 60)                           # windows clamped at its ends (the Java-level mode only)
        ls = len(short_ref)
        S.add("clamped_left:rows=%d" % rows, short_ref[3:3 + rows], short_ref, -rng.randrange(1, 20), rows + 24, int(0.4 * max_q(rows)), ALL)
        S.add("clamped_right:rows=%d" % rows, short_ref[ls - rows - 2:ls - 2], short_ref, ls - rows - 20, ls - 1 + rng.randrange(1, 20),
              int(0.4 * max_q(rows)), ALL)
        S.add("clamped_both:rows=%d" % rows, short_ref[30:30 + rows], short_ref, -5, ls + 5, int(0.4 * max_q(rows)), ALL)
    return S.out()


# ------------------------------------------------------------------------------------------------ walk
def ins_rows(n):
    """First rows of the planted insertion runs of n bases: ending at row 511, ending at 512, straddling 512 | 513, starting at 513."""
    r = {"end511": STRIP - n, "end512": STRIP + 1 - n, "start513": STRIP + 1}
    if n >= 2:
        r["straddle"] = STRIP + 1 - (n + 1) // 2
    return r


def walk_set():
    rng = random.Random(5123)
    ref = rand_seq(rng, 5000)
    S = _Set()
    rows = MAX_ROWS
    turn = 0
    for n in INS_N:                                                    # (a) an insertion run of n read bases on rows row .. row + n - 1
        for where, row in ins_rows(n).items():
            turn += 1
            st = rng.randrange(400, 3000)
            q = row - 1
            rd = ref[st:st + q] + _foreign(rng, n, ref[st + q - 1], ref[st + q]) + ref[st + q:st + rows - n]
            a, b = _window(rng, st, rows - n, rows)
            S.add("ins:n=%d:row=%d" % (n, row), rd, ref, a, b, int(0.5 * max_q(rows)), MODES[turn % 3])
    for n in DEL_N:                                                    # (b) n reference bases missing; the diagonal goes on at row `row`
        for row in (STRIP, STRIP + 1, 300):
            turn += 1
            q = row - 1
            st = _del_site(rng, ref, 400, 3000, q, n)
            rd = ref[st:st + q] + ref[st + q + n:st + n + rows]
            a, b = _window(rng, st, rows + n, rows)
            S.add("del:n=%d:row=%d:col=%d" % (n, row, st + q - a + 1), rd, ref, a, b, int(0.5 * max_q(rows)), MODES[turn % 3])
    for n in (520, 600):                                               # (c) a deletion streak past the 9-bit time (a 400-row read: the window fits)
        for fl in (LIM, UNL):
            q = 200
            st = _del_site(rng, ref, 400, 3000, q, n)
            rd = ref[st:st + q] + ref[st + q + n:st + n + 400]
            a, b = _window(rng, st, 400 + n, 400)
            S.add("longdel:n=%d:row=%d:col=%d" % (n, q + 1, st + q - a + 1), rd, ref, a, b, int(0.3 * max_q(400)), fl)
    st = rng.randrange(400, 3000)                                      # (d) an insertion streak past the 9-bit time, across the border
    rd = ref[st:st + 255] + _foreign(rng, 520, ref[st + 254], ref[st + 255]) + ref[st + 255:st + 510]
    a, b = _window(rng, st, 510, 510)
    S.add("longins:n=520:row=256", rd, ref, a, b, 0, UNL)
    for k in (1, 5, 70):                                               # (e) the read hangs over an end of its window by k bases
        for side in ("left", "right"):
            turn += 1
            st = rng.randrange(400, 3000)
            pad = rng.randrange(8, 31)
            a, b = (st + k, st + rows - 1 + pad) if side == "left" else (st - pad, st + rows - 1 - k)
            S.add("overhang_%s:k=%d:rows=%d" % (side, k, rows), ref[st:st + rows], ref, a, b, int(0.3 * max_q(rows)), MODES[turn % 3])
    st = rng.randrange(400, 3000)                                      # ... an overhang that begins in strip 0 and ends in strip 1
    S.add("overhang_right:k=70:rows=530", ref[st:st + 530], ref, st - 12, st + 529 - 70, int(0.3 * max_q(530)), UNL)
    for fl in (UNL, ALL):                                              # ... and one on the strip's last lane, in the last column: the records'
        st = rng.randrange(400, 3000)                                  # last, partial dword
        S.add("overhang_right:k=5:rows=512", ref[st:st + STRIP], ref, st - 9, st + STRIP - 1 - 5, int(0.3 * max_q(STRIP)), fl)
    for name, gaps in (("gap64", (64,)), ("gap65", (65,)), ("gap64_65", (64, 65)), ("gap65_600", (65, 600))):
        turn += 1                                                      # (f) '-' symbols at these columns of the window: each stands for 128 bases
        base = rand_seq(rng, rows + 40)
        gref = bytearray(base)
        for c in gaps:
            gref.insert(c - 1, ord("-"))
        gref = bytes(gref)                                             # window = the whole of it; the read starts under column 5
        S.add("%s:gaps=%d" % (name, len(gaps)), base[4:4 + rows], gref, 0, len(gref) - 1, int(0.3 * max_q(rows)), MODES[turn % 3])
    return S.out()


# ------------------------------------------------------------------------------------------------ mixed
def mixed_set():
    """One launch: ~300 jobs of 1-40 rows, twelve of 513-1030 rows spread through the list, three bad shapes and one job whose
    match string (a '-' expands to 128 symbols) does not fit MIXED_STRIDE.  Launched with MSAContext.align_batch and that stride."""
    rng = random.Random(5124)
    ref = rand_seq(rng, 4000)
    S = _Set()
    n_small = 314
    tall_at = {int(i * (n_small - 1) / 11) for i in range(12)}         # first, last, and between
    special = {40: "bad_rows", 140: "bad_columns", 250: "bad_columns_zero", 200: "overflow"}
    for i in range(n_small):
        fl = MODES[i % 3]
        if i in tall_at:
            rows = rng.choice([514, 600, 777, 1024, 1025, 1030])
            st = rng.randrange(300, 2600)
            rd = bytearray(ref[st:st + rows])
            for _ in range(3):
                q = rng.randrange(rows)
                rd[q] = other(rng, rd[q])
            del rd[rows // 2]
            a, b = _window(rng, st, rows, rows - 1)
            S.add("tall:rows=%d" % (rows - 1), rd, ref, a, b, int(0.5 * max_q(rows - 1)), fl)
        if i in special:
            name = special[i]
            st = rng.randrange(300, 2000)
            if name == "bad_rows":
                S.add(name, ref[st:st + MAX_ROWS + 1], ref, st - 4, st + MAX_ROWS + 10, 1000, LIM, check=False)
            elif name == "bad_columns":                                # maxColumns + 1 columns, and the raw modes do not clamp
                S.add(name, ref[st:st + 600], ref, st - 4, st - 4 + MAX_COLS, 1000, LIM, check=False)
            elif name == "bad_columns_zero":
                S.add(name, ref[st:st + 30], ref, st, st - 1, 1000, UNL, check=False)
            else:
                base = rand_seq(rng, MAX_ROWS + 30)
                gref = base[:400] + b"-" + base[400:]
                S.add("overflow:gaps=1", base[6:6 + MAX_ROWS], gref, 0, len(gref) - 1, int(0.3 * max_q(MAX_ROWS)), ALL)
        rows = rng.randint(1, 40)
        st = rng.randrange(300, 3000)
        rd = bytearray(ref[st:st + rows])
        if i % 4 == 1:
            q = rng.randrange(rows)
            rd[q] = other(rng, rd[q])
        if i % 4 == 2 and rows > 10:
            del rd[rows // 2]
        a, b = _window(rng, st, rows, len(rd))
        S.add("small:rows=%d" % len(rd), rd, ref, a, b, int(rng.choice([0.3, 0.6]) * max_q(len(rd))), fl)
    return S.out()


# ------------------------------------------------------------------------------------------------ one resident wave
def one_wave_set():
    """~40 jobs that a single resident wave (or slot) runs one after the other: tall-wide, tiny, mid, alternating; limited fills that
    finish, limited fills that die early, unlimited fills.  Each inherits the records, boundary rows and bookkeeping of the one before."""
    rng = random.Random(5125)
    ref = rand_seq(rng, 4000)
    S = _Set()
    shapes = ((1030, 1200), (3, 20), (513, 530), (1030, 1200), (3, 20), (600, 664))
    for i in range(42):
        rows, cols = shapes[i % len(shapes)]
        how = ("limited", "dies", "unlimited")[(i + i // len(shapes)) % 3]
        st = rng.randrange(400, 2400)
        rd = bytearray(ref[st:st + rows])
        if rows > 3:
            for _ in range(3):
                q = rng.randrange(rows)
                rd[q] = other(rng, rd[q])
            q = rng.randrange(10, rows - 10)
            rd = rd[:q] + rd[q + 1:] + ref[st + rows:st + rows + 1]     # one deleted base; the read keeps its length
        ms, fl = int(0.5 * max_q(rows)), (ALL if i % 2 else LIM)
        if how == "unlimited":
            fl = UNL
        if how == "dies":                                              # nothing reaches this once the first error is met
            ms, fl = max_q(rows) - 20, LIM
        a = st - rng.randrange(0, cols - rows - 1)
        S.add("%s:rows=%d:cols=%d" % (how, rows, cols), rd, ref, a, a + cols - 1, ms, fl)
    return S.out()


# ------------------------------------------------------------------------------------------------ banded contexts
BANDED_ROWS, BANDED_COLS = 600, 900


def banded_set():
    """~60 jobs of 60-600 rows in the three modes, for a context with a band: its limited fills leave the strip kernel."""
    rng = random.Random(5126)
    ref = rand_seq(rng, 4000)
    S = _Set(BANDED_ROWS, BANDED_COLS)
    lengths = [60, 64, 65, 100, 200, 333, 511, 512, 513, 599, 600] + [rng.randint(60, 600) for _ in range(49)]
    for i, rows in enumerate(lengths):
        st = rng.randrange(300, 3000)
        rd = bytearray(ref[st:st + rows + 8])
        for _ in range(i % 4):
            q = rng.randrange(rows)
            rd[q] = other(rng, rd[q])
        if i % 5 == 1:
            del rd[rows // 3:rows // 3 + rng.randint(1, 4)]
        if i % 5 == 3:
            rd.insert(rows // 2, other(rng, rd[rows // 2]))
        rd = rd[:rows]
        a, b = _window(rng, st, rows, rows)
        S.add("banded:rows=%d" % rows, rd, ref, a, b, int(rng.choice([0.3, 0.5, 0.7, 0.97]) * max_q(rows)), MODES[i % 3])
    return S.out()


SETS = {"rows": (rows_set, MAX_ROWS, MAX_COLS, (0, 0.0)), "death": (death_set, MAX_ROWS, MAX_COLS, (0, 0.0)),
        "cols": (cols_set, MAX_ROWS, MAX_COLS, (0, 0.0)), "walk": (walk_set, MAX_ROWS, MAX_COLS, (0, 0.0)),
        "mixed": (mixed_set, MAX_ROWS, MAX_COLS, (0, 0.0)), "one_wave": (one_wave_set, MAX_ROWS, MAX_COLS, (0, 0.0)),
        "banded_ratio": (banded_set, BANDED_ROWS, BANDED_COLS, (0, 0.18)), "banded_width": (banded_set, BANDED_ROWS, BANDED_COLS, (40, 0.0))}
_ANSWERS = {}


def answers(name):
    """(problems, flags, kinds, expected) of a set, the oracle's answers (tests.msa_check.oracle_align; None for a bad-shape job)
    computed once per process and shared by every test that needs them.  Nobody changes them."""
    if name not in _ANSWERS:
        from oracle.oracle import OracleMSA
        from tests.msa_check import oracle_align
        gen, maxRows, maxColumns, band = SETS[name]
        probs, flags, kinds = gen()
        om = OracleMSA(maxRows, maxColumns, band[0], band[1], scheme="9pacbio")
        exp = [None if k.startswith("bad_") else oracle_align(om, p[0], p[1], p[2], p[3], p[4], f) for p, f, k in zip(probs, flags, kinds)]
        _ANSWERS[name] = (probs, flags, kinds, exp)
    return _ANSWERS[name]
