"""Planted job sets for the gapped-reference path of the DP (bbmap_amd/csrc/msa_gapped.hip and the gapped tail of every fill
kernel): plain Python, fixed seeds, no GPU.

A read is built as blocks of the reference separated by long deletions, and carries the gap array BBIndex.makeGapArray would give
its site: {start, end of block 1, start of block 2, ..., stop}.  Arrays stay within the reference's contract (refStartLoc <=
gaps[0], refEndLoc >= gaps[last], every gap >= 256 = MINGAP, which is what fix_gaps2 leaves) except in the `refused` set.

Every generator takes the scheme ("11ts" or "9pacbio": read lengths and context shape follow SHAPES) and returns (problems, flags,
kinds): problems[k] = (read, ref, refStartLoc, refEndLoc, minScore, gaps) as MultiStateAligner11ts.alignGapped takes them (gaps:
a list, None, or RawGaps for a record no list can spell), flags[k] the job's mode, kinds[k] "class:what" -- the class name first.
pack() turns a set into what the device entries take.  tests/test_oracle_gapped.py proves from the oracle alone that every set
holds what it claims; tests/test_msa_gapped_edges_gpu.py holds the device to the oracle on them.

Sets:
  gap_steps    one gap at the smallest legal size and around the multiples of 128 (rem == 0 / div steps), at 63 | 64 | 65 symbols, 16 kb
  lane_sweep   first-block length x gap % 128: the '-' run, greflimit and the index of b on every residue mod 64, also behind a
               run of more than 64 symbols (the carry of the 64-index scans)
  blocks       2 .. 8 blocks (ngaps 4 .. 16), mixed gap sizes
  array_ends   windows clipped at either end of the reference array, last block 1 .. 127 bases before its end (the cushion's 'N')
  overhang     reads that start left of / stop right of the window (pad hints, translated starts left of the origin)
  fit          one shape for contexts whose maxColumns is greflimit + 2 .. - 3 and far too small
  modes        the same jobs under every mode a gapped job can carry
  slot         jobs whose strings the test fits exactly / misses by one byte
  refused      gap arrays the device must refuse, between jobs it must not disturb"""
import random
from collections import namedtuple

from bbmap_amd import msa as M
from tests.problems import rand_seq

KEEP_GAPS = M.TRACE_KEEP_GAPS
ALL = M.FILL_AND_SCORE_LIMITED | M.DO_TRACEBACK
KEEP = ALL | KEEP_GAPS
UNL = M.FILL_UNLIMITED_RAW | M.DO_SCORE | M.DO_TRACEBACK
SCORE_ONLY = M.FILL_AND_SCORE_LIMITED
MODES = (ALL, KEEP, UNL, M.FILL_UNLIMITED_RAW, SCORE_ONLY, ALL | M.NO_ITERATIONS)

# context shape and read lengths per scheme; 9PacBio: the shape tests/test_pacbio_gpu.py::test_pacbio_gapped_reference_jobs uses
SHAPES = {"11ts": dict(maxRows=224, maxColumns=1600, L=150, Lblocks=200, sweep0=97, match=70),
          "9pacbio": dict(maxRows=640, maxColumns=2400, L=450, Lblocks=480, sweep0=300, match=90)}
GAP_STEPS = (256, 257, 383, 384, 385, 511, 512, 8319, 8320, 8321, 8447, 8448, 16000, 16383)    # 8320: 64 symbols, 8448: 65
SWEEP_REMS = {"11ts": (0, 1, 37, 63, 64, 127), "9pacbio": (0, 127)}
SWEEP_REMS_BEHIND = {"11ts": (0, 64, 127), "9pacbio": (64,)}
FIT_SMALL = 120                          # a context no gapped reference of the set fits: the copy loops run past maxColumns + 2
FIT_DELTAS = (2, 1, 0, -1, -2, -3)       # maxColumns - greflimit; -2: the copy exactly fills maxColumns + 2, -3: one over

RawGaps = namedtuple("RawGaps", "ngaps entries")      # a bbmsa_gaps record as it stands (ngaps need not match the entries)


def max_q(scheme, rows):
    return SHAPES[scheme]["match"] + 100 * (rows - 1)


def gref_symbols(gap):
    """'-' symbols makeGref writes for one gap (MultiStateAligner11tsJNI.java:668-757)."""
    return (gap - 128) // 128


def gref_columns(g, a, b):
    """greflimit of a gap array in a window, from the definition: every block whole, every gap as 64 + gap % 128 bases, its
    symbols and 64 bases."""
    g = [min(g[0], a)] + list(g[1:-1]) + [max(g[-1], b)]
    n = sum(g[i + 1] - g[i] + 1 for i in range(0, len(g), 2))
    for i in range(1, len(g) - 1, 2):
        gap = g[i + 1] - g[i] - 1
        n += 128 + gap % 128 + gref_symbols(gap)
    return n


def planted(ref, st, blocks, dels):
    """The read made of `blocks` (lengths) of ref from st on, dels[i] reference bases skipped behind block i, and its gap array."""
    rd, g, pos = bytearray(), [], st
    for i, n in enumerate(blocks):
        rd += ref[pos:pos + n]
        g += [pos, pos + n - 1]
        pos += n + (dels[i] if i < len(dels) else 0)
    return rd, g


def split(L, k):
    """L in k blocks as equal as they get."""
    return [L // k + (1 if i < L % k else 0) for i in range(k)]


def other(rng, b):
    return rng.choice([x for x in b"ACGT" if x != b])


class _Set:
    def __init__(self, scheme, seed, ref_len):
        self.scheme, self.shape = scheme, SHAPES[scheme]
        self.rng = random.Random(seed)
        self.ref = rand_seq(self.rng, ref_len)
        self.probs, self.flags, self.kinds = [], [], []

    def errors(self, rd, nsub):
        """nsub substitutions away from the ends; 9PacBio: also a deleted base every ~53, as its reads have them."""
        rd = bytearray(rd)
        for _ in range(nsub):
            p = self.rng.randrange(8, len(rd) - 8)
            rd[p] = other(self.rng, rd[p])
        if self.scheme == "9pacbio":
            for pos in range(len(rd) - 12, 20, -53):
                del rd[pos]
        return rd

    def add(self, kind, rd, rf, a, b, frac, gaps, fl=ALL, ms=None):
        assert 1 <= len(rd) <= self.shape["maxRows"], kind
        self.probs.append((bytes(rd), rf, a, b, int(frac * max_q(self.scheme, len(rd))) if ms is None else ms, gaps))
        self.flags.append(fl)
        self.kinds.append(kind)

    def out(self):
        return self.probs, self.flags, self.kinds


def gap_steps(scheme="11ts"):
    s = _Set(scheme, 101, 20000)
    L = s.shape["L"]
    for gap in GAP_STEPS:
        for nsub in range(4):
            st = s.rng.randrange(300, 2500)
            cut = L // 2 - 9 + 6 * nsub
            rd, g = planted(s.ref, st, [cut, L - cut], [gap])
            s.add("gap_steps:gap=%d:subs=%d" % (gap, nsub), s.errors(rd, nsub), s.ref, st - 4, g[-1] + 4, (0.3, 0.5)[nsub & 1], g)
        # a short indel beside the gap: two read bases missing left of it / two extra right of it
        st = s.rng.randrange(300, 2500)
        cut = L // 2
        rd, g = planted(s.ref, st, [cut, L - cut], [gap])
        short = bytearray(rd)
        del short[cut - 8:cut - 6]
        s.add("gap_steps:gap=%d:del_beside" % gap, s.errors(short, 0), s.ref, st - 4, g[-1] + 4, 0.3, g)
        longer = bytearray(rd)
        longer[cut + 7:cut + 7] = bytes(other(s.rng, x) for x in rd[cut + 7:cut + 9])
        s.add("gap_steps:gap=%d:ins_beside" % gap, s.errors(longer, 0), s.ref, st - 4, g[-1] + 4, 0.3, g)
    return s.out()


def lane_sweep(scheme="11ts"):
    """64 consecutive first-block lengths (the read grows with them, so greflimit moves too) x gap % 128; then the same behind a
    first gap of 65 or more symbols, which puts the second run and b past the first 64-index chunk with a carry.  Every read
    runs two bases past its window's end: the pad hint is the only consumer of the index of b (a job without one gives the same
    record whatever that index is), so only such jobs pin it."""
    s = _Set(scheme, 202, 24000)
    L0 = s.shape["sweep0"]
    for rem in SWEEP_REMS[scheme]:
        for i in range(64):
            st = 400 + 7 * i
            rd, g = planted(s.ref, st, [30 + i, L0 - 30], [256 + rem + 128 * (i % 3)])
            g[-1] -= 2
            s.add("lane_sweep:rem=%d:i=%d" % (rem, i), s.errors(rd, i % 2), s.ref, st - 4, g[-1], 0.3, g)
    for k, rem in enumerate(SWEEP_REMS_BEHIND[scheme]):
        for i in range(64):
            st = 400 + 5 * i
            rd, g = planted(s.ref, st, [24, 20 + i, L0 - 44], [8448 + 131 * k, 256 + rem])         # 65, 66, 67 symbols in front
            g[-1] -= 2
            s.add("lane_sweep:behind:rem=%d:i=%d" % (rem, i), s.errors(rd, i % 2), s.ref, st - 4, g[-1], 0.3, g)
    return s.out()


def _block_gaps(k, variant):
    """k - 1 gap sizes: 256 + 37 i, or mixed sizes (large ones where few blocks leave the columns for them)."""
    if variant == 0:
        return [256 + 37 * i for i in range(k - 1)]
    if k <= 5:
        return [(387, 2600, 512, 300, 1500)[(i + k) % 5] for i in range(k - 1)]
    return [256 + 128 * ((i + k) % 3) + 11 * i for i in range(k - 1)]


def blocks(scheme="11ts"):
    s = _Set(scheme, 303, 16000)
    L = s.shape["Lblocks"]
    for k in range(2, 9):
        for variant in (0, 1):
            for rep in range(6):
                st = s.rng.randrange(300, 2000)
                rd, g = planted(s.ref, st, split(L, k), _block_gaps(k, variant))
                s.add("blocks:k=%d:v=%d" % (k, variant), s.errors(rd, rep % 3), s.ref, st - 4, g[-1] + 4, 0.3, g)
    return s.out()


def array_ends(scheme="11ts"):
    s = _Set(scheme, 404, 12000)
    L = s.shape["L"]
    for gap in (256, 300, 511, 1500, 8320):
        for over in (1, 4, 40):
            # the site starts at 0 and the window left of it
            rd, g = planted(s.ref, 0, split(L, 2), [gap])
            s.add("array_ends:left:gap=%d" % gap, s.errors(rd, 1), s.ref, -over, g[-1] + 4, 0.3, g)
            # the site stops at the array's last base and the window right of it: the whole cushion is 'N'
            rd, g = planted(s.ref, 700, split(L, 2), [gap])
            short = s.ref[:g[-1] + 1]
            s.add("array_ends:right:gap=%d" % gap, s.errors(rd, 1), short, 696, g[-1] + over, 0.3, g)
            # and the read runs two bases past the array: they meet the cushion's first 'N'
            s.add("array_ends:right:over:gap=%d" % gap, s.errors(rd, 1) + b"AC", short, 696, g[-1] + over, 0.3, g)
        # both at once
        rd, g = planted(s.ref, 0, split(L, 3), [gap, 256])
        short = s.ref[:g[-1] + 1]
        s.add("array_ends:both:gap=%d" % gap, s.errors(rd, 0), short, -3, g[-1] + 3, 0.3, g)
    for tail in (1, 2, 3, 63, 64, 65, 100, 126, 127):
        # the last block ends `tail` bases before the array does: the cushion is `tail` bases, then 'N'
        rd, g = planted(s.ref, 900, split(L, 2), [256 + tail])
        short = s.ref[:g[-1] + 1 + tail]
        s.add("array_ends:tail=%d" % tail, s.errors(rd, tail % 2), short, 896, g[-1] + 4, 0.3, g)
        s.add("array_ends:tail=%d:tight" % tail, s.errors(rd, 0), short, 900, g[-1], 0.5, g)
    return s.out()


def overhang(scheme="11ts"):
    """The window (and the gap array's ends with it) starts `left` bases inside the read's first block and ends `right` bases
    short of its last one; `tail`: the read goes on with bases that match nothing, behind a window that ends with the site (an
    insertion state in the last column but one); `deep`: so much of the read hangs over that the gapped reference has fewer columns
    than the read has rows (the kernels for windows narrower than the read take it)."""
    s = _Set(scheme, 505, 20000)
    L = s.shape["L"]
    for gap in (256, 300, 8320):
        for left in (0, 1, 3, 10, 25):
            for right in (0, 1, 10, 25):
                if left == 0 and right == 0:
                    continue
                st = s.rng.randrange(300, 2500)
                rd, g = planted(s.ref, st, split(L, 2), [gap])
                g[0] += left
                g[-1] -= right
                s.add("overhang:left=%d:right=%d:gap=%d" % (left, right, gap), s.errors(rd, 0), s.ref, g[0], g[-1], 0.3, g)
    for gap in (256, 300):
        for tail in (1, 2, 3, 4, 5, 6, 8, 12):
            st = s.rng.randrange(300, 2500)
            rd, g = planted(s.ref, st, split(L - tail, 2), [gap])
            after = s.ref[g[-1] + 1:g[-1] + 1 + tail]
            rd = s.errors(rd, 0) + bytes(other(s.rng, x) for x in after)
            s.add("overhang:tail=%d:gap=%d" % (tail, gap), rd, s.ref, g[0] - 4, g[-1], 0.3, g)
    for gap in (256, 384):
        for hang in (80, 90):
            st = s.rng.randrange(600, 2500)
            inner = s.shape["Lblocks"] - 2 * hang
            rd, g = planted(s.ref, st, split(inner, 2), [gap])
            rd = s.ref[st - hang:st] + rd + s.ref[g[-1] + 1:g[-1] + 1 + hang]
            rd = s.errors(rd, 0)
            s.add("overhang:deep:hang=%d:gap=%d" % (hang, gap), rd, s.ref, g[0], g[-1], 0, g, ALL, ms=1)
            s.add("overhang:deep:hang=%d:gap=%d:unlimited" % (hang, gap), rd, s.ref, g[0], g[-1], 0, g, UNL)
    return s.out()


def fit(scheme="11ts"):
    """Jobs of ONE greflimit (returned fourth) and a few ungapped neighbours narrow enough for every context of the test."""
    s = _Set(scheme, 606, 6000)
    L = s.shape["L"]
    lim = None
    for k, fl in enumerate((ALL, ALL, KEEP, UNL, UNL, SCORE_ONLY)):
        st = 500 + 300 * k
        rd, g = planted(s.ref, st, split(L, 2), [300])
        s.add("fit:gapped", s.errors(rd, k % 3), s.ref, st - 4, g[-1] + 4, 0.3, g, fl)
        assert lim in (None, gref_columns(g, st - 4, g[-1] + 4))
        lim = gref_columns(g, st - 4, g[-1] + 4)
    for k in range(3):
        st = 700 + 200 * k
        s.add("fit:plain", s.errors(s.ref[st:st + 100], k), s.ref, st - 4, st + 103, 0.3, None, ALL)
    return s.out() + (lim,)


def modes(scheme="11ts"):
    """The same jobs under every mode; `null`: a minScore out of reach, which only a job whose gapped reference is narrow enough
    for the limited fill (at most rows + min(170, rows + 20) columns) answers with null."""
    s = _Set(scheme, 707, 20000)
    L = s.shape["L"]
    base = []
    for gap in (256, 258, 270, 300, 512, 8320):
        for pad in (0, 4):
            st = s.rng.randrange(300, 2500)
            rd, g = planted(s.ref, st, split(L, 2), [gap])
            base.append((s.errors(rd, pad // 4), st - pad, g[-1] + pad, g, "gap=%d" % gap))
    for k in (3, 5):
        st = s.rng.randrange(300, 2500)
        rd, g = planted(s.ref, st, split(L, k), _block_gaps(k, 0))
        base.append((s.errors(rd, 1), st - 4, g[-1] + 4, g, "k=%d" % k))
    for rd, a, b, g, what in base:
        for fl in MODES:
            s.add("modes:%s:flags=%d" % (what, fl), rd, s.ref, a, b, 0.3, g, fl)
        s.add("modes:%s:null" % what, rd, s.ref, a, b, 0, g, ALL, ms=max_q(scheme, len(rd)) + 121)
        # within the band kernel's slack (11ts: 2000 below the best score); 9PacBio reads carry their deletions' cost
        s.add("modes:%s:tight" % what, rd, s.ref, a, b, 0, g, ALL,
              ms=max_q(scheme, len(rd)) - 1500 if scheme == "11ts" else int(0.8 * max_q(scheme, len(rd))))
    return s.out()


def slot(scheme="11ts"):
    s = _Set(scheme, 808, 20000)
    L = s.shape["L"]
    for k, gap in enumerate((256, 300, 512, 1500, 8320)):
        st = s.rng.randrange(300, 2500)
        rd, g = planted(s.ref, st, split(L - 3 * k, 2), [gap])
        s.add("slot:gap=%d" % gap, s.errors(rd, k % 2), s.ref, st - 4, g[-1] + 4, 0.3, g, ALL)
    return s.out()


def refused(scheme="11ts"):
    """Every refused array between two good jobs (`refused:neighbour`); `refused:pass`: ngaps 0 and -1 are plain jobs whatever the
    entries hold."""
    s = _Set(scheme, 909, 8000)
    L = s.shape["L"]

    def good(k):
        st = 400 + 150 * k
        rd, g = planted(s.ref, st, split(L, 2), [300 + 40 * k])
        return s.errors(rd, k % 2), st, g

    n = len(s.ref)
    cases = [("ngaps1", lambda g, a, b: (RawGaps(1, g), a, b)),
             ("ngaps3", lambda g, a, b: (RawGaps(3, g), a, b)),
             ("ngaps17", lambda g, a, b: (RawGaps(17, g + [g[-1]] * 12), a, b)),
             ("descending", lambda g, a, b: ([g[0], g[2], g[1], g[3]], a, b)),
             ("descending_last", lambda g, a, b: ([g[0], g[1], g[2], g[2] - 1], a, g[2] - 1)),
             ("negative", lambda g, a, b: ([-5, g[1], g[2], g[3]], -9, b)),
             ("past_end", lambda g, a, b: ([g[0], g[1], g[2], n], a, n + 3)),
             ("past_end_inner", lambda g, a, b: ([g[0], g[1], n + 7, n + 9], a, n + 9)),
             ("gap127", lambda g, a, b: ([g[0], g[1], g[1] + 128, g[3]], a, b)),
             ("gap0", lambda g, a, b: ([g[0], g[1], g[1] + 1, g[3]], a, b)),
             ("window_reversed", lambda g, a, b: (g, b, a))]
    for k, (name, bend) in enumerate(cases):
        rd, st, g = good(k)
        s.add("refused:neighbour", rd, s.ref, st - 4, g[-1] + 4, 0.3, list(g))
        g2, a, b = bend(list(g), st - 4, g[-1] + 4)
        s.add("refused:" + name, rd, s.ref, a, b, 0.3, g2)
    rd, st, g = good(len(cases))
    s.add("refused:neighbour", rd, s.ref, st - 4, g[-1] + 4, 0.3, list(g))
    for ngaps in (0, -1):
        st = 3000 + 200 * ngaps
        s.add("refused:pass:ngaps=%d" % ngaps, s.errors(s.ref[st:st + L], 1), s.ref, st - 4, st + L + 3, 0.3, RawGaps(ngaps, [7, 3, -2, 99999]))
    rd, st, g = good(len(cases) + 1)
    s.add("refused:neighbour", rd, s.ref, st - 4, g[-1] + 4, 0.3, list(g))
    return s.out()


SETS = {"gap_steps": gap_steps, "lane_sweep": lane_sweep, "blocks": blocks, "array_ends": array_ends, "overhang": overhang,
        "modes": modes, "slot": slot, "refused": refused}


def is_refused(kind):
    return kind.startswith("refused:") and not kind.startswith(("refused:neighbour", "refused:pass"))


def gaps_of(p):
    """A problem's gap array as the oracle takes it: a list, or None for a plain job (None, or ngaps <= 0)."""
    g = p[5]
    if isinstance(g, RawGaps):
        return None if g.ngaps <= 0 else list(g.entries[:g.ngaps])
    return g


def gap_records(problems):
    import numpy as np
    rec = np.zeros(len(problems), M.GAPS_DTYPE)
    for k, p in enumerate(problems):
        g = p[5]
        if g is None:
            continue
        ngaps, entries = (g.ngaps, g.entries) if isinstance(g, RawGaps) else (len(g), g)
        rec[k]["ngaps"] = ngaps
        rec[k]["gaps"][:min(16, len(entries))] = entries[:16]
    return rec


def pack(problems, flags):
    """(jobs, gaps, reads, refs) as bbmsa_align_gapped_batch and its device forms take them."""
    jobs, reads, refs = M.pack_problems([p[:5] for p in problems], list(flags))
    return jobs, gap_records(problems), reads, refs
