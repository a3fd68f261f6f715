"""Rescue-scan problems shared by the CPU and GPU tests."""
import random


def make_problems(seed, n, ref_len=20000):
    rng = random.Random(seed)
    body = bytearray(rng.choice(b"ACGT") for _ in range(ref_len))
    for _ in range(4):                                   # a few tandem / dispersed repeats: several equally good starts
        p, q = rng.randrange(500, ref_len - 900), rng.randrange(500, ref_len - 900)
        body[q:q + 300] = body[p:p + 300]
    p = rng.randrange(2000, ref_len - 2000)
    body[p:p + 60] = b"N" * 60
    ref = bytes(b"N" * 300 + body + b"N" * 300)
    probs = []
    for i in range(n):
        L = rng.choice([150, 150, 100, 75, 250, 40])
        true = rng.randrange(400, len(ref) - L - 400)
        rd = bytearray(ref[true:true + L])
        kind = rng.random()
        if kind < 0.3:
            pass
        elif kind < 0.7:
            for _ in range(rng.randint(1, 12)):
                rd[rng.randrange(L)] = rng.choice(b"ACGTN")
        elif kind < 0.8:
            rd = bytearray(rng.choice(b"ACGT") for _ in range(L))       # unrelated read: usually no rescue
        else:
            del rd[L // 2:L // 2 + 2]                                     # small deletion: half the read shifts
            rd += ref[true + L:true + L + 2]
        right = rng.random() < 0.5
        dist = rng.choice([200, 600, 1200, 3000])
        off = rng.randrange(0, dist + 100)
        loc = true - off if right else true + off
        ideal = true + rng.randrange(-80, 80)
        mam = rng.choice([L // 4, L // 8, 3, 0])
        probs.append((bytes(rd), 1, loc, dist, right, ideal, mam))
    # edges: search window clipped by both chromosome ends, read shorter than 10
    probs.append((ref[350:500], 1, 10, 400, True, 350, 5))
    probs.append((ref[len(ref) - 500:len(ref) - 350], 1, len(ref) - 100, 600, False, len(ref) - 500, 5))
    probs.append((ref[1000:1008], 1, 900, 300, True, 1000, 2))
    return ref, probs


# ---------------------------------------------------------------------------------------------------------------
# Edge sets for the rescue scan: several chromosomes, tandem repeats, block-edge distances, planted families, degenerate jobs.
# A job is the tuple make_problems uses: (bases, chrom, loc, searchDist, searchRight, idealStart, maxAllowedMismatches).
TANDEM_UNITS = (1, 2, 3, 5, 7, 31, 64, 65)
EDGE_LENGTHS = tuple(range(10, 20)) + (41, 63, 64, 65, 101, 127, 150, 151, 250, 301, 597, 598, 599, 600)
EDGE_DISTS = (0, 1, 63, 64, 65, 127, 128, 200, 600, 1200)
SUBSTITUTES = b"ACGTNacgt"
# (length, minIndex pad, trailing N pad): one chromosome shorter than 700, one shorter than every read that is scanned
CHROM_SHAPES = ((9000, 37, 20), (650, 11, 9), (6000, 150, 0), (3500, 301, 64), (48, 3, 2))


def _primitive_unit(rng, n):
    while True:
        u = bytes(rng.choice(b"ACGT") for _ in range(n))
        if (u + u).find(u, 1) == n:                       # no shorter period
            return u


def _make_chrom(rng, length, pad, tail):
    """Returns (chromosome, tandem spans).  N pad, then random sequence mixed with tandem repeats and N runs, a few lower-case
    stretches, N tail."""
    body, spans, room = bytearray(), [], length - pad - tail
    while len(body) < room:
        kind = rng.random()
        if kind < 0.3:
            body += bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(30, 300)))
        elif kind < 0.85:
            unit = _primitive_unit(rng, rng.choice(TANDEM_UNITS))
            total = rng.randrange(120, 1000)
            if len(body) + total <= room:
                spans.append((pad + len(body), pad + len(body) + total))
            body += (unit * (total // len(unit) + 1))[:total]
        else:
            body += b"N" * rng.randrange(1, 81)
    del body[room:]
    for _ in range(max(1, room // 1200)):
        p, n = rng.randrange(room), rng.randrange(5, 120)
        body[p:p + n] = bytes(body[p:p + n]).lower()
    return b"N" * pad + bytes(body) + b"N" * tail, spans


def _reference_set(seed):
    rng = random.Random(seed)
    made = [_make_chrom(rng, length, pad, tail) for length, pad, tail in CHROM_SHAPES]
    return [m[0] for m in made], [s[1] for s in CHROM_SHAPES], [m[1] for m in made]


def make_reference_set(seed):
    """Returns (chroms, min_index): chromosome k + 1 is chroms[k], with min_index[k] leading N."""
    chroms, min_index, _ = _reference_set(seed)
    return chroms, min_index


def make_edge_problems(seed, n):
    """n jobs spread over the chromosomes of make_reference_set(seed), chromosome numbers mixed.  Returns (chroms, min_index, probs)."""
    chroms, min_index, spans = _reference_set(seed)
    rng = random.Random(seed * 7919 + 1)
    probs = []
    for _ in range(n):
        ci = rng.choice((0, 0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4))
        ref, reflen = chroms[ci], len(chroms[ci])
        L = rng.choice(EDGE_LENGTHS)
        if reflen < L and rng.random() < 0.8:
            L = rng.choice([x for x in EDGE_LENGTHS if x <= reflen])
        if reflen < L:                                                   # the chromosome is shorter than the read: nothing to scan
            probs.append((bytes(rng.choice(b"ACGT") for _ in range(L)), ci + 1, rng.randrange(-5, reflen), rng.choice(EDGE_DISTS),
                          rng.random() < 0.5, rng.randrange(reflen), L // 4))
            continue
        last = reflen - L
        if spans[ci] and rng.random() < 0.6:                             # start in or near a tandem repeat
            a, b = rng.choice(spans[ci])
            true = min(last, max(0, rng.randrange(a - L // 2, b)))
        else:
            true = rng.randrange(max(0, min(last, min_index[ci] - 5)), last + 1)
        rd = bytearray(ref[true:true + L])
        kind = rng.random()
        if kind < 0.35:
            pass
        elif kind < 0.75:
            for _ in range(rng.randint(1, max(1, L // 12))):
                rd[rng.randrange(L)] = rng.choice(SUBSTITUTES)
        elif kind < 0.85:
            rd = bytearray(rng.choice(b"ACGT") for _ in range(L))
        elif true + L + 2 <= reflen:
            del rd[L // 2:L // 2 + 2]
            rd += ref[true + L:true + L + 2]
        right = rng.random() < 0.5
        dist = rng.choice(EDGE_DISTS)
        off = rng.randrange(0, dist + 1) if rng.random() < 0.9 else dist + rng.randrange(1, 60)
        loc = true - off if right else true + off
        where = rng.randrange(7)
        if where == 0:
            ideal = true
        elif where == 1:
            ideal = true + rng.choice((-1, 1))
        elif where == 2:
            ideal = true + rng.randrange(-30, 31)
        elif where == 3:
            ideal = true + rng.randrange(-200, 201)
        elif where == 4:                                                 # outside the window, on the side the search starts from
            ideal = loc - rng.randrange(1, 300) if right else loc + rng.randrange(1, 300)
        elif where == 5:                                                 # outside the window, on the far side
            ideal = loc + dist + rng.randrange(1, 300) if right else loc - dist - rng.randrange(1, 300)
        else:                                                            # far away, but idealStart +- absdif stays inside Java's int
            ideal = rng.choice((-1000000000, -1000000, -1, 0, 1000000, 1 << 30))
        mam = rng.choice((-2, -1, 0, 1, 3, L // 8, L // 4, L, L + 5))
        probs.append((bytes(rd), ci + 1, loc, dist, right, ideal, mam))
    return chroms, min_index, probs


def _other(rng, base):
    return rng.choice([c for c in b"ACGT" if c != (base & ~0x20)])


def make_planted_problems(seed, chrom):
    """The planted families, on a chromosome of their own with number `chrom`.  Returns (chromosome, minIndex, probs, families):
    families[i] names the family of probs[i] ("i:few", "i:half", "i:over", "ii:<chunk>", "iii", "iv", "v", "vi").  Each locus lies between random flanks longer than its search distance."""
    rng = random.Random(seed * 104729 + 5)
    pad = 23
    ref = bytearray(b"N" * pad)
    probs, fams = [], []

    def flank(n=260):
        return bytearray(rng.choice(b"ACGT") for _ in range(n))

    def place(locus, job, fam):
        """locus: bytes; job: (bases, loc, dist, right, ideal, mam) with coordinates relative to the locus"""
        at = len(ref) + 260
        ref.extend(flank() + locus + flank())
        b, loc, dist, right, ideal, mam = job
        probs.append((bytes(b), chrom, at + loc, dist, right, at + ideal, mam))
        fams.append(fam)

    lens = (10, 11, 12, 13, 41, 64, 65, 101, 150, 151, 250, 597, 598, 599, 600)
    # (i) read bases over reference N, everything else equal: few N, exactly len / 2 (still semiperfect), len / 2 + 1 (no longer)
    for rep in range(32):
        for which in range(3):
            L = lens[(rep + 5 * which) % len(lens)]
            rd = flank(L)
            k = (rng.randrange(1, min(6, L // 2 + 1)), L // 2, L // 2 + 1)[which]
            locus = bytearray(rd)
            for p in rng.sample(range(L), k):
                locus[p] = ord("N")
            right, off = rep % 2 == 0, rng.randrange(0, 130)
            place(locus, (rd, -off if right else off, 200, right, rng.randrange(-3, 4), L), ("i:few", "i:half", "i:over")[which])
    # (ii) the first hard mismatch (or read N) of the best site lies in 64-base chunk c
    for c in range(1, 10):
        for rep in range(24):
            L = rng.choice([x for x in (65, 101, 127, 150, 151, 250, 301, 597, 598, 599, 600) if x > 64 * c])
            locus = flank(L)
            rd = bytearray(locus)
            p = rng.randrange(64 * c, min(64 * c + 64, L))
            rd[p] = ord("N") if rep % 2 else _other(rng, rd[p])
            for q in range(p + 1, L):                                    # later mismatches do not move the exit
                if rng.random() < 0.01:
                    rd[q] = _other(rng, rd[q])
            mam = 3 + sum(1 for x, y in zip(rd, locus) if x != y)
            if rep % 3 == 0 and p > 2:                                   # a reference N before it: counted, not an exit
                q = rng.randrange(0, p)
                locus[q] = ord("N")
                mam += 1
            right, off = rep % 4 < 2, rng.randrange(0, 130)
            place(locus, (rd, -off if right else off, 200, right, rng.randrange(-40, 41), mam), "ii:%d" % c)
    # (iii) two perfect copies at idealStart - d and idealStart + d: the read has period 2d and the repeat holds exactly two starts
    for d in (1, 31, 32, 33, 63, 64, 65):
        for rep in range(24):
            right = rep % 2 == 0
            L = rng.choice([x for x in (max(10, 4 * d + 1), 4 * d + 38, 301, 597, 600) if 4 * d < x <= 600])
            unit = _primitive_unit(rng, 2 * d)
            locus = bytearray((unit * (L // len(unit) + 3))[:L + 2 * d])
            before, after = flank(), flank()
            before[-1] = _other(rng, unit[-1])                           # the repeat does not go on into the flanks
            after[0] = _other(rng, (unit * (L // len(unit) + 3))[L + 2 * d])
            off = rng.randrange(0, 70)
            at = len(ref) + 260
            ref.extend(before + locus + after)
            loc, dist = (at - off, off + 2 * d + rng.randrange(0, 80)) if right else (at + 2 * d + off, off + 2 * d + rng.randrange(0, 80))
            # maxAllowedMismatches -1 admits perfect starts only; with more, a start that runs a base or two into the flank can
            # outscore both copies (its completed match run counts, a perfect site's does not)
            probs.append((bytes(locus[:L]), chrom, loc, dist, right, at + d, (-1, -1, 0, 3)[rep // 2 % 4]))
            fams.append("iii")
    # (iv) within one 64-start block: a site with m1 mismatches, then one with m2 < m1, then one with m3 in (m2, m1].  The read is
    # a repeat of period p <= 3, the reference the same repeat with substitutions that enter and leave the window as it slides.
    for rep in range(120):
        right = rep % 2 == 0
        p = rng.choice((1, 2, 3))
        delta = rng.choice((2, 3)) if p > 1 else rng.choice((2, 3, 4))
        x = rng.choice([v for v in range(1, 9) if delta <= p * v < 2 * delta])
        m2 = rng.choice((0, 1, 2)) if right else rng.choice((1, 2))
        m1 = m2 + delta
        m3 = rng.randrange(m2 + 1, m1 + 1)
        y = rng.choice([v for v in range(1, 9) if p * v >= m3 - m2])
        L = rng.choice((41, 63, 64, 65, 101, 127, 150, 151, 250, 301, 597, 600))
        unit = _primitive_unit(rng, p)
        span = L + p * (x + y)
        locus = bytearray((unit * (span // p + 2))[:span])
        rd = bytes((unit * (L // p + 2))[:L])
        before, after = flank(), flank()
        for i in range(8):                                               # eight bases that do not continue the repeat
            before[-1 - i] = _other(rng, unit[(-1 - i) % p])
            after[i] = _other(rng, unit[(span + i) % p])

        def sub(q):
            locus[q] = ord("N") if rng.random() < 0.2 else _other(rng, locus[q])
        if right:                                                        # starts a = 0, b = p x, c = p (x + y), visited in that order
            for q in range(delta):
                sub(q)                                                   # in window a only, at its very start
            for q in range(m2):
                sub(L - 1 - q)                                           # in all three, at the end of window a
            for q in range(m3 - m2):
                sub(span - 1 - q)                                        # in window c only, at its very end
            off = rng.randrange(0, 64 - p * (x + y))
            first, second, third = 0, p * x, p * (x + y)
            loc, ideal = -off, third + rng.randrange(0, 30)
        else:                                                            # starts a = p (x + y), b = p y, c = 0, visited in that order
            for q in range(delta):
                sub(span - 1 - q)                                        # in window a only, at its very end
            for q in range(m2):
                sub(L - 1 - q)                                           # in all three, at the end of window c
            for q in range(m3 - m2):
                sub(q)                                                   # in window c only, at its very start
            off = rng.randrange(0, 64 - p * (x + y))
            first, second, third = p * (x + y), p * y, 0
            loc, ideal = first + off, third - rng.randrange(0, 30)
        at = len(ref) + 260
        ref.extend(before + locus + after)
        probs.append((rd, chrom, at + loc, off + p * (x + y) + rng.randrange(0, 40), right, at + ideal, m1 - 1 + rng.randrange(0, 3)))
        fams.append("iv")
    # (v) a read that is all N, allowed and not allowed to mismatch everywhere
    for rep in range(24):
        L = lens[rep % len(lens)]
        right, off = rep % 2 == 0, rng.randrange(0, 100)
        place(flank(L), (b"N" * L, -off if right else off, rng.choice((0, 63, 64, 200)), right, rng.randrange(-50, 50),
                         rng.choice((L + 5, L, L - 1, L - 2, 3))), "v")
    # (vi) a read equal to the reference except for case
    for rep in range(24):
        L = lens[rep % len(lens)]
        locus = flank(L)
        for _ in range(rng.randrange(1, 4)):
            q, n = rng.randrange(L), rng.randrange(1, 40)
            locus[q:q + n] = bytes(locus[q:q + n]).lower()
        rd = bytes(locus).upper() if rep % 3 else bytes(locus).lower()
        if rd == bytes(locus):                                           # the stretches covered the whole locus
            rd = rd.swapcase()
        right, off = rep % 2 == 0, rng.randrange(0, 100)
        place(locus, (rd, -off if right else off, 200, right, rng.randrange(-50, 50), rng.choice((L, L // 4, 3, 0))), "vi")
    ref.extend(b"N" * 31)
    return bytes(ref), pad, probs, fams


def make_degenerate_problems(seed, chroms):
    """Jobs the kernel answers without a scan: too short, too long, no chromosome, empty window, chromosome shorter than the read."""
    rng = random.Random(seed + 17)
    ref = chroms[0]

    def cut(n):
        s = rng.randrange(100, len(ref) - 800)
        return ref[s:s + n], s
    probs = []
    for L in (9, 1, 0, 601, 700, 601, 700):
        b, s = cut(L)
        probs.append((b, 1, s - 20, 200, True, s, 5))
    for ch in (0, -1, 0, -1):
        b, s = cut(100)
        probs.append((b, ch, s - 20, 200, ch == 0, s, 5))
    b, s = cut(100)
    probs.append((b, 1, len(ref) - 50, 300, True, s, 5))                 # loc beyond reflen - len
    probs.append((b, 1, -400, 300, False, s, 5))                         # loc below minIndex, searching left
    probs.append((b, 1, -700, 300, True, s, 5))                          # the whole window below zero
    tiny = [k for k, c in enumerate(chroms) if len(c) < 100][0]
    probs.append((b, tiny + 1, 0, 200, True, 0, 100))                    # reflen < len
    probs.append((b, tiny + 1, 40, 200, False, 0, 100))
    return probs


def make_full_set(seed, n):
    """Edge jobs, planted families and degenerate jobs in one batch over one chromosome list, planted and degenerate jobs at
    random positions among the others.  Returns (chroms, min_index, probs, families); family "B" is an edge job, "D" degenerate."""
    chroms, min_index, edge = make_edge_problems(seed, n)
    pchrom, ppad, planted, pf = make_planted_problems(seed, len(chroms) + 1)
    chroms, min_index = chroms + [pchrom], min_index + [ppad]
    rng = random.Random(seed + 29)
    items = [(p, "B") for p in edge]
    for p, f in list(zip(planted, pf)) + [(p, "D") for p in make_degenerate_problems(seed, chroms)]:
        items.insert(rng.randrange(len(items) // 4, 3 * len(items) // 4), (p, f))
    return chroms, min_index, [i[0] for i in items], [i[1] for i in items]


def scanned(p):
    """Whether the kernel scans job p at all: it has a chromosome and a read of at most 600 bases (shorter than 10 scans nothing)."""
    return p[1] >= 1 and len(p[0]) <= 600
