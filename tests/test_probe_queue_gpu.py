"""GPU tests of the index probe kernels as persistent kernels: every wavefront (or lane) pulls read after read from the work
queue and reuses its LDS, workspace and registers between them.  BBIDX_MAX_GROUPS caps the grid, so that each wave probes
many reads in turn; reads that end early (shorter than k, no keys, no hit, list overflow, declined, N runs, long deletions)
are each followed by an ordinary read, whose result must not depend on what the wave did before.  Also: the long-read
kernel's batch-wide LDS layout, the size limits with their raw result codes (0 / -1 / -2), the 32-block limit, and what
bases_rc_out receives.  Every site list is compared field by field with the CPU oracle (OracleIndex; the mapPacBio build of
it for BBIDX_PROFILE_PACBIO)."""
import os

import numpy as np
import pytest

from bbmap_amd import keys as K
from bbmap_amd.index import HostIndex, DeviceIndex, PROFILE_PACBIO
from oracle.oracle import OracleIndex, make_offsets
from tests.index_problems import make_genome, make_reads, revcomp
from tests.test_index_gpu import _hard_reads
from tests.test_index_long_gpu import pacbio_piece

pytestmark = pytest.mark.gpu

CAPS = (1, 3, None)
PB_CFG = None


def _pb_cfg():
    global PB_CFG
    if PB_CFG is None:
        PB_CFG = K.default_config(K.PROFILE_PACBIO)
    return PB_CFG


def _make(factory, cap):
    """A context created with BBIDX_MAX_GROUPS = cap (None: unset); the variable is read once, at creation."""
    old = os.environ.pop("BBIDX_MAX_GROUPS", None)
    if cap is not None:
        os.environ["BBIDX_MAX_GROUPS"] = str(cap)
    try:
        return factory()
    finally:
        os.environ.pop("BBIDX_MAX_GROUPS", None)
        if old is not None:
            os.environ["BBIDX_MAX_GROUPS"] = old


def _expect(oi, reads, max_sites, skip=()):
    """The oracle's lists and codes: (lists, codes) with None / -1 where the list overflows max_sites; reads in `skip` (ones
    the device declines and the oracle does not restate, such as descending key offsets) get None / -2."""
    lists, codes = [], []
    for i, r in enumerate(reads):
        if i in skip:
            lists.append(None)
            codes.append(-2)
            continue
        try:
            e = oi.find(r[0], revcomp(r[0]), r[1], r[2], r[3], cap=max_sites)
            lists.append(e)
            codes.append(len(e))
        except RuntimeError:
            lists.append(None)
            codes.append(-1)
    return lists, np.array(codes, np.int32)


def _check(got, ns, exp, codes, what, declined=()):
    """Device = oracle, read by read; `declined` reads must come back -2 instead."""
    for i in range(len(exp)):
        if i in declined:
            assert ns[i] == -2 and got[i] is None, "%s: read %d must be declined (-2), got %d" % (what, i, ns[i])
            continue
        assert ns[i] == codes[i], "%s: read %d: nsites %d, oracle %d" % (what, i, ns[i], codes[i])
        assert got[i] == exp[i], "%s: read %d: %s != %s" % (what, i, got[i], exp[i])


def _spread_offsets(length, k, n):
    """n ascending key offsets spread over a read of `length` bases."""
    offs = np.linspace(0, length - k, n).astype(np.int64)
    assert len(set(offs.tolist())) == n
    return offs.tolist()


def _pb_read(bp, offs=None):
    """(bases, baseScores, keyScores, offsets) with keys placed by bbkeys_make, or at the given offsets."""
    o, ks, bs = K.make_keys(bp, None, _pb_cfg())
    if offs is not None:
        o, ks = list(offs), [1200] * len(offs)
    return (bp, bs.tolist(), list(ks), list(o))


def _repeat_chrom(seed, families=2, copies=60, length=2500, div=0.03):
    """Many diverged copies of a few families: pieces drawn from it have dozens of candidate sites."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    fam = [rng.choice(acgt, length) for _ in range(families)]
    body = []
    for i in range(copies):
        cp = fam[i % families].copy()
        hit = rng.random(len(cp)) < div
        cp[hit] = rng.choice(acgt, int(hit.sum()))
        body += [cp, rng.choice(acgt, int(rng.integers(100, 800)))]
    return b"N" * 3000 + np.concatenate(body).tobytes() + b"N" * 3000


# ------------------------------------------------------------------------------------------------ BBMap profile problems
def _bbmap_problem():
    """Ordinary and hard reads, with the reads that end early interleaved, each followed by an ordinary read."""
    import random
    genomes = [make_genome(31, 250000), make_genome(32, 120000), _repeat_chrom(35, copies=40, length=800)]
    k = 13
    rng = random.Random(11)
    plain = [(r[0], r[2], r[3], r[4]) for r in make_reads(7, genomes, 220, k=k) + _hard_reads(33, genomes, 60, k)]
    G = genomes[0]

    def piece(L, st=None):
        st = rng.randrange(600, len(G) - L - 1200) if st is None else st
        return bytes(G[st:st + L])

    def plain_read(bp, density=1.9):
        offs = make_offsets(len(bp), k, density)
        return (bp, [0] * len(bp), [100 * k] * len(offs), offs)

    special, size_declined = [], []
    special.append(("short", (b"ACGTACGTAC", [0] * 10, [], [])))
    special.append(("no keys", (piece(150), [0] * 150, [], [])))
    special.append(("no hit", plain_read(bytes(rng.choice(b"ACGT") for _ in range(150)))))
    for _ in range(3):
        bp = bytearray(piece(150))
        p = rng.randrange(30, 100)
        bp[p:p + 12] = b"N" * 12
        special.append(("N run", plain_read(bytes(bp))))
    for _ in range(3):
        st = rng.randrange(600, len(G) - 2000)
        bp = bytes(G[st:st + 70] + G[st + 70 + rng.randint(300, 600):][:80])
        special.append(("long deletion", plain_read(bp)))
    bp = piece(600)
    special.append(("128 keys", (bp, [0] * 600, [100 * k] * 128, _spread_offsets(600, k, 128))))
    special.append(("600 bases", plain_read(piece(600))))
    bp = piece(600)
    special.append(("129 keys", (bp, [0] * 600, [100 * k] * 129, _spread_offsets(600, k, 129))))
    special.append(("601 bases", plain_read(piece(601))))
    # reads with many sites: repeat-family members overflow a small list
    special += [("repeat", (r[0], r[2], r[3], r[4])) for r in make_reads(8, genomes[2:], 12, k=k)]
    reads, followers = [], []
    pi = 0
    for name, r in special:
        if name in ("129 keys", "601 bases"):
            size_declined.append(len(reads))
        reads.append(r)
        followers.append(len(reads))
        reads.append(plain[pi])
        pi += 1
    reads += plain[pi:]
    return genomes, k, reads, followers, set(size_declined)


@pytest.fixture(scope="module")
def bbmap_problem():
    genomes, k, reads, followers, declined = _bbmap_problem()
    hi = HostIndex(genomes, k=k)
    oi = OracleIndex(genomes, k=k)
    max_sites = 12
    exp, codes = _expect(oi, reads, max_sites)
    assert (codes == -1).sum() >= 3 and (codes > 0).sum() > 200          # the overflow and the ordinary paths both run
    return dict(hi=hi, oi=oi, reads=reads, followers=followers, declined=declined, exp=exp, codes=codes, max_sites=max_sites)


BBMAP_ROUTES = [("auto", "0", 160), ("auto", "0", 600), ("auto", "1", 160), ("auto", "1", 600), ("lane", None, 600), ("long", None, 600)]


@pytest.mark.parametrize("kind,variant,maxlen", BBMAP_ROUTES)
def test_many_reads_per_wave_bbmap_profile(bbmap_problem, kind, variant, maxlen):
    P = bbmap_problem
    reads = P["reads"]
    declined = P["declined"] if kind != "long" else ()          # the long-read kernel takes BBMap-profile reads of any size here
    results = {}
    old = os.environ.pop("BBIDX_LONG_LISTS", None)
    try:
        if variant is not None:
            os.environ["BBIDX_LONG_LISTS"] = variant
        for cap in CAPS:
            di = _make(lambda: DeviceIndex(P["hi"]), cap)
            di.set_kernel(kind)
            di.set_max_read_len(maxlen)
            got, ns = di.find_batch(reads, max_sites=P["max_sites"], codes=True)
            ll = di.last_launch()
            what = "%s kernel (long lists %r, max len %d) at BBIDX_MAX_GROUPS %s" % (kind, variant, maxlen, cap)
            _check(got, ns, P["exp"], P["codes"], what, declined)
            if kind == "auto":
                assert ll["wave_groups"] >= 1 and ll["long_lists"] == int(variant) and ll["short_reads"] == int(maxlen <= 160), (what, ll)
                assert ll["pending"] >= 1 and ll["long_groups"] == 0, (what, ll)      # > 64 keys: the per-lane kernel ran too
            elif kind == "lane":
                assert ll["wave_groups"] == 0 and ll["long_groups"] == 0 and ll["pending"] == 0, (what, ll)
            else:
                assert ll["wave_groups"] == 0 and ll["lane_groups"] == 0 and ll["max_len"] == 601 and ll["max_keys"] == 129, (what, ll)
            groups = ll["long_groups"] if kind == "long" else ll["lane_groups"]
            if cap is None:
                assert groups > 3 and (kind != "auto" or ll["wave_groups"] > 3), (what, ll)
            else:
                assert groups == cap and (kind != "auto" or ll["wave_groups"] == cap), (what, ll)
            results[cap] = (got, ns.copy())
            di.close()
        for cap in CAPS[:-1]:
            assert np.array_equal(results[cap][1], results[None][1]) and results[cap][0] == results[None][0]
        # each read that follows one that ended early: the same result when probed on its own
        di = _make(lambda: DeviceIndex(P["hi"]), 1)
        di.set_kernel(kind)
        di.set_max_read_len(maxlen)
        for i in P["followers"]:
            g, ns = di.find_batch([reads[i]], max_sites=P["max_sites"], codes=True)
            assert ns[0] == results[1][1][i] and g[0] == results[1][0][i], "follower %d alone" % i
        di.close()
    finally:
        os.environ.pop("BBIDX_LONG_LISTS", None)
        if old is not None:
            os.environ["BBIDX_LONG_LISTS"] = old


# ------------------------------------------------------------------------------------------------ PacBio profile problems
@pytest.fixture(scope="module")
def pacbio_index():
    genomes = [make_genome(81, 400000), make_genome(82, 250000), _repeat_chrom(83, div=0.003)]
    return genomes, OracleIndex(genomes, profile="pacbio")


def _pb_build(genomes, cap):
    return _make(lambda: DeviceIndex.build(genomes, profile=PROFILE_PACBIO), cap)


def _pb_pieces(genomes, rng, n, lo, hi, strand_mix=True, err=(0.10, 0.16)):
    out = []
    for i in range(n):
        G = genomes[int(rng.integers(0, len(genomes)))]
        rd, st = pacbio_piece(rng, G, lo, hi, err=err)
        bp = revcomp(rd) if (strand_mix and i & 1) else rd
        out.append(_pb_read(bp))
    return out


def _pb_problem(genomes):
    rng = np.random.default_rng(17)
    G = genomes[0]
    plain = _pb_pieces(genomes, rng, 60, 200, 2600)
    k = 12
    special = []
    special.append(("length k - 1", (bytes(G[5000:5011]), [0] * 11, [], [])))
    special.append(("length k", _pb_read(bytes(G[5000:5012]))))
    special.append(("no keys", (bytes(G[9000:9800]), [0] * 800, [], [])))
    special.append(("one key", _pb_read(bytes(G[12000:12600]), offs=[250])))
    special.append(("no hit", _pb_read(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 900)))))
    for j in range(3):
        rd, _ = pacbio_piece(rng, G, 600, 1500, err=(0.02, 0.05))
        rd = bytearray(rd)
        p = int(rng.integers(100, len(rd) - 200))
        rd[p:p + 30] = b"N" * 30
        special.append(("N run", _pb_read(bytes(rd))))
    for j in range(3):
        st = int(rng.integers(2000, len(G) - 9000))
        rd = bytes(G[st:st + 700] + G[st + 700 + int(rng.integers(300, 700)):][:800])
        special.append(("long deletion", _pb_read(rd)))
    bp = bytes(G[20000:27000])
    special.append(("6017 bases", _pb_read(bp[:6017])))
    special.append(("2048 keys", _pb_read(bp[:5000], offs=_spread_offsets(5000, k, 2048))))
    r = _pb_read(bp[:1500])
    special.append(("descending offsets", (r[0], r[1], r[2], r[3][:40] + r[3][40:80][::-1] + r[3][80:])))
    special += [("repeat", x) for x in _pb_pieces([genomes[2]], rng, 6, 300, 900, err=(0.01, 0.03))]
    reads, followers, declined = [], [], set()
    for i, (name, r) in enumerate(special):
        if name in ("6017 bases", "2048 keys", "descending offsets"):
            declined.add(len(reads))
        reads.append(r)
        followers.append(len(reads))
        reads.append(plain[i])
    reads += plain[len(special):]
    return reads, followers, declined


def test_many_reads_per_wave_pacbio_profile(pacbio_index):
    genomes, oi = pacbio_index
    reads, followers, declined = _pb_problem(genomes)
    max_sites = 24
    exp, codes = _expect(oi, reads, max_sites, skip=declined)
    assert (codes > 0).sum() > 40 and (codes == -1).sum() >= 2
    results = {}
    for cap in CAPS:
        di = _pb_build(genomes, cap)
        got, ns = di.find_batch(reads, max_sites=max_sites, codes=True)
        ll = di.last_launch()
        what = "PacBio profile at BBIDX_MAX_GROUPS %s" % cap
        _check(got, ns, exp, codes, what, declined)
        assert ll["wave_groups"] == 0 and ll["lane_groups"] == 0, ll
        assert ll["max_len"] == 6016 and ll["max_keys"] == 2047, ll             # beyond the largest shape: clamped, and declined
        assert ll["long_groups"] == cap if cap else ll["long_groups"] > 3, (what, ll)
        results[cap] = (got, ns.copy())
        if cap == 1:
            for i in followers:
                g, n1 = di.find_batch([reads[i]], max_sites=max_sites, codes=True)
                assert n1[0] == ns[i] and g[0] == got[i], "follower %d alone" % i
        di.close()
    for cap in CAPS[:-1]:
        assert np.array_equal(results[cap][1], results[None][1]) and results[cap][0] == results[None][0]


def test_pacbio_batch_larger_than_the_resident_waves(pacbio_index):
    genomes, oi = pacbio_index
    rng = np.random.default_rng(23)
    reads = _pb_pieces(genomes, rng, 2600, 200, 900)
    exp, codes = _expect(oi, reads, 32)
    di = _pb_build(genomes, None)
    got, ns = di.find_batch(reads, max_sites=32, codes=True)
    ll = di.last_launch()
    assert 1 <= ll["long_groups"] < len(reads), ll                               # waves really took several pieces each
    _check(got, ns, exp, codes, "uncapped PacBio batch")
    di.close()


def _composition_set(genomes):
    rng = np.random.default_rng(29)
    S = _pb_pieces(genomes, rng, 40, 200, 900)
    G = genomes[1]
    big = _pb_read(bytes(G[30000:36016]), offs=_spread_offsets(6016, 12, 2047))
    over = _pb_read(bytes(G[40000:44500]), offs=_spread_offsets(4500, 12, 2048))
    return S, big, over


def test_long_kernel_batch_composition(pacbio_index):
    """The long kernel sizes its LDS layout by the batch's longest read and largest key count: a read's result must not
    depend on the other reads of its batch."""
    genomes, oi = pacbio_index
    S, big, over = _composition_set(genomes)
    n = len(S)
    exp, codes = _expect(oi, S + [big], 64)
    for cap in (2, None):
        di = _pb_build(genomes, cap)
        g0, n0 = di.find_batch(S, max_sites=64, codes=True)
        l0 = di.last_launch()
        g1, n1 = di.find_batch(S + [big], max_sites=64, codes=True)
        l1 = di.last_launch()
        g2, n2 = di.find_batch(S + [over], max_sites=64, codes=True)
        l2 = di.last_launch()
        _check(g1, n1, exp, codes, "S + 6016 bases / 2047 keys, cap %s" % cap)
        assert n2[n] == -2 and g2[n] is None
        for g, ns in ((g0, n0), (g2, n2)):
            assert np.array_equal(ns[:n], n1[:n]) and g[:n] == g1[:n]
        assert l0["max_len"] == max(len(r[0]) for r in S) and l0["max_keys"] == max(len(r[3]) for r in S), l0
        assert (l1["max_len"], l1["max_keys"]) == (6016, 2047), l1
        assert (l2["max_len"], l2["max_keys"]) == (4500, 2047), l2
        if cap:
            assert l0["long_groups"] == l1["long_groups"] == l2["long_groups"] == cap
        di.close()


def test_one_context_across_batches_of_different_shapes(pacbio_index):
    genomes, oi = pacbio_index
    S, big, _ = _composition_set(genomes)
    di = _pb_build(genomes, 3)
    a = di.find_batch(S, max_sites=64, codes=True)
    b = di.find_batch(S[:20] + [big] + S[20:], max_sites=64, codes=True)
    c = di.find_batch(S, max_sites=64, codes=True)
    assert np.array_equal(a[1], c[1]) and a[0] == c[0]
    assert np.array_equal(np.delete(b[1], 20), a[1]) and b[0][:20] + b[0][21:] == a[0]
    exp, codes = _expect(oi, S, 64)
    _check(a[0], a[1], exp, codes, "reused context")
    di.close()


# ------------------------------------------------------------------------------------------------ limits
def test_pacbio_size_limits_and_codes(pacbio_index):
    genomes, oi = pacbio_index
    G = genomes[0]
    bp = bytes(G[50000:57000])
    accepted = [_pb_read(bp[:6016]), _pb_read(bp[:6016], offs=_spread_offsets(6016, 12, 2047)),
                _pb_read(bp[1000:1700], offs=[300]), _pb_read(bp[2000:2012])]
    assert len(accepted[0][3]) > 1000 and len(accepted[3][3]) == 1
    r = _pb_read(bp[:3000])
    rejected = [(_pb_read(bp[:6017]), -2), (_pb_read(bp[:6000], offs=_spread_offsets(6000, 12, 2048)), -2),
                ((bp[:11], [0] * 11, [], []), 0), ((bp[:900], [0] * 900, [], []), 0),
                ((r[0], r[1], r[2], r[3][::-1]), -2)]
    assert len(rejected[0][0][3]) <= 2047
    exp, codes = _expect(oi, accepted, 64)
    for cap in (1, None):
        di = _pb_build(genomes, cap)
        got, ns = di.find_batch(accepted + [x for x, _ in rejected], max_sites=64, codes=True)
        _check(got[:len(accepted)], ns[:len(accepted)], exp, codes, "PacBio accepted, cap %s" % cap)
        assert ns[len(accepted):].tolist() == [c for _, c in rejected], ns
        di.close()


def test_bbmap_size_limits_and_codes():
    genomes = [make_genome(34, 150000)]
    k = 13
    hi = HostIndex(genomes, k=k)
    oi = OracleIndex(genomes, k=k)
    G = genomes[0]
    mk = lambda bp, offs: (bp, [0] * len(bp), [100 * k] * len(offs), offs)
    at = [mk(bytes(G[3000:3600]), _spread_offsets(600, k, 128)), mk(bytes(G[5000:5600]), make_offsets(600, k, 1.9))]
    over = [mk(bytes(G[3000:3600]), _spread_offsets(600, k, 129)), mk(bytes(G[5000:5601]), make_offsets(601, k, 1.9))]
    exp, codes = _expect(oi, at + over, 64)
    di = DeviceIndex(hi)
    for kind in ("auto", "lane", "long"):
        di.set_kernel(kind)
        got, ns = di.find_batch(at + over, max_sites=64, codes=True)
        _check(got, ns, exp, codes, "%s kernel at the BBMap limits" % kind, declined={2, 3} if kind != "long" else ())
    di.close()


def _many_chromosomes(n):
    return [make_genome(200 + i, 3000, pad=300) for i in range(n)]


@pytest.mark.parametrize("nchroms", [32, 33])
def test_32_block_limit(nchroms):
    """chromBits 0: one index block per chromosome; the prescan keeps 64 strand cycles, so 32 blocks are the most a read is
    probed over, and the 33rd declines every read (-2) in every kernel."""
    genomes = _many_chromosomes(nchroms)
    k = 10
    reads = [(r[0], r[2], r[3], r[4]) for r in make_reads(41, genomes, 80, k=k)]
    oi = OracleIndex(genomes, k=k, chromBits=0)
    exp, codes = _expect(oi, reads, 48)
    assert (codes > 0).sum() > 40
    declined = set(range(len(reads))) if nchroms > 32 else ()
    hi = HostIndex(genomes, k=k, chromBits=0)
    assert hi.nblocks == nchroms + 1
    di = DeviceIndex(hi)
    for kind in ("auto", "lane", "long"):
        di.set_kernel(kind)
        got, ns = di.find_batch(reads, max_sites=48, codes=True)
        _check(got, ns, exp, codes, "%s kernel, %d chromosomes" % (kind, nchroms), declined)
    di.close()
    pb = DeviceIndex.build(genomes, k=k, chromBits=0, profile=PROFILE_PACBIO)
    opb = OracleIndex(genomes, k=k, chromBits=0, profile="pacbio")
    exp, codes = _expect(opb, reads, 48)
    got, ns = pb.find_batch(reads, max_sites=48, codes=True)
    _check(got, ns, exp, codes, "PacBio profile, %d chromosomes" % nchroms, declined)
    pb.close()


@pytest.mark.parametrize("cap", [1, 2, 8])
def test_overflow_code_exactly_when_the_oracle_overflows(pacbio_index, cap):
    """Repeat-heavy pieces (and ordinary ones between them): nsites = -1 exactly where the oracle's list overflows max_sites."""
    genomes, oi = pacbio_index
    rng = np.random.default_rng(31)
    reads = [x for pair in zip(_pb_pieces([genomes[2]], rng, 30, 300, 1500, err=(0.01, 0.05)), _pb_pieces(genomes[:2], rng, 30, 300, 1500)) for x in pair]
    exp, codes = _expect(oi, reads, cap)
    assert (codes == -1).sum() >= 10 and (codes >= 0).sum() >= 10
    for groups in (1, None):
        di = _pb_build(genomes, groups)
        got, ns = di.find_batch(reads, max_sites=cap, codes=True)
        _check(got, ns, exp, codes, "max_sites %d, BBIDX_MAX_GROUPS %s" % (cap, groups))
        di.close()


# ------------------------------------------------------------------------------------------------ bases_rc_out
SENTINEL = 0xA5


def _check_rc(reads, ns, rc, k, size_declined, what):
    off = 0
    written = np.zeros(len(rc), bool)
    for i, (bp, bs, ks, offs) in enumerate(reads):
        L = len(bp)
        seg = rc[off:off + L]
        want = np.frombuffer(revcomp(bp), np.uint8)
        if L < k or len(offs) == 0 or i in size_declined:
            assert (seg == SENTINEL).all(), "%s: read %d (%d bases, %d keys, nsites %d) was written" % (what, i, L, len(offs), ns[i])
        elif ns[i] >= -1:
            assert np.array_equal(seg, want), "%s: read %d (nsites %d): wrong reverse complement" % (what, i, ns[i])
        else:
            assert (seg == SENTINEL).all() or np.array_equal(seg, want), "%s: read %d (nsites %d)" % (what, i, ns[i])
        written[off:off + L] = True
        off += L
    assert (rc[~written] == SENTINEL).all(), "%s: bytes outside the reads were written" % what


def test_rc_buffer_bbmap_kernels(bbmap_problem):
    P = bbmap_problem
    reads = P["reads"]
    for kind in ("auto", "lane", "long"):
        for cap in (1, None):
            di = _make(lambda: DeviceIndex(P["hi"]), cap)
            di.set_kernel(kind)
            got, ns, rc = di.find_batch_rc(reads, max_sites=P["max_sites"])
            declined = P["declined"] if kind != "long" else set()
            _check(got, ns, P["exp"], P["codes"], "%s kernel with bases_rc_out" % kind, declined)
            _check_rc(reads, ns, rc, 13, declined, "%s kernel, cap %s" % (kind, cap))
            di.close()


def test_rc_buffer_pacbio(pacbio_index):
    genomes, oi = pacbio_index
    reads, followers, declined = _pb_problem(genomes)
    size_declined = {i for i in declined if len(reads[i][0]) > 6016 or len(reads[i][3]) > 2047}
    assert len(size_declined) == 2
    exp, codes = _expect(oi, reads, 24, skip=declined)
    for cap in (1, None):
        di = _pb_build(genomes, cap)
        got, ns, rc = di.find_batch_rc(reads, max_sites=24)
        _check(got, ns, exp, codes, "PacBio with bases_rc_out", declined)
        _check_rc(reads, ns, rc, 12, size_declined, "PacBio, cap %s" % cap)
        di.close()
