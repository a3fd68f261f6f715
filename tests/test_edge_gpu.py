"""GPU tests of the boundary's edge behaviour: empty batches, bad arguments, shapes outside the limits."""
import ctypes as C

import numpy as np
import pytest

from bbmap_amd import _lib
from bbmap_amd import msa as M
from bbmap_amd.index import DeviceIndex
from bbmap_amd.rescue import quick_rescue_batch

pytestmark = pytest.mark.gpu


def test_empty_batches_are_fine():
    al = M.MultiStateAligner11ts(maxRows=64, maxColumns=128)
    assert al.align([]) == []
    assert al.alignGapped([]) == []
    assert quick_rescue_batch([], [b"ACGT" * 100]) == []
    di = DeviceIndex.build([b"N" * 50 + b"ACGTTGCA" * 200 + b"N" * 50], k=10)
    assert di.find_batch([]) == []
    di.close()


def test_bad_shapes_are_reported_not_computed():
    al = M.MultiStateAligner11ts(maxRows=64, maxColumns=128)
    ref = bytes(np.random.default_rng(1).choice(list(b"ACGT"), 1000).astype(np.uint8))
    too_long_read = (ref[100:180], ref, 96, 190, 1000)                 # 80 rows > maxRows
    too_wide = (ref[100:150], ref, 96, 400, 1000)                      # 305 columns > maxColumns, no clamp flag
    with pytest.raises(ValueError):
        al.align([too_long_read], M.FILL_LIMITED | M.DO_SCORE)
    with pytest.raises(ValueError):
        al.align([too_wide], M.FILL_LIMITED | M.DO_SCORE)
    # gapped jobs: odd gap arrays, gaps outside the reference, gaps shorter than the reference's minimum
    read = ref[100:150]
    bad = [(read, ref, 96, 760, 500, [100, 120, 700]),                 # odd count
           (read, ref, 96, 760, 500, [100, 120, 700, 2000]),           # beyond the reference array
           (read, ref, 96, 400, 500, [100, 120, 150, 400])]            # a 29-base "gap"
    got = al.alignGapped(bad)
    assert [g["status"] for g in got] == [M.ST_BAD_SHAPE] * 3
    assert all(g["score"] is None for g in got)


def test_index_build_rejects_bad_geometry_and_handles_tiny_chromosomes():
    with pytest.raises(_lib.BBMapAmdError):
        DeviceIndex.build([b"ACGT" * 100], k=7)
    with pytest.raises(_lib.BBMapAmdError):
        DeviceIndex.build([b"ACGT" * 100], k=16)
    # a chromosome shorter than k contributes nothing; an all-N chromosome neither
    di = DeviceIndex.build([b"ACGTAC", b"N" * 500, b"N" * 20 + b"ACGTTGCATGCATTGACCAGT" * 40 + b"N" * 20], k=11, chromBits=2)
    starts, sites, counts, hist = di.export_block(0)
    assert starts[-1] == len(sites) and len(sites) > 0
    assert ((sites >> (31 - 2)) == 3).all()                             # every entry belongs to chromosome 3
    # a read without a single defined k-mer has no site; a key offset that does not fit its read is an argument error
    assert di.find_batch([(b"N" * 60, [0] * 60, [1100, 1100], [0, 49])]) == [[]]
    with pytest.raises(_lib.BBMapAmdError):
        di.find_batch([(b"ACGTAC", [0] * 6, [1100], [0])])
    # the read-length announcement is a sizing hint: nonsense is refused, and a read longer than announced is still answered
    with pytest.raises(_lib.BBMapAmdError):
        di.set_max_read_len(0)
    rd = (b"ACGTTGCATGCATTGACCAGT" * 40)[5:205]
    offs = list(range(0, 190, 9))
    di.set_max_read_len(600)
    want = di.find_batch([(rd, [0] * len(rd), [1100] * len(offs), offs)])
    di.set_max_read_len(100)
    assert di.find_batch([(rd, [0] * len(rd), [1100] * len(offs), offs)]) == want
    di.close()


def test_rescue_edges():
    ref = bytes(np.random.default_rng(2).choice(list(b"ACGT"), 3000).astype(np.uint8))
    probs = [(ref[1000:1009], 1, 900, 300, True, 1000, 2),              # shorter than 10 bases: never rescued
             (ref[1000:1700], 1, 900, 300, True, 1000, 2),              # longer than the kernel's 600: reported, not computed
             (ref[1000:1100], 1, 2950, 300, True, 1000, 2),             # search range empty after clipping to the chromosome
             (ref[1000:1100], 1, 990, 0, True, 1000, 2)]                # searchDist 0, start not at loc
    got = quick_rescue_batch(probs, [ref])
    assert got == [None, None, None, None]
    assert quick_rescue_batch([(ref[1000:1100], 1, 1000, 0, True, 1000, 2)], [ref])[0]["start"] == 1000


def _complement_table():
    """AminoAcid.baseToComplementExtended restated: the reference's pairs (it pairs S with W), both cases, U -> A, five symbols
    that stay, and its fill of -1 (0xFF as a byte) everywhere else.  Java's table has 128 entries and an index of 128 or more
    would throw there; the project answers 0xFF for those too."""
    t = np.full(256, 0xFF, np.uint8)
    for a, b in ("AT", "CG", "MK", "RY", "SW", "VB", "HD", "NN", "XX"):
        for x, y in ((a, b), (b, a)):
            t[ord(x)], t[ord(x.lower())] = ord(y), ord(y.lower())
    t[ord("U")], t[ord("u")] = ord("A"), ord("a")
    for c in "? -*.":
        t[ord(c)] = ord(c)
    assert int((t[:128] != 0xFF).sum()) == 16 * 2 + 2 + 5
    return t


def test_revcomp_kernel():
    """bbpipe_revcomp_device against the complement table restated above, over every byte value.  Bytes of 128 and above map
    to 0xFF: that is the project's own answer, the Java would throw.  Lengths around the 64-lane stride, 1, 3, 4, 5 and 11 reads
    per launch (four waves per block), unaligned offsets, and canaries around every read of the output blob."""
    import torch
    from bbmap_amd.index import READ_DTYPE
    L = _lib.load()
    rng = np.random.default_rng(5)
    table = _complement_table()
    all_lens = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 6019]
    cases = [[n] for n in all_lens] + [all_lens[:3], all_lens[3:7], all_lens[6:], all_lens[::-1]]
    assert sorted({len(c) for c in cases}) == [1, 3, 4, 5, 11]
    dev = torch.device("cuda", 0)
    CANARY = 0xC3                                                           # not a value the table produces
    assert CANARY not in table.tolist()
    residues = set()
    for ci, lens in enumerate(cases):
        offs, pos = [], 0
        for i, n in enumerate(lens):
            pos += 1 + (5 * i + 3 * ci) % 13                                # canary bytes in front of every read
            offs.append(pos)
            pos += n
        total = pos + 37                                                    # and after the last one
        blob = np.full(total, CANARY, np.uint8)
        inside = np.zeros(total, bool)
        for off, n in zip(offs, lens):
            rd = rng.integers(0, 256, n).astype(np.uint8)
            if n >= 256:
                rd[:256] = rng.permutation(256)                             # every byte value, whatever the draw
            blob[off:off + n] = rd
            inside[off:off + n] = True
            residues.add(off % 16)
        recs = np.zeros(len(lens), READ_DTYPE)
        recs["bases_off"] = offs; recs["len"] = lens
        t_in = torch.from_numpy(blob).to(dev)
        t_out = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
        t_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
        _lib.check(L.bbpipe_revcomp_device(None, len(lens), t_recs.data_ptr(), t_in.data_ptr(), t_out.data_ptr()), "bbpipe_revcomp_device")
        out = t_out.cpu().numpy()
        for off, n in zip(offs, lens):
            assert (out[off:off + n] == table[blob[off:off + n][::-1]]).all(), (lens, off, n)
        assert (out[~inside] == CANARY).all(), lens                          # between the reads and after the last
        assert (t_in.cpu().numpy() == blob).all()
    assert len(residues) >= 12                                              # read offsets are not aligned to anything
    # byte values 0..255 one by one, in a read of their own
    blob = np.arange(256, dtype=np.uint8)
    recs = np.zeros(1, READ_DTYPE)
    recs["bases_off"] = 0; recs["len"] = 256
    t_in = torch.from_numpy(blob).to(dev); t_out = torch.zeros_like(t_in)
    t_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
    _lib.check(L.bbpipe_revcomp_device(None, 1, t_recs.data_ptr(), t_in.data_ptr(), t_out.data_ptr()), "bbpipe_revcomp_device")
    out = t_out.cpu().numpy()[::-1]
    assert out.tolist() == table.tolist()
    assert (out[128:] == 0xFF).all()
    comp = {ord(a): ord(b) for a, b in zip("ACGTNacgtnRYKM-", "TGCANtgcanYRMK-")}      # the pairs this test began with
    assert all(out[a] == b for a, b in comp.items())
