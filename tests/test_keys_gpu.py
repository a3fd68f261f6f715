"""bbkeys_make_batch_device -- quickMap's key stage on the device -- against the host form bbkeys_make_batch on the same input: the read
records field by field, keyinfo[:used], the base scores and `used`, all with np.array_equal.  Inputs: tests/keys_problems.py (what
they exercise: tests/test_keys_problems.py) and the PhiX fixture's reads with their real qualities."""
import ctypes as C

import numpy as np
import pytest
import torch          # before the HIP library is first loaded, as bbmap_amd.mapper does: the process then runs on one HIP runtime

from bbmap_amd import _lib, keys as K
from bbmap_amd.index import READ_DTYPE
from tests import keys_problems as P

pytestmark = pytest.mark.gpu
E_ARG = -2
CANARY, CANARY8 = -1234567, 77


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device(recs, blob, qblob, cfg, **kw):
    """the device form over the host answer's layout: (recs, keyinfo[:used], baseScores) as numpy"""
    inp = np.zeros(len(recs), READ_DTYPE)
    inp["bases_off"], inp["len"] = recs["bases_off"], recs["len"]
    inp["keys_off"], inp["nkeys"] = -1, -1
    d_recs, d_ki, d_bs = K.make_batch_device(_t(inp.view(np.uint8).reshape(-1)), _t(blob), None if qblob is None else _t(qblob), cfg, **kw)
    return d_recs.cpu().numpy().view(READ_DTYPE), d_ki.cpu().numpy(), d_bs.cpu().numpy()


def _same(host, dev):
    recs, blob, bs, ki, used = host
    d_recs, d_ki, d_bs = dev
    for f in READ_DTYPE.names:
        assert np.array_equal(d_recs[f], recs[f]), f
    assert len(d_ki) == used
    assert np.array_equal(d_ki, ki)
    assert np.array_equal(d_bs[:len(blob)], bs[:len(blob)])


def _check(reads, quals, cfg):
    host = P.host(reads, quals, cfg)
    qblob = None if quals is None else (np.concatenate(quals) if len(quals) else np.zeros(1, np.uint8))
    _same(host, _device(host[0], host[1], qblob, cfg))
    return host


@pytest.mark.parametrize("use_q,semi", [(True, 0), (False, 0), (True, 1)])
def test_mixed_lengths(gpu_msa_lib, use_q, semi):
    reads, quals, profile = P.problem("mixed")
    host = P.host_answer("mixed", use_q, semi)
    cfg = K.default_config(profile, semiperfectMode=semi)
    _same(host, _device(host[0], host[1], np.concatenate(quals) if use_q else None, cfg))
    assert len(set(host[0]["nkeys"].tolist())) > (10 if use_q else 5)       # one count per length without qualities


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_partial_wavefronts(gpu_msa_lib, n):
    reads, quals, _ = P.problem("reads150")
    _check(reads[100:100 + n], quals[100:100 + n], K.default_config())


@pytest.mark.parametrize("lens", [[0], [12], [13], [14], [0, 12, 13, 14] * 40 + [14, 13, 12, 0, 0, 13]])
@pytest.mark.parametrize("use_q", [True, False])
def test_shorter_than_k_one_slot_two_slots(gpu_msa_lib, lens, use_q):
    reads, quals = P.make_reads(lens, 21)
    if len(lens) == 1:                     # the clean read: 13 bases give the one key at 0, 14 bases the two keys 0 and 1
        quals = [np.full(lens[0], 35, np.uint8)]
    recs = _check(reads, quals if use_q else None, K.default_config())[0]
    if len(lens) == 1:
        assert recs["nkeys"][0] == {0: 0, 12: 0, 13: 1, 14: 2}[lens[0]]


@pytest.mark.parametrize("use_q", [True, False])
def test_pacbio_profile(gpu_msa_lib, use_q):
    reads, quals, profile = P.problem("pacbio")
    host = P.host_answer("pacbio", use_q)
    _same(host, _device(host[0], host[1], np.concatenate(quals) if use_q else None, K.default_config(profile)))
    if not use_q:                          # tests/test_keys.py: ceil(6000 * 2.8 / 12) = 1400 keys, the last at 5988
        recs, ki = host[0], host[3]
        r = int(np.nonzero(recs["len"] == 6000)[0][0])
        o, n = int(recs["keys_off"][r]), int(recs["nkeys"][r])
        assert n == 1400 and ki[o] == 0 and ki[o + n - 1] == 5988 and set(ki[o + n:o + 2 * n].tolist()) == {1200}


@pytest.mark.parametrize("profile", [K.PROFILE_BBMAP, K.PROFILE_PACBIO])
def test_phix_reads_with_their_qualities(gpu_msa_lib, profile):
    from tests.golden_phix import fixture_inputs
    reads, quals, _ = fixture_inputs("pe", True)
    assert len(reads) == 200
    _check(reads, quals, K.default_config(profile))


def _raw(cfg, recs, bases, quality, keyinfo, cap, base_scores, ws, ws_bytes):
    L = _lib.load()
    used = C.c_int64(-5)
    rc = L.bbkeys_make_batch_device(C.byref(cfg), C.c_void_p(torch.cuda.current_stream().cuda_stream), recs.numel() // 24, recs.data_ptr(),
                                    bases.data_ptr(), quality.data_ptr(), keyinfo.data_ptr(), cap, base_scores.data_ptr(), ws.data_ptr(),
                                    ws_bytes, C.byref(used))
    return rc, used.value


def test_gaps_canaries_and_capacities(gpu_msa_lib):
    reads, quals, _ = P.problem("mixed")
    reads, quals = reads[:300], quals[:300]
    cfg = K.default_config()
    h_recs, _, h_bs, h_ki, used = P.host(reads, quals, cfg)
    assert used > 1000
    # the same reads with 0..9 unused bytes in front of each: bases_off is not the running sum
    rng = np.random.default_rng(5)
    lens = h_recs["len"].astype(np.int64)
    offs = np.cumsum(rng.integers(0, 10, len(reads)) + np.concatenate([[0], lens[:-1]]))
    total = int(offs[-1] + lens[-1]) + 9
    blob, qblob = np.full(total, ord("N"), np.uint8), np.zeros(total, np.uint8)
    inside = np.zeros(total, bool)
    for o, b, q in zip(offs, reads, quals):
        blob[o:o + len(b)], qblob[o:o + len(b)], inside[o:o + len(b)] = b, q, True
    recs = np.zeros(len(reads), READ_DTYPE)
    recs["bases_off"], recs["len"], recs["keys_off"], recs["nkeys"] = offs, lens, -1, -1
    need = K.workspace_bytes(cfg, len(reads), int(lens.sum()))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    d_blob, d_q = _t(blob), _t(qblob)

    def fresh(cap):
        return (_t(recs.view(np.uint8).reshape(-1)), torch.full((cap + 64,), CANARY, dtype=torch.int32, device="cuda"),
                torch.full((total,), CANARY8, dtype=torch.int8, device="cuda"))
    # keyinfo_cap == used succeeds; nothing at or beyond `used`, and no byte between the reads, is written
    d_recs, d_ki, d_bs = fresh(used)
    assert _raw(cfg, d_recs, d_blob, d_q, d_ki, used, d_bs, ws, need) == (0, used)
    ki, bs, out = d_ki.cpu().numpy(), d_bs.cpu().numpy(), d_recs.cpu().numpy().view(READ_DTYPE)
    assert np.array_equal(ki[:used], h_ki) and (ki[used:] == CANARY).all()
    assert (bs[~inside] == CANARY8).all()
    assert np.array_equal(bs[inside], h_bs[:int(lens.sum())])
    assert np.array_equal(out["keys_off"], h_recs["keys_off"]) and np.array_equal(out["nkeys"], h_recs["nkeys"])
    assert np.array_equal(out["bases_off"], offs) and np.array_equal(out["len"], h_recs["len"])
    # one int less: BBMAP_E_ARG, keyinfo untouched, the needed size reported
    d_recs, d_ki, d_bs = fresh(used)
    assert _raw(cfg, d_recs, d_blob, d_q, d_ki, used - 1, d_bs, ws, need) == (E_ARG, used)
    assert (d_ki.cpu().numpy() == CANARY).all()
    assert b"keyinfo" in _lib.load().bbmap_last_error()
    # a workspace one byte short
    d_recs, d_ki, d_bs = fresh(used)
    rc, _ = _raw(cfg, d_recs, d_blob, d_q, d_ki, used, d_bs, ws, need - 1)
    assert rc == E_ARG and b"workspace" in _lib.load().bbmap_last_error()
    assert (d_ki.cpu().numpy() == CANARY).all() and (d_bs.cpu().numpy() == CANARY8).all()
    # no reads
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    assert _raw(cfg, empty, d_blob, d_q, d_ki, used, d_bs, ws, need) == (0, 0)
    r0, k0, _ = K.make_batch_device(empty, d_blob, d_q, cfg)
    assert r0.numel() == 0 and k0.numel() == 0


@pytest.mark.parametrize("mode,profile", [("pe", K.PROFILE_BBMAP), ("se1", K.PROFILE_PACBIO)])
def test_mapper_from_reads_equals_from_records(gpu_msa_lib, mode, profile):
    from bbmap_amd.index import DeviceIndex
    from bbmap_amd.mapper import Mapper
    from tests.golden_phix import PACBIO_MSA, fixture_inputs, phix_reference
    reads, quals, paired = fixture_inputs(mode, True)
    kcfg = K.default_config(profile)
    kw = dict(paired=paired, max_sites=32, profile=profile)
    if profile == K.PROFILE_PACBIO:
        kw.update(msaMaxColumns=PACBIO_MSA["msaMaxColumns"], finalStage=1)
    di = DeviceIndex.build([phix_reference()], profile=profile)
    recs, blob, bs, ki = K.make_batch(reads, quals, kcfg)
    a = Mapper.from_records(di, recs, blob, bs, ki, **kw)
    a.step()
    want = a.fetch()
    a.close()
    b = Mapper.from_reads(di, [len(r) for r in reads], np.concatenate(reads), np.concatenate(quals), kcfg, **kw)
    assert np.array_equal(b.reads.cpu().numpy().view(READ_DTYPE), recs)
    b.step()
    got = b.fetch()
    b.close()
    di.close()
    assert (want["final"]["mapped"] == 1).sum() >= 0.9 * len(reads)
    _same_outputs(got, want)


def _final_strings(out):
    fin, blob = out["final"], out["final_match"]
    return [blob[int(f["match_off"]): int(f["match_off"]) + int(f["match_len"])].tobytes() if int(f["match_len"]) > 0 else None for f in fin]


def _same_outputs(a, b):
    """Two mappers' outputs are the same: site lists, every fill keyed by (read, seq), final records and match strings.  Where a fill
    or a string lands in its log or pool follows the order in which threads claim slots, so those positions are compared through what
    they point at."""
    from tests.mapper_check import FINAL_FIELDS, SITE_FIELDS, gpu_fills
    assert np.array_equal(a["nsites"], b["nsites"]) and "overflow" not in a and "overflow" not in b
    for r in range(len(a["nsites"])):
        n = max(int(a["nsites"][r]), 0)
        for f in SITE_FIELDS + ("gaps",):
            assert np.array_equal(a["sites"][r, :n][f], b["sites"][r, :n][f]), (r, f)
    fa, fb = gpu_fills(a), gpu_fills(b)
    assert fa.keys() == fb.keys()
    for k in fa:
        assert {x: v for x, v in fa[k].items() if x != "index"} == {x: v for x, v in fb[k].items() if x != "index"}, k
    for f in FINAL_FIELDS:
        assert np.array_equal(a["final"][f], b["final"][f]), f
    assert _final_strings(a) == _final_strings(b)
