"""bench.py's host side: which legs a plain run leaves out, the threaded input generators (same bytes as one thread), and what
--dump-outputs writes."""
import numpy as np
import pytest

import bench as B
from bbmap_amd.mapper import FINAL_DTYPE, MSITE_DTYPE
from bbmap_amd import workload as W


def test_plain_run_leaves_the_extra_legs_out():
    a = B.parse_args(["--steps", "3", "--warmup", "1"])
    assert (a.steps, a.warmup, a.full) == (3, 1, False)
    assert a.no_cpu_baseline and a.parity_sample == 0 and a.stream_steps == 0 and a.default_set_steps == 0
    f = B.parse_args(["--full"])
    assert not f.no_cpu_baseline and (f.parity_sample, f.stream_steps, f.default_set_steps) == (600, 10, 3)
    g = B.parse_args(["--full", "--no-cpu-baseline", "--parity-sample", "0", "--stream-steps", "0"])
    assert g.no_cpu_baseline and g.parity_sample == 0 and g.stream_steps == 0 and g.default_set_steps == 3
    assert B.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    with pytest.raises(SystemExit):
        B.parse_args(["--steps", "0"])


@pytest.mark.parametrize("paired", [True, False])
def test_threaded_inputs_equal_one_thread(monkeypatch, paired):
    lens = [60000, 45000, 30000]
    chroms, path = B.shared_reference("t", lens, 0.1, 0, 1)
    assert path is None
    fam = max(50, 2000 // len(lens))
    for i, c in enumerate(chroms):
        assert np.array_equal(c, W.make_reference(lens[i], seed=38 + i, repeat_frac=0.1, families=fam))
    many, truth = B.make_batch(chroms, 3000, paired, 4, with_truth=True)
    monkeypatch.setattr(B, "usable_cores", lambda: 1)
    one, truth1 = B.make_batch(chroms, 3000, paired, 4, with_truth=True)
    assert np.array_equal(many, one)
    assert truth.keys() == truth1.keys() and all(np.array_equal(truth[k], truth1[k]) for k in truth)


def _fake_output(n, cap, rng):
    sites = np.zeros((n, cap), MSITE_DTYPE)
    for f in ("chrom", "start", "stop", "score", "slowScore"):
        sites[f] = rng.integers(0, 250_000_000, size=(n, cap))
    nsites = rng.integers(-3, cap + 1, size=n).astype(np.int32)
    fin = np.zeros(n, FINAL_DTYPE)
    fin["start"] = rng.integers(0, 250_000_000, size=n)
    fin["match_len"] = rng.integers(0, 6, size=n)
    fin["match_off"] = np.concatenate([[0], np.cumsum(fin["match_len"])[:-1]])
    blob = rng.integers(65, 90, size=int(fin["match_len"].sum()) + 1).astype(np.uint8)
    return {"sites": sites, "nsites": nsites, "final": fin, "final_match": blob}


def test_dump_is_a_fixed_float_sample_within_the_cap(tmp_path):
    rng = np.random.default_rng(3)
    n, cap = 200_000, 32
    out = _fake_output(n, cap, rng)
    d = B.mapper_outputs(out, cap)
    assert sum(a.nbytes for a in d.values()) <= B.DUMP_BYTES_MAX
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    k = B.dump_site_reads(cap)
    assert d["site_start"].shape == (k, cap) and d["nsites"].shape == (B.DUMP_READS,)
    cnt = np.maximum(out["nsites"][:k], 0)
    for r in range(0, k, 97):
        assert np.array_equal(d["site_start"][r, :cnt[r]], out["sites"]["start"][r, :cnt[r]])
        assert not d["site_start"][r, cnt[r]:].any()
    again = B.mapper_outputs(out, cap)
    assert all(np.array_equal(d[name], again[name]) for name in d)
    # the sample's records and match strings
    pick = np.sort(np.random.Generator(np.random.PCG64(B.DUMP_SEED)).choice(n, size=B.DUMP_READS, replace=False))
    assert np.array_equal(d["final_start"], out["final"]["start"][pick])
    assert np.array_equal(d["nsites"], out["nsites"][pick])
    B.write_outputs(str(tmp_path / "d"), d)
    assert np.array_equal(np.load(tmp_path / "d" / "final_match_crc32.npy"), d["final_match_crc32"])
    with pytest.raises(SystemExit):
        B.write_outputs(str(tmp_path / "big"), {"x": np.zeros(B.DUMP_BYTES_MAX // 8 + 1)})
