"""Times the two device stages of the merge (bbmerge_overlap_batch_device, bbmerge_join_batch_device) over a resident batch of
2 x 150 pairs beside the host form's single thread on pairs of the same batch.

    python scripts/measure_merge.py                       # 1 M pairs: HIP-event times of each call, the median of the repeats
    BBMAP_AMD_SO=bbmap_amd/_variants/lib_walkall.so python scripts/measure_merge.py --no-host      # a variant build

Pairs: fragments of a random 4 Mbase sequence, lengths normal(250, 50) clipped to 150..400 (beyond 292 the mates do not overlap), both
mates read to 150 with 0.5 % substitutions, qualities uniform in 20..41.  Seeded, needs nothing outside the tree, fails without a GPU.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEN = 150


def make_pairs(n, seed):
    """(bases [2n, LEN]: mate 1s, then mate 2s as sequenced; qualities [2n, LEN]; fragment lengths)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = rng.integers(0, 4, 4 << 20, dtype=np.uint8)
    frag = np.clip(rng.normal(250, 50, n), LEN, 400).astype(np.int64)
    start = (rng.random(n) * (len(genome) - 400)).astype(np.int64)
    col = np.arange(LEN)
    codes = np.concatenate([genome[start[:, None] + col], 3 - genome[(start + frag - 1)[:, None] - col]])      # (3 - code: the complement)
    err = rng.random(codes.shape, dtype=np.float32) < 0.005
    codes[err] = (codes[err] + rng.integers(1, 4, int(err.sum()), dtype=np.uint8)) & 3
    return acgt[codes], rng.integers(20, 42, codes.shape, dtype=np.uint8), frag


def timed(torch, fn, calls, warmup):
    ms = []
    for i in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--host-pairs", type=int, default=100000, help="the host form runs over the first so many pairs of the batch")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_merge.py needs a GPU")
    from bbmap_amd import merge as M
    from bbmap_amd.index import READ_DTYPE
    n = args.pairs
    b, q, frag = make_pairs(n, 41)
    reads = np.zeros(2 * n, READ_DTYPE)
    reads["bases_off"], reads["len"] = np.arange(2 * n, dtype=np.int64) * LEN, LEN
    r1, r2 = reads[:n].copy(), reads[n:].copy()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()       # noqa: E731
    d1, d2, db, dq = up(r1), up(r2), up(b), up(q)
    out = dict(pairs=n, length=LEN, library=os.environ.get("BBMAP_AMD_SO", "default"), overlapping_fragments=float((frag <= 2 * LEN - 8).mean()))
    configs = dict(flat=M.default_config(), quality_then_flat=M.default_config(useQuality=1), quality_only=M.default_config(useQuality=1, withoutQuality=0))
    recs = {}
    for name, cfg in configs.items():
        box = {}
        t = timed(torch, lambda: box.__setitem__("r", M.overlap_batch_device(d1, d2, db, dq, cfg)), args.calls, args.warmup)
        recs[name] = box["r"].cpu().numpy().view(M.REC_DTYPE).copy()
        t["pairs_per_s"] = n / (t["ms_median"] * 1e-3)
        t["merged"] = float(((recs[name]["insert"] > 0) & (recs[name]["ambig"] == 0)).mean())
        t["true_insert"] = float((recs[name]["insert"] == frag)[(recs[name]["insert"] > 0) & (recs[name]["ambig"] == 0)].mean())
        out["overlap_" + name] = t
    merged, total = M.slots_for(r1, r2)
    dm, dins = up(merged), torch.from_numpy(M.usual_inserts(recs["flat"])).cuda()
    ob, oq = torch.zeros(total, dtype=torch.uint8, device="cuda"), torch.zeros(total, dtype=torch.uint8, device="cuda")
    for name, qq, oqq in (("join_quality", dq, oq), ("join_noquality", None, None)):
        t = timed(torch, lambda: M.join_batch_device(d1, d2, db, qq, dins, dm, ob, oqq), args.calls, args.warmup)
        t["pairs_per_s"] = n / (t["ms_median"] * 1e-3)
        t["bases_written"] = int(dm.cpu().numpy().view(READ_DTYPE)["len"].sum())
        out[name] = t
    if not args.no_host:
        h = min(n, args.host_pairs)
        for name in ("flat", "quality_then_flat"):
            t0 = time.perf_counter()
            hrecs = M.overlap_batch(r1[:h], r2[:h], b.reshape(-1), q.reshape(-1), configs[name])
            s = time.perf_counter() - t0
            out["host_overlap_" + name] = dict(pairs=h, s=s, pairs_per_s_one_thread=h / s, same_as_device=bool((hrecs == recs[name][:h]).all()))
        ins = M.usual_inserts(recs["flat"][:h])
        t0 = time.perf_counter()
        hm, hb, hq = M.join_batch(r1[:h], r2[:h], b.reshape(-1), q.reshape(-1), ins)
        s = time.perf_counter() - t0
        dmh = dm.cpu().numpy().view(READ_DTYPE)[:h]
        out["host_join_quality"] = dict(pairs=h, s=s, pairs_per_s_one_thread=h / s, same_lengths_as_device=bool((hm["len"] == dmh["len"]).all()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
