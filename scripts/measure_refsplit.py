"""Times bbmap_add_split on a bench-shaped batch: 1 M pairs of 150 bp on a multi-scaffold genome split into 8 reference
sets, final stage on, all four flags; then the raw form on planted records of the two shapes that stress the counting (every read on
one key; every read on a key of its own).

    python scripts/measure_refsplit.py                  # HIP-event times, bytes moved, download sizes
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/measure_refsplit.py --calls 3 --no-shapes

Seeded, needs nothing outside the tree, fails without a GPU.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from measure_sam_records import KL, L, make_genome, make_pairs      # noqa: E402


def timed(torch, calls, warmup, before, call):
    ms = []
    for i in range(warmup + calls):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)))


def shape(torch, S, n, nkeys, calls, warmup):
    """the raw form over n single reads with one site each, read r on key r % nkeys (nkeys scaffolds of 100 bases, 8 sets)"""
    from bbmap_amd.index import READ_DTYPE
    from bbmap_amd.mapper import FINAL_DTYPE, MSITE_DTYPE
    loc = (8000 + 400 * np.arange(nkeys)).astype(np.int32)
    g = np.arange(n) % nkeys
    fin, rd, sites = np.zeros(n, FINAL_DTYPE), np.zeros(n, READ_DTYPE), np.zeros((n, 1), MSITE_DTYPE)
    fin["mapped"], fin["mapScore"], rd["len"], sites["score"] = 1, 500, 150, 1000
    for rec in (fin, sites[:, 0]):
        rec["chrom"], rec["start"], rec["stop"] = 1, loc[g] + 10, loc[g] + 159
    up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()        # noqa: E731
    cfg = S.config(S.SPLIT_ALL, S.AMBIG2_SPLIT, 200, 5, 8, nkeys)
    d = S.DeviceSplit(cfg, 1, np.array([0, 0, nkeys], np.int32), loc, 300, (np.uint64(1) << (np.arange(nkeys) % 8).astype(np.uint64)),
                      np.arange(nkeys, dtype=np.int32))
    args = (up(rd), up(fin), up(sites), torch.ones(n, dtype=torch.int32, device="cuda"))
    out = timed(torch, calls, warmup, lambda: None, lambda: d.add(*args, 1, False))
    st = d.stats()
    assert int(st.keys[:, 0].sum()) == n * (calls + warmup) and int(st.sets[:, 0].sum()) == n * (calls + warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--genome-mbp", type=float, default=98.0)
    ap.add_argument("--scaffolds", type=int, default=3000)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-shapes", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_refsplit.py needs a GPU")
    from bbmap_amd import _lib
    from bbmap_amd import refsplit as S
    from bbmap_amd.index import DeviceIndex
    from bbmap_amd.mapper import FINAL_DTYPE, MSITE_DTYPE, Mapper
    from oracle import oracle as O
    p = make_genome(args.genome_mbp, args.scaffolds, 5)
    g = 0
    for names in p.names:                                   # BBSplit's prefixes: scaffold i belongs to reference set i % sets
        for i in range(len(names)):
            names[i] = "ref%d$%s" % (g % args.sets, names[i])
            g += 1
    reads = make_pairs(p, args.pairs, 6)
    n = len(reads)
    di = DeviceIndex.build(p.chroms, k=KL)
    di.set_scaffolds(p)
    offs = O.make_offsets(L, KL, 1.9)
    mp = Mapper(di, n, L, offs, [100 * KL] * len(offs), paired=True, max_sites=32)
    mp.load_reads(reads)
    mp.step()
    tab = S.tables(p)
    mp.enable_split(tab, ambiguous2=S.AMBIG2_SPLIT)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = dict(reads=n, scaffolds=len(p.scaffold_names()), sets=tab.nsets, keys=tab.nkeys)
    out["add_split"] = timed(torch, args.calls, args.warmup, mp.reset_split,
                             lambda: _lib.check(mp.L.bbmap_add_split(mp.h, stream), "bbmap_add_split"))
    a, b, tot = C.c_void_p(), C.c_void_p(), C.c_int64()
    out["lists"] = timed(torch, args.calls, args.warmup, lambda: None,
                         lambda: _lib.check(mp.L.bbmap_get_split_lists_device(mp.h, stream, C.byref(a), C.byref(b), C.byref(tot)),
                                            "bbmap_get_split_lists_device"))
    recs, st = mp.split_records(), mp.split_stats()
    fin = mp.final(with_match=False)[0]
    ns = np.clip(fin["nsites"], 0, 5)
    # bytes per add: the read record, the final record and the count of every read, 16 bytes of every site looked at (a 64-byte
    # line each, in effect), the record written; per lists call the two masks read twice and the units written
    out["bytes"] = dict(add_read=int(n * (24 + FINAL_DTYPE.itemsize + 4) + 64 * int(ns.sum())), add_written=int(n * 32),
                        lists_read=int(2 * (n // 2) * 16), lists_written=int(4 * tot.value))
    out["units_listed"] = int(tot.value)
    out["cross_set_ambiguous_reads"] = int(np.count_nonzero(recs["flags"] & S.REC_AMBIG_SETS))
    out["mapped"] = int(np.count_nonzero(recs["flags"] & S.REC_MAPPED))
    out["download_bytes"] = dict(masks=int(n * 16), records=int(n * 32), stats=int(8 * (S.STATE_HEAD + 4 * (tab.nkeys + tab.nsets))),
                                 lists=int(4 * tot.value + 8 * (2 * tab.nsets + 1)),
                                 site_lists_all_slots=int(n * 32 * MSITE_DTYPE.itemsize), site_lists_packed=int(int(np.clip(fin["nsites"], 0, None).sum()) * MSITE_DTYPE.itemsize))
    out["refstats_head"] = S.refstats_lines(st, tab.set_names)[:3]
    mp.close()
    di.close()
    if not args.no_shapes:
        out["shape_one_key"] = shape(torch, S, n, 1, args.calls, args.warmup)
        out["shape_3000_keys"] = shape(torch, S, n, 3000, args.calls, args.warmup)
        out["shape_key_per_read"] = shape(torch, S, n, n // 2, args.calls, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
