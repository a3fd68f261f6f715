"""Times bbmap_add_run_stats on the batch of scripts/measure_sam_records.py: 1 M pairs of 150 bp, 3,000 scaffolds.

    python scripts/measure_run_stats.py                   # HIP-event times, bytes read, the host alternative
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/measure_run_stats.py --calls 3 --no-host

Seeded, needs nothing outside the tree, fails without a GPU.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.measure_sam_records import KL, L, make_genome, make_pairs       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--genome-mbp", type=float, default=98.0)
    ap.add_argument("--scaffolds", type=int, default=3000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_run_stats.py needs a GPU")
    from bbmap_amd import _lib
    from bbmap_amd.index import DeviceIndex
    from bbmap_amd.mapper import FINAL_DTYPE, Mapper
    from oracle import oracle as O
    p = make_genome(args.genome_mbp, args.scaffolds, 5)
    reads = make_pairs(p, args.pairs, 6)
    n = len(reads)
    di = DeviceIndex.build(p.chroms, k=KL)
    di.set_scaffolds(p)
    offs = O.make_offsets(L, KL, 1.9)
    mp = Mapper(di, n, L, offs, [100 * KL] * len(offs), paired=True, max_sites=32)
    mp.load_reads(reads)
    stream = torch.cuda.current_stream().cuda_stream
    ms = []
    for i in range(args.warmup + args.calls):
        mp.step()                                           # a batch is counted once: map it again for every timed call
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(mp.L.bbmap_add_run_stats(mp.h, C.c_void_p(stream), None), "bbmap_add_run_stats")
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    fin = mp.final(with_match=False)[0]
    ns = mp.fetch(with_match=False, rows=0)["nsites"]
    strings = int(fin["match_len"][fin["match_len"] > 0].sum())
    sites = int(ns[ns > 0].sum())
    # per call: every read's final record (mate 1 also reads mate 2's), its read record, its site count, its match string, and 7 ints
    # of each site of its list (whole 64-byte sectors in practice: bounded by the 128-byte records)
    out = dict(reads=n, ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), match_string_bytes=strings,
               sites=sites, bytes_read_min=int(n * (1.5 * FINAL_DTYPE.itemsize + 24 + 4) + strings + sites * 28),
               bytes_read_max=int(n * (1.5 * FINAL_DTYPE.itemsize + 24 + 4) + strings + sites * 128))
    if not args.no_host:
        t = time.perf_counter()
        fin, blob = mp.final()
        out["host_get_final_s"] = time.perf_counter() - t
        t = time.perf_counter()
        counts = np.bincount(blob, minlength=256)
        out["host_numpy_count_s"] = time.perf_counter() - t
        rs, _ = mp.run_stats()
        total = sum(int(rs["matchCount%s%d" % (c, m)]) for c in "MSDIN" for m in (1, 2))
        out["columns_device_per_batch"] = total // (args.warmup + args.calls)
        out["columns_host"] = int(sum(counts[ord(c)] for c in "mSDIXYNC"))
        # the two agree when the overflow tier mapped no read; a tier read's string reaches the device count only
        out["tier_reads"] = int(mp.stats()["reads_reprobed"])
    print(json.dumps(out))
    mp.close()
    di.close()


if __name__ == "__main__":
    main()
