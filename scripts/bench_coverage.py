"""Times the coverage calls on bench.py's default workload: the hg38-shaped reference with one scaffold per chromosome,
2,000,000 reads (1 M pairs of 150 bp) per batch.

    python scripts/bench_coverage.py                     # one JSON line
    python scripts/bench_coverage.py --workload chr21    # a smaller reference, same code path

In one session, HIP events, five repetitions after two warm-ups each (medians and the spread min .. max):
  bbmap_add_coverage per batch in the default and the exclude-deletions mode,
  bbmap_cov_finalize over the whole table with binsize 1000,
  and as yardsticks bbmap_add_run_stats on the same batch and the step itself.
A batch is counted once, so every timed add follows a step of its own.  Seeded, needs nothing outside the tree, fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench as B                                           # noqa: E402


class ChromosomeTable:
    """One scaffold per chromosome: the chromosome's bases between its two pads."""

    def __init__(self, lens, pad):
        self.locs, self.lengths = [[pad] for _ in lens], [[int(n)] for n in lens]
        self.names = [["chr%d" % (i + 1)] for i in range(len(lens))]
        self.inter_scaffold_padding = 300


def spread(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(B.WORKLOADS), default="hg38")
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--binsize", type=int, default=1000)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_coverage.py needs a GPU")
    from bbmap_amd import _lib
    from bbmap_amd import coverage as V
    from bbmap_amd import keys as K
    from bbmap_amd import workload as W
    from bbmap_amd.index import DeviceIndex
    from bbmap_amd.mapper import Mapper, _copy
    lens, paired, _ = B.WORKLOADS[args.workload]
    L, k = 150, 13
    n = args.reads - (args.reads % 2 if paired else 0)
    chroms, shm_path = B.shared_reference(args.workload, lens, 0.0 if args.workload == "ecoli" else 0.1, 0, 1)
    reads = B.make_batch(chroms, n, paired, 4, lead=B.LEAD_N.get(args.workload))
    kcfg = K.default_config(K.PROFILE_BBMAP, k=k)
    offsets, key_scores, _ = K.make_keys(np.frombuffer(b"ACGT" * ((L + 3) // 4), np.uint8)[:L], None, kcfg)
    di = DeviceIndex.build(chroms, k=k)
    di.set_scaffolds(ChromosomeTable(lens, W.START_PAD))
    stream = torch.cuda.current_stream().cuda_stream
    out = dict(workload=args.workload, reads=n, ref_bases=int(sum(lens)), scaffolds=len(lens), binsize=args.binsize, reps=args.reps)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for mode, flags in (("default", 0), ("exclude_deletions", V.COV_EXCLUDE_DELETIONS)):
        mp = Mapper(di, n, L, offsets, key_scores, paired=paired, max_sites=32)
        mp.load_reads(reads)
        mp.enable_coverage(flags)
        step, add, stats, fin = [], [], [], []
        view = V.bbmap_cov_view()
        for i in range(args.warmup + args.reps):
            t_step = timed(mp.step)
            t_add = timed(lambda: _lib.check(mp.L.bbmap_add_coverage(mp.h, C.c_void_p(stream)), "bbmap_add_coverage"))
            t_stats = timed(lambda: _lib.check(mp.L.bbmap_add_run_stats(mp.h, C.c_void_p(stream), None), "bbmap_add_run_stats"))
            t_fin = timed(lambda: _lib.check(mp.L.bbmap_cov_finalize(mp.h, C.c_void_p(stream), args.binsize, C.byref(view)), "bbmap_cov_finalize"))
            if i >= args.warmup:
                step.append(t_step); add.append(t_add); stats.append(t_stats); fin.append(t_fin)
        slots = int(view.slots)
        # finalize per strand: the difference array is read twice (tile sums, apply) and the depths are written once and read by the
        # statistics pass and by each of the median's rounds that a long scaffold takes (two for 16-bit depths)
        moved = slots * (2 * 4 + view.depth_bytes * (1 + 1 + 2))
        out[mode] = dict(ms_step=spread(step), ms_add_coverage=spread(add), ms_add_run_stats=spread(stats), ms_finalize=spread(fin),
                         finalize_bytes_moved=moved, finalize_GBps=moved / (np.median(fin) * 1e-3) / 1e9,
                         state_bytes=slots * (4 + view.depth_bytes))
        # (records and totals only: the depths stay on the device)
        recs = _copy(view.recs, view.nscaf * V.COVREC_DTYPE.itemsize).view(V.COVREC_DTYPE)
        totals = _copy(view.totals, V.COVTOTALS_DTYPE.itemsize).view(V.COVTOTALS_DTYPE)[0]
        out[mode]["mappedReads"] = int(totals["mappedReads"])
        out[mode]["max_depth"] = int(recs["strand"]["max"][:, 0].max())
        if not flags:                                       # nothing saturates here, so the depths sum to basehits
            out[mode]["sum_depth_equals_basehits"] = bool(int(recs["strand"]["sumDepth"][:, 0].sum()) == int(recs["basehits"].sum()))
        mp.close()
    print(json.dumps(out))
    di.close()
    if shm_path and os.path.exists(shm_path):
        os.remove(shm_path)


if __name__ == "__main__":
    main()
