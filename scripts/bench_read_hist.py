"""Times the read-histogram accumulate on bench.py's batch shape: the hg38-shaped reference, 2,000,000 reads (1 M pairs
of 150 bp) mapped once, synthetic qualities (uniform 2..41 per base, seeded).

    python scripts/bench_read_hist.py                     # one JSON line
    python scripts/bench_read_hist.py --workload chr21    # a smaller reference, same code path

In one process, HIP events, three repetitions after one warm-up (medians and the spread min .. max):
  bbmap_add_read_hist with all groups (the context form; a batch is counted once, so every timed add follows a step of its own),
  bbpipe_read_hist_add_device with all groups, with each group alone, without qualities and with every base at one quality (the
  raw form over the same records; the few reads of the overflow tier keep their main-list record there),
  and as yardsticks bbmap_add_coverage and bbmap_add_run_stats on the same batch, which read the same records and strings.
The line is also written to profiles/readhist_<workload>_bench_read_hist.json.  Seeded, needs nothing outside the tree, fails
without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench as B                                           # noqa: E402
from bench_coverage import ChromosomeTable, spread          # noqa: E402

GROUP_NAMES = ["match", "quality", "base", "accuracy", "indel", "error", "length", "gc", "identity"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(B.WORKLOADS), default="hg38")
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_read_hist.py needs a GPU")
    from bbmap_amd import _lib
    from bbmap_amd import keys as K
    from bbmap_amd import readstats as R
    from bbmap_amd import workload as W
    from bbmap_amd.index import DeviceIndex
    from bbmap_amd.mapper import Mapper, bbmap_output
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
    mp = Mapper(di, n, L, offsets, key_scores, paired=paired, max_sites=32)
    mp.load_reads(reads)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    quality = torch.randint(2, 42, (n * L,), dtype=torch.uint8, device="cuda", generator=gen)
    mp.enable_read_hist(R.RH_ALL)
    mp.enable_coverage(0)
    mp.step()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def series(call, before=None):
        ms = []
        for i in range(args.warmup + args.reps):
            if before:
                before()
            t = timed(call)
            if i >= args.warmup:
                ms.append(t)
        return spread(ms)

    out = dict(workload=args.workload, reads=n, read_len=L, reps=args.reps, ms_step=timed(mp.step))
    qp = C.c_void_p(quality.data_ptr())
    out["ms_add_read_hist_all"] = series(lambda: _lib.check(mp.L.bbmap_add_read_hist(mp.h, C.c_void_p(stream), qp), "bbmap_add_read_hist"),
                                         before=mp.step)
    out["ms_add_coverage"] = series(lambda: _lib.check(mp.L.bbmap_add_coverage(mp.h, C.c_void_p(stream)), "bbmap_add_coverage"),
                                    before=mp.step)
    out["ms_add_run_stats"] = series(lambda: _lib.check(mp.L.bbmap_add_run_stats(mp.h, C.c_void_p(stream), None), "bbmap_add_run_stats"),
                                     before=mp.step)
    h = mp.read_hist()
    out["mapped_with_string"] = int(h.id_hist.sum())
    out["bases_counted"] = int(h.base.sum())
    # ---- the raw form over the same records: all groups, each alone, all without qualities
    o = bbmap_output()
    _lib.check(mp.L.bbmap_get_output(mp.h, C.byref(o)), "bbmap_get_output")
    Lr = _lib.load()

    def raw(flags, q):
        state = R.DeviceState(flags)
        call = lambda: _lib.check(Lr.bbpipe_read_hist_add_device(C.c_void_p(stream), n, int(paired), flags, C.c_void_p(mp.reads.data_ptr()),
                                                                 C.c_void_p(mp.bases.data_ptr()), q, C.c_void_p(o.final), C.c_void_p(o.final_match),
                                                                 C.c_void_p(state.state.data_ptr())), "bbpipe_read_hist_add_device")
        return series(call)

    out["ms_raw_all"] = raw(R.RH_ALL, qp)
    out["ms_raw_all_no_quality"] = raw(R.RH_ALL, None)
    quality.fill_(37)                                       # every base at one quality: the worst case for the quality-indexed counters
    out["ms_raw_all_one_quality"] = raw(R.RH_ALL, qp)
    quality.random_(2, 42, generator=gen)
    out["ms_raw_group"] = {name: raw(g, qp) for name, g in zip(GROUP_NAMES, R.RH_GROUPS)}
    both = out["ms_add_coverage"]["median"] + out["ms_add_run_stats"]["median"]
    out["all_over_coverage_plus_run_stats"] = out["ms_add_read_hist_all"]["median"] / both
    print(json.dumps(out))
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "readhist_%s_bench_read_hist.json" % args.workload)
    with open(path, "w") as f:
        f.write(json.dumps(out) + "\n")
    mp.close()
    di.close()
    if shm_path and os.path.exists(shm_path):
        os.remove(shm_path)


if __name__ == "__main__":
    main()
