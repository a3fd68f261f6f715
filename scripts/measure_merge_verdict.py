"""Times bbmerge_verdict_batch_device beside the bare overlap search over the resident batch of scripts/measure_merge.py (1 M pairs of
2 x 150 with qualities): the verdict under the defaults, `strict` and `xstrict` (both modes), with and without the
counters, and bbmerge_overlap_batch_device under its defaults.  HIP events, 3 warm-ups, the median and the min..max of 20 calls.

    python scripts/measure_merge_verdict.py
    python scripts/measure_merge_verdict.py --overlap-library this=bbmap_amd/libbbmap_amd.so --overlap-library parent=/path/to/parent/libbbmap_amd.so

--overlap-library NAME=PATH (repeatable) times only bbmerge_overlap_batch_device of the named builds on the same pairs, bound by
hand so that a build from before the verdict can be loaded; the builds are visited in turn, twice, so that drift shows.
Seeded, needs nothing outside the tree, fails without a GPU.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_merge import LEN, make_pairs, timed      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--overlap-library", action="append", default=[], metavar="NAME=PATH")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_merge_verdict.py needs a GPU")
    from bbmap_amd import merge as M
    from bbmap_amd.index import READ_DTYPE
    n = args.pairs
    b, q, frag = make_pairs(n, 41)
    reads = np.zeros(2 * n, READ_DTYPE)
    reads["bases_off"], reads["len"] = np.arange(2 * n, dtype=np.int64) * LEN, LEN
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()       # noqa: E731
    d1, d2, db, dq = up(reads[:n].copy()), up(reads[n:].copy()), up(b), up(q)
    out = dict(pairs=n, length=LEN, calls=args.calls)
    if args.overlap_library:
        cfg = M.default_config()
        recs = torch.zeros(n * M.REC_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        libs = []
        for spec in args.overlap_library:
            name, path = spec.split("=", 1)
            fn = C.CDLL(os.path.abspath(path)).bbmerge_overlap_batch_device
            fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5
            libs.append((name, fn))
        first = None
        for visit in (1, 2):
            for name, fn in libs:
                def call():
                    rc = fn(C.byref(cfg), C.c_void_p(stream), n, d1.data_ptr(), d2.data_ptr(), db.data_ptr(), dq.data_ptr(), recs.data_ptr())
                    assert rc == 0, rc
                t = timed(torch, call, args.calls, args.warmup)
                got = recs.cpu().numpy().view(M.REC_DTYPE).copy()
                first = got if first is None else first
                t["same_records_as_first"] = bool((got == first).all())
                out["overlap_%s_visit%d" % (name, visit)] = t
        print(json.dumps(out))
        return
    box = {}
    t = timed(torch, lambda: box.__setitem__("r", M.overlap_batch_device(d1, d2, db, dq, M.default_config())), args.calls, args.warmup)
    r = box["r"].cpu().numpy().view(M.REC_DTYPE)
    t["merged"] = float(((r["insert"] > 0) & (r["ambig"] == 0)).mean())
    out["overlap_flat"] = t
    for name, cfg in (("defaults", M.default_verdict_config()), ("strict", M.verdict_from_flags("strict")), ("xstrict", M.verdict_from_flags("xstrict"))):
        for with_stats in (False, True):
            stats = M.new_stats_device("cuda") if with_stats else None
            t = timed(torch, lambda: box.__setitem__("r", M.verdict_batch_device(d1, d2, db, dq, cfg, stats)), args.calls, args.warmup)
            v = box["r"].cpu().numpy().view(M.VERDICT_DTYPE)
            t["pairs_per_s"] = n / (t["ms_median"] * 1e-3)
            t["merged"] = float((v["code"] > 0).mean())
            t["true_insert"] = float((v["code"] == frag)[v["code"] > 0].mean())
            t["ambiguous"] = float((v["code"] == M.RET_AMBIG).mean())
            t["normal_mode_ran"] = float(((v["info"] & M.INFO_NORMAL) != 0).mean())
            t["over_overlap_flat"] = t["ms_median"] / out["overlap_flat"]["ms_median"]
            if with_stats:
                s = stats.cpu().numpy().view(M.STATS_DTYPE)
                t["stats_pairs"] = int(s["pairs"][0])
                assert s["pairs"][0] == n * (args.calls + args.warmup) and s["merged"][0] == int((v["code"] > 0).sum()) * (args.calls + args.warmup)
            out["verdict_%s%s" % (name, "_stats" if with_stats else "")] = t
    print(json.dumps(out))


if __name__ == "__main__":
    main()
