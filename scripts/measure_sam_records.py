"""Times bbmap_get_sam_records on a bench-shaped batch: 1 M pairs of 150 bp on a multi-scaffold genome, final stage on.

    python scripts/measure_sam_records.py                 # HIP-event times, bytes moved, text size, host forms
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/measure_sam_records.py --calls 3 --no-host

Seeded, needs nothing outside the tree, fails without a GPU.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, KL = 150, 13
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    COMP[_a] = _b


def make_genome(mbp, scaffolds, seed):
    from bbmap_amd import reference as R
    rng = np.random.default_rng(seed)
    lens = np.exp(rng.uniform(np.log(2000), np.log(200000), scaffolds))
    lens = np.maximum(1000, (lens * (mbp * 1e6 / lens.sum())).astype(np.int64))
    recs = [("scaf%d" % i, ACGT[rng.integers(0, 4, int(n))]) for i, n in enumerate(lens)]
    body = int(lens.sum()) + 300 * scaffolds
    return R.pack(recs, max_length=body // 3 + 400000)


def make_pairs(p, pairs, seed):
    """mate 1 from the plus strand, mate 2 the reverse complement 250 bases on; 37 % of the reads carry 3 substitutions (the rest are
    perfect, as on the bench workload) and 2 % a 3-base deletion"""
    rng = np.random.default_rng(seed)
    sb = [(c, a, n) for c, a, n in p.scaffold_bases() if n >= 1000]
    w = np.array([n for _, _, n in sb], np.float64)
    pick = rng.choice(len(sb), pairs, p=w / w.sum())
    chrom_of = np.array([s[0] for s in sb])[pick]
    start_of = np.array([s[1] for s in sb])[pick]
    len_of = np.array([s[2] for s in sb])[pick]
    reads = np.empty((2 * pairs, L), np.uint8)
    col = np.arange(L)
    for c in range(1, p.nchroms + 1):
        sel = np.nonzero(chrom_of == c)[0]
        if not len(sel):
            continue
        o = start_of[sel] + (rng.random(len(sel)) * (len_of[sel] - 420)).astype(np.int64)
        ch = p.chroms[c - 1]
        reads[2 * sel] = ch[o[:, None] + col]
        reads[2 * sel + 1] = COMP[ch[o[:, None] + 250 + col[::-1]]]
    mut = np.nonzero(rng.random(2 * pairs) < 0.37)[0]
    for _ in range(3):
        pos = rng.integers(0, L, len(mut))
        reads[mut, pos] = ACGT[(np.searchsorted(ACGT, reads[mut, pos]) + rng.integers(1, 4, len(mut))) % 4]
    for r in np.nonzero(rng.random(2 * pairs) < 0.02)[0]:
        reads[r, 70:L - 3] = reads[r, 73:L]
    return reads


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
        raise SystemExit("measure_sam_records.py needs a GPU")
    from bbmap_amd import _lib
    from bbmap_amd.index import DeviceIndex
    from bbmap_amd.mapper import FINAL_DTYPE, SAMREC_DTYPE, SAM_MD, Mapper
    from oracle import oracle as O
    p = make_genome(args.genome_mbp, args.scaffolds, 5)
    reads = make_pairs(p, args.pairs, 6)
    n = len(reads)
    di = DeviceIndex.build(p.chroms, k=KL)
    di.set_scaffolds(p)
    offs = O.make_offsets(L, KL, 1.9)
    mp = Mapper(di, n, L, offs, [100 * KL] * len(offs), paired=True, max_sites=32)
    mp.load_reads(reads)
    mp.step()
    o = mp.output_pointers()
    stream = torch.cuda.current_stream().cuda_stream
    a, b, nb = C.c_void_p(), C.c_void_p(), C.c_int64(0)
    out = dict(reads=n, scaffolds=len(p.scaffold_names()), chromosomes=p.nchroms, final_match_bytes=int(o.final_match_bytes))
    fin = mp.final(with_match=False)[0]
    strings = int(fin["match_len"][fin["match_len"] > 0].sum())
    for name, flags in (("md_off", 0), ("md_on", SAM_MD)):
        ms = []
        for i in range(args.warmup + args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(mp.L.bbmap_get_sam_records(mp.h, C.c_void_p(stream), flags, C.byref(a), C.byref(b), C.byref(nb)), "bbmap_get_sam_records")
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        # bytes per call, from the records: both passes read the final record, the coordinate record, the read record and the match
        # string of every read; the sizing pass writes a record and a count, the scan and the emit pass the offsets and the text
        rd = 2 * (n * (FINAL_DTYPE.itemsize + 32 + 24) + strings) + n * (4 + 8 + 16)
        wr = n * (SAMREC_DTYPE.itemsize + 4 + 8 + 16) + nb.value
        out[name] = dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), text_bytes=int(nb.value),
                         match_string_bytes=strings, bytes_read=rd, bytes_written=wr)
    if not args.no_host:
        t = time.perf_counter(); mp.final(); out["host_get_final_s"] = time.perf_counter() - t
        t = time.perf_counter(); mp.sam_records_host(0); out["host_get_sam_s"] = time.perf_counter() - t
        t = time.perf_counter(); mp.sam_records_host(SAM_MD); out["host_get_sam_md_s"] = time.perf_counter() - t
        recs, _ = mp.sam_records(0)
        out["mapped"] = int(((recs["flag"] & 4) == 0).sum()); out["shortcut_share"] = float(np.mean(recs["cigar_len"] == 4))
    print(json.dumps(out))
    mp.close()
    di.close()


if __name__ == "__main__":
    main()
