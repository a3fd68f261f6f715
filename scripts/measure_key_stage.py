"""Times quickMap's key stage on the device (bbkeys_make_batch_device) beside the host form (bbkeys_make_batch) on the same input and
the same machine: 2 M reads of 150 bases with and without qualities, and 8,192 mapPacBio pieces of 6,000 bases.

    python scripts/measure_key_stage.py                   # HIP-event times of the whole call, the host form's wall time, bytes moved
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/measure_key_stage.py --calls 3 --no-host

Seeded (tests/keys_problems.py makes the qualities), needs nothing outside the tree, fails without a GPU.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_input(n, length, seed):
    """n reads of one length in the kinds of tests/keys_problems.py, vectorised: (bases [n, length], qualities [n, length])"""
    rng = np.random.default_rng(seed)
    b = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, length), dtype=np.uint8)]
    q = rng.integers(25, 41, (n, length), dtype=np.uint8)
    kind = rng.integers(0, 8, n)
    col = np.arange(length)
    w = rng.integers(1, 30, n)
    s = (rng.random(n) * (length - w + 1)).astype(np.int64)
    m = (kind == 1)[:, None] & (col >= s[:, None]) & (col < (s + w)[:, None])
    q[m] = 2
    w = rng.integers(1, 41, n)
    low = rng.integers(0, 3, (n, length), dtype=np.uint8)
    m = ((kind == 2)[:, None] & (col < w[:, None])) | ((kind == 3)[:, None] & (col >= length - w[:, None]))
    q[m] = low[m]
    m = (kind == 4)[:, None] & (rng.random((n, length), dtype=np.float32) < 0.15)
    b[m], q[m] = ord("N"), 0
    m = kind == 5
    q[m] = rng.integers(0, 12, (int(m.sum()), length), dtype=np.uint8)
    q[kind == 6] = 2
    return b, q


def measure(name, cfg, b, q, calls, warmup, host):
    import torch
    from bbmap_amd import _lib, keys as K
    from bbmap_amd.index import READ_DTYPE
    L = _lib.load()
    n, length = b.shape
    recs = np.zeros(n, READ_DTYPE)
    recs["bases_off"], recs["len"] = np.arange(n, dtype=np.int64) * length, length
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1)).cuda()
    d_b = torch.from_numpy(b.reshape(-1)).cuda()
    d_q = None if q is None else torch.from_numpy(q.reshape(-1)).cuda()
    total = n * length
    cap = K.keyinfo_bound(cfg, n, total)
    d_ki = torch.empty(cap, dtype=torch.int32, device="cuda")
    d_bs = torch.empty(total, dtype=torch.int8, device="cuda")
    need = K.workspace_bytes(cfg, n, total)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    used = C.c_int64(0)
    ms = []
    for i in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(L.bbkeys_make_batch_device(C.byref(cfg), C.c_void_p(stream), n, d_recs.data_ptr(), d_b.data_ptr(),
                                              None if d_q is None else d_q.data_ptr(), d_ki.data_ptr(), cap, d_bs.data_ptr(), ws.data_ptr(),
                                              need, C.byref(used)), "bbkeys_make_batch_device")
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    nprob = max(0, length - cfg.k + 1)
    # bytes the algorithm has to move per call: bases once, qualities for both passes of the chain and its trailing reader, base
    # scores, the read records in and out, the usable bits, the keys into their slots and from there into keyinfo
    rd = total * (1 if q is None else 4) + n * 24 * 3 + (0 if q is None else n * (nprob // 8)) + 4 * used.value
    wr = total + n * 24 + (0 if q is None else n * (nprob // 8)) + 2 * 4 * used.value + n * 7 * 4
    out = dict(reads=n, length=length, qualities=q is not None, keyinfo_ints=int(used.value), workspace_bytes=need,
               reads_without_keys=int((d_recs.cpu().numpy().view(READ_DTYPE)["nkeys"] == 0).sum()),
               ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), bytes_read=int(rd), bytes_written=int(wr))
    out["reads_per_s_device"] = n / (out["ms_median"] * 1e-3)
    if host:
        h_recs, h_ki, h_bs = np.zeros(n, READ_DTYPE), np.zeros(cap, np.int32), np.zeros(total, np.int8)
        lens, offs = np.full(n, length, np.int32), np.ascontiguousarray(recs["bases_off"])
        K.make_batch([], None, cfg)              # binds bbkeys_make_batch
        h_used = C.c_int64(0)
        t = time.perf_counter()
        _lib.check(L.bbkeys_make_batch(C.byref(cfg), n, offs.ctypes.data, lens.ctypes.data, b.ctypes.data,
                                       None if q is None else q.ctypes.data, h_recs.ctypes.data, h_ki.ctypes.data, cap, h_bs.ctypes.data,
                                       C.byref(h_used)), "bbkeys_make_batch")
        out["host_s"] = time.perf_counter() - t
        out["reads_per_s_host_one_thread"] = n / out["host_s"]
        out["same_as_host"] = bool(h_used.value == used.value and np.array_equal(h_ki[:h_used.value], d_ki[:used.value].cpu().numpy())
                                   and np.array_equal(h_bs, d_bs.cpu().numpy())
                                   and np.array_equal(h_recs, d_recs.cpu().numpy().view(READ_DTYPE)))
    return name, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--pieces", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_key_stage.py needs a GPU")
    from bbmap_amd import keys as K
    out = {}
    b, q = make_input(args.reads, 150, 31)
    for name, qq in (("reads150_qual", q), ("reads150_noqual", None)):
        k, v = measure(name, K.default_config(), b, qq, args.calls, args.warmup, not args.no_host)
        out[k] = v
    b, q = make_input(args.pieces, 6000, 32)
    k, v = measure("pacbio6000_qual", K.default_config(K.PROFILE_PACBIO), b, q, args.calls, args.warmup, not args.no_host)
    out[k] = v
    print(json.dumps(out))


if __name__ == "__main__":
    main()
