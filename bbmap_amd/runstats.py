"""Run statistics (bbmap_runstats, include/bbmap_amd.h): the record layouts, the raw device call and the derived figures of the table
BBMap prints at the end of a run (printOutput, current/align2/AbstractMapper.java:1363-1470) as numbers; the text layout stays with the
host."""
import ctypes as C

import numpy as np

from . import _lib
from .index import READ_DTYPE

PER_MATE = ("mappedRetained", "mappedRetainedBases", "ambiguousBestAlignment", "ambiguousBestAlignmentBases", "matchCountM", "matchCountS",
            "matchCountD", "matchCountI", "matchCountN", "readCountS", "readCountD", "readCountI", "readCountN", "readCountE", "rescuedP",
            "rescuedM", "perfectMatch", "perfectMatchBases", "perfectHitCount", "semiPerfectHitCount", "semiperfectMatch",
            "semiperfectMatchBases", "siteSum", "topSiteSum", "uniqueHit", "noHit", "firstSiteCorrectP", "firstSiteCorrectM",
            "firstSiteCorrectPaired", "firstSiteCorrectSolo", "firstSiteCorrectRescued", "firstSiteIncorrect", "firstSiteCorrectLoose",
            "firstSiteIncorrectLoose", "truePositiveP", "truePositiveM", "totalCorrectSites", "correctUniqueHit", "correctMultiHit",
            "correctLowHit", "falsePositive", "readsUsed", "basesUsed")
PAIR_LEVEL = ("bothUnmapped", "bothUnmappedBases", "numMated", "numMatedBases", "badPairs", "badPairBases", "innerLengthSum",
              "outerLengthSum", "insertSizeSum")
RUNSTATS_DTYPE = np.dtype([(n + "1", "<i8") for n in PER_MATE] + [(n + "2", "<i8") for n in PER_MATE] +
                          [(n, "<i8") for n in PAIR_LEVEL] + [("reserved", "<i8")])
TRUTH_DTYPE = np.dtype([("chrom", "<i4"), ("strand", "<i4"), ("start", "<i4"), ("stop", "<i4")])
INSERT_HIST_BINS = 40001            # ReadStats.MAXINSERTLEN + 1
RUNSTATS_MAX_WAVES = 8192           # wavefronts of the kernel's persistent grid
ADAPT_INSERT_LENGTH, ADAPT_RESCUE_SKIP = 1, 2


def run_stats_device(reads, finals, pool, sites, nsites, cap, paired=False, scheme=0, thresh=0, truth=None, counters=None, ihist=None):
    """bbpipe_run_stats_device over torch device tensors (uint8 views of READ_DTYPE / FINAL_DTYPE / MSITE_DTYPE records, int32 nsites,
    TRUTH_DTYPE truth or None); counters: int64[96] tensor that is ADDED to (made when None), ihist: int64[INSERT_HIST_BINS] or None.
    Returns (RUNSTATS_DTYPE scalar, the counters tensor)."""
    import torch
    L = _lib.load()
    n = reads.numel() // READ_DTYPE.itemsize
    if counters is None:
        counters = torch.zeros(RUNSTATS_DTYPE.itemsize // 8, dtype=torch.int64, device=reads.device)
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    _lib.check(L.bbpipe_run_stats_device(C.c_void_p(stream), n, int(paired), int(scheme), int(thresh), ptr(reads), ptr(finals), ptr(pool),
                                         ptr(sites), ptr(nsites), int(cap), ptr(truth), ptr(counters), ptr(ihist)), "bbpipe_run_stats_device")
    torch.cuda.current_stream().synchronize()
    return counters.cpu().numpy().view(RUNSTATS_DTYPE)[0], counters


def _div(a, b):
    return float(a) / float(b) if b else float("nan")


def summary(stats):
    """The derived figures of AbstractMapper.java:1363-1470 for mate 1's table and the pairing block, as numbers (NaN where the
    reference divides by zero).  stats: a RUNSTATS_DTYPE scalar or a dict of the same names."""
    g = lambda k: int(stats[k])
    reads1, bases1, bases = g("readsUsed1"), g("basesUsed1"), g("basesUsed1") + g("basesUsed2")
    pct = lambda k: 100.0 * _div(g(k), reads1)                      # x*invTrials100 (:1366)
    out = {
        "matedPercent": pct("numMated"),                            # :1372
        "badPairsPercent": pct("badPairs"),                         # :1374
        "matedPercentBases": 100.0 * _div(g("numMatedBases"), bases),       # :1375
        "badPairsPercentBases": 100.0 * _div(g("badPairBases"), bases),     # :1376
        "innerLengthAvg": _div(g("innerLengthSum"), g("numMated")),         # :1377
        "outerLengthAvg": _div(g("outerLengthSum"), g("numMated")),         # :1378
        "insertSizeAvg": _div(g("insertSizeSum"), g("numMated")),           # :1379
        "mappedPercent": pct("mappedRetained1"),                    # :1404
        "mappedPercentBases": 100.0 * _div(g("mappedRetainedBases1"), bases1),      # :1405
        "ambiguousPercent": pct("ambiguousBestAlignment1"),
        "perfectMatchPercent": pct("perfectMatch1"),                # :1386
        "semiperfectMatchPercent": pct("semiperfectMatch1"),        # :1387
        "rescuedPercent": pct("rescuedP1") + pct("rescuedM1"),      # :1406-1407
        "noHitPercent": pct("noHit1"),                              # :1420
        "truePositiveStrict": 100.0 * _div(g("firstSiteCorrectP1") + g("firstSiteCorrectM1"), reads1),      # :1412
        "truePositiveLoose": pct("firstSiteCorrectLoose1"),         # :1413
        "falsePositive": pct("firstSiteIncorrect1"),                # :1408
    }
    m, s, d, i, n = (g("matchCount%s1" % c) for c in "MSDIN")
    match_len = m + i + s + n + d                                   # :1460
    out.update(matchLen=match_len,
               errorRate=100.0 * _div(s + i + d, match_len),        # :1458, :1462
               matchRate=100.0 * _div(m, match_len),                # :1463
               subRate=100.0 * _div(s, match_len),                  # :1464
               delRate=100.0 * _div(d, match_len),                  # :1465
               insRate=100.0 * _div(i, match_len),                  # :1466
               nRate=100.0 * _div(n, match_len))                    # :1467
    return out
