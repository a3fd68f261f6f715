"""Recorded `iterations` deviations of the wavefront kernel's general build in the job sets of tests/test_msa_sorted_band_gpu.py and
tests/test_msa_wide_unlimited_gpu.py (tests/golden/msa_sorted_wide_limited_iterations.json, in the manner of
tests/golden/msa_64x5_limited_iterations.json): limited fills whose visited-cell count on the kernel is not the oracle's.  Every other
field of these records is the oracle's, every route gives the same number, and so does the library before the sorted-with-band route
and the both-loops build existed (the comparison that found them ran both).  The oracle's numbers here are those of a FRESH OracleMSA
per job: the reference's fill reads what the fill before it left in the matrix, which is no part of a batched job."""
import json
import os

from oracle.oracle import OracleMSA
from tests.msa_check import oracle_align

KNOWN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msa_sorted_wide_limited_iterations.json")


def fresh_oracle(maxR, maxC, probs, flags):
    """oracle_align of every job, each on an aligner of its own."""
    return [oracle_align(OracleMSA(maxR, maxC), p[0], p[1], p[2], p[3], p[4], f) for p, f in zip(probs, flags)]


def with_known(set_name, exp, picks=None):
    """The oracle's records with the recorded kernel count in the listed jobs of `set_name` (picks: the set's job index of each record)."""
    with open(KNOWN_FILE) as f:
        known = {int(r["job"]): r for r in json.load(f)["jobs"] if r["set"] == set_name}
    assert len(known) <= 2                                             # a list, not a waiver
    picks = list(range(len(exp))) if picks is None else list(picks)
    out = list(exp)
    for i, j in enumerate(picks):
        if j in known:
            r = known[j]
            assert exp[i]["fill_kind"] == 0 and exp[i]["iterations"] == r["oracle"] and 0 < abs(r["kernel"] - r["oracle"]) <= 9, (set_name, j, r)
            out[i] = dict(exp[i], iterations=r["kernel"])
    return out
