"""Oracle answer of one bbmsa job and the field-by-field check of a kernel's record against it (shared by the GPU parity
tests of the DP: tests/test_msa_gpu.py, tests/test_msa_routes_gpu.py)."""
from bbmap_amd import msa as M


def oracle_align(om, read, ref, a, b, ms, flags):
    """What the reference would produce for one job with these flags (oracle restatement)."""
    mode = flags & 7
    out = {"score": None, "match": None, "status": 0}
    if flags & M.CLAMP_WINDOW:
        a = max(0, a)
        b = min(len(ref) - 1, b)
    it_l0, it_u0 = om.iterationsLimited, om.iterationsUnlimited
    if mode == M.FILL_LIMITED_RAW:
        res, _ = om.fill_limited_raw(read, ref, a, b, ms)
        om.s.rows, om.s.columns = len(read), b - a + 1
        null = res[4] == 1
    elif mode == M.FILL_UNLIMITED_RAW:
        res, _ = om.fill_unlimited_raw(read, ref, a, b)
        res = res + [0]
        om.s.rows, om.s.columns = len(read), b - a + 1
        null = False
    else:
        r4 = om.fillLimited(read, ref, a, b, ms)
        null = r4 is None
        res = None if null else r4 + [0]
        if null:
            out["status"] = 1
    out["iterations"] = (om.iterationsLimited - it_l0) + (om.iterationsUnlimited - it_u0)
    out["fill_kind"] = 1 if om.iterationsUnlimited != it_u0 else 0
    out["result"] = res
    if not null:
        if flags & M.DO_SCORE:
            out["score"] = om.score(read, ref, a, b, res[0], res[1], res[2])
        if flags & M.DO_TRACEBACK:
            out["match"] = om.traceback(read, ref, a, b, res[0], res[1], res[2])
    return out


def check_job(g, exp, ctx):
    """g: one record as MultiStateAligner11ts.align returns it; exp: oracle_align's answer for the same job."""
    if exp["result"] is not None:
        assert g["result"] == exp["result"], ctx
    else:
        assert g["status"] == M.ST_NULL, ctx
    assert g["status"] == exp["status"], ctx
    assert g["iterations"] == exp["iterations"], ctx
    assert g["fill_kind"] == exp["fill_kind"], ctx
    assert g["score"] == exp["score"], ctx
    assert g["match"] == exp["match"], ctx
