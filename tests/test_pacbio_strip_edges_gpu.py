"""The strip-tiled 9PacBio kernel (bbmap_amd/csrc/msa_fill_strip.hip) at its tiling borders and penalty tiers: device = oracle, field
by field, on the planted job sets of tests/pacbio_strip_problems.py (what each set holds is pinned on the CPU by
tests/test_pacbio_strip_problems_cpu.py), in both forms of the kernel.

  rows / death / cols / walk   one launch per set in a 1030 x 1203 context: three strips of 512 rows, boundary rows of 1203 columns
  mixed                        330 jobs in one launch, more than the pipelined form has slots: waves that claim a job and arrive without
                               filling (fewer strips than waves, bad shapes) beside full-height jobs; one match string that overflows
  one wave                     BBMSA_STRIP_DIR_MB=1: a single resident wave (a single slot) runs 42 jobs of alternating shape one after
                               the other, so every job inherits the previous job's records, boundary rows and hand-shake words
  banded                       contexts with a band: every limited fill leaves the strip kernel for the one-thread kernel

The oracle's answers are computed once per process (pacbio_strip_problems.answers) and shared by both forms."""
import time

import pytest

from bbmap_amd import msa as M
from tests import pacbio_strip_problems as P
from tests.msa_check import check_job

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["sequential", "pipelined"])
def strip_form(request, monkeypatch):
    """Both forms of the strip kernel (as in tests/test_pacbio_gpu.py): one wavefront per job, or the strips of a job pipelined over
    several wavefronts.  BBMSA_STRIP_PIPE_JOBS is the job-count threshold of the pipelined form, read when the context is created."""
    monkeypatch.setenv("BBMSA_STRIP_PIPE_JOBS", "0" if request.param == "sequential" else "512")
    return request.param


def where(name, k, kinds, probs, flags, maxColumns):
    return "%s: job %d (%s) rows %d columns %d flags %#x minScore %d" % (
        name, k, kinds[k], len(probs[k][0]), P.columns_of(probs[k], flags[k], maxColumns), flags[k], probs[k][4])


def run_set(name, form):
    """One launch of the whole set through MultiStateAligner9PacBio.align; every record against the oracle's."""
    probs, flags, kinds, exp = P.answers(name)
    gen, maxRows, maxColumns, band = P.SETS[name]
    t0 = time.time()
    al = M.MultiStateAligner9PacBio(maxRows, maxColumns, bandwidth=band[0], bandwidthRatio=band[1])
    got = al.align(probs, flags)
    counts = al.ctx.last_counts()
    al.ctx.close()
    print("%s (%s): %d jobs, %.2f s on the device side, %d jobs to the one-thread kernel" % (name, form, len(probs), time.time() - t0, counts["generic"]))
    assert len(got) == len(probs)
    for k, g in enumerate(got):
        w = where(name, k, kinds, probs, flags, maxColumns)
        check_job(g, exp[k], w)
        assert g["columns"] == P.columns_of(probs[k], flags[k], maxColumns), w
    return counts


@pytest.mark.parametrize("name", ["rows", "death", "cols", "walk"])
def test_planted_set_matches_the_oracle(name, strip_form):
    counts = run_set(name, strip_form)
    assert counts["generic"] == 0                       # no band, no hand-shake timeout: the strip kernel answered every job itself


def test_mixed_launch(strip_form):
    """330 jobs, one launch through MSAContext.align_batch, one match_stride that one string does not fit.  The bad shapes come back
    all-zero with their columns, the overflowing job with match_len -1 and everything else right, and every other record is the
    oracle's.  (bbmsa_align_batch presets the records to 0xff, so a record nobody wrote fails every comparison; its staging buffer for
    the strings starts out undefined, so bytes past a string's end cannot be judged here.)"""
    probs, flags, kinds, exp = P.answers("mixed")
    jobs, reads, refs = M.pack_problems(probs, flags)
    ctx = M.MSAContext(P.MAX_ROWS, P.MAX_COLS, scheme=M.SCHEME_9PACBIO)
    t0 = time.time()
    res, match = ctx.align_batch(jobs, reads, refs, P.MIXED_STRIDE)
    counts = ctx.last_counts()
    ctx.close()
    print("mixed (%s): %d jobs, %.2f s on the device side" % (strip_form, len(probs), time.time() - t0))
    assert counts["generic"] == 0
    seen = set()
    for k, r in enumerate(res):
        w = where("mixed", k, kinds, probs, flags, P.MAX_COLS)
        ml = int(r["match_len"])
        if kinds[k].startswith("bad_"):
            assert r["status"] == M.ST_BAD_SHAPE and not r["result"].any() and not r["score"].any(), w
            assert r["iterations"] == 0 and r["score_len"] == 0 and ml == 0 and r["fill_kind"] == 0, w
            cols = {"bad_rows": P.columns_of(probs[k], flags[k]), "bad_columns": P.MAX_COLS + 1, "bad_columns_zero": 0}[kinds[k]]
            assert r["columns"] == cols, w
            seen.add(kinds[k])
            continue
        assert r["columns"] == P.columns_of(probs[k], flags[k]), w
        g = {"result": r["result"].tolist(), "status": int(r["status"]), "iterations": int(r["iterations"]),
             "score": None if r["score_len"] == 0 else r["score"][:r["score_len"]].tolist(),
             "match": match[k, :ml].tobytes() if ml > 0 else None, "fill_kind": int(r["fill_kind"])}
        if kinds[k].startswith("overflow"):
            assert ml == -1 and len(exp[k]["match"]) > P.MIXED_STRIDE, w
            check_job(g, dict(exp[k], match=None), w)                                # every other field as if the string had fitted
            seen.add("overflow")
            continue
        assert ml == (len(exp[k]["match"]) if exp[k]["match"] is not None else 0), w
        check_job(g, exp[k], w)
    assert seen == {"bad_rows", "bad_columns", "bad_columns_zero", "overflow"}


def test_one_resident_wave_runs_many_jobs(monkeypatch, strip_form):
    """BBMSA_STRIP_DIR_MB caps the memory of the traceback records and with it the grid (msa_host.hip, setup of the strip kernel).  At
    1030 x 1203 a strip's records take ((1203 + 64) >> 3) + 1 = 159 dwords x 8 rows per lane x 64 lanes = 81,408 dwords, a wave's three
    strips 976,896 bytes: one fits 1 MiB, two do not, so the two loops there shrink the grid to ONE block -- in the sequential form one
    wavefront takes all 42 jobs off the queue, in the pipelined form pipeSlots = min(.., blocks) = 1 slot of three wavefronts runs them
    in 42 rounds.  Tall-wide, tiny and mid jobs alternate, as do fills that finish, fills that die early and unlimited fills."""
    monkeypatch.setenv("BBMSA_STRIP_DIR_MB", "1")
    counts = run_set("one_wave", strip_form)
    assert counts["generic"] == 0


@pytest.mark.parametrize("name", ["banded_ratio", "banded_width"])
def test_banded_context_hands_limited_fills_to_the_one_thread_kernel(name, strip_form):
    """bandwidthRatio 0.18 / bandwidth 40: halfband > 0 for every job, so every limited fill goes through slow_list to
    msa_fill_generic_kernel<Scheme9PacBio> and every unlimited one stays in the strip kernel."""
    probs, flags, kinds, exp = P.answers(name)
    counts = run_set(name, strip_form)
    assert counts["generic"] == sum(e["fill_kind"] == 0 for e in exp) > 0
