"""What the key-stage test inputs (tests/keys_problems.py) are, measured through the host form: the GPU comparison in
tests/test_keys_gpu.py cannot pass on trivial input when a fair share of the reads lose keys, move their first key or get none."""
import pytest

from tests import keys_problems as P


@pytest.mark.parametrize("name", ["reads150", "mixed", "pacbio"])
def test_generated_reads_exercise_the_key_stage(name):
    recs, _, bs, ki, used = P.host_answer(name)
    plain, _, _, _, _ = P.host_answer(name, use_qualities=False)
    n = len(recs)
    assert used == int(2 * recs["nkeys"].astype("int64").sum()) and used > 0
    assert (recs["nkeys"] == 0).sum() >= 0.05 * n                      # reads quickMap refuses
    assert (P.first_offsets(recs, ki) > 0).sum() >= 0.05 * n           # a bad head moves the first key
    fewer = (recs["nkeys"] > 0) & (recs["nkeys"] < plain["nkeys"])
    assert fewer.sum() >= 0.05 * n                                     # misses and narrowed windows
    assert P.key_scores(recs, ki).min() < 400                          # keys over probably-wrong bases
    assert bs.min() < -50 and bs.max() == 0


def test_generator_is_seeded():
    a, qa = P.make_reads([150, 13, 0, 600], 3)
    b, qb = P.make_reads([150, 13, 0, 600], 3)
    assert all((x == y).all() for x, y in zip(a + qa, b + qb))
    assert [len(x) for x in a] == [150, 13, 0, 600]
