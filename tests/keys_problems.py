"""Inputs for the key stage's tests (bbkeys_make_batch on the host, bbkeys_make_batch_device on the GPU): seeded reads whose qualities
exercise every branch of quickMap's key stage -- clean reads, a bad stretch, a bad head or tail (the first key moves off offset 0),
undefined bases, uniformly poor qualities and unreadable reads -- and the host form's answers for them, computed once."""
import functools

import numpy as np

from bbmap_amd import keys as K

ACGT = np.frombuffer(b"ACGT", np.uint8)
MIXED_LENS = (13, 14, 20, 37, 64, 100, 150, 151, 250, 600)
PACBIO_LENS = (100, 1000, 6000, 6016)


def make_read(rng, n):
    """(bases, qualities) of one read of n bases: random ACGT at q 25..40, then one of eight kinds drawn uniformly."""
    b = ACGT[rng.integers(0, 4, n)]
    q = rng.integers(25, 41, n).astype(np.uint8)
    kind = int(rng.integers(0, 8))
    if n == 0:
        return b, q
    if kind == 1:                                    # a stretch of 1..29 bases at q 2, at a random place
        w = min(n, int(rng.integers(1, 30)))
        s = int(rng.integers(0, n - w + 1))
        q[s:s + w] = 2
    elif kind == 2:                                  # a head of 1..40 bases at q 0..2
        w = min(n, int(rng.integers(1, 41)))
        q[:w] = rng.integers(0, 3, w)
    elif kind == 3:                                  # a tail likewise
        w = min(n, int(rng.integers(1, 41)))
        q[n - w:] = rng.integers(0, 3, w)
    elif kind == 4:                                  # 15 % of the positions undefined
        m = rng.random(n) < 0.15
        b = np.where(m, np.uint8(ord("N")), b)
        q[m] = 0
    elif kind == 5:                                  # every quality poor
        q = rng.integers(0, 12, n).astype(np.uint8)
    elif kind == 6:                                  # unreadable
        q[:] = 2
    return b, q                                      # kinds 0 and 7: unchanged


def make_reads(lens, seed):
    """lens: one length per read.  Returns (reads, qualities): two lists of uint8 arrays."""
    rng = np.random.default_rng(seed)
    pairs = [make_read(rng, int(n)) for n in lens]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _draw(lens, n, seed):
    return np.asarray(lens)[np.random.default_rng(seed).integers(0, len(lens), n)]


@functools.lru_cache(maxsize=None)
def problem(name):
    """(reads, qualities, profile) of a named set: "reads150" 20,000 x 150 bases, "mixed" 4,096 reads of MIXED_LENS, "pacbio" 256 reads
    of PACBIO_LENS for the mapPacBio profile."""
    if name == "reads150":
        return make_reads([150] * 20000, 11) + (K.PROFILE_BBMAP,)
    if name == "mixed":
        return make_reads(_draw(MIXED_LENS, 4096, 12), 13) + (K.PROFILE_BBMAP,)
    if name == "pacbio":
        return make_reads(_draw(PACBIO_LENS, 256, 14), 15) + (K.PROFILE_PACBIO,)
    raise KeyError(name)


def host(reads, quals, cfg):
    """The host form's answer: (recs, blob, baseScores, keyinfo[:used], used)."""
    recs, blob, bs, ki = K.make_batch(reads, quals, cfg)
    used = int(recs["keys_off"][-1] + 2 * recs["nkeys"][-1]) if len(recs) else 0
    return recs, blob, bs, ki[:used], used


@functools.lru_cache(maxsize=None)
def host_answer(name, use_qualities=True, semiperfect=0):
    reads, quals, profile = problem(name)
    return host(reads, quals if use_qualities else None, K.default_config(profile, semiperfectMode=semiperfect))


def first_offsets(recs, keyinfo):
    """the first key offset of every read that has keys"""
    has = recs["nkeys"] > 0
    return keyinfo[recs["keys_off"][has]]


def key_scores(recs, keyinfo):
    has = recs["nkeys"] > 0
    return np.concatenate([keyinfo[o + n:o + 2 * n] for o, n in zip(recs["keys_off"][has], recs["nkeys"][has])]) if has.any() else np.zeros(0, np.int32)
