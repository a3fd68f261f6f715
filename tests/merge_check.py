"""Read.joinRead's overlapped branch (current/stream/Read.java:2744-2855), restated statement by statement for the merge tests: the
expected output of bbmerge_join_batch and bbmerge_join_batch_device.  Sequential on purpose: the loops run in Java's order over
Java's arrays, so nothing here shares a shape with the one-lane-per-base code under test.  `b` is mate 2 after BBMerge has
reverse-complemented it (Read.reverseComplement, :1127-1131: bases complemented and reversed, qualities reversed)."""
import numpy as np

MAX_MERGE_QUALITY = 41                     # Read.MAX_MERGE_QUALITY, maxq=


def _byte(x):
    """Java's (byte) cast of an int"""
    x &= 0xFF
    return x - 256 if x >= 128 else x


def join_read(a, b, insert, qa=None, qb=None, max_merge_quality=MAX_MERGE_QUALITY):
    """(bases, quals or None) of joinRead(a, b, insert), or None outside the overlapped branch (:2745 insert > 0, :2757 overlap <= 0).
    a, b: bytes; qa, qb: sequences of ints or None."""
    a_bases, b_bases = [_byte(x) for x in a], [_byte(x) for x in b]
    length_sum = len(a_bases) + len(b_bases)                              # :2746
    if insert <= 0:                                                       # :2745 (an assert in Java)
        return None
    overlap = min(insert, length_sum - insert)                            # :2747
    if overlap <= 0:                                                      # :2757, the branch left out
        return None
    bases = [0] * insert                                                  # :2750
    quals = None if qa is None or qb is None else [0] * insert            # :2751
    if quals is None:                                                     # :2805
        i = 0
        while i < len(a_bases) and i < len(bases):                        # :2806
            bases[i] = a_bases[i]                                         # :2807
            i += 1
        i, j = len(bases) - 1, len(b_bases) - 1                           # :2809
        while i >= 0 and j >= 0:
            ca, cb = bases[i], b_bases[j]                                 # :2810
            if ca == 0 or ca == ord("N"):                                 # :2811
                bases[i] = cb                                             # :2812
            elif ca == cb:                                                # :2813
                pass
            else:
                bases[i] = ca if ca >= cb else cb                         # :2815
            i -= 1
            j -= 1
    else:
        a_quals, b_quals = [_byte(int(x)) for x in qa], [_byte(int(x)) for x in qb]
        i = 0
        while i < len(a_bases) and i < len(bases):                        # :2820
            bases[i] = a_bases[i]                                         # :2821
            quals[i] = a_quals[i]                                         # :2822
            i += 1
        i, j = len(bases) - 1, len(b_bases) - 1                           # :2824
        while i >= 0 and j >= 0:
            ca, cb = bases[i], b_bases[j]                                 # :2825
            q_a, q_b = quals[i], b_quals[j]                               # :2826
            if ca == 0 or ca == ord("N"):                                 # :2827
                bases[i] = cb                                             # :2828
                quals[i] = q_b                                            # :2829
            elif cb == 0 or cb == ord("N"):                               # :2830
                pass
            elif ca == cb:                                                # :2832
                quals[i] = _byte(min(max(q_a, q_b) + int(min(q_a, q_b) / 4), max_merge_quality))       # :2833 (Java's / truncates)
            else:
                bases[i] = ca if q_a > q_b else cb if q_a < q_b else ord("N")                          # :2835
                quals[i] = _byte(max(q_a, q_b) - min(q_a, q_b))                                        # :2836
            i -= 1
            j -= 1
    out = bytes(x & 0xFF for x in bases)
    return out, (None if quals is None else np.array([x & 0xFF for x in quals], np.uint8))
