"""Test-local restatement of the reference's scaffold rules, the yardstick of the scaffold tests (the CPU oracle has no scaffold table):
Data.scaffoldIndex / Data.isSingleScaffold (current/dna/Data.java:1091-1140) and SamLine's coordinate block
(current/stream/SamLine.java:120-187, :267-268, with countLeadingClip / countTrailingClip / countLeadingIndels / countTrailingIndels,
:924-1020).  Tables are per chromosome number: locs[c] = ascending scaffold starts (entry 0 unused)."""
import bisect

import numpy as np

SCAFREC_DTYPE = np.dtype([("scaffold", "<i4"), ("start", "<i4"), ("stop", "<i4"), ("pos", "<i4"), ("end", "<i4"), ("scaflen", "<i4"),
                          ("flags", "<i4"), ("reserved", "<i4")])
MAPPED, PAIRED, INBOUNDS, SAME_SCAFFOLD = 1, 2, 4, 8


def _binary_search_rule(array, key):
    """Arrays.binarySearch + `exact hit, else max(0, insertPoint - 1)` (Data.java:1097-1107, :1117-1126)"""
    i = bisect.bisect_left(array, key)
    if i < len(array) and array[i] == key:
        return i
    return max(0, i - 1)


def scaffold_index(locs, pad, chrom, loc):
    """Data.scaffoldIndex (Data.java:1091-1108)"""
    array = locs[chrom]
    if array is None or len(array) < 2:
        return 0
    return _binary_search_rule(list(array), loc + pad // 2)


def is_single_scaffold(locs, pad, chrom, loc1, loc2):
    """Data.isSingleScaffold (Data.java:1111-1140)"""
    if locs is None:
        return True
    array = locs[chrom]
    if array is None or len(array) < 2:
        return True
    scaf = _binary_search_rule(list(array), loc1 + pad)
    if scaf == len(array) - 1:
        return True
    lower, upper = int(array[scaf]) - pad, int(array[scaf + 1])
    if loc2 < lower or loc1 > upper:
        return False
    return loc2 < upper


def count_leading_clip(match):
    """SamLine.countLeadingClip (:924-945)"""
    if not match or match[0] != ord("C"):
        return 0
    clips = current = 0
    for b in match:
        if 48 <= b <= 57:
            current = current * 10 + (b - 48)
        else:
            if current > 0:
                clips += current - 1
            current = 0
            if b != ord("C"):
                break
            clips += 1
    if current > 0:
        clips += current - 1
    return clips


def count_trailing_clip(match):
    """SamLine.countTrailingClip (:959-972)"""
    clips = 0
    for b in reversed(match or b""):
        if b == ord("C"):
            clips += 1
        else:
            break
    return clips


def count_leading_indels(rloc, match):
    """SamLine.countLeadingIndels (:975-996)"""
    if not match or rloc >= 0:
        return 0
    dels = inss = 0
    for b in match:
        if rloc >= 0:
            break
        if b == ord("D"):
            dels += 1
            rloc += 1
        elif b == ord("I"):
            inss += 1
        else:
            rloc += 1
    return dels - inss


def count_trailing_indels(rloc, rlen, match):
    """SamLine.countTrailingIndels (:999-1020): `if(match==null || rloc>=0){return 0;}`, and for rloc < 0 the loop condition
    rloc>=rlen is false at once -- 0 whenever rlen > 0."""
    if not match or rloc >= 0:
        return 0
    assert rlen > 0
    return 0


def scaffold_records(table, finals, matches, paired):
    """SamLine's block for each read: finals = per read (mapped, chrom, start, stop, paired) (a FINAL_DTYPE array), matches = per read
    bytes or None; table = (locs, lengths, pad, base) with base[c] = global number of chromosome c's first scaffold.  Returns a
    SCAFREC_DTYPE array."""
    locs, lengths, pad, base = table
    n = len(finals)
    out = np.zeros(n, SCAFREC_DTYPE)

    def mate(r):
        f = finals[r]
        if not int(f["mapped"]):
            return dict(mapped=False, single=True)
        chrom, start, stop = int(f["chrom"]), int(f["start"]), int(f["stop"])
        if not is_single_scaffold(locs, pad, chrom, start, stop):           # :126, :136-141
            return dict(mapped=False, single=False)
        idx = scaffold_index(locs, pad, chrom, (start + stop) // 2 if start + stop >= 0 else -((-(start + stop)) // 2))
        scaflen = int(lengths[chrom][idx])
        a1 = start - int(locs[chrom][idx])                                   # scaffoldRelativeLoc
        b1 = a1 - start + stop
        m = matches[r]
        pos0 = (a1 + 1) + count_leading_clip(m) + count_leading_indels(a1, m)           # :173-186
        pos1 = (b1 + 1) - count_trailing_clip(m) - count_trailing_indels(b1, scaflen, m)
        if pos1 > scaflen:
            pos1 = scaflen
        if pos0 < 1:
            pos0 = 1
        return dict(mapped=True, single=True, gscaf=int(base[chrom]) + idx, idx=idx, chrom=chrom, a1=a1, b1=b1, scaflen=scaflen,
                    pos0=pos0, pos1=pos1)

    def put(r, q, paired_after, same):
        rec = out[r]
        if q["mapped"]:
            rec["scaffold"], rec["start"], rec["stop"] = q["gscaf"], q["a1"], q["b1"]
            rec["pos"], rec["end"], rec["scaflen"] = q["pos0"], q["pos1"], q["scaflen"]
        else:
            rec["scaffold"] = -1
        inb = q["mapped"] and q["a1"] >= 0 and q["b1"] < q["scaflen"]         # :267-268
        rec["flags"] = (MAPPED if q["mapped"] else 0) | (PAIRED if paired_after else 0) | (INBOUNDS if inb else 0) | \
            (SAME_SCAFFOLD if same else 0)

    if not paired:
        for r in range(n):
            q = mate(r)
            put(r, q, bool(int(finals[r]["paired"])), False)
        return out
    for r in range(0, n - 1, 2):
        q1, q2 = mate(r), mate(r + 1)
        both = q1["single"] and q2["single"]                                 # setPaired(false) on both mates (:137-138, :157-158)
        same = q1["mapped"] and q2["mapped"] and q1["idx"] == q2["idx"] and q1["chrom"] == q2["chrom"]      # sameScaf (:160)
        put(r, q1, both and bool(int(finals[r]["paired"])), same)
        put(r + 1, q2, both and bool(int(finals[r + 1]["paired"])), same)
    return out


def table_of(packed):
    """(locs, lengths, pad, base) of a bbmap_amd.reference.Packed, indexed by chromosome number."""
    locs = [None] + [list(map(int, a)) for a in packed.locs]
    lengths = [None] + [list(map(int, a)) for a in packed.lengths]
    base = [0]
    acc = 0
    for a in packed.locs:
        base.append(acc)
        acc += len(a)
    return locs, lengths, packed.inter_scaffold_padding, base
