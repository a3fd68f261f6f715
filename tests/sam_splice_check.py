"""Test-local restatement of stream.SamLine under an intron limit and with the optional tags switched on: the yardstick of the spliced-read
SAM tests.  Sequential, one symbol at a time, statement by statement after the Java text -- nothing of the device's 64-symbol scheme.

What the limit does not touch is taken from tests/sam_check.py (pinned by hand in tests/test_sam_cpu.py): makeFlag, toMapq, the shortcut
tests, calcLeftClip / calcRightClip.  Restated here with the limit: toCigar14 / toCigar13 (current/stream/SamLine.java:679-750, :600-663),
the NM loop (:1514-1535), makeMdTag (:1361-1445), and new: makeXSTag (:1346-1359), makeStopTag / makeLengthTag / makeIdentityTag
(:1316-1330) with calcCigarLength / countLeadingClip (:757-846), Read.identityFlat (current/stream/Read.java:1529-1596),
Read.countErrors (:2189-2240), Read.insertSizeMapped (:2618-2670), XM / NH / X8 / XB (:1565-1581, :1599-1619, :1673-1681).

At intron_limit = 2**31 - 1 with the default tags every field and byte equals tests/sam_check.py's (tests/test_sam_splice_cpu.py)."""
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

from tests import sam_check as SK
from tests import scaffold_check as SC

SAMREC_DTYPE = SK.SAMREC_DTYPE
SAMTAGS_DTYPE = np.dtype([(n, "<i4") for n in ("present", "xs", "nh", "sm", "xm", "ys", "yl_query", "yl_ref", "yi_good", "yi_bad",
                                               "yi_perfect", "yr", "x8", "xb", "introns", "splices")])
assert SAMTAGS_DTYPE.itemsize == 64
CIGAR13, MD = 1, 2
NM, AM, SM, XM, XS, XS_SECONDSTRAND, NH, STOP, LENGTH, IDENTITY, SCORE, INSERT, BOUNDS, NO_TAGS = (1 << i for i in range(14))
ALL_TAGS = NM | AM | SM | XM | XS | NH | STOP | LENGTH | IDENTITY | SCORE | INSERT | BOUNDS
INT_MAX = 2 ** 31 - 1
f32 = np.float32


def to_cigar(match, read_start, read_stop, reflen, v13, intron_limit):
    """toCigar14 (:679-750) / toCigar13 (:600-663)"""
    if match is None or read_start == read_stop:
        return None
    sb = []
    count = 0
    mode = "="
    last_mode = "="
    refloc = read_start
    for b in match:
        m = chr(b)
        sfdflag = False
        if refloc < 0 or refloc >= reflen:                  # SOFT_CLIP (:696-699)
            mode = "S"
            if m != "I":
                refloc += 1
            if m == "D":
                sfdflag = True
        elif m in "ms" or (v13 and m in "SNB"):             # :700 / :621
            mode = "M" if v13 else "="
            refloc += 1
        elif m == "S":
            mode = "X"
            refloc += 1
        elif m in "IXY":
            mode = "I"
        elif m == "D":
            mode = "D"
            refloc += 1
        elif m == "C":
            mode = "S"
            refloc += 1
        elif m in "NB":
            mode = "M"
            refloc += 1
        else:
            raise RuntimeError("Invalid match string character " + m)
        if mode != last_mode:                               # :722-732
            if count > 0:
                sb.append(str(count))
                sb.append("N" if last_mode == "D" and count > intron_limit else last_mode)
            count = 0
            last_mode = mode
        count += 1
        if sfdflag:
            count -= 1
    sb.append(str(count))                                   # :737-742
    sb.append("N" if mode == "D" and count > intron_limit else mode)
    return "".join(sb)


def calc_cigar_length(cigar, include_soft_clip):
    """calcCigarLength (:757-789), includeHardClip false"""
    if cigar is None:
        return 0
    ln = current = 0
    for c in cigar:
        if c.isdigit():
            current = current * 10 + int(c)
        else:
            if c in "M=XDN":
                ln += current
            elif c == "S":
                if include_soft_clip:
                    ln += current
            elif c not in "HI":
                raise RuntimeError("Unhandled cigar symbol: " + c)
            current = 0
    return ln


def count_leading_clip_cigar(cigar):
    """countLeadingClip(cigar, true, false) (:822-846)"""
    if cigar is None:
        return 0
    ln = current = 0
    for c in cigar:
        if c.isalpha() or c == "=":
            if c == "S":
                ln += current
            elif c != "H":
                break
            current = 0
        else:
            current = current * 10 + int(c)
    return ln


def calc_nm(match, cigar, length, intron_limit):
    """the NM loop of makeOptionalTags (:1514-1535)"""
    nm = 0
    frm, to = SK.calc_left_clip(cigar), length - SK.calc_right_clip(cigar)
    dels_current = 0
    cpos = 0
    for b in match:
        c = chr(b)
        if frm <= cpos < to:
            if c in "ISNXY":
                nm += 1
            if c == "D":
                dels_current += 1
            else:
                if dels_current <= intron_limit:
                    nm += dels_current
                dels_current = 0
        if c != "D":
            cpos += 1
    if dels_current <= intron_limit:
        nm += dels_current
    return nm


def make_md_tag(chrom_arr, refstart, match, call, scafloc, scaflen, intron_limit):
    """makeMdTag (:1361-1445) without the "MD:Z:" in front; call = Read.bases as the read came in"""
    if match is None:
        return None
    md = []
    scafstop = scafloc + scaflen
    prev_m = "?"
    count = 0
    dels = 0
    prev_sub = False
    rpos, cpos = refstart, 0
    for b in match:
        c = int(call[cpos]) if cpos < len(call) else -1
        m = chr(b)
        if prev_m == "D" and m != "D":
            if dels <= intron_limit:                        # "Otherwise, ignore it" (:1380): and dels is NOT reset
                md.append(str(count))
                count = 0
                md.append("^")
                for i in range(rpos - dels, rpos):
                    md.append(chr(SK.chrom_get(chrom_arr, i)))
                dels = 0
        if m == "C" or rpos < scafloc or rpos >= scafstop:
            rpos += 1
            if m != "D":
                cpos += 1
        elif m in "ms":
            count += 1
            rpos += 1
            cpos += 1
        elif m == "S" or (m == "N" and c != SK.chrom_get(chrom_arr, rpos)):
            if count > 0 or not prev_sub:
                md.append(str(count))
            md.append(chr(SK.chrom_get(chrom_arr, rpos)))
            count = 0
            rpos += 1
            cpos += 1
            prev_sub = True
        elif m == "N":
            count += 1
            rpos += 1
            cpos += 1
        elif m in "IXY":
            cpos += 1
        elif m == "D":
            rpos += 1
            dels += 1
        prev_m = m
    md.append(str(count))
    return "".join(md)


def identity_counts(match, intron_limit):
    """Read.identityFlat (Read.java:1529-1596) on a long-format string: (good, bad) after the `n` folding of :1586-1588"""
    good = bad = n = 0
    mode, c, current = "0", "0", 0

    def close(mode, current):
        nonlocal good, bad, n
        if mode == "m":
            good += current
        elif mode in "RN":
            n += current
        elif mode == "C":
            pass
        elif mode != "0":
            if mode != "D" or current < intron_limit:
                bad += current

    for b in match:
        c = chr(b)
        assert not c.isdigit()
        if mode == c:
            current = max(current + 1, 2)
        else:
            current = max(current, 1)
            close(mode, current)
            mode = c
            current = 0
    current = max(current, 1)                               # :1567-1583 (`!Character.isDigit(c)` holds)
    close(mode, current)
    n = (n + 3) // 4
    return good + n, bad + 3 * n


def identity_text(good, bad, perfect):
    """makeIdentityTag (:1326-1330): String.format("%.2f") of the float product, which rounds the exact binary value HALF_UP"""
    if perfect:
        return "YI:f:100"
    f = f32(good) / f32(max(good + bad, 1))
    x = f32(100) * f
    return "YI:f:" + str(Decimal(float(x)).quantize(Decimal("0.01"), rounding=ROUND_HALF_UP))


def count_splices(match, min_splice):
    """Read.countErrors(minSplice)[5] (Read.java:2189-2240)"""
    prev = " "
    streak = splice = 0
    min_splice = max(min_splice, 1)
    for b in match:
        c = chr(b)
        streak = streak + 1 if c == prev else 1
        if c == "D" and streak == min_splice:
            splice += 1
        prev = c
    return splice


def _unstranded(r1, r2):
    """insertSizeMapped_Unstranded (:2643-2670), r2 != null"""
    if r1["start"] > r2["start"]:
        return _unstranded(r2, r1)
    if r1["start"] == r1["stop"] or r2["start"] == r2["stop"]:
        return 0
    if r1["chrom"] != r2["chrom"]:
        return 0
    a, b = r1["length"], r2["length"]
    if r1["start"] < r2["start"]:
        mid = r2["start"] - r1["stop"] - 1
        if -mid >= a + b:
            return 0
        return mid + a + b
    return min(a, b)


def _plus_left(r1, r2):
    """insertSizeMapped_PlusLeft (:2629-2641)"""
    if r1["strand"] > r2["strand"]:
        return _plus_left(r2, r1)
    if r1["strand"] == r2["strand"] or r1["start"] > r2["stop"]:
        return _unstranded(r2, r1)
    if r1["chrom"] != r2["chrom"]:
        return 0
    if r1["start"] == r1["stop"] or r2["start"] == r2["stop"]:
        return 0
    a, b = r1["length"], r2["length"]
    mid = r2["start"] - r1["stop"] - 1
    if -mid >= a + b:
        return _unstranded(r1, r2)
    return mid + a + b


def insert_size_mapped(r1, r2):
    """insertSizeMapped(r1, r2, false) (:2622-2626), r2 != null"""
    if not r1["mapped"] or not r2["mapped"] or r1["strand"] == r2["strand"]:
        return _unstranded(r1, r2)
    return _plus_left(r1, r2)


def sam_records(table, finals, matches, lengths, calls, chroms, paired, flags=0, intron_limit=INT_MAX, tags=NM | AM, site_scores=None,
                scaf=None):
    """SamLine per read, as tests/sam_check.sam_records, under an intron limit and a tag mask.  site_scores[r] = the scores of read r's
    site list in list order (XM); scaf: a SCAFREC_DTYPE array written by hand (then table is not read).  Returns (SAMREC_DTYPE array,
    SAMTAGS_DTYPE array, text bytes, [(cigar, md)] per read)."""
    n = len(finals)
    if scaf is None:
        scaf = SC.scaffold_records(table, finals, matches, paired)
    out = np.zeros(n, SAMREC_DTYPE)
    tg = np.zeros(n, SAMTAGS_DTYPE)
    strings = []
    v13 = bool(flags & CIGAR13)

    def view(r):
        s, f = scaf[r], finals[r]
        mapped = bool(int(s["flags"]) & SC.MAPPED)
        match = matches[r] if mapped and matches[r] else None            # r.match=null with setMapped(false) (:136-138)
        return dict(mapped=mapped, match=match, pos0=int(s["pos"]) if mapped else 0, pos1=int(s["end"]) if mapped else 0,
                    pos1_raw=int(s["stop"]) + 1 - SK.trailing_clip(match) if mapped else 0,
                    name=int(s["scaffold"]) if mapped else -1, a=int(s["start"]), b=int(s["stop"]), scaflen=int(s["scaflen"]) if mapped else 0,
                    start=int(f["start"]), stop=int(f["stop"]), strand=int(f["strand"]), score=int(f["mapScore"]),
                    ambig=bool(int(f["ambiguous"])), perfect=bool(int(f["perfect"])), paired=bool(int(s["flags"]) & SC.PAIRED),
                    chrom=int(f["chrom"]), inbounds=bool(int(s["flags"]) & SC.INBOUNDS), same=bool(int(s["flags"]) & SC.SAME_SCAFFOLD),
                    length=int(lengths[r]))

    for r in range(n):
        a = view(r)
        has_mate = bool(paired)
        b = view(r ^ 1) if has_mate else None
        rec, t = out[r], tg[r]
        same = a["same"]
        rec["flag"] = SK.make_flag(a["mapped"], a["match"], a["paired"], a["strand"], has_mate, b["mapped"] if b else False,
                                   b["match"] if b else None, b["strand"] if b else 0, r & 1, same)
        rname = a["name"] if a["mapped"] else (b["name"] if b and b["mapped"] else -1)          # :164
        pos0, pos1 = a["pos0"], a["pos1"]
        if b is not None and b["mapped"]:
            pos0m, pos1m = b["pos0"], b["pos1_raw"]
            if pos1m > a["scaflen"]:                        # :207
                pos1 = a["scaflen"]
        else:
            pos0m = pos1m = 0
        if b is None:                                       # :220-253
            pos, pnext, tlen = pos0, pos0m, 0
        elif a["mapped"] and b["mapped"]:
            pos, pnext = pos0, pos0m
            tlen = 1 + (max(pos1, pos1m) - min(pos0, pos0m)) if same else 0
        elif a["mapped"]:
            pos, pnext, tlen = pos0, pos0, 0
        elif b["mapped"]:
            pos, pnext, tlen = pos0m, pos0m, 0
        else:
            pos, pnext, tlen = pos0, pos0m, 0
        mapq = SK.to_mapq(a["score"], a["length"], a["mapped"], a["ambig"])
        cigar = None
        if a["mapped"] and a["match"] is not None:          # :269-301
            if not v13:
                if a["inbounds"] and a["perfect"] and not SK.contains_non_m(a["match"]):
                    cigar = "%d=" % a["length"]
                else:
                    cigar = to_cigar(a["match"], a["a"], a["b"], a["scaflen"], False, intron_limit)
            else:
                if a["inbounds"] and (a["perfect"] or not SK.contains_non_nms(a["match"])):
                    cigar = "%dM" % a["length"]
                else:
                    cigar = to_cigar(a["match"], a["a"], a["b"], a["scaflen"], True, intron_limit)
        if b is None or (not a["mapped"] and not b["mapped"]):                                  # :315
            rnext = -1
        elif a["mapped"] and b["mapped"]:
            rnext = -2 if same else b["name"]
        else:
            rnext = -2
        if not (b is None or a["start"] < b["start"] or (a["start"] == b["start"] and (r & 1) == 0)):      # :349-354
            tlen = -tlen
        nm = am = -1
        xt = 0
        md = None
        t["introns"] = cigar.count("N") if cigar else 0
        if a["match"] is not None:
            t["splices"] = count_splices(a["match"], intron_limit)
        if a["mapped"] and not tags & NO_TAGS:              # makeOptionalTags (:1481-1684)
            perfect = a["perfect"]
            present = 0
            if a["ambig"]:
                xt = 1
            if tags & NM:                                   # :1544-1547
                if perfect:
                    nm = 0
                elif a["match"] is not None:
                    nm = calc_nm(a["match"], cigar, a["length"], intron_limit)
            if tags & SM:                                   # :1548
                present |= SM
                t["sm"] = mapq
            if b is None:                                   # :1549
                other = mapq
            elif b["mapped"]:
                q = abs(b["score"]) // b["length"]          # Java's int division truncates toward zero
                other = max(1, q if b["score"] >= 0 else -q)
            else:
                other = 0
            if tags & AM:
                am = min(mapq, other)
            if tags & XM:                                   # :1565-1581
                x = 1
                ss = site_scores[r] if site_scores is not None else []
                if len(ss) > 0:
                    x += sum(1 for z in ss[1:] if z == ss[0])
                if a["ambig"]:
                    x = max(x, 2)
                present |= XM
                t["xm"] = x
            if tags & XS and cigar is not None and "N" in cigar:       # makeXSTag (:1346-1359)
                plus = a["strand"] == 0
                if has_mate and (r & 1) != 0:
                    plus = not plus
                if tags & XS_SECONDSTRAND:
                    plus = not plus
                present |= XS
                t["xs"] = 1 if plus else -1
            if flags & MD:                                  # :1594-1597
                md = make_md_tag(chroms[a["chrom"] - 1], a["start"], a["match"], calls[r], a["start"] - a["a"], a["scaflen"], intron_limit)
            if tags & NH:                                   # :1599-1605
                present |= NH
                t["nh"] = 1
            if perfect or a["match"] is not None:           # :1607-1611 (r.bases != null)
                if tags & STOP:                             # makeStopTag (:1316-1319); pos = the line's POS
                    present |= STOP
                    t["ys"] = pos + (a["length"] if cigar is None or perfect else calc_cigar_length(cigar, True)) - 1
                if tags & LENGTH:                           # makeLengthTag (:1321-1324)
                    present |= LENGTH
                    if cigar is None or perfect:
                        t["yl_query"] = t["yl_ref"] = a["length"]
                    else:
                        t["yl_query"] = a["length"] - count_leading_clip_cigar(cigar)
                        t["yl_ref"] = calc_cigar_length(cigar, False)
                if tags & IDENTITY:                         # makeIdentityTag (:1326-1330)
                    present |= IDENTITY
                    t["yi_perfect"] = int(perfect)
                    if not perfect:
                        t["yi_good"], t["yi_bad"] = identity_counts(a["match"], intron_limit)
            if tags & SCORE:                                # :1613
                present |= SCORE
                t["yr"] = a["score"]
            if tags & INSERT and b is not None:             # :1615-1619 (no originalSite)
                present |= INSERT
                t["x8"] = insert_size_mapped(a, b)
            if tags & BOUNDS:                               # :1673-1681
                present |= BOUNDS
                xb = ord("I" if a["inbounds"] else "O")
                if b is not None:
                    xb |= ord(("I" if b["inbounds"] else "O") if b["mapped"] else "U") << 8
                t["xb"] = xb
            t["present"] = present
        rec["rname"], rec["rnext"], rec["pos"], rec["pnext"], rec["tlen"], rec["mapq"] = rname, rnext, pos, pnext, tlen, mapq
        rec["nm"], rec["am"], rec["tags"] = nm, am, xt
        strings.append((cigar, md))
    text = bytearray()
    for r, (cigar, md) in enumerate(strings):               # packed in read order: CIGAR, then MD
        out[r]["cigar_off"] = len(text)
        out[r]["cigar_len"] = len(cigar) if cigar else 0
        text += (cigar or "").encode()
        out[r]["md_off"] = len(text)
        out[r]["md_len"] = len(md) if md else 0
        text += (md or "").encode()
    return out, tg, bytes(text), strings
