"""Test-local restatement of the rest of stream.SamLine's constructor (current/stream/SamLine.java:82-413), the yardstick of the SAM
tests (the CPU oracle has no SamLine).  Built on scaffold_check.scaffold_records, which restates the coordinate block; every function
below follows the Java text statement by statement, sequentially, one symbol at a time -- nothing of the device's 64-symbol scheme.

Fixed as in the device code: SOFT_CLIP = true, PENALIZE_AMBIG = true, INTRON_LIMIT = Integer.MAX_VALUE, NM and AM tags on."""
import math

import numpy as np

from tests import scaffold_check as SC

SAMREC_DTYPE = np.dtype([("flag", "<i4"), ("mapq", "<i4"), ("rname", "<i4"), ("rnext", "<i4"), ("pos", "<i4"), ("pnext", "<i4"),
                         ("tlen", "<i4"), ("nm", "<i4"), ("am", "<i4"), ("tags", "<i4"), ("cigar_off", "<i8"), ("cigar_len", "<i4"),
                         ("md_len", "<i4"), ("md_off", "<i8")])
CIGAR13, MD = 1, 2
f32 = np.float32


def make_flag(mapped, match, paired_flag, strand, has_mate, mate_mapped, mate_match, mate_strand, frag_num, same_scaf):
    """makeFlag (:2134-2151); valid() is true, secondary() and discarded() false"""
    flag = 0
    if has_mate:
        flag |= 0x1
        if mapped and match is not None and (same_scaf and paired_flag and mate_mapped and mate_match is not None):
            flag |= 0x2
        if frag_num == 0:
            flag |= 0x40
        if frag_num > 0:
            flag |= 0x80
    if not mapped:
        flag |= 0x4
    if has_mate and not mate_mapped:
        flag |= 0x8
    if strand == 1:
        flag |= 0x10
    if has_mate and mate_strand == 1:
        flag |= 0x20
    return flag


def java_round(x):
    """Math.round(float): floor(x + 1/2), exact (the float goes to double first)"""
    return int(math.floor(float(x) + 0.5))


def to_mapq(score, length, mapped, ambig):
    """toMapq (:1709-1721), float arithmetic one operation at a time; Tools.log2 = Math.log(d) * (1 / Math.log(2)) in double
    (current/align2/Tools.java:2304-2317)"""
    if not mapped or length < 1:
        return 0
    if ambig:
        mx = f32(3)
        adjusted = f32(f32(score) * mx) / f32(f32(100) * f32(length))
        return max(1, java_round(f32(adjusted)))
    score2 = f32(f32(score - length * 40) * f32(1.6))
    mx = f32(f32(f32(1.5) * f32(math.log(length) * (1 / math.log(2)))) + f32(36))
    adjusted = f32(f32(score2 * mx) / f32(f32(100) * f32(length)))
    return max(4, java_round(adjusted))


def _to_cigar(match, read_start, read_stop, reflen, v13):
    """toCigar14 (:679-750) / toCigar13 (:600-663): the two differ in the class table only"""
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
        if refloc < 0 or refloc >= reflen:                  # SOFT_CLIP
            mode = "S"
            if m != "I":
                refloc += 1
            if m == "D":
                sfdflag = True
        elif v13 and m in "msSNB":
            mode = "M"
            refloc += 1
        elif not v13 and m in "ms":
            mode = "="
            refloc += 1
        elif not v13 and m == "S":
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
        elif not v13 and m in "NB":
            mode = "M"
            refloc += 1
        else:
            raise RuntimeError("Invalid match string character " + m)
        if mode != last_mode:
            if count > 0:
                sb.append(str(count))
                sb.append(last_mode)                        # (count > INTRON_LIMIT never holds)
            count = 0
            last_mode = mode
        count += 1
        if sfdflag:
            count -= 1
    sb.append(str(count))
    sb.append(mode)
    return "".join(sb)


def to_cigar14(match, read_start, read_stop, reflen):
    return _to_cigar(match, read_start, read_stop, reflen, False)


def to_cigar13(match, read_start, read_stop, reflen):
    return _to_cigar(match, read_start, read_stop, reflen, True)


def contains_non_m(match):
    """Read.containsNonM (current/stream/Read.java:1815-1823)"""
    return any(b > ord("9") and b != ord("m") for b in match)


def contains_non_nms(match):
    """Read.containsNonNMS (:1855-1863)"""
    return any(b > ord("9") and chr(b) not in "msNS" for b in match)


def calc_left_clip(cig):
    """calcLeftClip (:1447-1460)"""
    if cig is None:
        return 0
    ln = 0
    for c in cig:
        if c.isdigit():
            ln = ln * 10 + int(c)
        else:
            return ln if c == "S" else 0
    return 0


def calc_right_clip(cig):
    """calcRightClip (:1462-1479)"""
    if cig is None or len(cig) < 1 or cig[-1] != "S":
        return 0
    pos = len(cig) - 2
    while pos >= 0 and cig[pos].isdigit():
        pos -= 1
    ln = 0
    for c in cig[pos + 1:]:
        if c.isdigit():
            ln = ln * 10 + int(c)
        else:
            return ln if c == "S" else 0
    return ln


def calc_nm(match, cigar, length):
    """the NM loop of makeOptionalTags (:1514-1535)"""
    nm = 0
    frm, to = calc_left_clip(cigar), length - calc_right_clip(cigar)
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
                nm += dels_current
                dels_current = 0
        if c != "D":
            cpos += 1
    nm += dels_current
    return nm


def chrom_get(arr, loc):
    """ChromosomeArray.get (current/dna/ChromosomeArray.java:232-234): minIndex 0, maxIndex = the array's last index"""
    return ord("N") if loc < 0 or loc >= len(arr) - 1 else int(arr[loc])


def make_md_tag(chrom_arr, refstart, match, call, scafloc, scaflen):
    """makeMdTag (:1361-1445) without the "MD:Z:" in front.  call = Read.bases as the read came in (see sam_records.hip)"""
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
            md.append(str(count))
            count = 0
            md.append("^")
            for i in range(rpos - dels, rpos):
                md.append(chr(chrom_get(chrom_arr, i)))
            dels = 0
        if m == "C" or rpos < scafloc or rpos >= scafstop:
            rpos += 1
            if m != "D":
                cpos += 1
        elif m in "ms":
            count += 1
            rpos += 1
            cpos += 1
        elif m == "S":
            if count > 0 or not prev_sub:
                md.append(str(count))
            md.append(chr(chrom_get(chrom_arr, rpos)))
            count = 0
            rpos += 1
            cpos += 1
            prev_sub = True
        elif m == "N":
            r = chrom_get(chrom_arr, rpos)
            if c == r:
                count += 1
                rpos += 1
                cpos += 1
            else:
                if count > 0 or not prev_sub:
                    md.append(str(count))
                md.append(chr(r))
                count = 0
                rpos += 1
                cpos += 1
                prev_sub = True
        elif m in "IXY":
            cpos += 1
        elif m == "D":
            rpos += 1
            dels += 1
        prev_m = m
    md.append(str(count))
    return "".join(md)


def trailing_clip(match):
    return SC.count_trailing_clip(match)


def sam_records(table, finals, matches, lengths, calls, chroms, paired, flags=0):
    """SamLine per read.  table / finals / matches as scaffold_check.scaffold_records takes them; lengths[r] = read length, calls[r] =
    the read's bases as it came in, chroms[c - 1] = chromosome c's array.  Returns (SAMREC_DTYPE array with offsets into the packed
    text, text bytes, [(cigar, md)] per read as str or None)."""
    n = len(finals)
    scaf = SC.scaffold_records(table, finals, matches, paired)
    out = np.zeros(n, SAMREC_DTYPE)
    strings = []
    v13 = bool(flags & CIGAR13)

    def view(r):
        s, f = scaf[r], finals[r]
        mapped = bool(int(s["flags"]) & SC.MAPPED)
        match = matches[r] if mapped and matches[r] else None            # r.match=null with setMapped(false) (:136-138)
        pos0 = int(s["pos"]) if mapped else 0
        pos1_unclamped = int(s["stop"]) + 1 - trailing_clip(match) if mapped else 0      # count_trailing_indels is 0
        return dict(mapped=mapped, match=match, pos0=pos0, pos1=int(s["end"]) if mapped else 0, pos1_raw=pos1_unclamped,
                    name=int(s["scaffold"]) if mapped else -1, a=int(s["start"]), b=int(s["stop"]), scaflen=int(s["scaflen"]) if mapped else 0,
                    start=int(f["start"]), strand=int(f["strand"]), score=int(f["mapScore"]), ambig=bool(int(f["ambiguous"])),
                    perfect=bool(int(f["perfect"])), paired=bool(int(s["flags"]) & SC.PAIRED), chrom=int(f["chrom"]),
                    inbounds=bool(int(s["flags"]) & SC.INBOUNDS), same=bool(int(s["flags"]) & SC.SAME_SCAFFOLD), length=int(lengths[r]))

    for r in range(n):
        a = view(r)
        has_mate = bool(paired)
        b = view(r ^ 1) if has_mate else None
        rec = out[r]
        same = a["same"]
        rec["flag"] = make_flag(a["mapped"], a["match"], a["paired"], a["strand"], has_mate, b["mapped"] if b else False,
                                b["match"] if b else None, b["strand"] if b else 0, r & 1, same)
        rname = a["name"] if a["mapped"] else (b["name"] if b and b["mapped"] else -1)          # :164
        pos0, pos1 = a["pos0"], a["pos1"]
        if b is not None and b["mapped"]:
            pos0m, pos1m = b["pos0"], b["pos1_raw"]
            if pos1m > a["scaflen"]:                        # `if(pos1_mate>scaflen){pos1=scaflen;}` (:207): pos1, and this line's scaflen
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
        mapq = to_mapq(a["score"], a["length"], a["mapped"], a["ambig"])
        cigar = None
        if a["mapped"] and a["match"] is not None:          # :269-301 (r1.bases != null)
            if not v13:
                if a["inbounds"] and a["perfect"] and not contains_non_m(a["match"]):
                    cigar = "%d=" % a["length"]
                else:
                    cigar = to_cigar14(a["match"], a["a"], a["b"], a["scaflen"])
            else:
                if a["inbounds"] and (a["perfect"] or not contains_non_nms(a["match"])):
                    cigar = "%dM" % a["length"]
                else:
                    cigar = to_cigar13(a["match"], a["a"], a["b"], a["scaflen"])
        if b is None or (not a["mapped"] and not b["mapped"]):                                  # :315
            rnext = -1
        elif a["mapped"] and b["mapped"]:
            rnext = -2 if same else b["name"]
        else:
            rnext = -2
        if not (b is None or a["start"] < b["start"] or (a["start"] == b["start"] and (r & 1) == 0)):      # :349-354
            tlen = -tlen
        nm = am = -1
        tags = 0
        md = None
        if a["mapped"]:                                     # makeOptionalTags (:1488-1549, :1594-1597)
            if a["ambig"]:
                tags |= 1
            if a["perfect"]:
                nm = 0
            elif a["match"] is not None:
                nm = calc_nm(a["match"], cigar, a["length"])
            if b is None:
                other = mapq
            elif b["mapped"]:
                q = abs(b["score"]) // b["length"]          # Java's int division truncates toward zero
                other = max(1, q if b["score"] >= 0 else -q)
            else:
                other = 0
            am = min(mapq, other)
            if flags & MD:
                md = make_md_tag(chroms[a["chrom"] - 1], a["start"], a["match"], calls[r], a["start"] - a["a"], a["scaflen"])
        rec["rname"], rec["rnext"], rec["pos"], rec["pnext"], rec["tlen"], rec["mapq"] = rname, rnext, pos, pnext, tlen, mapq
        rec["nm"], rec["am"], rec["tags"] = nm, am, tags
        strings.append((cigar, md))
    text = bytearray()
    for r, (cigar, md) in enumerate(strings):               # packed in read order: CIGAR, then MD
        out[r]["cigar_off"] = len(text)
        out[r]["cigar_len"] = len(cigar) if cigar else 0
        text += (cigar or "").encode()
        out[r]["md_off"] = len(text)
        out[r]["md_len"] = len(md) if md else 0
        text += (md or "").encode()
    return out, bytes(text), strings
