"""SAM text from the device's records: host Python for tests and scripting (the product boundary is the C ABI, bbmap_get_sam_records).

header() follows SamHeader.header0 / scaffolds (current/stream/SamHeader.java:33-66: @HD with the version and SO:unsorted, one @SQ per
scaffold in genome order); lines() follows SamLine.toBytes (current/stream/SamLine.java:1925-1959)."""
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

TAG_XT = 1
# BBMAP_SAM_MAKE_* in the header's order (include/bbmap_amd.h): bbmap_sam_config.tags and bbmap_samtags.present
(MAKE_NM, MAKE_AM, MAKE_SM, MAKE_XM, MAKE_XS, XS_SECONDSTRAND, MAKE_NH, MAKE_STOP, MAKE_LENGTH, MAKE_IDENTITY, MAKE_SCORE, MAKE_INSERT,
 MAKE_BOUNDS, NO_TAGS) = (1 << i for i in range(14))
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTNacgtn", b"TGCANtgcan"):
    _COMP[_a] = _b


def header(packed, cigar13=False):
    """@HD / @SQ lines (a list of str, no line ends) from a bbmap_amd.reference.Packed's scaffold names and lengths."""
    out = ["@HD\tVN:%s\tSO:unsorted" % ("1.3" if cigar13 else "1.4")]
    for names, lengths in zip(packed.names, packed.lengths):
        for n, ln in zip(names, lengths):
            out.append("@SQ\tSN:%s\tLN:%d" % (n, int(ln)))
    return out


def qname(name, paired):
    """The QNAME rule of SamLine.java:102-112: tabs become '_'; with a mate, a trailing ' 1', ' 2', '/1' or '/2' is cut off."""
    q = name.replace("\t", "_")
    if paired and len(q) > 2 and q[-1] in "12" and q[-2] in " /":
        q = q[:-2]
    return q


def identity_tag(good, bad, perfect):
    """makeIdentityTag (SamLine.java:1326-1330) from bbmap_samtags' yi_good / yi_bad / yi_perfect.  f is a Java float, and
    String.format("%.2f") rounds the exact binary value of the float product 100*f HALF_UP (Python's % rounds half-even: 3.125 -> 3.12)."""
    if perfect:
        return "YI:f:100"
    f = np.float32(good) / np.float32(max(int(good) + int(bad), 1))
    x = np.float32(100) * f
    return "YI:f:" + str(Decimal(float(x)).quantize(Decimal("0.01"), rounding=ROUND_HALF_UP))


def splice_counts(tags, paired):
    """(readCountSplice1, readCountSplice2) of a batch: the reads per mate with splices > 0 (AbstractMapThread.java:1528, :1679), the
    numerators of the table's "Splice Rate" line (AbstractMapper.java:1472, :1615: readCountSplice * 100 / mapped reads)."""
    hit = np.asarray(tags["splices"]) > 0
    if not paired:
        return int(hit.sum()), 0
    return int(hit[0::2].sum()), int(hit[1::2].sum())


def lines(records, text, names, reads, quals, scaffold_names, paired, tags=None):
    """One SAM line (str) per record, as SamLine.toBytes prints it.  records: SAMREC_DTYPE array; text: the blob; names[r]: the read's
    name; reads[r]: its bases as they came in (bytes or uint8 array); quals: None, or per read numeric phred values (None = `*`);
    scaffold_names: by global scaffold number; tags: None or the SAMTAGS_DTYPE array of the same call.  Null fields print `*`
    (:1930-1936, append :2056-2059); SEQ is reverse-complemented and QUAL reversed for a mapped minus-strand read (:1940-1946); tags in the
    order makeOptionalTags adds them: XT NM SM AM XM XS MD NH YS YL YI YR X8 XB (:1489-1681)."""
    text = np.asarray(text, np.uint8)
    out = []

    def ref(i):
        i = int(i)
        return "*" if i == -1 else "=" if i == -2 else scaffold_names[i]

    for r, rec in enumerate(records):
        flag = int(rec["flag"])
        cl, ml = int(rec["cigar_len"]), int(rec["md_len"])
        cigar = text[int(rec["cigar_off"]): int(rec["cigar_off"]) + cl].tobytes().decode() if cl > 0 else "*"
        seq = np.frombuffer(bytes(reads[r]), np.uint8) if not isinstance(reads[r], np.ndarray) else reads[r]
        q = None if quals is None else quals[r]
        minus = (flag & 0x4) == 0 and (flag & 0x10) != 0         # mapped() && strand()==Gene.MINUS
        if minus:
            seq = _COMP[seq[::-1]]
        seq_s = bytes(seq).decode() if len(seq) else "*"
        if q is None:
            qual_s = "*"
        else:
            qq = np.asarray(q, np.uint8)[::-1] if minus else np.asarray(q, np.uint8)
            qual_s = bytes(qq + 33).decode()
        f = [qname(names[r], paired), str(flag), ref(rec["rname"]), str(int(rec["pos"])), str(int(rec["mapq"])), cigar, ref(rec["rnext"]),
             str(int(rec["pnext"])), str(int(rec["tlen"])), seq_s, qual_s]
        if int(rec["tags"]) & TAG_XT:
            f.append("XT:A:R")
        t = None if tags is None else tags[r]
        have = 0 if t is None else int(t["present"])
        if int(rec["nm"]) >= 0:
            f.append("NM:i:%d" % int(rec["nm"]))
        if have & MAKE_SM:
            f.append("SM:i:%d" % int(t["sm"]))
        if int(rec["am"]) >= 0:
            f.append("AM:i:%d" % int(rec["am"]))
        if have & MAKE_XM:
            f.append("XM:i:%d" % int(t["xm"]))
        if have & MAKE_XS:
            f.append("XS:A:+" if int(t["xs"]) > 0 else "XS:A:-")
        if ml > 0:
            f.append("MD:Z:" + text[int(rec["md_off"]): int(rec["md_off"]) + ml].tobytes().decode())
        if have & MAKE_NH:
            f.append("NH:i:%d" % int(t["nh"]))
        if have & MAKE_STOP:
            f.append("YS:i:%d" % int(t["ys"]))
        if have & MAKE_LENGTH:
            f.append("YL:Z:%d,%d" % (int(t["yl_query"]), int(t["yl_ref"])))
        if have & MAKE_IDENTITY:
            f.append(identity_tag(int(t["yi_good"]), int(t["yi_bad"]), bool(int(t["yi_perfect"]))))
        if have & MAKE_SCORE:
            f.append("YR:i:%d" % int(t["yr"]))
        if have & MAKE_INSERT:
            f.append("X8:Z:%d" % int(t["x8"]))
        if have & MAKE_BOUNDS:
            xb = int(t["xb"])
            f.append("XB:Z:" + chr(xb & 0xff) + (chr(xb >> 8 & 0xff) if xb >> 8 else ""))
        out.append("\t".join(f))
    return out
