"""SAM text from the device's records: host Python for tests and scripting (the product boundary is the C ABI, bbmap_get_sam_records).

header() follows SamHeader.header0 / scaffolds (current/stream/SamHeader.java:33-66: @HD with the version and SO:unsorted, one @SQ per
scaffold in genome order); lines() follows SamLine.toBytes (current/stream/SamLine.java:1925-1959)."""
import numpy as np

TAG_XT = 1
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


def lines(records, text, names, reads, quals, scaffold_names, paired):
    """One SAM line (str) per record, as SamLine.toBytes prints it.  records: SAMREC_DTYPE array; text: the blob; names[r]: the read's
    name; reads[r]: its bases as they came in (bytes or uint8 array); quals: None, or per read numeric phred values (None = `*`);
    scaffold_names: by global scaffold number.  Null fields print `*` (:1930-1936, append :2056-2059); SEQ is reverse-complemented and
    QUAL reversed for a mapped minus-strand read (:1940-1946); tags in the order makeOptionalTags adds them: XT NM AM MD (:1489-1597)."""
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
        if int(rec["nm"]) >= 0:
            f.append("NM:i:%d" % int(rec["nm"]))
        if int(rec["am"]) >= 0:
            f.append("AM:i:%d" % int(rec["am"]))
        if ml > 0:
            f.append("MD:Z:" + text[int(rec["md_off"]): int(rec["md_off"]) + ml].tobytes().decode())
        out.append("\t".join(f))
    return out
