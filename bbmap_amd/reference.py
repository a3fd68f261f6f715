"""FASTA in, chromosome arrays out: what BBMap's index build does to a reference before anything is indexed.

read_fasta follows FastaToChromArrays2.nextScaffold (current/dna/FastaToChromArrays2.java:527-551) and the base conversion of
ChromosomeArray.set (current/dna/ChromosomeArray.java:168-190); pack follows makeNextChrom (:432-524) line by line.  The result feeds
DeviceIndex.build (the chromosome arrays, numbered from 1) and DeviceIndex.set_scaffolds (the scaffold table, Data.scaffoldLocs /
scaffoldLengths / scaffoldNames / interScaffoldPadding)."""
import gzip

import numpy as np

START_PADDING, MID_PADDING, END_PADDING = 8000, 300, 8000       # FastaToChromArrays2.java:569-571
MIN_SCAFFOLD = 1                                                # :572
MAX_LENGTH = (1 << 29) - 200000                                 # :575

# ChromosomeArray.set with CHANGE_U_TO_T and CHANGE_DEGENERATE_TO_N (both true, ChromosomeArray.java:422-423): every byte through
# AminoAcid.baseToACGTN (AminoAcid.java:584, :599-609): A C G T N in either case -> upper case, U / u -> T, anything else -> N
_ACGTN = np.full(256, ord("N"), np.uint8)
for _c in b"ACGTN":
    _ACGTN[_c] = _ACGTN[_c + 32] = _c
_ACGTN[ord("U")] = _ACGTN[ord("u")] = ord("T")


def convert_bases(seq):
    """bytes -> uint8 array as ChromosomeArray stores it."""
    return _ACGTN[np.frombuffer(bytes(seq), np.uint8)]


def trim_name(name):
    """Data.trimScaffoldNames (current/dna/Data.java:1173-1190): the name up to its first whitespace."""
    for i, ch in enumerate(name):
        if ch.isspace():
            return name[:i]
    return name


def read_fasta(path, trim_names=False):
    """[(name, bases uint8 array)] in file order; plain or gzip (by the magic bytes).  The name is the header line without '>',
    kept whole as nextScaffold keeps it (trim_names: cut at the first whitespace).  Lines before the first header join a record
    without a name (nextScaffold appends them too); its name is None."""
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    opener = gzip.open if gz else open
    records, name, chunks, seen = [], None, [], False
    with opener(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")                         # ByteFile1.nextLine drops the line terminator
            if line[:1] == b">":
                if seen or chunks:
                    records.append((name, b"".join(chunks)))
                name, chunks, seen = line[1:].decode("latin-1"), [], True
            else:
                chunks.append(line)
    if seen or chunks:
        records.append((name, b"".join(chunks)))
    out = []
    for n, seq in records:
        if n is not None and trim_names:
            n = trim_name(n)
        out.append((n, convert_bases(seq)))
    return out


class Packed:
    """chroms: list of uint8 arrays (chromosome 1 first); per chromosome locs / lengths (int32 arrays) and names (lists), all indexed
    from 0 = chromosome 1; inter_scaffold_padding = mid_pad."""

    def __init__(self, chroms, locs, lengths, names, inter_scaffold_padding):
        self.chroms, self.locs, self.lengths, self.names = chroms, locs, lengths, names
        self.inter_scaffold_padding = inter_scaffold_padding

    @property
    def nchroms(self):
        return len(self.chroms)

    def scaffold_names(self):
        """Every scaffold's name by global number (FASTA order among the packed scaffolds)."""
        return [n for ns in self.names for n in ns]

    def scaffold_bases(self):
        """[(chromosome number, start, length)] by global scaffold number."""
        return [(c + 1, int(a), int(l)) for c in range(self.nchroms) for a, l in zip(self.locs[c], self.lengths[c])]


def pack(records, start_pad=START_PADDING, mid_pad=MID_PADDING, end_pad=END_PADDING, min_scaffold=MIN_SCAFFOLD, max_length=MAX_LENGTH,
         merge=True):
    """FastaToChromArrays2.makeNextChrom (:432-524), called until the records run out.  records: [(name, bases)] (read_fasta's;
    bases as ChromosomeArray stores them, or anything convert_bases accepts)."""
    recs = [(n, b if isinstance(b, np.ndarray) and b.dtype == np.uint8 else convert_bases(b)) for n, b in records]
    chroms, locs, lengths, names = [], [], [], []
    it = iter(recs)
    current = None                  # currentScaffold: a record that did not fit the previous chromosome
    while True:
        arr = [np.full(start_pad, ord("N"), np.uint8)]     # :434: for(i<START_PADDING) ca.set(i, 'N')
        max_index = start_pad - 1
        lo, le, na = [], [], []
        scaffolds = 0
        if current is not None and len(current[1]) > 0:     # :440-459: the carried record opens the chromosome, whatever its length
            lo.append(max_index + 1); le.append(len(current[1])); na.append(current[0])
            arr.append(current[1]); max_index += len(current[1])
            scaffolds += 1
            current = None
        for rec in it:                                      # :463-480
            if len(rec[1]) + mid_pad + end_pad + max_index > max_length:
                current = rec
                break
            if scaffolds > 0 and not merge:
                current = rec
                break
            if scaffolds > 0:                               # MID_PADDING only between scaffolds -- also before one that is skipped
                arr.append(np.full(mid_pad, ord("N"), np.uint8)); max_index += mid_pad
            if len(rec[1]) >= min_scaffold:
                lo.append(max_index + 1); le.append(len(rec[1])); na.append(rec[0])
                arr.append(rec[1]); max_index += len(rec[1])
                scaffolds += 1
        if scaffolds == 0:                                  # :484
            break
        ca = np.concatenate(arr)
        if end_pad > 0:                                     # :486-500: count terminal N up to END_PADDING, then add N while
            terminal = 0                                    # terminalN <= END_PADDING -- END_PADDING + 1 - terminalN of them
            i = max_index
            while i >= 0 and terminal < end_pad:
                if ca[i] == ord("N"):
                    terminal += 1
                else:
                    break
                i -= 1
            add = 0
            while terminal <= end_pad and max_index + add < max_length - 1:
                add += 1
                terminal += 1
            ca = np.concatenate([ca, np.full(add, ord("N"), np.uint8)])
        chroms.append(ca)
        locs.append(np.array(lo, np.int32)); lengths.append(np.array(le, np.int32)); names.append(na)
        if current is None:
            break                                           # the records ran out inside this chromosome
    return Packed(chroms, locs, lengths, names, mid_pad)
