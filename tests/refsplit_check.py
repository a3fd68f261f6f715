"""Sequential restatement of align2.BBSplitter.printReads (current/align2/BBSplitter.java) for the tests of the device stage: it
works on Python sets of name strings, as the Java works on HashSet<String>, not on masks, so the device's mask arithmetic is checked
against something of another shape.  Line numbers are BBSplitter.java's unless another file is named.

A read is a dict: mapped, ambiguous, chrom, start, stop, mapScore, length, sites = [(chrom, start, stop, score), ...] in list order
(uncapped: capSiteList is applied here, AbstractMapThread.java:1309-1315)."""
import bisect
from collections import Counter

UNSET, FIRST, SPLIT, TOSS, RANDOM, ALL = 0, 1, 2, 3, 4, 5       # :1203-1208


def jdiv2(x):
    """Java's int division by 2: towards zero"""
    return -((-x) // 2) if x < 0 else x // 2


class Reference:
    """Data.scaffoldLocs / scaffoldNames / interScaffoldPadding: locs[c], names[c] for chromosome c + 1"""

    def __init__(self, locs, names, pad):
        self.locs, self.names, self.pad = [list(map(int, a)) for a in locs], [list(n) for n in names], int(pad)

    def scaffold_index(self, chrom, loc):
        """Data.scaffoldIndex (current/dna/Data.java:1091-1108)"""
        array = self.locs[chrom - 1]
        if len(array) < 2:                                  # :1093
            return 0
        loc = loc + self.pad // 2                           # :1096
        i = bisect.bisect_left(array, loc)                  # Arrays.binarySearch
        if i < len(array) and array[i] == loc:
            return i                                        # :1099
        return max(0, i - 1)                                # :1102-1104, insertPoint = i

    def scaffold_name(self, chrom, start, stop):
        """Read.getScaffoldName(false) / SiteScore.getScaffoldName(false) (Read.java:3304-3316, SiteScore.java:367-377)"""
        return self.names[chrom - 1][self.scaffold_index(chrom, jdiv2(start + stop))]


def key_of(name, prefixes):
    """:882-887 / :904-910"""
    if prefixes:
        idx = name.find("$")
        return name[idx + 1:] if idx >= 0 else name
    return name


def to_list_names(name, out):
    """toListNames (:1033-1048)"""
    x = name.find("$")
    if x >= 0:
        s = name[:x]
        if s.find(",") < 0:
            out.add(s)
        else:
            parts = s.split(",")
            while parts and parts[-1] == "":
                parts.pop()
            out.update(parts)
    return out


class Splitter:
    def __init__(self, ref, key_names, set_names, prefixes=True, mode=UNSET, clearzone=200, max_sites=5, scaf_stats=True, set_stats=True):
        assert mode != RANDOM                               # :694-695 throws
        self.ref, self.prefixes, self.mode, self.clearzone, self.max_sites = ref, prefixes, mode, clearzone, max_sites
        self.scaf = {k: [0, 0, 0, 0] for k in key_names} if scaf_stats else None      # mappedReads, mappedBases, ambiguousReads, ambiguousBases
        self.sets = {s: [0, 0, 0, 0] for s in set_names} if set_stats else None
        self.total_reads = 0
        self.tally = Counter()

    def sites(self, r):
        return r["sites"][:self.max_sites]                  # capSiteList

    def name_of_site(self, ss):
        return self.ref.scaffold_name(ss[0], ss[1], ss[2])

    def get_scaffolds(self, r):
        """getScaffolds(r, clearzone, set, includeMate=false) (:867-933)"""
        if not r["mapped"]:                                 # :869
            return None
        if not r["ambiguous"]:                              # :872-893
            return {key_of(self.ref.scaffold_name(r["chrom"], r["start"], r["stop"]), self.prefixes)}
        out = set()
        sites = self.sites(r)
        for ss in sites:                                    # :897-913
            if ss[3] + self.clearzone < sites[0][3]:
                break
            out.add(key_of(self.name_of_site(ss), self.prefixes))
        return out

    def add_to_scaf_counts(self, r):
        """addToScafCounts (:782-820)"""
        if self.scaf is None:
            return None
        keys = self.get_scaffolds(r)
        if not keys:
            return keys
        for k in keys:
            c = self.scaf[k]
            if r["ambiguous"]:
                c[2] += 1; c[3] += r["length"]              # :792-794
            else:
                c[0] += 1; c[1] += r["length"]              # :795-797
        return keys

    def get_sets(self, r1, r2):
        """getSets (:824-864)"""
        if not r1["mapped"] and (r2 is None or not r2["mapped"]):
            return None
        out = [set(), set(), set(), set()]
        for r, (pi, oi) in ((r1, (0, 1)), (r2, (2, 3))):
            if r is None or not r["mapped"]:
                continue
            sites = self.sites(r)
            if not sites:                                   # (cannot occur in the reference: the cap is at least 1)
                continue
            to_list_names(self.name_of_site(sites[0]), out[pi])
            for i in range(1, len(sites)):
                if sites[i][3] + self.clearzone < sites[0][3]:      # :844 / :855
                    self.tally["clearzone_break"] += 1
                    break
                if sites[i][3] + self.clearzone == sites[0][3]:
                    self.tally["clearzone_edge_kept"] += 1
                to_list_names(self.name_of_site(sites[i]), out[oi])
            else:
                if len(r["sites"]) > len(sites) and r["sites"][len(sites)][3] + self.clearzone >= sites[0][3]:
                    self.tally["cap_hides_site"] += 1       # a site inside the clearzone that only the cap keeps out
        return out

    def print_reads(self, reads, paired):
        """printReadsAndProcessAmbiguous (:641-757) over one read list; returns (per-unit verdicts, splitTable, splitTableA) with
        the tables as {set name: [index of r1, ...]}.  A verdict is (primarySet or None, ambigSet or None, ambiguous, stats set)."""
        self.total_reads += len(reads)
        step = 2 if paired else 1
        verdicts, table, tableA = [], {}, {}
        for i in range(0, len(reads), step):
            r1, r2 = reads[i], (reads[i + 1] if paired else None)
            self.add_to_scaf_counts(r1)                     # :645
            if r2 is not None:
                self.add_to_scaf_counts(r2)                 # :646
            sets = self.get_sets(r1, r2)                    # :650
            if sets is None:
                verdicts.append((None, None, False, set()))
                continue
            p1, s1, p2, s2 = [(s if s else None) for s in sets]       # :653-654
            ambiguous = False
            if p1 is not None and p2 is not None and p1 != p2:      # :661
                ambiguous = True; self.tally["p1_ne_p2"] += 1
            elif p1 is not None and s1 is not None and not p1.issuperset(s1):     # :662
                ambiguous = True; self.tally["s1_not_in_p1"] += 1
            elif p2 is not None and s2 is not None and not p2.issuperset(s2):     # :663
                ambiguous = True; self.tally["s2_not_in_p2"] += 1
            if r2 is not None and r1["mapped"] != r2["mapped"]:
                self.tally["single_mapped_mate"] += 1
            primary, ambig = set(), set()                   # :669-671
            if self.mode in (FIRST, UNSET):                 # :672-677
                if r2 is None or r1["mapScore"] >= r2["mapScore"]:
                    if r2 is not None:
                        self.tally["mapscore_tie" if r1["mapScore"] == r2["mapScore"] else "mapscore_r1"] += 1
                    primary |= p1 or set()
                else:
                    self.tally["mapscore_r2"] += 1
                    primary |= p2 or set()
            else:                                           # :678-681
                primary |= (p1 or set()) | (p2 or set())
            if ambiguous:                                   # :684-699
                if self.mode == SPLIT:
                    primary |= (s1 or set()) | (s2 or set())
                    ambig, primary = primary, None
                elif self.mode == ALL:
                    primary |= (s1 or set()) | (s2 or set())
                    ambig = None
                elif self.mode == TOSS:
                    primary = None
            for s in (primary or ()):                       # :701-710
                table.setdefault(s, []).append(i)
            for s in (ambig or ()):                         # :712-721
                tableA.setdefault(s, []).append(i)
            stat = (p1 or set()) | (p2 or set())            # :725-732
            if ambiguous:
                stat |= (s1 or set()) | (s2 or set())
            if self.sets is not None:
                incrR = 1 + (0 if r2 is None else 1)        # :734
                incrB = r1["length"] + (0 if r2 is None else r2["length"])      # :735
                for s in stat:
                    c = self.sets[s]
                    if ambiguous:
                        c[2] += incrR; c[3] += incrB        # :741-744
                    else:
                        c[0] += incrR; c[1] += incrB        # :747-750
            if len(stat) > 1 and not ambiguous:
                self.tally["shared_unambiguous"] += 1
            self.tally["ambiguous" if ambiguous else "unambiguous"] += 1
            verdicts.append((primary, ambig, ambiguous, stat))
        return verdicts, table, tableA


def print_counts(table, total_reads, header=True, nzo=True, sort=True):
    """printCounts (:1157-1189) over {name: [mappedReads, mappedBases, ambiguousReads, ambiguousBases]} in map order.  The float
    columns are given as exact Fractions' HALF_UP decimal of the double product, as String.format prints it."""
    from decimal import ROUND_HALF_UP, Decimal
    rows = [(n, c) for n, c in table.items()]
    if sort:                                                # Collections.sort, then reverse (:1164-1167); compareTo :1139-1143
        import functools

        def cmp(a, b):
            if a[1][0] != b[1][0]:
                return 1 if a[1][0] > b[1][0] else -1
            if a[1][2] != b[1][2]:
                return 1 if a[1][2] > b[1][2] else -1
            return (a[0] > b[0]) - (a[0] < b[0])
        rows.sort(key=functools.cmp_to_key(cmp))
        rows.reverse()
    out = []
    if header:
        out.append("#name\t%unambiguousReads\tunambiguousMB\t%ambiguousReads\tambiguousMB\tunambiguousReads\tambiguousReads")
    divR, divB = 100.0 / total_reads, 1.0 / 1000000         # :1173-1174
    f5 = lambda x: str(Decimal(x).quantize(Decimal("0.00001"), rounding=ROUND_HALF_UP))      # noqa: E731
    for name, c in rows:
        if (not nzo) or c[0] > 0 or c[2] > 0:               # :1176
            out.append("%s\t%s\t%s\t%s\t%s\t%d\t%d" % (name, f5(c[0] * divR), f5(c[1] * divB), f5(c[2] * divR), f5(c[3] * divB), c[0], c[2]))
    return out
