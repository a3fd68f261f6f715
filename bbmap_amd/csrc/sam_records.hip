// SAM record fields on the device: the part of stream.SamLine's constructor (current/stream/SamLine.java:82-413) behind the coordinate
// block that scaffold_coords_kernel (mapper.hip) already computes -- FLAG, POS / PNEXT / TLEN, RNAME / RNEXT, MAPQ, CIGAR, NM, AM, MD.
//
// One wavefront per read, every control value wave-uniform, the match string (long format, one symbol per alignment column) consumed
// 64 symbols per step with ballots.  What a line needs of the mate (mapped, scaffold, pos, strand, score, length) it reads from the
// mate's own records: the single-scaffold rule has been applied to both mates by the coordinate kernel, whose bbmap_scafrec array is
// this kernel's input.  Three launches and no atomics: sam_size_kernel (every fixed-size field and the string lengths), a device-wide
// exclusive scan of the per-read byte counts (host side, bbmap_get_sam_records in mapper_output.hip), sam_emit_kernel (the same walk again, writing).
//
// Configurable (bbmap_sam_config): INTRON_LIMIT (the `N` operator, the deletion runs NM and MD leave out, XS) and which optional tags
// are made; the further tags' values go to a second record per read, bbmap_samtags.  Fixed at the reference's defaults: SOFT_CLIP = true,
// PENALIZE_AMBIG = true; primary alignments only (Read.secondary, discarded and invalid are false).
// Three thresholds meet on one deletion run and are the reference's: `> limit` turns it into N and drops it from NM and MD, `< limit`
// makes it count against the identity, `>= max(limit, 1)` makes it a splice (Read.countErrors).
#include "sam_records.h"

#include <climits>
#include <cmath>

#include "insert_size.h"
#include "wave_prims.h"

namespace bbsam {
using wavep::u64;
using wavep::lt_mask;
using wavep::hibit;
using wavep::popc;

static_assert(sizeof(bbmap_samrec) == 64, "bbmap_samrec is 64 bytes");
static_assert(sizeof(bbmap_samtags) == 64, "bbmap_samtags is 64 bytes");
enum { KIND_NONE = 0, KIND_SHORTCUT = 1, KIND_WALK = 2 };       // how a read's CIGAR is made (sizing pass -> emit pass, parked in cigar_off)

__device__ inline int ndigits(int v) {
    return v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : v < 100000 ? 5 : v < 1000000 ? 6 : v < 10000000 ? 7 : v < 100000000 ? 8
           : v < 1000000000 ? 9 : 10;
}
// bounded writer: nothing is written at or behind `lim` (the bytes the sizing pass counted for this string)
struct Out { uint8_t *p; int lim; };
__device__ inline void put(const Out &o, int at, int ch) { if (at >= 0 && at < o.lim) o.p[at] = (uint8_t)ch; }
__device__ inline void put_uint(const Out &o, int at, int v, int nd) {
    for (int k = nd - 1; k >= 0; k--) { put(o, at + k, '0' + v % 10); v /= 10; }
}
// exclusive prefix sum over the wave; total = the wave's sum
__device__ inline int wave_excl_sum(int v, int lane, int &total) {
    int x = v;
    for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
    total = __shfl(x, 63, 64);
    return x - v;
}
// ChromosomeArray.get (current/dna/ChromosomeArray.java:232-234) with minIndex 0 and maxIndex = length - 1, as these arrays have them
__device__ inline int chrom_get(const uint8_t *chr, int chrLen, int loc) { return loc < 0 || loc >= chrLen - 1 ? 'N' : chr[loc]; }

// SamLine.countTrailingClip (:959-972)
__device__ inline int trailing_clip(const uint8_t *m, int ml, int lane) {
    int tclip = 0;
    for (int end = ml; end > 0; end -= 64) {
        const int i = end - 1 - lane;
        const u64 x = __ballot(i >= 0 && m[i] != 'C');
        if (x) { tclip += __builtin_ctzll(x); break; }
        tclip += min(64, end);
    }
    return tclip;
}

// SamLine.toMapq (:1709-1721).  Java evaluates every float operation on its own (no fused multiply-add), and Math.round(float) is
// floor(x + 1/2) computed exactly -- the double sum below is exact for these magnitudes.
#pragma clang fp contract(off)
__device__ inline int to_mapq(int score, int length, bool mapped, bool ambig, float maxv) {
    if (!mapped || length < 1) return 0;
    if (ambig) {                                            // PENALIZE_AMBIG
        const float mx = 3;
        const float adjusted = (score * mx) / (100.0f * length);
        return max(1, (int)floor((double)adjusted + 0.5));
    }
    const float score2 = (score - length * 40) * 1.6f;
    const float adjusted = (score2 * maxv) / (100.0f * length);
    return max(4, (int)floor((double)adjusted + 0.5));
}

// The deletion runs of a long-format string, 64 symbols per step: F = the lanes whose symbol is the first behind a run of `D`, and for
// those lanes the run's length (a run may have begun any number of steps earlier).  carry = the `D` symbols the string ends in so far.
__device__ inline int drun_step(int &carry, int ch, bool valid, int n, int lane, u64 &F) {
    const u64 Dm = __ballot(valid && ch == 'D'), nonD = __ballot(valid && ch != 'D');
    const bool prevD = lane ? (Dm >> (lane - 1)) & 1 : carry > 0;
    F = __ballot(valid && ch != 'D' && prevD);
    const u64 below = nonD & lt_mask(lane);
    const int len = below ? lane - 1 - hibit(below) : carry + lane;
    carry = nonD ? n - 1 - hibit(nonD) : carry + n;
    return len;
}

// introns: runs printed as N.  refLen / softLen: the counts of the M = X D N runs and of the S runs, i.e. calcCigarLength (:757-789)
// without and, added, with soft clips -- every counted symbol lies in exactly one printed run.
struct CigarInfo { int bytes, firstOp, firstCount, lastOp, lastCount, introns, refLen, softLen; };

// SamLine.toCigar14 (:679-750) / toCigar13 (:600-663).  Per symbol: refloc = readStart + the symbols before it that moved refloc, the
// soft-clip test `refloc<0 || refloc>=reflen` overriding its class (a `D` inside a clipped stretch is not counted: sfdflag).  Inside the
// clipped branch everything but `I` moves refloc, outside it `I`, `X` and `Y` do not: only where a 64-symbol step holds X / Y and
// touches the scaffold's ends does refloc depend on the clip decisions before it, and that step is walked symbol by symbol.
// A run is written when it ends, by the lane that heads the next one: the initial lastMode '=' with count 0, the `if(count>0)` that
// drops an empty run at a mode change, and the unconditional append of the last run (which can print 0S) are the reference's.
// A `D` run whose count -- the CIGAR's, without the clipped columns -- is above `limit` prints N (:725, :738): decided where the run
// is written, by the lane that heads the next run or behind the loop.  LENS: introns / refLen / softLen are wanted (the tags' sizing pass).
template <bool EMIT, bool LENS = false>
__device__ CigarInfo cigar_walk(const uint8_t *m, int ml, int readStart, int reflen, bool v13, int limit, Out out) {
    const int lane = threadIdx.x & 63;
    CigarInfo R;
    R.bytes = 0; R.firstOp = 0; R.firstCount = 0; R.introns = 0; R.refLen = 0; R.softLen = 0;
    int refloc = readStart, lastMode = '=', count = 0;
    bool first = true;
    for (int base = 0; base < ml; base += 64) {
        const int n = min(64, ml - base);
        const bool valid = lane < n;
        const int ch = valid ? m[base + lane] : 0;
        const bool isI = ch == 'I', isXY = ch == 'X' || ch == 'Y';
        const u64 xy = __ballot(valid && isXY);
        const bool allIn = refloc >= 0 && refloc + 64 < reflen;
        int myref, nextref;
        if (xy == 0 || allIn) {
            const u64 adv = __ballot(valid && !isI && !isXY);
            myref = refloc + popc(adv & lt_mask(lane));
            nextref = refloc + popc(adv);
        } else {
            int r = refloc;
            myref = r;
            for (int k = 0; k < n; k++) {
                const int c = __shfl(ch, k, 64);
                if (lane == k) myref = r;
                const bool cl = r < 0 || r >= reflen;
                r += cl ? (c != 'I') : !(c == 'I' || c == 'X' || c == 'Y');
            }
            nextref = r;
        }
        const bool clip = myref < 0 || myref >= reflen;     // SOFT_CLIP
        int mode;
        if (clip) mode = 'S';
        else if (ch == 'm' || ch == 's') mode = v13 ? 'M' : '=';
        else if (ch == 'S') mode = v13 ? 'M' : 'X';
        else if (isI || isXY) mode = 'I';
        else if (ch == 'D') mode = 'D';
        else if (ch == 'C') mode = 'S';
        else mode = 'M';                                    // N, B
        const bool counted = valid && !(clip && ch == 'D');
        int prevMode = __shfl_up(mode, 1, 64);
        if (lane == 0) prevMode = lastMode;
        const bool head = valid && mode != prevMode;
        const u64 heads = __ballot(head), nons = __ballot(counted);
        const u64 below = heads & lt_mask(lane);
        const int p = below ? hibit(below) : 0;
        const int pmode = __shfl(mode, p, 64);
        const int cnt = below ? popc(nons & lt_mask(lane) & ~lt_mask(p)) : count + popc(nons & lt_mask(lane));
        const int op = below ? pmode : lastMode;
        const bool emits = head && cnt > 0;
        const bool intron = op == 'D' && cnt > limit;
        const int nd = ndigits(cnt);
        int total;
        const int off = wave_excl_sum(emits ? nd + 1 : 0, lane, total);
        if (EMIT && emits) { put_uint(out, R.bytes + off, cnt, nd); put(out, R.bytes + off + nd, intron ? 'N' : op); }
        const u64 em = __ballot(emits);
        if (LENS) {
            R.introns += popc(__ballot(emits && intron));
            R.refLen += popc(__ballot(counted && mode != 'S' && mode != 'I'));
            R.softLen += popc(__ballot(counted && mode == 'S'));
        }
        if (first && em) {
            const int fl = __builtin_ctzll(em);
            R.firstOp = __shfl(op, fl, 64); R.firstCount = __shfl(cnt, fl, 64);
            first = false;
        }
        R.bytes += total;
        if (heads) {
            const int q = hibit(heads);
            count = popc(nons & ~lt_mask(q));
            lastMode = __shfl(mode, q, 64);
        } else count += popc(nons);
        refloc = nextref;
    }
    const int nd = ndigits(count);
    const bool intron = lastMode == 'D' && count > limit;
    if (EMIT && lane == 0) { put_uint(out, R.bytes, count, nd); put(out, R.bytes + nd, intron ? 'N' : lastMode); }
    R.introns += intron;
    R.bytes += nd + 1;
    R.lastOp = lastMode; R.lastCount = count;
    if (first) { R.firstOp = lastMode; R.firstCount = count; }
    return R;
}

// NM (makeOptionalTags :1514-1535): I S N X Y columns and deletions whose cpos lies in [from, to)
__device__ int nm_count(const uint8_t *m, int ml, int from, int to) {
    const int lane = threadIdx.x & 63;
    int nm = 0, cpos = 0;
    for (int base = 0; base < ml; base += 64) {
        const bool valid = base + lane < ml;
        const int ch = valid ? m[base + lane] : 0;
        const u64 nonD = __ballot(valid && ch != 'D');
        const int my = cpos + popc(nonD & lt_mask(lane));
        const bool hit = valid && my >= from && my < to && (ch == 'I' || ch == 'S' || ch == 'N' || ch == 'X' || ch == 'Y' || ch == 'D');
        nm += popc(__ballot(hit));
        cpos += popc(nonD);
    }
    return nm;
}
// The same under an intron limit: delsCurrent is added only when `<= limit` (:1529, :1535).  `D` does not move cpos, so a run and the
// symbol behind it share one cpos: a run in range is flushed by that symbol, or behind the loop when the string ends in it.
__device__ int nm_count_limit(const uint8_t *m, int ml, int from, int to, int limit) {
    const int lane = threadIdx.x & 63;
    int nm = 0, cpos = 0, carry = 0;
    for (int base = 0; base < ml; base += 64) {
        const int n = min(64, ml - base);
        const bool valid = lane < n;
        const int ch = valid ? m[base + lane] : 0;
        const u64 nonD = __ballot(valid && ch != 'D');
        const int my = cpos + popc(nonD & lt_mask(lane));
        const bool in = valid && my >= from && my < to;
        nm += popc(__ballot(in && (ch == 'I' || ch == 'S' || ch == 'N' || ch == 'X' || ch == 'Y')));
        u64 F;
        const int run = drun_step(carry, ch, valid, n, lane, F);
        const bool add = ((F >> lane) & 1) && in && run <= limit;
        if (__ballot(add)) { int total; wave_excl_sum(add ? run : 0, lane, total); nm += total; }
        cpos += popc(nonD);
    }
    if (carry > 0 && cpos >= from && cpos < to && carry <= limit) nm += carry;
    return nm;
}

// Read.identityFlat's counts (current/stream/Read.java:1529-1596) over a long-format string -- a run of `D` is bad only when shorter
// than the limit (:1557, :1578) -- before the `n` folding of :1586-1588, and Read.countErrors(limit)[5] (:2189-2240): the runs of `D`
// that reach max(limit, 1) symbols, each counted once.
struct TagCounts { int good, bad, ns, splices; };
__device__ TagCounts tag_walk(const uint8_t *m, int ml, int limit) {
    const int lane = threadIdx.x & 63;
    const int minSplice = max(limit, 1);
    TagCounts T = {0, 0, 0, 0};
    int carry = 0;
    for (int base = 0; base < ml; base += 64) {
        const int n = min(64, ml - base);
        const bool valid = lane < n;
        const int ch = valid ? m[base + lane] : 0;
        const bool isM = ch == 'm', isN = ch == 'N' || ch == 'R';
        T.good += popc(__ballot(isM));
        T.ns += popc(__ballot(isN));
        T.bad += popc(__ballot(valid && !isM && !isN && ch != 'C' && ch != 'D'));
        u64 F;
        const int run = drun_step(carry, ch, valid, n, lane, F);
        const bool ends = (F >> lane) & 1;
        T.splices += popc(__ballot(ends && run >= minSplice));
        const bool add = ends && run < limit;
        if (__ballot(add)) { int total; wave_excl_sum(add ? run : 0, lane, total); T.bad += total; }
    }
    if (carry > 0) { T.splices += carry >= minSplice; if (carry < limit) T.bad += carry; }
    return T;
}

// Read.containsNonM (current/stream/Read.java:1815-1823) / containsNonNMS (:1855-1863)
__device__ bool contains_other(const uint8_t *m, int ml, bool nms) {
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < ml; base += 64) {
        const bool valid = base + lane < ml;
        const int b = valid ? m[base + lane] : 0;
        const bool other = valid && b > '9' && b != 'm' && !(nms && (b == 's' || b == 'N' || b == 'S'));
        if (__ballot(other)) return true;
    }
    return false;
}

// SamLine.makeMdTag (:1361-1445), the value behind "MD:Z:".  rpos starts at the record's chromosome start; a column is skipped when
// `m=='C' || rpos<scafloc || rpos>=scafstop`, and a skipped column always moves rpos -- also an I / X / Y one, which does not move it
// otherwise: as in cigar_walk, a step that holds such a column and touches the scaffold's ends is walked symbol by symbol.
// `call` is Read.bases as SamLine sees it: the read as it came in, NOT the aligned strand.  The mapping threads never touch r.bases
// (AbstractMapThread.java:489-503 makes basesM a separate array; BBMapThread.processRead :389-704 only reads basesP / basesM), and
// ReadStreamByteWriter.java:489 passes the read on as it is (toBytes reverse-complements SEQ itself, :1940-1942).  So for a minus-strand
// read an `N` column compares the reference base with call[cpos] of the unreversed read; restated as it is.
// Output tokens in order: at column i first the deletion flush (`prevM=='D' && m!='D'`: count, '^', the dels bases in front of rpos),
// then the substitution (count unless `count==0 && prevSub`; prevSub is never cleared), and the final count.
// A flush with `dels > limit` prints nothing and resets neither count nor dels (:1380): dels only grows from there, so every later
// flush is dropped as well (`dead`), and up to the first dropped one every flush has reset dels, which is what delsF assumes.
template <bool EMIT>
__device__ int md_walk(const uint8_t *m, int ml, const uint8_t *chr, int chrLen, int refstart, const uint8_t *call, int callLen,
                       int scafloc, int scaflen, int limit, Out out) {
    const int lane = threadIdx.x & 63;
    const int scafstop = scafloc + scaflen;
    int rpos = refstart, cpos = 0, count = 0, dels = 0, prevM = '?', bytes = 0;
    bool prevSub = false, dead = false;
    for (int base = 0; base < ml; base += 64) {
        const int n = min(64, ml - base);
        const bool valid = lane < n;
        const int ch = valid ? m[base + lane] : 0;
        const bool ixy = ch == 'I' || ch == 'X' || ch == 'Y';
        const u64 anyIxy = __ballot(valid && ixy);
        const bool allIn = rpos >= scafloc && rpos + 64 < scafstop;
        int myr, nextr;
        if (anyIxy == 0 || allIn) {
            const u64 adv = __ballot(valid && !ixy);
            myr = rpos + popc(adv & lt_mask(lane));
            nextr = rpos + popc(adv);
        } else {
            int r = rpos;
            myr = r;
            for (int k = 0; k < n; k++) {
                const int c = __shfl(ch, k, 64);
                if (lane == k) myr = r;
                const bool skip = c == 'C' || r < scafloc || r >= scafstop;
                r += skip ? 1 : !(c == 'I' || c == 'X' || c == 'Y');
            }
            nextr = r;
        }
        const bool live = valid && !(ch == 'C' || myr < scafloc || myr >= scafstop);
        const u64 nonD = __ballot(valid && ch != 'D');
        const int mycpos = cpos + popc(nonD & lt_mask(lane));
        const bool isS = live && ch == 'S', isN = live && ch == 'N';
        int refb = 0;
        if (isS || isN) refb = chrom_get(chr, chrLen, myr);
        bool same = false;
        if (isN) same = (mycpos < callLen ? call[mycpos] : 0) == refb;
        const bool matchEv = live && (ch == 'm' || ch == 's' || (isN && same));
        const bool subEv = isS || (isN && !same);
        int prevCh = __shfl_up(ch, 1, 64);
        if (lane == 0) prevCh = prevM;
        const bool flushAny = valid && prevCh == 'D' && ch != 'D';
        const u64 M = __ballot(matchEv), S = __ballot(subEv), FA = __ballot(flushAny), D = __ballot(live && ch == 'D');
        const u64 belowF = FA & lt_mask(lane);
        const int delsF = belowF ? popc(D & lt_mask(lane) & ~lt_mask(hibit(belowF))) : dels + popc(D & lt_mask(lane));
        const u64 over = limit == INT_MAX ? 0 : __ballot(flushAny && delsF > limit);
        const bool flushEv = flushAny && !dead && !(over & ((lt_mask(lane) << 1) | 1));
        const u64 F = __ballot(flushEv);
        const u64 belowR = (S | F) & lt_mask(lane);
        const int cntBefore = belowR ? popc(M & lt_mask(lane) & ~lt_mask(hibit(belowR))) : count + popc(M & lt_mask(lane));
        const int ndF = ndigits(cntBefore);
        const int flushLen = flushEv ? ndF + 1 + delsF : 0;
        const int cntS = flushEv ? 0 : cntBefore;
        const bool subCount = subEv && (cntS > 0 || !(prevSub || (S & lt_mask(lane))));
        const int ndS = ndigits(cntS);
        const int subLen = subEv ? (subCount ? ndS : 0) + 1 : 0;
        int total;
        const int off = bytes + wave_excl_sum(flushLen + subLen, lane, total);
        if (EMIT) {
            if (flushEv) { put_uint(out, off, cntBefore, ndF); put(out, off + ndF, '^'); }
            if (subEv) {
                int at = off + flushLen;
                if (subCount) { put_uint(out, at, cntS, ndS); at += ndS; }
                put(out, at, refb);
            }
            for (u64 f = F; f; f &= f - 1) {                // the deleted bases, 64 per step by the whole wave
                const int l = __builtin_ctzll(f);
                const int o = __shfl(off + ndF + 1, l, 64), e = __shfl(myr, l, 64), d = __shfl(delsF, l, 64);
                for (int j = lane; j < d; j += 64) put(out, o + j, chrom_get(chr, chrLen, e - d + j));
            }
        }
        bytes += total;
        if (S | F) count = popc(M & ~lt_mask(hibit(S | F))); else count += popc(M);
        if (F) dels = popc(D & ~lt_mask(hibit(F))); else dels += popc(D);
        prevSub = prevSub || S != 0;
        dead = dead || over != 0;
        prevM = __shfl(ch, n - 1, 64);
        cpos += popc(nonD);
        rpos = nextr;
    }
    const int nd = ndigits(count);
    if (EMIT && lane == 0) put_uint(out, bytes, count, nd);
    return bytes + nd;
}

struct Line {                       // what both passes need of one read, wave-uniform
    const bbmap_final *f; const uint8_t *m; int ml;
    bbmap_scafrec s;
    int len; const uint8_t *call;
    bool mapped;
};
__device__ inline Line line_of(const Args &A, long long r) {
    Line L;
    const ReadRec R = record_of<TierRule::ByRecord>(A.V, r);
    L.f = R.f; L.m = R.m;
    L.s = A.scaf[r];
    L.mapped = (L.s.flags & BBMAP_SCAF_MAPPED) != 0;
    L.ml = L.mapped && L.f->match_len > 0 ? L.f->match_len : 0;        // a record the scaffold rule unmapped has lost its string (:138)
    if (!L.ml) L.m = nullptr;
    L.len = A.V.reads[r].len; L.call = A.V.bases + A.V.reads[r].bases_off;
    return L;
}

// XM (makeOptionalTags :1565-1581): 1 + the list's further sites with the top site's score, at least 2 for an ambiguous read
__device__ int xm_count(const Args &A, long long r, bool ambiguous) {
    const int lane = threadIdx.x & 63;
    const ReadRec R = record_of<TierRule::ByRecord, true>(A.V, r);
    int x = 1;
    if (R.n > 0) {
        const int z = R.s[0].score;
        for (int base = 1; base < R.n; base += 64) x += popc(__ballot(base + lane < R.n && R.s[base + lane].score == z));
    }
    return ambiguous ? max(x, 2) : x;
}

// TAGS: the bbmap_samtags records are wanted (an instantiation of its own: the plain one keeps the registers and the occupancy it had
// before there were tags)
template <bool TAGS>
__global__ __launch_bounds__(256) void sam_size_kernel(const Args A, bbmap_samrec *recs, bbmap_samtags *tagrecs, int *counts) {
    const long long r = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= A.V.n) return;
    const int lane = threadIdx.x & 63;
    const Line L = line_of(A, r);
    const bbmap_final &f = *L.f;
    const bool mapped = L.mapped, hasMatch = L.ml > 0;
    const bool perfect = f.perfect != 0;                    // `final boolean perfect=r1.perfect()` (:89)
    const bool sameScaf = (L.s.flags & BBMAP_SCAF_SAME_SCAFFOLD) != 0;
    const bool inbounds = (L.s.flags & BBMAP_SCAF_INBOUNDS) != 0;
    const int pos0 = mapped ? L.s.pos : 0;
    int pos1 = mapped ? L.s.end : 0;
    const int name1 = mapped ? L.s.scaffold : -1;
    bbmap_samrec w;
    int flag = 0;                                           // makeFlag (:2134-2151)
    bool mateMapped = false, mateInbounds = false;
    int mateScore = 0, mateLen = 1;
    bbinsert::Mate mate = {0, 0, 0, 0, 0};
    if (A.V.paired) {
        const long long q = r ^ 1;
        const ReadRec Q = record_of<TierRule::ByRecord>(A.V, q);
        const bbmap_final *f2 = Q.f;
        const uint8_t *m2 = Q.m;
        const bbmap_scafrec s2 = A.scaf[q];
        mateMapped = (s2.flags & BBMAP_SCAF_MAPPED) != 0;
        const bool mateMatch = mateMapped && f2->match_len > 0;
        mateScore = f2->mapScore; mateLen = A.V.reads[q].len;
        mateInbounds = (s2.flags & BBMAP_SCAF_INBOUNDS) != 0;
        mate = {f2->strand, f2->start, f2->stop, f2->chrom, mateLen};
        const int name2 = mateMapped ? s2.scaffold : -1;
        const int pos0m = mateMapped ? s2.pos : 0;
        // pos1_mate is NOT limited to the scaffold: `if(pos1_mate>scaflen){pos1=scaflen;}` (:207) limits pos1, by this line's scaflen
        const int pos1m = mateMapped ? s2.stop + 1 - (mateMatch ? trailing_clip(m2, f2->match_len, lane) : 0) : 0;
        if (mateMapped && pos1m > (mapped ? L.s.scaflen : 0)) pos1 = mapped ? L.s.scaflen : 0;
        flag |= 0x1;
        if (mapped && hasMatch && sameScaf && (L.s.flags & BBMAP_SCAF_PAIRED) && mateMapped && mateMatch) flag |= 0x2;
        flag |= (r & 1) ? 0x80 : 0x40;
        if (!mateMapped) flag |= 0x8;
        if (f2->strand == 1) flag |= 0x20;
        int tlen = 0;
        if (mapped && mateMapped) {                         // the POS / PNEXT / TLEN table (:220-253)
            w.pos = pos0; w.pnext = pos0m;
            if (sameScaf) tlen = 1 + (max(pos1, pos1m) - min(pos0, pos0m));
        } else if (mapped) { w.pos = pos0; w.pnext = pos0; }
        else if (mateMapped) { w.pos = pos0m; w.pnext = pos0m; }
        else { w.pos = 0; w.pnext = 0; }
        // sign (:349-354): r.start / r2.start are the records' chromosome coordinates, pairnum the mate number
        if (!(f.start < f2->start || (f.start == f2->start && (r & 1) == 0))) tlen = -tlen;
        w.tlen = tlen;
        w.rname = mapped ? name1 : name2;                   // :164
        w.rnext = !mapped && !mateMapped ? -1 : mapped && mateMapped ? (sameScaf ? -2 : name2) : -2;      // :315
    } else {
        w.pos = pos0; w.pnext = 0; w.tlen = 0;
        w.rname = name1; w.rnext = -1;
    }
    if (!mapped) flag |= 0x4;
    if (f.strand == 1) flag |= 0x10;
    w.flag = flag;
    const int len = L.len;
    const float maxv = A.mapqMax[min(max(len, 0), A.mapqMaxLen)];
    w.mapq = to_mapq(f.mapScore, len, mapped, f.ambiguous != 0, maxv);
    // CIGAR (:269-301)
    const bool v13 = (A.flags & BBMAP_SAM_CIGAR13) != 0;
    const int limit = A.intronLimit;
    int kind = KIND_NONE, cigarLen = 0, leftclip = 0, rightclip = 0, introns = 0, refLen = len, softLen = 0;
    if (mapped && hasMatch) {
        const bool shortcut = inbounds && (v13 ? (perfect || !contains_other(L.m, L.ml, true)) : (perfect && !contains_other(L.m, L.ml, false)));
        if (shortcut) { kind = KIND_SHORTCUT; cigarLen = ndigits(len) + 1; }
        else if (L.s.start != L.s.stop) {                   // toCigar: `readStart==readStop` gives null
            kind = KIND_WALK;
            const CigarInfo ci = cigar_walk<false, TAGS>(L.m, L.ml, L.s.start, L.s.scaflen, v13, limit, Out{nullptr, 0});
            cigarLen = ci.bytes; introns = ci.introns; refLen = ci.refLen; softLen = ci.softLen;
            leftclip = ci.firstOp == 'S' ? ci.firstCount : 0;               // calcLeftClip (:1447-1460)
            rightclip = ci.lastOp == 'S' ? ci.lastCount : 0;                // calcRightClip (:1462-1479)
        }
    }
    // tags (makeOptionalTags :1481-1549): only for a mapped read, none at all under NO_TAGS (:1482)
    w.nm = -1; w.am = -1; w.tags = 0;
    int mdLen = 0;
    const int make = A.tags;
    const bool tagged = mapped && !(make & BBMAP_SAM_NO_TAGS);
    if (tagged) {
        if (f.ambiguous) w.tags |= BBMAP_SAM_TAG_XT;
        if (make & BBMAP_SAM_MAKE_NM) {
            if (perfect) w.nm = 0;
            else if (hasMatch)
                w.nm = limit == INT_MAX ? nm_count(L.m, L.ml, leftclip, len - rightclip) : nm_count_limit(L.m, L.ml, leftclip, len - rightclip, limit);
        }
        const int other = !A.V.paired ? w.mapq : (mateMapped ? max(1, mateScore / max(mateLen, 1)) : 0);
        if (make & BBMAP_SAM_MAKE_AM) w.am = min(w.mapq, other);
        if ((A.flags & BBMAP_SAM_MD) && hasMatch)
            mdLen = md_walk<false>(L.m, L.ml, A.chromArr[f.chrom], A.chromArrLen[f.chrom], f.start, L.call, len, f.start - L.s.start,
                                   L.s.scaflen, limit, Out{nullptr, 0});
    }
    w.cigar_off = kind; w.cigar_len = cigarLen; w.md_len = mdLen; w.md_off = 0;      // (the emit pass replaces kind by the offset)
    if (lane == 0) { recs[r] = w; counts[r] = cigarLen + mdLen; }
    if (!TAGS) return;
    // the further tags (:1548, :1565-1619, :1673-1681), as values; the host prints them
    bbmap_samtags t = {};
    t.introns = introns;
    TagCounts tc = {0, 0, 0, 0};
    if (hasMatch && ((tagged && (make & BBMAP_SAM_MAKE_IDENTITY) && !perfect) || limit != INT_MAX)) tc = tag_walk(L.m, L.ml, limit);
    t.splices = tc.splices;
    if (tagged) {
        const bool noCigar = kind == KIND_NONE;
        int present = 0;
        if (make & BBMAP_SAM_MAKE_SM) { present |= BBMAP_SAM_MAKE_SM; t.sm = w.mapq; }
        if (make & BBMAP_SAM_MAKE_XM) { present |= BBMAP_SAM_MAKE_XM; t.xm = xm_count(A, r, f.ambiguous != 0); }
        if ((make & BBMAP_SAM_MAKE_XS) && introns > 0) {            // makeXSTag (:1346-1359)
            bool plus = f.strand == 0;
            if (A.V.paired && (r & 1)) plus = !plus;
            if (make & BBMAP_SAM_XS_SECONDSTRAND) plus = !plus;
            present |= BBMAP_SAM_MAKE_XS; t.xs = plus ? 1 : -1;
        }
        if (make & BBMAP_SAM_MAKE_NH) { present |= BBMAP_SAM_MAKE_NH; t.nh = 1; }       // (no secondary output: :1603)
        if (perfect || hasMatch) {
            if (make & BBMAP_SAM_MAKE_STOP) {                       // makeStopTag (:1316-1319)
                present |= BBMAP_SAM_MAKE_STOP; t.ys = w.pos + (noCigar || perfect ? len : refLen + softLen) - 1;
            }
            if (make & BBMAP_SAM_MAKE_LENGTH) {                     // makeLengthTag (:1321-1324); countLeadingClip = the first run, if S
                present |= BBMAP_SAM_MAKE_LENGTH;
                t.yl_query = noCigar || perfect ? len : len - leftclip; t.yl_ref = noCigar || perfect ? len : refLen;
            }
            if (make & BBMAP_SAM_MAKE_IDENTITY) {                   // makeIdentityTag (:1326-1330)
                present |= BBMAP_SAM_MAKE_IDENTITY;
                const int n = (tc.ns + 3) / 4;
                t.yi_perfect = perfect; t.yi_good = perfect ? 0 : tc.good + n; t.yi_bad = perfect ? 0 : tc.bad + 3 * n;
            }
        }
        if (make & BBMAP_SAM_MAKE_SCORE) { present |= BBMAP_SAM_MAKE_SCORE; t.yr = f.mapScore; }
        if ((make & BBMAP_SAM_MAKE_INSERT) && A.V.paired) {         // :1615-1619, Read.insertSizeMapped(false) (Read.java:2618-2626)
            const bbinsert::Mate me = {f.strand, f.start, f.stop, f.chrom, len};
            present |= BBMAP_SAM_MAKE_INSERT;
            t.x8 = !mateMapped || me.strand == mate.strand ? bbinsert::insert_unstranded(me, mate) : bbinsert::insert_plus_left(me, mate);
        }
        if (make & BBMAP_SAM_MAKE_BOUNDS) {                         // :1673-1681
            present |= BBMAP_SAM_MAKE_BOUNDS;
            t.xb = (inbounds ? 'I' : 'O') | (A.V.paired ? (mateMapped ? (mateInbounds ? 'I' : 'O') : 'U') << 8 : 0);
        }
        t.present = present;
    }
    if (lane == 0) tagrecs[r] = t;
}

__global__ __launch_bounds__(256) void sam_emit_kernel(const Args A, bbmap_samrec *recs, const long long *offsets, uint8_t *text) {
    const long long r = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= A.V.n) return;
    const int lane = threadIdx.x & 63;
    const int kind = (int)recs[r].cigar_off, cigarLen = recs[r].cigar_len, mdLen = recs[r].md_len;
    const long long off = offsets[r];
    const long long room = A.textCap - off;                 // nothing is written at or behind the blob's capacity
    const int cigarLim = (int)max(0ll, min((long long)cigarLen, room)), mdLim = (int)max(0ll, min((long long)mdLen, room - cigarLen));
    if (kind != KIND_NONE || mdLen > 0) {
        const Line L = line_of(A, r);
        const Out oc{text + off, cigarLim};
        if (kind == KIND_SHORTCUT) {
            const int nd = ndigits(L.len);
            if (lane == 0) { put_uint(oc, 0, L.len, nd); put(oc, nd, (A.flags & BBMAP_SAM_CIGAR13) ? 'M' : '='); }
        } else if (kind == KIND_WALK)
            cigar_walk<true>(L.m, L.ml, L.s.start, L.s.scaflen, (A.flags & BBMAP_SAM_CIGAR13) != 0, A.intronLimit, oc);
        if (mdLen > 0)
            md_walk<true>(L.m, L.ml, A.chromArr[L.f->chrom], A.chromArrLen[L.f->chrom], L.f->start, L.call, L.len, L.f->start - L.s.start,
                          L.s.scaflen, A.intronLimit, Out{text + off + cigarLen, mdLim});
    }
    if (lane == 0) { recs[r].cigar_off = off; recs[r].md_off = off + cigarLen; }
}

void fill_mapq_max(float *table, int maxLen) {
    const double invlog2 = 1 / std::log(2.0);               // Tools.java:2316-2317
    table[0] = 36;
    for (int len = 1; len <= maxLen; len++) {
        const float l2 = (float)(std::log((double)len) * invlog2);
        const float a = 1.5f * l2;                          // two roundings, as Java's float arithmetic
        table[len] = a + 36;
    }
}

hipError_t launch_size(const Args &a, bbmap_samrec *recs, bbmap_samtags *tags, int *counts, hipStream_t stream) {
    if (a.V.n > 0) hipLaunchKernelGGL(tags ? sam_size_kernel<true> : sam_size_kernel<false>, dim3((unsigned)((a.V.n + 3) / 4)), dim3(256), 0, stream, a,
                                      recs, tags, counts);
    return hipGetLastError();
}
hipError_t launch_emit(const Args &a, bbmap_samrec *recs, const long long *offsets, uint8_t *text, hipStream_t stream) {
    if (a.V.n > 0) hipLaunchKernelGGL(sam_emit_kernel, dim3((unsigned)((a.V.n + 3) / 4)), dim3(256), 0, stream, a, recs, offsets, text);
    return hipGetLastError();
}

}  // namespace bbsam
