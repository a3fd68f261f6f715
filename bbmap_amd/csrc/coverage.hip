// Coverage on the device: jgi.CoveragePileup as BBMap's mapping threads feed it (AbstractMapThread.java:552-558).
//   processRead (current/jgi/CoveragePileup.java:784-813) -> ScaffoldCoordinates.setFromIndex (current/stream/ScaffoldCoordinates.java:
//   37-56) -> addCoverage (:600-663) / addCoverageIgnoringDeletions (:665-722) -> CoverageArray2/3.incrementRange
//   (current/dna/CoverageArray2.java:145-164, CoverageArray3.java:155-174), and the integers behind writeStats (:991-1106), writeHist
//   (:1113-1132), writeCoveragePerBase (:1143-1177), writeCoveragePerBaseBinned2 (:1276-1315), standardDeviation (:1405-1438),
//   standardDeviationBinned (:1349-1402) and loadScaffoldsFromIndex -> ChromosomeArray.calcGC (:420-449,
//   current/dna/ChromosomeArray.java:204-209).
//
// Accumulate is O(reads): per strand one int32 DIFFERENCE array over the concatenated scaffolds, scaffold s owning length[s] + 1 slots
// at covoff[s].  A covered run [a, b] is +1 at a and -1 at b + 1; b <= length - 1, so the -1 lands in the scaffold's own last slot at
// the latest, every scaffold's slots sum to zero, and ONE plain prefix sum over the whole array yields every scaffold's depths with
// no segment flags.  Every increment of the reference is +1 with a cap per increment (65,535 or Integer.MAX_VALUE); counts only grow,
// so min(count, cap) at read-out is the same number, and the saturation happens where the prefix sum writes the depths.  One read
// per wavefront on a persistent grid (as run_stats.hip), every control value wave-uniform; all sums are integer atomics, so the
// result does not depend on the order of the adds.
//
// Finalize is a snapshot of the difference arrays: reduce-then-scan (tile sums, the scan of the sums on two levels, apply) -- no
// look-back scan, nothing here waits on another workgroup -- then one pass over the depths for the per-scaffold integers, the
// histogram and the bin sums, and a radix select per scaffold for Median_fold.
#include "coverage.h"

#include <climits>

#include "host_common.h"
#include "wave_prims.h"

namespace bbcov {
using wavep::u64;
using wavep::gt_mask;
using wavep::hibit;
using wavep::lt_mask;
using wavep::popc;
using wavep::uni;

// ------------------------------------------------------------------------------------------------------------------ accumulate

// addCoverageIgnoringDeletions' loop (:682-695) over the long-format string, 64 symbols per step: `for(rpos=start, mpos=0;
// mpos<match.length && rpos<=stop; mpos++)`, m / S / N cover rpos and advance it, D advances it, I / X / Y / C do nothing.
// Symbols that cover consecutive positions form a run; a run is broken by a D, by rpos > stop or by the string's end.  A run adds +1
// at its first position and -1 behind its last one, whichever steps it crosses: the step's last advancing symbol leaves the run
// open (`open`, `openEnd` = the slot behind it), and the next step's first advancing symbol either continues it or closes it.
// diff points at the scaffold's slot 0.  Returns basehits.
__device__ inline int walk_excluding_deletions(const uint8_t *m, int ml, int a, int b, int *diff, int lane) {
    int hits = 0, rbase = a, openEnd = 0;
    bool open = false;
    for (int base = 0; base < ml && rbase <= b; base += 64) {
        const int ch = base + lane < ml ? m[base + lane] : 0;
        const bool covers = ch == 'm' || ch == 'S' || ch == 'N';
        const u64 adv = __ballot(covers || ch == 'D');
        if (!adv) continue;
        const int rpos = rbase + popc(adv & lt_mask(lane));
        const u64 cov = __ballot(covers && rpos <= b);
        if (open && !((cov >> __builtin_ctzll(adv)) & 1) && lane == 0) atomicAdd(diff + openEnd, -1);
        const u64 below = adv & lt_mask(lane), above = adv & gt_mask(lane);
        const bool mine = (cov >> lane) & 1;
        const bool prevCov = below ? (cov >> hibit(below)) & 1 : open;
        if (mine && !prevCov) atomicAdd(diff + rpos, 1);
        if (mine && above && !((cov >> __builtin_ctzll(above)) & 1)) atomicAdd(diff + rpos + 1, -1);
        const int last = hibit(adv);
        open = (cov >> last) & 1;
        openEnd = rbase + popc(adv & lt_mask(last)) + 1;
        hits += popc(cov);
        rbase += popc(adv);
    }
    if (open && lane == 0) atomicAdd(diff + openEnd, -1);
    return hits;
}

__global__ __launch_bounds__(TB) void coverage_add_kernel(const AddArgs A) {
    __shared__ u64 acc[LDS_SCAF * N_ACC];
    const int lane = threadIdx.x & 63, wid = uni((int)(threadIdx.x >> 6));
    // Few scaffolds (a chromosome-level assembly) mean every read of the batch adds to the same handful of records: the block sums
    // them in LDS and adds each counter that moved once, at its end.  Many scaffolds spread the adds by themselves.
    const bool useLds = A.nscaf <= LDS_SCAF;
    if (useLds) for (int k = threadIdx.x; k < A.nscaf * N_ACC; k += TB) acc[k] = 0;
    __syncthreads();
    long long nProcessed = 0, nMapped = 0, nBases = 0;         // wave-uniform; added to the totals once per wavefront
    const long long nwaves = (long long)gridDim.x * WAVES_PER_BLOCK;
    for (long long r = (long long)blockIdx.x * WAVES_PER_BLOCK + wid; r < A.V.n; r += nwaves) {
        nProcessed++;                                           // processRead :785
        const ReadRec R = record_of<TierRule::ByList>(A.V, r);
        const bbmap_final &f = *R.f;
        if (!f.mapped) continue;
        const int chrom = uni(f.chrom), start = uni(f.start), stop = uni(f.stop), strand = uni(f.strand);
        if (chrom < 1 || chrom > A.T.nchroms) continue;
        if (!bbscaf::is_single_scaffold(A.T, chrom, start, stop)) continue;             // setFromIndex :43
        const int sb = A.T.off[chrom], ns = A.T.off[chrom + 1] - sb;
        const int mid = (int)((unsigned)start + (unsigned)stop) / 2;                   // Java's int sum, truncating division (:45)
        const int key = (int)((unsigned)mid + (unsigned)(A.T.pad / 2));                // Data.scaffoldIndex
        const int gs = sb + (ns < 2 ? 0 : bbscaf::wave_last_at_or_below(A.T.loc + sb, ns, key));
        const int L = A.T.len[gs];
        const int start0 = start - A.T.loc[gs], stop0 = start0 - start + stop;          // scaffoldRelativeLoc, :48-49
        const int a = max(start0, 0), b = min(stop0, L - 1);                            // addCoverage :605-606
        const bbidx_read rd = A.V.reads[r];
        const int len = rd.len;
        nMapped++; nBases += len;                                                       // :612-613
        // basecount (:619-624): charToNum's slots 0-3 are A/a, C/c, G/g, T/t/U/u
        int cA = 0, cC = 0, cG = 0, cT = 0;
        const uint8_t *bases = A.V.bases + rd.bases_off;
        for (int base = 0; base < len; base += 64) {
            const int ch = (base + lane < len ? bases[base + lane] : 0) & ~0x20;
            cA += popc(__ballot(ch == 'A')); cC += popc(__ballot(ch == 'C'));
            cG += popc(__ballot(ch == 'G')); cT += popc(__ballot(ch == 'T' || ch == 'U'));
        }
        int *diff = A.diff[(A.flags & BBMAP_COV_STRANDED) && strand == 1 ? 1 : 0] + A.covoff[gs];
        long long basehits;
        if (A.flags & BBMAP_COV_START_ONLY) {                                           // ca.increment(start) (:642-643)
            basehits = (long long)b - a + 1;
            if (a < L && lane < 2) atomicAdd(diff + a + lane, lane ? -1 : 1);
        } else if (!(A.flags & BBMAP_COV_EXCLUDE_DELETIONS)) {                          // ca.incrementRange(start, stop, 1) (:645)
            basehits = (long long)b - a + 1;                                            // negative for a record left of its scaffold
            if (b >= a && lane < 2) atomicAdd(diff + (lane ? b + 1 : a), lane ? -1 : 1);
        } else basehits = walk_excluding_deletions(R.m, R.ml, a, b, diff, lane);
        // the record's counters, one per lane: basehits, readhits, readhitsMinus, fraghits (2 - mateCount, :807), A C G T
        long long mine = 0;
        mine = lane == A_basehits ? basehits : mine;
        mine = lane == A_readhits ? 1 : mine;
        mine = lane == A_readhitsMinus ? (strand == 1) : mine;
        mine = lane == A_fraghits ? (A.V.paired ? 1 : 2) : mine;
        mine = lane == A_readBases ? cA : lane == A_readBases + 1 ? cC : lane == A_readBases + 2 ? cG : lane == A_readBases + 3 ? cT : mine;
        if (lane < N_ACC && mine) {
            if (useLds) atomicAdd(&acc[gs * N_ACC + lane], (u64)mine);
            else atomicAdd(&A.recs[(long long)gs * REC_WORDS + ACC_BASE + lane], (u64)mine);
        }
    }
    if (lane < 3) {
        const long long v = lane == 0 ? nProcessed : lane == 1 ? nMapped : nBases;
        if (v) atomicAdd(&A.totals[lane], (u64)v);
    }
    __syncthreads();
    if (useLds) for (int k = threadIdx.x; k < A.nscaf * N_ACC; k += TB) {
        const u64 v = acc[k];
        if (v) atomicAdd(&A.recs[(long long)(k / N_ACC) * REC_WORDS + ACC_BASE + (k % N_ACC)], v);
    }
}

hipError_t launch_add(const AddArgs &a, hipStream_t stream) {
    if (a.V.n <= 0) return hipSuccess;
    const long long want = (a.V.n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    const unsigned blocks = (unsigned)(want < MAX_BLOCKS ? want : MAX_BLOCKS);
    hipLaunchKernelGGL(coverage_add_kernel, dim3(blocks), dim3(TB), 0, stream, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ prefix sum

// exclusive scan of one value per thread over the block (TB threads); *total = the block's sum.  lds: WAVES_PER_BLOCK entries
__device__ inline long long block_exclusive_scan(long long v, long long *total, long long *lds) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    long long inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) lds[wid] = inc;
    __syncthreads();
    long long before = 0, all = 0;
    for (int w = 0; w < WAVES_PER_BLOCK; w++) { const long long t = lds[w]; before += w < wid ? t : 0; all += t; }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// sums[tile] = the sum of in[tile * TILE ...)
template <class T> __global__ __launch_bounds__(TB) void tile_sums_kernel(const T *in, long long n, long long *sums) {
    __shared__ long long lds[WAVES_PER_BLOCK];
    const long long at = (long long)blockIdx.x * TILE + (long long)threadIdx.x * PER_THREAD;
    long long v = 0;
    for (int j = 0; j < PER_THREAD; j++) v += at + j < n ? (long long)in[at + j] : 0;
    long long total;
    (void)block_exclusive_scan(v, &total, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data[i] becomes carry[tile] + the sum of its tile's elements before i (carry == nullptr: 0; one block then scans n <= TILE elements)
__global__ __launch_bounds__(TB) void scan_tiles_kernel(long long *data, long long n, const long long *carry) {
    __shared__ long long lds[WAVES_PER_BLOCK];
    const long long at = (long long)blockIdx.x * TILE + (long long)threadIdx.x * PER_THREAD;
    long long x[PER_THREAD], v = 0;
    for (int j = 0; j < PER_THREAD; j++) { x[j] = at + j < n ? data[at + j] : 0; v += x[j]; }
    long long total;
    long long run = block_exclusive_scan(v, &total, lds) + (carry ? carry[blockIdx.x] : 0);
    for (int j = 0; j < PER_THREAD; j++) {
        if (at + j < n) data[at + j] = run;
        run += x[j];
    }
}

// depth[i] = min(the sum of diff[0 .. i], cap): tile t starts from carry[t], an int64
template <class D> __global__ __launch_bounds__(TB) void apply_depth_kernel(const int *diff, long long n, const long long *carry, D *depth,
                                                                            long long cap) {
    __shared__ long long lds[WAVES_PER_BLOCK];
    const long long at = (long long)blockIdx.x * TILE + (long long)threadIdx.x * PER_THREAD;
    int x[PER_THREAD];
    long long v = 0;
    for (int j = 0; j < PER_THREAD; j++) { x[j] = at + j < n ? diff[at + j] : 0; v += x[j]; }
    long long total;
    long long run = block_exclusive_scan(v, &total, lds) + carry[blockIdx.x];
    for (int j = 0; j < PER_THREAD; j++) {
        run += x[j];
        if (at + j < n) depth[at + j] = (D)(run < 0 ? 0 : run > cap ? cap : run);
    }
}

// ------------------------------------------------------------------------------------------------------------------ statistics

// length, refBases and zeroed strand records for a new snapshot; totals.refBases (loadScaffoldsFromIndex :445)
__global__ __launch_bounds__(256) void prepare_records_kernel(int nscaf, long long slots, const int *len, const long long *refgc, u64 *recs,
                                                              u64 *totals) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s == 0) totals[3] = (u64)(slots - nscaf);
    if (s >= nscaf) return;
    u64 *rec = recs + (long long)s * REC_WORDS;
    rec[0] = (u64)len[s];
    for (int k = 0; k < 4; k++) rec[REF_BASE + k] = refgc ? (u64)refgc[4LL * s + k] : 0;
    for (int k = 0; k < 2 * STRAND_WORDS; k++) rec[STRAND_BASE + k] = 0;
}

// the scaffold that owns slot `at`: the last s with covoff[s] <= at
__device__ inline int scaffold_of_slot(const long long *covoff, int nscaf, long long at) {
    int lo = 0, hi = nscaf - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (covoff[mid] <= at) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct Moments { u64 covered, sum, sqLo, sqHi, mx; };
__device__ inline void add_to(Moments &a, const Moments &b) {
    a.covered += b.covered; a.sum += b.sum;
    const u64 lo = a.sqLo + b.sqLo;
    a.sqHi += b.sqHi + (lo < a.sqLo);
    a.sqLo = lo;
    a.mx = a.mx > b.mx ? a.mx : b.mx;
}
__device__ inline Moments shuffled_down(const Moments &m, int d) {
    Moments o;
    o.covered = __shfl_down(m.covered, d, 64); o.sum = __shfl_down(m.sum, d, 64);
    o.sqLo = __shfl_down(m.sqLo, d, 64); o.sqHi = __shfl_down(m.sqHi, d, 64); o.mx = __shfl_down(m.mx, d, 64);
    return o;
}

// One workgroup per CHUNK slots.  For every scaffold that reaches into the chunk, over its positions < length (the extra slot is not
// a base): covered, sum, sum of squares (128 bit) and max go to the scaffold's record with one atomic each per workgroup; the
// histogram's low bins are counted in LDS and added once per workgroup (depth 0 and the modal depth are otherwise single hot
// addresses), higher depths go to HBM directly; a bin's sum is added once per run of lanes that share the bin.
template <class D> __global__ __launch_bounds__(TB) void coverage_stats_kernel(const D *depth, const long long *covoff, int nscaf, long long slots,
                                                                               u64 *recs, int strand, u64 *hist, long long histmax,
                                                                               int binsize, const long long *binoff, u64 *bins) {
    __shared__ unsigned lh[HIST_LDS];
    __shared__ Moments part[WAVES_PER_BLOCK];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < HIST_LDS; k += TB) lh[k] = 0;
    __syncthreads();
    const long long t0 = (long long)blockIdx.x * CHUNK, t1 = min(slots, t0 + CHUNK);
    for (int s = scaffold_of_slot(covoff, nscaf, t0); s < nscaf && covoff[s] < t1; s++) {
        const long long first = covoff[s], L = covoff[s + 1] - first - 1;
        const long long lo = max(t0, first), hi = min(t1, first + L);
        Moments mine = {0, 0, 0, 0, 0};
        for (long long base = lo; base < hi; base += TB) {
            const long long i = base + threadIdx.x;
            const bool valid = i < hi;
            const u64 d = valid ? (u64)depth[i] : 0;
            // depth 0 is most of a shallow genome: its lanes are counted with one ballot and one LDS add, not 64 adds to one address
            const u64 zeros = __ballot(valid && d == 0);
            if (zeros && lane == __builtin_ctzll(zeros)) atomicAdd(&lh[0], (unsigned)popc(zeros));
            if (valid && d) {
                Moments one = {1, d, d * d, 0, d};
                add_to(mine, one);
                const long long h = (long long)d < histmax ? (long long)d : histmax;    // hist.increment(Tools.min(x, histmax)) (:1025)
                if (h < HIST_LDS) atomicAdd(&lh[h], 1u); else atomicAdd(&hist[h], 1ull);
            }
            if (binsize > 0) {                                                          // writeCoveragePerBaseBinned2's sums (:1298-1311)
                const int bin = valid ? (int)((i - first) / binsize) : -1;
                u64 inc = d;                                                            // inclusive prefix sums over the wavefront
                for (int k = 1; k < 64; k <<= 1) {
                    const u64 t = __shfl_up(inc, k, 64);
                    if (lane >= k) inc += t;
                }
                const int before = __shfl_up(bin, 1, 64), after = __shfl_down(bin, 1, 64);
                const u64 heads = __ballot(lane == 0 || bin != before);
                const int head = hibit(heads & (lt_mask(lane) | (1ull << lane)));       // where this lane's run of one bin begins
                const u64 ahead = __shfl(inc, head > 0 ? head - 1 : 0, 64);
                if (bin >= 0 && (lane == 63 || bin != after)) atomicAdd(&bins[binoff[s] + bin], inc - (head > 0 ? ahead : 0));
            }
        }
        for (int k = 32; k > 0; k >>= 1) add_to(mine, shuffled_down(mine, k));
        if (lane == 0) part[wid] = mine;
        __syncthreads();
        if (threadIdx.x == 0 && hi > lo) {
            Moments all = part[0];
            for (int w = 1; w < WAVES_PER_BLOCK; w++) add_to(all, part[w]);
            u64 *st = recs + (long long)s * REC_WORDS + STRAND_BASE + strand * STRAND_WORDS;
            if (all.covered) atomicAdd(&st[S_covered], all.covered);
            if (all.sum) atomicAdd(&st[S_sumDepth], all.sum);
            if (all.mx) atomicMax(&st[S_max], all.mx);
            // a 128-bit add in two halves: the low word's atomic returns what it added to, which tells the carry
            u64 carry = 0;
            if (all.sqLo) { const u64 old = atomicAdd(&st[S_sumSqLo], all.sqLo); carry = old + all.sqLo < old; }
            if (all.sqHi + carry) atomicAdd(&st[S_sumSqHi], all.sqHi + carry);
        }
        __syncthreads();
    }
    for (int k = threadIdx.x; k < HIST_LDS; k += TB) {
        const unsigned v = lh[k];
        if (v) atomicAdd(&hist[k], (u64)v);
    }
}

// ------------------------------------------------------------------------------------------------------------------ Median_fold
// writeStats sorts the scaffold's length + 1 elements descending and takes element length / 2 (:1033-1042).  That order statistic
// comes from a radix select on 8-bit digits from the top: count the digit among the elements that match the digits chosen so far,
// walk the counts from 255 down to the digit that holds rank k, go on with the rank inside it.  Two rounds for 16-bit depths, four
// for 32-bit ones.

// the digit that holds rank k among counts taken from 255 down; k becomes the rank inside that digit
__device__ inline int pick_digit(const unsigned *cnt, long long &k) {
    int d = 255;
    for (; d > 0; d--) {
        if (k < (long long)cnt[d]) break;
        k -= cnt[d];
    }
    return d;
}

// cnt[digit]++ for the calling lanes (any subset of the wavefront).  Digit 0 is the common one (the high byte of nearly every depth,
// the low byte of an uncovered base): its lanes are counted with one ballot and one add by their first lane.
__device__ inline void count_digit(unsigned *cnt, unsigned digit) {
    const u64 zeros = __ballot(digit == 0);
    if (digit) atomicAdd(&cnt[digit], 1u);
    else if ((int)(threadIdx.x & 63) == __builtin_ctzll(zeros)) atomicAdd(&cnt[0], (unsigned)popc(zeros));
}

// scaffolds of up to MEDIAN_SHORT bases: one workgroup per scaffold, the digit counts in LDS
template <class D, int ROUNDS> __global__ __launch_bounds__(TB) void median_short_kernel(const D *depth, const long long *covoff, int nscaf,
                                                                                         u64 *recs, int strand) {
    __shared__ unsigned cnt[256];
    __shared__ unsigned chosen;
    const int s = blockIdx.x;
    const long long first = covoff[s], L = covoff[s + 1] - first - 1;
    if (L > MEDIAN_SHORT) return;
    unsigned prefix = 0;
    long long k = L / 2;
    for (int round = 0; round < ROUNDS; round++) {
        const int shift = 8 * (ROUNDS - 1 - round);
        cnt[threadIdx.x] = 0;
        __syncthreads();
        for (long long i = threadIdx.x; i <= L; i += TB) {
            const unsigned v = (unsigned)depth[first + i];
            if (round == 0 || (v >> (shift + 8)) == (prefix >> (shift + 8))) count_digit(cnt, (v >> shift) & 255);
        }
        __syncthreads();
        if (threadIdx.x == 0) chosen = (unsigned)pick_digit(cnt, k);       // (every thread keeps its own k: only thread 0's is used)
        __syncthreads();
        prefix |= chosen << shift;
        __syncthreads();
    }
    if (threadIdx.x == 0) recs[(long long)s * REC_WORDS + STRAND_BASE + strand * STRAND_WORDS + S_median] = prefix;
}

// Longer scaffolds: many workgroups count, one thread per scaffold picks.  A long scaffold owns more than MEDIAN_SHORT slots, so
// covoff[s] / MEDIAN_SHORT is a number no other long scaffold has: its row of 256 counts in HBM.
struct Select { unsigned *prefix; long long *k; unsigned *counts; };

__global__ __launch_bounds__(256) void median_begin_kernel(const long long *covoff, int nscaf, Select S) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nscaf) return;
    S.prefix[s] = 0;
    S.k[s] = (covoff[s + 1] - covoff[s] - 1) / 2;
}

template <class D> __global__ __launch_bounds__(TB) void median_count_kernel(const D *depth, const long long *covoff, int nscaf, long long slots,
                                                                             Select S, int shift, int first_round) {
    __shared__ unsigned cnt[256];
    const long long t0 = (long long)blockIdx.x * CHUNK, t1 = min(slots, t0 + CHUNK);
    for (int s = scaffold_of_slot(covoff, nscaf, t0); s < nscaf && covoff[s] < t1; s++) {
        const long long first = covoff[s], L = covoff[s + 1] - first - 1;
        if (L <= MEDIAN_SHORT) continue;
        const long long lo = max(t0, first), hi = min(t1, first + L + 1);          // the extra slot takes part
        const unsigned prefix = S.prefix[s];
        cnt[threadIdx.x] = 0;
        __syncthreads();
        for (long long i = lo + threadIdx.x; i < hi; i += TB) {
            const unsigned v = (unsigned)depth[i];
            if (first_round || (v >> (shift + 8)) == (prefix >> (shift + 8))) count_digit(cnt, (v >> shift) & 255);
        }
        __syncthreads();
        const unsigned c = cnt[threadIdx.x];
        if (c) atomicAdd(&S.counts[(first / MEDIAN_SHORT) * 256 + threadIdx.x], c);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void median_pick_kernel(const long long *covoff, int nscaf, Select S, int shift, int last_round, u64 *recs,
                                                          int strand) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nscaf) return;
    const long long first = covoff[s], L = covoff[s + 1] - first - 1;
    if (L <= MEDIAN_SHORT) return;
    long long k = S.k[s];
    const unsigned prefix = S.prefix[s] | ((unsigned)pick_digit(S.counts + (first / MEDIAN_SHORT) * 256, k) << shift);
    S.prefix[s] = prefix; S.k[s] = k;
    if (last_round) recs[(long long)s * REC_WORDS + STRAND_BASE + strand * STRAND_WORDS + S_median] = prefix;
}

// ------------------------------------------------------------------------------------------------------------------ finalize

static long long tiles_of(long long n) { return (n + TILE - 1) / TILE; }
static long long up8(long long bytes) { return (bytes + 7) & ~7ll; }
static long long median_rows(long long slots) { return slots / MEDIAN_SHORT + 1; }

// workspace: sums of the tiles, sums of those, the select's prefix / rank per scaffold, its rows of counts
long long workspace_bytes(int nscaf, long long slots) {
    const long long t0 = tiles_of(slots), t1 = tiles_of(t0);
    return 8 * (t0 + t1) + up8(4LL * nscaf) + 8LL * nscaf + 1024 * median_rows(slots);
}

template <class D, int ROUNDS> static hipError_t finalize_strand(const FinArgs &a, int strand, hipStream_t stream) {
    const long long n = a.slots, t0 = tiles_of(n), t1 = tiles_of(t0);
    long long *sums0 = (long long *)a.ws, *sums1 = sums0 + t0;
    Select S;
    S.prefix = (unsigned *)(sums1 + t1);
    S.k = (long long *)((char *)S.prefix + up8(4LL * a.nscaf));
    S.counts = (unsigned *)(S.k + a.nscaf);
    D *depth = (D *)a.depth[strand];
    const long long cap = sizeof(D) == 2 ? 65535 : INT_MAX;
    // reduce-then-scan: sums of the tiles, sums of THEIR tiles (t1 <= TILE: one block scans them), and back down
    hipLaunchKernelGGL(tile_sums_kernel<int>, dim3((unsigned)t0), dim3(TB), 0, stream, a.diff[strand], n, sums0);
    hipLaunchKernelGGL(tile_sums_kernel<long long>, dim3((unsigned)t1), dim3(TB), 0, stream, (const long long *)sums0, t0, sums1);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(TB), 0, stream, sums1, t1, (const long long *)nullptr);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3((unsigned)t1), dim3(TB), 0, stream, sums0, t0, (const long long *)sums1);
    hipLaunchKernelGGL(apply_depth_kernel<D>, dim3((unsigned)t0), dim3(TB), 0, stream, a.diff[strand], n, (const long long *)sums0, depth, cap);
    const long long hb = hist_bins(a.flags);
    hipError_t e = hipMemsetAsync(a.hist[strand], 0, 8 * (size_t)hb, stream);
    if (e != hipSuccess) return e;
    if (a.binsize > 0 && a.nbins > 0 && (e = hipMemsetAsync(a.bins[strand], 0, 8 * (size_t)a.nbins, stream)) != hipSuccess) return e;
    const unsigned chunks = (unsigned)((n + CHUNK - 1) / CHUNK);
    hipLaunchKernelGGL(coverage_stats_kernel<D>, dim3(chunks), dim3(TB), 0, stream, (const D *)depth, a.covoff, a.nscaf, n, a.recs, strand,
                       a.hist[strand], hb - 1, a.binsize, a.binoff, a.bins[strand]);
    hipLaunchKernelGGL((median_short_kernel<D, ROUNDS>), dim3((unsigned)a.nscaf), dim3(TB), 0, stream, (const D *)depth, a.covoff, a.nscaf, a.recs,
                       strand);
    const unsigned sblocks = (unsigned)((a.nscaf + 255) / 256);
    if (n - a.nscaf > MEDIAN_SHORT) {                   // (only then can a scaffold be a long one)
        hipLaunchKernelGGL(median_begin_kernel, dim3(sblocks), dim3(256), 0, stream, a.covoff, a.nscaf, S);
        for (int round = 0; round < ROUNDS; round++) {
            const int shift = 8 * (ROUNDS - 1 - round);
            if ((e = hipMemsetAsync(S.counts, 0, 1024 * (size_t)median_rows(n), stream)) != hipSuccess) return e;
            hipLaunchKernelGGL(median_count_kernel<D>, dim3(chunks), dim3(TB), 0, stream, (const D *)depth, a.covoff, a.nscaf, n, S, shift,
                               round == 0);
            hipLaunchKernelGGL(median_pick_kernel, dim3(sblocks), dim3(256), 0, stream, a.covoff, a.nscaf, S, shift, round == ROUNDS - 1, a.recs,
                               strand);
        }
    }
    return hipGetLastError();
}

hipError_t launch_finalize(const FinArgs &a, hipStream_t stream) {
    if (a.nscaf <= 0) return hipSuccess;
    hipLaunchKernelGGL(prepare_records_kernel, dim3((unsigned)((a.nscaf + 255) / 256)), dim3(256), 0, stream, a.nscaf, a.slots, a.len, a.refgc,
                       a.recs, a.totals);
    const int strands = a.flags & BBMAP_COV_STRANDED ? 2 : 1;
    for (int t = 0; t < strands; t++) {
        const hipError_t e = a.flags & BBMAP_COV_32BIT ? finalize_strand<int, 4>(a, t, stream) : finalize_strand<uint16_t, 2>(a, t, stream);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ reference GC

// ChromosomeArray.countACGTINOC's slots 0-3 over [loc, loc + length) of the scaffold's chromosome; blockIdx.x = scaffold, the
// workgroups of one scaffold (blockIdx.y) take turns over pieces of 64 Ki bases
__global__ __launch_bounds__(TB) void reference_gc_kernel(const bbscaf::Table T, int nscaf, const uint8_t *const *chromArr, u64 *refgc) {
    __shared__ unsigned part[WAVES_PER_BLOCK][4];
    const int s = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int chrom = 1;
    while (chrom < T.nchroms && T.off[chrom + 1] <= s) chrom++;
    const uint8_t *ref = chromArr[chrom] + T.loc[s];
    const long long L = T.len[s];
    for (long long piece = (long long)blockIdx.y * CHUNK; piece < L; piece += (long long)gridDim.y * CHUNK) {
        const long long hi = min(L, piece + CHUNK);
        unsigned c[4] = {0, 0, 0, 0};
        for (long long i = piece + threadIdx.x; i < hi; i += TB) {
            const int ch = ref[i] & ~0x20;
            c[0] += ch == 'A'; c[1] += ch == 'C'; c[2] += ch == 'G'; c[3] += ch == 'T' || ch == 'U';
        }
        for (int j = 0; j < 4; j++) {
            for (int k = 32; k > 0; k >>= 1) c[j] += __shfl_down(c[j], k, 64);
            if (lane == 0) part[wid][j] = c[j];
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            u64 v = 0;
            for (int w = 0; w < WAVES_PER_BLOCK; w++) v += part[w][threadIdx.x];
            if (v) atomicAdd(&refgc[4LL * s + threadIdx.x], v);
        }
        __syncthreads();
    }
}

hipError_t launch_refgc(const bbscaf::Table &T, int nscaf, const uint8_t *const *chromArr, long long *refgc, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(refgc, 0, 32 * (size_t)nscaf, stream);
    if (e != hipSuccess) return e;
    // (blockIdx.x carries the scaffold: up to 2^31 - 1 of them; 64 workgroups per scaffold keep a chromosome-sized one busy)
    hipLaunchKernelGGL(reference_gc_kernel, dim3((unsigned)nscaf, 64), dim3(TB), 0, stream, T, nscaf, chromArr, (u64 *)refgc);
    return hipGetLastError();
}

}  // namespace bbcov

// ---------------------------------------------------------------------------------------------------------------------- raw C ABI

extern "C" int bbpipe_coverage_layout(int32_t nscaf, const int32_t *lengths, int32_t binsize, int64_t *covoff, int64_t *binoff) {
    if (nscaf < 0 || binsize < 0 || (nscaf > 0 && !lengths)) return bbfail(BBMAP_E_ARG, "bbpipe_coverage_layout: bad argument");
    int64_t slots = 0, bins = 0;
    for (int32_t s = 0; s < nscaf; s++) {
        const int64_t L = lengths[s];
        if (L < 1) return bbfail(BBMAP_E_ARG, "bbpipe_coverage_layout: a scaffold's length must be >= 1");
        if (covoff) covoff[s] = slots;
        if (binoff && binsize > 0) binoff[s] = bins;
        slots += L + 1;
        if (binsize > 0) bins += (L + binsize - 1) / binsize;       // the last bin is the short one (KEEP_SHORT_BINS)
    }
    if (covoff) covoff[nscaf] = slots;
    if (binoff && binsize > 0) binoff[nscaf] = bins;
    return BBMAP_OK;
}

extern "C" int64_t bbpipe_coverage_workspace_bytes(int32_t nscaf, int64_t slots) {
    if (nscaf < 0 || slots < 0 || slots > (1ll << 32)) return bbfail(BBMAP_E_ARG, "bbpipe_coverage_workspace_bytes: bad argument");
    return bbcov::workspace_bytes(nscaf, slots);
}

static const int COV_ALL_FLAGS = BBMAP_COV_START_ONLY | BBMAP_COV_EXCLUDE_DELETIONS | BBMAP_COV_STRANDED | BBMAP_COV_32BIT;

extern "C" int bbpipe_coverage_add_device(void *stream, int64_t n_reads, int32_t paired, int32_t flags, const bbidx_read *reads,
                                          const uint8_t *bases, const bbmap_final *finals, const uint8_t *pool, int32_t nchroms, int32_t nscaf,
                                          const int32_t *scaf_off, const int32_t *scaf_loc, const int32_t *scaf_len, int32_t pad,
                                          const int64_t *covoff, int32_t *diff0, int32_t *diff1, bbmap_covrec *recs, bbmap_covtotals *totals) {
    if (n_reads < 0 || (paired && (n_reads & 1)) || nchroms < 1 || nscaf < nchroms || pad < 0)
        return bbfail(BBMAP_E_ARG, "bbpipe_coverage_add_device: bad argument");
    if (flags & ~COV_ALL_FLAGS) return bbfail(BBMAP_E_ARG, "bbpipe_coverage_add_device: unknown flag bits");
    if (n_reads == 0) return BBMAP_OK;
    if (!reads || !bases || !finals || !pool || !scaf_off || !scaf_loc || !scaf_len || !covoff || !diff0 || !recs || !totals ||
        ((flags & BBMAP_COV_STRANDED) && !diff1))
        return bbfail(BBMAP_E_ARG, "bbpipe_coverage_add_device: null buffer");
    bbcov::AddArgs a = {};
    a.V.reads = reads; a.V.bases = bases; a.V.fin = finals; a.V.pool = pool;      // (no tier)
    a.V.n = n_reads; a.V.paired = paired ? 1 : 0; a.flags = flags;
    a.T.off = scaf_off; a.T.loc = scaf_loc; a.T.len = scaf_len; a.T.pad = pad; a.T.nchroms = nchroms;
    a.nscaf = nscaf; a.covoff = (const long long *)covoff;
    a.diff[0] = diff0; a.diff[1] = diff1;
    a.recs = (unsigned long long *)recs; a.totals = (unsigned long long *)totals;
    BBHIP(bbcov::launch_add(a, (hipStream_t)stream));
    return BBMAP_OK;
}

extern "C" int bbpipe_coverage_finalize_device(void *stream, int32_t flags, int32_t nscaf, int64_t slots, const int32_t *scaf_len,
                                               const int64_t *covoff, const int32_t *diff0, const int32_t *diff1, void *depth0, void *depth1,
                                               bbmap_covrec *recs, const int64_t *refgc, int64_t *hist0, int64_t *hist1, int32_t binsize,
                                               const int64_t *binoff, int64_t nbins, int64_t *bins0, int64_t *bins1, bbmap_covtotals *totals,
                                               void *workspace, int64_t workspace_bytes) {
    if (nscaf < 1 || slots < 2LL * nscaf || slots > (1ll << 32) || binsize < 0 || nbins < 0)
        return bbfail(BBMAP_E_ARG, "bbpipe_coverage_finalize_device: bad argument");
    if (flags & ~COV_ALL_FLAGS) return bbfail(BBMAP_E_ARG, "bbpipe_coverage_finalize_device: unknown flag bits");
    const bool two = flags & BBMAP_COV_STRANDED;
    if (!scaf_len || !covoff || !diff0 || !depth0 || !recs || !hist0 || !totals || !workspace || (two && (!diff1 || !depth1 || !hist1)) ||
        (binsize > 0 && (!binoff || !bins0 || (two && !bins1))))
        return bbfail(BBMAP_E_ARG, "bbpipe_coverage_finalize_device: null buffer");
    if (workspace_bytes < bbcov::workspace_bytes(nscaf, slots))
        return bbfail(BBMAP_E_ARG, "bbpipe_coverage_finalize_device: the workspace is smaller than bbpipe_coverage_workspace_bytes");
    bbcov::FinArgs a = {};
    a.flags = flags; a.nscaf = nscaf; a.slots = slots; a.len = scaf_len; a.covoff = (const long long *)covoff;
    a.diff[0] = diff0; a.diff[1] = diff1; a.depth[0] = depth0; a.depth[1] = depth1;
    a.recs = (unsigned long long *)recs; a.refgc = (const long long *)refgc;
    a.hist[0] = (unsigned long long *)hist0; a.hist[1] = (unsigned long long *)hist1;
    a.binsize = binsize; a.binoff = (const long long *)binoff; a.nbins = nbins;
    a.bins[0] = (unsigned long long *)bins0; a.bins[1] = (unsigned long long *)bins1;
    a.totals = (unsigned long long *)totals; a.ws = workspace;
    BBHIP(bbcov::launch_finalize(a, (hipStream_t)stream));
    return BBMAP_OK;
}
