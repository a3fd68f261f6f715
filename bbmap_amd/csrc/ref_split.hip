// Reference-set binning on the device: align2.BBSplitter.printReads as AbstractMapThread.writeList calls it
// (current/align2/AbstractMapThread.java:608-610) -- scafstats, refstats and the assignment of every read or pair to the output streams
// of its reference sets.
//   printReadsAndProcessAmbiguous (current/align2/BBSplitter.java:641-757), addToScafCounts (:782-820), getSets (:824-864),
//   getScaffolds (:867-933), toListNames (:1033-1048); the scaffold of a record or a site is Data.scaffoldIndex(chrom, (start+stop)/2)
//   (current/stream/Read.java:3304-3316, current/stream/SiteScore.java:367-377, current/dna/Data.java:1091-1108).
// Names are the host's: a scaffold carries a 64-bit mask of reference sets and a key index, so a HashSet of set names is an OR of
// masks, equals / containsAll are mask arithmetic, and the scafstats key set of an ambiguous read is a short list of integers.
//
// refsplit_assign_kernel, one read per lane.  A lane walks the first min(nsites, maxSites) sites of its read down to the clearzone break
// (:844 / :900), one binary search in the scaffold table per site; mates sit in neighbouring lanes and exchange (primary, other,
// mapScore, length) with one xor-1 shuffle each, then both compute the pair's verdict and write the same masks.  Counting is written
// for contention: a workgroup combines equal keys in an open-addressed LDS table (key -> four 64-bit sums) and keeps the 64 x 4 set
// counters in LDS outright; after a chunk of CHUNK reads every slot that moved goes to the state with one 64-bit atomic per counter
// that moved.  An insert that finds MAX_PROBES slots taken by other keys adds to the state directly, so a chunk with more distinct
// keys than slots (a metagenome) degrades to what it would cost without the table.  Everything is an integer: the result does not
// depend on the order of the adds.
//
// The stream lists are a stable partition of the units over 2 x nsets rows without atomics: per-workgroup row counts (one ballot and
// popcount per row and wavefront), a device-wide exclusive scan over (row, workgroup), and a placing pass that repeats the ballots and
// puts a unit at its workgroup's base + the units of earlier wavefronts + the lanes below it.
#include "ref_split.h"

#include <hipcub/hipcub.hpp>

#include "host_common.h"
#include "wave_prims.h"

namespace bbsplit {
using wavep::u64;
using wavep::lt_mask;
using wavep::popc;

constexpr int EMPTY = -1;
enum { KEEP = 8 };                  // distinct keys of one ambiguous read held in registers; more are found by walking the list again

struct ToLL { __host__ __device__ long long operator()(int v) const { return (long long)v; } };

const char *check_config(const bbmap_split_config &cfg) {
    if (cfg.flags & ~BBMAP_SPLIT_ALL) return "unknown flag bits";
    if (cfg.ambiguous2 == BBMAP_AMBIG2_RANDOM) return "AMBIGUOUS2_RANDOM is not implemented (the reference throws)";
    if (cfg.ambiguous2 < BBMAP_AMBIG2_UNSET || cfg.ambiguous2 > BBMAP_AMBIG2_ALL) return "unknown ambiguous2 mode";
    if (cfg.nsets < 0 || cfg.nsets > BBMAP_SPLIT_MAX_SETS) return "at most 64 reference sets are supported";
    if (cfg.nkeys < 0 || cfg.maxSites < 1 || cfg.clearzone < 0) return "bad nkeys, maxSites or clearzone";
    return nullptr;
}

struct Lds { int key[SLOTS]; u64 sum[SLOTS * 4]; u64 set[MAX_SETS * 4]; };

// counters[key][2 cls], [2 cls + 1] += 1, len (cls 0 = unambiguous, 1 = ambiguous) through the workgroup's table
__device__ inline void add_key(Lds &L, u64 *keyState, int key, int cls, int len) {
    const u64 bases = (u64)(long long)len;
    unsigned h = ((unsigned)key * 2654435761u) >> 22;
    for (int t = 0; t < MAX_PROBES; t++) {
        const int prev = atomicCAS(&L.key[h], EMPTY, key);
        if (prev == EMPTY || prev == key) {
            atomicAdd(&L.sum[h * 4 + 2 * cls], 1ull);
            atomicAdd(&L.sum[h * 4 + 2 * cls + 1], bases);
            return;
        }
        h = (h + 1) & (SLOTS - 1);
    }
    atomicAdd(keyState + 4ll * key + 2 * cls, 1ull);
    atomicAdd(keyState + 4ll * key + 2 * cls + 1, bases);
}

// Data.scaffoldIndex(chrom, (start + stop) / 2) as a global scaffold number; -1 for a chromosome outside the table
__device__ inline int scaffold_of(const bbscaf::Table &T, int chrom, int start, int stop) {
    if (chrom < 1 || chrom > T.nchroms) return -1;
    const int b = T.off[chrom], ns = T.off[chrom + 1] - b;
    if (ns < 1) return -1;
    const int mid = (int)((unsigned)start + (unsigned)stop) / 2;
    const int key = (int)((unsigned)mid + (unsigned)(T.pad / 2));                           // :1096
    return b + (ns < 2 ? 0 : bbscaf::last_at_or_below(T.loc + b, ns, key));
}

__global__ __launch_bounds__(TB) void refsplit_assign_kernel(const Args A) {
    __shared__ Lds L;
    const bool doScaf = (A.flags & BBMAP_SPLIT_SCAF_STATS) && A.state && A.nkeys > 0;
    const bool doSet = (A.flags & BBMAP_SPLIT_SET_STATS) && A.state && A.nsets > 0;
    u64 *keyState = A.state + HEAD, *setState = A.state + HEAD + 4ll * A.nkeys;
    const u64 setMask = A.nsets >= 64 ? ~0ull : (1ull << A.nsets) - 1ull;
    for (int k = threadIdx.x; k < SLOTS; k += TB) L.key[k] = EMPTY;
    for (int k = threadIdx.x; k < SLOTS * 4; k += TB) L.sum[k] = 0;
    for (int k = threadIdx.x; k < MAX_SETS * 4; k += TB) L.set[k] = 0;
    __syncthreads();
    if (A.state && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(A.state, (u64)A.V.n);         // totalReads
    for (long long chunk = blockIdx.x; chunk * CHUNK < A.V.n; chunk += gridDim.x) {
        const long long end = min(A.V.n, (chunk + 1) * CHUNK);
        for (long long base = chunk * CHUNK; base < end; base += TB) {
            const long long r = base + threadIdx.x;
            const bool valid = r < end;
            u64 p = 0, o = 0;
            int mapScore = 0, len = 0, ownKey = -1;
            bool mapped = false, ambRead = false;
            if (valid) {
                const ReadRec R = record_of<TierRule::ByList, true>(A.V, r);
                const int nlist = min(R.n, A.maxSites);                                          // capSiteList
                const bool flagged = (R.flag == BBMAP_NSITES_OVERFLOW) | (R.flag == BBMAP_NSITES_MATE_OVERFLOW);
                len = A.V.reads[r].len;
                mapped = R.f->mapped != 0 && !flagged;
                mapScore = R.f->mapScore;
                ambRead = mapped && R.f->ambiguous != 0;
                if (mapped) {
                    const int gs = scaffold_of(A.T, R.f->chrom, R.f->start, R.f->stop);
                    const int k = gs >= 0 ? A.scafKey[gs] : -1;
                    ownKey = (unsigned)k < (unsigned)A.nkeys ? k : -1;
                    if (doScaf && !ambRead && ownKey >= 0) add_key(L, keyState, ownKey, 0, len);         // :872-893
                }
                if (mapped && nlist > 0) {
                    int kept[KEEP], nk = 0;
#pragma unroll
                    for (int k = 0; k < KEEP; k++) kept[k] = -1;
                    const int s0 = R.s[0].score;
                    for (int j = 0; j < nlist; j++) {
                        const bbmap_msite *ss = R.s + j;
                        if (j > 0 && (int)((unsigned)ss->score + (unsigned)A.clearzone) < s0) break;     // :844 / :900
                        const int gs = scaffold_of(A.T, ss->chrom, ss->start, ss->stop);
                        if (gs < 0) continue;
                        const u64 m = A.scafSets[gs] & setMask;                                   // toListNames
                        if (j == 0) p = m; else o |= m;
                        if (!(doScaf && ambRead)) continue;
                        const int key = A.scafKey[gs];                                           // getScaffolds :897-913
                        if ((unsigned)key >= (unsigned)A.nkeys) continue;
                        bool seen = false;
#pragma unroll
                        for (int k = 0; k < KEEP; k++) seen |= kept[k] == key;
                        if (!seen && nk == KEEP)
                            for (int i = 0; i < j && !seen; i++) {
                                const int gi = scaffold_of(A.T, R.s[i].chrom, R.s[i].start, R.s[i].stop);
                                seen = gi >= 0 && A.scafKey[gi] == key;
                            }
                        if (seen) continue;
#pragma unroll
                        for (int k = 0; k < KEEP; k++) if (k == nk) kept[k] = key;
                        nk = min(nk + 1, (int)KEEP);
                        add_key(L, keyState, key, 1, len);
                    }
                }
            }
            // the mate's values (lanes r and r ^ 1: CHUNK and TB are even, so a valid lane's mate is valid and in this wavefront)
            const int mate = A.V.paired ? (int)(threadIdx.x & 1) : 0;
            u64 po = __shfl_xor(p, 1, 64), oo = __shfl_xor(o, 1, 64);
            int mso = __shfl_xor(mapScore, 1, 64), leno = __shfl_xor(len, 1, 64);
            if (!A.V.paired) { po = 0; oo = 0; mso = 0; leno = 0; }
            const u64 p1 = mate ? po : p, s1 = mate ? oo : o, p2 = mate ? p : po, s2 = mate ? o : oo;
            const int ms1 = mate ? mso : mapScore, ms2 = mate ? mapScore : mso;
            // (an unmapped read has empty sets, so getSets' "neither mate is mapped" needs no test of its own)
            const bool amb = (p1 && p2 && p1 != p2) || (p1 && (s1 & ~p1)) || (p2 && (s2 & ~p2));          // :661-663
            u64 prim, ambm = 0;
            if (A.mode == BBMAP_AMBIG2_FIRST || A.mode == BBMAP_AMBIG2_UNSET) prim = (!A.V.paired || ms1 >= ms2) ? p1 : p2;        // :672-677
            else prim = p1 | p2;                                                                    // :678-681
            if (amb) {                                                                              // :684-699
                if (A.mode == BBMAP_AMBIG2_SPLIT) { ambm = prim | s1 | s2; prim = 0; }
                else if (A.mode == BBMAP_AMBIG2_ALL) prim |= s1 | s2;
                else if (A.mode == BBMAP_AMBIG2_TOSS) prim = 0;
            }
            const u64 stat = p1 | p2 | (amb ? s1 | s2 : 0ull);                                      // :725-732
            if (doSet && valid && mate == 0 && stat) {
                const u64 incrR = A.V.paired ? 2 : 1, incrB = (u64)((long long)len + (long long)leno);  // :734-735
                for (u64 m = stat; m; m &= m - 1) {
                    const int s = __builtin_ctzll(m);
                    atomicAdd(&L.set[s * 4 + (amb ? 2 : 0)], incrR);
                    atomicAdd(&L.set[s * 4 + (amb ? 3 : 1)], incrB);
                }
            }
            if (A.recs && valid) {
                bbmap_splitrec out;
                out.primary_mask = prim; out.ambig_mask = ambm;
                out.flags = (amb ? BBMAP_SPLITREC_AMBIG_SETS : 0) | (ambRead ? BBMAP_SPLITREC_AMBIG_READ : 0) | (mapped ? BBMAP_SPLITREC_MAPPED : 0);
                out.key = ownKey; out.stats_mask = stat;
                A.recs[r] = out;
            }
        }
        __syncthreads();
        // every slot and set counter that moved goes to the state once, and is empty for the next chunk
        if (doScaf)
            for (int slot = threadIdx.x; slot < SLOTS; slot += TB) {
                const int k = L.key[slot];
                if (k == EMPTY) continue;
                for (int c = 0; c < 4; c++) {
                    const u64 v = L.sum[slot * 4 + c];
                    if (!v) continue;
                    L.sum[slot * 4 + c] = 0;
                    atomicAdd(keyState + 4ll * k + c, v);
                }
                L.key[slot] = EMPTY;
            }
        if (doSet)
            for (int k = threadIdx.x; k < 4 * A.nsets; k += TB) {
                const u64 v = L.set[k];
                if (!v) continue;
                L.set[k] = 0;
                atomicAdd(setState + k, v);
            }
        __syncthreads();
    }
}

hipError_t launch_assign(const Args &a, hipStream_t stream) {
    if (a.V.n <= 0) return hipSuccess;
    const long long want = (a.V.n + CHUNK - 1) / CHUNK;
    const unsigned blocks = (unsigned)(want < MAX_BLOCKS ? want : MAX_BLOCKS);
    hipLaunchKernelGGL(refsplit_assign_kernel, dim3(blocks), dim3(TB), 0, stream, a);
    return hipGetLastError();
}

// ---- the stream lists
// counts[row * nblocks + block] (PLACE = false), or units placed at offsets[row * nblocks + block] + rank (PLACE = true)
template <bool PLACE>
__global__ __launch_bounds__(LIST_TB) void refsplit_lists_kernel(const bbmap_splitrec *recs, long long units, int paired, int nsets, long long nblocks,
                                                                  int *counts, const long long *offsets, int *out, long long cap) {
    __shared__ int wc[LIST_WAVES][2 * MAX_SETS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rows = 2 * nsets;
    const long long u = (long long)blockIdx.x * LIST_TB + threadIdx.x, r = paired ? 2 * u : u;
    u64 pm = 0, am = 0;
    if (u < units) { pm = recs[r].primary_mask; am = recs[r].ambig_mask; }
    for (int row = 0; row < rows; row++) {
        const bool bit = row < nsets ? (pm >> row) & 1 : (am >> (row - nsets)) & 1;
        const u64 b = __ballot(bit);
        if (lane == 0) wc[wave][row] = popc(b);
    }
    __syncthreads();
    if (!PLACE) {
        for (int row = threadIdx.x; row < rows; row += LIST_TB) {
            int sum = 0;
            for (int w = 0; w < LIST_WAVES; w++) sum += wc[w][row];
            counts[row * nblocks + blockIdx.x] = sum;
        }
        return;
    }
    for (int row = 0; row < rows; row++) {
        const bool bit = row < nsets ? (pm >> row) & 1 : (am >> (row - nsets)) & 1;
        const u64 b = __ballot(bit);
        if (!bit) continue;
        int before = 0;
        for (int w = 0; w < wave; w++) before += wc[w][row];
        const long long pos = offsets[row * nblocks + blockIdx.x] + before + popc(b & lt_mask(lane));
        if (pos < cap) out[pos] = (int)r;
    }
}

__global__ void refsplit_setoff_kernel(const long long *offsets, long long nblocks, int rows, long long *setOff) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= rows) setOff[i] = offsets[(long long)i * nblocks];                 // (entry rows * nblocks is the scan's total)
}

long long list_blocks(long long n, int paired) {
    const long long units = paired ? n / 2 : n;
    return (units + LIST_TB - 1) / LIST_TB;
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

static hipError_t scan_bytes(long long items, size_t *need) {
    auto wide = hipcub::TransformInputIterator<long long, ToLL, const int *>((const int *)nullptr, ToLL());
    *need = 0;
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *need, wide, (long long *)nullptr, (int)items);
}

long long lists_workspace_bytes(long long n, int paired, int nsets) {
    const long long items = 2ll * nsets * list_blocks(n, paired) + 1;
    if (items >= (1ll << 31)) return -1;
    size_t need = 0;
    if (scan_bytes(items, &need) != hipSuccess) return -1;
    return (long long)(align256((size_t)items * 4) + align256((size_t)items * 8) + align256(need) + 256);
}

hipError_t launch_lists(long long n, int paired, int nsets, const bbmap_splitrec *recs, void *ws, long long wsBytes, long long *setOff,
                        int *units, long long unitsCap, hipStream_t stream) {
    const long long nunits = paired ? n / 2 : n, nblocks = list_blocks(n, paired);
    const int rows = 2 * nsets;
    if (rows == 0 || nblocks == 0) return hipMemsetAsync(setOff, 0, 8 * (size_t)(rows + 1), stream);
    const long long items = (long long)rows * nblocks + 1;
    size_t need = 0;
    hipError_t e = scan_bytes(items, &need);
    if (e != hipSuccess) return e;
    char *base = (char *)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    int *counts = (int *)base;
    long long *offsets = (long long *)(base + align256((size_t)items * 4));
    void *tmp = (char *)offsets + align256((size_t)items * 8);
    if ((char *)tmp + need > (char *)ws + wsBytes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(refsplit_lists_kernel<false>, dim3((unsigned)nblocks), dim3(LIST_TB), 0, stream, recs, nunits, paired, nsets, nblocks, counts,
                       (const long long *)nullptr, (int *)nullptr, 0ll);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemsetAsync(counts + items - 1, 0, 4, stream)) != hipSuccess) return e;          // so that the last offset is the total
    auto wide = hipcub::TransformInputIterator<long long, ToLL, const int *>((const int *)counts, ToLL());
    if ((e = hipcub::DeviceScan::ExclusiveSum(tmp, need, wide, offsets, (int)items, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(refsplit_setoff_kernel, dim3((unsigned)((rows + 1 + 127) / 128)), dim3(128), 0, stream, (const long long *)offsets, nblocks, rows, setOff);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (!units || unitsCap <= 0) return hipSuccess;
    hipLaunchKernelGGL(refsplit_lists_kernel<true>, dim3((unsigned)nblocks), dim3(LIST_TB), 0, stream, recs, nunits, paired, nsets, nblocks, (int *)nullptr,
                       (const long long *)offsets, units, unitsCap);
    return hipGetLastError();
}

}  // namespace bbsplit

// ---------------------------------------------------------------------------------------------------------------------- raw C ABI

extern "C" int64_t bbpipe_refsplit_state_bytes(int32_t nkeys, int32_t nsets) {
    if (nkeys < 0 || nsets < 0 || nsets > BBMAP_SPLIT_MAX_SETS) return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_state_bytes: bad argument");
    return 8ll * (BBMAP_SPLIT_STATE_HEAD + 4ll * nkeys + 4ll * nsets);
}

extern "C" int bbpipe_refsplit_add_device(void *stream, int64_t n_reads, int32_t paired, const bbmap_split_config *cfg, const bbidx_read *reads,
                                          const bbmap_final *finals, const bbmap_msite *sites, const int32_t *nsites, int32_t cap_stride,
                                          int32_t nchroms, const int32_t *scaf_off, const int32_t *scaf_loc, int32_t pad, const uint64_t *scaf_sets,
                                          const int32_t *scaf_key, void *state, bbmap_splitrec *records_out) {
    if (!cfg) return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_add_device: null configuration");
    if (n_reads < 0 || (paired && (n_reads & 1)) || cap_stride < 0 || nchroms < 0 || pad < 0) return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_add_device: bad argument");
    if (const char *why = bbsplit::check_config(*cfg)) return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_add_device: %s", why);
    if (n_reads == 0 || cfg->flags == 0) return BBMAP_OK;
    if (!scaf_off || !scaf_loc) return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_add_device: no scaffold table");
    if (!reads || !finals || !nsites || (cap_stride > 0 && !sites) || !scaf_sets || !scaf_key) return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_add_device: null buffer");
    if ((cfg->flags & (BBMAP_SPLIT_SCAF_STATS | BBMAP_SPLIT_SET_STATS)) && !state) return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_add_device: null state");
    if ((cfg->flags & (BBMAP_SPLIT_RECORDS | BBMAP_SPLIT_LISTS)) && !records_out) return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_add_device: null records");
    bbsplit::Args a = {};
    a.V.reads = reads; a.V.fin = finals; a.V.sites = sites; a.V.nsites = nsites; a.V.cap = cap_stride;      // (no tier)
    a.T.off = scaf_off; a.T.loc = scaf_loc; a.T.len = nullptr; a.T.pad = pad; a.T.nchroms = nchroms;
    a.scafSets = (const unsigned long long *)scaf_sets; a.scafKey = scaf_key;
    a.V.n = n_reads; a.V.paired = paired ? 1 : 0;
    a.flags = cfg->flags; a.mode = cfg->ambiguous2; a.clearzone = cfg->clearzone; a.maxSites = cfg->maxSites; a.nsets = cfg->nsets; a.nkeys = cfg->nkeys;
    a.state = (unsigned long long *)state;
    a.recs = cfg->flags & (BBMAP_SPLIT_RECORDS | BBMAP_SPLIT_LISTS) ? records_out : nullptr;
    BBHIP(bbsplit::launch_assign(a, (hipStream_t)stream));
    return BBMAP_OK;
}

extern "C" int64_t bbpipe_refsplit_lists_workspace_bytes(int64_t n_reads, int32_t paired, int32_t nsets) {
    if (n_reads < 0 || (paired && (n_reads & 1)) || nsets < 0 || nsets > BBMAP_SPLIT_MAX_SETS)
        return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_lists_workspace_bytes: bad argument");
    const long long b = bbsplit::lists_workspace_bytes(n_reads, paired ? 1 : 0, nsets);
    if (b < 0) return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_lists_workspace_bytes: the batch is too large for one scan");
    return b;
}

extern "C" int bbpipe_refsplit_lists_device(void *stream, int64_t n_reads, int32_t paired, int32_t nsets, const bbmap_splitrec *records, void *workspace,
                                            int64_t workspace_bytes, int64_t *set_off, int32_t *units, int64_t units_cap) {
    if (n_reads < 0 || (paired && (n_reads & 1)) || nsets < 0 || nsets > BBMAP_SPLIT_MAX_SETS || units_cap < 0)
        return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_lists_device: bad argument");
    if (!set_off || (n_reads > 0 && !records) || (units_cap > 0 && !units)) return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_lists_device: null buffer");
    const long long need = bbsplit::lists_workspace_bytes(n_reads, paired ? 1 : 0, nsets);
    if (need < 0) return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_lists_device: the batch is too large for one scan");
    if (n_reads > 0 && nsets > 0 && (!workspace || workspace_bytes < need))
        return bbfail(BBMAP_E_ARG, "bbpipe_refsplit_lists_device: the workspace is too small (bbpipe_refsplit_lists_workspace_bytes)");
    BBHIP(bbsplit::launch_lists(n_reads, paired ? 1 : 0, nsets, records, workspace, workspace_bytes, (long long *)set_off, units, units_cap, (hipStream_t)stream));
    return BBMAP_OK;
}
