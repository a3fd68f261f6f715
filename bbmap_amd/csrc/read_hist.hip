// Read histograms on the device: align2.ReadStats as BBMap's mapping threads feed it (AbstractMapThread.java:478-482, :523-529).
//   addToMatchHistogram2 (current/align2/ReadStats.java:516-576), addToQualityAccuracy (:336-387), addToErrorHistogram (:395-399,
//   Read.countSubs, current/stream/Read.java:1916-1925), addToIndelHistogram (:472-508), addToIdentityHistogram (:446-452,
//   Read.identityFlat, Read.java:1529-1596), addToQualityHistogram2 and the three loops behind it (:273-328), addToBaseHistogram2
//   (:648-664), addToLengthHistogram (:407-411), addToGCHistogram (:413-438, Read.gc, Read.java:2530-2542).  "Defined" is
//   AminoAcid.baseToNumber[b] >= 0 (current/dna/AminoAcid.java:615-624: A/a C/c G/g T/t U/u -> 0 1 2 3 3, everything else -1).
//
// Nearly every increment of a fixed-length batch lands on the same few hundred addresses (at 2 x 150 bases every read moves the same
// 150 positions), so the kernel is written for contention, not traffic: NO counter that every read moves is updated in HBM once per
// read.  A workgroup counts in its LDS (32-bit counters; read_hist.h has the budget): the per-position arrays for positions below
// TILE, a positions x qualities sub-table of bqualHist, and all of the small histograms.  It takes CHUNK pairs at a time, few enough
// that no 32-bit counter can overflow, and adds every counter that moved to the 64-bit state with one atomic at the chunk's end.
// Positions beyond the tile (long reads, where few reads share an address), qualities beyond the sub-table and the far bins of the
// error / length histograms go to HBM directly.  The two maxima (gcMaxReadLen, idMaxReadLen) are kept in a register per wavefront.
//
// One pair (or single read) per wavefront and turn, every control value wave-uniform.  A read is walked 64 bases per step for the
// histograms that need no string (lane = position, so a wavefront never adds twice to one per-position counter in a step) and its
// string 64 symbols per step (as coverage.hip walks it): the step is a ballot of the D lanes, rpos is the carried base plus the
// popcount below the lane, "first D of a run" is the ballot shifted by one with the last symbol carried across steps.  Every lane
// then knows (rpos, symbol, base, quality) and the match histogram, the quality accuracy, the S count and identity's three counts
// come from that one walk; a minus-strand read walks its string from the far end.  The indel histogram walks the string a second
// time because Java does: without strand reversal and with an rpos that every symbol advances.
#include "read_hist.h"

#include "host_common.h"
#include "wave_prims.h"

namespace bbrh {
using wavep::u64;
using wavep::hibit;
using wavep::lt_mask;
using wavep::popc;
using wavep::uni;

Layout layout_of(int flags) {
    static const long long size[N_ARRAYS] = {2ll * N_MATCH_ARRAYS * MAXLEN, 2ll * MAXLEN, 2ll * MAXLEN * QBINS, 2ll * QBINS, 10ll * MAXPOS,
                                             4ll * ABINS, INS_BINS, DEL_BINS, DEL2_BINS, MAXPOS + 1, MAXPOS + 1, GC_WORDS, ID_WORDS};
    static const int group[N_ARRAYS] = {BBMAP_RH_MATCH, BBMAP_RH_QUALITY, BBMAP_RH_QUALITY, BBMAP_RH_QUALITY, BBMAP_RH_BASE,
                                        BBMAP_RH_ACCURACY, BBMAP_RH_INDEL, BBMAP_RH_INDEL, BBMAP_RH_INDEL, BBMAP_RH_ERROR, BBMAP_RH_LENGTH,
                                        BBMAP_RH_GC, BBMAP_RH_IDENTITY};
    Layout L;
    long long at = 0;
    for (int a = 0; a < N_ARRAYS; a++) {
        L.off[a] = flags & group[a] ? at : -1;
        if (flags & group[a]) at += size[a];
    }
    L.words = at;
    return L;
}

struct Table { Segment seg[N_SEGMENTS]; long long off[N_ARRAYS]; };

static Table table_of(int flags) {
    const Layout L = layout_of(flags);
    Table T;
    for (int a = 0; a < N_ARRAYS; a++) T.off[a] = L.off[a];
    auto flat = [](int lds, int n, long long hbm) { return Segment{lds, 1, n, 1, hbm, 0, 1}; };
    auto plus = [](long long off, long long d) { return off < 0 ? off : off + d; };
    int k = 0;
    T.seg[k++] = Segment{L_MATCH, 2 * N_MATCH_ARRAYS, TILE, 1, L.off[A_MATCH], MAXLEN, 1};
    T.seg[k++] = Segment{L_BASE, 10, TILE, 1, L.off[A_BASE], MAXPOS, 1};
    T.seg[k++] = Segment{L_QLEN, 2, TILE, 1, L.off[A_QLEN], MAXLEN, 1};
    T.seg[k++] = Segment{L_BQUAL, 2, TILE, QTILE, L.off[A_BQUAL], (long long)MAXLEN * QBINS, QBINS};
    T.seg[k++] = flat(L_ACC, 4 * ABINS, L.off[A_ACC]);
    T.seg[k++] = flat(L_INS, INS_BINS, L.off[A_INS]);
    T.seg[k++] = flat(L_DEL, DEL_BINS, L.off[A_DEL]);
    T.seg[k++] = flat(L_DEL2, BBMAP_RH_DEL2_LDS_BINS, L.off[A_DEL2]);
    T.seg[k++] = flat(L_ERR, BBMAP_RH_ERR_LDS_BINS, L.off[A_ERR]);
    T.seg[k++] = flat(L_ID, ID_BINS, L.off[A_ID]);
    T.seg[k++] = flat(L_IDBASE, ID_BINS, plus(L.off[A_ID], ID_BINS));
    T.seg[k++] = flat(L_GC, BBMAP_RH_GC_BINS + 1, L.off[A_GC]);
    T.seg[k++] = flat(L_LEN, BBMAP_RH_LEN_LDS_BINS, L.off[A_LEN]);
    T.seg[k++] = flat(L_QCOUNT, 2 * QBINS, L.off[A_QCOUNT]);
    static_assert(N_SEGMENTS == 14, "one entry per piece of the LDS counters");
    return T;
}

// AminoAcid.baseToNumber
__device__ inline int base_to_number(int b) {
    const int c = b & ~0x20;
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : ((c == 'T') | (c == 'U')) ? 3 : -1;
}

// counter `i` of a histogram whose first ldsBins bins are in LDS
__device__ inline void bump(unsigned *lds, int ldsBins, u64 *hbm, int i, unsigned by = 1) {
    if (i < ldsBins) atomicAdd(lds + i, by); else atomicAdd(hbm + i, (u64)by);
}
// position `pos` of row `row` of a per-position array (rows of `stride` positions in the state, of TILE in LDS)
__device__ inline void bump_pos(unsigned *lds, u64 *hbm, int row, int pos, int stride) {
    if (pos < TILE) atomicAdd(lds + row * TILE + pos, 1u); else atomicAdd(hbm + (long long)row * stride + pos, 1ull);
}

// hist[key]++ for the calling lanes with `active` set (called by the whole wavefront).  A batch whose bases share one quality would
// put all 64 lanes on one LDS address: the lanes that hold the first active lane's key are counted with one ballot and one add by
// that lane, the others add for themselves.
__device__ inline void bump_keyed(unsigned *hist, int key, bool active, int lane) {
    const u64 act = __ballot(active);
    if (!act) return;
    const int first = __builtin_ctzll(act), k0 = wavep::rl(key, first);
    const u64 same = __ballot(active & (key == k0));
    if (lane == first) atomicAdd(hist + k0, (unsigned)popc(same));
    if (active & (key != k0)) atomicAdd(hist + key, 1u);
}

// What the kernel's loops share: the LDS counters, the state's arrays (nullptr = not selected), the two maxima of this wavefront
struct Ctx {
    unsigned *cnt;
    u64 *arr[N_ARRAYS];
    int flags, lane;
    int gcMax, idMax;
};

// The histograms that need no string: base content, the quality tables, the A/T and G/C counts for GC.  Returns Read.gc().
__device__ inline float read_pass(Ctx &X, const uint8_t *bases, const uint8_t *qual, int len, int mate) {
    const bool doBase = X.flags & BBMAP_RH_BASE, doGC = X.flags & BBMAP_RH_GC;
    const bool doQ = ((X.flags & BBMAP_RH_QUALITY) != 0) & (qual != nullptr) & (len >= 1);       // :275
    int at = 0, gc = 0;
    if (doBase | doGC | doQ) for (int base = 0; base < len; base += 64) {
        const int pos = base + X.lane;
        const bool valid = pos < len;
        const int x = base_to_number(valid ? bases[pos] : 0);
        if (doBase & valid) bump_pos(X.cnt + L_BASE, X.arr[A_BASE], mate * 5 + x + 1, pos, MAXPOS);       // :659-663
        if (doGC) {                                                                       // Read.gc :2533-2539
            at += popc(__ballot(valid & ((x == 0) | (x == 3))));
            gc += popc(__ballot(valid & ((x == 1) | (x == 2))));
        }
        if (doQ) {
            const int q = valid ? min((int)qual[pos], QBINS - 1) : 0;
            bump_keyed(X.cnt + L_QCOUNT + mate * QBINS, q, valid, X.lane);                // :325-327, over all bases
            if (valid & (pos < MAXLEN)) {                                                           // :315-319
                if ((pos < TILE) & (q < QTILE)) atomicAdd(X.cnt + L_BQUAL + (mate * TILE + pos) * QTILE + q, 1u);
                else atomicAdd(X.arr[A_BQUAL] + ((long long)mate * MAXLEN + pos) * QBINS + q, 1ull);
            }
        }
    }
    if (X.lane == 0) {
        if (doQ) bump_pos(X.cnt + L_QLEN, X.arr[A_QLEN], mate, min(len, (int)MAXLEN) - 1, MAXLEN);          // :300-303
        if (X.flags & BBMAP_RH_LENGTH) bump(X.cnt + L_LEN, BBMAP_RH_LEN_LDS_BINS, X.arr[A_LEN], max(len, 0));   // :409-410
    }
    if (gc < 1) return 0.f;                                                               // :2540
    return __fdiv_rn(__fmul_rn((float)gc, 1.f), (float)(at + gc));                        // gc*1f/(at+gc)
}

// addToMatchHistogram2's and addToQualityAccuracy's loops over the long-format string, 64 symbols per step, with countSubs and
// identityFlat's counts taken on the way.  `for(mpos=0; mpos<match.length && rpos<limit; mpos++)`: D does not advance rpos, so a
// symbol takes part when the number of non-D symbols in front of it is below the limit -- min(len, MAXLEN) for the match histogram,
// len for the accuracy (the stated deviation; Java has no limit there and throws).
__device__ inline void match_pass(Ctx &X, const uint8_t *m, int ml, bool plus, const uint8_t *bases, const uint8_t *qual, int len, int mate) {
    const bool doMatch = X.flags & BBMAP_RH_MATCH;
    const bool doAcc = ((X.flags & BBMAP_RH_ACCURACY) != 0) & (qual != nullptr);           // :337
    const int limit = min(len, (int)MAXLEN);
    int rbase = 0, subs = 0, good = 0, ns = 0, bad = 0;
    bool lastD = false;                                                                   // lastm == 'D' at the step's first symbol
    for (int base = 0; base < ml; base += 64) {
        const int mpos = base + X.lane;
        const bool valid = mpos < ml;
        const int ch = valid ? m[plus ? mpos : ml - 1 - mpos] : 0;                        // :545 / :350
        const bool isD = ch == 'D';
        const u64 dmask = __ballot(isD), adv = __ballot(valid & !isD);
        const int rpos = rbase + popc(adv & lt_mask(X.lane));
        const bool prevD = X.lane ? (dmask >> (X.lane - 1)) & 1 : lastD;
        const bool inRead = valid & (rpos < len);
        const int b = inRead ? bases[rpos] : 0;
        if (doMatch & valid & (rpos < limit)) {
            int row = -1;
            if (isD) row = prevD ? -1 : M_del;                                            // :547-549 / :564-566: once per run
            else if (b == 'N') row = M_N;                                                 // :546-550
            else row = ch == 'm' ? M_match : ch == 'S' ? M_sub : ch == 'I' ? M_ins : ch == 'C' ? M_clip : M_other;      // :552-570
            if (row >= 0) bump_pos(X.cnt + L_MATCH, X.arr[A_MATCH], row * 2 + mate, rpos, MAXLEN);
        }
        if (doAcc) {
            unsigned *acc = X.cnt + L_ACC;
            const int q = inRead ? min((int)qual[rpos], ABINS - 1) : 0;
            bump_keyed(acc + Q_match * ABINS, q, inRead & (ch == 'm'), X.lane);           // :353-354
            const bool defined = base_to_number(b) >= 0;
            if (!inRead | (ch == 'm')) {}
            else if (ch == 'S') atomicAdd(acc + Q_sub * ABINS + q, 1u);                   // :355-356
            else if ((ch == 'I') & defined) atomicAdd(acc + Q_ins * ABINS + q, 1u);       // :357-358
            else if (isD & !prevD) {                                                      // :363-376
                const int before = max(rpos - 1, 0);
                if (defined) atomicAdd(acc + Q_del * ABINS + q, 1u);
                if ((rpos >= 1) & (base_to_number(bases[before]) >= 0)) atomicAdd(acc + Q_del * ABINS + min((int)qual[before], ABINS - 1), 1u);
            }
        }
        const bool isM = ch == 'm', isN = (ch == 'N') | (ch == 'R');
        subs += popc(__ballot(ch == 'S'));                                                // countSubs
        good += popc(__ballot(isM));                                                      // identityFlat :1547-1561
        ns += popc(__ballot(isN));
        bad += popc(__ballot(valid & !isM & !isN & (ch != 'C')));
        lastD = (dmask >> 63) & 1;
        rbase += popc(adv);
    }
    if (X.lane == 0) {
        if (X.flags & BBMAP_RH_ERROR) bump(X.cnt + L_ERR, BBMAP_RH_ERR_LDS_BINS, X.arr[A_ERR], min(subs, (int)MAXPOS));       // :397-398
        if (X.flags & BBMAP_RH_IDENTITY) {
            const int n = (ns + 3) / 4;                                                   // :1586-1589
            good += n; bad += 3 * n;
            const float id = __fdiv_rn((float)good, (float)max(good + bad, 1));
            const int bin = (int)__fmul_rn(id, (float)BBMAP_RH_ID_BINS);                  // :449
            atomicAdd(X.cnt + L_ID + bin, 1u);
            atomicAdd(X.cnt + L_IDBASE + bin, (unsigned)len);                             // :450
        }
    }
    if (X.flags & BBMAP_RH_IDENTITY) X.idMax = max(X.idMax, len);                         // :451
}

// a run of `streak` equal symbols has ended (:485-492)
__device__ inline void indel_run(Ctx &X, int sym, int streak) {
    if (sym == 'D') {
        const int s = min(streak, (int)BBMAP_RH_MAXDELLEN2);
        if (s < BBMAP_RH_MAXDELLEN) atomicAdd(X.cnt + L_DEL + s, 1u);
        bump(X.cnt + L_DEL2, BBMAP_RH_DEL2_LDS_BINS, X.arr[A_DEL2], s / 100);
    } else if (sym == 'I') atomicAdd(X.cnt + L_INS + min(streak, (int)BBMAP_RH_MAXINSLEN), 1u);
}

// addToIndelHistogram's loop (:480-507): match[mpos] as it lies, rpos advances on every symbol, so the first min(len, MAXLEN)
// symbols are examined and a run is cut there.  A lane whose symbol differs from the one before it closes that one's run; the
// run's first symbol is the nearest such lane below, or lies `carry` symbols back in an earlier step.
__device__ inline void indel_pass(Ctx &X, const uint8_t *m, int ml, int len) {
    const int nsym = min(ml, min(len, (int)MAXLEN));
    int carry = 0, lastCh = 'A';
    for (int base = 0; base < nsym; base += 64) {
        const int mpos = base + X.lane, nvalid = min(64, nsym - base);
        const bool valid = mpos < nsym;
        const int ch = valid ? m[mpos] : 0;
        int prev = __shfl_up(ch, 1, 64);
        prev = X.lane ? prev : lastCh;
        const u64 starts = __ballot(valid & (ch != prev));
        if ((starts >> X.lane) & 1) {
            const u64 below = starts & lt_mask(X.lane);
            indel_run(X, prev, below ? X.lane - hibit(below) : carry + X.lane);
        }
        carry = starts ? nvalid - hibit(starts) : carry + nvalid;
        lastCh = wavep::rl(ch, nvalid - 1);
    }
    if (X.lane == 0) indel_run(X, lastCh, carry);                                         // :500-507
}

__global__ __launch_bounds__(TB) void read_hist_add_kernel(const Args A, const Table T) {
    __shared__ unsigned cnt[L_TOTAL];
    Ctx X;
    X.cnt = cnt; X.flags = A.flags; X.lane = threadIdx.x & 63; X.gcMax = 0; X.idMax = 0;
    for (int a = 0; a < N_ARRAYS; a++) X.arr[a] = T.off[a] >= 0 ? A.state + T.off[a] : nullptr;
    const int wid = uni((int)(threadIdx.x >> 6));
    for (int k = threadIdx.x; k < L_TOTAL; k += TB) cnt[k] = 0;
    __syncthreads();
    const long long units = A.V.paired ? A.V.n / 2 : A.V.n;
    const int mates = A.V.paired ? 2 : 1;
    const int needString = BBMAP_RH_MATCH | BBMAP_RH_ACCURACY | BBMAP_RH_ERROR | BBMAP_RH_IDENTITY | BBMAP_RH_INDEL;
    for (long long chunk = blockIdx.x; chunk * CHUNK < units; chunk += gridDim.x) {
        const long long end = min(units, (chunk + 1) * CHUNK);
        for (long long u = chunk * CHUNK + wid; u < end; u += WAVES_PER_BLOCK) {
            float gcOf[2] = {-1.f, -1.f};
            int lenOf[2] = {0, 0};
            for (int mate = 0; mate < mates; mate++) {
                const long long r = u * mates + mate;
                const bbidx_read rd = A.V.reads[r];
                const int len = uni(min(max(rd.len, 0), (int)MAXPOS));
                const uint8_t *bases = A.V.bases + rd.bases_off, *qual = A.qual ? A.qual + rd.bases_off : nullptr;
                const float gc = read_pass(X, bases, qual, len, mate);
                lenOf[mate] = len;
                gcOf[mate] = len > 0 ? gc : -1.f;                                         // :418-419
                if (!(A.flags & needString) || len < 1) continue;
                const ReadRec R = record_of<TierRule::ByList>(A.V, r);
                const int ml = uni(R.ml);
                if (!uni(R.f->mapped) || ml < 1) continue;
                if (A.flags & (needString & ~BBMAP_RH_INDEL)) match_pass(X, R.m, ml, uni(R.f->strand) == 0, bases, qual, len, mate);
                if (A.flags & BBMAP_RH_INDEL) indel_pass(X, R.m, ml, len);
            }
            if ((A.flags & BBMAP_RH_GC) && X.lane == 0) {                                 // addToGCHistogram :413-438, usePairGC
                const int total = lenOf[0] + lenOf[1];
                float gc = gcOf[0];
                if (mates == 2)                                                           // (gc1*len1+gc2*len2)/(len1+len2), left to right, no FMA
                    gc = __fdiv_rn(__fadd_rn(__fmul_rn(gcOf[0], (float)lenOf[0]), __fmul_rn(gcOf[1], (float)lenOf[1])), (float)total);
                if (!(gc < 0.f) && total >= 1) {                                          // :435
                    atomicAdd(cnt + L_GC + min((int)BBMAP_RH_GC_BINS, (int)__fmul_rn(gc, (float)(BBMAP_RH_GC_BINS + 1))), 1u);
                    X.gcMax = max(X.gcMax, total);
                }
            }
        }
        __syncthreads();
        // every counter that moved goes to the state once, and is zero for the next chunk
        for (int s = 0; s < N_SEGMENTS; s++) {
            const Segment g = T.seg[s];
            if (g.hbm < 0) continue;
            const int n = g.n0 * g.n1 * g.n2;
            for (int k = threadIdx.x; k < n; k += TB) {
                const unsigned v = cnt[g.lds + k];
                if (!v) continue;
                cnt[g.lds + k] = 0;
                const int i2 = k % g.n2, t = k / g.n2, i1 = t % g.n1, i0 = t / g.n1;
                atomicAdd(A.state + g.hbm + i0 * g.s0 + i1 * g.s1 + i2, (u64)v);
            }
        }
        __syncthreads();
    }
    // the two maxima: one atomic per wavefront that has something to say
    X.gcMax = uni(__shfl(X.gcMax, 0, 64));
    if (X.lane == 0) {
        if (X.gcMax > 0 && X.arr[A_GC]) atomicMax(X.arr[A_GC] + BBMAP_RH_GC_BINS + 1, (u64)X.gcMax);
        if (X.idMax > 0 && X.arr[A_ID]) atomicMax(X.arr[A_ID] + 2 * ID_BINS, (u64)X.idMax);
    }
}

hipError_t launch_add(const Args &a, hipStream_t stream) {
    const long long units = a.V.paired ? a.V.n / 2 : a.V.n;
    if (units <= 0) return hipSuccess;
    const long long want = (units + CHUNK - 1) / CHUNK;
    const unsigned blocks = (unsigned)(want < MAX_BLOCKS ? want : MAX_BLOCKS);
    hipLaunchKernelGGL(read_hist_add_kernel, dim3(blocks), dim3(TB), 0, stream, a, table_of(a.flags));
    return hipGetLastError();
}

}  // namespace bbrh

// ---------------------------------------------------------------------------------------------------------------------- raw C ABI

extern "C" int64_t bbpipe_read_hist_bytes(int32_t flags) {
    if (flags & ~BBMAP_RH_ALL) return bbfail(BBMAP_E_ARG, "bbpipe_read_hist_bytes: unknown flag bits");
    return 8 * bbrh::layout_of(flags).words;
}

extern "C" int bbpipe_read_hist_view(int32_t flags, const void *state, bbmap_readhist_view *out) {
    if (!out) return bbfail(BBMAP_E_ARG, "bbpipe_read_hist_view: null argument");
    if (flags & ~BBMAP_RH_ALL) return bbfail(BBMAP_E_ARG, "bbpipe_read_hist_view: unknown flag bits");
    const bbrh::Layout L = bbrh::layout_of(flags);
    const int64_t *base = (const int64_t *)state;
    auto at = [&](int a) { return L.off[a] < 0 ? (const int64_t *)nullptr : base + L.off[a]; };
    *out = bbmap_readhist_view{};
    out->flags = flags; out->words = L.words; out->state = base;
    out->match = at(bbrh::A_MATCH); out->qual_length = at(bbrh::A_QLEN); out->bqual = at(bbrh::A_BQUAL); out->qcount = at(bbrh::A_QCOUNT);
    out->base = at(bbrh::A_BASE); out->accuracy = at(bbrh::A_ACC); out->ins = at(bbrh::A_INS); out->del = at(bbrh::A_DEL);
    out->del2 = at(bbrh::A_DEL2); out->error = at(bbrh::A_ERR); out->length = at(bbrh::A_LEN); out->gc = at(bbrh::A_GC);
    out->identity = at(bbrh::A_ID);
    return BBMAP_OK;
}

extern "C" int bbpipe_read_hist_add_device(void *stream, int64_t n_reads, int32_t paired, int32_t flags, const bbidx_read *reads,
                                           const uint8_t *bases, const uint8_t *quality, const bbmap_final *finals, const uint8_t *pool,
                                           void *state) {
    if (n_reads < 0 || (paired && (n_reads & 1))) return bbfail(BBMAP_E_ARG, "bbpipe_read_hist_add_device: bad argument");
    if (flags & ~BBMAP_RH_ALL) return bbfail(BBMAP_E_ARG, "bbpipe_read_hist_add_device: unknown flag bits");
    if (n_reads == 0 || flags == 0) return BBMAP_OK;
    if (!reads || !bases || !finals || !pool || !state) return bbfail(BBMAP_E_ARG, "bbpipe_read_hist_add_device: null buffer");
    bbrh::Args a = {};
    a.V.reads = reads; a.V.bases = bases; a.V.fin = finals; a.V.pool = pool;      // (no tier)
    a.qual = quality;
    a.V.n = n_reads; a.V.paired = paired ? 1 : 0; a.flags = flags;
    a.state = (unsigned long long *)state;
    BBHIP(bbrh::launch_add(a, (hipStream_t)stream));
    return BBMAP_OK;
}
