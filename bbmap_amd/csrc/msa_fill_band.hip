// Band path of the MultiStateAligner11ts DP for gfx950: ONE JOB OVER Q LANES, a band of B = 4 * Q diagonals in registers, TWO JOBS
// PER LANE GROUP.
//
// Why: fillLimitedX (jni/MultiStateAligner11tsJNI.c:361-704) only visits the columns of a row between the first "good" column of
// the row above and one past the last good one.  With a tight minScore that window follows one diagonal; the wavefront kernel
// (msa_fill_fast.hip) sweeps the whole rectangle whatever the window is.  This kernel walks a band of B diagonals only:
//   * position i of the band at row r is column r + D0 + i, D0 = (columns - rows) / 2 - B / 2.  Lane q of a job's group owns
//     positions 4q .. 4q+3 and keeps their three planes of the previous row in 12 registers, updated in place left to right (cell i
//     reads old[i] = diagonal, old[i+1] = up, new[i-1] = left);
//   * lane q computes row r at turn T = 2r + q.  Its left neighbour's cell (position 4q-1, row r) was finished by lane q-1 at T-1,
//     its upper neighbour's (position 4q+4, row r-1) by lane q+1 at T-1: one DPP move each (wave_shr:1 / wave_shl:1);
//   * with one job a lane would be busy every other turn.  So a group carries two jobs, A and B, in two register sets X and Y:
//     X holds A on even lanes and B on odd lanes, Y the other one.  Every lane works on X in the even turns and on Y in the odd
//     turns; the neighbours worked on the same job, in their other set, the turn before.  The two turn bodies stand one after the
//     other in the loop: no divergence, no register swap, no idle half;
//   * a wave is 64 / Q groups x 2 = 16 jobs (Q = 8), four cells per lane and turn, 2 * (rows + Q / 2) turns;
//   * the cell is cell_update<Scheme11ts, false, LdsPen> (msa_cell.h), the tables are the wavefront kernel's, one copy per block;
//   * read bases and the rows + B reference bytes the band can touch sit in LDS per job; horizLimit has the closed form
//     minScore - (MATCH + (columns-1-col) * MATCH2), valid when every base of the window is defined -- other jobs are handed on;
//   * per lane and row one dword goes to a scratch slot: four 4-bit traceback records and the four "good" bits.  The row extents
//     (-> iterations, the null cases), the last row's best cell and the walk over the records are then done by the job's Q lanes
//     together, the walk as the wavefront kernel does it (a diagonal run of Q cells per step).
// Exactness: a cell is active iff the row above has a good cell at or before its column -- known from the
// lane's own cells of that row, the prefix flag that came with the left neighbour's cell then, and the good bit that comes with
// the upper neighbour's cell.  A job stays here only if no row has a good cell at position 0 or at position B-1 (unless that is
// the last column), and row 1 -- which visits every column -- has none outside the band; then no cell outside the band is ever
// good, every value inside it is the reference's, and everything else is handed to the wavefront kernel through `fast_list`.
#include "msa_common.h"
#include "msa_cell.h"

namespace bbmsa {

namespace {

// value of lane-1 (DPP wave_shr:1) / of lane+1 (DPP wave_shl:1); lanes with no source keep `fill`
__device__ __forceinline__ int from_left(int x, int fill) { return __builtin_amdgcn_update_dpp(fill, x, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int from_right(int x, int fill) { return __builtin_amdgcn_update_dpp(fill, x, 0x130, 0xf, 0xf, false); }

__device__ __forceinline__ unsigned ld_coherent(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned ld_coherent(const uint8_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// what a lane keeps of ONE job between its turns
struct BandSet {
    int M[4], D[4], I[4];        // the lane's four positions: row r-1 before the turn, row r after it
    int rows, columns;           // rows == 0: no job
    int c0off;                   // column of the lane's first position at row r = r + c0off
    int minScoreOff, vs;         // vs: base costs of the read from the current row on (vertLimit = minScoreOff - vs)
    unsigned w;                  // reference bytes of the four positions (byte i = position i), slides one column per row
    int gprev;                   // the row above has a good cell left of the lane's positions
    int gmask, mprev;            // good bits / match bits of the lane's cells of the row above (bit i = position i)
    int gpass;                   // gprev | own good cells of the row just done: the next lane's gprev
    int bail;                    // a good cell at an edge of the band
    int rdOff, rfOff;            // LDS byte offsets: read bases (index row-1), reference bytes (index col - D0)
    int slot;                    // 0 = job A, 1 = job B of the group
};

}  // namespace

#ifndef BBMSA_BAND_OCC
#define BBMSA_BAND_OCC 4
#endif

template <int Q>
__global__ __launch_bounds__(256, BBMSA_BAND_OCC) void msa_fill_band_kernel(const NarrowParams p) {
    constexpr int B = 4 * Q;                 // diagonals
    constexpr int GROUPS = 64 / Q;           // lane groups per wave
    constexpr int JOBS = 2 * GROUPS;         // jobs per wave
    static_assert(Q == 4 || Q == 8 || Q == 16, "a group is a power of two of lanes, its good bits fit 64");
    extern __shared__ int lds[];
    const int TL = p.tableLen;
    int *delC = lds, *insC = lds + TL, *delExt = lds + 2 * TL, *insExt = delExt + 128;
    int4 *mTab = reinterpret_cast<int4 *>(delExt + 192);
    LdsPen pen; pen.delC = delC; pen.insC = insC; pen.delExt = delExt; pen.insExt = insExt; pen.mTab = mTab;
    for (int i = threadIdx.x; i < TL; i += blockDim.x) { delC[i] = calc_del_off(i); insC[i] = calc_ins_cum_off(i); }
    for (int i = threadIdx.x; i < 128; i += blockDim.x) delExt[i] = SpelledPen<Scheme11ts>().del_ext(i);
    if (threadIdx.x < 32) insExt[threadIdx.x] = SpelledPen<Scheme11ts>().ins_ext(threadIdx.x);
    if (threadIdx.x < 32) {                  // index = min(streak, 5) | match << 3 | prevMatch << 4 (msa_cell.h)
        const int st = threadIdx.x & 7, mt = (threadIdx.x >> 3) & 1, pv = threadIdx.x >> 4;
        const MEntry e = SpelledPen<Scheme11ts>().m_entry(min(st, 5), 0, 0, pv != 0, mt != 0);
        int4 v; v.x = e.addA; v.y = e.bonus; v.z = e.t3sub; v.w = 0;
        mTab[threadIdx.x] = v;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane & (Q - 1), grp = lane / Q, groupBase = grp * Q;
    const int RB = (p.bandRows + 4 + 3) & ~3, FB = (p.bandRows + B + 4 + 3) & ~3;      // bytes per job: read, reference
    uint8_t *jobLds = reinterpret_cast<uint8_t *>(lds + lds_table_ints(TL)) + (long long)wave * JOBS * (RB + FB);
    unsigned *dir = p.dirbuf32 + ((long long)blockIdx.x * 4 + wave) * (long long)(p.bandRows + 1) * 128;   // [(row * 2 + slot) * 64 + lane]
    // with a list (the width sort's candidates, msa_sort.hip) the queue runs over the list's entries; without one over every job
    const long long NJ = p.list ? (long long)ld_coherent(p.list_count) : job_count(p.njobs, p.njobs_dev);
    unsigned nDone = 0, nLeft = 0;

    for (;;) {
        // ------------------------------------------------------------------ one candidate job per slot (lanes 0 .. JOBS-1 pull them)
        long long myJ = -1;
        if (lane < JOBS) {
            for (;;) {
                const long long e_ = (long long)atomicAdd(p.queue, 1u);
                if (e_ >= NJ || e_ >= p.njobs) break;
                const long long t_ = p.list ? (long long)p.list[e_] : e_;
                const bbmsa_job t = p.jobs[t_];
                int ta = t.refStartLoc, tb = t.refEndLoc;
                if (t.flags & BBMSA_CLAMP_WINDOW) {
                    ta = max(0, ta); tb = min(t.ref_len - 1, tb);
                    if (tb - ta >= p.maxColumns) tb = min(t.ref_len - 1, ta + p.maxColumns - 1);
                }
                // (msa_common.h: the rule the width sort uses to make the list, so every entry of a list passes it)
                if (band_is_candidate(t.flags, t.minScore, t.read_len, tb - ta + 1, p.maxRows, p.maxColumns, p.bandRows, p.maxSlack)) { myJ = t_; break; }
                const unsigned k = atomicAdd(p.fast_count, 1u);
                p.fast_list[k] = (int)t_;
            }
        }
        if (!__any(myJ >= 0)) break;

        // ------------------------------------------------------------------ job setup, the group's two jobs one after the other
        BandSet S[2];                                                 // [0] = X (even turns), [1] = Y (odd turns)
        long long jobJ[2]; bool jobOk[2];
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const long long j = __shfl(myJ, grp * 2 + s, 64);
            jobJ[s] = j;
            bbmsa_job jb;
            jb.read_off = 0; jb.ref_off = 0; jb.read_len = 0; jb.ref_len = 0; jb.refStartLoc = 0; jb.refEndLoc = -1; jb.minScore = 0; jb.flags = 0;
            if (j >= 0) jb = p.jobs[j];
            int a = jb.refStartLoc, b = jb.refEndLoc;
            if (jb.flags & BBMSA_CLAMP_WINDOW) {
                a = max(0, a); b = min(jb.ref_len - 1, b);
                if (b - a >= p.maxColumns) b = min(jb.ref_len - 1, a + p.maxColumns - 1);
            }
            const int rows = jb.read_len, columns = b - a + 1;
            int minScore = jb.minScore;
            if ((jb.flags & BBMSA_MODE_MASK) == BBMSA_FILL_LIMITED) minScore -= 120;
            const int D0 = (columns - rows) / 2 - B / 2;
            const uint8_t *rd = p.reads + jb.read_off, *rf = p.refs + jb.ref_off + a;
            const int rdOff = (grp * 2 + s) * (RB + FB), rfOff = rdOff + RB;
            // read bases, reference bytes by column (column 0 holds '!', jni/...c:463; off the matrix: 0), base costs, all defined?
            int cost = 0; bool allDef = true;
#pragma unroll 4
            for (int i = q; i < rows; i += Q) {
                const int cb = rd[i];
                jobLds[rdOff + i] = (uint8_t)cb;
                if (fully_defined(cb)) cost += (i + 1 < rows && fully_defined(rd[i + 1])) ? P_MATCH2 : P_MATCH;
            }
            if (j >= 0)
#pragma unroll 4
            for (int k = q; k < rows + B + 1; k += Q) {
                const int col = k + D0;
                int v = 0;
                if (col == 0) v = '!';
                else if (col >= 1 && col <= columns) { v = rf[col - 1]; allDef = allDef && fully_defined(v); }
                jobLds[rfOff + k] = (uint8_t)v;
            }
            for (int c = 1 + q; c <= columns; c += Q) if (c < 1 + D0 || c > D0 + B) allDef = allDef && fully_defined(rf[c - 1]);
            int nd = allDef ? 0 : 1;
            for (int d = 1; d < Q; d <<= 1) { cost += __shfl_xor(cost, d, 64); nd |= __shfl_xor(nd, d, 64); }
            bool ok = j >= 0 && nd == 0;

            const int minScoreOff = minScore * 2048;
            const int floorv = minScoreOff - ((rows - 1) * P_MATCH2 + P_MATCH);
            const int subfloor = floorv - 5 * P_MATCH2;
            // row 1 visits every column: the ones outside the band must hold no good cell (no left dependency: deletions are barred in rows < 3)
            if (ok) {
                const int cl1 = rd[0];
                const int c0cost = fully_defined(cl1) ? ((rows > 1 && fully_defined(rd[1])) ? P_MATCH2 : P_MATCH) : 0;
                const int vlimP = max(minScoreOff - (cost - c0cost), floorv) + 2048;
                int outGood = 0;
                for (int c = 1 + q; c <= columns; c += Q) {
                    if (c >= 1 + D0 && c <= D0 + B) continue;
                    const int ref1 = rf[c - 1];
                    const int hs = c <= columns - 1 ? P_MATCH + (columns - 1 - c) * P_MATCH2 : 0;
                    CellIn ci;
                    ci.row = 1; ci.c = c; ci.rows = rows; ci.insNeededBase = (columns - c) + 1;
                    ci.cl1 = cl1; ci.ref1 = ref1; ci.refN = false; ci.gap = false; ci.match = cl1 == ref1; ci.act = true;
                    ci.refPen = 0; ci.limitP = max(vlimP, max(minScoreOff - hs, floorv) + 2048); ci.floorP = floorv + 2048; ci.subfloor = subfloor;
                    ci.dgM = 0; ci.dgD = 0; ci.dgI = 0;
                    ci.lM = c == 1 ? insC[1] : subfloor; ci.lD = ci.lM; ci.upM = 0; ci.upI = 0;
                    ci.delForce = INT_MAX;
                    ci.insForce = (c > 1 || (1 > rows - 2 && c < columns - 1)) ? INT_MAX : INT_MIN;
                    ci.pm8 = 0;
                    const CellOut co = cell_update<Scheme11ts, false>(pen, ci);
                    outGood |= (co.goodM | co.goodD | co.goodI) ? 1 : 0;
                }
                for (int d = 1; d < Q; d <<= 1) outGood |= __shfl_xor(outGood, d, 64);
                if (outGood) ok = false;
            }
            if (j >= 0 && !ok && q == 0) { const unsigned k = atomicAdd(p.fast_count, 1u); p.fast_list[k] = (int)j; nLeft++; }
            jobOk[s] = ok;

            // this job lives in set X on even lanes when it is job A, on odd lanes when it is job B -- in set Y otherwise
            const int set = (q & 1) ^ s;
#pragma unroll
            for (int x = 0; x < 2; x++) if (x == set) {
                BandSet &T = S[x];
                for (int i = 0; i < 4; i++) { T.M[i] = 0; T.D[i] = 0; T.I[i] = 0; }      // row 0 is all zero
                T.rows = ok ? rows : 0; T.columns = columns; T.c0off = D0 + 4 * q;
                T.minScoreOff = minScoreOff; T.vs = cost;
                T.w = 0; T.gprev = 1; T.gmask = 0; T.mprev = 0; T.gpass = 0; T.bail = 0;    // row 1's window is [1, columns]
                T.rdOff = rdOff; T.rfOff = rfOff; T.slot = s;
            }
        }
        // (the selects above are per lane: set x of this lane took the job with (q & 1) ^ s == x)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int x = 0; x < 2; x++) {                                  // reference bytes of row 1's positions 0..2 in bytes 1..3
            BandSet &T = S[x];
            if (T.rows > 0) for (int i = 0; i < 3; i++) T.w |= (unsigned)jobLds[T.rfOff + 1 + 4 * q + i] << (8 * (i + 1));
        }
        int maxRowsWave = max(S[0].rows, S[1].rows);
        for (int d = 32; d >= 1; d >>= 1) maxRowsWave = max(maxRowsWave, __shfl_xor(maxRowsWave, d, 64));

        // ------------------------------------------------------------------ fill: iteration k is turn 2k on set X, turn 2k+1 on set Y
        const int rowLagX = (q + 1) >> 1, rowLagY = q >> 1;           // lane q computes row k - lag of the set's job
        for (int k = 1; k <= maxRowsWave + Q / 2; k++) {
#pragma unroll
            for (int x = 0; x < 2; x++) {
                BandSet &T = S[x];
                const BandSet &O = S[1 - x];                           // where the neighbours left this job's cells the turn before
                const int row = k - (x == 0 ? rowLagX : rowLagY);
                // left neighbour: its last position of this row and the good prefix; upper neighbour: its first position of the row above
                int lM = from_left(O.M[3], 0), lD = from_left(O.D[3], 0), gIn = from_left(O.gpass, 0);
                int uM = from_right(O.M[0], 0), uI = from_right(O.I[0], 0), uG = from_right(O.gmask, 0);
                const bool rowAct = row >= 1 && row <= T.rows;
                if (rowAct) {
                    const int rows = T.rows, columns = T.columns;
                    const int floorv = T.minScoreOff - ((rows - 1) * P_MATCH2 + P_MATCH);
                    const int subfloor = floorv - 5 * P_MATCH2, floorP = floorv + 2048;
                    if (q == 0) { lM = subfloor; lD = subfloor; gIn = 0; }
                    if (q == Q - 1) { uM = row == 1 ? 0 : subfloor; uI = uM; uG = 0; }
                    const int cl1 = jobLds[T.rdOff + row - 1];
                    const int clN = row < rows ? jobLds[T.rdOff + row] : 0;
                    T.vs -= fully_defined(cl1) ? (fully_defined(clN) ? P_MATCH2 : P_MATCH) : 0;
                    const int vlimP = max(T.minScoreOff - T.vs, floorv) + 2048;
                    T.w = (T.w >> 8) | ((unsigned)jobLds[T.rfOff + row + 4 * q + 3] << 24);
                    const int c0 = row + T.c0off;
                    const int insRow = insC[row], insPrev = insC[row - 1];
                    const int delForce = (row < 3 || row > rows - 3) ? INT_MAX : INT_MIN;
                    const unsigned g5 = (unsigned)T.gmask | (((unsigned)uG & 1u) << 4);      // good bits of the row above, positions 4q .. 4q+4
                    const bool rowOne = row == 1;
                    unsigned goods = 0, mbits = 0, word = 0;
                    int leftM = lM, leftD = lD;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int c = c0 + i;
                        const int ref1 = (int)((T.w >> (8 * i)) & 255u);
                        const bool inRange = (c >= 1) & (c <= columns);
                        const bool started = (T.gprev != 0) | ((g5 & ((4u << i) - 1u)) != 0u);
                        const bool first = c == 1;
                        const int hs = c <= columns - 1 ? P_MATCH + (columns - 1 - c) * P_MATCH2 : 0;
                        CellIn ci;
                        ci.row = row; ci.c = c; ci.rows = rows; ci.insNeededBase = (columns - c) + 1;
                        ci.cl1 = cl1; ci.ref1 = ref1; ci.refN = false; ci.gap = false; ci.match = cl1 == ref1; ci.act = inRange & started;
                        ci.refPen = 0; ci.limitP = max(vlimP, max(T.minScoreOff - hs, floorv) + 2048); ci.floorP = floorP; ci.subfloor = subfloor;
                        ci.dgM = first ? insPrev : T.M[i]; ci.dgD = first ? insPrev : T.D[i]; ci.dgI = first ? insPrev : T.I[i];
                        ci.lM = first ? insRow : leftM; ci.lD = first ? insRow : leftD;
                        ci.upM = i < 3 ? T.M[i + 1] : uM; ci.upI = i < 3 ? T.I[i + 1] : uI;
                        ci.delForce = delForce;
                        ci.insForce = ((rowOne & (c > 1)) | ((row > rows - 2) & (c < columns - 1))) ? INT_MAX : INT_MIN;
                        ci.pm8 = ((T.mprev >> i) & 1) ? 8 : 0;
                        const CellOut co = cell_update<Scheme11ts, false>(pen, ci);
                        const bool good = co.goodM | co.goodD | co.goodI;
                        goods |= good ? (1u << i) : 0u;
                        mbits |= ci.match ? (1u << i) : 0u;
                        word |= co.nib << (4 * i);
                        T.M[i] = co.nM; T.D[i] = co.nD; T.I[i] = co.nI;
                        leftM = co.nM; leftD = co.nD;
                    }
                    // a good cell at an edge of the band (the last column is an edge of the matrix: nothing lies beyond it)
                    if (q == 0 && (goods & 1u) && c0 >= 1) T.bail = 1;
                    if (q == Q - 1 && (goods & 8u) && c0 + 3 < columns) T.bail = 1;
                    T.gprev = gIn; T.gmask = (int)goods; T.mprev = (int)mbits; T.gpass = (gIn | (goods ? 1 : 0));
                    dir[((long long)row * 2 + T.slot) * 64 + lane] = word | (goods << 16);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the records are written before anyone reads them
        __builtin_amdgcn_wave_barrier();

        // ------------------------------------------------------------------ per job, its Q lanes together: extents, result[], the walk
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const long long j = jobJ[s];
            const int set = (q & 1) ^ s;
            int lastM[4], lastD[4], lastI[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { lastM[i] = set ? S[1].M[i] : S[0].M[i]; lastD[i] = set ? S[1].D[i] : S[0].D[i]; lastI[i] = set ? S[1].I[i] : S[0].I[i]; }
            int bail = set ? S[1].bail : S[0].bail;
            for (int d = 1; d < Q; d <<= 1) bail |= __shfl_xor(bail, d, 64);
            const bool live = jobOk[s];                                // group-uniform
            if (live && bail) { if (q == 0) { const unsigned k = atomicAdd(p.fast_count, 1u); p.fast_list[k] = (int)j; nLeft++; } }
            if (!(live && !bail)) continue;

            const bbmsa_job jb = p.jobs[j];
            int a = jb.refStartLoc, b = jb.refEndLoc;
            if (jb.flags & BBMSA_CLAMP_WINDOW) {
                a = max(0, a); b = min(jb.ref_len - 1, b);
                if (b - a >= p.maxColumns) b = min(jb.ref_len - 1, a + p.maxColumns - 1);
            }
            const int rows = jb.read_len, columns = b - a + 1, mode = jb.flags & BBMSA_MODE_MASK;
            const int minScoreOff = (mode == BBMSA_FILL_LIMITED ? jb.minScore - 120 : jb.minScore) * 2048;
            const int subfloor = minScoreOff - ((rows - 1) * P_MATCH2 + P_MATCH) - 5 * P_MATCH2;
            const int D0 = (columns - rows) / 2 - B / 2;
            const uint8_t *rdL = jobLds + (grp * 2 + s) * (RB + FB), *rfL = rdL + RB;      // rfL[col - D0]
            const unsigned *jdir = dir + s * 64 + groupBase;           // record dword of (row, lane q'): jdir[row * 128 + q']

            // row extents -> iterations, the null cases (jni/...c:441-449, :660-661; the formula of msa_fill_fast.hip).  Lane q takes
            // rows q*per+1 .. (q+1)*per.  A row is entered iff the row above has a good cell, so the entered rows are a prefix.
            const int per = (rows + Q - 1) / Q;
            const int rFirst = q * per + 1, rLast = min(rows, (q + 1) * per);
            int iters = 0, lastColStart = 1, lastHasGood = 0, lastEntered = 0;
            {
                unsigned long long pg = 0;
                if (rFirst > 1 && rFirst <= rLast) for (int l = 0; l < Q; l++) pg |= (unsigned long long)((ld_coherent(jdir + (long long)(rFirst - 1) * 128 + l) >> 16) & 15u) << (4 * l);
                for (int r = rFirst; r <= rLast; r++) {
                    unsigned long long g = 0;
                    for (int l = 0; l < Q; l++) g |= (unsigned long long)((ld_coherent(jdir + (long long)r * 128 + l) >> 16) & 15u) << (4 * l);
                    const bool entered = r == 1 || pg != 0;
                    const int colStart = r == 1 ? 1 : (r - 1) + D0 + __builtin_ctzll(pg | (1ull << 63));
                    const int colStop = r == 1 ? columns : (r - 1) + D0 + (63 - __builtin_clzll(pg | 1ull));
                    const int maxG = g ? r + D0 + (63 - __builtin_clzll(g)) : -2;
                    const int endc = min(columns, max(colStop, maxG) + 1);
                    if (entered) iters += endc - colStart + 1;
                    if (r == rows) { lastColStart = colStart; lastHasGood = g != 0; lastEntered = entered; }
                    pg = g;
                }
            }
            for (int d = 1; d < Q; d <<= 1) iters += __shfl_xor(iters, d, 64);
            {
                const int owner = groupBase + (rows - 1) / per;
                lastColStart = __shfl(lastColStart, owner, 64); lastHasGood = __shfl(lastHasGood, owner, 64); lastEntered = __shfl(lastEntered, owner, 64);
            }
            // the last row's best cell: highest score; among equals the match plane before D before I, then the lowest column (:672-703)
            int bScore = INT_MIN, bKey = INT_MAX, bPacked = 0;          // key = state * 65536 + column
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int c = rows + D0 + 4 * q + i;
                if (c >= 1 && c <= columns) {
                    const int v[3] = {lastM[i], lastD[i], lastI[i]};
#pragma unroll
                    for (int st = 0; st < 3; st++) {
                        const int sc = v[st] & kScoreMask, key = st * 65536 + c;
                        if (sc > bScore || (sc == bScore && key < bKey)) { bScore = sc; bKey = key; bPacked = v[st]; }
                    }
                }
            }
            for (int d = 1; d < Q; d <<= 1) {
                const int os = __shfl_xor(bScore, d, 64), ok_ = __shfl_xor(bKey, d, 64), op = __shfl_xor(bPacked, d, 64);
                if (os > bScore || (os == bScore && ok_ < bKey)) { bScore = os; bKey = ok_; bPacked = op; }
            }
            const int bCol = bKey & 65535, bState = bKey >> 16;

            int res1, res2, res3, res4 = 0;
            bool fillNull = false;
            if (!lastEntered) { res1 = 1; res2 = 0; res3 = kBadOff; res4 = 1; fillNull = true; }
            else if (!lastHasGood) { res1 = max(1, lastColStart - 1); res2 = 0; res3 = subfloor; res4 = 1; fillNull = true; }
            else if (bScore < minScoreOff) { res1 = bCol; res2 = bState; res3 = bScore; res4 = 1; fillNull = true; }
            else { res1 = bCol; res2 = bState; res3 = bScore >> kScoreOffset; }

            // score2 + traceback2 on the records (MultiStateAligner11tsJNI.java:376-495, :537-658), as msa_fill_fast.hip walks them
            const bool wantScore = !fillNull && (jb.flags & BBMSA_DO_SCORE);
            const bool wantTrace = !fillNull && (jb.flags & BBMSA_DO_TRACEBACK) && p.match != nullptr;
            int sc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int scoreLen = 0, matchLen = 0;
            if (wantScore || wantTrace) {
                uint8_t *out = p.match ? p.match + j * (long long)p.match_stride : nullptr;
                auto nib_at = [&](int r, int c) -> unsigned {
                    const int pos = c - r - D0;
                    if (pos < 0 || pos >= B) return 0u;
                    return (ld_coherent(jdir + (long long)r * 128 + (pos >> 2)) >> (4 * (pos & 3))) & 15u;
                };
                int row = rows, col = res1, state = res2, n = 0, stateTime = 0;
                while (row > 0 && col > 0) {
                    if (state == 0) {
                        // diagonal run: lane q looks at cell (row-q, col-q)
                        const int rr = row - q, cq = col - q;
                        const bool inside = rr >= 1 && cq >= 1;
                        const unsigned nibv = inside ? nib_at(rr, cq) : 0u;
                        const bool brk = !inside || (nibv & 3u) != 0u;
                        const unsigned long long mine = (__ballot(brk) >> groupBase) & ((1ull << Q) - 1ull);
                        const int fb = mine ? __builtin_ctzll(mine) : Q;
                        const int fbInside = __shfl((int)inside, groupBase + min(fb, Q - 1), 64);
                        const int fbPrev = __shfl((int)(nibv & 3u), groupBase + min(fb, Q - 1), 64);
                        const int consumed = (fb < Q && fbInside) ? fb + 1 : fb;
                        if (wantTrace && q < consumed && n + q < p.match_stride) {
                            const int cb = rdL[rr - 1], rb = rfL[min(max(cq - D0, 0), rows + B)];
                            out[n + q] = (cb == rb) ? 'm' : ((!fully_defined(cb) || !fully_defined(rb)) ? 'N' : 'S');
                        }
                        stateTime += fb;
                        if (fb < Q && fbInside) { stateTime = 0; state = fbPrev; }
                        row -= consumed; col -= consumed; n += consumed;
                    } else {
                        const unsigned nibv = nib_at(row, col);
                        int prev;
                        uint8_t sym;
                        if (state == 1) { prev = (nibv & 4u) ? 1 : 0; sym = 'D'; col--; }
                        else { prev = (nibv & 8u) ? 2 : 0; sym = (col >= columns) ? 'Y' : 'I'; row--; }
                        if (wantTrace && q == 0 && n < p.match_stride) out[n] = sym;
                        n++;
                        if (prev == state) stateTime++; else stateTime = 0;
                        state = prev;
                    }
                }
                // score2 tail: MultiStateAligner11tsJNI.java:625-657
                int colS = col;
                if (row > colS) colS -= row;
                const int bestRefStart = a + colS, bestRefStop = a + res1 - 1;
                int padLeft = 0, padRight = 0;
                if (bestRefStart < a) padLeft = max(0, a - bestRefStart);
                else if (bestRefStart == a && state == 2) padLeft = stateTime;
                const int bW = (jb.flags & BBMSA_INTERNAL_GAPPED) ? jb.ref_len : b;      // see msa_fill_fast.hip
                if (bestRefStop > bW) padRight = max(0, bestRefStop - bW);
                else if (bestRefStop == bW && res2 == 2) padRight = bPacked & kTimeMask;
                if (wantScore) {
                    sc[0] = bScore >> kScoreOffset; sc[1] = bestRefStart; sc[2] = bestRefStop; sc[3] = rows; sc[4] = res1; sc[5] = res2;
                    scoreLen = (padLeft > 0 || padRight > 0) ? 8 : 6;
                    if (scoreLen == 8) { sc[6] = padLeft; sc[7] = padRight; }
                }
                if (wantTrace) {
                    // traceback2 tail (:460-471): leftover read bases become 'X'; the window holds no gap symbol (all bases defined)
                    const int xs = (col != row) ? row : 0;
                    for (int i = q; i < xs; i += Q) if (n + i < p.match_stride) out[n + i] = 'X';
                    n += xs;
                    if (n > p.match_stride) matchLen = -1;
                    else {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        __builtin_amdgcn_wave_barrier();
                        for (int i = q; i < n / 2; i += Q) {              // reverse in place
                            const uint8_t lo = (uint8_t)ld_coherent(out + i), hi = (uint8_t)ld_coherent(out + n - 1 - i);
                            out[i] = hi; out[n - 1 - i] = lo;
                        }
                        matchLen = n;
                    }
                }
            }
            if (q == 0) {
                bbmsa_result r;
                r.result[0] = rows; r.result[1] = res1; r.result[2] = res2; r.result[3] = res3; r.result[4] = res4;
                r.status = (fillNull && mode == BBMSA_FILL_LIMITED) ? BBMSA_ST_NULL : BBMSA_ST_OK;
                r.iterations = iters;
#pragma unroll
                for (int i = 0; i < 8; i++) r.score[i] = sc[i];
                r.score_len = scoreLen; r.match_len = matchLen; r.fill_kind = 0; r.columns = columns;
                p.results[j] = r;
                nDone++;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (p.stats) {
        for (int d = 32; d >= 1; d >>= 1) { nDone += __shfl_xor(nDone, d, 64); nLeft += __shfl_xor(nLeft, d, 64); }
        if (lane == 0) { if (nDone) atomicAdd(&p.stats[BAND_STAT_DONE], nDone); if (nLeft) atomicAdd(&p.stats[BAND_STAT_HANDED], nLeft); }
    }
}

template __global__ void msa_fill_band_kernel<8>(const NarrowParams);

const void *band_kernel() { return (const void *)msa_fill_band_kernel<8>; }
int band_lds_bytes(int tableLen, int bandRows) {
    constexpr int Q = 8, B = 4 * Q, JOBS = 2 * (64 / Q);
    const int RB = (bandRows + 4 + 3) & ~3, FB = (bandRows + B + 4 + 3) & ~3;
    return lds_table_ints(tableLen) * 4 + 4 * JOBS * (RB + FB);
}

}  // namespace bbmsa
