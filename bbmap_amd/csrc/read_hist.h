// Read histograms on the device (include/bbmap_amd.h, bbmap_hist_* / bbpipe_read_hist_*): the launch of read_hist.hip.
// Out of scope (bbmap_amd.h has the reasons): aqhist=, timehist=, ihist= (bbmap_get_run_stats' histogram), ID_BINS_AUTO /
// GC_BINS_AUTO / GC_PLOT_X, the SamLine branches of pairnum, JNI natives for BBMapHIP.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_view.h"
#include "bbmap_amd.h"

namespace bbrh {

enum { WAVES_PER_BLOCK = 16, TB = 64 * WAVES_PER_BLOCK, MAX_BLOCKS = BBMAP_RH_MAX_BLOCKS, CHUNK = BBMAP_RH_CHUNK_UNITS };
enum { MAXLEN = BBMAP_RH_MAXLEN, MAXPOS = BBMAP_RH_MAX_POS, QBINS = BBMAP_RH_QUAL_BINS, ABINS = BBMAP_RH_ACC_BINS };
enum { TILE = BBMAP_RH_POS_TILE, QTILE = BBMAP_RH_QUAL_TILE };
enum { INS_BINS = BBMAP_RH_MAXINSLEN + 1, DEL_BINS = BBMAP_RH_MAXDELLEN, DEL2_BINS = BBMAP_RH_DEL2_BINS };
enum { GC_WORDS = BBMAP_RH_GC_BINS + 2, ID_BINS = BBMAP_RH_ID_BINS + 1, ID_WORDS = 2 * ID_BINS + 1 };
enum { M_match, M_sub, M_del, M_ins, M_N, M_clip, M_other, N_MATCH_ARRAYS };
enum { Q_match, Q_sub, Q_ins, Q_del };
// The arrays of the state, in the order they lie in it
enum { A_MATCH, A_QLEN, A_BQUAL, A_QCOUNT, A_BASE, A_ACC, A_INS, A_DEL, A_DEL2, A_ERR, A_LEN, A_GC, A_ID, N_ARRAYS };

// A workgroup's LDS counters (32 bit), 131,880 bytes of the CU's 160 KiB: one workgroup of 16 wavefronts per CU.
//   per-position arrays, positions < TILE:  7 x 2 (mhist) + 2 x 5 (bhist) + 2 (qualLength) rows of 256      26,624 B
//   bqualHist, positions < TILE x qualities < QTILE, per mate: 2 x 256 x 44                                 90,112 B
//   accuracy 4 x 99, ins 1001, del 1000, del2 64, error 256, identity 2 x 101, GC 101, length 512,
//   qcountHist 2 x 127                                                                                        15,144 B
enum { L_MATCH = 0, L_BASE = L_MATCH + 2 * N_MATCH_ARRAYS * TILE, L_QLEN = L_BASE + 10 * TILE, L_BQUAL = L_QLEN + 2 * TILE,
       L_ACC = L_BQUAL + 2 * TILE * QTILE, L_INS = L_ACC + 4 * ABINS, L_DEL = L_INS + INS_BINS, L_DEL2 = L_DEL + DEL_BINS,
       L_ERR = L_DEL2 + BBMAP_RH_DEL2_LDS_BINS, L_ID = L_ERR + BBMAP_RH_ERR_LDS_BINS, L_IDBASE = L_ID + ID_BINS, L_GC = L_IDBASE + ID_BINS,
       L_LEN = L_GC + BBMAP_RH_GC_BINS + 1, L_QCOUNT = L_LEN + BBMAP_RH_LEN_LDS_BINS, L_TOTAL = L_QCOUNT + 2 * QBINS };
static_assert(4 * L_TOTAL <= 160 * 1024, "the counters of one workgroup fit the CU's LDS");
// The largest amount one read adds to one 32-bit counter is its length (idBaseHist, qcountHist): a chunk's reads cannot overflow it
static_assert(2ll * CHUNK * MAXPOS < (1ll << 32), "a chunk's reads cannot overflow a 32-bit counter");

// A piece of the LDS counters and where it goes in the state: LDS index ((i0 * n1) + i1) * n2 + i2 -> word hbm + i0 * s0 + i1 * s1 + i2
struct Segment { int lds, n0, n1, n2; long long hbm, s0, s1; };
enum { N_SEGMENTS = 14 };

struct Layout { long long off[N_ARRAYS]; long long words; };           // off < 0: the group is not selected
Layout layout_of(int flags);

struct Args {
    BatchView V;
    const uint8_t *qual;                                               // by bases_off, as V.bases; nullptr: no qualities
    int flags;
    unsigned long long *state;
};
hipError_t launch_add(const Args &a, hipStream_t stream);

}  // namespace bbrh
