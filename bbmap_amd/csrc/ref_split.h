// Reference-set binning on the device (include/bbmap_amd.h, bbmap_split_* / bbpipe_refsplit_*): the launches of ref_split.hip.
// Out of scope (bbmap_amd.h has the reasons): AMBIGUOUS2_RANDOM, more than 64 sets, reference merging, file streams, bamscript.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_view.h"
#include "bbmap_amd.h"
#include "scaffold.h"

namespace bbsplit {

enum { TB = 256, CHUNK = BBMAP_SPLIT_CHUNK_READS, MAX_BLOCKS = BBMAP_SPLIT_MAX_BLOCKS };
enum { SLOTS = BBMAP_SPLIT_LDS_SLOTS, MAX_PROBES = BBMAP_SPLIT_MAX_PROBES, MAX_SETS = BBMAP_SPLIT_MAX_SETS, HEAD = BBMAP_SPLIT_STATE_HEAD };
enum { LIST_TB = BBMAP_SPLIT_LIST_BLOCK, LIST_WAVES = LIST_TB / 64 };
// A workgroup's LDS: the key table (4 B key + 4 x 8 B sums per slot) and the 64 x 4 set counters, 38,912 bytes of the CU's 160 KiB:
// four workgroups of four wavefronts per CU.
static_assert((SLOTS & (SLOTS - 1)) == 0 && SLOTS == 1 << 10, "the slot of a key is the top 10 bits of its hash");
static_assert(SLOTS * 36 + MAX_SETS * 32 <= 64 * 1024, "static LDS of one workgroup");
static_assert(CHUNK % TB == 0 && TB % 2 == 0, "mates sit in neighbouring lanes of one workgroup");
static_assert(sizeof(bbmap_splitrec) == 32 && sizeof(bbmap_split_config) == 32, "ABI sizes");

struct Args {
    BatchView V;                    // (bases and match strings are not read)
    bbscaf::Table T;
    const unsigned long long *scafSets; const int *scafKey;
    int flags, mode, clearzone, maxSites, nsets, nkeys;
    unsigned long long *state;      // HEAD words, 4 per key, 4 per set
    bbmap_splitrec *recs;           // nullptr = not wanted
};
// nullptr when the configuration is fine, else what is wrong with it
const char *check_config(const bbmap_split_config &cfg);
hipError_t launch_assign(const Args &a, hipStream_t stream);

long long list_blocks(long long n, int paired);
long long lists_workspace_bytes(long long n, int paired, int nsets);
hipError_t launch_lists(long long n, int paired, int nsets, const bbmap_splitrec *recs, void *ws, long long wsBytes, long long *setOff,
                        int *units, long long unitsCap, hipStream_t stream);

}  // namespace bbsplit
