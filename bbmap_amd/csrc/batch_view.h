// A finished batch as the output stages' kernels see it, and the one lookup "which record does read r have".
//
// A read that the overflow tier mapped takes the tier's final record, match-string pool and site list; every other read takes the
// main context's.  tierIdx[r] is the read's record in the tier (-1 = none; mapper_output.hip fills it per call), and two rules
// decide whether a read with a tier record is a tier read:
//   ByList    the main list's count says so, nsites[r] == BBMAP_NSITES_IN_TIER (mark_tier_kernel wrote it): run statistics,
//             coverage, read histograms, reference-set binning
//   ByRecord  the main final record says so, fin[r].nsites == BBMAP_NSITES_IN_TIER: SAM records, scaffold records, and
//             bbmap_get_final's loop on the host
// They can disagree.  The main context's final stage writes fin[r].nsites from the list as it was then, and the tier's last pass
// marks the list afterwards: a read whose record says -1 or -2 (flagged) and whose list count says -3 is a tier read by the list
// and a main-context read by the record.  Each stage keeps the rule it was written with; which one is right is an open question.
#pragma once
#include <hip/hip_runtime.h>

#include "bbmap_amd.h"

struct BatchView {
    const bbidx_read *reads; const uint8_t *bases;          // the batch's reads, plus strands
    long long n; int paired;
    // the main context's final records, their string pool, and its site lists (cap slots per read, nsites[r] used or a flag < 0)
    const bbmap_final *fin; const uint8_t *pool; const bbmap_msite *sites; const int *nsites; int cap;
    // the overflow tier's, and read -> tier record: all null / 0 when the tier mapped no read
    const bbmap_final *tfin; const uint8_t *tpool; const bbmap_msite *tsites; const int *tnsites; int tcap;
    const int *tierIdx;
};

// One read's record, wave- or thread-uniform as the caller is.  m / ml: the match string (null / 0 without one).  s / n: the site
// list, n clamped to [0, cap] of the list taken; flag: the main list's raw count, before any substitution.  The three list fields
// are filled by record_of<RULE, true> only.
struct ReadRec { const bbmap_final *f; const uint8_t *m; int ml; const bbmap_msite *s; int n; int flag; };

enum class TierRule { ByList, ByRecord };

// (V by value: the callers hand in a member of their kernel's argument block, and through a reference to it read_hist_add_kernel's
// mate loop is no longer unrolled and its two per-mate arrays land in scratch)
template <TierRule RULE, bool SITES = false> __host__ __device__ inline ReadRec record_of(const BatchView V, long long r) {
    ReadRec R;
    R.f = V.fin + r;
    R.s = nullptr; R.n = R.flag = 0;
    const uint8_t *pl = V.pool;
    int cap = 0;
    if constexpr (SITES) { R.s = V.sites + r * V.cap; R.n = R.flag = V.nsites[r]; cap = V.cap; }
    // (nsites may be null where tierIdx is: the raw calls of the stages that read no list)
    if (V.tierIdx && (RULE == TierRule::ByRecord ? R.f->nsites : SITES ? R.flag : V.nsites[r]) == BBMAP_NSITES_IN_TIER && V.tierIdx[r] >= 0) {
        const long long t = V.tierIdx[r];
        R.f = V.tfin + t; pl = V.tpool;
        if constexpr (SITES) { R.s = V.tsites + t * V.tcap; R.n = V.tnsites[t]; cap = V.tcap; }
    }
    if constexpr (SITES) R.n = R.n < 0 ? 0 : R.n > cap ? cap : R.n;
    R.ml = R.f->match_len > 0 ? R.f->match_len : 0;
    R.m = R.ml ? pl + R.f->match_off : nullptr;
    return R;
}
