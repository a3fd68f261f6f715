// Host harness of tests/test_batch_view_cpu.py: record_of (bbmap_amd/csrc/batch_view.h) under both tier rules on a hand-made view of
// four reads.  Prints one line per read and rule: "<read> <rule> <t|m> <n> <flag> <ml>" (t: the tier's record was taken, m: the main one).
#include <cstdio>

#include "batch_view.h"

template <TierRule RULE> static void show(const BatchView &V, const bbmap_final *tfin, const char *rule) {
    for (long long r = 0; r < V.n; r++) {
        const ReadRec R = record_of<RULE, true>(V, r);
        const ReadRec P = record_of<RULE>(V, r);            // without the list: the same record and string, no list fields
        const bool tier = R.f >= tfin && R.f < tfin + 4;
        const bool agree = P.f == R.f && P.m == R.m && P.ml == R.ml && !P.s && !P.n && !P.flag;
        printf("%lld %s %c %d %d %d%s\n", r, rule, tier ? 't' : 'm', R.n, R.flag, R.ml, agree ? "" : " LISTLESS-DIFFERS");
    }
}

int main() {
    // read 0: plain.  read 1: a tier read, marked in the list and in the record.  read 2: marked in the list only (its record was
    // written with nsites -1 before the tier marked the list).  read 3: marked in both, but without a tier record (tierIdx -1).
    bbmap_final fin[4] = {}, tfin[4] = {};
    bbmap_msite sites[4 * 2] = {}, tsites[4 * 3] = {};
    uint8_t pool[16] = {}, tpool[16] = {};
    const int nsites[4] = {5, BBMAP_NSITES_IN_TIER, BBMAP_NSITES_IN_TIER, BBMAP_NSITES_IN_TIER};      // 5 > cap: clamped to 2
    const int tnsites[4] = {3, 1, 0, 0};
    const int tierIdx[4] = {-1, 0, 1, -1};
    fin[0].nsites = 5; fin[0].match_len = 7;
    fin[1].nsites = BBMAP_NSITES_IN_TIER;
    fin[2].nsites = BBMAP_NSITES_OVERFLOW;
    fin[3].nsites = BBMAP_NSITES_IN_TIER;
    tfin[0].match_len = 9; tfin[1].match_len = 4;
    BatchView V = {};
    V.n = 4; V.fin = fin; V.pool = pool; V.sites = sites; V.nsites = nsites; V.cap = 2;
    V.tfin = tfin; V.tpool = tpool; V.tsites = tsites; V.tnsites = tnsites; V.tcap = 3; V.tierIdx = tierIdx;
    show<TierRule::ByList>(V, tfin, "list");
    show<TierRule::ByRecord>(V, tfin, "record");
    V.tierIdx = nullptr;                                    // no tier read in the batch: every read is the main context's
    show<TierRule::ByList>(V, tfin, "list-notier");
    return 0;
}
