// Which kernels one DP launch runs (bbmsa_align_impl, msa_host.hip), decided in one place from the context's switches and the launch's
// size.  Host only and without a HIP call, so that the rule is tested without a device (tests/test_msa_route_cpu.py).
#pragma once
#include "bbmap_amd.h"

// What the decision reads: bbmsa_create and the setters of msa_ctx.h write it, nothing else does.
struct RouteSwitches {
    int scheme = 0;                 // BBMSA_SCHEME_*
    bool banded = false;            // the context has a band (bandwidth / bandwidthRatio)
    bool bandPresent = false;       // the band kernel was set up (never in a banded context; BBMSA_NARROW=0: no)
    bool bandOff = false;           // switched off by the caller for launches whose jobs it cannot take (bbmsa_use_narrow)
    // widest windows first (bbmsa_sort_by_width): two jobs share a wavefront and step together, so a 600-column job beside a
    // 200-column one idles half the wave for 400 steps; in width order neighbours are alike, and the longest jobs do not end up last
    bool sortByWidth = false;
    bool sortWithBand = false;      // sort also the launches that run the band kernel (bbmsa_sort_with_band): the candidates get a list of their own
    bool unlimitedLoop = true;      // a width-sorted launch runs its unlimited fills in the wavefront kernel's build for them (BBMSA_UNLIMITED_LOOP=0: no)
    bool wideUnlimited = false;     // the 64-lane launches run unlimited fills in the prune-free loop (bbmsa_set_wide_unlimited)
    bool widePresent = false;       // the 64-lane geometry was set up (setup_wide_pass)
    long long latencyJobs = 0;      // launches with at most this many jobs go straight to the 64-lane geometry (bbmsa_set_latency_jobs)
    int pipeJobsMax = 0;            // 9PacBio: launches with at most this many jobs take the strip kernel's pipelined form (0: never)
};

// One launch's route.  bbmsa_ctx::last keeps the last one for the read-back entries (bbmsa_last_route and its kin).
struct Route {
    bool band = false;              // the band kernel runs in front of the first pass
    bool sorted = false;            // the width sort writes the first pass's lists
    bool latency = false;           // no first pass: the 64-lane geometry takes every job
    bool indirect = false;          // the job count is read on the device
    bool wide = false;              // the wide pass runs
    bool unlList = false;           // the unlimited build gets a launch over the sort's list of unlimited fills
    bool wideBoth = false;          // the 64-lane launch asks for the build with both step loops
    bool pipelined = false;         // 9PacBio: the strip kernel's pipelined form
    long long jobs = 0;
};

inline Route plan_route(const RouteSwitches &s, long long n_jobs, bool indirect) {
    Route r;
    r.indirect = indirect; r.jobs = n_jobs;
    if (s.scheme != BBMSA_SCHEME_11TS) {
        // few jobs (the late scoreSlow rounds of mapPacBio): a lone 6,000 x 6,100 fill is one wavefront's dependent chain, 370 ms;
        // with its strips pipelined over `pipeK` wavefronts it is ~50
        r.pipelined = !indirect && s.pipeJobsMax > 0 && n_jobs <= s.pipeJobsMax;
        return r;
    }
    r.band = s.bandPresent && !s.bandOff;
    r.wide = s.widePresent;
    // Both the band kernel and the sort write the wavefront kernel's list.  Together only on request (bbmsa_sort_with_band): the sort
    // then gives the band kernel a list of its candidates, and the band kernel appends what it hands on behind the sorted list.
    r.sorted = s.sortByWidth && !indirect && n_jobs >= 256 && n_jobs > s.latencyJobs && (!r.band || s.sortWithBand);
    // A launch with few jobs is a wavefront's latency, not throughput: (columns + lanes - 1) steps of one dependent chain.  The wide
    // pass's geometry (64 lanes x 3 rows, one job per block) has the shorter chain per step (3 rows instead of 5: ~450 instead of
    // ~740 instructions), so such launches go to it directly (bbmsa_set_latency_jobs; the mapper's late rounds hold a few hundred fills).
    r.latency = r.wide && !indirect && !r.band && n_jobs <= s.latencyJobs;
    // the sort made a list of the unlimited fills: the build without limits and prune tests takes them, the general build the rest
    r.unlList = r.sorted && s.unlimitedLoop;
    // one job per wavefront: which step loop runs is wave-uniform, so one build can hold both and give an unlimited fill the
    // prune-free one (bbmsa_set_wide_unlimited; a banded context has no such build)
    r.wideBoth = s.wideUnlimited && !s.banded;
    return r;
}
