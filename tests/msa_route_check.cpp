// Host harness of tests/test_msa_route_cpu.py: plan_route (bbmap_amd/csrc/msa_route.h) on hand-picked switch settings, then four
// properties over the full cross product of the switches.  Prints one line per case: "<case> n=<jobs>[ dev]: <the Route fields that
// are true, in declaration order, or ->" (dev: the job count is read on the device).
#include <cstdio>

#include "msa_route.h"

static void show(const char *name, const RouteSwitches &s, long long n, bool dev = false) {
    const Route r = plan_route(s, n, dev);
    const bool on[8] = {r.band, r.sorted, r.latency, r.indirect, r.wide, r.unlList, r.wideBoth, r.pipelined};
    const char *names[8] = {"band", "sorted", "latency", "indirect", "wide", "unlList", "wideBoth", "pipelined"};
    printf("%s n=%lld%s:", name, n, dev ? " dev" : "");
    bool any = false;
    for (int i = 0; i < 8; i++) if (on[i]) { printf(" %s", names[i]); any = true; }
    printf("%s%s\n", any ? "" : " -", r.jobs == n ? "" : " JOBS-DIFFER");
}

int main() {
    RouteSwitches base;                       // an 11ts context with a wide pass and the band kernel, every switch as bbmsa_create leaves it
    base.scheme = BBMSA_SCHEME_11TS; base.widePresent = true; base.bandPresent = true;
    RouteSwitches s = base;
    show("1", s, 5200);
    s.sortByWidth = true;
    show("2", s, 5200);
    s.sortWithBand = true;
    show("3", s, 5200);
    s.unlimitedLoop = false;
    show("4", s, 5200);
    s.unlimitedLoop = true;
    show("5", s, 255);
    show("5", s, 256);
    show("6", s, 5200, true);

    s = base; s.bandOff = true; s.sortByWidth = true; s.latencyJobs = 4096;
    show("7", s, 4096);
    show("7", s, 4097);
    show("7", s, 4096, true);
    s = base; s.sortByWidth = true; s.sortWithBand = true; s.latencyJobs = 4096;
    show("8", s, 300);
    s = base; s.bandOff = true;
    show("9", s, 1);
    s = base; s.bandOff = true; s.widePresent = false; s.latencyJobs = 4096;
    show("10", s, 10);
    s = base; s.bandPresent = false; s.wideUnlimited = true;
    show("11-plain", s, 5200);
    s.banded = true;
    show("11-banded", s, 5200);

    s = base; s.scheme = BBMSA_SCHEME_9PACBIO; s.pipeJobsMax = 512;            // the 11ts switches are not a PacBio launch's business
    s.sortByWidth = s.sortWithBand = s.wideUnlimited = true; s.latencyJobs = 4096;
    show("12", s, 512);
    show("12", s, 513);
    show("12", s, 10, true);
    s.pipeJobsMax = 0;
    show("12-nopipe", s, 10);

    long long routes = 0, bad = 0;
    const long long ns[6] = {1, 255, 256, 257, 4096, 4097};
    for (int bits = 0; bits < (1 << 12); bits++) {
        RouteSwitches x;
        x.scheme = (bits & 1) ? BBMSA_SCHEME_9PACBIO : BBMSA_SCHEME_11TS;
        x.banded = bits & 2; x.bandPresent = bits & 4; x.bandOff = bits & 8; x.sortByWidth = bits & 16; x.sortWithBand = bits & 32;
        x.unlimitedLoop = bits & 64; x.wideUnlimited = bits & 128; x.widePresent = bits & 256;
        x.latencyJobs = (bits & 512) ? 4096 : 0; x.pipeJobsMax = (bits & 1024) ? 512 : 0;
        const bool dev = bits & 2048;
        for (long long n : ns) {
            const Route r = plan_route(x, n, dev);
            routes++;
            if (r.sorted && r.latency) bad++;
            if (dev && (r.sorted || r.latency || r.pipelined)) bad++;
            if (r.unlList && !r.sorted) bad++;
            if (r.latency && (r.band || !r.wide)) bad++;
        }
    }
    printf("cross product: %lld routes, %lld broken\n", routes, bad);
    return 0;
}
