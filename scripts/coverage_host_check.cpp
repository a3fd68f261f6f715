// Stand-alone check of coverage.hip's host side: the layout arithmetic (covoff, bin offsets), the workspace size and the argument
// checks that every raw entry point makes before its first HIP call.  No device is needed.  Meant for a sanitizer build:
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Ibbmap_amd/csrc -Xarch_host -fsanitize=address,undefined \
//       scripts/coverage_host_check.cpp bbmap_amd/csrc/coverage.hip bbmap_amd/csrc/host_common.hip -o coverage_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bbmap_amd.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    // ---- layout: exact-size buffers, so that one entry too many is an out-of-bounds write the sanitizer sees
    const std::vector<int32_t> len = {1, 63, 64, 65, 2047, 2048, 2049, 65536, 65537, 2147483647};
    const int32_t n = (int32_t)len.size();
    std::vector<int64_t> covoff((size_t)n + 1), binoff((size_t)n + 1);
    CHECK(bbpipe_coverage_layout(n, len.data(), 64, covoff.data(), binoff.data()) == BBMAP_OK);
    int64_t slots = 0, bins = 0;
    for (int32_t s = 0; s < n; s++) {
        CHECK(covoff[(size_t)s] == slots && binoff[(size_t)s] == bins);
        slots += (int64_t)len[(size_t)s] + 1;
        bins += ((int64_t)len[(size_t)s] + 63) / 64;
    }
    CHECK(covoff[(size_t)n] == slots && binoff[(size_t)n] == bins && slots > (1ll << 31));
    CHECK(bbpipe_coverage_layout(n, len.data(), 1, nullptr, binoff.data()) == BBMAP_OK && binoff[(size_t)n] == slots - n);
    CHECK(bbpipe_coverage_layout(n, len.data(), 2147483647, nullptr, binoff.data()) == BBMAP_OK && binoff[(size_t)n] == n);
    CHECK(bbpipe_coverage_layout(n, len.data(), 0, covoff.data(), nullptr) == BBMAP_OK);
    CHECK(bbpipe_coverage_layout(0, nullptr, 0, covoff.data(), nullptr) == BBMAP_OK && covoff[0] == 0);
    const int32_t bad[2] = {5, 0};
    CHECK(bbpipe_coverage_layout(2, bad, 0, covoff.data(), nullptr) == BBMAP_E_ARG);
    CHECK(!std::strcmp(bbmap_last_error(), "bbpipe_coverage_layout: a scaffold's length must be >= 1"));
    CHECK(bbpipe_coverage_layout(-1, bad, 0, nullptr, nullptr) == BBMAP_E_ARG && bbpipe_coverage_layout(2, nullptr, 0, nullptr, nullptr) == BBMAP_E_ARG);
    CHECK(bbpipe_coverage_layout(2, bad, -1, nullptr, nullptr) == BBMAP_E_ARG);
    // ---- workspace: grows with both arguments, refuses what the two-level scan cannot hold
    CHECK(bbpipe_coverage_workspace_bytes(1, 2) > 0 && bbpipe_coverage_workspace_bytes(1, 2) % 8 == 0);
    CHECK(bbpipe_coverage_workspace_bytes(3, 1ll << 32) > bbpipe_coverage_workspace_bytes(3, 1ll << 31));
    CHECK(bbpipe_coverage_workspace_bytes(4, 1000) > bbpipe_coverage_workspace_bytes(3, 1000));
    CHECK(bbpipe_coverage_workspace_bytes(1, (1ll << 32) + 1) == BBMAP_E_ARG && bbpipe_coverage_workspace_bytes(-1, 5) == BBMAP_E_ARG);
    // ---- argument checks: every refusal comes before the first HIP call
    int dummy[8] = {0};
    void *p = dummy;
    CHECK(bbpipe_coverage_add_device(nullptr, -1, 0, 0, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                                     nullptr, nullptr, nullptr) == BBMAP_E_ARG);
    CHECK(bbpipe_coverage_add_device(nullptr, 3, 1, 0, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                                     nullptr, nullptr, nullptr) == BBMAP_E_ARG);           // paired with an odd count
    CHECK(bbpipe_coverage_add_device(nullptr, 2, 0, 16, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                                     nullptr, nullptr, nullptr) == BBMAP_E_ARG);
    CHECK(!std::strcmp(bbmap_last_error(), "bbpipe_coverage_add_device: unknown flag bits"));
    CHECK(bbpipe_coverage_add_device(nullptr, 2, 0, BBMAP_COV_STRANDED, (const bbidx_read *)p, (const uint8_t *)p, (const bbmap_final *)p,
                                     (const uint8_t *)p, 1, 1, (const int32_t *)p, (const int32_t *)p, (const int32_t *)p, 0, (const int64_t *)p,
                                     (int32_t *)p, nullptr, (bbmap_covrec *)p, (bbmap_covtotals *)p) == BBMAP_E_ARG);      // no second array
    CHECK(!std::strcmp(bbmap_last_error(), "bbpipe_coverage_add_device: null buffer"));
    CHECK(bbpipe_coverage_add_device(nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                                     nullptr, nullptr, nullptr) == BBMAP_OK);              // an empty batch needs nothing
    CHECK(bbpipe_coverage_finalize_device(nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                          0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0) == BBMAP_E_ARG);
    CHECK(bbpipe_coverage_finalize_device(nullptr, 0, 2, 3, (const int32_t *)p, (const int64_t *)p, (const int32_t *)p, nullptr, p, nullptr,
                                          (bbmap_covrec *)p, nullptr, (int64_t *)p, nullptr, 0, nullptr, 0, nullptr, nullptr,
                                          (bbmap_covtotals *)p, p, 1 << 20) == BBMAP_E_ARG);       // fewer slots than 2 per scaffold
    CHECK(bbpipe_coverage_finalize_device(nullptr, 0, 2, 10, (const int32_t *)p, (const int64_t *)p, (const int32_t *)p, nullptr, p, nullptr,
                                          (bbmap_covrec *)p, nullptr, (int64_t *)p, nullptr, 4, nullptr, 3, nullptr, nullptr,
                                          (bbmap_covtotals *)p, p, 1 << 20) == BBMAP_E_ARG);       // a binsize without bin arrays
    CHECK(!std::strcmp(bbmap_last_error(), "bbpipe_coverage_finalize_device: null buffer"));
    CHECK(bbpipe_coverage_finalize_device(nullptr, 0, 2, 10, (const int32_t *)p, (const int64_t *)p, (const int32_t *)p, nullptr, p, nullptr,
                                          (bbmap_covrec *)p, nullptr, (int64_t *)p, nullptr, 0, nullptr, 0, nullptr, nullptr,
                                          (bbmap_covtotals *)p, p, 8) == BBMAP_E_ARG);
    CHECK(!std::strcmp(bbmap_last_error(), "bbpipe_coverage_finalize_device: the workspace is smaller than bbpipe_coverage_workspace_bytes"));
    std::puts("coverage_host_check: ok");
    return 0;
}
