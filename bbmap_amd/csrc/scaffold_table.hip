// bbidx_set_scaffolds: the per-chromosome scaffold table of an index context (include/bbmap_amd.h; device layout: scaffold.h).
// The reference keeps it in Data.scaffoldLocs / scaffoldLengths / interScaffoldPadding (current/dna/Data.java), filled from the
// packer's scaffold list (FastaToChromArrays2.java:449-472).
#include <hip/hip_runtime.h>

#include <vector>

#include "bbmap_amd.h"
#include "host_common.h"
#include "index_ctx.h"

static void clear_table(bbidx_ctx *c) {
    if (c->scafBuf) (void)hipFree(c->scafBuf);
    c->scafBuf = nullptr;
    c->scaf = bbscaf::Table{};
    c->scafFilter = false;
    c->scafGen++;
}

extern "C" int bbidx_set_scaffolds(bbidx_ctx *c, int32_t nchroms, const int32_t *counts, const int32_t *const *locs,
                                   const int32_t *const *lengths, int32_t inter_scaffold_padding) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbidx_set_scaffolds: null context");
    if (hipSetDevice(c->device) != hipSuccess) return bbfail(BBMAP_E_ARG, "bbidx_set_scaffolds: bad device");
    if (!counts) { clear_table(c); return BBMAP_OK; }
    const int nc = c->dev.nchroms;
    if (nchroms != nc) return bbfail(BBMAP_E_ARG, "bbidx_set_scaffolds: nchroms is not the index's");
    if (!locs || !lengths) return bbfail(BBMAP_E_ARG, "bbidx_set_scaffolds: null locs / lengths");
    std::vector<int32_t> alen((size_t)nc + 1, 0);
    if (hipMemcpy(alen.data(), c->dev.chromArrLen, ((size_t)nc + 1) * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return bbfail(BBMAP_E_ARG, "bbidx_set_scaffolds: could not read the chromosome lengths");
    // validate everything before the table in force is touched
    long long total = 0;
    bool multi = false;
    for (int ch = 1; ch <= nc; ch++) {
        const int n = counts[ch];
        if (n < 1) return bbfail(BBMAP_E_ARG, "bbidx_set_scaffolds: every chromosome needs at least one scaffold");
        if (!locs[ch] || !lengths[ch]) return bbfail(BBMAP_E_ARG, "bbidx_set_scaffolds: null locs / lengths of a chromosome");
        for (int i = 0; i < n; i++) {
            const int a = locs[ch][i], l = lengths[ch][i];
            if (a < 0 || (i > 0 && a <= locs[ch][i - 1])) return bbfail(BBMAP_E_ARG, "bbidx_set_scaffolds: scaffold starts must ascend strictly from 0 on");
            if (l < 1 || (long long)a + l > alen[(size_t)ch]) return bbfail(BBMAP_E_ARG, "bbidx_set_scaffolds: a scaffold reaches past its chromosome array");
        }
        total += n;
        multi = multi || n >= 2;
    }
    if (multi && inter_scaffold_padding <= 0) return bbfail(BBMAP_E_ARG, "bbidx_set_scaffolds: inter_scaffold_padding must be > 0");
    if (total > (1ll << 30)) return bbfail(BBMAP_E_ARG, "bbidx_set_scaffolds: too many scaffolds");
    std::vector<int32_t> h((size_t)(nc + 2) + 2 * (size_t)total);
    int32_t *off = h.data(), *loc = off + nc + 2, *len = loc + total;
    off[0] = off[1] = 0;
    for (int ch = 1; ch <= nc; ch++) {
        const int b = off[ch], n = counts[ch];
        for (int i = 0; i < n; i++) { loc[b + i] = locs[ch][i]; len[b + i] = lengths[ch][i]; }
        off[ch + 1] = b + n;
    }
    void *d = nullptr;
    if (hipMalloc(&d, h.size() * 4) != hipSuccess) { (void)hipGetLastError(); return bbfail(BBMAP_E_NOMEM, "bbidx_set_scaffolds: device allocation failed"); }
    if (hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return bbfail(BBMAP_E_HIP, "bbidx_set_scaffolds: upload failed");
    }
    clear_table(c);
    c->scafBuf = d;
    const int32_t *dd = (const int32_t *)d;
    c->scaf.off = dd; c->scaf.loc = dd + nc + 2; c->scaf.len = dd + nc + 2 + total;
    c->scaf.pad = inter_scaffold_padding;
    c->scaf.nchroms = nc;
    c->scafFilter = multi;
    return BBMAP_OK;
}
