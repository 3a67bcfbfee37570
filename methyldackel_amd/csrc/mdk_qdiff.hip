// mdk_qdiff.hip -- libmdk_stats.so (include/mdk_stats.h): two groups of replicate samples compared site by site on the device, the
// quasi-binomial F test.  The rule is mdk_qdiff_core.h's; entries, limits and refusals are mdk_diff_core.h's.  A library of its own, as
// mdk_tabix.hip's is -- one code object, its own stream, its own pinned status block, its own error text -- that links nothing of
// libmdk_hip.so.
//
// One synchronous call and one kernel:
//   k_qdiff  a lane per site, 256 per workgroup (k_diff's layout: dealing terms instead of sites to the lanes was measured slower there,
//            DESIGN.md section 4).  `order` holds the samples in the rule's visiting order, group A's ascending and then group B's; its
//            index is the same in every lane, so its loads are uniform.
//            pass 1  the site's entries of the named samples, row after row -- every row read coalesced along n --, each entry checked
//                    and pooled in 64 bits, the covered samples of each group counted; then the four margins checked.  A refusal: (site
//                    << 8 | bit) into the status by atomicMin, the kernel's one atomic; the site's outputs are those of a site without
//                    anything to test, and it is not tested
//            pass 2  the same rows once more (a lane cannot keep 1024 entries): qdiff_term of every covered sample of a group whose
//                    pooled counts are both above 0, added in visiting order from 0.0
//            test    qdiff_site on the lane -- the score, the dispersion, the tail's series --, the nine outputs and `steps` stored
//                    coalesced
//            A wavefront takes as long as the longest series of its 64 sites, and that is what the kernel's time was measured to
//            follow -- not the mean series, and not the rows' bytes.
// Per site 8 S bytes read twice (int32 matrices) and 60 written, against S + 20 and some dozens of double-precision divisions.  Nothing
// is read outside the named rows of the two matrices and `order`, nothing written outside the outputs.  Plain C++, vector loads and
// stores, no LDS.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include "mdk_stats.h"
#include "mdk_qdiff_core.h"

#define QDIFF_WG 256

struct StatsStatus { unsigned long long first; };              // the smallest (site << 8 | refusal's bit number); all ones: none
struct StatsPinned { StatsStatus st; int32_t order[DIFF_MAX_SAMPLES]; int32_t group_end[DIFF_MAX_SAMPLES]; };          // (group_end: md_stats_gdiff's)

struct KQdiff {
    const void *m, *u; const int32_t *order; int32_t n_a, n_b; int64_t n; double min_dispersion;
    int64_t *a, *b, *c, *d; double *diff, *p; int32_t *df; double *dispersion, *statistic; uint32_t *steps;
    StatsStatus *st;
};

template <typename T>
__global__ __launch_bounds__(QDIFF_WG) void k_qdiff(const KQdiff K) {
    MDK_DIFF_NO_CONTRACT
    const int64_t i = (int64_t)blockIdx.x * QDIFF_WG + threadIdx.x;
    if(i >= K.n) return;
    const T *const M = (const T *)K.m, *const U = (const T *)K.u;
    const int32_t *const __restrict__ order = K.order;
    const int32_t n_all = K.n_a + K.n_b;
    int64_t a = 0, b = 0, c = 0, d = 0; int32_t ka = 0, kb = 0; uint32_t err = 0;
    for(int32_t k = 0; k < n_all; k++) {
        const int64_t at = (int64_t)order[k] * K.n + i;        // (order[k] is the same for every lane)
        const int64_t m = (int64_t)M[at], u = (int64_t)U[at];
        const uint32_t e = diff_entry_check(m) | diff_entry_check(u);
        err |= e;
        if(!e) {                                               // (a refused entry is not added: the sums stay below 2^37)
            const int32_t covered = m + u > 0;
            if(k < K.n_a) { a += m; b += u; ka += covered; } else { c += m; d += u; kb += covered; }
        }
    }
    if(!err) err = diff_margin_check(a, b, c, d);
    if(err) {
        atomicMin(&K.st->first, ((unsigned long long)i << 8) | (unsigned long long)(__ffs(err) - 1));
        K.a[i] = 0; K.b[i] = 0; K.c[i] = 0; K.d[i] = 0; K.diff[i] = 0.0;
        K.p[i] = 1.0; K.df[i] = 0; K.dispersion[i] = 1.0; K.statistic[i] = 0.0;
        if(K.steps) K.steps[i] = 0;
        return;                                                // (not tested: its margins may be past what the rule takes)
    }
    const bool in_a = a > 0 && b > 0, in_b = c > 0 && d > 0;   // a group all methylated or all unmethylated contributes nothing
    double pearson = 0.0;
    for(int32_t k = 0; k < n_all; k++) {
        const bool first = k < K.n_a;
        if(!(first ? in_a : in_b)) continue;
        const int64_t at = (int64_t)order[k] * K.n + i;
        const int64_t m = (int64_t)M[at], u = (int64_t)U[at];
        if(m + u > 0) pearson = pearson + (first ? qdiff_term(m, u, a, b) : qdiff_term(m, u, c, d));
    }
    qdiff_result r;
    qdiff_site(a, b, c, d, ka, kb, pearson, K.min_dispersion, &r);
    K.a[i] = a; K.b[i] = b; K.c[i] = c; K.d[i] = d; K.diff[i] = diff_meth(a, b, c, d);
    K.p[i] = r.p; K.df[i] = r.df; K.dispersion[i] = r.dispersion; K.statistic[i] = r.statistic;
    if(K.steps) K.steps[i] = r.steps;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
#define SIDE_ERR_ARG MD_STATS_ERR_ARG
#define SIDE_ERR_HIP MD_STATS_ERR_HIP
#define SIDE_ERR_NOMEM MD_STATS_ERR_NOMEM
#include "mdk_side.hpp"
extern "C" const char *md_stats_last_error(void) { return g_err; }

struct md_stats : SideHandle<StatsStatus, StatsPinned> {
    int32_t *d_order = nullptr, *d_group_end = nullptr;                      // (d_group_end: md_stats_gdiff's, the groups' ends in d_order)
    SideBuf<double> d_design; SideBuf<double, true> pin_design;            // (md_stats_mdiff's, made at its first call: a row of the design per entry of d_order, and its pinned mirror)
    int32_t mom_shape = 0, mom_chunk = 0, mom_tile = 0, mom_grid = 0;      // md_stats_moments_limits; 0: the default of each
    int32_t prof_range = 0, prof_band = 0, prof_grid = 0;                  // md_stats_profile_limits; likewise
};

extern "C" int md_stats_open(int device, md_stats **out) {
    return side_open(device, out, "md_stats_open", md_stats_close, [](md_stats *h) {
        const hipError_t e = hipMalloc((void **)&h->d_order, DIFF_MAX_SAMPLES * sizeof(int32_t));
        return e != hipSuccess ? e : hipMalloc((void **)&h->d_group_end, DIFF_MAX_SAMPLES * sizeof(int32_t));
    });
}

extern "C" void md_stats_close(md_stats *h) {
    if(!h) return;
    h->close(); (void)hipFree(h->d_order); (void)hipFree(h->d_group_end); h->d_design.release(); h->pin_design.release();
    delete h;
}

extern "C" int md_stats_qdiff(md_stats *h, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n,
                              const int32_t *order, int32_t n_a, int32_t n_b, double min_dispersion,
                              int64_t *nmeth_a, int64_t *nunmeth_a, int64_t *nmeth_b, int64_t *nunmeth_b, double *meth_diff,
                              double *pvalue, int32_t *df, double *dispersion, double *statistic, uint32_t *steps) {
    const char *const what = "md_stats_qdiff";
    if(!h || !order || (elem_bytes != 4 && elem_bytes != 8) || n_samples < 1 || n_samples > DIFF_MAX_SAMPLES || n < 0 || n > DIFF_MAX_SITES || n_a < 0 || n_b < 0)
        return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    if(n && (!nmeth || !nunmeth || !nmeth_a || !nunmeth_a || !nmeth_b || !nunmeth_b || !meth_diff || !pvalue || !df || !dispersion || !statistic))
        return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    if(!(min_dispersion >= 0x1p-55 && min_dispersion <= 0x1p800)) {
        snprintf(g_err, sizeof g_err, "%s: min_dispersion must be within 2^-55 and 2^800", what);
        return MD_STATS_ERR_ARG;
    }
    if(!n_a || !n_b) {
        snprintf(g_err, sizeof g_err, "%s: group %s has no sample", what, n_a ? "B" : "A");
        return MD_STATS_ERR_ARG;
    }
    // the order: few, and the kernel trusts it
    if((int64_t)n_a + n_b > n_samples) {
        snprintf(g_err, sizeof g_err, "%s: the groups name %lld samples, the matrices hold %d: a sample is named twice", what, (long long)n_a + n_b, (int)n_samples);
        return MD_STATS_ERR_ARG;
    }
    bool seen[DIFF_MAX_SAMPLES];
    memset(seen, 0, sizeof seen);
    for(int32_t k = 0; k < n_a + n_b; k++) {
        const int32_t s = order[k];
        if(s < 0 || s >= n_samples) {
            snprintf(g_err, sizeof g_err, "%s: group %s names sample %d: the matrices hold samples 0 to %d", what, k < n_a ? "A" : "B", (int)s, (int)n_samples - 1);
            return MD_STATS_ERR_ARG;
        }
        if(seen[s]) {
            snprintf(g_err, sizeof g_err, "%s: sample %d is named twice", what, (int)s);
            return MD_STATS_ERR_ARG;
        }
        seen[s] = true;
    }
    if(!n) return 0;
    SIDECHK(hipSetDevice(h->device));
    memcpy(h->pin->order, order, (size_t)(n_a + n_b) * sizeof(int32_t));
    SIDECHK(hipMemcpyAsync(h->d_order, h->pin->order, (size_t)(n_a + n_b) * sizeof(int32_t), hipMemcpyHostToDevice, h->st));
    SIDE_STATUS_UP(h, &h->pin->st, StatsStatus);
    KQdiff K;
    K.m = nmeth; K.u = nunmeth; K.order = h->d_order; K.n_a = n_a; K.n_b = n_b; K.n = n; K.min_dispersion = min_dispersion;
    K.a = nmeth_a; K.b = nunmeth_a; K.c = nmeth_b; K.d = nunmeth_b; K.diff = meth_diff; K.p = pvalue; K.df = df; K.dispersion = dispersion; K.statistic = statistic;
    K.steps = steps; K.st = h->d_st;
    const dim3 grid((uint32_t)((n + QDIFF_WG - 1) / QDIFF_WG));
    if(elem_bytes == 4) hipLaunchKernelGGL(k_qdiff<int32_t>, grid, dim3(QDIFF_WG), 0, h->st, K);
    else hipLaunchKernelGGL(k_qdiff<int64_t>, grid, dim3(QDIFF_WG), 0, h->st, K);
    SIDECHK(hipGetLastError());
    SIDE_STATUS_DOWN(h, &h->pin->st, StatsStatus);
    const unsigned long long first = h->pin->st.first;
    if(first == ~0ull) return 0;
    const uint32_t bit = 1u << (first & 0xffu);
    snprintf(g_err, sizeof g_err, "%s: %s (site %lld)", what,
             bit == DIFF_E_NEGATIVE ? "a count is negative" :
             bit == DIFF_E_ENTRY ? "a count is 2^26 or more" : "a pooled margin (a group's depth, or the methylated or the unmethylated of both) is 2^26 or more",
             (long long)(first >> 8));
    return MD_STATS_ERR_ARG;
}

// the pairwise sample moments: the library's other calls, on the same handle
#include "mdk_moments.hip"
// the count profile: likewise
#include "mdk_profile.hip"
