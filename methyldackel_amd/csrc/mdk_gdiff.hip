// mdk_gdiff.hip -- more of libmdk_stats.so (include/mdk_gdiff.h), in mdk_qdiff.hip's chain of includes (mdk_profile.hip, the
// file that ends mdk_qdiff.hip, includes it at its own end, and it includes mdk_mdiff.hip at its own): three or more groups of replicate
// samples compared site by site on the device, the quasi-binomial F test with q = groups - 1 numerator degrees of freedom.  The rule is
// mdk_gdiff_core.h's; entries, limits and refusals are mdk_diff_core.h's.  The code object, the md_stats handle, its stream, its status
// word and its error text are mdk_qdiff.hip's.
//
// One synchronous call and one kernel:
//   k_gdiff  a lane per site, 256 per workgroup: k_qdiff's layout, for the reason recorded there.  `order` holds the samples in the rule's
//            visiting order -- group 0's ascending, then group 1's, ... -- and `group_end` the G cumulative ends of the groups in it; both
//            are the same in every lane, so their loads are uniform, and the loop over the groups has a wave-uniform index.  A lane keeps
//            NO array by group: what it has to remember of a group goes to the [G, n] output matrices, which are outputs anyway.
//            pass 1  group after group: the site's entries of the group's samples, row after row -- every row read coalesced along n --,
//                    each entry checked and pooled in 64 bits, the covered samples counted; the group's pooled pair stored coalesced to
//                    row g of nmeth_g / nunmeth_g; K, M, the covered groups and samples and the two extremes (index and pair) kept in
//                    registers.  Then the margins checked.  A refusal: (site << 8 | bit) into the status by atomicMin, the kernel's one
//                    atomic; the site's outputs are those of a site without anything to test -- its column of the two matrices zeroed
//                    again --, and it is not tested
//            pass 2  not for a site without anything to test.  Group after group: the pooled pair read back (16 bytes a lane, coalesced;
//                    the lane's own store), the group's term of the score added -- or, with two covered groups, qdiff_score of the two --,
//                    and, for a group whose pooled counts are both above 0, its rows once more for qdiff_term of every covered sample
//            test    gdiff_site on the lane, the eight outputs and `steps` stored coalesced
// Per site 8 S bytes read twice (int32 matrices) and 16 G + 48 written, 16 G read back.  Nothing is read outside the named rows of the
// two matrices, `order` and `group_end`, nothing written outside the outputs.  Plain C++, vector loads and stores, no LDS, no scratch.
#include "mdk_gdiff_core.h"

struct KGdiff {
    const void *m, *u; const int32_t *order, *group_end; int32_t n_groups; int64_t n; double min_dispersion;
    int64_t *gm, *gu; double *diff; int32_t *lo, *hi; double *p; int32_t *df, *dfg; double *dispersion, *statistic; uint32_t *steps;
    StatsStatus *st;
};

template <typename T>
__global__ __launch_bounds__(QDIFF_WG) void k_gdiff(const KGdiff A) {
    MDK_DIFF_NO_CONTRACT
    const int64_t i = (int64_t)blockIdx.x * QDIFF_WG + threadIdx.x;
    if(i >= A.n) return;
    const T *const Mm = (const T *)A.m, *const Uu = (const T *)A.u;
    const int32_t *const __restrict__ order = A.order, *const __restrict__ group_end = A.group_end;
    const int32_t G = A.n_groups;
    int64_t K = 0, M = 0, lo_m = 0, lo_n = 0, hi_m = 0, hi_n = 0; int32_t g_eff = 0, k = 0, lo = -1, hi = -1; uint32_t err = 0, margin = 0;
    for(int32_t g = 0, s = 0; g < G; g++) {                    // (g, s and end are the same for every lane)
        const int32_t end = group_end[g];
        int64_t a = 0, b = 0; int32_t kg = 0;
        for(; s < end; s++) {
            const int64_t at = (int64_t)order[s] * A.n + i;
            const int64_t m = (int64_t)Mm[at], u = (int64_t)Uu[at];
            const uint32_t e = diff_entry_check(m) | diff_entry_check(u);
            err |= e;
            if(!e) { a += m; b += u; kg += m + u > 0; }         // (a refused entry is not added: the sums stay below 2^37)
        }
        A.gm[(int64_t)g * A.n + i] = a; A.gu[(int64_t)g * A.n + i] = b;
        margin |= gdiff_margin_check(a + b, 0, 0);
        if(a + b == 0) continue;
        K += a; M += b; k += kg; g_eff++;
        if(lo < 0 || gdiff_below(a, a + b, lo_m, lo_n)) { lo = g; lo_m = a; lo_n = a + b; }
        if(hi < 0 || gdiff_below(hi_m, hi_n, a, a + b)) { hi = g; hi_m = a; hi_n = a + b; }
    }
    if(!err) err = margin | gdiff_margin_check(0, K, M);
    if(err) {
        atomicMin(&A.st->first, ((unsigned long long)i << 8) | (unsigned long long)(__ffs(err) - 1));
        for(int32_t g = 0; g < G; g++) { A.gm[(int64_t)g * A.n + i] = 0; A.gu[(int64_t)g * A.n + i] = 0; }
        A.diff[i] = 0.0; A.lo[i] = -1; A.hi[i] = -1;
        A.p[i] = 1.0; A.df[i] = 0; A.dfg[i] = 0; A.dispersion[i] = 1.0; A.statistic[i] = 0.0;
        if(A.steps) A.steps[i] = 0;
        return;                                                // (not tested: its margins may be past what the rule takes)
    }
    double X = 0.0, pearson = 0.0;
    const int32_t nu = k - (g_eff > 2 ? g_eff : 2);
    if(g_eff >= 2 && nu >= 1 && K > 0 && M > 0) {
        int64_t first_m = 0, first_u = 0; int32_t seen = 0;
        for(int32_t g = 0; g < G; g++) {
            const int64_t a = A.gm[(int64_t)g * A.n + i], b = A.gu[(int64_t)g * A.n + i];
            if(a + b > 0) {
                if(g_eff != 2) X = X + gdiff_score_term(a, b, K, M);
                else if(!seen) { first_m = a; first_u = b; }
                else X = qdiff_score(first_m, first_u, a, b);
                seen++;
            }
            if(a > 0 && b > 0) {                               // a group all methylated or all unmethylated contributes nothing
                const int32_t end = group_end[g];
                for(int32_t s = g ? group_end[g - 1] : 0; s < end; s++) {
                    const int64_t at = (int64_t)order[s] * A.n + i;
                    const int64_t m = (int64_t)Mm[at], u = (int64_t)Uu[at];
                    if(m + u > 0) pearson = pearson + qdiff_term(m, u, a, b);
                }
            }
        }
    }
    gdiff_result r;
    gdiff_site(g_eff, k, K, M, X, pearson, A.min_dispersion, &r);
    A.diff[i] = lo < 0 ? 0.0 : diff_meth(lo_m, lo_n - lo_m, hi_m, hi_n - hi_m);
    A.lo[i] = lo; A.hi[i] = hi;
    A.p[i] = r.p; A.df[i] = r.df; A.dfg[i] = r.df_groups; A.dispersion[i] = r.dispersion; A.statistic[i] = r.statistic;
    if(A.steps) A.steps[i] = r.steps;
}

extern "C" int md_stats_gdiff(md_stats *h, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n,
                              const int32_t *order, const int32_t *group_end, int32_t n_groups, double min_dispersion,
                              int64_t *nmeth_g, int64_t *nunmeth_g, double *meth_diff, int32_t *group_lo, int32_t *group_hi,
                              double *pvalue, int32_t *df, int32_t *df_groups, double *dispersion, double *statistic, uint32_t *steps) {
    const char *const what = "md_stats_gdiff";
    if(!h || !order || !group_end || (elem_bytes != 4 && elem_bytes != 8) || n_samples < 1 || n_samples > DIFF_MAX_SAMPLES || n < 0 || n > DIFF_MAX_SITES)
        return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    if(n && (!nmeth || !nunmeth || !nmeth_g || !nunmeth_g || !meth_diff || !group_lo || !group_hi || !pvalue || !df || !df_groups || !dispersion || !statistic))
        return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    if(!(min_dispersion >= 0x1p-55 && min_dispersion <= 0x1p800)) {
        snprintf(g_err, sizeof g_err, "%s: min_dispersion must be within 2^-55 and 2^800", what);
        return MD_STATS_ERR_ARG;
    }
    if(n_groups < 2 || n_groups > n_samples) {
        snprintf(g_err, sizeof g_err, "%s: %d groups: 2 to %d, the samples of the matrices", what, (int)n_groups, (int)n_samples);
        return MD_STATS_ERR_ARG;
    }
    // the ends and the order: few, and the kernel trusts them
    for(int32_t g = 0; g < n_groups; g++) {
        const int32_t from = g ? group_end[g - 1] : 0;
        if(group_end[g] < from) {
            snprintf(g_err, sizeof g_err, "%s: group_end is not ascending at group %d", what, (int)g);
            return MD_STATS_ERR_ARG;
        }
        if(group_end[g] == from) {
            snprintf(g_err, sizeof g_err, "%s: group %d has no sample", what, (int)g);
            return MD_STATS_ERR_ARG;
        }
        if(group_end[g] > n_samples) {
            snprintf(g_err, sizeof g_err, "%s: the groups name %d samples or more, the matrices hold %d: a sample is named twice", what, (int)group_end[g], (int)n_samples);
            return MD_STATS_ERR_ARG;
        }
    }
    const int32_t n_all = group_end[n_groups - 1];
    bool seen[DIFF_MAX_SAMPLES];
    memset(seen, 0, sizeof seen);
    for(int32_t g = 0, k = 0; g < n_groups; g++)
        for(; k < group_end[g]; k++) {
            const int32_t s = order[k];
            if(s < 0 || s >= n_samples) {
                snprintf(g_err, sizeof g_err, "%s: group %d names sample %d: the matrices hold samples 0 to %d", what, (int)g, (int)s, (int)n_samples - 1);
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
    memcpy(h->pin->order, order, (size_t)n_all * sizeof(int32_t));
    memcpy(h->pin->group_end, group_end, (size_t)n_groups * sizeof(int32_t));
    SIDECHK(hipMemcpyAsync(h->d_order, h->pin->order, (size_t)n_all * sizeof(int32_t), hipMemcpyHostToDevice, h->st));
    SIDECHK(hipMemcpyAsync(h->d_group_end, h->pin->group_end, (size_t)n_groups * sizeof(int32_t), hipMemcpyHostToDevice, h->st));
    SIDE_STATUS_UP(h, &h->pin->st, StatsStatus);
    KGdiff A;
    A.m = nmeth; A.u = nunmeth; A.order = h->d_order; A.group_end = h->d_group_end; A.n_groups = n_groups; A.n = n; A.min_dispersion = min_dispersion;
    A.gm = nmeth_g; A.gu = nunmeth_g; A.diff = meth_diff; A.lo = group_lo; A.hi = group_hi; A.p = pvalue; A.df = df; A.dfg = df_groups;
    A.dispersion = dispersion; A.statistic = statistic; A.steps = steps; A.st = h->d_st;
    const dim3 grid((uint32_t)((n + QDIFF_WG - 1) / QDIFF_WG));
    if(elem_bytes == 4) hipLaunchKernelGGL(k_gdiff<int32_t>, grid, dim3(QDIFF_WG), 0, h->st, A);
    else hipLaunchKernelGGL(k_gdiff<int64_t>, grid, dim3(QDIFF_WG), 0, h->st, A);
    SIDECHK(hipGetLastError());
    SIDE_STATUS_DOWN(h, &h->pin->st, StatsStatus);
    const unsigned long long first = h->pin->st.first;
    if(first == ~0ull) return 0;
    const uint32_t bit = 1u << (first & 0xffu);
    snprintf(g_err, sizeof g_err, "%s: %s (site %lld)", what,
             bit == DIFF_E_NEGATIVE ? "a count is negative" :
             bit == DIFF_E_ENTRY ? "a count is 2^26 or more" : "a pooled margin (a group's depth, or the methylated or the unmethylated of all) is 2^26 or more",
             (long long)(first >> 8));
    return MD_STATS_ERR_ARG;
}

// a design's tested columns given the others -- covariates --: the library's last call, on the same handle
#include "mdk_mdiff.hip"
