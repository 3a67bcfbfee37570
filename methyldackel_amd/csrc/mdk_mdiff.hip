// mdk_mdiff.hip -- more of libmdk_stats.so (include/mdk_mdiff.h), the last of mdk_qdiff.hip's chain of includes (mdk_gdiff.hip includes it
// at its own end): a site's counts regressed on a design matrix on the device, the quasi-binomial F test of the design's tested columns
// given the others -- covariates, paired designs, slopes.  The rule is mdk_mdiff_core.h's; entries, limits and refusals are
// mdk_diff_core.h's.  The code object, the md_stats handle, its stream, its status word and its error text are mdk_qdiff.hip's.
//
// One synchronous call and one kernel:
//   k_mdiff<P>  a lane per site, 256 per workgroup: k_qdiff's layout.  `order` holds the used samples in the rule's visiting order and
//            `design` a row of P doubles for each of them; both are the same in every lane, so their loads are uniform and a design row
//            sits in scalar registers.  The width P is the template's: a lane's coefficients, its gradient and the P (P + 1) / 2 entries
//            of its normal matrix are indexed by constants alone, so they are registers, not scratch -- a runtime index into a lane's own
//            array would put it there.  The reduced fit's width r is not known to the compiler: the kernel holds the fits of every
//            width 1 .. P and branches to r's, a branch every lane takes alike.
//            first   the site's entries of the used samples, row after row -- every row read coalesced along n --, each entry checked
//                    and pooled in 64 bits, the covered samples counted; then the margins checked.  A refusal: (site << 8 | bit) into
//                    the status by atomicMin, the kernel's one atomic; the site's outputs are those of a site without anything to
//                    test, and it is not tested
//            fits    mdiff_site<P> on the lane: the rank test's pass, the reduced fit, the full fit, the last pass.  EVERY pass reads the
//                    used rows again, coalesced along n (a lane cannot keep 1024 entries), and so does the step's cap between two
//                    passes; a site of 8 passes reads its rows some 20 times, from L2 after the first.  A wavefront takes as long as
//                    the site of its 64 that needs the most passes
//            store   the P coefficients to coef[P, n], the nine other outputs and `steps`, coalesced
// Nothing is read outside the named rows of the two matrices, `order` and `design`, nothing written outside the outputs.  Plain C++,
// vector loads and stores, no LDS, no scratch.
#include "mdk_mdiff_core.h"

struct KMdiff {
    const void *m, *u; const int32_t *order; const double *design; int32_t n_used, r, wide; int64_t n; double min_dispersion;
    double *coef; int64_t *K, *M; double *p; int32_t *df; double *dispersion, *statistic; uint8_t *flags; int32_t *iterations; uint32_t *steps;
    StatsStatus *st;
};

// a lane's site, as mdk_mdiff_core.h's templates take it
template <int P>
struct MdiffLane {
    const void *m, *u; const int32_t *__restrict__ order; const double *__restrict__ design; int32_t used, wide; int64_t n, i;
    __host__ __device__ int32_t samples() const { return used; }
    __host__ __device__ void entry(int32_t s, int64_t *mm, int64_t *uu) const {
        const int64_t at = (int64_t)order[s] * n + i;          // (order[s] is the same for every lane)
        if(wide) { *mm = ((const int64_t *)m)[at]; *uu = ((const int64_t *)u)[at]; }
        else { *mm = (int64_t)((const int32_t *)m)[at]; *uu = (int64_t)((const int32_t *)u)[at]; }
    }
    __host__ __device__ double x(int32_t s, int a) const { return design[s * P + a]; }
};

template <int P>
__global__ __launch_bounds__(QDIFF_WG) void k_mdiff(const KMdiff A) {
    MDK_DIFF_NO_CONTRACT
    const int64_t i = (int64_t)blockIdx.x * QDIFF_WG + threadIdx.x;
    if(i >= A.n) return;
    const MdiffLane<P> S = { A.m, A.u, A.order, A.design, A.n_used, A.wide, A.n, i };
    int64_t K = 0, M = 0; int32_t k = 0; uint32_t err = 0;
    for(int32_t s = 0; s < A.n_used; s++) {
        int64_t m, u;
        S.entry(s, &m, &u);
        const uint32_t e = diff_entry_check(m) | diff_entry_check(u);
        err |= e;
        if(!e) { K += m; M += u; k += m + u > 0; }              // (a refused entry is not added: the sums stay below 2^37)
    }
    if(!err) err = mdiff_margin_check(K, M);
    double coef[P];
    mdiff_result r;
    if(err) {
        atomicMin(&A.st->first, ((unsigned long long)i << 8) | (unsigned long long)(__ffs(err) - 1));
        K = 0; M = 0;
        r.statistic = 0.0; r.dispersion = 1.0; r.p = 1.0; r.df = 0; r.iterations = 0; r.steps = 0; r.flags = 0;
        MDIFF_UNROLL
        for(int a = 0; a < P; a++) coef[a] = 0.0;              // (not tested: its margins may be past what the rule takes)
    } else mdiff_site<P>(S, A.r, k, K, M, A.min_dispersion, coef, &r);
    MDIFF_UNROLL
    for(int a = 0; a < P; a++) A.coef[(int64_t)a * A.n + i] = coef[a];
    A.K[i] = K; A.M[i] = M;
    A.p[i] = r.p; A.df[i] = r.df; A.dispersion[i] = r.dispersion; A.statistic[i] = r.statistic;
    A.flags[i] = (uint8_t)r.flags; A.iterations[i] = r.iterations;
    if(A.steps) A.steps[i] = r.steps;
}

extern "C" int md_stats_mdiff(md_stats *h, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n,
                              const int32_t *order, int32_t n_used, const double *design, int32_t p, int32_t q, double min_dispersion,
                              double *coef, int64_t *nmeth_all, int64_t *nunmeth_all, double *pvalue, int32_t *df, double *dispersion, double *statistic,
                              uint8_t *flags, int32_t *iterations, uint32_t *steps) {
    const char *const what = "md_stats_mdiff";
    if(!h || !order || !design || (elem_bytes != 4 && elem_bytes != 8) || n_samples < 1 || n_samples > DIFF_MAX_SAMPLES || n < 0 || n > DIFF_MAX_SITES)
        return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    if(n && (!nmeth || !nunmeth || !coef || !nmeth_all || !nunmeth_all || !pvalue || !df || !dispersion || !statistic || !flags || !iterations))
        return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    if(!(min_dispersion >= 0x1p-55 && min_dispersion <= 0x1p800)) {
        snprintf(g_err, sizeof g_err, "%s: min_dispersion must be within 2^-55 and 2^800", what);
        return MD_STATS_ERR_ARG;
    }
    if(p < 2 || p > MDIFF_MAX_COLUMNS) {
        snprintf(g_err, sizeof g_err, "%s: a design of %d columns: 2 to %d", what, (int)p, (int)MDIFF_MAX_COLUMNS);
        return MD_STATS_ERR_ARG;
    }
    if(q < 1 || q >= p) {
        snprintf(g_err, sizeof g_err, "%s: %d tested columns of %d: 1 to %d, a reduced model is left", what, (int)q, (int)p, (int)p - 1);
        return MD_STATS_ERR_ARG;
    }
    if(n_used < 1 || n_used > n_samples) {
        snprintf(g_err, sizeof g_err, "%s: the design names %d samples, the matrices hold %d: a sample is named twice", what, (int)n_used, (int)n_samples);
        return MD_STATS_ERR_ARG;
    }
    // the order and the design: few, and the kernel trusts them
    bool seen[DIFF_MAX_SAMPLES];
    memset(seen, 0, sizeof seen);
    for(int32_t k = 0; k < n_used; k++) {
        const int32_t s = order[k];
        if(s < 0 || s >= n_samples) {
            snprintf(g_err, sizeof g_err, "%s: row %d of the design names sample %d: the matrices hold samples 0 to %d", what, (int)k, (int)s, (int)n_samples - 1);
            return MD_STATS_ERR_ARG;
        }
        if(seen[s]) {
            snprintf(g_err, sizeof g_err, "%s: sample %d is named twice", what, (int)s);
            return MD_STATS_ERR_ARG;
        }
        seen[s] = true;
    }
    for(int64_t k = 0; k < (int64_t)n_used * p; k++)
        if(!(design[k] >= -MDIFF_DESIGN_MAX && design[k] <= MDIFF_DESIGN_MAX)) {                   // (a NaN is in no range)
            snprintf(g_err, sizeof g_err, "%s: the design's entry in row %d, column %d is not a finite number of at most 2^20 in magnitude", what, (int)(k / p), (int)(k % p));
            return MD_STATS_ERR_ARG;
        }
    if(!mdiff_independent(design, n_used, p)) {
        snprintf(g_err, sizeof g_err, "%s: the design's %d columns are dependent over its %d samples (or one of them is empty): no coefficient for every column", what, (int)p, (int)n_used);
        return MD_STATS_ERR_ARG;
    }
    if(!n) return 0;
    SIDECHK(hipSetDevice(h->device));
    // the design's two buffers are made here, at the first call: a handle that fits no model holds what it held before this call existed
    const size_t room = (size_t)DIFF_MAX_SAMPLES * MDIFF_MAX_COLUMNS;
    if(h->d_design.need(room, what) || h->pin_design.need(room, what)) return SIDE_ERR_NOMEM;
    memcpy(h->pin->order, order, (size_t)n_used * sizeof(int32_t));
    memcpy(h->pin_design, design, (size_t)n_used * p * sizeof(double));
    SIDECHK(hipMemcpyAsync(h->d_order, h->pin->order, (size_t)n_used * sizeof(int32_t), hipMemcpyHostToDevice, h->st));
    SIDECHK(hipMemcpyAsync(h->d_design, h->pin_design, (size_t)n_used * p * sizeof(double), hipMemcpyHostToDevice, h->st));
    SIDE_STATUS_UP(h, &h->pin->st, StatsStatus);
    KMdiff A;
    A.m = nmeth; A.u = nunmeth; A.order = h->d_order; A.design = h->d_design; A.n_used = n_used; A.r = p - q; A.wide = elem_bytes == 8; A.n = n;
    A.min_dispersion = min_dispersion;
    A.coef = coef; A.K = nmeth_all; A.M = nunmeth_all; A.p = pvalue; A.df = df; A.dispersion = dispersion; A.statistic = statistic; A.flags = flags;
    A.iterations = iterations; A.steps = steps; A.st = h->d_st;
    const dim3 grid((uint32_t)((n + QDIFF_WG - 1) / QDIFF_WG));
    switch(p) {
    case 2: hipLaunchKernelGGL(k_mdiff<2>, grid, dim3(QDIFF_WG), 0, h->st, A); break;
    case 3: hipLaunchKernelGGL(k_mdiff<3>, grid, dim3(QDIFF_WG), 0, h->st, A); break;
    case 4: hipLaunchKernelGGL(k_mdiff<4>, grid, dim3(QDIFF_WG), 0, h->st, A); break;
    case 5: hipLaunchKernelGGL(k_mdiff<5>, grid, dim3(QDIFF_WG), 0, h->st, A); break;
    case 6: hipLaunchKernelGGL(k_mdiff<6>, grid, dim3(QDIFF_WG), 0, h->st, A); break;
    case 7: hipLaunchKernelGGL(k_mdiff<7>, grid, dim3(QDIFF_WG), 0, h->st, A); break;
    default: hipLaunchKernelGGL(k_mdiff<8>, grid, dim3(QDIFF_WG), 0, h->st, A); break;
    }
    SIDECHK(hipGetLastError());
    SIDE_STATUS_DOWN(h, &h->pin->st, StatsStatus);
    const unsigned long long first = h->pin->st.first;
    if(first == ~0ull) return 0;
    const uint32_t bit = 1u << (first & 0xffu);
    snprintf(g_err, sizeof g_err, "%s: %s (site %lld)", what,
             bit == DIFF_E_NEGATIVE ? "a count is negative" :
             bit == DIFF_E_ENTRY ? "a count is 2^26 or more" : "a pooled margin (the methylated or the unmethylated of all used samples) is 2^26 or more",
             (long long)(first >> 8));
    return MD_STATS_ERR_ARG;
}
