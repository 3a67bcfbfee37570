// mdk_diff.hip -- two groups of samples compared site by site on the device (include/mdk_hip.h, "two groups compared"): per site the
// groups' pooled counts, the difference of their methylation and the two-sided p-value of Fisher's exact test, from two count matrices
// [S, n] -- a Cohort's, or Regions' sums stacked -- without a file or the host.
//
// The rule is mdk_diff_core.h's: IEEE doubles with *, / and + in one order per site, a multiplication and a division per term, so the
// result is the same bits as the host's (tools/diff_emu) whatever lane a site runs on.  One synchronous call on the md_text handle -- its
// stream and its status block are what this needs; it keeps nothing on the handle and voids no measure -- and one kernel:
//   k_diff   a lane per site, 256 per workgroup.
//            pool    the site's entries of the samples of each group added in 64 bits, one row of the matrices after the other -- every
//                    row read coalesced along n, every entry once --, each entry and then the four margins checked (a refusal: its bit
//                    into the status, the smallest refused site by atomicMin).  The four sums and meth_diff go to the outputs, coalesced
//            test    diff_pvalue on the lane: the walk to the observed table, then the two sums
//            A wavefront takes as long as the deepest of its 64 sites; the device evens that out between wavefronts, eight of them a
//            SIMD.  Dealing terms instead of sites to the lanes of a workgroup was measured and was slower.
// Double-precision division-bound: per site 32 + 8 S bytes (int32 matrices) against some dozens to hundreds of divisions.  Nothing is
// read outside the two matrices and the marks, nothing written outside the six outputs.  Plain C++, vector loads and stores.
#include "mdk_text_internal.hpp"
#include "mdk_diff_core.h"

#define DIFF_WG 256

template <typename T>
__global__ __launch_bounds__(DIFF_WG) void k_diff(const KDiff K) {
    const int64_t i = (int64_t)blockIdx.x * DIFF_WG + threadIdx.x;
    if(i >= K.n) return;
    const T *const M = (const T *)K.m, *const U = (const T *)K.u;
    int64_t a = 0, b = 0, c = 0, d = 0; uint32_t err = 0;
    for(int32_t s = 0; s < K.n_samples; s++) {
        const int32_t g = K.group[s];                          // (the same for every lane)
        if(g < 0) continue;
        const int64_t m = (int64_t)M[(int64_t)s * K.n + i], u = (int64_t)U[(int64_t)s * K.n + i];
        const uint32_t e = diff_entry_check(m) | diff_entry_check(u);
        err |= e;
        if(!e) { if(g == 0) { a += m; b += u; } else { c += m; d += u; } }          // (a refused entry is not added: the sums stay below 2^37)
    }
    if(!err) err = diff_margin_check(a, b, c, d);
    if(err) {
        atomicOr(&K.st->err, err);
        atomicMin(&K.st->first, ((unsigned long long)i << 8) | (unsigned long long)(__ffs(err) - 1));
    }
    K.a[i] = a; K.b[i] = b; K.c[i] = c; K.d[i] = d;
    K.diff[i] = err ? 0.0 : diff_meth(a, b, c, d);
    K.p[i] = err ? 1.0 : diff_pvalue(a, b, c, d, nullptr);     // (a refused site is not tested: its margins may be past what the rule takes)
}

extern "C" int md_text_diff(md_text *t, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n, const int32_t *group,
                            int64_t *nmeth_a, int64_t *nunmeth_a, int64_t *nmeth_b, int64_t *nunmeth_b, double *meth_diff, double *pvalue) {
    const char *const what = "md_text_diff";
    if(!t || !group || (elem_bytes != 4 && elem_bytes != 8) || n_samples < 1 || n_samples > DIFF_MAX_SAMPLES || n < 0 || n > DIFF_MAX_SITES) return fail(MDK_ERR_ARG, what, hipSuccess);
    if(n && (!nmeth || !nunmeth || !nmeth_a || !nunmeth_a || !nmeth_b || !nunmeth_b || !meth_diff || !pvalue)) return fail(MDK_ERR_ARG, what, hipSuccess);
    HIPCHK(hipSetDevice(t->device));
    // the marks: few, and the kernel trusts them
    int32_t marks[DIFF_MAX_SAMPLES]; int in_a = 0, in_b = 0;
    HIPCHK(hipMemcpyAsync(marks, group, (size_t)n_samples * sizeof(int32_t), hipMemcpyDeviceToHost, t->st));
    HIPCHK(hipStreamSynchronize(t->st));
    for(int32_t s = 0; s < n_samples; s++) {
        if(marks[s] < -1 || marks[s] > 1) {
            snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: the mark of sample %d is %d: 0 (group A), 1 (group B) or -1 (not used)", what, (int)s, (int)marks[s]);
            return MDK_ERR_ARG;
        }
        in_a += marks[s] == 0; in_b += marks[s] == 1;
    }
    if(!in_a || !in_b) {
        snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: group %s has no sample", what, in_a ? "B" : "A");
        return MDK_ERR_ARG;
    }
    if(!n) return 0;
    KDiff K;
    K.m = nmeth; K.u = nunmeth; K.group = group; K.n_samples = n_samples; K.n = n;
    K.a = nmeth_a; K.b = nunmeth_a; K.c = nmeth_b; K.d = nunmeth_b; K.diff = meth_diff; K.p = pvalue; K.st = t->d_st;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    HIPCHK(hipMemsetAsync(&t->d_st->first, 0xff, sizeof(t->d_st->first), t->st));
    const dim3 grid((uint32_t)((n + DIFF_WG - 1) / DIFF_WG));
    if(elem_bytes == 4) hipLaunchKernelGGL(k_diff<int32_t>, grid, dim3(DIFF_WG), 0, t->st, K);
    else hipLaunchKernelGGL(k_diff<int64_t>, grid, dim3(DIFF_WG), 0, t->st, K);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(t->h_st, t->d_st, sizeof(TextStatus), hipMemcpyDeviceToHost, t->st));
    HIPCHK(hipStreamSynchronize(t->st));
    const uint32_t err = t->h_st->err;
    if(!err) return 0;
    const uint32_t bit = 1u << (t->h_st->first & 0xffu);
    snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: %s (site %lld)", what,
             bit == DIFF_E_NEGATIVE ? "a count is negative" :
             bit == DIFF_E_ENTRY ? "a count is 2^26 or more" : "a pooled margin (a group's depth, or the methylated or the unmethylated of both) is 2^26 or more",
             (long long)(t->h_st->first >> 8));
    return MDK_ERR_ARG;
}
