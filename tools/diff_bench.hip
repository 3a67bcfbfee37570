// diff_bench.hip -- TEST INFRASTRUCTURE: k_diff (csrc/mdk_diff.hip) timed on the table DESIGN.md section 4 records: 2^22 sites, two samples,
// pooled depths drawn uniformly from 10 to 200 with one site in 1,000 at 5,000, both groups at one methylation level drawn per site.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Imethyldackel_amd/csrc -o tools/_build/diff_bench tools/diff_bench.hip
//   diff_bench [sites]
// The kernel is launched as md_text_diff launches it, on a stream of its own: 3 launches to warm up, then 10 timed one by one between
// two events; the median, the smallest and the largest are printed, and the p-values of every 4099th site are compared with the host
// build of the same header, bit for bit.  The library's source is compiled in (its two helpers are given here), so what is timed is
// the tree's kernel, not a copy.
#include "../methyldackel_amd/csrc/mdk_diff.hip"
#include <algorithm>
#include <random>
#include <vector>
#include <string.h>

static char errbuf[MDK_ERR_BYTES];
char *mdk_err_buf() { return errbuf; }
int fail(int code, const char *what, hipError_t e) { fprintf(stderr, "%s: %d (%s)\n", what, code, hipGetErrorString(e)); return code; }

#define CK(x) do { hipError_t e_ = (x); if(e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while(0)

int main(int argc, char **argv) {
    const int64_t N = argc > 1 ? atoll(argv[1]) : 1ll << 22;
    if(N < 1 || N > DIFF_MAX_SITES) { fprintf(stderr, "usage: diff_bench [sites]\n"); return 2; }
    const int S = 2;
    std::vector<int32_t> m((size_t)S * N), u((size_t)S * N);
    std::mt19937_64 rng(12345);
    double mean_depth = 0;
    for(int64_t i = 0; i < N; i++) {
        const int depth = (rng() % 1000 == 0) ? 5000 : 10 + (int)(rng() % 191);
        const int na = depth / 2, nb = depth - na;
        const double level = (double)(rng() >> 11) / 9007199254740992.0;
        std::binomial_distribution<int> A(na, level), B(nb, level);
        const int ma = A(rng), mb = B(rng);
        m[i] = ma; u[i] = na - ma; m[N + i] = mb; u[N + i] = nb - mb;
        mean_depth += depth;
    }
    printf("sites %lld samples %d mean pooled depth %.1f\n", (long long)N, S, mean_depth / N);
    int32_t *dm, *du, *dg; int64_t *o[4]; double *dd, *dp; TextStatus *st;
    CK(hipMalloc(&dm, m.size() * 4)); CK(hipMalloc(&du, u.size() * 4)); CK(hipMalloc(&dg, S * 4)); CK(hipMalloc(&st, sizeof(TextStatus)));
    for(int q = 0; q < 4; q++) CK(hipMalloc(&o[q], N * 8));
    CK(hipMalloc(&dd, N * 8)); CK(hipMalloc(&dp, N * 8));
    const int32_t marks[2] = {0, 1};
    CK(hipMemcpy(dm, m.data(), m.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(du, u.data(), u.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dg, marks, 8, hipMemcpyHostToDevice));
    CK(hipMemset(st, 0, sizeof(TextStatus)));
    KDiff K; K.m = dm; K.u = du; K.group = dg; K.n_samples = S; K.n = N; K.a = o[0]; K.b = o[1]; K.c = o[2]; K.d = o[3]; K.diff = dd; K.p = dp; K.st = st;
    hipStream_t s; CK(hipStreamCreate(&s));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const dim3 grid((uint32_t)((N + DIFF_WG - 1) / DIFF_WG));
    for(int w = 0; w < 3; w++) hipLaunchKernelGGL(k_diff<int32_t>, grid, dim3(DIFF_WG), 0, s, K);
    CK(hipStreamSynchronize(s)); CK(hipGetLastError());
    std::vector<float> ms;
    for(int it = 0; it < 10; it++) {
        CK(hipEventRecord(e0, s)); hipLaunchKernelGGL(k_diff<int32_t>, grid, dim3(DIFF_WG), 0, s, K); CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1));
        float t; CK(hipEventElapsedTime(&t, e0, e1)); ms.push_back(t);
    }
    CK(hipGetLastError());
    std::sort(ms.begin(), ms.end());
    printf("k_diff<int32_t>: median %.3f ms, min %.3f, max %.3f (10 launches after 3)\n", ms[5], ms[0], ms[9]);
    std::vector<double> got((size_t)N);
    CK(hipMemcpy(got.data(), dp, N * 8, hipMemcpyDeviceToHost));
    int bad = 0; int64_t seen = 0;
    for(int64_t i = 0; i < N; i += 4099, seen++) { const double p = diff_pvalue(m[i], u[i], m[N + i], u[N + i], nullptr); if(memcmp(&p, &got[i], 8)) bad++; }
    TextStatus hst; CK(hipMemcpy(&hst, st, sizeof hst, hipMemcpyDeviceToHost));
    printf("host header against device on %lld sites: %d differ; status err %u\n", (long long)seen, bad, hst.err);
    return bad || hst.err ? 1 : 0;
}
