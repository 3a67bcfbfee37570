// profile_bench.hip -- TEST INFRASTRUCTURE: md_stats_profile (csrc/mdk_profile.hip) timed on the tables DESIGN.md section 4 records: 2^22
// sites, S = 1, 6, 12 and 96 samples of int32 counts, G = 1 (no group column) and 3, the default bins (min_depth 1, 1024 depth bins, 20
// level bins).  The counts are made on the device from a hash of (sample, site) with the concentration of a real library: a tenth of the
// cells uncovered, the others' depth binomial(40, 1/4) -- Poisson-like around 10, nine cells in ten within a dozen bins --, the levels
// bimodal: four cells in ten all methylated, three in ten not at all, the rest uniform.  The groups are a hash of the site: 0, 1, 2 in
// the shares 1 : 3 : 12, about those of CpG, CHG and CHH.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Imethyldackel_amd/csrc -o tools/_build/profile_bench tools/profile_bench.hip
//   profile_bench [sites [samples [groups [range_sites band_samples max_workgroups]]]]   defaults: 2^22, all four S, both G, 0 0 0
// Per case one md_stats_profile first: the call as a user makes it, which must be accepted.  Then what that call puts on the stream -- the
// five memsets and the kernel --, between two events: 2 rounds to warm up and 7 timed; the median is printed with the bytes the
// algorithm must read (8 S n, and n more with a group column), their rate and its share of the measured HBM rate.  The first two samples
// are compared with the host build of the same header, exactly.  The library's source is compiled in, so what is timed is the tree's
// kernel, not a copy.
#include "../methyldackel_amd/csrc/mdk_qdiff.hip"
#include <algorithm>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if(e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while(0)
#define HBM_MEASURED_TBS 6.29            // what a float4 copy reaches on an MI355X, 79 % of the 8.0 TB/s of the specification
#define BENCH_B 1024
#define BENCH_L 20

__host__ __device__ static inline uint64_t bench_hash(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull; return x ^ (x >> 31);
}
__host__ __device__ static inline void bench_cell(int64_t at, int32_t *m, int32_t *u) {
    const uint64_t r = bench_hash((uint64_t)at), q = bench_hash(r);
    if(r % 10 == 0) { *m = 0; *u = 0; return; }
    const int32_t depth = __builtin_popcountll(q & bench_hash(q) & ((1ull << 40) - 1));     // (40 bits, each set with probability 1/4)
    const uint64_t kind = (r >> 8) % 10;
    *m = kind < 4 ? depth : kind < 7 ? 0 : (int32_t)((r >> 24) % (uint64_t)(depth + 1)); *u = depth - *m;
}
__host__ __device__ static inline uint8_t bench_group(int64_t k) { const uint64_t r = bench_hash(~(uint64_t)k) % 16; return r < 1 ? 0 : r < 4 ? 1 : 2; }
__global__ void k_bench_fill(int32_t *m, int32_t *u, int64_t cells) {
    for(int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; at < cells; at += (int64_t)gridDim.x * blockDim.x) bench_cell(at, m + at, u + at);
}
__global__ void k_bench_groups(uint8_t *g, int64_t n) {
    for(int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) g[k] = bench_group(k);
}

static int bench(int64_t N, int S, int G, int range, int band, int grid) {
    const int64_t cells = (int64_t)S * N;
    const size_t sg = (size_t)S * G, words = sg * (BENCH_B + 1 + BENCH_L + 3);
    int32_t *dm, *du; uint8_t *dg = nullptr; int64_t *out;
    CK(hipMalloc(&dm, cells * 4)); CK(hipMalloc(&du, cells * 4)); CK(hipMalloc(&out, words * 8));
    hipLaunchKernelGGL(k_bench_fill, dim3(4096), dim3(256), 0, 0, dm, du, cells);
    if(G > 1) { CK(hipMalloc(&dg, N)); hipLaunchKernelGGL(k_bench_groups, dim3(4096), dim3(256), 0, 0, dg, N); }
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    int64_t *const dh = out, *const lh = dh + sg * (BENCH_B + 1), *const ms = lh + sg * BENCH_L, *const us = ms + sg, *const mx = us + sg;
    md_stats *h;
    if(md_stats_open(0, &h)) { fprintf(stderr, "%s\n", md_stats_last_error()); return 1; }
    if(md_stats_profile_limits(h, range, band, grid)) { fprintf(stderr, "%s\n", md_stats_last_error()); return 1; }
    if(md_stats_profile(h, dm, du, 4, S, N, dg, G, 1, BENCH_B, BENCH_L, dh, lh, ms, us, mx)) { fprintf(stderr, "%s\n", md_stats_last_error()); return 1; }
    std::vector<int64_t> first(words), again(words);
    CK(hipMemcpy(first.data(), out, words * 8, hipMemcpyDeviceToHost));
    KProf K;
    K.m = dm; K.u = du; K.group = dg; K.min_depth = 1; K.st = h->d_st;
    K.dh = (unsigned long long *)dh; K.lh = (unsigned long long *)lh; K.ms = (unsigned long long *)ms; K.us = (unsigned long long *)us; K.mx = (unsigned long long *)mx;
    const ProfPlan p = prof_plan(h, S, N, G, BENCH_B, BENCH_L, &K);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int warm = 2, rounds = 7;
    std::vector<float> t;
    for(int it = 0; it < warm + rounds; it++) {
        CK(hipEventRecord(e0, h->st));
        CK(hipMemsetAsync(out, 0, words * 8, h->st));
        CK(prof_launch(h, p, K, G, 4));
        CK(hipEventRecord(e1, h->st));
        CK(hipEventSynchronize(e1)); CK(hipGetLastError());
        float x; CK(hipEventElapsedTime(&x, e0, e1));
        if(it >= warm) t.push_back(x);
    }
    std::sort(t.begin(), t.end());
    CK(hipMemcpy(again.data(), out, words * 8, hipMemcpyDeviceToHost));
    const double med = t[t.size() / 2] * 1e-3, bytes = 8.0 * (double)cells + (G > 1 ? (double)N : 0.0);
    printf("S %d G %d sites %lld: band %d, %lld items of %lld sites, %d workgroups, %zu bytes of LDS: median %.3f ms, min %.3f, max %.3f (%d rounds after %d); %.0f bytes, %.3f TB/s, %.0f %% of the measured HBM rate (%.2f TB/s)\n",
           S, G, (long long)N, p.band, (long long)K.items, (long long)K.range, p.grid, p.lds, med * 1e3, t.front(), t.back(), rounds, warm,
           bytes, bytes / med / 1e12, 100.0 * bytes / med / 1e12 / HBM_MEASURED_TBS, HBM_MEASURED_TBS);
    int bad = again != first;                                    // the timed rounds give the call's tensors
    // the first two samples on the host, from the same hash
    const int seen = S < 2 ? S : 2;
    for(int s = 0; s < seen; s++) {
        std::vector<int64_t> hd((size_t)G * (BENCH_B + 1), 0), hl((size_t)G * BENCH_L, 0), hm(G, 0), hu(G, 0), hx(G, 0);
        for(int64_t k = 0; k < N; k++) {
            int32_t a, b; uint32_t err = 0;
            bench_cell((int64_t)s * N + k, &a, &b);
            const int g = G > 1 ? bench_group(k) : 0;
            const uint32_t w = prof_cell(a, b, 1, BENCH_B, BENCH_L, &err);
            hd[(size_t)g * (BENCH_B + 1) + (w & PROF_DEPTH_MASK)]++;
            if(a + b > hx[g]) hx[g] = a + b;
            if((w >> PROF_COVERED_BIT) & 1u) { hl[(size_t)g * BENCH_L + (w >> 16)]++; hm[g] += a; hu[g] += b; }
        }
        for(int g = 0; g < G; g++) {
            const size_t to = (size_t)s * G + g;
            bad += !std::equal(hd.begin() + (size_t)g * (BENCH_B + 1), hd.begin() + (size_t)(g + 1) * (BENCH_B + 1), first.begin() + to * (BENCH_B + 1));
            bad += !std::equal(hl.begin() + (size_t)g * BENCH_L, hl.begin() + (size_t)(g + 1) * BENCH_L, first.begin() + (lh - out) + to * BENCH_L);
            bad += first[(ms - out) + to] != hm[g] || first[(us - out) + to] != hu[g] || first[(mx - out) + to] != hx[g];
        }
    }
    printf("S %d G %d: host header against device on %d samples and the timed rounds against the call: %d differ\n", S, G, seen, bad);
    md_stats_close(h);
    CK(hipFree(dm)); CK(hipFree(du)); CK(hipFree(out)); if(dg) CK(hipFree(dg));
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    const int64_t N = argc > 1 ? atoll(argv[1]) : 1ll << 22;
    const int only = argc > 2 ? atoi(argv[2]) : 0, only_g = argc > 3 ? atoi(argv[3]) : 0;
    const int range = argc > 6 ? atoi(argv[4]) : 0, band = argc > 6 ? atoi(argv[5]) : 0, grid = argc > 6 ? atoi(argv[6]) : 0;
    if(N < 1 || N > MOM_MAX_SITES || only < 0 || only > MOM_MAX_SAMPLES || only_g < 0 || only_g > PROF_MAX_GROUPS) {
        fprintf(stderr, "usage: profile_bench [sites [samples [groups [range_sites band_samples max_workgroups]]]]\n"); return 2;
    }
    const int all[4] = { 1, 6, 12, 96 }, groups[2] = { 1, 3 };
    int rc = 0;
    for(int q = 0; q < 4 && !rc; q++) if(!only || q == 0)
        for(int j = 0; j < 2 && !rc; j++) if(!only_g || j == 0)
            rc = bench(N, only ? only : all[q], only_g ? only_g : groups[j], range, band, grid);
    return rc;
}
