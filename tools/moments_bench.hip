// moments_bench.hip -- TEST INFRASTRUCTURE: md_stats_moments (csrc/mdk_moments.hip) timed on the tables DESIGN.md section 4 records: 2^22
// sites, S = 2, 12, 96 and 1024 samples of int32 counts made on the device from a hash of (sample, site) -- depths 1 to 30 with a tenth
// of the cells uncovered, the methylated count uniform within the depth.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Imethyldackel_amd/csrc -o tools/_build/moments_bench tools/moments_bench.hip
//   moments_bench [sites [samples [shape chunk_sites pair_tile max_workgroups]]]      defaults: 2^22, all four S, 0 0 0 0
// Per S one md_stats_moments first: the call as a user makes it, which must be accepted.  Then what that call puts on the stream -- the
// four memsets and the kernel --, between two events: 2 rounds to warm up and 7 timed (3 from 512 samples on); the median is printed with
// the pair-sites per second, the bytes the algorithm needs (8 per cell) and, up to 12 samples, the share of the measured HBM rate.  Up to
// 16 pairs are compared with the host build of the same header, exactly.  The library's source is compiled in, so what is timed is the
// tree's kernels, not a copy.
#include "../methyldackel_amd/csrc/mdk_qdiff.hip"
#include <algorithm>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if(e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while(0)
#define HBM_MEASURED_TBS 6.29            // what a float4 copy reaches on an MI355X, 79 % of the 8.0 TB/s of the specification

__host__ __device__ static inline uint64_t bench_hash(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull; return x ^ (x >> 31);
}
__host__ __device__ static inline void bench_cell(int64_t at, int32_t *m, int32_t *u) {
    const uint64_t r = bench_hash((uint64_t)at);
    if(r % 10 == 0) { *m = 0; *u = 0; return; }
    const int32_t depth = 1 + (int32_t)((r >> 8) % 30);
    *m = (int32_t)((r >> 24) % (uint64_t)(depth + 1)); *u = depth - *m;
}
__global__ void k_bench_fill(int32_t *m, int32_t *u, int64_t cells) {
    for(int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; at < cells; at += (int64_t)gridDim.x * blockDim.x) bench_cell(at, m + at, u + at);
}

static int bench(int64_t N, int S, int shape, int chunk, int tile, int grid) {
    const int64_t cells = (int64_t)S * N;
    int32_t *dm, *du; int64_t *out;
    CK(hipMalloc(&dm, cells * 4)); CK(hipMalloc(&du, cells * 4)); CK(hipMalloc(&out, (size_t)4 * S * S * 8));
    hipLaunchKernelGGL(k_bench_fill, dim3(4096), dim3(256), 0, 0, dm, du, cells);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    int64_t *const on = out, *const osx = out + (size_t)S * S, *const osxx = out + (size_t)2 * S * S, *const osxy = out + (size_t)3 * S * S;
    md_stats *h;
    if(md_stats_open(0, &h)) { fprintf(stderr, "%s\n", md_stats_last_error()); return 1; }
    if(md_stats_moments_limits(h, shape, chunk, tile, grid)) { fprintf(stderr, "%s\n", md_stats_last_error()); return 1; }
    if(md_stats_moments(h, dm, du, 4, S, N, 1, on, osx, osxx, osxy)) { fprintf(stderr, "%s\n", md_stats_last_error()); return 1; }
    std::vector<int64_t> first((size_t)4 * S * S), again((size_t)4 * S * S);
    CK(hipMemcpy(first.data(), out, first.size() * 8, hipMemcpyDeviceToHost));
    KMom K;
    K.m = dm; K.u = du; K.min_depth = 1; K.st = h->d_st;
    K.on = (unsigned long long *)on; K.osx = (unsigned long long *)osx; K.osxx = (unsigned long long *)osxx; K.osxy = (unsigned long long *)osxy;
    const MomPlan p = mom_plan(h, S, N, &K);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int warm = 2, rounds = S >= 512 ? 3 : 7;
    std::vector<float> ms;
    for(int it = 0; it < warm + rounds; it++) {
        CK(hipEventRecord(e0, h->st));
        CK(hipMemsetAsync(out, 0, (size_t)4 * S * S * 8, h->st));
        mom_launch(h, p, K, 4);
        CK(hipEventRecord(e1, h->st));
        CK(hipEventSynchronize(e1)); CK(hipGetLastError());
        float t; CK(hipEventElapsedTime(&t, e0, e1));
        if(it >= warm) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    CK(hipMemcpy(again.data(), out, again.size() * 8, hipMemcpyDeviceToHost));
    const double med = ms[ms.size() / 2] * 1e-3, bytes = 8.0 * (double)cells, pair_sites = (double)S * S * (double)N;
    printf("S %d sites %lld: %s t %d, %lld items of %lld sites, %d workgroups, chunk %d: median %.3f ms, min %.3f, max %.3f (%d rounds after %d); %.3g pair-sites/s; %.0f bytes, %.3f TB/s",
           S, (long long)N, p.shape == MOM_SHAPE_LANES ? "k_mom_lanes" : "k_mom_staged", p.t, (long long)K.items, (long long)K.range, p.grid, (int)K.chunk,
           med * 1e3, ms.front(), ms.back(), rounds, warm, pair_sites / med, bytes, bytes / med / 1e12);
    if(S <= 12) printf(", %.0f %% of the measured HBM rate (%.2f TB/s)", 100.0 * bytes / med / 1e12 / HBM_MEASURED_TBS, HBM_MEASURED_TBS);
    printf("\n");
    int bad = again != first;                                    // the timed rounds give the call's matrices
    // some pairs on the host, from the same hash
    int seen = 0;
    for(int q = 0; q < 16 && q < S * S; q++, seen++) {
        const int i = (int)(((int64_t)q * 7919) % S), j = (int)(((int64_t)q * 104729 + q / 3) % S);
        int64_t n = 0, sx = 0, sxx = 0, sxy = 0;
        for(int64_t k = 0; k < N; k++) {
            int32_t mi, ui, mj, uj; uint32_t err = 0;
            bench_cell((int64_t)i * N + k, &mi, &ui); bench_cell((int64_t)j * N + k, &mj, &uj);
            const uint32_t wi = mom_cell(mi, ui, 1, &err), wj = mom_cell(mj, uj, 1, &err);
            const uint32_t xi = wi & MOM_LEVEL_MASK, xj = wj & MOM_LEVEL_MASK, xm = (wj >> MOM_COVERED_BIT) ? xi : 0u;
            n += (wi >> MOM_COVERED_BIT) & (wj >> MOM_COVERED_BIT); sx += xm; sxx += (int64_t)xm * xi; sxy += (int64_t)xi * xj;
        }
        const size_t at = (size_t)i * S + j;
        if(first[at] != n || first[(size_t)S * S + at] != sx || first[(size_t)2 * S * S + at] != sxx || first[(size_t)3 * S * S + at] != sxy) bad++;
    }
    printf("S %d: host header against device on %d pairs and the timed rounds against the call: %d differ\n", S, seen, bad);
    md_stats_close(h);
    CK(hipFree(dm)); CK(hipFree(du)); CK(hipFree(out));
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    const int64_t N = argc > 1 ? atoll(argv[1]) : 1ll << 22;
    const int only = argc > 2 ? atoi(argv[2]) : 0;
    const int shape = argc > 6 ? atoi(argv[3]) : 0, chunk = argc > 6 ? atoi(argv[4]) : 0, tile = argc > 6 ? atoi(argv[5]) : 0, grid = argc > 6 ? atoi(argv[6]) : 0;
    if(N < 1 || N > MOM_MAX_SITES || only < 0 || only > MOM_MAX_SAMPLES) { fprintf(stderr, "usage: moments_bench [sites [samples [shape chunk_sites pair_tile max_workgroups]]]\n"); return 2; }
    const int all[4] = { 2, 12, 96, 1024 };
    int rc = 0;
    for(int q = 0; q < 4 && !rc; q++) if(!only || q == 0) rc = bench(N, only ? only : all[q], shape, chunk, tile, grid);
    return rc;
}
