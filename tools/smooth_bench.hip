// smooth_bench.hip -- TEST INFRASTRUCTURE: k_smooth_window and k_smooth_sum (csrc/mdk_smooth.hip) timed on the table DESIGN.md section 4
// records: 2^22 sites on 4 contigs of equal size, 6 samples of int32 counts, the steps between neighbouring starts drawn uniformly from
// 1 to 199 (mean spacing 100 bases), depths 0 to 30 with a tenth of the entries uncovered; seeded.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Imethyldackel_amd/csrc -o tools/_build/smooth_bench tools/smooth_bench.hip
//   smooth_bench [sites [half_bases min_sites kernel [tile_sites chunk_sites sample_batch]]]      defaults: 2^22, 1000 70 0 (tricube), 0 0 0
// One md_smooth_run first: the call as a user makes it, which also sizes the handle's scratch and must be accepted.  Then the two kernels
// as that call launches them, on the handle's stream: 3 rounds to warm up, 9 timed, each kernel between two events; the medians are
// printed with the pairs (the sum of nsites times the samples) per second, the bytes the algorithm needs, and the least time the
// hardware could take.  Every 4099th site is compared with the host build of the same header, bit for bit.  The library's source is
// compiled in, so what is timed is the tree's kernels, not a copy.
#include "../methyldackel_amd/csrc/mdk_smooth.hip"
#include <algorithm>
#include <random>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if(e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while(0)
#define HBM_MEASURED_TBS 6.29            // what a float4 copy reaches on an MI355X, 79 % of the 8.0 TB/s of the specification

int main(int argc, char **argv) {
    const int64_t N = argc > 1 ? atoll(argv[1]) : 1ll << 22;
    const int32_t half_bases = argc > 4 ? atoi(argv[2]) : 1000, min_sites = argc > 4 ? atoi(argv[3]) : 70, kernel = argc > 4 ? atoi(argv[4]) : SMO_TRICUBE;
    const int32_t tile = argc > 7 ? atoi(argv[5]) : 0, chunk = argc > 7 ? atoi(argv[6]) : 0, batch = argc > 7 ? atoi(argv[7]) : 0;
    if(N < 4 || N > (1ll << 26)) { fprintf(stderr, "usage: smooth_bench [sites [half_bases min_sites kernel [tile_sites chunk_sites sample_batch]]]\n"); return 2; }
    const int S = 6, CONTIGS = 4;
    std::vector<int32_t> contig(N), start(N), m((size_t)S * N), u((size_t)S * N);
    std::mt19937_64 rng(20240607);
    for(int64_t i = 0, x = 0; i < N; i++) {
        contig[i] = (int32_t)(i * CONTIGS / N);
        if(i && contig[i] != contig[i - 1]) x = 0;
        x += 1 + (int64_t)(rng() % 199);
        start[i] = (int32_t)x;
    }
    for(size_t at = 0; at < (size_t)S * N; at++) {
        if(rng() % 10 == 0) { m[at] = 0; u[at] = 0; continue; }
        const int depth = 1 + (int)(rng() % 30);
        m[at] = (int32_t)(rng() % (depth + 1)); u[at] = depth - m[at];
    }
    int32_t *dc, *dx, *dm, *du, *dn, *dh; double *dl, *dd;
    CK(hipMalloc(&dc, N * 4)); CK(hipMalloc(&dx, N * 4)); CK(hipMalloc(&dm, m.size() * 4)); CK(hipMalloc(&du, u.size() * 4));
    CK(hipMalloc(&dn, N * 4)); CK(hipMalloc(&dh, N * 4)); CK(hipMalloc(&dl, (size_t)S * N * 8)); CK(hipMalloc(&dd, (size_t)S * N * 8));
    CK(hipMemcpy(dc, contig.data(), N * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dx, start.data(), N * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dm, m.data(), m.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(du, u.data(), u.size() * 4, hipMemcpyHostToDevice));
    md_smooth *h;
    if(md_smooth_open(0, &h)) { fprintf(stderr, "%s\n", md_smooth_last_error()); return 1; }
    if(md_smooth_limits(h, tile, chunk, batch, 0)) { fprintf(stderr, "%s\n", md_smooth_last_error()); return 1; }
    if(md_smooth_run(h, dc, dx, dm, du, 4, S, N, half_bases, min_sites, kernel, dl, dd, dn, dh)) { fprintf(stderr, "%s\n", md_smooth_last_error()); return 1; }
    const KSmooth K = smo_arguments(h, dc, dx, dm, du, S, N, half_bases, min_sites, kernel, dl, dd, dn, dh);
    hipEvent_t e0, e1, e2; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1)); CK(hipEventCreate(&e2));
    std::vector<float> tw, ts, tt;
    for(int it = 0; it < 12; it++) {
        CK(hipEventRecord(e0, h->st)); smo_launch_window(h, K); CK(hipEventRecord(e1, h->st)); smo_launch_sum(h, K, 4); CK(hipEventRecord(e2, h->st));
        CK(hipEventSynchronize(e2)); CK(hipGetLastError());
        float a, b, c; CK(hipEventElapsedTime(&a, e0, e1)); CK(hipEventElapsedTime(&b, e1, e2)); CK(hipEventElapsedTime(&c, e0, e2));
        if(it >= 3) { tw.push_back(a); ts.push_back(b); tt.push_back(c); }
    }
    std::sort(tw.begin(), tw.end()); std::sort(ts.begin(), ts.end()); std::sort(tt.begin(), tt.end());
    std::vector<int32_t> nsites(N), half(N); std::vector<double> level((size_t)S * N), depth((size_t)S * N);
    CK(hipMemcpy(nsites.data(), dn, N * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(half.data(), dh, N * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(level.data(), dl, level.size() * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(depth.data(), dd, depth.size() * 8, hipMemcpyDeviceToHost));
    double pairs = 0;
    for(int64_t i = 0; i < N; i++) pairs += nsites[i];
    const double mean_window = pairs / N;
    pairs *= S;
    // what the algorithm needs: the two site columns and the two matrices read once, the four outputs written once
    const double bytes = (double)N * (8.0 + 8.0 * S + 16.0 * S + 8.0);
    // per pair: the weight's conversion, 4 products and a difference (tricube) once, then 2 products and 2 sums per sample -- none fused
    const double flops = pairs / S * (kernel == SMO_TRICUBE ? 7.0 : 0.0) + pairs * 4.0;
    printf("sites %lld samples %d contigs %d half_bases %d min_sites %d kernel %s blocking tile %d chunk %d batch %d: mean window %.1f sites\n", (long long)N, S, CONTIGS,
           (int)half_bases, (int)min_sites, kernel == SMO_TRICUBE ? "tricube" : "flat", (int)K.tile, (int)K.chunk, (int)K.batch, mean_window);
    printf("k_smooth_window: median %.3f ms, min %.3f, max %.3f (9 rounds after 3)\n", tw[4], tw[0], tw[8]);
    printf("k_smooth_sum<int32_t>: median %.3f ms, min %.3f, max %.3f: %.3g pairs/s, %.3g double-precision operations/s\n", ts[4], ts[0], ts[8], pairs / (ts[4] * 1e-3), flops / (ts[4] * 1e-3));
    printf("both: median %.3f ms, min %.3f, max %.3f; algorithmic bytes %.0f (%.3f TB/s over both)\n", tt[4], tt[0], tt[8], bytes, bytes / (tt[4] * 1e-3) / 1e12);
    printf("least possible time: HBM %.3f ms (%.2f TB/s measured peak); no measured f64 vector peak is at hand, so no compute bound and no share of it is given\n",
           bytes / (HBM_MEASURED_TBS * 1e12) * 1e3, HBM_MEASURED_TBS);
    int bad = 0; int64_t seen = 0;
    for(int64_t i = 0; i < N; i += 4099, seen++) {
        int64_t c0, c1;
        smo_contig_run(contig.data(), N, i, &c0, &c1);
        const smo_window w = smo_window_of(start.data(), c0, c1, i, half_bases, min_sites);
        if(nsites[i] != w.hi - w.lo || half[i] != w.half) { bad++; continue; }
        const double inv = smo_inverse(w.half);
        for(int s = 0; s < S; s++) {
            double M = 0.0, D = 0.0;
            for(int64_t j = w.lo; j < w.hi; j++) {
                const int64_t dx = (int64_t)start[j] - start[i];
                const size_t at = (size_t)s * N + j;
                smo_add(smo_weight(kernel, dx < 0 ? -dx : dx, w.half, inv), (double)m[at], (double)((int64_t)m[at] + u[at]), &M, &D);
            }
            const double l = smo_level(M, D);
            if(memcmp(&l, &level[(size_t)s * N + i], 8) || memcmp(&D, &depth[(size_t)s * N + i], 8)) bad++;
        }
    }
    printf("host header against device on %lld sites: %d differ\n", (long long)seen, bad);
    md_smooth_close(h);
    return bad ? 1 : 0;
}
