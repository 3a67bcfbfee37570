// moments_emu.cpp -- TEST INFRASTRUCTURE: the pairwise sample moments and their centring (csrc/mdk_moments_core.h) executed on the host:
// every cell quantised by mom_cell, the sums formed site after site as the kernels' mom_add forms them, centred by mom_cxy and mom_vxx.
//   build: g++ -O2 -Wall -o tools/_build/moments_emu tools/moments_emu.cpp -Imethyldackel_amd/csrc
//   moments_emu < jobs.txt > results.tsv
//       the input holds jobs, one after the other, all numbers decimal and separated by white space:
//         T S N MIN_DEPTH        a table: then S x N pairs `nmeth nunmeth`, sample-major
//         C S                    sums to centre: then four S x S matrices n, sx, sxx, sxy, row-major
//       The output holds per job a line `err at` -- the MOM_E_* bit and the site (T) or the MOM_E_SUM_* bit and the cell (C) of the refusal
//       that is reported, `0 -1` without one.  For an accepted table four S x S matrices follow, n, sx, sxx and sxy, a line per row,
//       decimal; and for either kind, accepted, two more, cxy and vxx, the doubles as the 16 hexadecimal digits of their 64-bit patterns.
// Exit 0; 2 for input that is no job.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "mdk_moments_core.h"

static uint64_t pattern(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }

static void print_ints(const std::vector<int64_t> &v, int S) {
    for(int i = 0; i < S; i++) for(int j = 0; j < S; j++) printf("%" PRId64 "%c", v[(size_t)i * S + j], j + 1 < S ? '\t' : '\n');
}

// the sums checked and centred; what is printed after an accepted job's sums
static bool center(const std::vector<int64_t> &n, const std::vector<int64_t> &sx, const std::vector<int64_t> &sxx, const std::vector<int64_t> &sxy, int S, bool report) {
    uint64_t first = ~0ull;
    for(int at = 0; at < S * S; at++) {
        const uint32_t err = mom_sums_check(n[at], sx[at], sxx[at], sxy[at]);
        if(err) { const uint64_t key = mom_refusal_key(at, err); if(key < first) first = key; }
    }
    if(first != ~0ull) { printf("%u\t%lld\n", 1u << (first & 0xffu), (long long)(first >> 8)); return false; }
    if(report) printf("0\t-1\n");
    return true;
}
static void print_centred(const std::vector<int64_t> &n, const std::vector<int64_t> &sx, const std::vector<int64_t> &sxx, const std::vector<int64_t> &sxy, int S) {
    for(int i = 0; i < S; i++) for(int j = 0; j < S; j++) {
        const size_t at = (size_t)i * S + j;
        printf("%016" PRIx64 "%c", pattern(mom_cxy(n[at], sxy[at], sx[at], sx[(size_t)j * S + i])), j + 1 < S ? '\t' : '\n');
    }
    for(int i = 0; i < S; i++) for(int j = 0; j < S; j++) {
        const size_t at = (size_t)i * S + j;
        printf("%016" PRIx64 "%c", pattern(mom_vxx(n[at], sxx[at], sx[at])), j + 1 < S ? '\t' : '\n');
    }
}

int main(int argc, char **argv) {
    if(argc > 1) { fprintf(stderr, "usage: moments_emu < jobs.txt > results.tsv\n"); return 2; }
    char kind[8]; int32_t S;
    while(scanf("%7s %" SCNd32, kind, &S) == 2) {
        if(S < 1 || S > MOM_MAX_SAMPLES || (strcmp(kind, "T") && strcmp(kind, "C"))) { fprintf(stderr, "not a job's first line\n"); return 2; }
        const size_t cells = (size_t)S * S;
        std::vector<int64_t> n(cells, 0), sx(cells, 0), sxx(cells, 0), sxy(cells, 0);
        if(kind[0] == 'C') {
            std::vector<int64_t> *const all[4] = { &n, &sx, &sxx, &sxy };
            for(int q = 0; q < 4; q++) for(size_t at = 0; at < cells; at++) if(scanf("%" SCNd64, &(*all[q])[at]) != 1) { fprintf(stderr, "not sums: matrix %d entry %zu\n", q, at); return 2; }
            if(center(n, sx, sxx, sxy, S, true)) print_centred(n, sx, sxx, sxy, S);
            continue;
        }
        int64_t N, min_depth;
        if(scanf("%" SCNd64 " %" SCNd64, &N, &min_depth) != 2 || N < 0 || N > (1 << 24) || min_depth < 1 || min_depth >= MOM_LIMIT) { fprintf(stderr, "not a table's first line\n"); return 2; }
        std::vector<int64_t> m((size_t)S * N), u((size_t)S * N);
        for(size_t at = 0; at < (size_t)S * N; at++) if(scanf("%" SCNd64 " %" SCNd64, &m[at], &u[at]) != 2) { fprintf(stderr, "not a table: entry %zu\n", at); return 2; }
        uint64_t first = ~0ull;
        std::vector<uint32_t> w(S);
        for(int64_t k = 0; k < N; k++) {
            uint32_t err = 0;
            for(int s = 0; s < S; s++) w[s] = mom_cell(m[(size_t)s * N + k], u[(size_t)s * N + k], min_depth, &err);
            if(err) { const uint64_t key = mom_refusal_key(k, err); if(key < first) first = key; }
            for(int i = 0; i < S; i++) {
                const uint32_t xi = w[i] & MOM_LEVEL_MASK, ci = w[i] >> MOM_COVERED_BIT;
                for(int j = 0; j < S; j++) {
                    const uint32_t xj = w[j] & MOM_LEVEL_MASK, cj = w[j] >> MOM_COVERED_BIT;
                    const uint32_t xm = cj ? xi : 0u;
                    const size_t at = (size_t)i * S + j;
                    n[at] += ci & cj; sx[at] += xm; sxx[at] += (int64_t)((uint64_t)xm * xi); sxy[at] += (int64_t)((uint64_t)xi * xj);
                }
            }
        }
        if(first != ~0ull) { printf("%u\t%lld\n", 1u << (first & 0xffu), (long long)(first >> 8)); continue; }
        printf("0\t-1\n");
        print_ints(n, S); print_ints(sx, S); print_ints(sxx, S); print_ints(sxy, S);
        if(center(n, sx, sxx, sxy, S, false)) print_centred(n, sx, sxx, sxy, S);
    }
    return 0;
}
