// profile_emu.cpp -- TEST INFRASTRUCTURE: the count profile (csrc/mdk_profile_core.h) executed on the host: every cell made one word by
// prof_cell, as the kernel makes it, and counted site after site.
//   build: g++ -O2 -Wall -o tools/_build/profile_emu tools/profile_emu.cpp -Imethyldackel_amd/csrc
//   profile_emu < jobs.txt > results.tsv
//       the input holds jobs, one after the other, all numbers decimal and separated by white space:
//         P S N G MIN_DEPTH B L HAS_GROUP      a table: then S x N pairs `nmeth nunmeth`, sample-major, and, if HAS_GROUP is 1, N groups
//       The output holds per job a line `err at` -- the refusal's bit (MOM_E_NEGATIVE, MOM_E_ENTRY, PROF_E_GROUP) and its site, `0 -1`
//       without one.  For an accepted table three lines follow per sample and group, sample-major: the B + 1 depth bins, the L level
//       bins, and `nmeth_sum nunmeth_sum max_depth`, decimal and tab-separated.
// Exit 0; 2 for input that is no job.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "mdk_profile_core.h"

int main(int argc, char **argv) {
    if(argc > 1) { fprintf(stderr, "usage: profile_emu < jobs.txt > results.tsv\n"); return 2; }
    char kind[8]; int32_t S;
    while(scanf("%7s %" SCNd32, kind, &S) == 2) {
        if(S < 1 || S > MOM_MAX_SAMPLES || strcmp(kind, "P")) { fprintf(stderr, "not a job's first line\n"); return 2; }
        int64_t N, min_depth; int32_t G, B, L, has_group;
        if(scanf("%" SCNd64 " %" SCNd32 " %" SCNd64 " %" SCNd32 " %" SCNd32 " %" SCNd32, &N, &G, &min_depth, &B, &L, &has_group) != 6 || N < 0 || N > (1 << 24) ||
           G < 1 || G > PROF_MAX_GROUPS || min_depth < 1 || min_depth >= MOM_LIMIT || B < 1 || B > PROF_MAX_DEPTH_BINS || L < 1 || L > PROF_MAX_LEVEL_BINS || (has_group != 0 && has_group != 1)) {
            fprintf(stderr, "not a table's first line\n"); return 2;
        }
        std::vector<int64_t> m((size_t)S * N), u((size_t)S * N);
        std::vector<uint32_t> group((size_t)N, 0u);
        for(size_t at = 0; at < (size_t)S * N; at++) if(scanf("%" SCNd64 " %" SCNd64, &m[at], &u[at]) != 2) { fprintf(stderr, "not a table: entry %zu\n", at); return 2; }
        if(has_group) for(size_t k = 0; k < (size_t)N; k++) if(scanf("%" SCNu32, &group[k]) != 1 || group[k] > 255) { fprintf(stderr, "not a group: site %zu\n", k); return 2; }
        const size_t cells = (size_t)S * G;
        std::vector<int64_t> dh(cells * (B + 1), 0), lh(cells * L, 0), ms(cells, 0), us(cells, 0), mx(cells, 0);
        uint64_t first = ~0ull;
        for(int64_t k = 0; k < N; k++) {
            uint32_t err = prof_group_check(group[k], G);
            const bool site_ok = !err;
            for(int s = 0; s < S; s++) {
                const int64_t a = m[(size_t)s * N + k], b = u[(size_t)s * N + k];
                const uint32_t w = prof_cell(a, b, min_depth, B, L, &err);
                if(w == PROF_REFUSED || !site_ok) continue;
                const size_t to = (size_t)s * G + group[k];
                dh[to * (B + 1) + (w & PROF_DEPTH_MASK)]++;
                if(a + b > mx[to]) mx[to] = a + b;
                if((w >> PROF_COVERED_BIT) & 1u) { lh[to * L + (w >> 16)]++; ms[to] += a; us[to] += b; }
            }
            if(err) { const uint64_t key = mom_refusal_key(k, err); if(key < first) first = key; }
        }
        if(first != ~0ull) { printf("%u\t%lld\n", 1u << (first & 0xffu), (long long)(first >> 8)); continue; }
        printf("0\t-1\n");
        for(size_t to = 0; to < cells; to++) {
            for(int b = 0; b <= B; b++) printf("%" PRId64 "%c", dh[to * (B + 1) + b], b < B ? '\t' : '\n');
            for(int l = 0; l < L; l++) printf("%" PRId64 "%c", lh[to * L + l], l + 1 < L ? '\t' : '\n');
            printf("%" PRId64 "\t%" PRId64 "\t%" PRId64 "\n", ms[to], us[to], mx[to]);
        }
    }
    return 0;
}
