// qdiff_emu.cpp -- TEST INFRASTRUCTURE: the quasi-binomial F test of two groups of replicates per site (csrc/mdk_qdiff_core.h) executed on
// the host, a site as a kernel would take it: the entries checked and pooled, then the group rows once more for Pearson's terms.
//   build: g++ -O2 -ffp-contract=off -o tools/_build/qdiff_emu tools/qdiff_emu.cpp -Imethyldackel_amd/csrc
//   qdiff_emu < sites.txt > results.tsv
//       the input holds a line per site, of one of two kinds:
//         s FLOOR NA NB m u m u ...    a site: FLOOR is min_dispersion as the 16 hexadecimal digits of its 64-bit pattern, then the entries
//                                      (methylated, unmethylated) of group A's NA samples and of group B's NB samples, in visiting order
//         t F NU                       the tail alone: F as 16 hexadecimal digits, NU the degrees of freedom (at least 1)
//       The output holds a line per input line.  A site: `err nmeth_a nunmeth_a nmeth_b nunmeth_b meth_diff pvalue df dispersion
//       statistic steps` -- err the DIFF_E_* bits of the site (its entries checked, then its margins; 0: accepted), the four doubles as
//       the 16 hexadecimal digits of their 64-bit patterns, steps the terms that were added to the series.  A refused site has zeros in
//       the other columns.  A tail: `pvalue steps`.
// Exit 0; 2 for input that is neither.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mdk_qdiff_core.h"

static uint64_t pattern(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
static double number(uint64_t u) { double x; memcpy(&x, &u, 8); return x; }

int main(int argc, char **argv) {
    if(argc > 1) { fprintf(stderr, "usage: qdiff_emu < sites.txt > results.tsv\n"); return 2; }
    char kind[8];
    while(scanf("%7s", kind) == 1) {
        if(!strcmp(kind, "t")) {
            uint64_t f; int32_t nu; uint32_t steps = 0;
            if(scanf("%" SCNx64 " %" SCNd32, &f, &nu) != 2 || nu < 1) { fprintf(stderr, "not a tail\n"); return 2; }
            const double p = qdiff_tail(number(f), nu, &steps);
            printf("%016" PRIx64 "\t%u\n", pattern(p), steps);
            continue;
        }
        uint64_t fl; int32_t na, nb;
        if(strcmp(kind, "s") || scanf("%" SCNx64 " %" SCNd32 " %" SCNd32, &fl, &na, &nb) != 3 || na < 0 || nb < 0 || na + nb > DIFF_MAX_SAMPLES) { fprintf(stderr, "not a site\n"); return 2; }
        std::vector<int64_t> m(na + nb), u(na + nb);
        for(int32_t s = 0; s < na + nb; s++)
            if(scanf("%" SCNd64 " %" SCNd64, &m[s], &u[s]) != 2) { fprintf(stderr, "not a site: %d entries\n", (int)s); return 2; }
        // pass 1: the entries checked and pooled, the covered samples counted
        int64_t g[2][2] = {{0, 0}, {0, 0}}; int32_t k[2] = {0, 0}; uint32_t err = 0;
        for(int32_t s = 0; s < na + nb; s++) {
            const uint32_t e = diff_entry_check(m[s]) | diff_entry_check(u[s]);
            err |= e;
            if(!e) { g[s >= na][0] += m[s]; g[s >= na][1] += u[s]; k[s >= na] += m[s] + u[s] > 0; }
        }
        if(!err) err = diff_margin_check(g[0][0], g[0][1], g[1][0], g[1][1]);
        if(err) { printf("%u\t0\t0\t0\t0\t%016" PRIx64 "\t%016" PRIx64 "\t0\t%016" PRIx64 "\t%016" PRIx64 "\t0\n", err, (uint64_t)0, (uint64_t)0, (uint64_t)0, (uint64_t)0); continue; }
        // pass 2: Pearson's sum
        double pearson = 0.0;
        for(int32_t s = 0; s < na + nb; s++) {
            const int64_t *const gs = g[s >= na];
            if(gs[0] > 0 && gs[1] > 0 && m[s] + u[s] > 0) pearson = pearson + qdiff_term(m[s], u[s], gs[0], gs[1]);
        }
        qdiff_result r;
        qdiff_site(g[0][0], g[0][1], g[1][0], g[1][1], k[0], k[1], pearson, number(fl), &r);
        printf("0\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%016" PRIx64 "\t%016" PRIx64 "\t%d\t%016" PRIx64 "\t%016" PRIx64 "\t%u\n", g[0][0], g[0][1], g[1][0], g[1][1],
               pattern(diff_meth(g[0][0], g[0][1], g[1][0], g[1][1])), pattern(r.p), (int)r.df, pattern(r.dispersion), pattern(r.statistic), r.steps);
    }
    return 0;
}
