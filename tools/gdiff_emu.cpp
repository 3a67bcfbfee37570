// gdiff_emu.cpp -- TEST INFRASTRUCTURE: the quasi-binomial F test of several groups of replicates per site (csrc/mdk_gdiff_core.h) executed
// on the host, a site as k_gdiff takes it: pass 1 checks and pools every group and keeps its pooled pair, pass 2 takes the pairs again
// for the score and walks the groups' rows once more for Pearson's terms.
//   build: g++ -O2 -ffp-contract=off -o tools/_build/gdiff_emu tools/gdiff_emu.cpp -Imethyldackel_amd/csrc
//   gdiff_emu < sites.txt > results.tsv
//       the input holds a line per site, of one of two kinds:
//         s FLOOR G size_0 .. size_{G-1} m u m u ...   a site: FLOOR is min_dispersion as the 16 hexadecimal digits of its 64-bit pattern,
//                                      G the groups, then every group's samples, then the entries (methylated, unmethylated) of the
//                                      samples in visiting order: group 0's, then group 1's, ...
//         t W NU Q                     the tail alone: W as 16 hexadecimal digits, NU and Q the degrees of freedom (at least 1 each)
//       The output holds a line per input line.  A site: `err meth_diff group_lo group_hi pvalue df df_groups dispersion statistic steps`
//       and then every group's pooled `nmeth nunmeth` -- err the DIFF_E_* bits of the site (its entries checked, then its margins; 0:
//       accepted), the four doubles as the 16 hexadecimal digits of their 64-bit patterns, steps the terms that were added to the
//       series.  A refused site has what a site without anything to test has: counts 0, -1 -1, p 1.0, dispersion 1.0.  A tail: `pvalue
//       steps`.
// Exit 0; 2 for input that is neither.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mdk_gdiff_core.h"

static uint64_t pattern(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
static double number(uint64_t u) { double x; memcpy(&x, &u, 8); return x; }

int main(int argc, char **argv) {
    if(argc > 1) { fprintf(stderr, "usage: gdiff_emu < sites.txt > results.tsv\n"); return 2; }
    char kind[8];
    while(scanf("%7s", kind) == 1) {
        if(!strcmp(kind, "t")) {
            uint64_t w; int32_t nu, q; uint32_t steps = 0;
            if(scanf("%" SCNx64 " %" SCNd32 " %" SCNd32, &w, &nu, &q) != 3 || nu < 1 || q < 1) { fprintf(stderr, "not a tail\n"); return 2; }
            const double p = gdiff_tail(number(w), nu, q, &steps);
            printf("%016" PRIx64 "\t%u\n", pattern(p), steps);
            continue;
        }
        uint64_t fl; int32_t G;
        if(strcmp(kind, "s") || scanf("%" SCNx64 " %" SCNd32, &fl, &G) != 2 || G < 1 || G > DIFF_MAX_SAMPLES) { fprintf(stderr, "not a site\n"); return 2; }
        std::vector<int32_t> end(G);
        int32_t all = 0;
        for(int32_t g = 0; g < G; g++) {
            int32_t size;
            if(scanf("%" SCNd32, &size) != 1 || size < 0 || all + size > DIFF_MAX_SAMPLES) { fprintf(stderr, "not a site: group %d\n", (int)g); return 2; }
            all += size; end[g] = all;
        }
        std::vector<int64_t> m(all), u(all), gm(G), gu(G);
        for(int32_t s = 0; s < all; s++)
            if(scanf("%" SCNd64 " %" SCNd64, &m[s], &u[s]) != 2) { fprintf(stderr, "not a site: %d entries\n", (int)s); return 2; }
        // pass 1: the entries checked and pooled group by group, the covered groups and samples counted, the extremes kept
        int64_t K = 0, M = 0, lo_m = 0, lo_n = 0, hi_m = 0, hi_n = 0; int32_t g_eff = 0, k = 0, lo = -1, hi = -1; uint32_t err = 0, margin = 0;
        for(int32_t g = 0, s = 0; g < G; g++) {
            int64_t a = 0, b = 0; int32_t kg = 0;
            for(; s < end[g]; s++) {
                const uint32_t e = diff_entry_check(m[s]) | diff_entry_check(u[s]);
                err |= e;
                if(!e) { a += m[s]; b += u[s]; kg += m[s] + u[s] > 0; }
            }
            gm[g] = a; gu[g] = b;
            margin |= gdiff_margin_check(a + b, 0, 0);
            if(a + b == 0) continue;
            K += a; M += b; k += kg; g_eff++;
            if(lo < 0 || gdiff_below(a, a + b, lo_m, lo_n)) { lo = g; lo_m = a; lo_n = a + b; }
            if(hi < 0 || gdiff_below(hi_m, hi_n, a, a + b)) { hi = g; hi_m = a; hi_n = a + b; }
        }
        if(!err) err = margin | gdiff_margin_check(0, K, M);
        if(err) {
            printf("%u\t%016" PRIx64 "\t-1\t-1\t%016" PRIx64 "\t0\t0\t%016" PRIx64 "\t%016" PRIx64 "\t0", err, pattern(0.0), pattern(1.0), pattern(1.0), pattern(0.0));
            for(int32_t g = 0; g < G; g++) printf("\t0\t0");
            printf("\n");
            continue;
        }
        // pass 2: the score from the pooled pairs, Pearson's sum from the rows -- not for a site that has nothing to test
        double X = 0.0, pearson = 0.0;
        const int32_t nu = k - (g_eff > 2 ? g_eff : 2);
        if(g_eff >= 2 && nu >= 1 && K > 0 && M > 0) {
            int64_t first_m = 0, first_u = 0; int32_t seen = 0;
            for(int32_t g = 0, s = 0; g < G; g++) {
                const int64_t a = gm[g], b = gu[g];
                if(a + b > 0) {
                    if(g_eff != 2) X = X + gdiff_score_term(a, b, K, M);
                    else if(!seen) { first_m = a; first_u = b; }
                    else X = qdiff_score(first_m, first_u, a, b);
                    seen++;
                }
                if(a > 0 && b > 0) {
                    for(s = g ? end[g - 1] : 0; s < end[g]; s++)
                        if(m[s] + u[s] > 0) pearson = pearson + qdiff_term(m[s], u[s], a, b);
                }
            }
        }
        gdiff_result r;
        gdiff_site(g_eff, k, K, M, X, pearson, number(fl), &r);
        const double diff = lo < 0 ? 0.0 : diff_meth(lo_m, lo_n - lo_m, hi_m, hi_n - hi_m);
        printf("0\t%016" PRIx64 "\t%d\t%d\t%016" PRIx64 "\t%d\t%d\t%016" PRIx64 "\t%016" PRIx64 "\t%u", pattern(diff), (int)lo, (int)hi, pattern(r.p), (int)r.df, (int)r.df_groups,
               pattern(r.dispersion), pattern(r.statistic), r.steps);
        for(int32_t g = 0; g < G; g++) printf("\t%" PRId64 "\t%" PRId64, gm[g], gu[g]);
        printf("\n");
    }
    return 0;
}
