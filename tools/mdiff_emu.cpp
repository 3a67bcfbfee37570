// mdiff_emu.cpp -- TEST INFRASTRUCTURE: the quasi-binomial F test of a design's tested columns per site (csrc/mdk_mdiff_core.h) executed on
// the host, a site as k_mdiff takes it: a first walk checks and pools the entries and counts the covered samples, then mdiff_site of
// the design's width walks the samples again on every pass.
//   build: g++ -O2 -std=c++17 -ffp-contract=off -o tools/_build/mdiff_emu tools/mdiff_emu.cpp -Imethyldackel_amd/csrc
//   mdiff_emu < sites.txt > results.tsv
//       the input holds a line per request, of one of three kinds; every double is the 16 hexadecimal digits of its 64-bit pattern:
//         s FLOOR S P Q m u .. x ..    a site: FLOOR is min_dispersion, S the used samples, P the design's columns, Q the tested ones (the
//                                      last Q), then the S entries (methylated, unmethylated) in visiting order, then the S rows of P doubles
//         e T                          mdiff_exp alone: T in [-40, 0]
//         d S P x ..                   the host's test of a design: S rows of P doubles
//       The output holds a line per input line.  A site: `err pvalue df dispersion statistic flags iterations steps K M` and then the P
//       coefficients -- err the DIFF_E_* bits of the site (its entries checked, then its margins; 0: accepted).  A refused site has what
//       a site without anything to test has, and K = M = 0.  An exponential: its value.  A design: 1 where its columns are independent, 0
//       where they are not.
// Exit 0; 2 for input that is none of these.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mdk_mdiff_core.h"

static uint64_t pattern(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
static double number(uint64_t u) { double x; memcpy(&x, &u, 8); return x; }

struct HostSite {
    const int64_t *m, *u; const double *design; int32_t used, p;
    int32_t samples() const { return used; }
    void entry(int32_t s, int64_t *mm, int64_t *uu) const { *mm = m[s]; *uu = u[s]; }
    double x(int32_t s, int a) const { return design[(int64_t)s * p + a]; }
};

static void site(const HostSite &S, int32_t r, int32_t k, int64_t K, int64_t M, double floor, double *coef, mdiff_result *out) {
    switch(S.p) {
    case 2: mdiff_site<2>(S, r, k, K, M, floor, coef, out); break;
    case 3: mdiff_site<3>(S, r, k, K, M, floor, coef, out); break;
    case 4: mdiff_site<4>(S, r, k, K, M, floor, coef, out); break;
    case 5: mdiff_site<5>(S, r, k, K, M, floor, coef, out); break;
    case 6: mdiff_site<6>(S, r, k, K, M, floor, coef, out); break;
    case 7: mdiff_site<7>(S, r, k, K, M, floor, coef, out); break;
    default: mdiff_site<8>(S, r, k, K, M, floor, coef, out); break;
    }
}

static bool doubles(std::vector<double> &x) {
    for(double &v : x) {
        uint64_t w;
        if(scanf("%" SCNx64, &w) != 1) return false;
        v = number(w);
    }
    return true;
}

int main(int argc, char **argv) {
    if(argc > 1) { fprintf(stderr, "usage: mdiff_emu < sites.txt > results.tsv\n"); return 2; }
    char kind[8];
    while(scanf("%7s", kind) == 1) {
        if(!strcmp(kind, "e")) {
            uint64_t t;
            if(scanf("%" SCNx64, &t) != 1 || !(number(t) >= -40.0 && number(t) <= 0.0)) { fprintf(stderr, "not an exponent\n"); return 2; }
            printf("%016" PRIx64 "\n", pattern(mdiff_exp(number(t))));
            continue;
        }
        if(!strcmp(kind, "d")) {
            int32_t S, p;
            if(scanf("%" SCNd32 " %" SCNd32, &S, &p) != 2 || S < 1 || S > DIFF_MAX_SAMPLES || p < 2 || p > MDIFF_MAX_COLUMNS) { fprintf(stderr, "not a design\n"); return 2; }
            std::vector<double> x((size_t)S * p);
            if(!doubles(x)) { fprintf(stderr, "not a design: its entries\n"); return 2; }
            printf("%d\n", mdiff_independent(x.data(), S, p) ? 1 : 0);
            continue;
        }
        uint64_t fl; int32_t S, p, q;
        if(strcmp(kind, "s") || scanf("%" SCNx64 " %" SCNd32 " %" SCNd32 " %" SCNd32, &fl, &S, &p, &q) != 4 || S < 1 || S > DIFF_MAX_SAMPLES || p < 2 || p > MDIFF_MAX_COLUMNS ||
           q < 1 || q >= p) { fprintf(stderr, "not a site\n"); return 2; }
        std::vector<int64_t> m(S), u(S);
        std::vector<double> x((size_t)S * p);
        for(int32_t s = 0; s < S; s++)
            if(scanf("%" SCNd64 " %" SCNd64, &m[s], &u[s]) != 2) { fprintf(stderr, "not a site: %d entries\n", (int)s); return 2; }
        if(!doubles(x)) { fprintf(stderr, "not a site: its design\n"); return 2; }
        int64_t K = 0, M = 0; int32_t k = 0; uint32_t err = 0;
        for(int32_t s = 0; s < S; s++) {
            const uint32_t e = diff_entry_check(m[s]) | diff_entry_check(u[s]);
            err |= e;
            if(!e) { K += m[s]; M += u[s]; k += m[s] + u[s] > 0; }
        }
        if(!err) err = mdiff_margin_check(K, M);
        double coef[MDIFF_MAX_COLUMNS];
        mdiff_result r;
        if(err) {
            r.statistic = 0.0; r.dispersion = 1.0; r.p = 1.0; r.df = 0; r.iterations = 0; r.steps = 0; r.flags = 0; K = 0; M = 0;
            for(int a = 0; a < p; a++) coef[a] = 0.0;
        } else {
            const HostSite H = { m.data(), u.data(), x.data(), S, p };
            site(H, p - q, k, K, M, number(fl), coef, &r);
        }
        printf("%u\t%016" PRIx64 "\t%d\t%016" PRIx64 "\t%016" PRIx64 "\t%u\t%d\t%u\t%" PRId64 "\t%" PRId64, err, pattern(r.p), (int)r.df, pattern(r.dispersion), pattern(r.statistic),
               r.flags, (int)r.iterations, r.steps, K, M);
        for(int a = 0; a < p; a++) printf("\t%016" PRIx64, pattern(coef[a]));
        printf("\n");
    }
    return 0;
}
