// diff_emu.cpp -- TEST INFRASTRUCTURE: the device's test of two groups per site (csrc/mdk_diff_core.h, the very functions the kernel of
// csrc/mdk_diff.hip runs) executed on the host.
//   build: g++ -O2 -ffp-contract=off -o tools/_build/diff_emu tools/diff_emu.cpp -Imethyldackel_amd/csrc
//   diff_emu < tables.tsv > results.tsv
//       the input holds a table a line, `a b c d` (four integers: methylated and unmethylated of group A, of group B).  The output holds
//       a line per table: `err pvalue meth_diff steps` -- err the DIFF_E_* bits of the table (its four entries checked, then its margins;
//       0: accepted), the two doubles as the 16 hexadecimal digits of their 64-bit patterns, steps the terms that were added to the
//       sums.  A refused table has zeros in the other three columns.
// Exit 0; 2 for a line that is not four integers.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mdk_diff_core.h"

static uint64_t pattern(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }

int main(int argc, char **argv) {
    if(argc > 1) { fprintf(stderr, "usage: diff_emu < tables.tsv > results.tsv\n"); return 2; }
    char line[256];
    while(fgets(line, sizeof line, stdin)) {
        int64_t v[4];
        if(sscanf(line, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64, &v[0], &v[1], &v[2], &v[3]) != 4) { fprintf(stderr, "not a table: %s", line); return 2; }
        uint32_t err = 0, steps = 0;
        for(int q = 0; q < 4; q++) err |= diff_entry_check(v[q]);
        if(!err) err = diff_margin_check(v[0], v[1], v[2], v[3]);
        if(err) { printf("%u\t%016" PRIx64 "\t%016" PRIx64 "\t0\n", err, (uint64_t)0, (uint64_t)0); continue; }
        const double diff = diff_meth(v[0], v[1], v[2], v[3]), p = diff_pvalue(v[0], v[1], v[2], v[3], &steps);
        printf("0\t%016" PRIx64 "\t%016" PRIx64 "\t%u\n", pattern(p), pattern(diff), steps);
    }
    return 0;
}
