// merge_emu.cpp -- TEST INFRASTRUCTURE: the device's mergeContext over rows (csrc/mdk_merge_core.h, the very function k_merge_len and
// k_merge_fill of csrc/mdk_merge.hip run) executed on the host in the kernels' blocking.
//   build: g++ -O2 -o tools/_build/merge_emu tools/merge_emu.cpp -Imethyldackel_amd/csrc
//   merge_emu [--min-depth D] [--contigs N] < rows.tsv > merged.tsv
//       rows `contig start end nmeth nunmeth context strand`, all integers (contig an index, context 0 CpG / 1 CHG / 2 CHH, strand +1 / -1 / 0),
//       the merged rows in the same layout.  --min-depth: rows below it are dropped (default 1).  --contigs: the number of contig names
//       (default: the largest index of the input + 1).
// The passes are the kernels': workgroups of 256 rows, wavefronts of 64 lanes; a lane takes rows i - 1 and i + 1 from the lanes beside it,
// lanes 0 and 63 of a wavefront from the table (nothing before row 0 or past row n - 1); the count pass leaves a total per workgroup, the
// totals are scanned 1024 at a time with a carry, and the fill pass repeats the count pass, checks its total against the recorded one and its
// offset against the size of the result, and writes into columns of exactly that size (a write outside them is counted, never made).
// Exit 0 and the rows; exit 3 and, on stderr, `error: <name>` for every refused condition (merged, context, contig, order, lone_g, sum);
// exit 4 if the two passes disagree.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mdk_merge_core.h"

static const uint32_t WG = 256, WAVE = 64, SCAN_WG = 1024;

struct table { std::vector<mrg_row> row; int32_t n_contigs, min_depth; };

// one workgroup's pass: has[t] / out[t] for its lanes, the refusals in err; returns its total
static uint32_t workgroup(const table &T, uint32_t b, uint32_t *has, mrg_row *out, uint32_t &err) {
    const uint32_t n = (uint32_t)T.row.size();
    mrg_row lane[WG]; memset(lane, 0, sizeof(lane));
    for(uint32_t t = 0; t < WG; t++) { const uint32_t i = b * WG + t; if(i < n) { lane[t] = T.row[i]; lane[t].has = 1; } }
    uint32_t total = 0;
    for(uint32_t t = 0; t < WG; t++) {
        const uint32_t i = b * WG + t, l = t % WAVE;
        has[t] = 0;
        if(i >= n) continue;
        mrg_row prev, next;
        if(l == 0) { memset(&prev, 0, sizeof(prev)); if(i > 0) { prev = T.row[i - 1]; prev.has = 1; } } else prev = lane[t - 1];
        if(l == WAVE - 1) { memset(&next, 0, sizeof(next)); if(i + 1 < n) { next = T.row[i + 1]; next.has = 1; } } else next = lane[t + 1];
        has[t] = (uint32_t)mrg_row_out(prev, lane[t], next, T.n_contigs, T.min_depth, out[t], err);
        total += has[t];
    }
    return total;
}

int main(int argc, char **argv) {
    table T; T.n_contigs = -1; T.min_depth = 1;
    for(int i = 1; i < argc; i++) {
        if(!strcmp(argv[i], "--min-depth") && i + 1 < argc) T.min_depth = atoi(argv[++i]);
        else if(!strcmp(argv[i], "--contigs") && i + 1 < argc) T.n_contigs = atoi(argv[++i]);
        else { fprintf(stderr, "usage: merge_emu [--min-depth D] [--contigs N] < rows.tsv > merged.tsv\n"); return 2; }
    }
    char line[512]; int32_t top = -1;
    while(fgets(line, sizeof(line), stdin)) {
        long long v[7];
        if(sscanf(line, "%lld %lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) != 7) { fprintf(stderr, "merge_emu: bad row: %s", line); return 2; }
        mrg_row r = {(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3], (int32_t)v[4], (int32_t)(uint8_t)v[5], (int32_t)(int8_t)v[6], 1};
        if(r.contig > top) top = r.contig;
        T.row.push_back(r);
    }
    if(T.n_contigs < 0) T.n_contigs = top + 1;
    const uint32_t n = (uint32_t)T.row.size(), nb = (n + WG - 1) / WG;
    uint32_t has[WG], err = 0; static mrg_row out[WG];
    // k_merge_len
    std::vector<uint32_t> btot(nb); std::vector<int64_t> boff(nb);
    for(uint32_t b = 0; b < nb; b++) btot[b] = workgroup(T, b, has, out, err);
    if(err) {
        static const char *name[] = {"merged", "context", "contig", "order", "lone_g", "sum"};
        for(int k = 0; k < 6; k++) if(err >> k & 1) fprintf(stderr, "error: %s\n", name[k]);
        return 3;
    }
    // k_merge_blocks: SCAN_WG totals a round, the carry between the rounds
    int64_t carry = 0;
    for(uint32_t b0 = 0; b0 < nb; b0 += SCAN_WG) {
        int64_t ex = 0;
        for(uint32_t b = b0; b < nb && b < b0 + SCAN_WG; b++) { boff[b] = carry + ex; ex += btot[b]; }
        carry += ex;
    }
    const int64_t rows = carry;
    // k_merge_fill
    std::vector<mrg_row> dst((size_t)rows); uint64_t outside = 0, changed = 0;
    for(uint32_t b = 0; b < nb; b++) {
        uint32_t e2 = 0;
        const uint32_t total = workgroup(T, b, has, out, e2);
        if(e2 || total != btot[b] || boff[b] < 0 || boff[b] + (int64_t)total > rows) { changed++; continue; }
        uint32_t ex = 0;
        for(uint32_t t = 0; t < WG; t++) if(has[t]) { const int64_t o = boff[b] + ex++; if(o < 0 || o >= rows) outside++; else dst[(size_t)o] = out[t]; }
    }
    if(outside || changed) { fprintf(stderr, "merge_emu: the passes disagree (%" PRIu64 " workgroups, %" PRIu64 " rows outside the result)\n", changed, outside); return 4; }
    for(const mrg_row &r : dst) printf("%d\t%d\t%d\t%d\t%d\t%d\t%d\n", r.contig, r.start, r.end, r.m, r.u, r.ctx, r.strand);
    return ferror(stdout) ? 4 : 0;
}
