// region_emu.cpp -- TEST INFRASTRUCTURE: the device's sums over intervals (csrc/mdk_region_core.h, the very functions k_region_rows and
// k_region_sum of csrc/mdk_regions.hip run) executed on the host in the kernels' blocking.
//   build: g++ -O2 -o tools/_build/region_emu tools/region_emu.cpp -Imethyldackel_amd/csrc
//   region_emu [--contigs N] [--contexts MASK] [--strands MASK] [--min-depth D] < table.tsv > sums.tsv
//       the input holds rows `contig start end nmeth nunmeth context strand` (seven integers; contig an index, context 0 CpG / 1 CHG / 2 CHH,
//       strand +1 / -1 / 0) and intervals `contig start end` (three integers), told apart by their number of fields, each kind in its own
//       order; the output is one line `nsites nmeth nunmeth` per interval, in the intervals' order.  --contexts: bit t for context t
//       (default 7); --strands: bit 0 for +1, bit 1 for -1, bit 2 for 0 (default 7); --min-depth (default 1); --contigs: the number of
//       contig names (default: the largest index of the rows and intervals + 1).
// The passes are the kernels': workgroups of 256 rows whose lanes take row i - 1 from the lane beside them, lane 0 of a wavefront of 64 from
// the table (nothing before row 0); a (nsites, nmeth, nunmeth) total per workgroup; the totals scanned in place 4096 at a time with a
// carry, the grand totals as entry nb; per interval the two searches, whole blocks as the difference of two prefix entries and the rows
// of the two partial blocks read with the filter applied again.  Every read of a row, an interval or a prefix entry goes through a bounds
// check: one outside its table is counted, never made.
// Exit 0 and the sums; exit 3 and, on stderr, `error: <name>` for every refused condition (order, contig, context, iv_contig, iv_range);
// exit 4 if a read fell outside its table.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mdk_region_core.h"

static const uint32_t WG = RGN_ROWS, WAVE = 64, SCAN_WG = 1024 * 4;          // SCAN_WG: the entries of a round, four per thread

struct row { int32_t contig, start, m, u, ctx, strand; };
static uint64_t outside = 0;

int main(int argc, char **argv) {
    rgn_filter F; F.context_mask = 7; F.strand_mask = 7; F.min_depth = 1;
    int32_t n_contigs = -1;
    for(int i = 1; i < argc; i++) {
        if(!strcmp(argv[i], "--min-depth") && i + 1 < argc) F.min_depth = atoi(argv[++i]);
        else if(!strcmp(argv[i], "--contigs") && i + 1 < argc) n_contigs = atoi(argv[++i]);
        else if(!strcmp(argv[i], "--contexts") && i + 1 < argc) F.context_mask = (uint32_t)atoi(argv[++i]);
        else if(!strcmp(argv[i], "--strands") && i + 1 < argc) F.strand_mask = (uint32_t)atoi(argv[++i]);
        else { fprintf(stderr, "usage: region_emu [--contigs N] [--contexts MASK] [--strands MASK] [--min-depth D] < table.tsv > sums.tsv\n"); return 2; }
    }
    std::vector<int32_t> contig, start, ivc, ivs, ive; std::vector<row> rows;
    char line[512]; int32_t top = -1;
    while(fgets(line, sizeof(line), stdin)) {
        long long v[7];
        const int f = sscanf(line, "%lld %lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]);
        if(f == 7) {
            const row r = {(int32_t)v[0], (int32_t)v[1], (int32_t)v[3], (int32_t)v[4], (int32_t)(uint8_t)v[5], (int32_t)(int8_t)v[6]};
            rows.push_back(r); contig.push_back(r.contig); start.push_back(r.start);
        } else if(f == 3) { ivc.push_back((int32_t)v[0]); ivs.push_back((int32_t)v[1]); ive.push_back((int32_t)v[2]); }
        else { fprintf(stderr, "region_emu: bad line: %s", line); return 2; }
        if((int32_t)v[0] > top) top = (int32_t)v[0];
    }
    if(n_contigs < 0) n_contigs = top + 1;
    const uint32_t n = (uint32_t)rows.size(), k = (uint32_t)ivc.size(), nb = (n + WG - 1) / WG;
    uint32_t err = 0;
    // k_region_rows
    std::vector<uint32_t> pre_sites((size_t)nb + 1, 0u); std::vector<int64_t> pre_m((size_t)nb + 1, 0), pre_u((size_t)nb + 1, 0);
    for(uint32_t b = 0; b < nb; b++) {
        row lane[WG]; memset(lane, 0, sizeof(lane));
        for(uint32_t t = 0; t < WG; t++) if(b * WG + t < n) lane[t] = rows[b * WG + t];
        for(uint32_t t = 0; t < WG; t++) {
            const uint32_t i = b * WG + t;
            if(i >= n) continue;
            int has_prev = 1; int32_t pc = 0, ps = 0;
            if(t % WAVE == 0) {
                has_prev = i > 0;
                if(has_prev) { if(i - 1 >= n) { outside++; continue; } pc = rows[i - 1].contig; ps = rows[i - 1].start; }
            } else { pc = lane[t - 1].contig; ps = lane[t - 1].start; }
            err |= rgn_row_check(has_prev, pc, ps, lane[t].contig, lane[t].start, lane[t].ctx, n_contigs);
            if(rgn_counts(F, lane[t].m, lane[t].u, lane[t].ctx, lane[t].strand)) { pre_sites[b]++; pre_m[b] += lane[t].m; pre_u[b] += lane[t].u; }
        }
    }
    // k_region_blocks: SCAN_WG totals a round in place, the carry between the rounds, the sum of all as entry nb
    {
        int64_t cs = 0, cm = 0, cu = 0;
        for(uint32_t b0 = 0; b0 < nb; b0 += SCAN_WG) {
            int64_t es = 0, em = 0, eu = 0;
            for(uint32_t b = b0; b < nb && b < b0 + SCAN_WG; b++) {
                const int64_t vs = pre_sites[b], vm = pre_m[b], vu = pre_u[b];
                pre_sites[b] = (uint32_t)(cs + es); pre_m[b] = cm + em; pre_u[b] = cu + eu;
                es += vs; em += vm; eu += vu;
            }
            cs += es; cm += em; cu += eu;
        }
        pre_sites[nb] = (uint32_t)cs; pre_m[nb] = cm; pre_u[nb] = cu;
    }
    // k_region_sum
    std::vector<int32_t> nsites(k, 0); std::vector<int64_t> nmeth(k, 0), nunmeth(k, 0);
    for(uint32_t j = 0; j < k; j++) {
        const uint32_t e = rgn_interval_check(ivc[j], ivs[j], ive[j], n_contigs);
        if(e) { err |= e; continue; }
        const uint32_t lo = rgn_lower_bound(contig.data(), start.data(), 0, n, ivc[j], ivs[j]);
        const uint32_t hi = rgn_lower_bound(contig.data(), start.data(), lo, n, ivc[j], ive[j]);
        if(lo > hi || hi > n) { outside++; continue; }
        const rgn_split sp = rgn_split_range(lo, hi);
        uint32_t sites = 0; int64_t sm = 0, su = 0;
        if(sp.b0 < sp.b1) {
            if(sp.b1 > nb) { outside++; continue; }
            sites = pre_sites[sp.b1] - pre_sites[sp.b0]; sm = pre_m[sp.b1] - pre_m[sp.b0]; su = pre_u[sp.b1] - pre_u[sp.b0];
        }
        const uint32_t la = sp.a_end - lo, len = la + (hi - sp.b_beg);
        if(sp.a_end < lo || sp.b_beg > hi || len > 2 * (WG - 1)) { outside++; continue; }
        for(uint32_t r = 0; r < len; r++) {
            const uint32_t i = r < la ? lo + r : sp.b_beg + (r - la);
            if(i >= n) { outside++; continue; }
            if(rgn_counts(F, rows[i].m, rows[i].u, rows[i].ctx, rows[i].strand)) { sites++; sm += rows[i].m; su += rows[i].u; }
        }
        nsites[j] = (int32_t)sites; nmeth[j] = sm; nunmeth[j] = su;
    }
    if(outside) { fprintf(stderr, "region_emu: %" PRIu64 " reads outside a table\n", outside); return 4; }
    if(err) {
        static const char *name[] = {"order", "contig", "context", "iv_contig", "iv_range"};
        for(int b = 0; b < 5; b++) if(err >> b & 1) fprintf(stderr, "error: %s\n", name[b]);
        return 3;
    }
    for(uint32_t j = 0; j < k; j++) printf("%d\t%" PRId64 "\t%" PRId64 "\n", nsites[j], nmeth[j], nunmeth[j]);
    return ferror(stdout) ? 4 : 0;
}
