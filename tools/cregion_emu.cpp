// cregion_emu.cpp -- TEST INFRASTRUCTURE: every sample's sums over intervals (csrc/mdk_cregion_core.h over csrc/mdk_region_core.h, the very
// functions the kernels of csrc/mdk_cregion.hip run) executed on the host in the kernels' blocking.
//   build: g++ -O2 -o tools/_build/cregion_emu tools/cregion_emu.cpp -Imethyldackel_amd/csrc
//   cregion_emu --samples S [--contigs N] [--filter CONTEXTS:STRANDS:DEPTH]... [--sample-block B] [--max-workgroups G] < table.tsv > sums.tsv
//       the input holds sites `contig start context strand m0 u0 m1 u1 ...` (4 + 2 S integers; contig an index, context 0 CpG / 1 CHG /
//       2 CHH, strand +1 / -1 / 0) and intervals `contig start end` (three integers), told apart by their number of fields, each kind in
//       its own order.  Per --filter (masks as mdk_region_core.h's: bit t for context t; bit 0 for +1, bit 1 for -1, bit 2 for 0; without
//       one: 7:7:1), in their order, one line per interval in the intervals' order: `nsites nmeth nunmeth` of sample 0, of sample 1, ...
//       --contigs: the number of contig names (default: the largest index of the sites and intervals + 1).  --sample-block (1 to 64) and
//       --max-workgroups are md_cohort_limits': the samples of a batch and the most workgroups of a launch.  The library's defaults are 32
//       and 65536; this tool's are 4 and 8, so that tables of a few thousand sites go through a second batch and a second turn of every
//       grid-stride loop.
//   cregion_emu --cell S I N
//       prints crg_cell(S, I, N) and crg_entry(S, nb, nb) for nb = crg_blocks(N): the offsets the kernels form, as 64-bit values
// The passes are the kernels', launch by launch, each under the grid cap with the items dealt as crg_grid deals them: k_cregion_sites (blocks
// of 256 rows; a lane takes row i - 1 from the lane beside it, lane 0 of a wavefront from the table, nothing before row 0; the refusals and
// the byte per site), k_cregion_ranges (a lane per interval, the two searches), k_cregion_totals (a wavefront per block of sites and batch
// of samples, the sites' bytes kept across the batch), k_cregion_scan (a workgroup per sample, CRG_SCAN_ROUND entries a round with a
// carry), k_cregion_sum (a wavefront per 64 intervals and batch; whole blocks from two prefix entries, the partial blocks' rows read with
// the cell's cut).  Every read and write of a site, a cell, an interval, a range, a table entry or a result goes through a bounds check:
// one outside is counted, never made.
// Exit 0 and the sums; exit 3 and, on stderr, `error: <name>` for every refused condition (order, contig, context, iv_contig, iv_range);
// exit 4 if an access fell outside its array.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "mdk_cregion_core.h"

static const int WG = 256, WAVE = 64, WAVES = WG / WAVE;
static uint64_t outside = 0;

// an array whose every access is checked: one outside is counted and lands in a spare entry
template <typename T> struct checked {
    std::vector<T> v; T spare;
    void size(int64_t n) { v.assign((size_t)n, T()); spare = T(); }
    T &operator[](int64_t i) { if(i < 0 || i >= (int64_t)v.size()) { outside++; spare = T(); return spare; } return v[(size_t)i]; }
};

struct table {
    int32_t S = 0, n_contigs = 0; int64_t n = 0, k = 0, nb = 0;
    checked<int32_t> contig, start, ctx, strand, m, u, ivc, ivs, ive;
};

static void run(table &T, const rgn_filter &F, int32_t sblock_limit, int32_t grid_limit, uint32_t &err, checked<int32_t> &nsites, checked<int64_t> &nmeth, checked<int64_t> &nunmeth) {
    const int32_t sblock = T.S < sblock_limit ? T.S : sblock_limit, nbt = crg_batches(T.S, sblock);
    checked<uint8_t> pass; checked<uint32_t> lo, hi, pre_sites; checked<int64_t> pre_m, pre_u;
    pass.size(T.n); lo.size(T.k); hi.size(T.k);
    const int64_t entries = crg_entry(T.S, 0, T.nb);
    pre_sites.size(entries); pre_m.size(entries); pre_u.size(entries);
    nsites.size(crg_cell(T.S, 0, T.k)); nmeth.size(crg_cell(T.S, 0, T.k)); nunmeth.size(crg_cell(T.S, 0, T.k));
    if(T.nb) {
        // k_cregion_sites
        for(int64_t w = 0, grid = crg_grid(T.nb, grid_limit); w < grid; w++)
            for(int64_t b = w; b < T.nb; b += grid)
                for(int t = 0; t < WG; t++) {
                    const int64_t i = b * RGN_ROWS + t;
                    if(i >= T.n) continue;
                    int has_prev = 1;
                    if(t % WAVE == 0) has_prev = i > 0;                      // (otherwise the lane beside it, which holds row i - 1 of this block)
                    const int32_t pc = has_prev ? T.contig[i - 1] : 0, ps = has_prev ? T.start[i - 1] : 0;
                    err |= rgn_row_check(has_prev, pc, ps, T.contig[i], T.start[i], T.ctx[i], T.n_contigs);
                    pass[i] = crg_site_passes(F, T.ctx[i], T.strand[i]);
                }
        // k_cregion_totals
        const int64_t items = T.nb * nbt;
        for(int64_t w = 0, grid = crg_grid((items + WAVES - 1) / WAVES, grid_limit); w < grid; w++)
            for(int wave = 0; wave < WAVES; wave++)
                for(int64_t item = w * WAVES + wave; item < items; item += grid * WAVES) {
                    const int32_t t = (int32_t)(item / T.nb);
                    const int64_t b = item - (int64_t)t * T.nb;
                    int32_t s0, s1;
                    crg_batch(t, T.S, sblock, s0, s1);
                    uint8_t kept[RGN_ROWS];                                  // the sites' bytes, loaded once a batch
                    for(int r = 0; r < RGN_ROWS; r++) kept[r] = b * RGN_ROWS + r < T.n ? pass[b * RGN_ROWS + r] : (uint8_t)0;
                    for(int32_t s = s0; s < s1; s++) {
                        uint32_t sites = 0; int64_t sm = 0, su = 0;
                        for(int r = 0; r < RGN_ROWS; r++) {
                            const int64_t i = b * RGN_ROWS + r;
                            if(i >= T.n) continue;
                            const int32_t m = T.m[crg_cell(s, i, T.n)], u = T.u[crg_cell(s, i, T.n)];
                            if(crg_cell_counts(kept[r], m, u, F.min_depth)) { sites++; sm += m; su += u; }
                        }
                        const int64_t e = crg_entry(s, b, T.nb);
                        pre_sites[e] = sites; pre_m[e] = sm; pre_u[e] = su;
                    }
                }
        // k_cregion_scan
        for(int64_t w = 0, grid = crg_grid(T.S, grid_limit); w < grid; w++)
            for(int64_t s = w; s < T.S; s += grid) {
                const int64_t e = crg_entry((int32_t)s, 0, T.nb);
                int64_t cs = 0, cm = 0, cu = 0;
                for(int64_t b0 = 0; b0 < T.nb; b0 += CRG_SCAN_ROUND) {
                    int64_t es = 0, em = 0, eu = 0;
                    for(int64_t b = b0; b < T.nb && b < b0 + CRG_SCAN_ROUND; b++) {
                        const int64_t vs = pre_sites[e + b], vm = pre_m[e + b], vu = pre_u[e + b];
                        pre_sites[e + b] = (uint32_t)(cs + es); pre_m[e + b] = cm + em; pre_u[e + b] = cu + eu;
                        es += vs; em += vm; eu += vu;
                    }
                    cs += es; cm += em; cu += eu;
                }
                pre_sites[e + T.nb] = (uint32_t)cs; pre_m[e + T.nb] = cm; pre_u[e + T.nb] = cu;
            }
    }
    if(T.k) {
        // k_cregion_ranges (the searches read the site columns inside [0, n) by construction: rgn_lower_bound's)
        for(int64_t w = 0, grid = crg_grid((T.k + WG - 1) / WG, grid_limit); w < grid; w++)
            for(int t = 0; t < WG; t++)
                for(int64_t j = w * WG + t; j < T.k; j += grid * WG) {
                    const int32_t c = T.ivc[j], s = T.ivs[j], e = T.ive[j];
                    const uint32_t bad = rgn_interval_check(c, s, e, T.n_contigs);
                    uint32_t l = 0, h = 0;
                    if(bad) err |= bad;
                    else {
                        l = rgn_lower_bound(T.contig.v.data(), T.start.v.data(), 0, (uint32_t)T.n, c, s);
                        h = rgn_lower_bound(T.contig.v.data(), T.start.v.data(), l, (uint32_t)T.n, c, e);
                        if(l > h || h > T.n) { outside++; l = h = 0; }
                    }
                    lo[j] = l; hi[j] = h;
                }
        // k_cregion_sum
        const int64_t groups = (T.k + 63) / 64, items = groups * nbt;
        for(int64_t w = 0, grid = crg_grid((items + WAVES - 1) / WAVES, grid_limit); w < grid; w++)
            for(int wave = 0; wave < WAVES; wave++)
                for(int64_t item = w * WAVES + wave; item < items; item += grid * WAVES) {
                    const int32_t t = (int32_t)(item / groups);
                    const int64_t j0 = (item - (int64_t)t * groups) * 64;
                    int32_t s0, s1;
                    crg_batch(t, T.S, sblock, s0, s1);
                    crg_range R[WAVE];                                       // a lane each, kept across the sample loop
                    for(int l = 0; l < WAVE; l++) R[l] = j0 + l < T.k ? crg_range_of(lo[j0 + l], hi[j0 + l]) : crg_range_of(0, 0);
                    for(int32_t s = s0; s < s1; s++)
                        for(int l = 0; l < WAVE && j0 + l < T.k; l++) {
                            const crg_range &r = R[l];
                            uint32_t sites = 0; int64_t sm = 0, su = 0;
                            if(r.sp.b0 < r.sp.b1) {
                                const int64_t e0 = crg_entry(s, r.sp.b0, T.nb), e1 = crg_entry(s, r.sp.b1, T.nb);
                                if((int64_t)r.sp.b1 > T.nb) { outside++; continue; }
                                sites = pre_sites[e1] - pre_sites[e0]; sm = pre_m[e1] - pre_m[e0]; su = pre_u[e1] - pre_u[e0];
                            }
                            const uint32_t la = r.sp.a_end - r.lo, len = la + (r.hi - r.sp.b_beg);
                            if(r.sp.a_end < r.lo || r.sp.b_beg > r.hi || len > 2 * (RGN_ROWS - 1)) { outside++; continue; }
                            for(uint32_t q = 0; q < len; q++) {
                                const int64_t i = q < la ? r.lo + q : r.sp.b_beg + (q - la);
                                const int32_t m = T.m[crg_cell(s, i, T.n)], u = T.u[crg_cell(s, i, T.n)];
                                if(i >= T.n) { outside++; continue; }         // (a cell of another sample is inside the matrix, and still outside the row)
                                if(crg_cell_counts(pass[i], m, u, F.min_depth)) { sites++; sm += m; su += u; }
                            }
                            const int64_t o = crg_cell(s, j0 + l, T.k);
                            nsites[o] = (int32_t)sites; nmeth[o] = sm; nunmeth[o] = su;
                        }
                }
    }
}

int main(int argc, char **argv) {
    std::vector<rgn_filter> filters;
    table T; T.n_contigs = -1;
    int32_t sblock = 4, grid = 8;
    const char *usage = "usage: cregion_emu --samples S [--contigs N] [--filter CONTEXTS:STRANDS:DEPTH]... [--sample-block B] [--max-workgroups G] < table.tsv > sums.tsv\n";
    if(argc == 5 && !strcmp(argv[1], "--cell")) {                           // the offsets alone, as 64-bit values: no table
        const int32_t s = (int32_t)atoll(argv[2]); const int64_t i = atoll(argv[3]), n = atoll(argv[4]);
        printf("%" PRId64 "\t%" PRId64 "\n", crg_cell(s, i, n), crg_entry(s, crg_blocks(n), crg_blocks(n)));
        return 0;
    }
    for(int i = 1; i < argc; i++) {
        if(!strcmp(argv[i], "--samples") && i + 1 < argc) T.S = atoi(argv[++i]);
        else if(!strcmp(argv[i], "--contigs") && i + 1 < argc) T.n_contigs = atoi(argv[++i]);
        else if(!strcmp(argv[i], "--sample-block") && i + 1 < argc) sblock = atoi(argv[++i]);
        else if(!strcmp(argv[i], "--max-workgroups") && i + 1 < argc) grid = atoi(argv[++i]);
        else if(!strcmp(argv[i], "--filter") && i + 1 < argc) {
            unsigned cm, sm; int d;
            if(sscanf(argv[++i], "%u:%u:%d", &cm, &sm, &d) != 3 || cm > 7 || sm > 7 || d < 0) { fputs(usage, stderr); return 2; }
            rgn_filter f; f.context_mask = cm; f.strand_mask = sm; f.min_depth = d;
            filters.push_back(f);
        } else { fputs(usage, stderr); return 2; }
    }
    if(T.S < 1 || T.S > 1024 || sblock < 1 || sblock > CRG_BATCH_MAX || grid < 1) { fputs(usage, stderr); return 2; }
    if(filters.empty()) { rgn_filter f; f.context_mask = 7; f.strand_mask = 7; f.min_depth = 1; filters.push_back(f); }
    std::vector<int32_t> contig, start, ctx, strand, ivc, ivs, ive; std::vector<std::vector<int32_t>> m((size_t)T.S), u((size_t)T.S);
    std::string line; int32_t top = -1;
    for(int ch; (ch = getchar()) != EOF || !line.empty();) {
        if(ch != '\n' && ch != EOF) { line.push_back((char)ch); continue; }
        if(line.empty()) { if(ch == EOF) break; continue; }
        std::vector<long long> v;
        char *p = &line[0], *end;
        for(;;) { const long long x = strtoll(p, &end, 10); if(end == p) break; v.push_back(x); p = end; }
        while(*p == ' ' || *p == '\t' || *p == '\r') p++;
        if(*p || (v.size() != 3 && v.size() != (size_t)(4 + 2 * T.S))) { fprintf(stderr, "cregion_emu: bad line: %s\n", line.c_str()); return 2; }
        if(v.size() == 3) { ivc.push_back((int32_t)v[0]); ivs.push_back((int32_t)v[1]); ive.push_back((int32_t)v[2]); }
        else {
            contig.push_back((int32_t)v[0]); start.push_back((int32_t)v[1]); ctx.push_back((int32_t)(uint8_t)v[2]); strand.push_back((int32_t)(int8_t)v[3]);
            for(int32_t s = 0; s < T.S; s++) { m[s].push_back((int32_t)v[4 + 2 * s]); u[s].push_back((int32_t)v[5 + 2 * s]); }
        }
        if((int32_t)v[0] > top) top = (int32_t)v[0];
        line.clear();
        if(ch == EOF) break;
    }
    if(T.n_contigs < 0) T.n_contigs = top + 1;
    T.n = (int64_t)contig.size(); T.k = (int64_t)ivc.size(); T.nb = crg_blocks(T.n);
    T.contig.v = contig; T.start.v = start; T.ctx.v = ctx; T.strand.v = strand; T.ivc.v = ivc; T.ivs.v = ivs; T.ive.v = ive;
    T.m.size(crg_cell(T.S, 0, T.n)); T.u.size(crg_cell(T.S, 0, T.n));
    for(int32_t s = 0; s < T.S; s++) for(int64_t i = 0; i < T.n; i++) { T.m[crg_cell(s, i, T.n)] = m[s][i]; T.u[crg_cell(s, i, T.n)] = u[s][i]; }
    uint32_t err = 0;
    std::string outtext;
    for(const rgn_filter &F : filters) {
        checked<int32_t> nsites; checked<int64_t> nmeth, nunmeth;
        run(T, F, sblock, grid, err, nsites, nmeth, nunmeth);
        char buf[96];
        for(int64_t j = 0; j < T.k; j++)
            for(int32_t s = 0; s < T.S; s++) {
                const int64_t o = crg_cell(s, j, T.k);
                snprintf(buf, sizeof buf, "%d\t%" PRId64 "\t%" PRId64 "%c", nsites[o], nmeth[o], nunmeth[o], s + 1 < T.S ? '\t' : '\n');
                outtext += buf;
            }
    }
    if(outside) { fprintf(stderr, "cregion_emu: %" PRIu64 " accesses outside an array\n", outside); return 4; }
    if(err) {
        static const char *name[] = {"order", "contig", "context", "iv_contig", "iv_range"};
        for(int b = 0; b < 5; b++) if(err >> b & 1) fprintf(stderr, "error: %s\n", name[b]);
        return 3;
    }
    fputs(outtext.c_str(), stdout);
    return ferror(stdout) ? 4 : 0;
}
