// unite_emu.cpp -- TEST INFRASTRUCTURE: the device's join of samples into one site table (csrc/mdk_unite_core.h, the very functions the
// kernels of csrc/mdk_unite.hip run) executed on the host in the kernels' blocking.
//   build: g++ -O2 -o tools/_build/unite_emu tools/unite_emu.cpp -Imethyldackel_amd/csrc
//   unite_emu [--contigs N] [--min-samples K] [--min-depth D] [--stats] < samples.tsv > united.tsv
//       the input holds rows `contig start end nmeth nunmeth context strand` (seven integers; contig an index, context 0 CpG / 1 CHG / 2 CHH,
//       strand +1 / -1 / 0), sample after sample, a line that begins with `#` between two samples: S - 1 such lines make S samples,
//       empty ones among them.  The output is one line per site of the result, ascending: `contig start end context strand nsamples`
//       and then `nmeth nunmeth` of every sample.  --min-samples (default: S); --min-depth (default 1); --contigs: the number of contig
//       names (default: the largest index of the rows + 1).  --stats: on stderr, `stats: words W word_rounds R union N site_rounds Q
//       atomics A` -- the bitmap's words, the rounds k_unite_blocks takes over their block table, the sites of the union, the rounds over
//       the sites' block table, and the atomicOr k_unite_mark issues.
// The passes are the kernels': workgroups of 256 rows of one sample whose lanes take row i - 1 from the lane beside them, lane 0 of a
// wavefront of 64 from the table (nothing before a sample's row 0); the extents as maxima of the contigs' last rows; their words scanned
// 1024 contigs a round; the bits of a wavefront's rows combined by the segmented OR over its lanes, one OR into the bitmap per run of
// equal words; the bits set per 16 words from four lanes of four words; a block table scanned in place 1024 entries a round with a carry;
// the ranks of four words a lane; the tally with the first row to arrive as the site's writer; the kept sites' places from a scan
// inside every 256 sites and the scan of their totals; the sites' columns from the writers' rows, then every row's counts and the
// comparison with what the writer wrote.  Every index into a table is checked, in mdk_unite_core.h or here: one outside its table is
// counted, never made.
// Exit 0 and the rows; exit 3 and, on stderr, `error: <name>` for every refused condition (order, contig, context, start, disagree,
// changed; extent: more than 2^35 bits, before anything is allocated; sites: more than 2^30); exit 4 if an index fell outside its table.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mdk_unite_core.h"

static const uint32_t WG = UNI_ROWS, WAVE = 64;

struct row { int32_t contig, start, end, m, u, ctx, strand; };
static uint64_t outside = 0;

// k_unite_blocks: UNI_SCAN entries a round in place, the carry between the rounds; returns the total, counts the rounds
static int64_t scan_blocks(std::vector<uint32_t> &tot, uint32_t nb, uint32_t &rounds) {
    int64_t carry = 0;
    rounds = 0;
    for(uint32_t b0 = 0; b0 < nb; b0 += UNI_SCAN) {
        int64_t ex = 0;
        for(uint32_t b = b0; b < nb && b < b0 + UNI_SCAN; b++) { const int64_t v = tot[b]; tot[b] = (uint32_t)(carry + ex); ex += v; }
        carry += ex; rounds++;
    }
    return carry;
}

static int refused(uint32_t err) {
    static const char *name[] = {"order", "contig", "context", "start", "disagree", "changed"};
    for(int b = 0; b < 6; b++) if(err >> b & 1) fprintf(stderr, "error: %s\n", name[b]);
    return 3;
}

int main(int argc, char **argv) {
    int32_t n_contigs = -1, min_samples = -1, min_depth = 1; bool stats = false;
    for(int i = 1; i < argc; i++) {
        if(!strcmp(argv[i], "--min-depth") && i + 1 < argc) min_depth = atoi(argv[++i]);
        else if(!strcmp(argv[i], "--min-samples") && i + 1 < argc) min_samples = atoi(argv[++i]);
        else if(!strcmp(argv[i], "--contigs") && i + 1 < argc) n_contigs = atoi(argv[++i]);
        else if(!strcmp(argv[i], "--stats")) stats = true;
        else { fprintf(stderr, "usage: unite_emu [--contigs N] [--min-samples K] [--min-depth D] [--stats] < samples.tsv > united.tsv\n"); return 2; }
    }
    std::vector<std::vector<row>> samples(1);
    char line[512]; int32_t top = -1;
    while(fgets(line, sizeof(line), stdin)) {
        if(line[0] == '#') { samples.emplace_back(); continue; }
        long long v[7];
        if(sscanf(line, "%lld %lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) != 7) { fprintf(stderr, "unite_emu: bad line: %s", line); return 2; }
        const row r = {(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3], (int32_t)v[4], (int32_t)(uint8_t)v[5], (int32_t)(int8_t)v[6]};
        samples.back().push_back(r);
        if(r.contig > top) top = r.contig;
    }
    const uint32_t S = (uint32_t)samples.size();
    if(n_contigs < 0) n_contigs = top + 1;
    if(min_samples < 0) min_samples = (int32_t)S;
    if(S > UNI_MAX_SAMPLES || min_samples < 1 || min_samples > (int32_t)S || min_depth < 0) { fprintf(stderr, "unite_emu: 1 to 1024 samples, min-samples 1 to S, min-depth not negative\n"); return 2; }
    uint32_t err = 0;
    // k_unite_rows
    std::vector<uint32_t> extent((size_t)(n_contigs > 0 ? n_contigs : 1), 0u);
    for(uint32_t s = 0; s < S; s++) {
        const std::vector<row> &R = samples[s];
        const uint32_t n = (uint32_t)R.size();
        for(uint32_t b = 0; b * WG < n; b++) {
            row lane[WG]; memset(lane, 0, sizeof(lane));
            for(uint32_t t = 0; t < WG; t++) if(b * WG + t < n) lane[t] = R[b * WG + t];
            for(uint32_t t = 0; t < WG; t++) {
                const uint32_t i = b * WG + t;
                if(i >= n) continue;
                int has_prev = 1; int32_t pc = 0, ps = 0;
                if(t % WAVE == 0) { has_prev = i > 0; if(has_prev) { pc = R[i - 1].contig; ps = R[i - 1].start; } }
                else { pc = lane[t - 1].contig; ps = lane[t - 1].start; }
                const uint32_t e = uni_row_check(has_prev, pc, ps, lane[t].contig, lane[t].start, lane[t].ctx, n_contigs);
                err |= e;
                if(has_prev && pc != lane[t].contig && pc >= 0 && pc < n_contigs && ps >= 0 && extent[pc] < (uint32_t)ps + 1u) extent[pc] = (uint32_t)ps + 1u;
                if(i == n - 1 && !(e & (UNI_E_CONTIG | UNI_E_START)) && extent[lane[t].contig] < (uint32_t)lane[t].start + 1u) extent[lane[t].contig] = (uint32_t)lane[t].start + 1u;
            }
        }
    }
    // k_unite_offsets: UNI_SCAN contigs a round
    std::vector<int64_t> base(extent.size(), 0);
    int64_t words = 0;
    for(int32_t c0 = 0; c0 < n_contigs; c0 += UNI_SCAN) {
        int64_t ex = 0;
        for(int32_t c = c0; c < n_contigs && c < c0 + UNI_SCAN; c++) { base[c] = words + ex; ex += uni_words(extent[c]); }
        words += ex;
    }
    if(err) return refused(err);
    if(words > UNI_MAX_WORDS) { fprintf(stderr, "error: extent\n"); return 3; }
    uni_tables T; T.extent = extent.data(); T.base = base.data(); T.bits = T.rankw = nullptr; T.n_contigs = n_contigs; T.n_union = 0;
    T.n_words = (words + UNI_BLOCK_WORDS - 1) / UNI_BLOCK_WORDS * UNI_BLOCK_WORDS;
    const uint32_t nb = (uint32_t)(T.n_words / UNI_BLOCK_WORDS), quads = (uint32_t)(T.n_words / 4);
    std::vector<uint32_t> bits((size_t)T.n_words, 0u), rankw((size_t)T.n_words, 0u), btot(nb, 0u);
    T.bits = bits.data(); T.rankw = rankw.data();
    // k_unite_mark: a wavefront at a time
    uint64_t atomics = 0;
    for(uint32_t s = 0; s < S; s++) {
        const std::vector<row> &R = samples[s];
        const uint32_t n = (uint32_t)R.size();
        for(uint32_t i0 = 0; i0 < n; i0 += WAVE) {
            uint32_t w[WAVE], bit[WAVE];
            for(uint32_t l = 0; l < WAVE; l++) {
                w[l] = UNI_NONE; bit[l] = 0;
                if(i0 + l >= n) continue;
                const row &r = R[i0 + l];
                const int64_t at = uni_word(T, r.contig, r.start);
                if(at < 0) { outside++; continue; }
                w[l] = (uint32_t)at;
                if(uni_present(r.m, r.u, min_depth)) bit[l] = uni_bit(r.start);
            }
            for(uint32_t d = 1; d < WAVE; d <<= 1) {
                uint32_t nxt[WAVE];
                for(uint32_t l = 0; l < WAVE; l++) nxt[l] = bit[l] | (l >= d && w[l - d] == w[l] ? bit[l - d] : 0u);
                memcpy(bit, nxt, sizeof(bit));
            }
            for(uint32_t l = 0; l < WAVE; l++) if(bit[l] && (l == WAVE - 1 || w[l + 1] != w[l])) { bits[w[l]] |= bit[l]; atomics++; }
        }
    }
    // k_unite_count: four words a lane, four lanes a block
    for(uint32_t t = 0; t < quads; t++) {
        uint32_t sum = 0;
        for(uint32_t q = 0; q < 4; q++) sum += uni_popc(bits[(size_t)t * 4 + q]);
        btot[t >> 2] += sum;
    }
    uint32_t word_rounds = 0, site_rounds = 0;
    const int64_t sites = scan_blocks(btot, nb, word_rounds);
    // k_unite_ranks
    for(uint32_t t = 0; t < quads; t++) {
        uint32_t r = btot[t >> 2];
        for(uint32_t q = t & ~3u; q < t; q++) for(uint32_t k = 0; k < 4; k++) r += uni_popc(bits[(size_t)q * 4 + k]);          // the lanes below in the block
        for(uint32_t k = 0; k < 4; k++) { rankw[(size_t)t * 4 + k] = r; r += uni_popc(bits[(size_t)t * 4 + k]); }
    }
    if(sites > UNI_MAX_SITES) { fprintf(stderr, "error: sites\n"); return 3; }
    T.n_union = (uint32_t)sites;
    // k_unite_tally
    std::vector<uint32_t> count(T.n_union, 0u), owner(T.n_union, UNI_NONE), map(T.n_union, UNI_NONE);
    for(uint32_t s = 0; s < S; s++)
        for(const row &r : samples[s]) {
            if(!uni_present(r.m, r.u, min_depth)) continue;
            const uint32_t site = uni_locate(T, r.contig, r.start);
            if(site == UNI_NONE) { err |= UNI_E_CHANGED; continue; }
            if(count[site]++ == 0) owner[site] = s;
        }
    // k_unite_keep, then k_unite_blocks over the sites' block table
    const uint32_t nkb = (T.n_union + WG - 1) / WG;
    std::vector<uint32_t> ktot(nkb, 0u);
    for(uint32_t b = 0; b < nkb; b++) {
        uint32_t ex = 0;
        for(uint32_t t = 0; t < WG; t++) {
            const uint32_t r = b * WG + t;
            if(r >= T.n_union) break;
            if(count[r] >= (uint32_t)min_samples) map[r] = ex++;
        }
        ktot[b] = ex;
    }
    const int64_t n_out = scan_blocks(ktot, nkb, site_rounds);
    // k_unite_sites, k_unite_fill
    std::vector<row> site((size_t)n_out); std::vector<int32_t> nsamples((size_t)n_out, 0), om((size_t)n_out * S, 0), ou((size_t)n_out * S, 0); std::vector<char> written((size_t)n_out, 0);
    for(int pass = 0; pass < 2; pass++)
        for(uint32_t s = 0; s < S; s++)
            for(const row &r : samples[s]) {
                if(!uni_present(r.m, r.u, min_depth)) continue;
                const uint32_t k = uni_locate(T, r.contig, r.start);
                if(k == UNI_NONE) { err |= UNI_E_CHANGED; continue; }
                if(pass == 0 && owner[k] != s) continue;
                const int64_t o = uni_place(ktot.data(), map.data(), k);
                if(o < 0) continue;
                if(o >= n_out) { outside++; continue; }
                if(pass == 0) { site[o] = r; nsamples[o] = (int32_t)count[k]; written[o]++; }
                else {
                    om[(size_t)s * n_out + o] = r.m; ou[(size_t)s * n_out + o] = r.u;
                    if(!uni_agree(r.end, r.ctx, r.strand, site[o].end, site[o].ctx, site[o].strand)) err |= UNI_E_DISAGREE;
                }
            }
    for(int64_t o = 0; o < n_out; o++) if(written[o] != 1) outside++;          // every kept site has exactly one writer
    if(outside) { fprintf(stderr, "unite_emu: %" PRIu64 " indices outside a table\n", outside); return 4; }
    if(err) return refused(err);
    if(stats) fprintf(stderr, "stats: words %" PRId64 " word_rounds %u union %u site_rounds %u atomics %" PRIu64 "\n", words, word_rounds, T.n_union, site_rounds, atomics);
    for(int64_t o = 0; o < n_out; o++) {
        printf("%d\t%d\t%d\t%d\t%d\t%d", site[o].contig, site[o].start, site[o].end, site[o].ctx, site[o].strand, nsamples[o]);
        for(uint32_t s = 0; s < S; s++) printf("\t%d\t%d", om[(size_t)s * n_out + o], ou[(size_t)s * n_out + o]);
        putchar('\n');
    }
    return ferror(stdout) ? 4 : 0;
}
