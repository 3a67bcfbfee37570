// parse_emu.cpp -- TEST INFRASTRUCTURE: the device's text parser (csrc/mdk_parse_core.h, the very functions k_parse_len and k_parse_fill of
// csrc/mdk_parse.hip run) executed on the host in the kernels' blocking.
//   build: g++ -O2 -o tools/_build/parse_emu tools/parse_emu.cpp -Imethyldackel_amd/csrc
//   parse_emu bedgraph|report CONTIGS < text > rows.tsv
//       CONTIGS: a file with a line per contig, `name` or `name <tab> bases` (bases: the contig is resident, as after md_text_reference;
//       `name <tab>` alone is a resident contig of no bases).  Rows `contig start end nmeth nunmeth context strand` (bedgraph) or
//       `contig pos strand nmeth nunmeth context tri` (report), contig an index, context 0 / 1 / 2, strand +1 / -1.
// The passes are the kernels': a workgroup of 256 lanes owns a span of 4096 bytes, 16 per lane, taken as four little-endian words; a lane's
// newlines come from prs_newlines, "the byte before my first is a newline" from the lane below, for lanes 0, 64, 128, 192 from the text;
// `track` lines are cleared from an image of the span plus its look-ahead (16 bytes in the counting pass, 512 in the fill), which holds
// the text only as far as it goes and 0xAA behind it; the totals are scanned 1024 at a time with a carry; the fill repeats the marks,
// checks its total against the recorded one, lists the span's line starts and parses them in rounds of 256 from the image, writing into
// columns of exactly the measured size (a write outside them is counted, never made).
// Exit 0 and the rows; exit 3 and, on stderr, `error: <name>` for every refusal met, `first: <name>` and `offset: <byte>` for the refused line
// that starts earliest; exit 4 if the two passes disagree.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "mdk_parse_core.h"

static const uint32_t WG = 256, WAVE = 64, SCAN_WG = 1024, AHEAD_LEN = PARSE_LANE, AHEAD_FILL = PARSE_MAX_LINE;

struct input { std::vector<uint8_t> text; int64_t bytes; };

// a lane's quad as the device loads it: whole if it lies inside the text, else the bytes that do, zero behind them
static void quad(const input &I, int64_t at, uint8_t *dst) {
    memset(dst, 0, PARSE_LANE);
    for(int i = 0; i < PARSE_LANE; i++) if(at + i < I.bytes) dst[i] = I.text[(size_t)(at + i)];
}

// one workgroup's marks: starts[t] for its lanes, img filled; returns its total
static uint32_t workgroup(const input &I, uint32_t b, uint32_t ahead, uint8_t *img, uint32_t *starts) {
    const int64_t base = (int64_t)b * PARSE_SPAN;
    memset(img, 0xAA, PARSE_SPAN + AHEAD_FILL);
    uint32_t nl[WG];
    for(uint32_t t = 0; t < WG; t++) {
        quad(I, base + PARSE_LANE * t, img + PARSE_LANE * t);
        uint32_t w[4]; memcpy(w, img + PARSE_LANE * t, 16);
        nl[t] = prs_newlines(w[0], w[1], w[2], w[3]);
    }
    for(uint32_t k = 0; k < ahead / PARSE_LANE; k++) { const int64_t a = base + PARSE_SPAN + PARSE_LANE * k; if(a < I.bytes) quad(I, a, img + PARSE_SPAN + PARSE_LANE * k); }
    uint32_t total = 0;
    for(uint32_t t = 0; t < WG; t++) {
        const int64_t at = base + PARSE_LANE * t;
        bool prev_nl = t % WAVE ? (nl[t - 1] >> 15 & 1u) != 0 : (at == 0 || (at <= I.bytes && I.text[(size_t)(at - 1)] == '\n'));
        uint32_t s = prs_starts(nl[t], prev_nl, at, I.bytes);
        for(uint32_t m = s; m; m &= m - 1) { const uint32_t k = (uint32_t)__builtin_ctz(m); if(prs_is_track(img + PARSE_LANE * t + k, I.bytes - (at + k))) s &= ~(1u << k); }
        starts[t] = s; total += (uint32_t)__builtin_popcount(s);
    }
    return total;
}

int main(int argc, char **argv) {
    if(argc != 3 || (strcmp(argv[1], "bedgraph") && strcmp(argv[1], "report"))) { fprintf(stderr, "usage: parse_emu bedgraph|report CONTIGS < text > rows.tsv\n"); return 2; }
    const int fmt = !strcmp(argv[1], "report") ? MD_PARSE_CYTOSINE_REPORT : MD_PARSE_BEDGRAPH;
    // the name table, its index and the resident bases
    std::vector<std::string> name, bases; std::vector<int64_t> ref_len;
    {
        FILE *f = fopen(argv[2], "rb");
        if(!f) { fprintf(stderr, "parse_emu: cannot open %s\n", argv[2]); return 2; }
        std::string all; char buf[65536]; size_t r;
        while((r = fread(buf, 1, sizeof(buf), f)) > 0) all.append(buf, r);
        fclose(f);
        for(size_t i = 0; i < all.size(); ) {
            size_t e = all.find('\n', i); if(e == std::string::npos) e = all.size();
            const std::string l = all.substr(i, e - i); const size_t tab = l.find('\t');
            name.push_back(l.substr(0, tab));
            bases.push_back(tab == std::string::npos ? std::string() : l.substr(tab + 1));
            ref_len.push_back(tab == std::string::npos ? -1 : (int64_t)bases.back().size());
            i = e + 1;
        }
    }
    const int32_t n = (int32_t)name.size();
    std::vector<uint32_t> name_off(n + 1, 0u), sorted(n); std::string names; std::vector<const uint8_t *> ref(n);
    for(int32_t i = 0; i < n; i++) { names += name[i]; name_off[i + 1] = (uint32_t)names.size(); sorted[i] = (uint32_t)i; ref[i] = (const uint8_t *)bases[i].data(); }
    const uint8_t *const nb_ = (const uint8_t *)names.data();
    std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t x, uint32_t y) { return prs_name_cmp(nb_ + name_off[x], name_off[x + 1] - name_off[x], nb_ + name_off[y], name_off[y + 1] - name_off[y]) < 0; });
    bool any_ref = false; for(int64_t l : ref_len) any_ref |= l >= 0;
    const prs_tab T = {name_off.data(), nb_, sorted.data(), n, any_ref ? ref.data() : nullptr, ref_len.data()};

    input I;
    { uint8_t buf[65536]; size_t r; while((r = fread(buf, 1, sizeof(buf), stdin)) > 0) I.text.insert(I.text.end(), buf, buf + r); }
    I.bytes = (int64_t)I.text.size();
    if(I.bytes > INT32_MAX) { fprintf(stderr, "parse_emu: more than 2^31 - 1 bytes\n"); return 2; }
    const uint32_t nb = (uint32_t)((I.bytes + PARSE_SPAN - 1) / PARSE_SPAN);
    static uint8_t img[PARSE_SPAN + AHEAD_FILL]; static uint32_t starts[WG]; static uint16_t list[PARSE_SPAN];
    // k_parse_len
    std::vector<uint32_t> btot(nb); std::vector<int64_t> boff(nb);
    for(uint32_t b = 0; b < nb; b++) btot[b] = workgroup(I, b, AHEAD_LEN, img, starts);
    // k_parse_blocks: SCAN_WG totals a round, the carry between the rounds
    int64_t carry = 0;
    for(uint32_t b0 = 0; b0 < nb; b0 += SCAN_WG) {
        int64_t ex = 0;
        for(uint32_t b = b0; b < nb && b < b0 + SCAN_WG; b++) { boff[b] = carry + ex; ex += btot[b]; }
        carry += ex;
    }
    const int64_t rows = carry;
    // k_parse_fill
    std::vector<prs_row> dst((size_t)rows); uint64_t outside = 0, changed = 0, first = ~0ull; uint32_t err = 0;
    for(uint32_t b = 0; b < nb; b++) {
        const uint32_t total = workgroup(I, b, AHEAD_FILL, img, starts);
        if(total != btot[b] || boff[b] < 0 || boff[b] + (int64_t)total > rows) { changed++; continue; }
        uint32_t j = 0;
        for(uint32_t t = 0; t < WG; t++) for(uint32_t m = starts[t]; m; m &= m - 1) list[j++] = (uint16_t)(PARSE_LANE * t + (uint32_t)__builtin_ctz(m));
        const int64_t base = (int64_t)b * PARSE_SPAN;
        for(uint32_t r0 = 0; r0 < total; r0 += WG) for(uint32_t t = 0; t < WG && r0 + t < total; t++) {
            const uint32_t r = r0 + t, s = list[r];
            const int64_t at = base + s;
            prs_row row; memset(&row, 0, sizeof(row));
            const uint32_t e = prs_line(img + s, I.bytes - at, fmt, T, row);
            if(e) { err |= e; const uint64_t v = (uint64_t)at << 8 | (uint64_t)__builtin_ctz(e); if(v < first) first = v; continue; }
            const int64_t o = boff[b] + r;
            if(o < 0 || o >= rows) outside++; else dst[(size_t)o] = row;
        }
    }
    if(outside || changed) { fprintf(stderr, "parse_emu: the passes disagree (%" PRIu64 " workgroups, %" PRIu64 " rows outside the result)\n", changed, outside); return 4; }
    if(err) {
        for(int k = 0; k < PRS_N_ERRORS; k++) if(err >> k & 1) fprintf(stderr, "error: %s\n", prs_error_name(1u << k));
        fprintf(stderr, "first: %s\noffset: %" PRIu64 "\nmessage: %s\n", prs_error_name(1u << (first & 0xffu)), first >> 8, prs_error_text(1u << (first & 0xffu)));
        return 3;
    }
    for(const prs_row &r : dst) {
        if(fmt == MD_PARSE_CYTOSINE_REPORT) printf("%d\t%d\t%d\t%d\t%d\t%d\t%c%c%c\n", r.contig, r.a, r.strand, r.m, r.u, r.ctx, r.tri[0], r.tri[1], r.tri[2]);
        else printf("%d\t%d\t%d\t%d\t%d\t%d\t%d\n", r.contig, r.a, r.b, r.m, r.u, r.ctx, r.strand);
    }
    return ferror(stdout) ? 4 : 0;
}
