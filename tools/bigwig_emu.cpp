// bigwig_emu -- TEST INFRASTRUCTURE: the host build of csrc/mdk_bigwig_core.h, in the decomposition its kernels have (csrc/mdk_bigwig.hip): the rule walked row by
// row, bin by bin and section by section, every section through the phases of csrc/mdk_deflate_core.h lane by lane (tools/deflate_walk.h).
// With the deflate core it makes a whole bigWig on the CPU; zlib must inflate every section (tests/test_bigwig_cpu.py).
//   bigwig_emu [--coverage] [--pieces N] contigs.tsv rows.tsv out.bw
//       contigs.tsv: name <tab> length, the list's order; rows.tsv: contig index, start, end, nmeth, nunmeth per line.  A refused table:
//       "row R: why" on stderr, exit status 3.  --pieces N: the file is assembled N bytes at a time through bw_cut_range, the header's map of
//       a byte range onto the layout's pieces and the packed sections (what md_track_bigwig_fill_range runs), in place of the plain copies
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "mdk_bigwig_core.h"
#include "deflate_walk.h"

static dfl_walk_stats g_st;

// one section: in[0, n) as a zlib stream into slot (BW_SLOT bytes); its length (0: it does not fit, never)
static uint32_t compress_section(const uint8_t *in, uint32_t n, uint8_t *slot, uint32_t *tok, dfl_state &S) {
    const uint32_t stream_bytes = dfl_walk_stream(S, in, n, slot, BW_SLOT, tok, g_st);
    uint64_t a = 0, b = 0;
    for(uint32_t lane = 0; lane < 64; lane++) { uint64_t la, lb; bw_adler_lane(in, n, lane, la, lb); a += la; b += lb; }
    const uint32_t adler = bw_adler_finish(a, b, n), len = 2 + stream_bytes + 4;
    if(BW_SLOT_LEAD + len > BW_SLOT || stream_bytes > 5 + n) return 0;
    ((uint32_t *)slot)[4] = bw_zlib_dword(S.first_dw);
    for(uint32_t i = 0; i < 4; i++) slot[18 + stream_bytes + i] = bw_adler_byte(i, adler);
    return len;
}

int main(int argc, char **argv) {
    int mode = BW_VALUE_PERCENT, a0 = 1; long long piece_bytes = 0;
    for(;;) {
        if(argc > a0 && !strcmp(argv[a0], "--coverage")) { mode = BW_VALUE_COVERAGE; a0++; }
        else if(argc > a0 + 1 && !strcmp(argv[a0], "--pieces")) { piece_bytes = atoll(argv[a0 + 1]); a0 += 2; if(piece_bytes < 1) { fprintf(stderr, "bigwig_emu: --pieces takes a number of bytes, 1 or more\n"); return 2; } }
        else break;
    }
    if(argc - a0 != 3) { fprintf(stderr, "usage: bigwig_emu [--coverage] [--pieces N] contigs.tsv rows.tsv out.bw\n"); return 2; }
    std::vector<std::string> names; std::vector<uint32_t> len;
    {
        FILE *f = fopen(argv[a0], "r");
        if(!f) { perror(argv[a0]); return 2; }
        char name[1024]; unsigned long long l;
        while(fscanf(f, "%1023[^\t]\t%llu\n", name, &l) == 2) { names.push_back(name); len.push_back((uint32_t)l); }
        fclose(f);
    }
    std::vector<int32_t> contig, start, end, m, u;
    {
        FILE *f = fopen(argv[a0 + 1], "r");
        if(!f) { perror(argv[a0 + 1]); return 2; }
        long long c, s, e, mm, uu;
        while(fscanf(f, "%lld %lld %lld %lld %lld", &c, &s, &e, &mm, &uu) == 5) { contig.push_back((int32_t)c); start.push_back((int32_t)s); end.push_back((int32_t)e); m.push_back((int32_t)mm); u.push_back((int32_t)uu); }
        fclose(f);
    }
    const uint32_t n = (uint32_t)contig.size(), nc = (uint32_t)names.size();
    // ---- the refusals, and every contig's run of rows ----
    unsigned long long first_bad = ~0ull;
    std::vector<uint32_t> first(nc, 0), last(nc, 0);
    for(uint32_t i = 0; i < n; i++) {
        const uint32_t code = bw_row_check(mode, (int32_t)nc, len.data(), contig[i], start[i], end[i], m[i], u[i]);
        if(code && ((unsigned long long)i << 8 | code) < first_bad) first_bad = (unsigned long long)i << 8 | code;
        if(i) {
            const uint32_t pair = bw_pair_check(contig[i - 1], start[i - 1], end[i - 1], contig[i], start[i]);
            const unsigned long long key = (unsigned long long)(pair == BW_E_OVERLAP ? i - 1 : i) << 8 | pair;
            if(pair && key < first_bad) first_bad = key;
        }
        if(contig[i] < 0 || contig[i] >= (int32_t)nc) continue;
        if(!i || contig[i - 1] != contig[i]) first[contig[i]] = i;
        if(i == n - 1 || contig[i + 1] != contig[i]) last[contig[i]] = i + 1;
    }
    if(first_bad != ~0ull) { fprintf(stderr, "row %llu: %s\n", first_bad >> 8, bw_error_text((uint32_t)(first_bad & 0xff))); return 3; }
    // ---- sections: raw, compressed ----
    std::vector<std::vector<uint8_t>> sec;                          // the compressed sections: data, then the written levels'
    std::vector<bw_entry> entry; std::vector<uint32_t> size; uint32_t raw_max = 0;
    std::vector<uint32_t> raw(BW_RAW_STRIDE / 4), slot32(BW_SLOT / 4), tok(BW_RAW_STRIDE);
    dfl_state *S = new dfl_state();
    auto compress = [&](uint32_t raw_len, const bw_entry &e) -> bool {
        // the section's input in a buffer of exactly raw_len bytes: a read before byte 0 or past the last one is a read outside an allocation
        std::vector<uint8_t> piece((const uint8_t *)raw.data(), (const uint8_t *)raw.data() + raw_len);
        const uint32_t l = compress_section(piece.data(), raw_len, (uint8_t *)slot32.data(), tok.data(), *S);
        if(!l) { fprintf(stderr, "bigwig_emu: section %zu does not fit its slot\n", sec.size()); return false; }
        const uint8_t *p = (const uint8_t *)slot32.data() + BW_SLOT_LEAD;
        sec.emplace_back(p, p + l); entry.push_back(e); size.push_back(l); if(raw_len > raw_max) raw_max = raw_len;
        return true;
    };
    for(uint32_t c = 0; c < nc; c++) for(uint32_t r0 = first[c]; r0 < last[c]; r0 += BW_ITEMS) {
        const uint32_t cnt = last[c] - r0 < BW_ITEMS ? last[c] - r0 : BW_ITEMS;
        bw_section_header(raw.data(), c, (uint32_t)start[r0], (uint32_t)end[r0 + cnt - 1], cnt);
        for(uint32_t k = 0; k < cnt; k++) bw_item(raw.data() + 6 + 3 * k, (uint32_t)start[r0 + k], (uint32_t)end[r0 + k], bw_value(mode, m[r0 + k], u[r0 + k]));
        if(!compress(24 + 12 * cnt, bw_entry{c, (uint32_t)start[r0], c, (uint32_t)end[r0 + cnt - 1]})) return 1;
    }
    const uint64_t n_data = sec.size();
    // ---- zoom: every level's bins, a contig after the other ----
    std::vector<std::vector<uint32_t>> base(BW_LEVELS, std::vector<uint32_t>(nc + 1, 0));
    std::vector<std::vector<bw_bin>> bins(BW_LEVELS);
    for(int k = 0; k < BW_LEVELS; k++) {
        for(uint32_t c = 0; c < nc; c++) base[k][c + 1] = base[k][c] + bw_level_bins(len[c], k);
        bins[k].resize(base[k][nc]);
        for(uint32_t x = 0; x < base[k][nc]; x++) {
            const uint32_t c = bw_find_contig(base[k].data(), nc, x), bin = x - base[k][c];
            bw_bin &b = bins[k][x];
            if(k == 0) { bw_zoom0(b, mode, start.data(), end.data(), m.data(), u.data(), first[c], last[c], bin, len[c]); continue; }
            bw_bin_clear(b);
            const uint32_t kids = base[k - 1][c + 1] - base[k - 1][c];
            for(uint32_t j = 0; j < 4; j++) { const uint64_t cb = 4ull * bin + j; if(cb >= kids) break; bw_bin_child(b, bins[k - 1][base[k - 1][c] + (uint32_t)cb]); }
        }
    }
    int64_t zcount[BW_LEVELS]; bool written[BW_LEVELS]; uint64_t zsec[BW_LEVELS];
    for(int k = 0; k < BW_LEVELS; k++) { zcount[k] = 0; for(const bw_bin &b : bins[k]) zcount[k] += b.valid != 0; }
    bw_plan_levels(n, zcount, written);
    for(int k = 0; k < BW_LEVELS; k++) {
        zsec[k] = 0;
        if(!written[k]) continue;
        uint32_t at = 0; bw_entry e = {0, 0, 0, 0};
        for(uint32_t x = 0; x < base[k][nc]; x++) {
            if(!bins[k][x].valid) continue;
            const uint32_t c = bw_find_contig(base[k].data(), nc, x);
            uint32_t *rec = raw.data() + 8 * at;
            bw_zoom_record(rec, c, x - base[k][c], k, len[c], bins[k][x]);
            if(at == 0) { e.c0 = rec[0]; e.s0 = rec[1]; }
            e.c1 = rec[0]; e.e1 = rec[2];
            if(++at == BW_ZITEMS) { if(!compress(32 * at, e)) return 1; zsec[k]++; at = 0; }
        }
        if(at) { if(!compress(32 * at, e)) return 1; zsec[k]++; }
    }
    bw_summary total = {0, 0.0, 0.0, 0.0, 0.0};
    for(const bw_bin &b : bins[BW_LEVELS - 1]) bw_total_add(total, b);
    // ---- the file ----
    const bw_layout lay = bw_make_layout(names, len, n_data, written, zcount, zsec, entry.data(), size.data(), raw_max, total);
    std::vector<uint8_t> file((size_t)lay.total, 0);
    if(!piece_bytes) {
        for(const bw_piece &p : lay.pieces) memcpy(file.data() + p.at, p.bytes.data(), p.bytes.size());
        for(size_t s = 0; s < sec.size(); s++) memcpy(file.data() + lay.sec_off[s], sec[s].data(), sec[s].size());
    } else {
        std::vector<uint8_t> store;                                // the sections one behind the other, as the device keeps them
        for(const std::vector<uint8_t> &s : sec) store.insert(store.end(), s.begin(), s.end());
        const std::vector<bw_region> regions = bw_make_regions(lay, n_data, written, zsec, size.data());
        for(int64_t at = 0; at < lay.total; at += piece_bytes) {
            const int64_t want = std::min<int64_t>(piece_bytes, lay.total - at);
            std::vector<uint8_t> piece((size_t)want, 0);          // a buffer of exactly the range: a cut past it is a write outside an allocation
            int64_t got = 0;
            for(const bw_cut &c : bw_cut_range(lay, regions, at, want)) {
                memcpy(piece.data() + c.dst, c.piece ? lay.pieces[c.index].bytes.data() + c.src : store.data() + c.src, (size_t)c.bytes);
                got += c.bytes;
            }
            if(got != want) { fprintf(stderr, "bigwig_emu: bytes [%lld, %lld) of the file are covered by %lld bytes of cuts\n", (long long)at, (long long)(at + want), (long long)got); return 1; }
            memcpy(file.data() + at, piece.data(), (size_t)want);
        }
    }
    FILE *f = fopen(argv[a0 + 2], "wb");
    if(!f || fwrite(file.data(), 1, file.size(), f) != file.size() || fclose(f)) { perror(argv[a0 + 2]); return 2; }
    delete S;
    return 0;
}
