// tabix_emu -- TEST INFRASTRUCTURE: the host build of csrc/mdk_tabix_core.h.  The members of a BGZF file are inflated with zlib (as inflate_emu
// does), the text is walked line after line through tbx_line / tbx_flags -- where the device (csrc/mdk_tabix.hip) has a lane per line, a scan
// and a compaction --, the records go through tbx_builder, and the payload becomes BGZF through the phases of csrc/mdk_deflate_core.h lane by
// lane (tools/deflate_walk.h, as bigwig_emu does).
//   tabix_emu [--payload] in.gz format col_seq col_beg col_end meta skip out.tbi     --payload: the payload as it is, not BGZF
// A refused file: "line N: why" on stderr, exit status 3, and no output file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include <string>
#include <vector>
#include "mdk_tabix_core.h"
#include "deflate_walk.h"
#include "mdk_crc32_core.h"

static CrcConst g_crc;
static dfl_walk_stats g_st;

static uint32_t crc_member(const uint8_t *d, uint32_t L) {
    uint32_t c[64], t[64];
    for(int lane = 0; lane < 64; lane++) c[lane] = crc_lane(g_crc.T, g_crc.Z, d, L, lane);
    for(int l = 0; l < 6; l++) {
        memcpy(t, c, sizeof t);
        for(int lane = 1 << l; lane < 64; lane++) c[lane] ^= crc_mul(t[lane - (1 << l)], g_crc.lvl[l]);
    }
    return crc_finish(c[63], L, g_crc.p8);
}

static std::vector<uint8_t> bgzf(const std::vector<uint8_t> &in) {
    std::vector<uint8_t> out;
    std::vector<uint32_t> tok(DFL_MEMBER), slot32(DFL_SLOT / 4);
    dfl_state *S = new dfl_state();
    for(size_t o = 0; o < in.size(); o += DFL_MEMBER) {
        const uint32_t n = (uint32_t)(in.size() - o < DFL_MEMBER ? in.size() - o : DFL_MEMBER);
        std::vector<uint8_t> piece(in.begin() + o, in.begin() + o + n);        // exactly n bytes: a read outside is a read outside an allocation
        uint8_t *slot = (uint8_t *)slot32.data();
        const uint32_t stream_bytes = dfl_walk_stream(*S, piece.data(), n, slot, DFL_SLOT, tok.data(), g_st);
        const uint32_t crc = crc_member(piece.data(), n), member = 18 + stream_bytes + 8;
        for(uint32_t i = 0; i < 5; i++) slot32[i] = dfl_header_dword(i, member, S->first_dw);
        for(uint32_t i = 0; i < 8; i++) slot[18 + stream_bytes + i] = dfl_trailer_byte(i, crc, n);
        out.insert(out.end(), slot, slot + member);
    }
    for(uint32_t i = 0; i < 28; i++) out.push_back(dfl_eof_byte(i));
    delete S;
    return out;
}

int main(int argc, char **argv) {
    bool raw = false; int a0 = 1;
    if(argc > 1 && !strcmp(argv[1], "--payload")) { raw = true; a0 = 2; }
    if(argc - a0 != 8) { fprintf(stderr, "usage: tabix_emu [--payload] in.gz format col_seq col_beg col_end meta skip out.tbi\n"); return 2; }
    tbx_builder B;
    B.cf = tbx_conf{(int32_t)strtol(argv[a0 + 1], 0, 0), atoi(argv[a0 + 2]), atoi(argv[a0 + 3]), atoi(argv[a0 + 4]), atoi(argv[a0 + 5]), atoi(argv[a0 + 6])};
    crc_make_const(g_crc);
    std::vector<uint8_t> file;
    {
        FILE *f = fopen(argv[a0], "rb");
        if(!f) { perror(argv[a0]); return 2; }
        uint8_t buf[1 << 16]; size_t got;
        while((got = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + got);
        fclose(f);
    }
    // ---- the members, and the text ----
    std::vector<uint8_t> text; std::vector<tbx_member> members; uint64_t c_end = 0;
    for(size_t o = 0; o < file.size();) {
        if(o + 18 > file.size() || file[o] != 0x1f || file[o + 1] != 0x8b) { fprintf(stderr, "tabix_emu: no BGZF member at byte %zu\n", o); return 2; }
        const uint32_t xlen = file[o + 10] | file[o + 11] << 8;
        uint32_t bs = 0;
        for(size_t x = o + 12; x + 4 <= o + 12 + xlen;) {
            const uint32_t slen = file[x + 2] | file[x + 3] << 8;
            if(file[x] == 66 && file[x + 1] == 67 && slen == 2) bs = (file[x + 4] | file[x + 5] << 8) + 1u;
            x += 4 + slen;
        }
        if(!bs || o + bs > file.size()) { fprintf(stderr, "tabix_emu: no BGZF member at byte %zu\n", o); return 2; }
        const uint32_t isize = file[o + bs - 4] | file[o + bs - 3] << 8 | file[o + bs - 2] << 16 | (uint32_t)file[o + bs - 1] << 24;
        if(isize) {
            std::vector<uint8_t> out(isize);
            z_stream z; memset(&z, 0, sizeof z);
            if(inflateInit2(&z, -15) != Z_OK) return 2;
            z.next_in = file.data() + o + 12 + xlen; z.avail_in = bs - 12 - xlen - 8; z.next_out = out.data(); z.avail_out = isize;
            const int rc = inflate(&z, Z_FINISH);
            inflateEnd(&z);
            if(rc != Z_STREAM_END || z.total_out != isize) { fprintf(stderr, "tabix_emu: the member at byte %zu does not inflate\n", o); return 2; }
            members.push_back(tbx_member{(uint64_t)o, (uint64_t)text.size(), isize});
            text.insert(text.end(), out.begin(), out.end());
            c_end = o + bs;
        }
        o += bs;
    }
    // ---- the lines ----
    const int64_t bytes = (int64_t)text.size();
    unsigned long long refused = ~0ull;                    // line << 8 | code
    int64_t line = 0, prev_at = -1; tbx_entry prev; uint64_t prev_end = 0, ord = 0;
    memset(&prev, 0, sizeof prev);
    for(int64_t at = 0; at < bytes && refused == ~0ull;) {
        line++;
        // the line in a buffer of exactly the bytes tbx_line may read: a read outside is a read outside an allocation
        const int64_t avail = bytes - at;
        std::vector<uint8_t> img(text.begin() + at, text.begin() + at + (avail < TBX_MAX_LINE ? avail : TBX_MAX_LINE));
        tbx_entry e;
        const int rc = tbx_line(img.data(), avail, line <= B.cf.skip, B.cf, e);
        int64_t next = at;
        while(next < bytes && text[next] != '\n') next++;
        if(next < bytes) next++;
        if(rc > 0) { refused = (unsigned long long)line << 8 | (unsigned)rc; break; }
        if(rc == 0) {
            bool unordered;
            const uint32_t fl = tbx_flags(prev_at >= 0, text.data() + (prev_at >= 0 ? prev_at : 0), prev, img.data(), e, unordered);
            if(unordered) { refused = (unsigned long long)line << 8 | TBX_E_ORDER; break; }
            if(fl) {
                const tbx_rec r = {(uint64_t)at, prev_end, e.bin, e.beg0, e.end0, fl, (uint32_t)ord, e.name_len};
                B.add(r, ord, img.data() + e.name_off);
                if(B.returned >= 0) { refused = (unsigned long long)line << 8 | TBX_E_RETURN; break; }
            }
            prev = e; prev_at = at; prev_end = (uint64_t)next; ord++;
        }
        at = next;
    }
    if(refused != ~0ull) {
        const int code = (int)(refused & 0xff);
        if(code == TBX_E_RETURN) fprintf(stderr, "line %llu: not sorted: contig %s appears in two places\n", refused >> 8, B.returned_name.c_str());
        else fprintf(stderr, "line %llu: %s\n", refused >> 8, tbx_error_text(code));
        return 3;
    }
    B.finish(prev_end, ord);
    const std::vector<uint8_t> payload = B.payload(members, c_end);
    const std::vector<uint8_t> out = raw ? payload : bgzf(payload);
    FILE *f = fopen(argv[a0 + 7], "wb");
    if(!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f)) { perror(argv[a0 + 7]); return 2; }
    return 0;
}
