// deflate_emu -- TEST INFRASTRUCTURE: the device BGZF compressor (csrc/mdk_deflate.hip k_deflate) on the host, in the kernel's own
// decomposition: the same phases of csrc/mdk_deflate_core.h, walked lane by lane where the kernel runs 64 lanes at once, with a loop where the
// kernel has a wave prefix sum or reads another lane's register.  stdin -> BGZF on stdout: members of 65280 input bytes, then the EOF member
// (--no-eof leaves it out).  The bytes must be the device's (tests/test_gpu_deflate.py) and zlib must inflate them (tests/test_deflate_cpu.py).
//   deflate_emu [--no-eof] [--stats] < text > text.gz         --stats: members, bytes, forms (stored, dynamic) and tokens on stderr
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
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

// one member: in[0, n) -> slot (DFL_SLOT bytes); its length
static uint32_t compress_member(const uint8_t *in, uint32_t n, uint8_t *slot, uint32_t *tok, dfl_state &S) {
    uint32_t *const slot32 = (uint32_t *)slot;
    const uint32_t stream_bytes = dfl_walk_stream(S, in, n, slot, DFL_SLOT, tok, g_st);
    const uint32_t crc = crc_member(in, n);
    const uint32_t member = 18 + stream_bytes + 8;
    for(uint32_t i = 0; i < 5; i++) slot32[i] = dfl_header_dword(i, member, S.first_dw);
    for(uint32_t i = 0; i < 8; i++) slot[18 + stream_bytes + i] = dfl_trailer_byte(i, crc, n);
    return member;
}

int main(int argc, char **argv) {
    bool eof = true, stats = false;
    for(int i = 1; i < argc; i++) {
        if(!strcmp(argv[i], "--no-eof")) eof = false;
        else if(!strcmp(argv[i], "--stats")) stats = true;
        else { fprintf(stderr, "usage: deflate_emu [--no-eof] [--stats] < text > text.gz\n"); return 2; }
    }
    crc_make_const(g_crc);
    std::vector<uint8_t> in;
    { uint8_t buf[1 << 16]; size_t got; while((got = fread(buf, 1, sizeof buf, stdin)) > 0) in.insert(in.end(), buf, buf + got); }
    std::vector<uint32_t> tok(DFL_MEMBER), slot32(DFL_SLOT / 4);
    dfl_state *S = new dfl_state();
    unsigned long long out_bytes = 0, members = 0;
    for(size_t o = 0; o < in.size(); o += DFL_MEMBER) {
        const uint32_t n = (uint32_t)(in.size() - o < DFL_MEMBER ? in.size() - o : DFL_MEMBER);
        // the member's input in a buffer of exactly n bytes: a read before byte 0 or past byte n - 1 is a read outside an allocation
        std::vector<uint8_t> piece(in.begin() + o, in.begin() + o + n);
        const uint32_t len = compress_member(piece.data(), n, (uint8_t *)slot32.data(), tok.data(), *S);
        if(len > DFL_SLOT || len > 18 + 5 + n + 8) { fprintf(stderr, "deflate_emu: member %llu is %u bytes\n", members, len); return 1; }
        if(fwrite(slot32.data(), 1, len, stdout) != len) return 2;
        out_bytes += len; members++;
    }
    if(eof) { uint8_t e[28]; for(uint32_t i = 0; i < 28; i++) e[i] = dfl_eof_byte(i); if(fwrite(e, 1, 28, stdout) != 28) return 2; out_bytes += 28; }
    if(stats) fprintf(stderr, "{\"members\": %llu, \"in_bytes\": %zu, \"out_bytes\": %llu, \"stored\": %llu, \"dynamic\": %llu, \"tokens\": %llu, \"matches\": %llu}\n",
                      members, in.size(), out_bytes, g_st.forms[0], g_st.forms[1], g_st.tokens, g_st.matches);
    delete S;
    return 0;
}
