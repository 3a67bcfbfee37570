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
#include "mdk_deflate_core.h"
#include "mdk_crc32_core.h"

static CrcConst g_crc;
static unsigned long long g_forms[2], g_tokens, g_matches;

static uint32_t crc_member(const uint8_t *d, uint32_t L) {
    uint32_t c[64], t[64];
    for(int lane = 0; lane < 64; lane++) c[lane] = crc_lane(g_crc.T, g_crc.Z, d, L, lane);
    for(int l = 0; l < 6; l++) {
        memcpy(t, c, sizeof t);
        for(int lane = 1 << l; lane < 64; lane++) c[lane] ^= crc_mul(t[lane - (1 << l)], g_crc.lvl[l]);
    }
    return crc_finish(c[63], L, g_crc.p8);
}

static void build_tree(dfl_state &S, uint32_t a0, uint32_t nsym, uint32_t nall, uint32_t limit) {
    for(uint32_t lane = 0; lane < 64; lane++) dfl_tree_counts(S, a0, nsym, lane);
    dfl_tree_two(S, nsym);
    for(;;) {
        for(uint32_t lane = 0; lane < 64; lane++) dfl_tree_rank(S, nsym, lane);
        dfl_tree_merge(S);
        if(S.maxdepth <= limit) break;
        for(uint32_t lane = 0; lane < 64; lane++) dfl_tree_halve(S, nsym, lane);
    }
    for(uint32_t lane = 0; lane < 64; lane++) dfl_tree_clear(S, a0, nall, lane);
    for(uint32_t lane = 0; lane < 64; lane++) dfl_tree_lens(S, a0, lane);
}

// one member: in[0, n) -> slot (DFL_SLOT bytes); its length
static uint32_t compress_member(const uint8_t *in, uint32_t n, uint8_t *slot, uint32_t *tok, dfl_state &S) {
    uint32_t *const slot32 = (uint32_t *)slot;
    for(uint32_t i = 0; i < DFL_HASH; i++) S.head[i] = 0;
    for(uint32_t i = 0; i < DFL_NSYM; i++) S.freq[i] = 0;
    uint32_t e = 0, ntok = 0, m[64];
    for(uint32_t s0 = 0; s0 < n; s0 += 64) {
        for(uint32_t lane = 0; lane < 64; lane++) dfl_stripe_load(S, in, n, s0, lane);
        const bool skip = e >= s0 + 64;
        if(!skip) for(uint32_t lane = 0; lane < 64; lane++) m[lane] = dfl_stripe_match(S, in, n, s0, e, lane);
        for(uint32_t lane = 0; lane < 64; lane++) dfl_stripe_enter(S, n, s0, lane);
        if(skip) continue;
        uint32_t cur = e - s0; uint64_t sel = 0;
        while(cur < 64 && s0 + cur < n) { sel |= 1ull << cur; cur += m[cur] & 511u; }
        e = s0 + cur;
        for(uint32_t lane = 0; lane < 64; lane++) if(sel >> lane & 1) {
            const uint32_t t = dfl_token(S, in, s0 + lane, m[lane]);
            tok[ntok + (uint32_t)__builtin_popcountll(sel & ((1ull << lane) - 1))] = t; g_matches += t >> 31;
        }
        ntok += (uint32_t)__builtin_popcountll(sel);
    }
    g_tokens += ntok;
    S.freq[DFL_EOB] = 1;
    build_tree(S, DFL_LIT0, 286, 286, 15);
    build_tree(S, DFL_DIST0, 30, 30, 15);
    dfl_rle(S);
    build_tree(S, DFL_CL0, 19, 19, 7);
    for(uint32_t lane = 0; lane < 64; lane++) dfl_assign_codes(S, DFL_CL0, 19, lane);
    dfl_choose(S, n);
    g_forms[S.mode]++;
    const uint32_t crc = crc_member(in, n);
    uint32_t stream_bytes;
    if(S.mode == DFL_MODE_STORED) {
        stream_bytes = 5 + n;
        S.first_dw = 0x01u << 16 | (n & 255u) << 24;
        slot[20] = (uint8_t)(n >> 8); slot[21] = (uint8_t)~n; slot[22] = (uint8_t)(~n >> 8);
        for(uint32_t i = 0; i < n; i++) slot[23 + i] = in[i];
    } else {
        for(uint32_t lane = 0; lane < 64; lane++) { dfl_assign_codes(S, DFL_LIT0, 286, lane); dfl_assign_codes(S, DFL_DIST0, 30, lane); }
        const uint32_t nh = dfl_header_items(S), total = nh + ntok + 1;
        uint32_t bitpos = 0;
        for(uint32_t k = 0; k < DFL_WIN; k++) S.win[k] = 0;
        for(uint32_t i0 = 0; i0 < total; i0 += 64) {
            uint64_t v[64]; uint32_t nb[64], run = 0;
            for(uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t i = i0 + lane;
                v[lane] = 0;
                nb[lane] = i < nh ? dfl_header_item(S, i, v[lane]) : i < nh + ntok ? dfl_token_bits(S, tok[i - nh], v[lane]) : i == nh + ntok ? dfl_token_bits(S, DFL_EOB, v[lane]) : 0u;
            }
            const uint32_t abs0 = DFL_STREAM_BIT0 + bitpos, wd0 = abs0 >> 5;
            for(uint32_t lane = 0; lane < 64; lane++) { dfl_win_or(S.win, (abs0 & 31u) + run, v[lane], nb[lane]); run += nb[lane]; }
            bitpos += run;
            const uint32_t nd = ((DFL_STREAM_BIT0 + bitpos) >> 5) - wd0;
            for(uint32_t k = 0; k < nd; k++) { if(wd0 + k == 4) S.first_dw = S.win[k]; else if(wd0 + k < DFL_SLOT / 4) slot32[wd0 + k] = S.win[k]; }
            const uint32_t carry = S.win[nd];
            for(uint32_t k = 0; k < DFL_WIN; k++) S.win[k] = k == 0 ? carry : 0u;
        }
        stream_bytes = (bitpos + 7) >> 3;
        const uint32_t wd0 = (DFL_STREAM_BIT0 + bitpos) >> 5, end = 18 + stream_bytes;
        if(wd0 == 4) S.first_dw = S.win[0];
        else for(uint32_t b = wd0 * 4; b < end; b++) slot[b] = (uint8_t)(S.win[0] >> (8 * (b & 3u)));
    }
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
                      members, in.size(), out_bytes, g_forms[0], g_forms[1], g_tokens, g_matches);
    delete S;
    return 0;
}
