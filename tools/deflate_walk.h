// deflate_walk.h -- TEST INFRASTRUCTURE: the phases of csrc/mdk_deflate_core.h walked lane by lane on the host, where the device
// (csrc/mdk_deflate.hip k_deflate) runs 64 lanes at once: a loop where the kernel has a wave prefix sum or reads another lane's
// register.  Shared by tools/deflate_emu.cpp (BGZF members) and tools/bigwig_emu.cpp (a bigWig's zlib sections), which frame the stream.
#ifndef DEFLATE_WALK_H
#define DEFLATE_WALK_H
#include "mdk_deflate_core.h"

struct dfl_walk_stats { unsigned long long forms[2], tokens, matches; };

static void dfl_walk_tree(dfl_state &S, uint32_t a0, uint32_t nsym, uint32_t nall, uint32_t limit) {
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

// in[0, n) as one raw RFC 1951 stream from byte 18 of `slot` (slot_bytes long); the number of the stream's bytes.  The stream's first two bytes are
// the upper half of S.first_dw, which the caller completes into dword 4 of the slot with its own framing
static uint32_t dfl_walk_stream(dfl_state &S, const uint8_t *in, uint32_t n, uint8_t *slot, uint32_t slot_bytes, uint32_t *tok, dfl_walk_stats &st) {
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
            tok[ntok + (uint32_t)__builtin_popcountll(sel & ((1ull << lane) - 1))] = t; st.matches += t >> 31;
        }
        ntok += (uint32_t)__builtin_popcountll(sel);
    }
    st.tokens += ntok;
    S.freq[DFL_EOB] = 1;
    dfl_walk_tree(S, DFL_LIT0, 286, 286, 15);
    dfl_walk_tree(S, DFL_DIST0, 30, 30, 15);
    dfl_rle(S);
    dfl_walk_tree(S, DFL_CL0, 19, 19, 7);
    for(uint32_t lane = 0; lane < 64; lane++) dfl_assign_codes(S, DFL_CL0, 19, lane);
    dfl_choose(S, n);
    st.forms[S.mode]++;
    uint32_t stream_bytes;
    if(S.mode == DFL_MODE_STORED) {
        stream_bytes = 5 + n;
        if(23 + n > slot_bytes) return stream_bytes;
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
            for(uint32_t k = 0; k < nd; k++) { if(wd0 + k == 4) S.first_dw = S.win[k]; else if(wd0 + k < slot_bytes / 4) slot32[wd0 + k] = S.win[k]; }
            const uint32_t carry = S.win[nd];
            for(uint32_t k = 0; k < DFL_WIN; k++) S.win[k] = k == 0 ? carry : 0u;
        }
        stream_bytes = (bitpos + 7) >> 3;
        const uint32_t wd0 = (DFL_STREAM_BIT0 + bitpos) >> 5, end = 18 + stream_bytes;
        if(wd0 == 4) S.first_dw = S.win[0];
        else for(uint32_t b = wd0 * 4; b < end; b++) slot[b] = (uint8_t)(S.win[0] >> (8 * (b & 3u)));
    }
    return stream_bytes;
}
#endif
