// mdk_deflate_core.h -- one BGZF member compressed by ONE WAVEFRONT (RFC 1951 deflate, RFC 1952 framing as bgzip writes it): the parts a lane
// runs on its own, and the few a single lane runs for all.  Plain C++: compiled for the device by mdk_deflate.hip (k_deflate) and for the
// host by tools/deflate_emu.cpp, which walks the same phases lane by lane and must give the same bytes.
//
// A member's bytes depend on its input alone.  The phases, each a pure function of what the phases before it left behind:
//   stripes   the input in stripes of 64 positions, a lane per position.  A lane's candidate source is the NEAREST earlier position of its own
//             stripe that holds the same four bytes (the stripe's words stand in `w`; a previous bedGraph line is ~30 bytes back), else
//             what the hash table holds for its four bytes.  The table is filled with atomicMax on position + 1 AFTER the stripe's lookups, so a
//             lookup only ever sees positions of earlier stripes, which are settled: no order of lanes can change what it reads.  The
//             candidate is verified byte by byte (up to 258; minimum 4).  Greedy selection walks step[p] = match length or 1 from the
//             position the previous stripe's walk left off at; the selected lanes append their tokens and count their symbols.
//   codes     Huffman code lengths of the three alphabets from the counts: ranks by counting (every lane its symbols), the classic
//             two-queue merge by one lane, the leaves' depths by all.  A tree deeper than the limit (15; 7 for the code-length alphabet) is
//             rebuilt from halved counts -- (f + 1) / 2 keeps every used symbol -- until it fits: always a complete code.  Alphabets with
//             fewer than two used symbols are given dummies, as zlib does, so no tree is a single code.
//   choice    the exact size of the dynamic block against the stored form's; the stored form wins a tie: a member is never longer than
//             18 + 5 + n + 8 bytes, and bytes without structure (random ones, at any length) are stored.  Fixed blocks are not used: they
//             would win only below a few dozen bytes.
//   emission  header items, then tokens, 64 at a time: bit lengths prefix-summed over the wavefront, every lane ORs its bits into a window
//             (OR commutes: order-free) whose complete dwords leave as dword stores.  The dword that holds BSIZE and the stream's first two
//             bytes is kept back and written with the header.
// Nothing is read before in[0] or past in[n - 1]; nothing is written past the member's slot of DFL_SLOT bytes.
#ifndef MDK_DEFLATE_CORE_H
#define MDK_DEFLATE_CORE_H
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define DFL_HD __host__ __device__ __forceinline__
#else
#define DFL_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DFL_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define DFL_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define DFL_ATOMIC_OR(p, v) atomicOr((p), (v))
#else
#define DFL_ATOMIC_MAX(p, v) do { if(*(p) < (v)) *(p) = (v); } while(0)
#define DFL_ATOMIC_ADD(p, v) (*(p) += (v))
#define DFL_ATOMIC_OR(p, v) (*(p) |= (v))
#endif

#define DFL_MEMBER 65280u                 // input bytes of a member: bgzip's cut
#define DFL_SLOT 65536u                   // bytes a member is compressed into: the stored form of 65280 bytes is 65311
#define DFL_HASH_BITS 12
#define DFL_HASH (1u << DFL_HASH_BITS)
#define DFL_MIN_MATCH 4u
#define DFL_MAX_MATCH 258u
#define DFL_MAX_DIST 32768u
#define DFL_LIT0 0u                        // the alphabets in one index space: literal/length [0, 286) of [0, 288), distance [288, 318) of [288, 320), code lengths [320, 339)
#define DFL_DIST0 288u
#define DFL_CL0 320u
#define DFL_NSYM 339u
#define DFL_WIN 104u                       // dwords of the window: 64 tokens of at most 48 bits behind a carried dword
#define DFL_EOB 256u
#define DFL_MODE_STORED 0u
#define DFL_MODE_DYNAMIC 1u
#define DFL_STREAM_BIT0 144u               // the stream starts at byte 18 of the slot

struct dfl_state {
    uint32_t head[DFL_HASH];               // per hash: position + 1 of the latest settled position with it (0: none)
    uint32_t w[64];                        // the stripe's four-byte words
    uint32_t freq[DFL_NSYM];
    uint32_t code[DFL_NSYM];               // bit-reversed code << 8 | length
    uint32_t wf[288];                      // the counts a tree is built from
    uint32_t nodew[576];
    uint32_t rle[320];                     // the code lengths as code-length symbols: symbol | extra value << 8 | extra bits << 16
    uint32_t win[DFL_WIN];
    uint16_t sorted[288], parent[576];
    uint8_t depth[576];
    uint8_t lens[DFL_NSYM + 1];
    uint32_t m, maxdepth, n_rle, nlit, ndist, ncl, mode, first_dw;
};

DFL_HD uint32_t dfl_load32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }       // (any alignment; host and device are little-endian)
DFL_HD uint32_t dfl_hash(uint32_t w) { return (w * 2654435761u) >> (32 - DFL_HASH_BITS); }
DFL_HD uint32_t dfl_log2(uint32_t v) { uint32_t k = 0; while(v >>= 1) k++; return k; }
DFL_HD uint32_t dfl_rev(uint32_t c, uint32_t n) { uint32_t r = 0; for(uint32_t i = 0; i < n; i++) { r = r << 1 | (c & 1u); c >>= 1; } return r; }
// length 3..258 and distance 1..32768 as symbol, number of extra bits and their value (RFC 1951 3.2.5, from the tables' own regularity)
DFL_HD void dfl_len_sym(uint32_t len, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    const uint32_t l = len - 3;
    if(l < 8) { sym = l; eb = 0; ev = 0; }
    else if(l == 255) { sym = 28; eb = 0; ev = 0; }
    else { eb = dfl_log2(l) - 2; sym = 4 * eb + 4 + ((l >> eb) & 3u); ev = l & ((1u << eb) - 1); }
}
DFL_HD void dfl_dist_sym(uint32_t dist, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    const uint32_t d = dist - 1;
    if(d < 4) { sym = d; eb = 0; ev = 0; }
    else { const uint32_t k = dfl_log2(d); eb = k - 1; sym = 2 * k + ((d >> eb) & 1u); ev = d & ((1u << eb) - 1); }
}
DFL_HD uint32_t dfl_len_extra(uint32_t k) { return k < 8 || k == 28 ? 0 : (k - 4) >> 2; }       // extra bits of length symbol 257 + k
DFL_HD uint32_t dfl_dist_extra(uint32_t k) { return k < 4 ? 0 : (k - 2) >> 1; }

// ---- stripes ----
DFL_HD void dfl_stripe_load(dfl_state &S, const uint8_t *in, uint32_t n, uint32_t s0, uint32_t lane) {
    const uint32_t p = s0 + lane;
    S.w[lane] = p + 4 <= n ? dfl_load32(in + p) : 0u;
}
DFL_HD uint32_t dfl_match_len(const uint8_t *in, uint32_t q, uint32_t p, uint32_t maxlen) {
    uint32_t l = 4;
    while(l + 16 <= maxlen) {                 // 16 bytes a round: eight loads that do not wait for one another
        const uint8_t *a = in + q + l, *b = in + p + l;
        const uint32_t x = (dfl_load32(a) ^ dfl_load32(b)) | (dfl_load32(a + 4) ^ dfl_load32(b + 4)) | (dfl_load32(a + 8) ^ dfl_load32(b + 8)) | (dfl_load32(a + 12) ^ dfl_load32(b + 12));
        if(x) break;
        l += 16;
    }
    while(l + 4 <= maxlen && dfl_load32(in + q + l) == dfl_load32(in + p + l)) l += 4;
    while(l < maxlen && in[q + l] == in[p + l]) l++;
    return l;
}
// position s0 + lane: step | distance << 9.  step: the match length, 1 for a literal, 0 past the input.  Positions before `e`, the next position
// the greedy walk reaches, lie inside a match already and are not looked at
DFL_HD uint32_t dfl_stripe_match(const dfl_state &S, const uint8_t *in, uint32_t n, uint32_t s0, uint32_t e, uint32_t lane) {
    const uint32_t p = s0 + lane;
    if(p >= n) return 0;
    if(p < e || p + 4 > n) return 1;
    const uint32_t w = S.w[lane];
    uint32_t q = 0xffffffffu;
    for(uint32_t j = 0; j < 64; j++) { const uint32_t x = S.w[j]; if(j < lane && x == w) q = s0 + j; }       // the last hit is the nearest; every lane reads the same word: no lane waits for another's exit
    if(q == 0xffffffffu) {
        const uint32_t hq = S.head[dfl_hash(w)];                 // < s0 + 1: only earlier stripes have been entered
        if(hq && hq <= s0 && p - (hq - 1) <= DFL_MAX_DIST && dfl_load32(in + hq - 1) == w) q = hq - 1;
    }
    if(q == 0xffffffffu) return 1;
    const uint32_t room = n - p;
    return dfl_match_len(in, q, p, room < DFL_MAX_MATCH ? room : DFL_MAX_MATCH) | (p - q) << 9;
}
DFL_HD void dfl_stripe_enter(dfl_state &S, uint32_t n, uint32_t s0, uint32_t lane) {
    const uint32_t p = s0 + lane;
    if(p + 4 <= n) DFL_ATOMIC_MAX(&S.head[dfl_hash(S.w[lane])], p + 1);
}
// a selected position's token -- a literal is its byte, a match 1 << 31 | (length - 3) << 16 | (distance - 1) -- and its symbols counted
DFL_HD uint32_t dfl_token(dfl_state &S, const uint8_t *in, uint32_t p, uint32_t m) {
    const uint32_t step = m & 511u;
    if(step < DFL_MIN_MATCH) { const uint32_t b = in[p]; DFL_ATOMIC_ADD(&S.freq[b], 1u); return b; }
    const uint32_t dist = m >> 9;
    uint32_t ls, ds, eb, ev;
    dfl_len_sym(step, ls, eb, ev); dfl_dist_sym(dist, ds, eb, ev);
    DFL_ATOMIC_ADD(&S.freq[257 + ls], 1u); DFL_ATOMIC_ADD(&S.freq[DFL_DIST0 + ds], 1u);
    return 0x80000000u | (step - 3) << 16 | (dist - 1);
}

// ---- codes: the alphabet [a0, a0 + nsym) ----
DFL_HD void dfl_tree_counts(dfl_state &S, uint32_t a0, uint32_t nsym, uint32_t lane) { for(uint32_t s = lane; s < nsym; s += 64) S.wf[s] = S.freq[a0 + s]; }
// one lane: at least two used symbols
DFL_HD void dfl_tree_two(dfl_state &S, uint32_t nsym) {
    uint32_t m = 0;
    for(uint32_t s = 0; s < nsym; s++) m += S.wf[s] != 0;
    while(m < 2) { if(!S.wf[0]) S.wf[0] = 1; else S.wf[1] = 1; m++; }
    S.m = m;
}
// every lane its symbols: the used symbols in ascending (count, symbol) as the leaves 0 .. m - 1
DFL_HD void dfl_tree_rank(dfl_state &S, uint32_t nsym, uint32_t lane) {
    for(uint32_t s = lane; s < nsym; s += 64) {
        const uint32_t f = S.wf[s];
        if(!f) continue;
        uint32_t r = 0;
        for(uint32_t t = 0; t < nsym; t++) { const uint32_t g = S.wf[t]; r += g && (g < f || (g == f && t < s)); }
        S.sorted[r] = (uint16_t)s; S.nodew[r] = f;
    }
}
// one lane: the merge (leaves and made nodes are two queues in ascending weight; a leaf goes first on a tie) and the made nodes' depths
DFL_HD void dfl_tree_merge(dfl_state &S) {
    const uint32_t m = S.m;
    uint32_t a = 0, b = m, k = m;
    while(k < 2 * m - 1) {
        uint32_t x[2];
        for(int j = 0; j < 2; j++) x[j] = (a < m && (b >= k || S.nodew[a] <= S.nodew[b])) ? a++ : b++;
        S.nodew[k] = S.nodew[x[0]] + S.nodew[x[1]];
        S.parent[x[0]] = (uint16_t)k; S.parent[x[1]] = (uint16_t)k; k++;
    }
    S.depth[2 * m - 2] = 0;
    uint32_t mx = 0;
    for(uint32_t i = 2 * m - 2; i-- > m; ) { const uint32_t d = S.depth[S.parent[i]] + 1u; S.depth[i] = (uint8_t)d; if(d > mx) mx = d; }
    S.maxdepth = mx + 1;
}
DFL_HD void dfl_tree_halve(dfl_state &S, uint32_t nsym, uint32_t lane) { for(uint32_t s = lane; s < nsym; s += 64) { const uint32_t f = S.wf[s]; if(f) S.wf[s] = (f + 1) >> 1; } }
DFL_HD void dfl_tree_clear(dfl_state &S, uint32_t a0, uint32_t nall, uint32_t lane) { for(uint32_t s = lane; s < nall; s += 64) S.lens[a0 + s] = 0; }
DFL_HD void dfl_tree_lens(dfl_state &S, uint32_t a0, uint32_t lane) { for(uint32_t i = lane; i < S.m; i += 64) S.lens[a0 + S.sorted[i]] = (uint8_t)(S.depth[S.parent[i]] + 1u); }
// every lane its symbols: the canonical code (RFC 1951 3.2.2) of the lengths of [a0, a0 + nall), bit-reversed
DFL_HD void dfl_assign_codes(dfl_state &S, uint32_t a0, uint32_t nall, uint32_t lane) {
    for(uint32_t s = lane; s < nall; s += 64) {
        const uint32_t l = S.lens[a0 + s];
        uint32_t c = 0;
        if(l) for(uint32_t t = 0; t < nall; t++) { const uint32_t lt = S.lens[a0 + t]; if(lt && lt < l) c += 1u << (l - lt); else if(lt == l && t < s) c++; }
        S.code[a0 + s] = l ? dfl_rev(c, l) << 8 | l : 0u;
    }
}

// one lane: the literal/length and the distance lengths as code-length symbols (runs as zlib cuts them: 18 and 17 for zeros, 16 behind a
// length written once), each alphabet for itself, and the code-length alphabet's counts
DFL_HD void dfl_rle_one(dfl_state &S, uint32_t a0, uint32_t cnt) {
    uint32_t i = 0, k = S.n_rle;
    while(i < cnt) {
        const uint32_t v = S.lens[a0 + i];
        uint32_t r = 1;
        while(i + r < cnt && S.lens[a0 + i + r] == v) r++;
        uint32_t sym, ev = 0, nb = 0;
        if(v == 0 && r >= 11) { if(r > 138) r = 138; sym = 18; ev = r - 11; nb = 7; }
        else if(v == 0 && r >= 3) { sym = 17; ev = r - 3; nb = 3; }
        else if(v && r >= 4) { S.rle[k++] = v; S.freq[DFL_CL0 + v]++; r = r - 1 > 6 ? 6 : r - 1; sym = 16; ev = r - 3; nb = 2; i++; }
        else { sym = v; r = 1; }
        S.rle[k++] = sym | ev << 8 | nb << 16; S.freq[DFL_CL0 + sym]++;
        i += r;
    }
    S.n_rle = k;
}
DFL_HD void dfl_rle(dfl_state &S) {
    uint32_t nlit = 286, ndist = 30;
    while(nlit > 257 && !S.lens[nlit - 1]) nlit--;
    while(ndist > 1 && !S.lens[DFL_DIST0 + ndist - 1]) ndist--;
    S.nlit = nlit; S.ndist = ndist; S.n_rle = 0;
    for(uint32_t s = 0; s < 19; s++) S.freq[DFL_CL0 + s] = 0;
    dfl_rle_one(S, DFL_LIT0, nlit); dfl_rle_one(S, DFL_DIST0, ndist);
}
DFL_HD uint32_t dfl_cl_order(uint32_t k) { return k < 3 ? 16 + k : k == 3 ? 0 : (k & 1u) ? 8 - ((k - 3) >> 1) : 8 + ((k - 4) >> 1) + 0u; }       // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15

// one lane: the form.  The exact bit count of the dynamic block against the stored form's 5 + n bytes
DFL_HD void dfl_choose(dfl_state &S, uint32_t n) {
    uint32_t ncl = 19;
    while(ncl > 4 && !S.lens[DFL_CL0 + dfl_cl_order(ncl - 1)]) ncl--;
    S.ncl = ncl;
    uint64_t dyn = 3 + 14 + 3 * ncl;
    for(uint32_t i = 0; i < S.n_rle; i++) { const uint32_t it = S.rle[i]; dyn += S.lens[DFL_CL0 + (it & 255u)] + (it >> 16); }
    for(uint32_t s = 0; s < 286; s++) { const uint32_t f = S.freq[s], x = s > 256 ? dfl_len_extra(s - 257) : 0; dyn += (uint64_t)f * (S.lens[s] + x); }
    for(uint32_t s = 0; s < 30; s++) { const uint32_t f = S.freq[DFL_DIST0 + s], x = dfl_dist_extra(s); dyn += (uint64_t)f * (S.lens[DFL_DIST0 + s] + x); }
    S.mode = 5ull + n <= (dyn + 7) >> 3 ? DFL_MODE_STORED : DFL_MODE_DYNAMIC;
}

// ---- emission ----
// item i of the block's header, of 4 + ncl + n_rle: its bits and their number
DFL_HD uint32_t dfl_header_item(const dfl_state &S, uint32_t i, uint64_t &v) {
    if(i == 0) { v = 1u | 2u << 1; return 3; }                    // the final block, dynamic
    if(i == 1) { v = S.nlit - 257; return 5; }
    if(i == 2) { v = S.ndist - 1; return 5; }
    if(i == 3) { v = S.ncl - 4; return 4; }
    if(i < 4 + S.ncl) { v = S.lens[DFL_CL0 + dfl_cl_order(i - 4)]; return 3; }
    const uint32_t it = S.rle[i - 4 - S.ncl], c = S.code[DFL_CL0 + (it & 255u)], l = c & 255u;
    v = (uint64_t)(c >> 8) | (uint64_t)((it >> 8) & 255u) << l;
    return l + (it >> 16);
}
DFL_HD uint32_t dfl_header_items(const dfl_state &S) { return 4u + S.ncl + S.n_rle; }
// a token's bits (DFL_EOB: the end of the block) and their number, at most 48
DFL_HD uint32_t dfl_token_bits(const dfl_state &S, uint32_t tok, uint64_t &v) {
    if(!(tok >> 31)) { const uint32_t c = S.code[tok]; v = c >> 8; return c & 255u; }
    uint32_t ls, leb, lev, ds, deb, dev;
    dfl_len_sym(((tok >> 16) & 255u) + 3, ls, leb, lev); dfl_dist_sym((tok & 32767u) + 1, ds, deb, dev);
    const uint32_t lc = S.code[257 + ls], dc = S.code[DFL_DIST0 + ds];
    uint32_t nb = lc & 255u;
    v = lc >> 8;
    v |= (uint64_t)lev << nb; nb += leb;
    v |= (uint64_t)(dc >> 8) << nb; nb += dc & 255u;
    v |= (uint64_t)dev << nb; nb += deb;
    return nb;
}
// nb bits of v into the window at bit `bit`
DFL_HD void dfl_win_or(uint32_t *win, uint32_t bit, uint64_t v, uint32_t nb) {
    if(!nb) return;
    const uint32_t k = bit >> 5, sh = bit & 31u;
    const uint64_t x = v << sh;
    const uint32_t w0 = (uint32_t)x, w1 = (uint32_t)(x >> 32), w2 = sh ? (uint32_t)(v >> (64 - sh)) : 0u;
    if(w0) DFL_ATOMIC_OR(&win[k], w0);
    if(w1) DFL_ATOMIC_OR(&win[k + 1], w1);
    if(w2) DFL_ATOMIC_OR(&win[k + 2], w2);
}
// the 18 header bytes as dwords 0 .. 4 of the slot (dword 4 takes the stream's first two bytes from `first_dw`), and byte i of the trailer
DFL_HD uint32_t dfl_header_dword(uint32_t i, uint32_t member_bytes, uint32_t first_dw) {
    return i == 0 ? 0x04088b1fu : i == 1 ? 0u : i == 2 ? 0x0006ff00u : i == 3 ? 0x00024342u : ((member_bytes - 1) & 0xffffu) | (first_dw & 0xffff0000u);
}
DFL_HD uint8_t dfl_trailer_byte(uint32_t i, uint32_t crc, uint32_t n) { return (uint8_t)((i < 4 ? crc : n) >> (8 * (i & 3u))); }
DFL_HD uint8_t dfl_eof_byte(uint32_t i) { return i == 0 ? 0x1f : i == 1 ? 0x8b : i == 2 ? 8 : i == 3 ? 4 : i == 9 ? 0xff : i == 10 ? 6 : i == 12 ? 0x42 : i == 13 ? 0x43 : i == 14 ? 2 : i == 16 ? 0x1b : i == 18 ? 3 : 0; }
#endif
