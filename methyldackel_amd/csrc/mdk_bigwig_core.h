// mdk_bigwig_core.h -- a table of calls as a bigWig track: THE RULE, plain C++ for the device and the host.  Built for the host by
// tools/bigwig_emu.cpp and for the device by mdk_bigwig.hip (libmdk_track.so): both must give the same file byte for byte.
// bbi version 4, little-endian; the file's bytes are a function of the columns and the arguments alone.
//
// Rows.  Row i is the item [start, end) of contig `contig` with the value
//   percent    (float)(((double)m * 100.0) / (double)(m + u))        one IEEE division, one rounding to float, no contraction
//   coverage   (float)(m + u)                                        the sum formed in 64 bits, rounded once
// Refused (bw_row_check, bw_pair_check; the row with the smallest number is named, of two refusals of one row the smaller code): a contig outside
// the list, start < 0, end <= start or end past the contig; a negative count; m + u == 0 under percent; rows not strictly ascending in
// (contig, start) -- the later row is named --; a row whose end exceeds the next row's start on its contig -- the earlier row is named.
//
// File.  In this order, nothing between the parts:
//   header (64)          magic 888FFC26, version 4, zoom levels, the offsets of the chromosome tree, the data and the main index, fieldCount 0,
//                        definedFieldCount 0, autoSql 0, the offset of the total summary, uncompressBufSize (the largest raw section, data or
//                        zoom; 0 without rows), 8 reserved bytes
//   zoom headers (24 each, written levels only)   reductionLevel (the bin width), reserved, data offset, index offset
//   total summary (40)   basesCovered (u64), min, max, sum, sumSquares (doubles): level 7's bins added in ascending (contig, bin) order
//   chromosome B+ tree   header (32: magic 78CA8C91, block size 256, key size = the longest name (at least 1), value size 8, item count, 8 reserved),
//                        then the nodes, root first, a level after the other: every contig, covered or not, in ascending order of its zero-padded
//                        name (the order of the list among equal names), as (name, index in the list, length); leaves of up to 256, one level of
//                        (first name, child offset) nodes above for every factor of 256
//   data count (8)       the number of sections
//   data sections        bedGraph sections (type 1) of up to 1024 rows that never span contigs: a 24-byte header (contig, first start, last end,
//                        step 0, span 0, type 1, reserved 0, item count) and 12 bytes a row (start, end, value); each ONE zlib stream: 78 9C, one
//                        raw RFC 1951 stream made by the rule of mdk_deflate_core.h (a dynamic block, or a stored one where that is no larger),
//                        Adler-32 big-endian
//   main index           the R-tree (bw_rtree) over the data sections
//   per written level    the record count (4), the records in sections of up to 512, each a zlib stream as above (a section may span contigs),
//                        and the R-tree over them
//   magic (4)            once more, as the UCSC writer ends a file
// R-tree: header (48: magic 2468ACE0, block size 256, item count, the bounds of all items (first contig, first start, last contig, last end), the
// offset where the indexed data ends, items per slot (1024; 512 for a zoom level), 4 reserved), then the nodes root first, a level after the other:
// leaves (1, 0, count; per section contig, start, contig, end, offset, size) of up to 256 sections, nodes (0, 0, count; per child its bounds and its
// offset) of up to 256 children above them until one node is the root.  No section gives one leaf of count 0.
//
// Zoom.  Level k = 0 .. 7 has bins of w = 1024 * 4^k bases, aligned to multiples of w from base 0 of every contig; bin b of a contig of `len` bases
// covers [b w, min((b + 1) w, len)).  A bin's summary: validCount (the covered bases), min, max (floats), sum and sumSquares (doubles).
//   level 0   the bin's rows in ascending order, each with the bases it has inside the bin: sum = sum + value * bases, then
//             sumSquares = sumSquares + (value * value) * bases, in double, every operation rounded on its own (no fused multiply-add)
//   level k   the bin's up to four children 4 b .. 4 b + 3 of level k - 1 in ascending order: sums added from the children's doubles
// A bin with validCount 0 is no record.  A record is contig, start, end, validCount, min, max, (float)sum, (float)sumSquares: 32 bytes, the casts
// made only here.  All eight levels are computed; level k is WRITTEN if it has fewer than half as many records as the level written last
// (the first: as the table has rows).
#ifndef MDK_BIGWIG_CORE_H
#define MDK_BIGWIG_CORE_H
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>

#if defined(__HIPCC__)
#define BW_HD __host__ __device__ __forceinline__
#else
#define BW_HD static inline
#endif
#if defined(__clang__)
#define BW_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define BW_NO_CONTRACT                     // (gcc: built with -ffp-contract=off, tools/bigwig_emu)
#endif

#define BW_MAGIC 0x888FFC26u
#define BW_CHROM_MAGIC 0x78CA8C91u
#define BW_RTREE_MAGIC 0x2468ACE0u
#define BW_BLOCK 256u                      // children of a tree node, of either tree
#define BW_ITEMS 1024u                     // rows of a data section
#define BW_ZITEMS 512u                     // records of a zoom section
#define BW_LEVELS 8
#define BW_W0_SHIFT 10                     // level k's bins are 1 << (10 + 2 k) bases wide
#define BW_RAW_STRIDE 16384u               // bytes between two raw sections: a data section has at most 24 + 12 * 1024, a zoom section 32 * 512
#define BW_SLOT 16448u                     // bytes a section is compressed into: 16 unused, 78 9C, the stream (at most 5 + 16384 stored), the Adler-32
#define BW_SLOT_LEAD 16u                   // the zlib stream starts here: its two header bytes fill up the dword the raw stream starts in (mdk_deflate_core.h first_dw)
#define BW_MAX_ROWS (1ll << 30)
#define BW_MAX_BINS (1ll << 30)
enum { BW_VALUE_PERCENT = 0, BW_VALUE_COVERAGE = 1 };
enum { BW_E_ROW = 1, BW_E_NEGATIVE = 2, BW_E_EMPTY = 3, BW_E_ORDER = 4, BW_E_OVERLAP = 5 };

BW_HD float bw_value(int mode, int32_t m, int32_t u) {
    BW_NO_CONTRACT
    const int64_t cov = (int64_t)m + (int64_t)u;
    if(mode == BW_VALUE_COVERAGE) return (float)cov;
    const double x = (double)m * 100.0;
    const double q = x / (double)cov;
    return (float)q;
}
// what is wrong with a row by itself, and with a row behind the row before it
BW_HD uint32_t bw_row_check(int mode, int32_t n_contigs, const uint32_t *len, int32_t c, int32_t s, int32_t e, int32_t m, int32_t u) {
    if(c < 0 || c >= n_contigs || s < 0 || e <= s || (uint32_t)e > len[c]) return BW_E_ROW;
    if(m < 0 || u < 0) return BW_E_NEGATIVE;
    if(mode == BW_VALUE_PERCENT && (int64_t)m + (int64_t)u == 0) return BW_E_EMPTY;
    return 0;
}
BW_HD uint32_t bw_pair_check(int32_t c0, int32_t s0, int32_t e0, int32_t c1, int32_t s1) {
    if(c1 < c0 || (c1 == c0 && s1 <= s0)) return BW_E_ORDER;
    if(c1 == c0 && e0 > s1) return BW_E_OVERLAP;
    return 0;
}
BW_HD const char *bw_error_text(uint32_t code) {
    return code == BW_E_ROW ? "its contig is not in the list, or its interval is empty, negative or past the contig's end" :
           code == BW_E_NEGATIVE ? "a negative count" :
           code == BW_E_EMPTY ? "nmeth + nunmeth is 0, which has no percentage (select the covered rows, or write the coverage)" :
           code == BW_E_ORDER ? "it is not behind the row before it: the rows must be strictly ascending in (contig, start)" :
           code == BW_E_OVERLAP ? "its end is past the next row's start; merged CpG and CHG rows overlap at CGG: pass one context" : "?";
}

BW_HD uint32_t bw_level_shift(int k) { return BW_W0_SHIFT + 2u * (uint32_t)k; }
BW_HD uint32_t bw_level_bins(uint32_t len, int k) { const uint32_t sh = bw_level_shift(k); return (uint32_t)(((uint64_t)len + ((1ull << sh) - 1)) >> sh); }

// a raw data section: its header as six dwords and a row as three
BW_HD void bw_section_header(uint32_t *dst, uint32_t contig, uint32_t start, uint32_t end, uint32_t count) {
    dst[0] = contig; dst[1] = start; dst[2] = end; dst[3] = 0; dst[4] = 0; dst[5] = 1u | count << 16;
}
BW_HD uint32_t bw_float_bits(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }
BW_HD void bw_item(uint32_t *dst, uint32_t start, uint32_t end, float v) { dst[0] = start; dst[1] = end; dst[2] = bw_float_bits(v); }

// ---- zlib framing: Adler-32.  Lane l adds the bytes i = l, l + 64, ... and their weights n - i; the sums are integers, so no order changes them
BW_HD void bw_adler_lane(const uint8_t *in, uint32_t n, uint32_t lane, uint64_t &a, uint64_t &b) {
    a = 0; b = 0;
    for(uint32_t i = lane; i < n; i += 64) { const uint32_t d = in[i]; a += d; b += (uint64_t)d * (n - i); }
}
BW_HD uint32_t bw_adler_finish(uint64_t a, uint64_t b, uint32_t n) { return (uint32_t)((b + n) % 65521u) << 16 | (uint32_t)((a + 1) % 65521u); }
// the dword of the slot that holds the zlib header and the raw stream's first two bytes; byte i of the trailer
BW_HD uint32_t bw_zlib_dword(uint32_t first_dw) { return 0x9c78u | (first_dw & 0xffff0000u); }
BW_HD uint8_t bw_adler_byte(uint32_t i, uint32_t adler) { return (uint8_t)(adler >> (8 * (3 - i))); }

// ---- zoom ----
struct bw_bin { uint32_t valid; float mn, mx; double sum, sq; };
BW_HD void bw_bin_clear(bw_bin &b) { b.valid = 0; b.mn = 0.0f; b.mx = 0.0f; b.sum = 0.0; b.sq = 0.0; }
BW_HD void bw_bin_row(bw_bin &b, float v, uint32_t bases) {
    BW_NO_CONTRACT
    const double dv = (double)v, db = (double)bases;
    const double x = dv * db;
    b.sum = b.sum + x;
    const double vv = dv * dv;
    const double y = vv * db;
    b.sq = b.sq + y;
    if(!b.valid || v < b.mn) b.mn = v;
    if(!b.valid || v > b.mx) b.mx = v;
    b.valid += bases;
}
BW_HD void bw_bin_child(bw_bin &b, const bw_bin &c) {
    BW_NO_CONTRACT
    if(!c.valid) return;
    b.sum = b.sum + c.sum;
    b.sq = b.sq + c.sq;
    if(!b.valid || c.mn < b.mn) b.mn = c.mn;
    if(!b.valid || c.mx > b.mx) b.mx = c.mx;
    b.valid += c.valid;
}
// the first of the rows [r0, r1) -- one contig's, ascending and apart -- whose end is past `lo`
BW_HD uint32_t bw_first_row(const int32_t *end, uint32_t r0, uint32_t r1, uint32_t lo) {
    while(r0 < r1) { const uint32_t mid = r0 + ((r1 - r0) >> 1); if((uint32_t)end[mid] > lo) r1 = mid; else r0 = mid + 1; }
    return r0;
}
// level 0: bin `bin` of a contig whose rows are [r0, r1)
BW_HD void bw_zoom0(bw_bin &b, int mode, const int32_t *start, const int32_t *end, const int32_t *m, const int32_t *u, uint32_t r0, uint32_t r1, uint32_t bin, uint32_t len) {
    const uint64_t hi64 = ((uint64_t)bin + 1) << BW_W0_SHIFT;
    const uint32_t lo = bin << BW_W0_SHIFT, hi = hi64 < len ? (uint32_t)hi64 : len;
    bw_bin_clear(b);
    for(uint32_t r = bw_first_row(end, r0, r1, lo); r < r1 && (uint32_t)start[r] < hi; r++) {
        const uint32_t s = (uint32_t)start[r] > lo ? (uint32_t)start[r] : lo, e = (uint32_t)end[r] < hi ? (uint32_t)end[r] : hi;
        bw_bin_row(b, bw_value(mode, m[r], u[r]), e - s);
    }
}
BW_HD void bw_zoom_record(uint32_t *dst, uint32_t contig, uint32_t bin, int k, uint32_t len, const bw_bin &b) {
    const uint32_t sh = bw_level_shift(k);
    const uint64_t hi = ((uint64_t)bin + 1) << sh;
    dst[0] = contig; dst[1] = bin << sh; dst[2] = hi < len ? (uint32_t)hi : len; dst[3] = b.valid;
    dst[4] = bw_float_bits(b.mn); dst[5] = bw_float_bits(b.mx); dst[6] = bw_float_bits((float)b.sum); dst[7] = bw_float_bits((float)b.sq);
}
// the contig of entry x of a table made of the contigs' runs: base[c] <= x < base[c + 1] (empty runs are passed over)
BW_HD uint32_t bw_find_contig(const uint32_t *base, uint32_t n_contigs, uint32_t x) {
    uint32_t a = 0, b = n_contigs;
    while(b - a > 1) { const uint32_t mid = a + ((b - a) >> 1); if(base[mid] <= x) a = mid; else b = mid; }
    return a;
}

// ------------------------------------------------------------------------------------------------
// the host's part: which levels are written, the two trees, the file's layout
// ------------------------------------------------------------------------------------------------
struct bw_summary { uint64_t bases; double mn, mx, sum, sq; };
struct bw_entry { uint32_t c0, s0, c1, e1; };               // a section's bounds: first item's contig and start, last item's contig and end
struct bw_piece { int64_t at; std::vector<uint8_t> bytes; };
struct bw_layout {
    int64_t total = 0; std::vector<int64_t> sec_off;         // the sections' offsets: the data sections, then the written levels' in ascending order
    std::vector<bw_piece> pieces;                           // everything that is no section
};

static inline void bw_put(std::vector<uint8_t> &b, uint64_t v, int n) { for(int i = 0; i < n; i++) b.push_back((uint8_t)(v >> (8 * i))); }
static inline void bw_put_double(std::vector<uint8_t> &b, double d) { uint64_t v; memcpy(&v, &d, 8); bw_put(b, v, 8); }

static inline void bw_total_add(bw_summary &t, const bw_bin &b) {
    BW_NO_CONTRACT
    if(!b.valid) return;
    if(!t.bases || (double)b.mn < t.mn) t.mn = (double)b.mn;
    if(!t.bases || (double)b.mx > t.mx) t.mx = (double)b.mx;
    t.sum = t.sum + b.sum;
    t.sq = t.sq + b.sq;
    t.bases += b.valid;
}
// written[k] for the levels' record counts
static inline int bw_plan_levels(int64_t n_rows, const int64_t *count, bool *written) {
    int64_t last = n_rows; int n = 0;
    for(int k = 0; k < BW_LEVELS; k++) { written[k] = 2 * count[k] < last; if(written[k]) { last = count[k]; n++; } }
    return n;
}

// the nodes of a tree of n items in blocks of BW_BLOCK: nodes[l] = the number of nodes of level l (0: the leaves); the last level has one
static inline std::vector<uint64_t> bw_tree_levels(uint64_t n) {
    std::vector<uint64_t> nodes;
    uint64_t k = (n + BW_BLOCK - 1) / BW_BLOCK;
    nodes.push_back(k ? k : 1);
    while(nodes.back() > 1) nodes.push_back((nodes.back() + BW_BLOCK - 1) / BW_BLOCK);
    return nodes;
}

static inline std::vector<uint8_t> bw_chrom_tree(const std::vector<std::string> &names, const std::vector<uint32_t> &len, int64_t at) {
    const uint32_t n = (uint32_t)names.size();
    uint32_t key = 1;
    for(const std::string &s : names) key = std::max<uint32_t>(key, (uint32_t)s.size());
    std::vector<std::string> padded(n);
    for(uint32_t i = 0; i < n; i++) { padded[i] = names[i]; padded[i].resize(key, '\0'); }
    std::vector<uint32_t> order(n);
    for(uint32_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return memcmp(padded[a].data(), padded[b].data(), key) < 0; });
    std::vector<uint8_t> out;
    bw_put(out, BW_CHROM_MAGIC, 4); bw_put(out, BW_BLOCK, 4); bw_put(out, key, 4); bw_put(out, 8, 4); bw_put(out, n, 8); bw_put(out, 0, 8);
    const std::vector<uint64_t> nodes = bw_tree_levels(n);
    const int L = (int)nodes.size();
    const uint64_t isz = key + 8;
    // a node of level l spans BW_BLOCK^(l + 1) items; every node but a level's last is full
    std::vector<uint64_t> span(L), level_at(L);
    for(int l = 0; l < L; l++) span[l] = l ? span[l - 1] * BW_BLOCK : BW_BLOCK;
    auto children = [&](int l, uint64_t j) -> uint64_t { const uint64_t below = l ? nodes[l - 1] : n, first = j * BW_BLOCK; return first >= below ? 0 : std::min<uint64_t>(BW_BLOCK, below - first); };
    uint64_t o = (uint64_t)at + 32;
    for(int l = L - 1; l >= 0; l--) { level_at[l] = o; for(uint64_t j = 0; j < nodes[l]; j++) o += 4 + isz * children(l, j); }
    auto node_at = [&](int l, uint64_t j) -> uint64_t { return level_at[l] + j * (4 + isz * BW_BLOCK); };      // (the nodes before j are full)
    for(int l = L - 1; l >= 0; l--) for(uint64_t j = 0; j < nodes[l]; j++) {
        const uint64_t cnt = children(l, j);
        bw_put(out, l == 0 ? 1 : 0, 1); bw_put(out, 0, 1); bw_put(out, cnt, 2);
        for(uint64_t c = 0; c < cnt; c++) {
            const uint64_t child = j * BW_BLOCK + c;
            const uint32_t item = order[(size_t)(l ? child * span[l - 1] : child)];
            out.insert(out.end(), padded[item].begin(), padded[item].end());
            if(l == 0) { bw_put(out, item, 4); bw_put(out, len[item], 4); }
            else bw_put(out, node_at(l - 1, child), 8);
        }
    }
    return out;
}

static inline bool bw_bound_less(uint32_t c0, uint32_t p0, uint32_t c1, uint32_t p1) { return c0 < c1 || (c0 == c1 && p0 < p1); }
// the R-tree over sections e[0, n) with offsets off[] and sizes size[], written at `at`; `data_end`: where the indexed data ends
static inline std::vector<uint8_t> bw_rtree(const bw_entry *e, const int64_t *off, const uint32_t *size, uint64_t n, int64_t at, int64_t data_end, uint32_t per_slot) {
    std::vector<uint8_t> out;
    const std::vector<uint64_t> nodes = bw_tree_levels(n);
    const int L = (int)nodes.size();
    // the bounds of every node, level by level
    std::vector<std::vector<bw_entry>> bound(L);
    auto children = [&](int l, uint64_t j) -> uint64_t { const uint64_t below = l ? nodes[l - 1] : n, first = j * BW_BLOCK; return first >= below ? 0 : std::min<uint64_t>(BW_BLOCK, below - first); };
    for(int l = 0; l < L; l++) {
        bound[l].resize((size_t)nodes[l]);
        for(uint64_t j = 0; j < nodes[l]; j++) {
            bw_entry b = {0, 0, 0, 0};
            const uint64_t cnt = children(l, j);
            for(uint64_t c = 0; c < cnt; c++) {
                const bw_entry &x = l ? bound[l - 1][(size_t)(j * BW_BLOCK + c)] : e[j * BW_BLOCK + c];
                if(c == 0) b = x;
                else {
                    if(bw_bound_less(x.c0, x.s0, b.c0, b.s0)) { b.c0 = x.c0; b.s0 = x.s0; }
                    if(bw_bound_less(b.c1, b.e1, x.c1, x.e1)) { b.c1 = x.c1; b.e1 = x.e1; }
                }
            }
            bound[l][(size_t)j] = b;
        }
    }
    const bw_entry all = bound[L - 1][0];
    bw_put(out, BW_RTREE_MAGIC, 4); bw_put(out, BW_BLOCK, 4); bw_put(out, n, 8);
    bw_put(out, all.c0, 4); bw_put(out, all.s0, 4); bw_put(out, all.c1, 4); bw_put(out, all.e1, 4);
    bw_put(out, (uint64_t)data_end, 8); bw_put(out, per_slot, 4); bw_put(out, 0, 4);
    std::vector<uint64_t> level_at(L);
    uint64_t o = (uint64_t)at + 48;
    for(int l = L - 1; l >= 0; l--) { level_at[l] = o; for(uint64_t j = 0; j < nodes[l]; j++) o += 4 + (l ? 24 : 32) * children(l, j); }
    auto node_at = [&](int l, uint64_t j) -> uint64_t { return level_at[l] + j * (4 + (uint64_t)(l ? 24 : 32) * BW_BLOCK); };
    for(int l = L - 1; l >= 0; l--) for(uint64_t j = 0; j < nodes[l]; j++) {
        const uint64_t cnt = children(l, j);
        bw_put(out, l == 0 ? 1 : 0, 1); bw_put(out, 0, 1); bw_put(out, cnt, 2);
        for(uint64_t c = 0; c < cnt; c++) {
            const uint64_t child = j * BW_BLOCK + c;
            const bw_entry &x = l ? bound[l - 1][(size_t)child] : e[child];
            bw_put(out, x.c0, 4); bw_put(out, x.s0, 4); bw_put(out, x.c1, 4); bw_put(out, x.e1, 4);
            if(l == 0) { bw_put(out, (uint64_t)off[child], 8); bw_put(out, size[child], 8); }
            else bw_put(out, node_at(l - 1, child), 8);
        }
    }
    return out;
}

// The layout.  Sections come as one list: the n_data data sections, then the sections of the written levels in ascending order of the level
// (zsec[k] of them, of zcount[k] records); entry[], size[] (compressed bytes) and raw_max (the largest raw section) describe them.
static inline bw_layout bw_make_layout(const std::vector<std::string> &names, const std::vector<uint32_t> &len, uint64_t n_data, const bool *written,
                                       const int64_t *zcount, const uint64_t *zsec, const bw_entry *entry, const uint32_t *size, uint32_t raw_max, const bw_summary &total) {
    bw_layout lay;
    int n_levels = 0; uint64_t n_sec = n_data;
    for(int k = 0; k < BW_LEVELS; k++) if(written[k]) { n_levels++; n_sec += zsec[k]; }
    lay.sec_off.resize((size_t)n_sec);
    const int64_t summary_at = 64 + 24 * n_levels, chrom_at = summary_at + 40;
    const std::vector<uint8_t> chrom = bw_chrom_tree(names, len, chrom_at);
    const int64_t data_at = chrom_at + (int64_t)chrom.size();
    int64_t o = data_at + 8;
    for(uint64_t s = 0; s < n_data; s++) { lay.sec_off[(size_t)s] = o; o += size[s]; }
    const int64_t index_at = o;
    bw_piece index; index.at = index_at; index.bytes = bw_rtree(entry, lay.sec_off.data(), size, n_data, index_at, index_at, BW_ITEMS);
    o += (int64_t)index.bytes.size();
    std::vector<uint8_t> zh;
    std::vector<bw_piece> zp;
    uint64_t s0 = n_data;
    for(int k = 0; k < BW_LEVELS; k++) if(written[k]) {
        const int64_t zdata_at = o;
        bw_piece cnt; cnt.at = o; bw_put(cnt.bytes, (uint64_t)zcount[k], 4); o += 4;
        for(uint64_t s = s0; s < s0 + zsec[k]; s++) { lay.sec_off[(size_t)s] = o; o += size[s]; }
        bw_piece zi; zi.at = o; zi.bytes = bw_rtree(entry + s0, lay.sec_off.data() + s0, size + s0, zsec[k], o, o, BW_ZITEMS);
        bw_put(zh, 1ull << bw_level_shift(k), 4); bw_put(zh, 0, 4); bw_put(zh, (uint64_t)zdata_at, 8); bw_put(zh, (uint64_t)o, 8);
        o += (int64_t)zi.bytes.size();
        zp.push_back(cnt); zp.push_back(zi);
        s0 += zsec[k];
    }
    bw_piece head; head.at = 0;
    std::vector<uint8_t> &h = head.bytes;
    bw_put(h, BW_MAGIC, 4); bw_put(h, 4, 2); bw_put(h, (uint64_t)n_levels, 2); bw_put(h, (uint64_t)chrom_at, 8); bw_put(h, (uint64_t)data_at, 8); bw_put(h, (uint64_t)index_at, 8);
    bw_put(h, 0, 2); bw_put(h, 0, 2); bw_put(h, 0, 8); bw_put(h, (uint64_t)summary_at, 8); bw_put(h, raw_max, 4); bw_put(h, 0, 8);
    h.insert(h.end(), zh.begin(), zh.end());
    bw_put(h, total.bases, 8); bw_put_double(h, total.mn); bw_put_double(h, total.mx); bw_put_double(h, total.sum); bw_put_double(h, total.sq);
    h.insert(h.end(), chrom.begin(), chrom.end());
    bw_put(h, n_data, 8);
    lay.pieces.push_back(head); lay.pieces.push_back(index);
    for(bw_piece &p : zp) lay.pieces.push_back(p);
    bw_piece tail; tail.at = o; bw_put(tail.bytes, BW_MAGIC, 4); o += 4;
    lay.pieces.push_back(tail);
    lay.total = o;
    return lay;
}

// A byte range of the file.  The data sections are contiguous in the file, and so are the sections of every written level: with the sections'
// bytes packed one behind the other in a store, in the list's order, the file is the pieces plus 1 + levels regions of that store.
struct bw_region { int64_t at, bytes, store; };              // bytes [at, at + bytes) of the file are bytes [store, store + bytes) of the store
struct bw_cut { int piece; size_t index; int64_t src, dst, bytes; };       // piece 1: from pieces[index].bytes, 0: from the store; src: the offset there, dst: in the range
static inline std::vector<bw_region> bw_make_regions(const bw_layout &lay, uint64_t n_data, const bool *written, const uint64_t *zsec, const uint32_t *size) {
    std::vector<bw_region> out;
    int64_t store = 0; uint64_t s0 = 0;
    for(int k = -1; k < BW_LEVELS; k++) {
        if(k >= 0 && !written[k]) continue;
        const uint64_t cnt = k < 0 ? n_data : zsec[k];
        int64_t bytes = 0;
        for(uint64_t s = s0; s < s0 + cnt; s++) bytes += size[s];
        if(cnt) out.push_back(bw_region{lay.sec_off[(size_t)s0], bytes, store});
        store += bytes; s0 += cnt;
    }
    return out;
}
// what makes up bytes [offset, offset + bytes) of the file, in no particular order; the cuts' bytes add up to the range's where it lies inside the file
static inline std::vector<bw_cut> bw_cut_range(const bw_layout &lay, const std::vector<bw_region> &regions, int64_t offset, int64_t bytes) {
    std::vector<bw_cut> out;
    const int64_t lo = offset, hi = offset + bytes;
    auto cut = [&](int piece, size_t index, int64_t at, int64_t len, int64_t src0) {
        const int64_t a = std::max(lo, at), b = std::min(hi, at + len);
        if(a < b) out.push_back(bw_cut{piece, index, src0 + (a - at), a - lo, b - a});
    };
    for(size_t i = 0; i < lay.pieces.size(); i++) cut(1, i, lay.pieces[i].at, (int64_t)lay.pieces[i].bytes.size(), 0);
    for(size_t i = 0; i < regions.size(); i++) cut(0, i, regions[i].at, regions[i].bytes, regions[i].store);
    return out;
}
#endif
