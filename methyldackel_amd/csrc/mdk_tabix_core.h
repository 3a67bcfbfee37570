// mdk_tabix_core.h -- the .tbi of a BGZF table, byte by byte: the tabix index of the SAM/tabix specification (binning with min_shift 14 and
// 5 levels, reg2bin, linear windows of 16384 bases, BGZF-wrapped) with every choice the specification leaves open fixed, so that the bytes
// are a function of the data file alone.  csrc/mdk_tabix.hip (libmdk_index.so) runs the per-line half on the device; tools/tabix_emu.cpp is
// this header's host build, line after line; tests/tabix_rule.py restates it in numpy.
//
// CONFIGURATION.  format, col_seq, col_beg, col_end, meta, skip, as the header of a .tbi holds them (columns are 1-based).  Presets: "bed"
// (0x10000, 1, 2, 3, '#', skip) for the bedGraph, fraction and counts files; "methylKit" (0, 2, 3, 3, '#', 1); "cytosine_report"
// (0, 1, 2, 2, '#', 0).
//
// LINES.  The decompressed text is cut at '\n' (a last line without one is a line; nothing is done about '\r').  The first `skip` lines give no
// entry and are not judged.  Every other line is judged in this order: an empty line is refused (TBX_E_EMPTY); a line of more than 511 bytes
// before its '\n' is refused (TBX_E_LONG: the parser's limit, PARSE_MAX_LINE with the '\n'); a line whose first byte is `meta` gives no
// entry; every other line is an entry.  An entry's fields are separated by single tabs; coordinates are 1 to 10 decimal digits and nothing else.
//
// INTERVALS, 0-based and half-open.  With the UCSC flag (0x10000) beg0 = v(col_beg), end0 = v(col_end); without it and col_end == col_beg
// [v - 1, v); without it and two columns [v(col_beg) - 1, v(col_end)).
//
// REFUSALS.  An entry is refused with the first that applies of: fewer fields than the largest column index (TBX_E_FEW); an empty
// coordinate, a non-digit in one, more than 10 digits (TBX_E_COORD); beg0 < 0 or end0 <= beg0 (TBX_E_RANGE); end0 > 2^29 (TBX_E_BIG: a .tbi
// ends at 512 Mb, and CSI is not written); a name that is empty or longer than 255 bytes (TBX_E_NAME).  Then, against the entry before it:
// the same name and a smaller beg0 (TBX_E_ORDER); and a name that returns after another name has followed it (TBX_E_RETURN).  A refusal
// names the 1-based line; of several the earliest line wins, and the codes are numbered so that of two on one line the smaller is the one
// this order gives.
//
// NAMES are the names that have an entry, in order of first appearance; tid is that order.
//
// VIRTUAL OFFSETS.  Member j has compressed file offset c_j, decompressed start u_j and size isize_j.  A decompressed offset u becomes
// (c_j << 16) | (u - u_j) for the member that HOLDS byte u (members with isize 0 hold none; so a position at the exact end of a member is
// offset 0 of the next member that holds a byte).  u == the text's length: where the member after the last one that holds a byte starts
// (the EOF member, if the file has one; the file's length if nothing follows), with 0 in the low bits.  The map is monotone, which is why
// everything before the end works in decompressed offsets.
//
// BINS AND CHUNKS.  An entry's bin is reg2bin(beg0, end0).  Per tid, in file order, each maximal run of consecutive entries with one bin is
// one chunk: from the first byte of the run's first line to one past the newline of its last line.  Skipped `meta` lines neither break nor
// join a run.  No chunks are merged and no bin is lifted into its parent.  Bins ascend by number; a bin's chunks stand in file order.
// Every tid also has pseudo-bin 37450 with two chunks: (begin of its first line, end of its last), then (the number of its entries, 0).
//
// LINEAR INDEX.  For every window w in beg0 >> 14 .. (end0 - 1) >> 14, ioff[w] is the smallest begin of an entry that touches it;
// n_intv = 1 + the largest w; an unset ioff[w] takes the value of the next set one above it.
//
// FILE.  "TBI\1", n_ref, the six configuration fields, l_nm, the names (each zero-terminated), then per tid n_bin, the bins (bin, n_chunk,
// the chunks), n_intv and ioff, then n_no_coor = 0 as a uint64; little-endian; that payload as BGZF by mdk_deflate_core.h's rule (members
// of 65280 bytes plus the EOF member).  A data file without entries gives n_ref = 0.
//
// RECORDS.  What the per-line half leaves for the rest: one tbx_rec for every entry that starts a run (another name or another bin than
// the entry before it, or no entry before it), that begins a name, or whose bin lies above the leaves (bin < 4681: it touches more than
// one window, so the run's begin does not say what it does to ioff).  tbx_builder, host only, makes the payload of them.
#ifndef MDK_TABIX_CORE_H
#define MDK_TABIX_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MDK_TBX __host__ __device__ __forceinline__
#else
#define MDK_TBX static inline
#endif

#define TBX_MAX_LINE 512               // bytes of a line, its '\n' included
#define TBX_SPAN 4096                  // bytes of the text a workgroup owns: 16 per lane
#define TBX_LANE 16
#define TBX_UCSC 0x10000
#define TBX_MAX_END (1 << 29)
#define TBX_LEAF0 4681                 // the first bin of the lowest level: ((1 << 15) - 1) / 7
#define TBX_PSEUDO_BIN 37450
#define TBX_NAME_SLOT 256              // bytes a name-change record's name takes

enum { TBX_E_FEW = 1, TBX_E_COORD = 2, TBX_E_RANGE = 3, TBX_E_BIG = 4, TBX_E_NAME = 5, TBX_E_LONG = 6, TBX_E_EMPTY = 7, TBX_E_ORDER = 8, TBX_E_RETURN = 9 };
enum { TBX_F_RUN = 1, TBX_F_NAME = 2, TBX_F_WIDE = 4 };
enum { TBX_NONE = -1 };                // tbx_line: the line gives no entry

struct tbx_conf { int32_t format, col_seq, col_beg, col_end, meta, skip; };
// an entry: its name is the line's bytes [name_off, name_off + name_len)
struct tbx_entry { uint32_t name_off, name_len; int32_t beg0, end0; uint32_t bin, line_len; };
// a record: `begin` the decompressed offset of the entry's line, `prev_end` the end (one past the newline) of the line of the entry before it
// (0: none), `ord` the number of entries before it in the piece
struct tbx_rec { uint64_t begin, prev_end; uint32_t bin; int32_t beg0, end0; uint32_t flags, ord, name_len; };

MDK_TBX uint32_t tbx_reg2bin(int32_t beg, int32_t end) {
    --end;
    if(beg >> 14 == end >> 14) return ((1u << 15) - 1u) / 7u + (uint32_t)(beg >> 14);
    if(beg >> 17 == end >> 17) return ((1u << 12) - 1u) / 7u + (uint32_t)(beg >> 17);
    if(beg >> 20 == end >> 20) return ((1u << 9) - 1u) / 7u + (uint32_t)(beg >> 20);
    if(beg >> 23 == end >> 23) return ((1u << 6) - 1u) / 7u + (uint32_t)(beg >> 23);
    if(beg >> 26 == end >> 26) return ((1u << 3) - 1u) / 7u + (uint32_t)(beg >> 26);
    return 0;
}

// p[f0 .. f1) as a coordinate: true and v, or false
MDK_TBX bool tbx_number(const uint8_t *p, uint32_t f0, uint32_t f1, int64_t &v) {
    if(f1 == f0 || f1 - f0 > 10) return false;
    int64_t x = 0;
    for(uint32_t i = f0; i < f1; i++) { if(p[i] < '0' || p[i] > '9') return false; x = x * 10 + (int64_t)(p[i] - '0'); }
    v = x;
    return true;
}

// the line at p, with `avail` bytes of the text from p on, of which at most TBX_MAX_LINE are read; `skipped`: it is one of the first `skip`
// lines.  TBX_NONE (no entry), 0 and `e`, or the TBX_E_* that refuses it
MDK_TBX int tbx_line(const uint8_t *p, int64_t avail, bool skipped, const tbx_conf &cf, tbx_entry &e) {
    if(skipped) return TBX_NONE;
    const uint32_t lim = avail < TBX_MAX_LINE ? (uint32_t)avail : (uint32_t)TBX_MAX_LINE;
    uint32_t L = 0;
    while(L < lim && p[L] != '\n') L++;
    if(L == 0) return TBX_E_EMPTY;
    if(L == TBX_MAX_LINE) return TBX_E_LONG;
    if(p[0] == (uint8_t)cf.meta) return TBX_NONE;
    const int32_t last = cf.col_seq > cf.col_beg ? (cf.col_seq > cf.col_end ? cf.col_seq : cf.col_end) : (cf.col_beg > cf.col_end ? cf.col_beg : cf.col_end);
    uint32_t s0 = 0, s1 = 0, b0 = 0, b1 = 0, e0 = 0, e1 = 0;
    int32_t col = 1; uint32_t f0 = 0;
    for(uint32_t i = 0; i <= L && col <= last; i++) {
        if(i < L && p[i] != '\t') continue;
        if(col == cf.col_seq) { s0 = f0; s1 = i; }
        if(col == cf.col_beg) { b0 = f0; b1 = i; }
        if(col == cf.col_end) { e0 = f0; e1 = i; }
        col++; f0 = i + 1;
    }
    if(col <= last) return TBX_E_FEW;
    int64_t vb = 0, ve = 0;
    if(!tbx_number(p, b0, b1, vb) || !tbx_number(p, e0, e1, ve)) return TBX_E_COORD;
    const int64_t beg0 = cf.format & TBX_UCSC ? vb : vb - 1, end0 = ve;
    if(beg0 < 0 || end0 <= beg0) return TBX_E_RANGE;
    if(end0 > (int64_t)TBX_MAX_END) return TBX_E_BIG;
    if(s1 == s0 || s1 - s0 > 255) return TBX_E_NAME;
    e.name_off = s0; e.name_len = s1 - s0; e.beg0 = (int32_t)beg0; e.end0 = (int32_t)end0; e.bin = tbx_reg2bin(e.beg0, e.end0); e.line_len = L;
    return 0;
}

MDK_TBX bool tbx_same_name(const uint8_t *p, const tbx_entry &a, const uint8_t *q, const tbx_entry &b) {
    if(a.name_len != b.name_len) return false;
    for(uint32_t i = 0; i < a.name_len; i++) if(p[a.name_off + i] != q[b.name_off + i]) return false;
    return true;
}

// an entry against the entry before it (have_prev: there is one): the record flags it gets (0: no record), and whether it is out of order
MDK_TBX uint32_t tbx_flags(bool have_prev, const uint8_t *pp, const tbx_entry &pe, const uint8_t *p, const tbx_entry &e, bool &unordered) {
    unordered = false;
    uint32_t f = e.bin < TBX_LEAF0 ? (uint32_t)TBX_F_WIDE : 0u;
    if(!have_prev || !tbx_same_name(pp, pe, p, e)) return f | TBX_F_RUN | TBX_F_NAME;
    unordered = e.beg0 < pe.beg0;
    return pe.bin != e.bin ? f | TBX_F_RUN : f;
}

MDK_TBX const char *tbx_error_text(int code) {
    return code == TBX_E_FEW ? "a line has fewer fields than the index's columns" :
           code == TBX_E_COORD ? "a coordinate is empty, holds something else than decimal digits or has more than 10 of them" :
           code == TBX_E_RANGE ? "an interval begins before the contig's first base or ends at or before its begin" :
           code == TBX_E_BIG ? "an interval ends past 2^29: a .tbi ends at 512 Mb, and CSI is not written" :
           code == TBX_E_NAME ? "a sequence name is empty or longer than 255 bytes" :
           code == TBX_E_LONG ? "a line is longer than 512 bytes" :
           code == TBX_E_EMPTY ? "an empty line" :
           code == TBX_E_ORDER ? "not sorted: a begin is smaller than that of the line before it on the same contig" :
           code == TBX_E_RETURN ? "not sorted: a contig appears in two places" : "the text is not the one that was measured";
}

#if defined(__cplusplus) && !defined(MDK_TABIX_NO_BUILDER)
// ---- the rest, host only: records in file order -> the payload ----
#include <algorithm>
#include <map>
#include <string>
#include <vector>

struct tbx_member { uint64_t c, u; uint32_t isize; };      // a member that holds bytes: file offset, decompressed start, size
struct tbx_chunk { uint32_t bin; uint64_t beg, end; };
struct tbx_ref { std::string name; std::vector<tbx_chunk> chunks; std::vector<uint64_t> ioff; uint64_t first, last, entries; };

struct tbx_builder {
    tbx_conf cf;
    std::vector<tbx_ref> refs;
    std::map<std::string, uint32_t> seen;
    bool open = false; uint64_t open_ord = 0;
    int64_t returned = -1;                                 // the begin of the first entry whose name returned, if any
    std::string returned_name;

    void window(tbx_ref &r, uint32_t w, uint64_t begin) {
        if(r.ioff.size() <= w) r.ioff.resize((size_t)w + 1, ~0ull);
        if(begin < r.ioff[w]) r.ioff[w] = begin;
    }
    void close_run(uint64_t end, uint64_t ord) {
        if(!open) return;
        tbx_ref &r = refs.back();
        r.chunks.back().end = end; r.last = end; r.entries += ord - open_ord;
        open = false;
    }
    // a record, `ord` its entry's number in the file, `name` its name's bytes if it begins one
    void add(const tbx_rec &x, uint64_t ord, const uint8_t *name) {
        if(x.flags & TBX_F_RUN) close_run(x.prev_end, ord);
        if(x.flags & TBX_F_NAME) {
            const std::string nm((const char *)name, x.name_len);
            if(seen.count(nm)) { if(returned < 0) { returned = (int64_t)x.begin; returned_name = nm; } }
            else seen[nm] = (uint32_t)refs.size();
            refs.push_back(tbx_ref{nm, {}, {}, x.begin, x.begin, 0});
        }
        if(refs.empty()) return;
        tbx_ref &r = refs.back();
        if(x.flags & TBX_F_RUN) { r.chunks.push_back(tbx_chunk{x.bin, x.begin, x.begin}); open = true; open_ord = ord; }
        if(x.flags & TBX_F_WIDE) for(uint32_t w = (uint32_t)(x.beg0 >> 14); w <= (uint32_t)((x.end0 - 1) >> 14); w++) window(r, w, x.begin);
        else if(x.flags & TBX_F_RUN) window(r, x.bin - TBX_LEAF0, x.begin);
    }
    // the end of the last entry's line, and the number of entries in the file
    void finish(uint64_t last_end, uint64_t entries) { close_run(last_end, entries); }

    static uint64_t voffset(const std::vector<tbx_member> &m, uint64_t c_end, uint64_t u) {
        size_t lo = 0, hi = m.size();                     // the last member with u_j <= u
        while(lo < hi) { const size_t mid = (lo + hi) / 2; if(m[mid].u <= u) lo = mid + 1; else hi = mid; }
        if(lo == 0) return c_end << 16;
        const tbx_member &x = m[lo - 1];
        if(u - x.u >= x.isize) return c_end << 16;        // (only u == the text's length gets here)
        return x.c << 16 | (u - x.u);
    }
    static void put32(std::vector<uint8_t> &o, uint32_t v) { for(int i = 0; i < 4; i++) o.push_back((uint8_t)(v >> (8 * i))); }
    static void put64(std::vector<uint8_t> &o, uint64_t v) { for(int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i))); }

    std::vector<uint8_t> payload(const std::vector<tbx_member> &m, uint64_t c_end) {
        std::vector<uint8_t> o;
        o.push_back('T'); o.push_back('B'); o.push_back('I'); o.push_back(1);
        put32(o, (uint32_t)refs.size());
        put32(o, (uint32_t)cf.format); put32(o, (uint32_t)cf.col_seq); put32(o, (uint32_t)cf.col_beg); put32(o, (uint32_t)cf.col_end); put32(o, (uint32_t)cf.meta); put32(o, (uint32_t)cf.skip);
        uint32_t l_nm = 0;
        for(const tbx_ref &r : refs) l_nm += (uint32_t)r.name.size() + 1;
        put32(o, l_nm);
        for(const tbx_ref &r : refs) { o.insert(o.end(), r.name.begin(), r.name.end()); o.push_back(0); }
        for(tbx_ref &r : refs) {
            std::stable_sort(r.chunks.begin(), r.chunks.end(), [](const tbx_chunk &a, const tbx_chunk &b) { return a.bin < b.bin; });
            uint32_t n_bin = 1;
            for(size_t i = 0; i < r.chunks.size(); i++) n_bin += i == 0 || r.chunks[i].bin != r.chunks[i - 1].bin;
            put32(o, n_bin);
            for(size_t i = 0; i < r.chunks.size();) {
                size_t j = i;
                while(j < r.chunks.size() && r.chunks[j].bin == r.chunks[i].bin) j++;
                put32(o, r.chunks[i].bin); put32(o, (uint32_t)(j - i));
                for(; i < j; i++) { put64(o, voffset(m, c_end, r.chunks[i].beg)); put64(o, voffset(m, c_end, r.chunks[i].end)); }
            }
            put32(o, TBX_PSEUDO_BIN); put32(o, 2);
            put64(o, voffset(m, c_end, r.first)); put64(o, voffset(m, c_end, r.last)); put64(o, r.entries); put64(o, 0);
            for(size_t w = r.ioff.size(); w-- > 0;) if(r.ioff[w] == ~0ull) r.ioff[w] = r.ioff[w + 1];      // (the last one is set)
            put32(o, (uint32_t)r.ioff.size());
            for(uint64_t v : r.ioff) put64(o, voffset(m, c_end, v));
        }
        put64(o, 0);
        return o;
    }
};
#endif
#endif
