// mdk_parse_core.h -- the way back from text to columns: the lines of a per-cytosine bedGraph or of a cytosine_report.txt read into the column
// layouts the rest of the library takes (csrc/mdk_parse.hip: Calls.read, Cytosines.read).  The inverse of mdk_text_core.h.
//
// LINES.  A line starts at byte 0 of the text and after every '\n'; it ends before the next '\n' or at the end of the text (a last line
// without '\n' is a line; a text that ends in '\n' has no line behind it).  One '\r' directly before the '\n' is dropped.  A line whose first
// five bytes are `track` is no row, wherever it stands -- the command skips it too, and concatenated files carry several.  EVERY other line is
// a row, malformed or not: the number of rows follows from the line starts alone (prs_newlines, prs_is_track), and what is wrong with a line
// is found when it is parsed (prs_line).  A line with its '\n' is at most PARSE_MAX_LINE = 512 bytes: a 255-byte name, five 10-digit numbers,
// tabs and CRLF fit.
//
// MD_PARSE_BEDGRAPH: exactly six fields separated by single tabs, chrom start end pct nmeth nunmeth.  chrom is looked up in the name table
// through an index sorted by name (prs_find: a binary search, the first of equal names); start, end, nmeth, nunmeth are 1 to 10 decimal digits
// and nothing else, at most INT32_MAX; pct is any non-empty run of bytes and is ignored, as the command ignores it.  end must be start + 1
// (only per-cytosine files are read; a merged file is refused by name), start must lie inside the contig, and the reference base at start
// decides the strand: +1 for C / c, -1 for G / g, anything else is refused (the command aborts there).  The context is site_of's five-base
// window of csrc/host/mdk_mergecontext.c -- letter for letter k_classify's rule (csrc/mdk_hip.hip), 'N' and the contig's ends included --, so
// a row read back carries exactly the context and strand a session would have given it.
// MD_PARSE_CYTOSINE_REPORT: seven fields, chrom pos +|- nmeth nunmeth CG|CHG|CHH tri.  pos stays 1-based and must be at least 1; tri is
// exactly three bytes of ACGTN.  No reference is needed.
//
// This is deliberately STRICTER than the command: its strtoll takes signs and leading blanks and stops at the first non-digit, its strtok
// swallows doubled tabs and tolerates trailing columns, and a number past INT32_MAX wraps.  All of these are refused here (PRS_E_*).  The
// promise is one-way: every file the parser accepts gives, after merge_context, what the command prints for it.
//
// A line is refused with exactly ONE bit: the first that applies in the order too long, empty, too few / too many fields, an empty field,
// then the fields from left to right (unknown contig; a non-digit, then an overflow, per number; a position below 1, a bad strand / context /
// trinucleotide token in a report), then for a bedGraph end != start + 1, no resident reference, start outside the contig, a base that is
// neither C nor G.  tests/parse_rule.py restates this with str.split.
//
// Plain C++ as mdk_text_core.h and mdk_merge_core.h: it compiles for the device (mdk_parse.hip) and for the host (tools/parse_emu.cpp runs
// the kernels' blocking over it), which is how it is tested without a GPU.  No function keeps an array.
#ifndef MDK_PARSE_CORE_H
#define MDK_PARSE_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MDK_PRS __host__ __device__ __forceinline__
#else
#define MDK_PRS static inline
#endif

#ifndef MD_PARSE_FORMATS              // (include/mdk_hip.h declares the same)
#define MD_PARSE_FORMATS
enum { MD_PARSE_BEDGRAPH = 0, MD_PARSE_CYTOSINE_REPORT = 1 };
#endif
#define PARSE_MAX_LINE 512             // bytes of a line, its '\n' included
#define PARSE_SPAN 4096                // bytes of the text a workgroup owns: 16 per lane
#define PARSE_LANE 16

enum { PRS_E_EMPTY = 1, PRS_E_FEW = 2, PRS_E_MANY = 4, PRS_E_FIELD = 8, PRS_E_DIGIT = 16, PRS_E_OVERFLOW = 32, PRS_E_CONTIG = 64, PRS_E_MERGED = 128,
       PRS_E_RANGE = 256, PRS_E_BASE = 512, PRS_E_STRAND = 1024, PRS_E_CONTEXT = 2048, PRS_E_TRI = 4096, PRS_E_LONG = 8192, PRS_E_NOREF = 16384,
       PRS_E_CHANGED = 32768 };
#define PRS_N_ERRORS 16

// what a line is looked up in: name c = names[name_off[c] .. name_off[c + 1]), `sorted` the contig indices in ascending (name, index) order;
// ref[c] / ref_len[c] the resident bases of contig c (ref_len[c] < 0: none; ref == nullptr: none of any contig)
struct prs_tab { const uint32_t *name_off; const uint8_t *names; const uint32_t *sorted; int32_t n_contigs; const uint8_t *const *ref; const int64_t *ref_len; };
// a row of either layout: a = start (calls) or pos (report), b = end (calls only), tri (report only)
struct prs_row { int32_t contig, a, b, m, u, ctx, strand; uint8_t tri[3]; };

// ---- line starts ----
// which of the four bytes of w are '\n': bit k for byte k (little endian: byte k is bits 8k .. 8k + 7).  Exact: x has a zero byte where w has
// a newline; (x & 0x7f..) + 0x7f.. carries into bit 7 of every byte with a low bit set, | x covers bit 7 itself, and no carry crosses a byte
MDK_PRS uint32_t prs_newlines4(uint32_t w) {
    const uint32_t x = w ^ 0x0a0a0a0au;
    const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);       // 0x80 in every byte that is zero
    return (((z >> 7) * 0x00204081u) >> 21) & 0xfu;                                  // bits 0, 8, 16, 24 gathered into 0..3 (no two products meet)
}
// the same for a lane's 16 bytes: bit k for byte k
MDK_PRS uint32_t prs_newlines(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    return prs_newlines4(w0) | prs_newlines4(w1) << 4 | prs_newlines4(w2) << 8 | prs_newlines4(w3) << 12;
}
// the line starts among a lane's 16 bytes, the first of them byte `at` of a text of `bytes` bytes: a byte inside the text whose predecessor is
// a newline (prev_nl: the byte before the lane's first is one, or the lane's first byte is byte 0)
MDK_PRS uint32_t prs_starts(uint32_t newlines, bool prev_nl, int64_t at, int64_t bytes) {
    const int64_t left = bytes - at;
    const uint32_t inside = left >= PARSE_LANE ? 0xffffu : left > 0 ? (1u << (int)left) - 1u : 0u;
    return ((newlines << 1) | (prev_nl ? 1u : 0u)) & inside;
}
// is the line at p, with `avail` bytes of the text from p on, a `track` line?
MDK_PRS bool prs_is_track(const uint8_t *p, int64_t avail) { return avail >= 5 && p[0] == 't' && p[1] == 'r' && p[2] == 'a' && p[3] == 'c' && p[4] == 'k'; }

// ---- fields ----
// the contig named p[0 .. n): its index, or -1.  lower bound over `sorted` by (bytes, then length); equal names: the smallest index
MDK_PRS int prs_name_cmp(const uint8_t *p, uint32_t n, const uint8_t *q, uint32_t m) {
    const uint32_t k = n < m ? n : m;
    for(uint32_t i = 0; i < k; i++) if(p[i] != q[i]) return p[i] < q[i] ? -1 : 1;
    return n < m ? -1 : n > m ? 1 : 0;
}
MDK_PRS int32_t prs_find(const prs_tab &T, const uint8_t *p, uint32_t n) {
    int32_t lo = 0, hi = T.n_contigs;
    while(lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t c = T.sorted[mid], o = T.name_off[c];
        if(prs_name_cmp(T.names + o, T.name_off[c + 1] - o, p, n) < 0) lo = mid + 1; else hi = mid;
    }
    if(lo >= T.n_contigs) return -1;
    const uint32_t c = T.sorted[lo], o = T.name_off[c];
    return prs_name_cmp(T.names + o, T.name_off[c + 1] - o, p, n) == 0 ? (int32_t)c : -1;
}
// p[f0 .. f1), not empty, as a number: 0 and v, or PRS_E_DIGIT / PRS_E_OVERFLOW
MDK_PRS uint32_t prs_number(const uint8_t *p, uint32_t f0, uint32_t f1, int32_t &v) {
    uint64_t x = 0;
    for(uint32_t i = f0; i < f1; i++) if(p[i] < '0' || p[i] > '9') return PRS_E_DIGIT;
    if(f1 - f0 > 10) return PRS_E_OVERFLOW;
    for(uint32_t i = f0; i < f1; i++) x = x * 10u + (uint32_t)(p[i] - '0');
    if(x > (uint64_t)INT32_MAX) return PRS_E_OVERFLOW;
    v = (int32_t)x;
    return 0;
}
// the end of the field that starts at c of a line of L bytes
MDK_PRS uint32_t prs_field_end(const uint8_t *p, uint32_t c, uint32_t L) { while(c < L && p[c] != '\t') c++; return c; }

// the base of contig bases[0 .. n) at q folded to upper case, 0 outside the contig ((x & 0x5f) maps no other FASTA letter onto C or G)
MDK_PRS uint8_t prs_base(const uint8_t *bases, int64_t n, int64_t q) { return q >= 0 && q < n ? (uint8_t)(bases[q] & 0x5f) : (uint8_t)0; }

// ---- a line ----
// the line at p, with `avail` bytes of the text from p on of which the caller holds min(avail, PARSE_MAX_LINE + 1): 0 and `out`, or the one
// PRS_E_* bit that refuses it
MDK_PRS uint32_t prs_line(const uint8_t *p, int64_t avail, int fmt, const prs_tab &T, prs_row &out) {
    const uint32_t lim = avail < PARSE_MAX_LINE ? (uint32_t)avail : (uint32_t)PARSE_MAX_LINE;
    uint32_t L = 0;
    while(L < lim && p[L] != '\n') L++;
    if(L == lim && avail > PARSE_MAX_LINE) return PRS_E_LONG;          // no newline among the first 512 bytes, and the text goes on
    if(L && p[L - 1] == '\r') L--;
    if(!L) return PRS_E_EMPTY;
    {
        uint32_t tabs = 0; bool gap = true, hole = false;
        for(uint32_t i = 0; i < L; i++) { const bool t = p[i] == '\t'; if(t) { tabs++; hole |= gap; } gap = t; }
        hole |= gap;
        const uint32_t want = fmt == MD_PARSE_CYTOSINE_REPORT ? 7u : 6u;
        if(tabs + 1 < want) return PRS_E_FEW;
        if(tabs + 1 > want) return PRS_E_MANY;
        if(hole) return PRS_E_FIELD;
    }
    uint32_t f0 = 0, f1 = prs_field_end(p, 0, L), e;
    const int32_t contig = prs_find(T, p, f1);
    if(contig < 0) return PRS_E_CONTIG;
    int32_t a = 0, b = 0, m = 0, u = 0, ctx, strand;
    f0 = f1 + 1; f1 = prs_field_end(p, f0, L);
    if((e = prs_number(p, f0, f1, a)) != 0) return e;
    if(fmt == MD_PARSE_CYTOSINE_REPORT) {
        if(a < 1) return PRS_E_RANGE;
        f0 = f1 + 1; f1 = prs_field_end(p, f0, L);
        if(f1 - f0 != 1 || (p[f0] != '+' && p[f0] != '-')) return PRS_E_STRAND;
        strand = p[f0] == '+' ? 1 : -1;
        f0 = f1 + 1; f1 = prs_field_end(p, f0, L);
        if((e = prs_number(p, f0, f1, m)) != 0) return e;
        f0 = f1 + 1; f1 = prs_field_end(p, f0, L);
        if((e = prs_number(p, f0, f1, u)) != 0) return e;
        f0 = f1 + 1; f1 = prs_field_end(p, f0, L);
        if(f1 - f0 == 2 && p[f0] == 'C' && p[f0 + 1] == 'G') ctx = 0;
        else if(f1 - f0 == 3 && p[f0] == 'C' && p[f0 + 1] == 'H' && (p[f0 + 2] == 'G' || p[f0 + 2] == 'H')) ctx = p[f0 + 2] == 'G' ? 1 : 2;
        else return PRS_E_CONTEXT;
        f0 = f1 + 1; f1 = prs_field_end(p, f0, L);
        if(f1 - f0 != 3) return PRS_E_TRI;
        for(uint32_t i = 0; i < 3; i++) { const uint8_t c = p[f0 + i]; if(c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != 'N') return PRS_E_TRI; }
        out.tri[0] = p[f0]; out.tri[1] = p[f0 + 1]; out.tri[2] = p[f0 + 2];
    } else {
        f0 = f1 + 1; f1 = prs_field_end(p, f0, L);
        if((e = prs_number(p, f0, f1, b)) != 0) return e;
        f0 = f1 + 1; f1 = prs_field_end(p, f0, L);                      // the percentage: not empty, not looked at
        f0 = f1 + 1; f1 = prs_field_end(p, f0, L);
        if((e = prs_number(p, f0, f1, m)) != 0) return e;
        f0 = f1 + 1; f1 = prs_field_end(p, f0, L);
        if((e = prs_number(p, f0, f1, u)) != 0) return e;
        if((int64_t)b != (int64_t)a + 1) return PRS_E_MERGED;
        const int64_t n = T.ref ? T.ref_len[contig] : -1;
        if(n < 0) return PRS_E_NOREF;
        if((int64_t)a >= n) return PRS_E_RANGE;
        const uint8_t *const s = T.ref[contig];
        const uint8_t c0 = prs_base(s, n, a);
        if(c0 == 'C') { strand = 1; ctx = prs_base(s, n, (int64_t)a + 1) == 'G' ? 0 : prs_base(s, n, (int64_t)a + 2) == 'G' ? 1 : 2; }
        else if(c0 == 'G') { strand = -1; ctx = prs_base(s, n, (int64_t)a - 1) == 'C' ? 0 : prs_base(s, n, (int64_t)a - 2) == 'C' ? 1 : 2; }
        else return PRS_E_BASE;
        out.tri[0] = out.tri[1] = out.tri[2] = 0;
    }
    out.contig = contig; out.a = a; out.b = b; out.m = m; out.u = u; out.ctx = ctx; out.strand = strand;
    return 0;
}

// the refusal a status word names first, as the library's message says it and as tools/parse_emu prints it
MDK_PRS const char *prs_error_name(uint32_t e) {
    return e & PRS_E_CHANGED ? "changed" : e & PRS_E_LONG ? "long" : e & PRS_E_EMPTY ? "empty" : e & PRS_E_FEW ? "few" : e & PRS_E_MANY ? "many" : e & PRS_E_FIELD ? "field" :
           e & PRS_E_CONTIG ? "contig" : e & PRS_E_DIGIT ? "digit" : e & PRS_E_OVERFLOW ? "overflow" : e & PRS_E_MERGED ? "merged" : e & PRS_E_NOREF ? "noref" :
           e & PRS_E_RANGE ? "range" : e & PRS_E_BASE ? "base" : e & PRS_E_STRAND ? "strand" : e & PRS_E_CONTEXT ? "context" : "tri";
}
MDK_PRS const char *prs_error_text(uint32_t e) {
    return e & PRS_E_CHANGED ? "the text is not the one that was measured" :
           e & PRS_E_LONG ? "a line is longer than 512 bytes" :
           e & PRS_E_EMPTY ? "an empty line" :
           e & PRS_E_FEW ? "a line has too few fields" :
           e & PRS_E_MANY ? "a line has too many fields" :
           e & PRS_E_FIELD ? "a line has an empty field (fields are separated by single tabs)" :
           e & PRS_E_CONTIG ? "a line's contig is not among the contig names" :
           e & PRS_E_DIGIT ? "a number holds something else than decimal digits" :
           e & PRS_E_OVERFLOW ? "a number is larger than INT32_MAX" :
           e & PRS_E_MERGED ? "end is not start + 1: only per-cytosine files are read, and this one looks merged already" :
           e & PRS_E_NOREF ? "a bedGraph line's contig has no resident reference (md_text_reference)" :
           e & PRS_E_RANGE ? "a position lies outside the contig" :
           e & PRS_E_BASE ? "the reference base at a line's start is neither C nor G" :
           e & PRS_E_STRAND ? "a strand is neither + nor -" :
           e & PRS_E_CONTEXT ? "a context is none of CG, CHG, CHH" : "a trinucleotide is not three letters of ACGTN";
}
#endif
