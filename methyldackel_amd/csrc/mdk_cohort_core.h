// mdk_cohort_core.h -- a Cohort (the united table: n sites, S samples, the counts [S, n]) as text and back: the two formats Cohort.write
// makes and the one Cohort.read takes (csrc/mdk_cohort.hip; tools/cohort_emu.cpp runs the kernels' blocking over this header on the host;
// tests/cohort_rule.py restates it with str.join / str.split).  Digits are mdk_text_core.h's, line starts and numbers mdk_parse_core.h's.
//
// COH_FMT_COHORT round-trips exactly.  Two '#' lines made on the host, then one line per site, `0 0` cells included:
//     #methyldackel_amd cohort 1 \t samples=S \t merged=0|1 \t contexts=<comma list of 0,1,2> \t n_union=N \n
//     #chrom \t start \t end \t context \t strand \t nsamples \t NAME0.nmeth \t NAME0.nunmeth \t ... \n
//     chrom \t start \t end \t CG|CHG|CHH \t +|-|. \t nsamples \t m0 \t u0 \t ... \t m(S-1) \t u(S-1) \n
// start and end are the columns as they are (0-based, half open: BED); the strand character is '.' for strand 0; start, end, nsamples are
// written as txt_put_i32 writes them, the counts as txt_put_u32 does.
// COH_FMT_METHYLBASE is write-only: the columns of methylKit's getData(methylBase) as write.table(sep = "\t", quote = FALSE, row.names =
// FALSE) lays them out, under the header line  chr start end strand coverage1 numCs1 numTs1 ... :
//     chr \t start+1 \t start+1 \t +|- \t cov0 \t m0 \t u0 \t ... \n          '+' for strand >= 0, '-' below; cov = m + u in uint32
//
// A LINE IN PIECES.  A line is its PREFIX (the fields before the first count, no tab behind them), then one CELL per sample -- a tab, then
// the sample's numbers separated by tabs --, then '\n'.  The kernels cut a line into the prefix and one stretch per block of `sample_block`
// samples; the newline belongs to the last block's stretch.  The longest line of a legal "cohort" table is 288 + 22 * 1024 + 1 = 22,817 bytes, the longest of any
// table the writer takes 295 + 33 * 1024 + 1: the offset of a block inside its line fits 16 bits.
//
// WRITE REFUSALS, the first site's first: a negative contig or start, a contig index outside the names, end <= start, a context above 2,
// then a negative count, the first sample's.  coh_write_key orders them in one 64-bit word for an atomicMin.
//
// READ.  Every line behind the two '#' lines is a row.  A line is refused with exactly ONE code, the smallest RANK that applies:
//     long (more than COHORT_MAX_LINE bytes with its '\n'), a '#' line, empty, too few fields, too many, an empty field,
//     then the fields from left to right -- unknown contig; per number a non-digit, then an overflow; a bad context token; a bad strand --,
//     then end <= start, then nsamples > S; a row that does not ascend strictly behind its predecessor comes last.
// A number is looked at over its first 11 bytes only: a non-digit among them is `digit`; otherwise more than 10 bytes, or a value above
// INT32_MAX, is `overflow`.  So a field's owner reads a bounded stretch, whatever the line holds.  A contig name is at most 255 bytes.
// Plain C++ for device and host; no function keeps an array.
#ifndef MDK_COHORT_CORE_H
#define MDK_COHORT_CORE_H
#include <stdint.h>
#include "mdk_text_core.h"
#include "mdk_parse_core.h"

#if defined(__HIPCC__)
#define MDK_COH __host__ __device__ __forceinline__
#else
#define MDK_COH static inline
#endif

enum { COH_FMT_COHORT = 0, COH_FMT_METHYLBASE = 1, COH_N_FORMATS = 2 };
#define COHORT_MAX_LINE 32768          // bytes of a line a reader takes, its '\n' included
#define COH_MAX_SAMPLES 1024
#define COH_SITE_FIELDS 6              // fields before the first count of a "cohort" line
#define COH_LANE 16                    // bytes of a line a lane looks at: one aligned quad
#define COH_NUMBER_LOOK 11             // bytes of a number its owner reads

// ---- write ----
MDK_COH uint32_t coh_prefix_len(int fmt, uint32_t name_len, int32_t start, int32_t end, uint32_t ctx, int32_t nsamples) {
    if(fmt == COH_FMT_METHYLBASE) return name_len + 1 + 2 * (uint32_t)txt_digits_i32(start + 1) + 1 + 2;
    return name_len + 1 + txt_digits_i32(start) + 1 + txt_digits_i32(end) + 1 + (ctx == 0 ? 2u : 3u) + 3 + txt_digits_i32(nsamples);
}
MDK_COH char *coh_put_prefix(char *q, int fmt, const uint8_t *name, uint32_t name_len, int32_t start, int32_t end, uint32_t ctx, int32_t strand, int32_t nsamples) {
    q = txt_put_name(q, name, name_len); *q++ = '\t';
    if(fmt == COH_FMT_METHYLBASE) {
        q = txt_put_i32(q, start + 1); *q++ = '\t'; q = txt_put_i32(q, start + 1); *q++ = '\t'; *q++ = strand >= 0 ? '+' : '-';
        return q;
    }
    q = txt_put_i32(q, start); *q++ = '\t'; q = txt_put_i32(q, end); *q++ = '\t';
    *q++ = 'C'; if(ctx != 0) *q++ = 'H'; *q++ = ctx == 2 ? 'H' : 'G'; *q++ = '\t';
    *q++ = strand > 0 ? '+' : strand < 0 ? '-' : '.'; *q++ = '\t';
    return txt_put_i32(q, nsamples);
}
MDK_COH uint32_t coh_cell_len(int fmt, uint32_t m, uint32_t u) {
    return (fmt == COH_FMT_METHYLBASE ? 1u + txt_digits_u32(m + u) : 0u) + 1 + txt_digits_u32(m) + 1 + txt_digits_u32(u);
}
MDK_COH char *coh_put_cell(char *q, int fmt, uint32_t m, uint32_t u) {
    if(fmt == COH_FMT_METHYLBASE) { *q++ = '\t'; q = txt_put_u32(q, m + u); }
    *q++ = '\t'; q = txt_put_u32(q, m); *q++ = '\t';
    return txt_put_u32(q, u);
}
#define COH_CELL_MAX 33                // a methylBase cell of three 10-digit numbers
#define COH_PREFIX_MAX (255 + 40)      // a 255-byte name, a "cohort" line's five other fields (an nsamples of 11 characters) and their tabs

enum { COH_W_POSITION = 1, COH_W_CONTIG = 2, COH_W_END = 3, COH_W_CONTEXT = 4, COH_W_NEGATIVE = 5 };
MDK_COH uint32_t coh_site_check(int32_t contig, int32_t start, int32_t end, uint32_t ctx, int32_t n_contigs) {
    return contig < 0 || start < 0 ? COH_W_POSITION : contig >= n_contigs ? COH_W_CONTIG : end <= start ? COH_W_END : ctx > 2 ? COH_W_CONTEXT : 0;
}
// (site, refusal, sample) in one word that orders them: the smallest is the one reported
MDK_COH uint64_t coh_write_key(int64_t site, uint32_t what, int32_t sample) { return (uint64_t)site << 16 | (uint64_t)what << 11 | (uint32_t)sample; }
MDK_COH const char *coh_write_error_text(uint32_t what) {
    return what == COH_W_POSITION ? "a contig or a start is negative" : what == COH_W_CONTIG ? "a contig index lies outside the contig names" :
           what == COH_W_END ? "end is not above start" : what == COH_W_CONTEXT ? "a context is above 2" : "a count is negative";
}

// ---- read ----
// which of the four bytes of w equal c: bit k for byte k (prs_newlines4's arithmetic for any byte)
MDK_COH uint32_t coh_bytes4(uint32_t w, uint32_t c) {
    const uint32_t x = w ^ (c * 0x01010101u);
    const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
    return (((z >> 7) * 0x00204081u) >> 21) & 0xfu;
}
MDK_COH uint32_t coh_tabs(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    return coh_bytes4(w0, 9) | coh_bytes4(w1, 9) << 4 | coh_bytes4(w2, 9) << 8 | coh_bytes4(w3, 9) << 12;
}
// the bytes of a stretch that starts at text position p which lie inside [lo, hi): bit k for byte k
MDK_COH uint32_t coh_inside(int64_t p, int64_t lo, int64_t hi) {
    const int64_t a = lo > p ? lo - p : 0, b = hi - p < COH_LANE ? hi - p : COH_LANE;
    return b <= a ? 0u : (((1u << (int)b) - 1u) & ~((1u << (int)a) - 1u));
}

// the line starts among the 16 bytes w0..w3 at text position p, of the lines of text[begin .. bytes): bit k for byte k.  prev_nl: byte p - 1
// is a newline (asked only where p > begin); the byte at `begin` starts a line whatever stands before it
MDK_COH uint32_t coh_line_starts(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, bool prev_nl, int64_t p, int64_t begin, int64_t bytes) {
    uint32_t s = prs_starts(prs_newlines(w0, w1, w2, w3), prev_nl, p, bytes) & coh_inside(p, begin, bytes);
    if(begin >= p && begin < p + COH_LANE && begin < bytes) s |= 1u << (int)(begin - p);
    return s;
}

// the codes of a refused line, in the order in which a status word ranks them
enum { COH_E_LONG = 1, COH_E_HASH, COH_E_EMPTY, COH_E_FEW, COH_E_MANY, COH_E_FIELD, COH_E_CONTIG, COH_E_DIGIT, COH_E_OVERFLOW, COH_E_CONTEXT,
       COH_E_STRAND, COH_E_END, COH_E_NSAMPLES, COH_E_ORDER, COH_N_ERRORS };
// ranks inside a line: structural ones are their codes; a field's are 16 + 2 f + (0: first, 1: second reason); the two relations follow
#define COH_RANK_FIELD0 16u
#define COH_RANK_END 0xfffff0u
#define COH_RANK_NSAMPLES 0xfffff1u
#define COH_RANK_NONE 0xffffffffu
MDK_COH uint32_t coh_field_rank(uint32_t f, uint32_t second) { return COH_RANK_FIELD0 + 2u * f + second; }
MDK_COH uint32_t coh_rank_code(uint32_t rank) {
    if(rank < COH_RANK_FIELD0) return rank;
    if(rank == COH_RANK_END) return COH_E_END;
    if(rank == COH_RANK_NSAMPLES) return COH_E_NSAMPLES;
    const uint32_t f = (rank - COH_RANK_FIELD0) >> 1, second = (rank - COH_RANK_FIELD0) & 1u;
    return f == 0 ? COH_E_CONTIG : f == 3 ? COH_E_CONTEXT : f == 4 ? COH_E_STRAND : second ? COH_E_OVERFLOW : COH_E_DIGIT;
}
MDK_COH const char *coh_error_name(uint32_t code) {
    const char *const names[COH_N_ERRORS] = { "none", "long", "hash", "empty", "few", "many", "field", "contig", "digit", "overflow", "context", "strand", "end", "nsamples", "order" };
    return code < COH_N_ERRORS ? names[code] : "none";
}
MDK_COH const char *coh_error_text(uint32_t code) {
    return code == COH_E_LONG ? "a line is longer than 32768 bytes" :
           code == COH_E_HASH ? "a # line behind the two header lines (concatenated files are not read)" :
           code == COH_E_EMPTY ? "an empty line" :
           code == COH_E_FEW ? "a line has too few fields" :
           code == COH_E_MANY ? "a line has too many fields" :
           code == COH_E_FIELD ? "a line has an empty field (fields are separated by single tabs)" :
           code == COH_E_CONTIG ? "a line's contig is not among the contig names" :
           code == COH_E_DIGIT ? "a number holds something else than decimal digits" :
           code == COH_E_OVERFLOW ? "a number is larger than INT32_MAX" :
           code == COH_E_CONTEXT ? "a context is none of CG, CHG, CHH" :
           code == COH_E_STRAND ? "a strand is none of +, - and ." :
           code == COH_E_END ? "end is not above start" :
           code == COH_E_NSAMPLES ? "nsamples is above the number of samples" : "a row is not strictly ascending in (contig, start) behind its predecessor";
}

// the line [ls, le) of the text without its '\n' and one '\r' before it: its end.  `bytes`: the text's
MDK_COH int64_t coh_line_end(const uint8_t *text, int64_t ls, int64_t le) {
    if(le > ls && text[le - 1] == '\n') le--;
    if(le > ls && text[le - 1] == '\r') le--;
    return le;
}
// the number that starts at fs and ends before the next tab or at le: 0 and v, or 1 (digit) / 2 (overflow)
MDK_COH uint32_t coh_number(const uint8_t *text, int64_t fs, int64_t le, int32_t &v) {
    uint64_t x = 0; int k = 0;
    for(; k < COH_NUMBER_LOOK && fs + k < le && text[fs + k] != '\t'; k++) {
        const uint8_t c = text[fs + k];
        if(c < '0' || c > '9') return 1;
        x = x * 10u + (uint32_t)(c - '0');
    }
    if(k > 10 || x > (uint64_t)INT32_MAX) return 2;
    v = (int32_t)x;
    return 0;
}
// field f of a line that ends at le, its first byte at fs (a field's owner knows no more): the rank that refuses it (COH_RANK_NONE: none) and
// its value -- the contig's index, a number, the context, the strand
MDK_COH uint32_t coh_field(const uint8_t *text, int64_t fs, int64_t le, uint32_t f, const prs_tab &T, int32_t &v) {
    if(fs >= le || text[fs] == '\t') return COH_E_FIELD;
    if(f == 0) {
        uint32_t k = 0;
        while(k <= MD_TEXT_NAME_MAX && fs + k < le && text[fs + k] != '\t') k++;
        v = k > MD_TEXT_NAME_MAX ? -1 : prs_find(T, text + fs, k);
        return v < 0 ? coh_field_rank(0, 0) : COH_RANK_NONE;
    }
    if(f == 3) {
        const int64_t left = le - fs;
        const bool two = left >= 2 && (left == 2 || text[fs + 2] == '\t'), three = left >= 3 && (left == 3 || text[fs + 3] == '\t');
        if(two && text[fs] == 'C' && text[fs + 1] == 'G') { v = 0; return COH_RANK_NONE; }
        if(three && text[fs] == 'C' && text[fs + 1] == 'H' && (text[fs + 2] == 'G' || text[fs + 2] == 'H')) { v = text[fs + 2] == 'G' ? 1 : 2; return COH_RANK_NONE; }
        return coh_field_rank(3, 0);
    }
    if(f == 4) {
        const uint8_t c = text[fs];
        if((fs + 1 < le && text[fs + 1] != '\t') || (c != '+' && c != '-' && c != '.')) return coh_field_rank(4, 0);
        v = c == '+' ? 1 : c == '-' ? -1 : 0;
        return COH_RANK_NONE;
    }
    const uint32_t e = coh_number(text, fs, le, v);
    return e ? coh_field_rank(f, e - 1) : COH_RANK_NONE;
}
// what the whole line says before any field is looked at: [ls, le) the line without its end, `with_end` its bytes with it
MDK_COH uint32_t coh_line_rank(const uint8_t *text, int64_t ls, int64_t le, int64_t with_end) {
    return with_end > COHORT_MAX_LINE ? COH_E_LONG : le > ls && text[ls] == '#' ? COH_E_HASH : le == ls ? COH_E_EMPTY : COH_RANK_NONE;
}
MDK_COH uint32_t coh_count_rank(uint32_t tabs, int32_t S) {
    const uint32_t want = COH_SITE_FIELDS + 2u * (uint32_t)S;
    return tabs + 1 < want ? COH_E_FEW : tabs + 1 > want ? COH_E_MANY : COH_RANK_NONE;
}
MDK_COH uint32_t coh_row_rank(int32_t start, int32_t end, int32_t nsamples, int32_t S) {
    return end <= start ? COH_RANK_END : nsamples > S ? COH_RANK_NSAMPLES : COH_RANK_NONE;
}
MDK_COH bool coh_ascends(int32_t c0, int32_t x0, int32_t c1, int32_t x1) { return c1 > c0 || (c1 == c0 && x1 > x0); }
#endif
