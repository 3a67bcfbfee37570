// mdk_text_core.h -- the text of `extract`'s output lines, made without printf: what csrc/host/mdk_emit.c put_site writes for a row, byte for
// byte, from integer arithmetic alone.
//
// Six formats (the layouts of put_site, and of perRead's addRead as csrc/host/mdk_cmd_perread.c writes it):
//   MD_TEXT_BEDGRAPH         chrom \t start \t end \t (int)(100.0 * m / cov) \t m \t u \n
//   MD_TEXT_FRACTION         chrom \t start \t end \t %f of m / cov \n
//   MD_TEXT_COUNTS           chrom \t start \t end \t cov \n
//   MD_TEXT_METHYLKIT        chrom . start+1 \t chrom \t start+1 \t F|R \t cov \t %6.2f of 100 m / cov \t %6.2f of 100 u / cov \n
//   MD_TEXT_CYTOSINE_REPORT  chrom \t pos \t +|- \t m \t u \t C G|HG|HH \t trinucleotide \n
//   MD_TEXT_PERREAD          name \t chrom \t pos \t %f of 100 m / cov, or the characters 0.0 when cov == 0 \t cov \n   (txt_read_*: a row is a read)
// with cov = m + u in uint32, as the host adds them.  --logit is not here: its value is log(f) - log(1 - f), and neither glibc's log nor the
// device library's is correctly rounded, so the same bytes cannot be promised.
//
// %f and %6.2f: glibc prints the EXACT binary value of the double, rounded half-to-even at the last printed digit.  The same in integers
// (txt_scaled): the double is mantissa * 2^-s; mantissa * 10^decimals is a 128-bit product in two 64-bit words; the product shifted right by
// s is the printed number's digits, and the bits shifted out decide the rounding -- above half up, exactly half to even.  The double itself is
// formed as the host forms it, ((double)m) / cov and 100.0 * ((double)m) / cov from left to right, with IEEE division (no fast-math, no
// reciprocal): the 100.0 * m is exact (m < 2^32), the division is the one rounding.
//
// Plain C++ without wave intrinsics, as mdk_inflate_core.h: it compiles for the device (mdk_text.hip) and for the host (tools/text_emu.cpp
// compares every function here with snprintf and renders whole files), which is how it is tested without a GPU.  No function keeps an array:
// digits are written backwards from their known end, so the device code needs no scratch memory.
#ifndef MDK_TEXT_CORE_H
#define MDK_TEXT_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MDK_TXT __host__ __device__ __forceinline__
#else
#define MDK_TXT static inline
#endif

#ifndef MD_TEXT_FORMATS               // (include/mdk_hip.h declares the same)
#define MD_TEXT_FORMATS
enum { MD_TEXT_BEDGRAPH = 0, MD_TEXT_FRACTION, MD_TEXT_COUNTS, MD_TEXT_METHYLKIT, MD_TEXT_CYTOSINE_REPORT, MD_TEXT_PERREAD, MD_TEXT_N_FORMATS };
#endif
#define MD_TEXT_NAME_MAX 255           // bytes of a contig name a renderer takes, and of a read name

// ---- integers: what printf's %u / %i write (put_u32 / put_i32 of mdk_emit.c) ----
MDK_TXT int txt_digits_u64(uint64_t v) { int n = 1; while(v >= 10) { v /= 10; n++; } return n; }
MDK_TXT int txt_digits_u32(uint32_t v) {
    return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
MDK_TXT int txt_digits_i32(int32_t v) { return v < 0 ? 1 + txt_digits_u32((uint32_t)(-(int64_t)v)) : txt_digits_u32((uint32_t)v); }
// the digits of v at q; returns their end
MDK_TXT char *txt_put_u32(char *q, uint32_t v) {
    char *const end = q + txt_digits_u32(v); char *p = end;
    do { *--p = (char)('0' + v % 10u); v /= 10u; } while(v);
    return end;
}
MDK_TXT char *txt_put_i32(char *q, int32_t v) {
    if(v < 0) { *q++ = '-'; return txt_put_u32(q, (uint32_t)(-(int64_t)v)); }
    return txt_put_u32(q, (uint32_t)v);
}
MDK_TXT char *txt_put_u64(char *q, uint64_t v) {
    char *const end = q + txt_digits_u64(v); char *p = end;
    do { *--p = (char)('0' + (int)(v % 10u)); v /= 10u; } while(v);
    return end;
}

// ---- the values, formed as the host forms them ----
MDK_TXT double txt_fraction(uint32_t m, uint32_t cov) { return ((double)m) / cov; }
MDK_TXT double txt_percent(uint32_t m, uint32_t cov) { return 100.0 * ((double)m) / cov; }
MDK_TXT int32_t txt_percent_int(uint32_t m, uint32_t cov) { return (int32_t)txt_percent(m, cov); }      // column 4 of the default bedGraph

// ---- x * mul, rounded half-to-even to an integer, exactly: 0 <= x < 2^52 finite, mul <= 10^6 (the result is below 2^63 for x < 2^43) ----
MDK_TXT uint64_t txt_scaled(double x, uint32_t mul) {
    uint64_t bits; __builtin_memcpy(&bits, &x, 8);
    const uint32_t ex = (uint32_t)(bits >> 52) & 0x7ffu;
    const uint64_t frac = bits & ((1ull << 52) - 1), mant = ex ? frac | (1ull << 52) : frac;
    const int s = 1075 - (int)(ex ? ex : 1u);                       // x = mant * 2^-s, s >= 1 for x < 2^52
    // the 128-bit product (phi, plo) = mant * mul, from 32-bit halves (mant < 2^53, mul < 2^20: neither partial product overflows)
    const uint64_t lo = (mant & 0xffffffffull) * mul, hi = (mant >> 32) * mul;
    const uint64_t plo = lo + (hi << 32), phi = (hi >> 32) + (plo < lo ? 1u : 0u);
    uint64_t q, rhi, rlo, hhi, hlo;                                  // quotient, remainder and half of the divisor 2^s
    if(s >= 128) return 0;                                           // the product is below 2^73: far under half
    if(s > 64) { const int t = s - 64; q = phi >> t; rhi = phi & ((1ull << t) - 1); rlo = plo; hhi = 1ull << (t - 1); hlo = 0; }
    else if(s == 64) { q = phi; rhi = 0; rlo = plo; hhi = 0; hlo = 1ull << 63; }
    else { q = (phi << (64 - s)) | (plo >> s); rhi = 0; rlo = plo & ((1ull << s) - 1); hhi = 0; hlo = 1ull << (s - 1); }
    const bool above = rhi > hhi || (rhi == hhi && rlo > hlo), half = rhi == hhi && rlo == hlo;
    return q + ((above || (half && (q & 1))) ? 1u : 0u);
}
// %f (dec = 6, width 0) and %6.2f (dec = 2, width 6) of x: the length, and the characters
MDK_TXT uint32_t txt_pow10(int dec) { return dec == 6 ? 1000000u : 100u; }
MDK_TXT int txt_fixed_len(double x, int dec, int width) {
    const int n = txt_digits_u64(txt_scaled(x, txt_pow10(dec)) / txt_pow10(dec)) + 1 + dec;
    return n < width ? width : n;
}
MDK_TXT char *txt_put_fixed(char *q, double x, int dec, int width) {
    const uint32_t p10 = txt_pow10(dec);
    const uint64_t v = txt_scaled(x, p10), ip = v / p10; uint32_t fp = (uint32_t)(v % p10);
    for(int pad = width - (txt_digits_u64(ip) + 1 + dec); pad > 0; pad--) *q++ = ' ';
    q = txt_put_u64(q, ip); *q++ = '.';
    char *const end = q + dec;
    for(char *p = end; p > q; ) { *--p = (char)('0' + fp % 10u); fp /= 10u; }
    return end;
}

// ---- lines ----
// one row: a, b = start, end of a call (bedGraph columns 2 and 3), or a = the 1-based position of a report row; strand > 0 a C, < 0 a G,
// 0 a --mergeContext row; context 0 CpG, 1 CHG, 2 CHH; tri: the three letters of the report's last column (report rows only)
struct txt_row { int32_t a, b; uint32_t m, u; int32_t strand; uint32_t context; const uint8_t *tri; };

// has the row a line in this format?  The call formats print no row without coverage (put_site's depth test with -d >= 1), the report every row
MDK_TXT bool txt_row_printed(int fmt, const txt_row &r) { return fmt == MD_TEXT_CYTOSINE_REPORT || r.m + r.u != 0u; }

// the length of the row's line, its newline included, for a contig name of name_len bytes
MDK_TXT uint32_t txt_line_len(int fmt, uint32_t name_len, const txt_row &r) {
    const uint32_t cov = r.m + r.u;
    switch(fmt) {
    case MD_TEXT_FRACTION: return name_len + 1 + txt_digits_i32(r.a) + 1 + txt_digits_i32(r.b) + 1 + txt_fixed_len(txt_fraction(r.m, cov), 6, 0) + 1;
    case MD_TEXT_COUNTS: return name_len + 1 + txt_digits_i32(r.a) + 1 + txt_digits_i32(r.b) + 1 + txt_digits_i32((int32_t)cov) + 1;
    case MD_TEXT_METHYLKIT: {
        const int p = txt_digits_i32(r.a + 1);
        return 2 * name_len + 2 * p + 7 + txt_digits_i32((int32_t)cov) + txt_fixed_len(txt_percent(r.m, cov), 2, 6) + 1 + txt_fixed_len(txt_percent(r.u, cov), 2, 6) + 1;
    }
    case MD_TEXT_CYTOSINE_REPORT:
        return name_len + 1 + txt_digits_i32(r.a) + 3 + txt_digits_u32(r.m) + 1 + txt_digits_u32(r.u) + 2 + (r.context == 0 ? 1 : 2) + 1 + 3 + 1;
    default:
        return name_len + 1 + txt_digits_i32(r.a) + 1 + txt_digits_i32(r.b) + 1 + txt_digits_i32(txt_percent_int(r.m, cov)) + 1 + txt_digits_u32(r.m) + 1 + txt_digits_u32(r.u) + 1;
    }
}

MDK_TXT char *txt_put_name(char *q, const uint8_t *name, uint32_t name_len) { for(uint32_t i = 0; i < name_len; i++) q[i] = (char)name[i]; return q + name_len; }

// the row's line at q (txt_line_len bytes); returns its end
MDK_TXT char *txt_put_line(char *q, int fmt, const uint8_t *name, uint32_t name_len, const txt_row &r) {
    const uint32_t cov = r.m + r.u;
    q = txt_put_name(q, name, name_len);
    if(fmt == MD_TEXT_METHYLKIT) {
        *q++ = '.'; q = txt_put_i32(q, r.a + 1); *q++ = '\t';
        q = txt_put_name(q, name, name_len); *q++ = '\t';
        q = txt_put_i32(q, r.a + 1); *q++ = '\t'; *q++ = r.strand > 0 ? 'F' : 'R'; *q++ = '\t';
        q = txt_put_i32(q, (int32_t)cov); *q++ = '\t';
        q = txt_put_fixed(q, txt_percent(r.m, cov), 2, 6); *q++ = '\t';
        q = txt_put_fixed(q, txt_percent(r.u, cov), 2, 6);
    } else if(fmt == MD_TEXT_CYTOSINE_REPORT) {
        *q++ = '\t'; q = txt_put_i32(q, r.a); *q++ = '\t'; *q++ = r.strand > 0 ? '+' : '-'; *q++ = '\t';
        q = txt_put_u32(q, r.m); *q++ = '\t'; q = txt_put_u32(q, r.u); *q++ = '\t';
        *q++ = 'C'; if(r.context != 0) *q++ = 'H'; *q++ = r.context == 2 ? 'H' : 'G'; *q++ = '\t';
        *q++ = (char)r.tri[0]; *q++ = (char)r.tri[1]; *q++ = (char)r.tri[2];
    } else {
        *q++ = '\t'; q = txt_put_i32(q, r.a); *q++ = '\t'; q = txt_put_i32(q, r.b); *q++ = '\t';
        if(fmt == MD_TEXT_FRACTION) q = txt_put_fixed(q, txt_fraction(r.m, cov), 6, 0);
        else if(fmt == MD_TEXT_COUNTS) q = txt_put_i32(q, (int32_t)cov);
        else { q = txt_put_i32(q, txt_percent_int(r.m, cov)); *q++ = '\t'; q = txt_put_u32(q, r.m); *q++ = '\t'; q = txt_put_u32(q, r.u); }
    }
    *q++ = '\n';
    return q;
}
// ---- a perRead line: every row has one, covered or not (addRead prints the read whatever it counted) ----
// what follows the read name: \t chrom \t pos \t V \t cov \n with cov = m + u in uint32, V = %f of 100. * ((double)m) / cov, or 0.0 without coverage
MDK_TXT uint32_t txt_read_tail_len(uint32_t contig_len, int32_t pos, uint32_t m, uint32_t u) {
    const uint32_t cov = m + u;
    return 1 + contig_len + 1 + txt_digits_i32(pos) + 1 + (cov ? (uint32_t)txt_fixed_len(txt_percent(m, cov), 6, 0) : 3u) + 1 + txt_digits_u32(cov) + 1;
}
MDK_TXT uint32_t txt_read_line_len(uint32_t name_len, uint32_t contig_len, int32_t pos, uint32_t m, uint32_t u) { return name_len + txt_read_tail_len(contig_len, pos, m, u); }
MDK_TXT char *txt_put_read_tail(char *q, const uint8_t *contig, uint32_t contig_len, int32_t pos, uint32_t m, uint32_t u) {
    const uint32_t cov = m + u;
    *q++ = '\t'; q = txt_put_name(q, contig, contig_len); *q++ = '\t'; q = txt_put_i32(q, pos); *q++ = '\t';
    if(cov) q = txt_put_fixed(q, txt_percent(m, cov), 6, 0); else { *q++ = '0'; *q++ = '.'; *q++ = '0'; }
    *q++ = '\t'; q = txt_put_u32(q, cov); *q++ = '\n';
    return q;
}
// the whole line at q (txt_read_line_len bytes), the name a byte at a time; returns its end
MDK_TXT char *txt_put_read_line(char *q, const uint8_t *name, uint32_t name_len, const uint8_t *contig, uint32_t contig_len, int32_t pos, uint32_t m, uint32_t u) {
    return txt_put_read_tail(txt_put_name(q, name, name_len), contig, contig_len, pos, m, u);
}
// n bytes from buf[s ..) to dst, four at a time (k_rtext_fill: a read name from the staged span in LDS into the image): whole 4-byte
// ALIGNED words of dst, each made of the two aligned words of buf that hold its bytes; the bytes before the first and after the last whole
// word singly.  buf is 4-byte aligned and readable up to the aligned word after the one holding byte s + n - 1 (its value is not used).
MDK_TXT uint32_t txt_word(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4); return v; }
MDK_TXT void txt_copy_words(uint8_t *dst, const uint8_t *buf, uint32_t s, uint32_t n) {
    uint32_t i = 0;
    while(i < n && ((uintptr_t)(dst + i) & 3u)) { dst[i] = buf[s + i]; i++; }
    if(i + 4 <= n) {
        const uint32_t sh = 8u * ((s + i) & 3u);
        const uint8_t *w = buf + ((s + i) & ~3u);
        uint32_t lo = txt_word(w);
        for(; i + 4 <= n; i += 4) {
            w += 4;
            const uint32_t hi = txt_word(w), v = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;       // (little endian: byte k of a word is bits 8k..8k+7)
            __builtin_memcpy(__builtin_assume_aligned(dst + i, 4), &v, 4);
            lo = hi;
        }
    }
    for(; i < n; i++) dst[i] = buf[s + i];
}

// ---- a workgroup's lines, assembled in an image and streamed out as aligned 16-byte quads (k_text_fill; tools/text_emu --emulate) ----
// The image holds the workgroup's `total` bytes from offset sh = (destination address) mod 16 on, so image quad k is the ALIGNED destination
// quad k counted from (destination - sh).  Quads [quad0, quad1) lie wholly inside the workgroup's text and go out whole; image bytes
// [sh, head_end) before them and [tail0, end) after them share their quads with the neighbouring workgroups' text and go out as bytes.
struct txt_image_plan { uint32_t sh, end, quad0, quad1, head_end, tail0; };
MDK_TXT txt_image_plan txt_plan_image(uint64_t dst_address, uint32_t total) {
    txt_image_plan p;
    p.sh = (uint32_t)(dst_address & 15u); p.end = p.sh + total;
    p.quad0 = p.sh ? 1u : 0u; p.quad1 = p.end >> 4;
    p.head_end = p.sh ? (p.end < 16u ? p.end : 16u) : 0u;
    p.tail0 = (p.end & ~15u) > p.head_end ? (p.end & ~15u) : p.head_end;
    return p;
}
#endif
