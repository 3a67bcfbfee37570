// text_emu.cpp -- TEST INFRASTRUCTURE: the device text formatter's arithmetic (csrc/mdk_text_core.h, the very functions k_text_len,
// k_text_fill, k_rtext_len and k_rtext_fill of csrc/mdk_text.hip run) executed on the host and compared with glibc's printf.
//   build: g++ -O2 -o tools/_build/text_emu tools/text_emu.cpp -Imethyldackel_amd/csrc
//   text_emu --selfcheck [N]    %f of m/cov, %6.2f of 100 m/cov and 100 u/cov, (int)(100.0 m/cov) and the integer digits against snprintf: every
//                               (m, u) in 0..600 x 0..600, N (default 2 * 10^7) seeded pseudo-random pairs with counts up to 2^31, the int32
//                               extremes; and for every case txt_line_len against what txt_put_line wrote.  Prints {"cases": .., "mismatches": ..};
//                               exit 0 when there is no mismatch
//   text_emu --emulate [N]      N rounds of k_text_fill's workgroup restated on the host (emulate(), below): lines assembled in the image at the
//                               destination's misalignment and streamed out as aligned quads, against the plain concatenation of the lines
//   text_emu --render FMT [--prefix P --context CpG|CHG|CHH [--merged]] < rows.tsv > file
//                               FMT bedGraph|fraction|counts|methylKit: rows `chrom start end nmeth nunmeth [strand: + - or .]`, the header of the
//                               command's file first when --prefix is given; FMT cytosine_report: rows `chrom pos +|- nmeth nunmeth CG|CHG|CHH tri`;
//                               FMT perRead: rows `name chrom pos nmeth nunmeth`, every row a line (no header: the command prints none)
//   text_emu --selfcheck-reads [N]  the perRead line (txt_read_line_len, txt_put_read_line) against the snprintf calls of mdk_cmd_perread.c: every
//                               (m, u) in 0..700 x 0..700, N (default 10^7) seeded pairs with counts up to 2^31, rows without coverage, negative positions
//   text_emu --emulate-reads [N]  N rounds of k_rtext_fill's workgroup on the host (emulate_reads(), below): the names' span staged as aligned quads at
//                               every misalignment of the source, names of 0..255 bytes moved four bytes at a time into the image, the image at every
//                               misalignment of the destination, the direct path -- against snprintf's lines
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "mdk_text_core.h"

static uint64_t g_cases, g_bad;
static void bad(const char *what, uint32_t m, uint32_t u, const char *got, const char *want) {
    if(g_bad++ < 20) fprintf(stderr, "MISMATCH %s m=%u u=%u: core '%s' printf '%s'\n", what, m, u, got, want);
}
static void check_fixed(const char *what, uint32_t m, uint32_t u, double x, int dec, int width) {
    char got[64], want[64];
    char *e = txt_put_fixed(got, x, dec, width); *e = 0;
    if(dec == 6) snprintf(want, sizeof(want), "%f", x); else snprintf(want, sizeof(want), "%6.2f", x);
    g_cases++;
    if(strcmp(got, want) || (int)(e - got) != txt_fixed_len(x, dec, width)) bad(what, m, u, got, want);
}
static void check_pair(uint32_t m, uint32_t u) {
    const uint32_t cov = m + u;
    char got[64], want[64];
    if(cov) {
        check_fixed("%f m/cov", m, u, ((double)m) / cov, 6, 0);
        check_fixed("%6.2f 100m/cov", m, u, 100.0 * ((double)m) / cov, 2, 6);
        check_fixed("%6.2f 100u/cov", m, u, 100.0 * ((double)u) / cov, 2, 6);
        *txt_put_i32(got, txt_percent_int(m, cov)) = 0; snprintf(want, sizeof(want), "%i", (int)(100.0 * ((double)m) / cov));
        g_cases++; if(strcmp(got, want)) bad("(int) percent", m, u, got, want);
    }
    *txt_put_u32(got, m) = 0; snprintf(want, sizeof(want), "%" PRIu32, m);
    g_cases++; if(strcmp(got, want) || (int)strlen(got) != txt_digits_u32(m)) bad("%u", m, u, got, want);
    *txt_put_i32(got, (int32_t)cov) = 0; snprintf(want, sizeof(want), "%i", (int32_t)cov);
    g_cases++; if(strcmp(got, want) || (int)strlen(got) != txt_digits_i32((int32_t)cov)) bad("%i", m, u, got, want);
}
// the five layouts against the snprintf calls of put_site, and txt_line_len against the bytes written
static void check_lines(int32_t pos, uint32_t m, uint32_t u, int width, int strand, uint32_t context) {
    static const char *cctx[3] = {"G", "HG", "HH"};
    const char *chrom = "chrUn_KI270742v1"; const uint8_t tri[3] = {'C', 'A', 'G'};
    const uint32_t cov = m + u, cl = (uint32_t)strlen(chrom);
    for(int fmt = 0; fmt < MD_TEXT_PERREAD; fmt++) {              // (the perRead line has a row type of its own: check_read)
        char got[400], want[400];
        txt_row r = {fmt == MD_TEXT_CYTOSINE_REPORT ? pos + 1 : pos, pos + width, m, u, strand, context, tri};
        if(!txt_row_printed(fmt, r)) continue;
        char *e = txt_put_line(got, fmt, (const uint8_t *)chrom, cl, r); *e = 0;
        if(fmt == MD_TEXT_FRACTION) snprintf(want, sizeof(want), "%s\t%i\t%i\t%f\n", chrom, pos, pos + width, ((double)m) / cov);
        else if(fmt == MD_TEXT_COUNTS) snprintf(want, sizeof(want), "%s\t%i\t%i\t%i\n", chrom, pos, pos + width, cov);
        else if(fmt == MD_TEXT_METHYLKIT) snprintf(want, sizeof(want), "%s.%i\t%s\t%i\t%c\t%i\t%6.2f\t%6.2f\n", chrom, pos + 1, chrom, pos + 1, strand > 0 ? 'F' : 'R', cov, 100.0 * ((double)m) / cov, 100.0 * ((double)u) / cov);
        else if(fmt == MD_TEXT_CYTOSINE_REPORT) snprintf(want, sizeof(want), "%s\t%i\t%c\t%" PRIu32 "\t%" PRIu32 "\tC%s\t%s\n", chrom, pos + 1, strand > 0 ? '+' : '-', m, u, cctx[context], "CAG");
        else snprintf(want, sizeof(want), "%s\t%i\t%i\t%i\t%" PRIu32 "\t%" PRIu32 "\n", chrom, pos, pos + width, (int)(100.0 * ((double)m) / cov), m, u);
        g_cases++;
        if(strcmp(got, want) || (uint32_t)(e - got) != txt_line_len(fmt, cl, r)) bad("line", m, u, got, want);
    }
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
// a count below 2^31 whose magnitude is as likely small as large
static uint32_t rnd_count() { const int bits = 1 + (int)(rnd() % 31); return (uint32_t)(rnd() & ((1ull << bits) - 1)); }

static int selfcheck(uint64_t n_random) {
    for(uint32_t m = 0; m <= 600; m++) for(uint32_t u = 0; u <= 600; u++) { check_pair(m, u); if((m * 601 + u) % 97 == 0) check_lines((int32_t)(m * 1000 + u), m, u, 1 + (int)(u % 3), (m & 1) ? 1 : -1, u % 3); }
    for(uint64_t i = 0; i < n_random; i++) {
        const uint32_t m = rnd_count(), u = rnd_count();
        check_pair(m, u);
        if(i % 64 == 0) check_lines((int32_t)(rnd() & 0x7ffffff0), m, u, 1 + (int)(i % 3), (i & 64) ? 1 : -1, (uint32_t)(i % 3));
    }
    {   // the int32 extremes of %i, and the values where a digit count changes
        const int32_t v[] = {INT32_MIN, INT32_MIN + 1, -1000000000, -999999999, -10, -9, -1, 0, 1, 9, 10, 99, 100, 999999999, 1000000000, INT32_MAX - 1, INT32_MAX};
        for(int32_t x : v) {
            char got[32], want[32];
            *txt_put_i32(got, x) = 0; snprintf(want, sizeof(want), "%i", x);
            g_cases++; if(strcmp(got, want) || (int)strlen(got) != txt_digits_i32(x)) bad("%i extreme", (uint32_t)x, 0, got, want);
            *txt_put_u32(got, (uint32_t)x) = 0; snprintf(want, sizeof(want), "%" PRIu32, (uint32_t)x);
            g_cases++; if(strcmp(got, want) || (int)strlen(got) != txt_digits_u32((uint32_t)x)) bad("%u extreme", (uint32_t)x, 0, got, want);
        }
        for(uint32_t p = 1; p; p = p > UINT32_MAX / 10 ? 0 : p * 10) for(int d = -1; d <= 1; d++) check_pair(p + (uint32_t)d, 0), check_pair(7, p + (uint32_t)d);
        check_pair(0x7fffffffu, 0x7fffffffu); check_pair(0xffffffffu, 0); check_pair(1, 0xfffffffeu);
    }
    printf("{\"cases\": %" PRIu64 ", \"random_pairs\": %" PRIu64 ", \"mismatches\": %" PRIu64 "}\n", g_cases, n_random, g_bad);
    return g_bad ? 1 : 0;
}

static int render(int argc, char **argv) {
    static const char *fmts[] = {"bedGraph", "fraction", "counts", "methylKit", "cytosine_report", "perRead"};
    static const char *what[] = {" methylation levels", " methylation fractions", " methylation counts"};
    int fmt = -1, merged = 0; const char *prefix = NULL, *context = "CpG";
    for(int i = 0; i < MD_TEXT_N_FORMATS; i++) if(argc > 2 && !strcmp(argv[2], fmts[i])) fmt = i;
    if(fmt < 0) { fprintf(stderr, "text_emu --render: unknown format\n"); return 2; }
    for(int i = 3; i < argc; i++) {
        if(!strcmp(argv[i], "--prefix") && i + 1 < argc) prefix = argv[++i];
        else if(!strcmp(argv[i], "--context") && i + 1 < argc) context = argv[++i];
        else if(!strcmp(argv[i], "--merged")) merged = 1;
        else { fprintf(stderr, "text_emu --render: unknown option %s\n", argv[i]); return 2; }
    }
    if(prefix && fmt == MD_TEXT_METHYLKIT) fputs("chrBase\tchr\tbase\tstrand\tcoverage\tfreqC\tfreqT\n", stdout);
    else if(prefix && fmt != MD_TEXT_CYTOSINE_REPORT) printf("track type=\"bedGraph\" description=\"%s %s%s%s\"\n", prefix, context, merged ? " merged" : "", what[fmt]);
    char line[4096]; std::vector<char> out(2 * MD_TEXT_NAME_MAX + 128);
    while(fmt == MD_TEXT_PERREAD && fgets(line, sizeof(line), stdin)) {
        char name[1024], chrom[1024]; long long pos, m, u;
        if(sscanf(line, "%1023s %1023s %lld %lld %lld", name, chrom, &pos, &m, &u) != 5) { fprintf(stderr, "text_emu: bad perRead row: %s", line); return 2; }
        const uint32_t nl = (uint32_t)strlen(name), cl = (uint32_t)strlen(chrom);
        if(nl > MD_TEXT_NAME_MAX || cl > MD_TEXT_NAME_MAX) { fprintf(stderr, "text_emu: name longer than %d bytes\n", MD_TEXT_NAME_MAX); return 2; }
        char *e = txt_put_read_line(out.data(), (const uint8_t *)name, nl, (const uint8_t *)chrom, cl, (int32_t)pos, (uint32_t)m, (uint32_t)u);
        if((uint32_t)(e - out.data()) != txt_read_line_len(nl, cl, (int32_t)pos, (uint32_t)m, (uint32_t)u)) { fprintf(stderr, "text_emu: txt_read_line_len disagrees with txt_put_read_line\n"); return 3; }
        fwrite(out.data(), 1, (size_t)(e - out.data()), stdout);
    }
    while(fgets(line, sizeof(line), stdin)) {
        char chrom[1024], f3[64], f6[64] = ".", f7[64] = ""; long long a, b, m, u; txt_row r; uint8_t tri[3] = {'N', 'N', 'N'};
        memset(&r, 0, sizeof(r));
        if(fmt == MD_TEXT_CYTOSINE_REPORT) {
            if(sscanf(line, "%1023s %lld %63s %lld %lld %63s %63s", chrom, &a, f3, &m, &u, f6, f7) != 7 || strlen(f7) != 3) { fprintf(stderr, "text_emu: bad report row: %s", line); return 2; }
            r.a = (int32_t)a; r.strand = f3[0] == '+' ? 1 : -1; r.context = !strcmp(f6, "CG") ? 0 : !strcmp(f6, "CHG") ? 1 : 2; memcpy(tri, f7, 3);
        } else {
            const int n = sscanf(line, "%1023s %lld %lld %lld %lld %63s", chrom, &a, &b, &m, &u, f6);
            if(n < 5) { fprintf(stderr, "text_emu: bad row: %s", line); return 2; }
            r.a = (int32_t)a; r.b = (int32_t)b; r.strand = f6[0] == '+' ? 1 : f6[0] == '-' ? -1 : 0;
            if(fmt == MD_TEXT_METHYLKIT && r.strand == 0) { fprintf(stderr, "text_emu: a methylKit row needs its strand\n"); return 2; }
        }
        r.m = (uint32_t)m; r.u = (uint32_t)u; r.tri = tri;
        const uint32_t cl = (uint32_t)strlen(chrom);
        if(cl > MD_TEXT_NAME_MAX) { fprintf(stderr, "text_emu: contig name longer than %d bytes\n", MD_TEXT_NAME_MAX); return 2; }
        if(!txt_row_printed(fmt, r)) continue;
        char *e = txt_put_line(out.data(), fmt, (const uint8_t *)chrom, cl, r);
        if((uint32_t)(e - out.data()) != txt_line_len(fmt, cl, r)) { fprintf(stderr, "text_emu: txt_line_len disagrees with txt_put_line\n"); return 3; }
        fwrite(out.data(), 1, (size_t)(e - out.data()), stdout);
    }
    return ferror(stdout) ? 3 : 0;
}

// k_text_len / k_text_blocks / k_text_fill restated on the host, workgroup by workgroup with the kernel's per-lane bodies and its barriers
// as loop boundaries: random rows in every format into a destination at every misalignment 0..15, with guard bytes around it -- the image
// plan (txt_plan_image) must reproduce the plain concatenation of the lines, store only aligned quads, and touch nothing outside
static int emulate(uint64_t rounds) {
    const uint32_t WGS = 256, IMG = 24 * 1024, GUARD = 64;
    static const char *names[] = {"chr1", "chrUn_KI270742v1", "X", NULL, NULL};
    std::string long_a(255, 'L'), long_b(130, 'M'); names[3] = long_a.c_str(); names[4] = long_b.c_str();
    uint64_t bad_rounds = 0, direct_blocks = 0, image_blocks = 0, quads = 0;
    for(uint64_t round = 0; round < rounds; round++) {
        const int fmt = (int)(round % MD_TEXT_PERREAD), n_names = (round % 7 == 3) ? 5 : 3; const uint32_t n = 1 + (uint32_t)(rnd() % 1500), mis = (uint32_t)(round % 16);
        std::vector<txt_row> row(n); std::vector<uint32_t> nm(n), len(n); std::vector<uint8_t> tri(3 * (size_t)n, 'A');
        std::string want;
        for(uint32_t i = 0; i < n; i++) {
            txt_row &r = row[i]; const uint64_t x = rnd();
            r.a = (int32_t)(rnd() & 0x7ffffff0) >> (int)(x % 28); r.b = r.a + 1 + (int32_t)(x % 3); r.m = (x & 256) ? rnd_count() : (uint32_t)(rnd() % 40); r.u = (x & 512) ? rnd_count() : (uint32_t)(rnd() % 40);
            r.strand = (x & 1024) ? 1 : -1; r.context = (uint32_t)((x >> 12) % 3); r.tri = &tri[3 * (size_t)i]; nm[i] = (uint32_t)((x >> 16) % n_names);
            const uint32_t cl = (uint32_t)strlen(names[nm[i]]);
            len[i] = txt_row_printed(fmt, r) && (x >> 20) % 5 ? txt_line_len(fmt, cl, r) : 0;        // (a fifth of the rows filtered out, as rows of another context are)
            if(len[i]) { char buf[1024]; char *e = txt_put_line(buf, fmt, (const uint8_t *)names[nm[i]], cl, r); want.append(buf, (size_t)(e - buf)); }
        }
        std::vector<uint8_t> mem(want.size() + 2 * GUARD + 32, 0xEE);
        uint8_t *dst = mem.data() + GUARD; dst += (16 - ((uintptr_t)dst & 15)) % 16 + mis;
        uint64_t off = 0; int ok = 1;
        for(uint32_t b0 = 0; b0 < n; b0 += WGS) {
            const uint32_t b1 = b0 + WGS < n ? b0 + WGS : n; uint32_t total = 0; std::vector<uint32_t> ex(WGS, 0);
            for(uint32_t i = b0; i < b1; i++) { ex[i - b0] = total; total += len[i]; }
            uint8_t *g = dst + off;
            if(total > IMG) { direct_blocks++; for(uint32_t i = b0; i < b1; i++) if(len[i]) txt_put_line((char *)g + ex[i - b0], fmt, (const uint8_t *)names[nm[i]], (uint32_t)strlen(names[nm[i]]), row[i]); }
            else if(total) {
                static uint8_t img[24 * 1024 + 16];
                const txt_image_plan P = txt_plan_image((uint64_t)(uintptr_t)g, total);
                for(uint32_t i = b0; i < b1; i++) if(len[i]) txt_put_line((char *)img + P.sh + ex[i - b0], fmt, (const uint8_t *)names[nm[i]], (uint32_t)strlen(names[nm[i]]), row[i]);
                uint8_t *g0 = g - P.sh;
                if(((uintptr_t)g0 & 15) || P.end > sizeof(img) || P.quad1 * 16 > P.end || (P.quad0 && P.sh == 0)) ok = 0;
                for(uint32_t k = P.quad0; k < P.quad1; k++) { memcpy(g0 + 16 * k, img + 16 * k, 16); quads++; }
                for(uint32_t t = 0; t < WGS; t++) { if(P.sh + t < P.head_end) g0[P.sh + t] = img[P.sh + t]; if(P.tail0 + t < P.end) g0[P.tail0 + t] = img[P.tail0 + t]; }
                if(P.head_end > P.sh + WGS || P.end > P.tail0 + WGS) ok = 0;
                image_blocks++;
            }
            off += total;
        }
        if(off != want.size() || memcmp(dst, want.data(), want.size())) ok = 0;
        for(uint8_t *q = mem.data(); q < dst; q++) if(*q != 0xEE) ok = 0;
        for(uint8_t *q = dst + want.size(); q < mem.data() + mem.size(); q++) if(*q != 0xEE) ok = 0;
        if(!ok && bad_rounds++ < 5) fprintf(stderr, "MISMATCH emulate round %" PRIu64 " fmt %d n %u misalignment %u\n", round, fmt, n, mis);
    }
    printf("{\"rounds\": %" PRIu64 ", \"image_blocks\": %" PRIu64 ", \"direct_blocks\": %" PRIu64 ", \"quads\": %" PRIu64 ", \"mismatches\": %" PRIu64 "}\n", rounds, image_blocks, direct_blocks, quads, bad_rounds);
    return bad_rounds ? 1 : 0;
}

// ---- perRead ----
// a read's line as the command prints it (mdk_cmd_perread.c:81-82), the name given by length
static int want_read_line(char *want, size_t cap, const uint8_t *name, uint32_t nl, const char *chrom, int32_t pos, uint32_t m, uint32_t u) {
    if(m + u > 0) return snprintf(want, cap, "%.*s\t%s\t%" PRId64 "\t%f\t%" PRIu32 "\n", (int)nl, (const char *)name, chrom, (int64_t)pos, 100. * ((double)m) / (m + u), m + u);
    return snprintf(want, cap, "%.*s\t%s\t%" PRId64 "\t0.0\t%" PRIu32 "\n", (int)nl, (const char *)name, chrom, (int64_t)pos, m + u);
}
static uint64_t g_zero_cov, g_negative;
static void check_read(int32_t pos, uint32_t m, uint32_t u) {
    if(m + u == 0) g_zero_cov++;
    if(pos < 0) g_negative++;
    static const char *name = "A00123:45:HXXXXXXXX:1:1101:12345:67890", *chrom = "chr21";
    char got[256], want[256];
    const uint32_t nl = (uint32_t)strlen(name), cl = (uint32_t)strlen(chrom);
    char *e = txt_put_read_line(got, (const uint8_t *)name, nl, (const uint8_t *)chrom, cl, pos, m, u); *e = 0;
    const int l = want_read_line(want, sizeof(want), (const uint8_t *)name, nl, chrom, pos, m, u);
    g_cases++;
    if(strcmp(got, want) || (int)(e - got) != l || txt_read_line_len(nl, cl, pos, m, u) != (uint32_t)l) bad("perRead line", m, u, got, want);
}
static int selfcheck_reads(uint64_t n_random) {
    for(uint32_t m = 0; m <= 700; m++) for(uint32_t u = 0; u <= 700; u++) check_read((int32_t)(m * 701 + u), m, u);
    for(uint64_t i = 0; i < n_random; i++) {
        const uint32_t m = rnd_count(), u = rnd_count(); const int32_t pos = (int32_t)(rnd() & 0x7fffffff) >> (int)(i % 31);
        check_read(i % 16 == 5 ? -pos - 1 : pos, i % 64 == 9 ? 0 : m, i % 64 == 9 ? 0 : u);
    }
    {
        const int32_t v[] = {INT32_MIN, INT32_MIN + 1, -1000000000, -999999999, -10, -9, -1, 0, 1, 9, 10, 999999999, 1000000000, INT32_MAX};
        for(int32_t x : v) { check_read(x, 0, 0); check_read(x, 3, 4); check_read(x, 0xffffffffu, 1); }      // (2^32 - 1 + 1 wraps to 0, as the host's sum does)
        for(uint32_t p = 1; p; p = p > UINT32_MAX / 10 ? 0 : p * 10) for(int d = -1; d <= 1; d++) { check_read(7, p + (uint32_t)d, 0); check_read(7, 0, p + (uint32_t)d); check_read(7, 1, p + (uint32_t)d); }
        check_read(0, 0x7fffffffu, 0x7fffffffu); check_read(0, 0x80000000u, 0x80000000u);
    }
    printf("{\"cases\": %" PRIu64 ", \"random_pairs\": %" PRIu64 ", \"zero_coverage\": %" PRIu64 ", \"negative_positions\": %" PRIu64 ", \"mismatches\": %" PRIu64 "}\n", g_cases, n_random, g_zero_cov, g_negative, g_bad);
    return g_bad ? 1 : 0;
}

// k_rtext_len / k_rtext_fill restated on the host, workgroup by workgroup: the rows' names are one span of a name buffer that starts at
// every misalignment 0..15 (and not at offset 0: the range begins inside the column), staged as aligned quads plus head and tail bytes into
// a stage that holds junk elsewhere; lanes move their names out of it with txt_copy_words and write the tail of the line; the image goes out
// as in emulate().  A workgroup over the image or the stage writes its lines directly.  Against the lines snprintf makes.
static int emulate_reads(uint64_t rounds) {
    const uint32_t WGS = 256, IMG = 30 * 1024, STAGE = 22 * 1024, GUARD = 64;
    static const char *chroms[] = {"chr1", "chr21", "chrUn_KI270742v1", NULL, NULL};
    std::string long_a(255, 'L'), long_b(130, 'M'); chroms[3] = long_a.c_str(); chroms[4] = long_b.c_str();
    alignas(16) static uint8_t img[30 * 1024 + 16], stage[22 * 1024 + 32];
    uint64_t bad_rounds = 0, image_blocks = 0, direct_text = 0, direct_names = 0, quads = 0, stage_quads = 0, eighty = 0, seen[256] = {0};
    for(uint64_t round = 0; round < rounds; round++) {
        const int regime = (int)(round % 8);
        const uint32_t n = 1 + (uint32_t)(rnd() % 1500), mis = (uint32_t)(round % 16), smis = (uint32_t)((round / 16) % 16), lead = (uint32_t)(rnd() % 300);
        std::vector<int64_t> off(n + 1); std::vector<uint32_t> ch(n), m(n), u(n), len(n); std::vector<int32_t> pos(n);
        std::vector<uint8_t> nmem(lead + (size_t)n * 255 + 2 * GUARD + 32, 0x5A);
        uint8_t *names = nmem.data() + GUARD; names += (16 - ((uintptr_t)names & 15)) % 16 + smis;
        // (names[0 .. lead) belong to the rows before the range)
        int64_t o = lead; std::string want;
        for(uint32_t i = 0; i < n; i++) {
            const uint64_t x = rnd();
            uint32_t nl;
            switch(regime) {
            case 3: nl = 80; ch[i] = 1; break;                                             // every name 80 bytes on a 5-byte contig name: must take the image
            case 4: nl = (uint32_t)(x % 256); ch[i] = (uint32_t)((x >> 16) % 3); break;
            case 5: nl = 30 + (uint32_t)(x % 40); ch[i] = 3 + (uint32_t)((x >> 16) % 2); break;  // contig names of hundreds of bytes: over the image
            case 6: nl = 89 + (uint32_t)(x % 8); ch[i] = 0; break;                         // names over the stage while the text may fit the image
            case 7: nl = (x & 7) ? (uint32_t)((x >> 8) % 12) : 255; ch[i] = (uint32_t)((x >> 16) % 3); break;        // very short, empty, and the longest
            default: nl = 30 + (uint32_t)(x % 40); ch[i] = (uint32_t)((x >> 16) % 3);
            }
            seen[nl]++;
            off[i] = o; for(uint32_t k = 0; k < nl; k++) names[o + k] = (uint8_t)(33 + (rnd() % 94)); o += nl;
            pos[i] = (int32_t)((rnd() & 0x7fffffff) >> (int)(x % 28)); if((x >> 40) % 50 == 0) pos[i] = -pos[i];
            m[i] = (x & 256) ? rnd_count() : (uint32_t)(rnd() % 40); u[i] = (x & 512) ? rnd_count() : (uint32_t)(rnd() % 40);
            if((x >> 44) % 9 == 0) m[i] = u[i] = 0;
            const uint32_t cl = (uint32_t)strlen(chroms[ch[i]]);
            len[i] = txt_read_line_len(nl, cl, pos[i], m[i], u[i]);
            char buf[1024]; const int l = want_read_line(buf, sizeof(buf), names + off[i], nl, chroms[ch[i]], pos[i], m[i], u[i]); want.append(buf, (size_t)l);
        }
        off[n] = o;
        std::vector<uint8_t> mem(want.size() + 2 * GUARD + 32, 0xEE);
        uint8_t *dst = mem.data() + GUARD; dst += (16 - ((uintptr_t)dst & 15)) % 16 + mis;
        uint64_t at = 0; int ok = 1;
        for(uint32_t b0 = 0; b0 < n; b0 += WGS) {
            const uint32_t b1 = b0 + WGS < n ? b0 + WGS : n; uint32_t total = 0; std::vector<uint32_t> ex(WGS, 0);
            for(uint32_t i = b0; i < b1; i++) { ex[i - b0] = total; total += len[i]; }
            uint8_t *g = dst + at;
            const int64_t s0 = off[b0]; const uint32_t span = (uint32_t)(off[b1] - s0);
            if(regime == 3 && b1 - b0 == WGS) { eighty++; if(total > IMG || span > STAGE) ok = 0; }
            if(total > IMG || span > STAGE) {
                if(total > IMG) direct_text++; else direct_names++;
                for(uint32_t i = b0; i < b1; i++) txt_put_read_line((char *)g + ex[i - b0], names + off[i], (uint32_t)(off[i + 1] - off[i]), (const uint8_t *)chroms[ch[i]], (uint32_t)strlen(chroms[ch[i]]), pos[i], m[i], u[i]);
            } else {
                memset(stage, 0xA5, sizeof(stage)); memset(img, 0xC3, sizeof(img));
                const uint8_t *src = names + s0;
                const txt_image_plan S = txt_plan_image((uint64_t)(uintptr_t)src, span);
                const uint8_t *src0 = src - S.sh;
                if(((uintptr_t)src0 & 15) || S.end + 8 > sizeof(stage)) ok = 0;
                for(uint32_t k = S.quad0; k < S.quad1; k++) { if(16 * k < S.sh || 16 * k + 16 > S.end) ok = 0; memcpy(stage + 16 * k, src0 + 16 * k, 16); stage_quads++; }      // (a quad read lies inside the span)
                for(uint32_t t = 0; t < WGS; t++) { if(S.sh + t < S.head_end) stage[S.sh + t] = src0[S.sh + t]; if(S.tail0 + t < S.end) stage[S.tail0 + t] = src0[S.tail0 + t]; }
                if(S.head_end > S.sh + WGS || S.end > S.tail0 + WGS) ok = 0;
                const txt_image_plan P = txt_plan_image((uint64_t)(uintptr_t)g, total);
                for(uint32_t i = b0; i < b1; i++) {
                    uint8_t *q = img + P.sh + ex[i - b0]; const uint32_t nl = (uint32_t)(off[i + 1] - off[i]);
                    txt_copy_words(q, stage, S.sh + (uint32_t)(off[i] - s0), nl);
                    txt_put_read_tail((char *)q + nl, (const uint8_t *)chroms[ch[i]], (uint32_t)strlen(chroms[ch[i]]), pos[i], m[i], u[i]);
                }
                uint8_t *g0 = g - P.sh;
                if(((uintptr_t)g0 & 15) || P.end > sizeof(img) || P.quad1 * 16 > P.end || (P.quad0 && P.sh == 0)) ok = 0;
                for(uint32_t k = P.quad0; k < P.quad1; k++) { memcpy(g0 + 16 * k, img + 16 * k, 16); quads++; }
                for(uint32_t t = 0; t < WGS; t++) { if(P.sh + t < P.head_end) g0[P.sh + t] = img[P.sh + t]; if(P.tail0 + t < P.end) g0[P.tail0 + t] = img[P.tail0 + t]; }
                if(P.head_end > P.sh + WGS || P.end > P.tail0 + WGS) ok = 0;
                image_blocks++;
            }
            at += total;
        }
        if(at != want.size() || memcmp(dst, want.data(), want.size())) ok = 0;
        for(uint8_t *q = mem.data(); q < dst; q++) if(*q != 0xEE) ok = 0;
        for(uint8_t *q = dst + want.size(); q < mem.data() + mem.size(); q++) if(*q != 0xEE) ok = 0;
        if(!ok && bad_rounds++ < 5) fprintf(stderr, "MISMATCH emulate-reads round %" PRIu64 " regime %d n %u misalignment %u source %u\n", round, regime, n, mis, smis);
    }
    uint32_t lengths = 0; for(int i = 0; i < 256; i++) if(seen[i]) lengths++;
    printf("{\"rounds\": %" PRIu64 ", \"image_blocks\": %" PRIu64 ", \"direct_text_blocks\": %" PRIu64 ", \"direct_names_blocks\": %" PRIu64 ", \"eighty_byte_blocks\": %" PRIu64
           ", \"stage_quads\": %" PRIu64 ", \"quads\": %" PRIu64 ", \"name_lengths\": %u, \"mismatches\": %" PRIu64 "}\n",
           rounds, image_blocks, direct_text, direct_names, eighty, stage_quads, quads, lengths, bad_rounds);
    return bad_rounds ? 1 : 0;
}

int main(int argc, char **argv) {
    if(argc >= 2 && !strcmp(argv[1], "--emulate-reads")) return emulate_reads(argc > 2 ? strtoull(argv[2], NULL, 10) : 4000ull);
    if(argc >= 2 && !strcmp(argv[1], "--selfcheck-reads")) return selfcheck_reads(argc > 2 ? strtoull(argv[2], NULL, 10) : 10000000ull);
    if(argc >= 2 && !strcmp(argv[1], "--emulate")) return emulate(argc > 2 ? strtoull(argv[2], NULL, 10) : 4000ull);
    if(argc >= 2 && !strcmp(argv[1], "--selfcheck")) return selfcheck(argc > 2 ? strtoull(argv[2], NULL, 10) : 20000000ull);
    if(argc >= 3 && !strcmp(argv[1], "--render")) return render(argc, argv);
    fprintf(stderr, "usage: text_emu --selfcheck [N] | --emulate [N] | --selfcheck-reads [N] | --emulate-reads [N] | --render bedGraph|fraction|counts|methylKit|cytosine_report|perRead [--prefix P --context CpG|CHG|CHH [--merged]] < rows > file\n");
    return 2;
}
