// cohort_emu -- csrc/mdk_cohort_core.h on the host, in the blocking of csrc/mdk_cohort.hip's kernels: tiles of sites, blocks of samples, a
// wavefront's image and its plan of aligned quads and ragged ends, a line's 16-byte stretches dealt over 64 lanes.  The GPU-less half of the
// tests: tests/test_cohort_io_cpu.py holds it against tests/cohort_rule.py.
//
// stdin, one job:
//   R fmt tile sample_block S n n_contigs lead      render: the table's lines (no header) as they come to lie `lead` bytes behind a 16-byte
//     then n_contigs names, one a line; n lines    boundary.  stdout: "OK bytes\n" and the bytes, or "ERR what site sample\n"
//     "contig start end context strand nsamples";
//     S * n lines "m u", sample-major
//   P tile S n_contigs bytes begin has_prev c x     parse text[begin .. bytes): stdout "OK rows\n" and a line per row, the six site columns
//     then the names; then `bytes` raw bytes        and m u per sample, or "ERR name row offset\n"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "mdk_cohort_core.h"

#define LANES 64
#define WAVES 4
#define SPAN 4096
#define PARSE_ROWS 64
#define LDS_BYTES (64 << 10)

static std::vector<uint8_t> g_names; static std::vector<uint32_t> g_off, g_sorted;

static void read_names(int nc) {
    char buf[1024];
    g_off.assign(1, 0);
    for(int c = 0; c < nc; c++) {
        if(!fgets(buf, sizeof buf, stdin)) exit(2);
        size_t k = strlen(buf);
        if(k && buf[k - 1] == '\n') k--;
        g_names.insert(g_names.end(), buf, buf + k);
        g_off.push_back((uint32_t)g_names.size());
    }
    g_sorted.resize(nc);
    for(int c = 0; c < nc; c++) g_sorted[c] = c;
    std::stable_sort(g_sorted.begin(), g_sorted.end(), [&](uint32_t a, uint32_t b) {
        return prs_name_cmp(g_names.data() + g_off[a], g_off[a + 1] - g_off[a], g_names.data() + g_off[b], g_off[b + 1] - g_off[b]) < 0; });
    g_names.resize(g_names.size() + 16);
}

// image bytes [p.sh, p.end) to dst as the lanes store them: whole quads, then the ragged ends
static void store_image(const uint8_t *img, const txt_image_plan &p, uint8_t *dst, uint32_t nl) {
    uint8_t *const base = dst - p.sh;
    for(uint32_t l = 0; l < nl; l++) {
        for(uint32_t q = p.quad0 + l; q < p.quad1; q += nl) memcpy(base + 16u * q, img + 16u * q, 16);
        for(uint32_t i = p.sh + l; i < p.head_end; i += nl) base[i] = img[i];
        for(uint32_t i = p.tail0 + l; i < p.end; i += nl) base[i] = img[i];
    }
}

static int render() {
    int fmt, tile, sblock, S, nc; long long n_, lead;
    if(scanf("%d %d %d %d %lld %d %lld\n", &fmt, &tile, &sblock, &S, &n_, &nc, &lead) != 7) return 2;
    const int64_t n = n_;
    read_names(nc);
    std::vector<int32_t> contig(n), start(n), end(n), ctx(n), strand(n), ns(n), M((size_t)S * n), U((size_t)S * n);
    for(int64_t i = 0; i < n; i++) if(scanf("%d %d %d %d %d %d", &contig[i], &start[i], &end[i], &ctx[i], &strand[i], &ns[i]) != 6) return 2;
    for(int64_t i = 0; i < (int64_t)S * n; i++) if(scanf("%d %d", &M[i], &U[i]) != 2) return 2;
    if(sblock > S) sblock = S;
    const int nb = (S + sblock - 1) / sblock;
    // k_ctext_len: a lane per site
    std::vector<int64_t> len(n + 1, 0); std::vector<uint16_t> part((size_t)nb * (n ? n : 1));
    uint64_t first = ~0ull;
    for(int64_t i = 0; i < n; i++) {
        const uint32_t what = coh_site_check(contig[i], start[i], end[i], (uint32_t)ctx[i] & 255u, nc);
        if(what) { first = std::min(first, coh_write_key(i, what, 0)); continue; }
        uint32_t acc = coh_prefix_len(fmt, g_off[contig[i] + 1] - g_off[contig[i]], start[i], end[i], (uint32_t)ctx[i], ns[i]);
        int bad = -1;
        for(int b = 0; b < nb; b++) {
            part[(size_t)b * n + i] = (uint16_t)acc;
            for(int s = b * sblock; s < std::min(S, (b + 1) * sblock); s++) {
                const int32_t m = M[(size_t)s * n + i], u = U[(size_t)s * n + i];
                if((m < 0 || u < 0) && bad < 0) bad = s;
                acc += coh_cell_len(fmt, (uint32_t)m, (uint32_t)u);
            }
        }
        if(bad >= 0) first = std::min(first, coh_write_key(i, COH_W_NEGATIVE, bad));
        len[i] = (int64_t)acc + 1;
    }
    if(first != ~0ull) { printf("ERR %u %lld %u\n", (unsigned)(first >> 11) & 31u, (long long)(first >> 16), (unsigned)(first & 2047u)); return 0; }
    int64_t run = 0;
    for(int64_t i = 0; i <= n; i++) { const int64_t x = len[i]; len[i] = run; run += x; }
    const int64_t total = len[n];
    uint8_t *const buf = (uint8_t *)aligned_alloc(16, (size_t)((lead + total + 31) & ~15ll) + 16);
    memset(buf, 0xee, (size_t)((lead + total + 31) & ~15ll) + 16);
    uint8_t *const out = buf + lead;
    // k_ctext_fill: items (tile, block), block -1 the prefixes
    const uint32_t imgw = (16u + (uint32_t)sblock * COH_CELL_MAX + 1u + 15u) & ~15u;
    std::vector<uint8_t> images(std::max<size_t>((size_t)WAVES * imgw, (size_t)64 * 320));
    for(int64_t t0 = 0; t0 < n; t0 += tile) {
        const int64_t t1 = std::min<int64_t>(n, t0 + tile);
        for(int blk = -1; blk < nb; blk++) {
            if(blk < 0) {
                for(int64_t g0 = t0; g0 < t1; g0 += 64) {
                    for(int64_t i = g0; i < std::min<int64_t>(t1, g0 + 64); i++) {
                        uint8_t *const dst = out + len[i];
                        const uint32_t o = g_off[contig[i]];
                        coh_put_prefix((char *)&images[(size_t)(i - g0) * 320] + ((uint64_t)dst & 15u), fmt, g_names.data() + o, g_off[contig[i] + 1] - o, start[i], end[i], (uint32_t)ctx[i], strand[i], ns[i]);
                    }
                    for(int64_t i = g0; i < std::min<int64_t>(t1, g0 + 64); i++) {
                        uint8_t *const dst = out + len[i];
                        store_image(&images[(size_t)(i - g0) * 320], txt_plan_image((uint64_t)dst, part[i]), dst, 16);
                    }
                }
                continue;
            }
            const int s0 = blk * sblock, nbk = std::min(sblock, S - s0);
            const bool last = blk == nb - 1;
            for(int64_t i = t0; i < t1; i++) {
                uint8_t *const img = &images[(size_t)((i - t0) % WAVES) * imgw];
                uint32_t incl[LANES], w[LANES], sum = 0;
                for(int l = 0; l < LANES; l++) {
                    w[l] = l < nbk ? coh_cell_len(fmt, (uint32_t)M[(size_t)(s0 + l) * n + i], (uint32_t)U[(size_t)(s0 + l) * n + i]) : 0u;
                    sum += w[l]; incl[l] = sum;
                }
                const uint32_t tot = incl[LANES - 1] + (last ? 1u : 0u);
                uint8_t *const dst = out + len[i] + part[(size_t)blk * n + i];
                const txt_image_plan p = txt_plan_image((uint64_t)dst, tot);
                for(int l = 0; l < nbk; l++) coh_put_cell((char *)img + p.sh + (incl[l] - w[l]), fmt, (uint32_t)M[(size_t)(s0 + l) * n + i], (uint32_t)U[(size_t)(s0 + l) * n + i]);
                if(last) img[p.sh + tot - 1] = '\n';
                store_image(img, p, dst, LANES);
            }
        }
    }
    // nothing in front of the text and nothing behind it was touched
    for(int64_t k = 0; k < lead; k++) if(buf[k] != 0xee) return 3;
    for(int64_t k = 0; k < 16; k++) if(out[total + k] != 0xee) return 3;
    printf("OK %lld\n", (long long)total);
    fwrite(out, 1, (size_t)total, stdout);
    free(buf);
    return 0;
}

static void load16(const uint8_t *text, int64_t bytes, int64_t p, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    for(int k = 0; k < COH_LANE && p + k < bytes; k++) w[k >> 2] |= (uint32_t)text[p + k] << (8 * (k & 3));
}

static int parse() {
    int tile, S, nc, has_prev, pc, px; long long bytes_, begin_;
    if(scanf("%d %d %d %lld %lld %d %d %d\n", &tile, &S, &nc, &bytes_, &begin_, &has_prev, &pc, &px) != 8) return 2;
    read_names(nc);
    const int64_t bytes = bytes_, begin = begin_;
    std::vector<uint8_t> tv((size_t)bytes + 32, 0);
    if(bytes && fread(tv.data(), 1, (size_t)bytes, stdin) != (size_t)bytes) return 2;
    const uint8_t *const text = tv.data();
    prs_tab T; T.name_off = g_off.data(); T.names = g_names.data(); T.sorted = g_sorted.data(); T.n_contigs = nc; T.ref = nullptr; T.ref_len = nullptr;
    // k_cparse_len / k_cparse_starts: a lane per 16 bytes, a span per workgroup
    std::vector<int64_t> line;
    for(int64_t p = 0; p < bytes; p += COH_LANE) {
        uint32_t w[4];
        if(p + COH_LANE <= begin) continue;
        load16(text, bytes, p, w);
        uint32_t s = coh_line_starts(w[0], w[1], w[2], w[3], p > begin && text[p - 1] == '\n', p, begin, bytes);
        while(s) { const int k = __builtin_ctz(s); s &= s - 1; line.push_back(p + k); }
    }
    const int64_t rows = (int64_t)line.size();
    line.push_back(bytes);
    // k_cparse_fill: tiles of R rows, a wavefront a line, a lane a stretch
    int R = std::min(tile, PARSE_ROWS);
    while(R > 1 && (size_t)8 * S * (R | 1) + (size_t)R * (COH_SITE_FIELDS + 1) * 4 > LDS_BYTES) R--;
    const int Rp = R | 1;
    const uint32_t want = COH_SITE_FIELDS + 2u * (uint32_t)S;
    std::vector<int32_t> stage((size_t)2 * S * Rp), rec((size_t)R * COH_SITE_FIELDS), col[COH_SITE_FIELDS], M((size_t)S * rows), U((size_t)S * rows);
    std::vector<uint32_t> rank_of(R);
    for(auto &c : col) c.assign(rows, 0);
    uint64_t first = ~0ull;
    for(int64_t row0 = 0; row0 < rows; row0 += R) {
        const int nr = (int)std::min<int64_t>(R, rows - row0);
        for(int r = 0; r < nr; r++) {
            const int64_t ls = line[row0 + r], nx = line[row0 + r + 1], le = coh_line_end(text, ls, nx);
            uint32_t rank = coh_line_rank(text, ls, le, nx - ls);
            if(rank == COH_RANK_NONE) {
                int32_t v = 0;
                rank = coh_field(text, ls, le, 0, T, v);
                if(rank == COH_RANK_NONE) rec[(size_t)r * COH_SITE_FIELDS] = v;
                uint32_t tabs = 0;
                for(int64_t q = ls & ~(int64_t)(COH_LANE - 1); q < le; q += LANES * COH_LANE) {
                    uint32_t mask[LANES], before[LANES], sum = 0;
                    for(int l = 0; l < LANES; l++) {
                        const int64_t p = q + (int64_t)l * COH_LANE;
                        uint32_t w[4];
                        mask[l] = 0;
                        if(p < le) { load16(text, bytes, p, w); mask[l] = coh_tabs(w[0], w[1], w[2], w[3]) & coh_inside(p, ls, le); }
                        before[l] = sum; sum += (uint32_t)__builtin_popcount(mask[l]);
                    }
                    for(int l = LANES - 1; l >= 0; l--) {                   // (the lanes in no particular order)
                        const int64_t p = q + (int64_t)l * COH_LANE;
                        uint32_t f = tabs + before[l], m = mask[l];
                        while(m) {
                            const int k = __builtin_ctz(m); m &= m - 1; f++;
                            if(f < want) {
                                const uint32_t e = coh_field(text, p + k + 1, le, f, T, v);
                                if(e != COH_RANK_NONE) rank = std::min(rank, e);
                                else if(f < COH_SITE_FIELDS) rec[(size_t)r * COH_SITE_FIELDS + f] = v;
                                else stage[(size_t)(((f - COH_SITE_FIELDS) & 1u) * S + ((f - COH_SITE_FIELDS) >> 1)) * Rp + r] = v;
                            }
                        }
                    }
                    tabs += sum;
                }
                rank = std::min(rank, coh_count_rank(tabs, S));
            }
            rank_of[r] = rank;
        }
        for(int r = 0; r < nr; r++) {
            const int32_t *const e = &rec[(size_t)r * COH_SITE_FIELDS];
            uint32_t rank = rank_of[r];
            if(rank == COH_RANK_NONE) rank = coh_row_rank(e[1], e[2], e[5], S);
            if(rank != COH_RANK_NONE) { first = std::min(first, (uint64_t)(row0 + r) << 8 | coh_rank_code(rank)); continue; }
            for(int f = 0; f < COH_SITE_FIELDS; f++) col[f][row0 + r] = e[f];
            for(int s = 0; s < S; s++) { M[(size_t)s * rows + row0 + r] = stage[(size_t)s * Rp + r]; U[(size_t)s * rows + row0 + r] = stage[(size_t)(S + s) * Rp + r]; }
        }
    }
    // k_cparse_order
    for(int64_t i = 0; i < rows; i++) {
        if(i == 0 && !has_prev) continue;
        const int32_t c0 = i ? col[0][i - 1] : pc, x0 = i ? col[1][i - 1] : px;
        if(!coh_ascends(c0, x0, col[0][i], col[1][i])) first = std::min(first, (uint64_t)i << 8 | COH_E_ORDER);
    }
    if(first != ~0ull) { printf("ERR %s %lld %lld\n", coh_error_name((uint32_t)(first & 255u)), (long long)(first >> 8), (long long)line[first >> 8]); return 0; }
    printf("OK %lld\n", (long long)rows);
    for(int64_t i = 0; i < rows; i++) {
        for(int f = 0; f < COH_SITE_FIELDS; f++) printf(f ? " %d" : "%d", col[f][i]);
        for(int s = 0; s < S; s++) printf(" %d %d", M[(size_t)s * rows + i], U[(size_t)s * rows + i]);
        printf("\n");
    }
    return 0;
}

int main() {
    const int c = getchar();
    return c == 'R' ? render() : c == 'P' ? parse() : 2;
}
