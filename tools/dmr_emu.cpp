// dmr_emu.cpp -- TEST INFRASTRUCTURE: significant sites joined into regions (csrc/mdk_dmr_core.h, the very functions the kernels of
// csrc/mdk_dmr.hip run) executed on the host, in the kernels' own decomposition: a byte per row, blocks of 256 rows and wavefronts of 64,
// a candidate's previous candidate from the wavefront's 64-bit mask, then from the wavefronts before it, then from the block table; the
// heads' ordinals from the scanned head counts; a region's sums as prefix differences over whole blocks plus the rows of its two partial
// ends; the kept regions' places from the scanned keep counts.
//   build: g++ -O2 -ffp-contract=off -o tools/_build/dmr_emu tools/dmr_emu.cpp -Imethyldackel_amd/csrc
//   dmr_emu < table.tsv > regions.tsv
//       the input's first line holds `n n_contigs max_gap max_skip min_sites min_diff`, min_diff as the 16 hexadecimal digits of the
//       double's 64-bit pattern; then a line per row, `contig start end a b c d sig` (eight integers).  The output holds a line per kept
//       region: `contig start end nsites nsig direction a b c d meth_diff pvalue`, the two doubles as hexadecimal patterns.  A refused
//       table gives the single line `refused BIT ROW`: the DMR_E_* bit and the row the device names.
// Exit 0; 2 for input that is not such a table.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mdk_dmr_core.h"

static uint64_t pattern(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }

struct Status { uint32_t err = 0; uint64_t first = ~0ull; };
static void refuse(Status &st, uint32_t err, uint64_t row) {
    st.err |= err;
    const uint64_t v = (row << 8) | (uint64_t)(__builtin_ffs((int)err) - 1);
    if(v < st.first) st.first = v;
}

int main(int argc, char **argv) {
    if(argc > 1) { fprintf(stderr, "usage: dmr_emu < table.tsv > regions.tsv\n"); return 2; }
    long long n, n_contigs, max_gap, max_skip, min_sites; uint64_t bits;
    if(scanf("%lld %lld %lld %lld %lld %" SCNx64, &n, &n_contigs, &max_gap, &max_skip, &min_sites, &bits) != 6 || n < 0 || n > DMR_MAX_ROWS) { fprintf(stderr, "not a table\n"); return 2; }
    double min_diff; memcpy(&min_diff, &bits, 8);
    std::vector<int32_t> contig(n), start(n), end(n); std::vector<int64_t> a(n), b(n), c(n), d(n); std::vector<uint8_t> sig(n);
    for(long long i = 0; i < n; i++) {
        long long v[8];
        for(int q = 0; q < 8; q++) if(scanf("%lld", &v[q]) != 1) { fprintf(stderr, "row %lld is not eight integers\n", i); return 2; }
        contig[i] = (int32_t)v[0]; start[i] = (int32_t)v[1]; end[i] = (int32_t)v[2]; a[i] = v[3]; b[i] = v[4]; c[i] = v[5]; d[i] = v[6]; sig[i] = v[7] != 0;
    }
    const uint32_t N = (uint32_t)n, nb = (N + DMR_ROWS - 1) / DMR_ROWS, W = DMR_ROWS / 64;
    Status st;
    // k_dmr_rows: the checks, the bytes, the block table
    std::vector<uint8_t> code(n, DMR_CODE_NONE);
    std::vector<int32_t> blast(nb + 1, DMR_NO_ROW); std::vector<uint32_t> bcand(nb + 1, 0); std::vector<int64_t> ba(nb + 1, 0), bb(nb + 1, 0), bc(nb + 1, 0), bd(nb + 1, 0);
    for(uint32_t blk = 0; blk < nb; blk++)
        for(uint32_t i = blk * DMR_ROWS; i < N && i < (blk + 1) * DMR_ROWS; i++) {
            const uint32_t err = dmr_row_check(i > 0, i ? contig[i - 1] : 0, i ? start[i - 1] : 0, contig[i], start[i], (int32_t)n_contigs, a[i], b[i], c[i], d[i]);
            if(err) refuse(st, err, i);
            if(err & (DMR_E_NEGATIVE | DMR_E_ENTRY)) continue;
            code[i] = (uint8_t)dmr_code(sig[i], a[i], b[i], c[i], d[i]);
            if(code[i] != DMR_CODE_NONE) { blast[blk] = (int32_t)i; bcand[blk]++; }
            ba[blk] += a[i]; bb[blk] += b[i]; bc[blk] += c[i]; bd[blk] += d[i];
        }
    // k_dmr_blocks: exclusive prefixes in place, entry nb the totals
    { int32_t top = DMR_NO_ROW; uint32_t k = 0; int64_t sa = 0, sb = 0, sc = 0, sd = 0;
      for(uint32_t blk = 0; blk <= nb; blk++) {
          const int32_t l = blast[blk]; const uint32_t kk = bcand[blk]; const int64_t xa = ba[blk], xb = bb[blk], xc = bc[blk], xd = bd[blk];
          blast[blk] = top; bcand[blk] = k; ba[blk] = sa; bb[blk] = sb; bc[blk] = sc; bd[blk] = sd;
          if(blk < nb) { if(l > top) top = l; k += kk; sa += xa; sb += xb; sc += xc; sd += xd; }
      } }
    // the previous candidate of every row as the kernels find it: the wavefront's mask, the wavefronts before, the block table
    std::vector<uint64_t> cmask((size_t)nb * W, 0);
    for(uint32_t i = 0; i < N; i++) if(code[i] != DMR_CODE_NONE) cmask[i / 64] |= 1ull << (i % 64);
    auto prev_candidate = [&](uint32_t i) -> int32_t {
        const uint32_t blk = i / DMR_ROWS, wave = i / 64;
        const int near = dmr_prev_in_mask(cmask[wave], (int)(i % 64));
        if(near >= 0) return (int32_t)(wave * 64 + near);
        for(uint32_t w = wave; w-- > blk * W;) { const int top = dmr_last_in_mask(cmask[w]); if(top >= 0) return (int32_t)(w * 64 + top); }
        return blast[blk];
    };
    // k_dmr_heads: the head masks and the blocks' head counts; k_dmr_scan: the regions before each block
    std::vector<uint64_t> hmask((size_t)nb * W, 0); std::vector<uint32_t> htot(nb, 0); std::vector<int64_t> hoff(nb, 0);
    for(uint32_t i = 0; i < N; i++) {
        if(code[i] == DMR_CODE_NONE) continue;
        const int32_t p = prev_candidate(i);
        if(p == DMR_NO_ROW || !dmr_continues(contig[p], start[p], code[p], p, contig[i], start[i], code[i], (int32_t)i, (int32_t)max_gap, (int32_t)max_skip)) {
            hmask[i / 64] |= 1ull << (i % 64); htot[i / DMR_ROWS]++;
        }
    }
    int64_t raw = 0;
    for(uint32_t blk = 0; blk < nb; blk++) { hoff[blk] = raw; raw += htot[blk]; }
    if(st.err) { printf("refused %u %" PRIu64 "\n", 1u << (st.first & 0xff), st.first >> 8); return 0; }
    if(!raw) return 0;
    // k_dmr_bounds: the heads' ordinals, first and last
    std::vector<int32_t> first(raw, 0), last(raw, 0);
    for(uint32_t i = 0; i < N; i++) {
        const uint64_t hm = hmask[i / 64];
        if(!(hm >> (i % 64) & 1)) continue;
        int64_t r = hoff[i / DMR_ROWS] + __builtin_popcountll(hm & ((1ull << (i % 64)) - 1ull));
        for(uint32_t w = i / DMR_ROWS * W; w < i / 64; w++) r += __builtin_popcountll(hmask[w]);
        first[r] = (int32_t)i;
        if(r > 0) last[r - 1] = prev_candidate(i);
    }
    last[raw - 1] = blast[nb];
    // k_dmr_sum: whole blocks from the prefixes, the partial ends row by row; the margins, the filter, the places
    std::vector<int32_t> rnsig(raw); std::vector<int64_t> ra(raw), rb(raw), rc(raw), rd(raw); std::vector<uint32_t> rpos(raw, DMR_NO_PLACE);
    const uint32_t nrb = (uint32_t)((raw + DMR_ROWS - 1) / DMR_ROWS);
    std::vector<uint32_t> ktot(nrb, 0); std::vector<int64_t> koff(nrb, 0);
    for(int64_t r = 0; r < raw; r++) {
        const uint32_t lo = (uint32_t)first[r], hi = (uint32_t)last[r] + 1u;
        const rgn_split sp = rgn_split_range(lo, hi);
        uint32_t nsig = 0; int64_t sa = 0, sb = 0, sc = 0, sd = 0;
        if(sp.b0 < sp.b1) { nsig = bcand[sp.b1] - bcand[sp.b0]; sa = ba[sp.b1] - ba[sp.b0]; sb = bb[sp.b1] - bb[sp.b0]; sc = bc[sp.b1] - bc[sp.b0]; sd = bd[sp.b1] - bd[sp.b0]; }
        const uint32_t la = sp.a_end - lo, len = la + (hi - sp.b_beg);
        for(uint32_t q = 0; q < len; q++) {
            const uint32_t i = q < la ? lo + q : sp.b_beg + (q - la);
            nsig += code[i] != DMR_CODE_NONE; sa += a[i]; sb += b[i]; sc += c[i]; sd += d[i];
        }
        rnsig[r] = (int32_t)nsig; ra[r] = sa; rb[r] = sb; rc[r] = sc; rd[r] = sd;
        const uint32_t err = diff_margin_check(sa, sb, sc, sd);
        if(err) { refuse(st, err, lo); continue; }
        if(dmr_keep((int32_t)nsig, sa, sb, sc, sd, dmr_code_dir(code[lo]), (int32_t)min_sites, min_diff)) rpos[r] = ktot[r / DMR_ROWS]++;
    }
    int64_t n_out = 0;
    for(uint32_t blk = 0; blk < nrb; blk++) { koff[blk] = n_out; n_out += ktot[blk]; }
    if(st.err) { printf("refused %u %" PRIu64 "\n", 1u << (st.first & 0xff), st.first >> 8); return 0; }
    // k_dmr_fill: every kept region at its place
    std::vector<int64_t> at(n_out, -1);
    for(int64_t r = 0; r < raw; r++) if(rpos[r] != DMR_NO_PLACE) at[koff[r / DMR_ROWS] + rpos[r]] = r;
    for(int64_t o = 0; o < n_out; o++) {
        const int64_t r = at[o];
        if(r < 0) { fprintf(stderr, "place %lld has no region\n", (long long)o); return 1; }
        const int32_t f = first[r], l = last[r];
        printf("%d\t%d\t%d\t%d\t%d\t%d\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%016" PRIx64 "\t%016" PRIx64 "\n", contig[f], start[f], end[l], l - f + 1, rnsig[r],
               dmr_code_dir(code[f]), ra[r], rb[r], rc[r], rd[r], pattern(diff_meth(ra[r], rb[r], rc[r], rd[r])), pattern(diff_pvalue(ra[r], rb[r], rc[r], rd[r], nullptr)));
    }
    return 0;
}
