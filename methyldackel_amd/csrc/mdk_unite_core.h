// mdk_unite_core.h -- samples' rows joined into one site table: which sites the table holds, where a row finds its site, and what is
// refused (csrc/mdk_unite.hip: mdk.unite).
//
// S samples, each n_s rows strictly ascending in (contig, start).  A row is PRESENT in its sample if nmeth + nunmeth >= min_depth, the sum
// formed in 64 bits; a site is a (contig, start) some sample holds a present row of; the table holds the sites at least min_samples
// samples hold, ascending, with the counts of every sample.  (contig, start) is a bounded integer domain, so there is no sort:
//   the extent    of contig c is the largest start + 1 of any row of any sample on it (the last row of c in every sample: the rows ascend),
//                 rounded up to whole 32-bit words; the contigs' words lie one behind the other, base[c] the first of c (uni_words)
//   the bitmap    bit (start & 31) of word base[contig] + (start >> 5) is set for every present row.  Only word indices are ever formed:
//                 a bit offset passes 2^32 where a word index -- at most UNI_MAX_WORDS, 2^35 bits, a bitmap of 4 GiB -- does not
//   the rank      rankw[w] = the bits set in the words before w; the site of a row is rankw[w] + the bits of word w below its own
//                 (uni_locate).  The sites of the union are thus numbered 0 .. n_union - 1 in ascending (contig, start)
//   the tally     count[site] = the samples that hold it; keep = count >= min_samples; the kept sites are numbered by a scan
// What is refused (UNI_E_*): of a row, looking at rows i - 1 and i of its sample alone -- not strictly ascending, a contig index outside
// the names, a context above 2, a negative start --; of a kept site, a sample whose present row gives another end, context or strand than
// the row that wrote the site (uni_agree): samples of one reference never do; of the whole, more than UNI_MAX_WORDS words or more than
// UNI_MAX_SITES sites in the union (the caller's: they are sums).  UNI_E_CHANGED is the fill's: a present row that has no bit in the
// bitmap, which only columns changed since the measure give.
//
// Plain C++ as mdk_region_core.h: it compiles for the device (mdk_unite.hip) and for the host (tools/unite_emu.cpp runs the kernels'
// blocking over it), which is how it is tested without a GPU.
#ifndef MDK_UNITE_CORE_H
#define MDK_UNITE_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MDK_UNI __host__ __device__ __forceinline__
#else
#define MDK_UNI static inline
#endif

enum { UNI_E_ORDER = 1, UNI_E_CONTIG = 2, UNI_E_CONTEXT = 4, UNI_E_START = 8, UNI_E_DISAGREE = 16, UNI_E_CHANGED = 32 };
// UNI_ROWS: rows, and union sites, of a workgroup; UNI_BLOCK_WORDS: bitmap words of one entry of the block table; UNI_SCAN: entries of a
// round of the one-workgroup scan of a block table (k_unite_blocks)
enum { UNI_ROWS = 256, UNI_BLOCK_WORDS = 16, UNI_SCAN = 1024, UNI_MAX_SAMPLES = 1024 };
#define UNI_MAX_WORDS (1ll << 30)
#define UNI_MAX_SITES (1ll << 30)
#define UNI_NONE 0xFFFFFFFFu

MDK_UNI int uni_present(int32_t m, int32_t u, int32_t min_depth) { return (int64_t)m + (int64_t)u >= (int64_t)min_depth; }

// what is wrong with row (contig, start, ctx) behind row (pcontig, pstart) of its sample; has_prev 0 for the sample's first row
MDK_UNI uint32_t uni_row_check(int has_prev, int32_t pcontig, int32_t pstart, int32_t contig, int32_t start, int32_t ctx, int32_t n_contigs) {
    uint32_t err = 0;
    if((uint32_t)ctx > 2u) err |= UNI_E_CONTEXT;
    if(contig < 0 || contig >= n_contigs) err |= UNI_E_CONTIG;
    if(start < 0) err |= UNI_E_START;
    if(has_prev && !(pcontig < contig || (pcontig == contig && pstart < start))) err |= UNI_E_ORDER;
    return err;
}

// the words of a contig whose extent is `extent` bits (at most 2^31: a start is an int32)
MDK_UNI uint32_t uni_words(uint32_t extent) { return (extent >> 5) + ((extent & 31u) != 0u); }
MDK_UNI uint32_t uni_bit(int32_t start) { return 1u << (start & 31); }
MDK_UNI uint32_t uni_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// the tables of a measure: extent and base per contig, the bitmap and the rank of each of its n_words words, the sites of the union
struct uni_tables { const uint32_t *extent; const int64_t *base; const uint32_t *bits, *rankw; int32_t n_contigs; int64_t n_words; uint32_t n_union; };

// the word of (contig, start), or -1: outside the names, or outside the extent the measure found (rows of the measured columns never are)
MDK_UNI int64_t uni_word(const uni_tables &T, int32_t contig, int32_t start) {
    if(contig < 0 || contig >= T.n_contigs || start < 0 || (uint32_t)start >= T.extent[contig]) return -1;
    const int64_t w = T.base[contig] + (start >> 5);
    return w < T.n_words ? w : -1;
}

// the site of a present row, 0 .. n_union - 1, or UNI_NONE if its bit is not set
MDK_UNI uint32_t uni_locate(const uni_tables &T, int32_t contig, int32_t start) {
    const int64_t w = uni_word(T, contig, start);
    if(w < 0) return UNI_NONE;
    const uint32_t word = T.bits[w], bit = uni_bit(start);
    if(!(word & bit)) return UNI_NONE;
    const uint32_t r = T.rankw[w] + uni_popc(word & (bit - 1u));
    return r < T.n_union ? r : UNI_NONE;
}

// where kept site r stands in the result: the scanned total of its block of UNI_ROWS sites + its place inside (UNI_NONE: not kept)
MDK_UNI int64_t uni_place(const uint32_t *ktot, const uint32_t *map, uint32_t r) {
    const uint32_t in = map[r];
    return in == UNI_NONE ? -1 : (int64_t)ktot[r / UNI_ROWS] + in;
}

// does a sample's row say of the site what the row that wrote it said?
MDK_UNI int uni_agree(int32_t end, int32_t ctx, int32_t strand, int32_t site_end, int32_t site_ctx, int32_t site_strand) {
    return end == site_end && ctx == site_ctx && strand == site_strand;
}
#endif
