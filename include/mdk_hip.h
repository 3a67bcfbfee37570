/*
 * mdk_hip.h -- C ABI of the MI355X device library (libmdk_hip.so) for the `MethylDackel extract`
 * hot path.  Plain pointers and sizes only; no HIP, torch or C++ types cross this boundary, so
 * the C host (and the reference's own C code) can include it directly.
 *
 * What this boundary replaces in the reference (the reference has no FFI layer; its seam for the
 * hot path is the htslib pileup engine + callbacks it drives from extractCalls):
 *   md_dev_open / md_dev_cfg      <- the subset of `Config` the per-base arithmetic reads
 *                                    (MethylDackel.h:90-126: keepCpG/CHG/CHH, minPhred, minOppositeDepth,
 *                                    bounds[16], absoluteBounds[16]; defaults extract.c:715-753)
 *   md_dev_set_reference          <- faidx_fetch_seq window handed to the column loop (extract.c:381,388-390)
 *   md_read_batch / md_dev_upload <- the reads bam_mplp64_auto pulls through filter_func for one chunk
 *                                    (extract.c:379,394-399; common.c:407-463) *after* admission, with the
 *                                    CIGAR -> (qpos, is_del, is_refskip) resolution htslib does per column
 *                                    (resolve_cigar2) done once per read on the host
 *   md_dev_launch                 <- the whole per-chunk pileup: trimming (common.c:137-208), mate-overlap
 *                                    resolution (overlaps.c:54-147), context classification
 *                                    (common.c:49-82, extract.c:407-418) and the per-read-base counting
 *                                    loop (extract.c:420-441, 225-239; common.c:118-134)
 *   md_sites / md_dev_download    <- the (pos, nmethyl, nunmethyl, nOff, nVariant) tuple that reaches the
 *                                    variant filter and writeCall/processLast (extract.c:444-491)
 *
 * All functions return 0 on success and a negative value on failure (never throw, never exit);
 * md_dev_last_error() gives a message for the calling thread's last failure.
 */
#ifndef MDK_HIP_H
#define MDK_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MDK_ERR_HIP      (-1)   /* a HIP runtime call failed */
#define MDK_ERR_NODEVICE (-2)   /* no usable MI355X/gfx950 device */
#define MDK_ERR_ARG      (-3)   /* bad argument */
#define MDK_ERR_NOREF    (-4)   /* reference for the batch's contig was never uploaded */
#define MDK_ERR_STRAND0  (-5)   /* a read of undeterminable strand reached a methylation call
                                   (the reference aborts there: common.c:122-125) */
#define MDK_ERR_NOMEM    (-6)
#define MDK_ERR_PREP_HOST (-7)  /* device chunk preparation met a read name it does not handle (more records of one name than a
                                   lane keeps): prepare this chunk on the host (md_dev_submit of a host-built batch) */

typedef struct md_dev md_dev;

typedef struct {
    int32_t keepCpG, keepCHG, keepCHH;   /* contexts to count (Config.keep*) */
    int32_t minPhred;                    /* -p, already normalised to >= 1 (extract.c:997-1000) */
    int32_t minOppositeDepth;            /* >0: also produce nOff / nVariant per site */
    int32_t bounds[16];                  /* --OT/--OB/--CTOT/--CTOB, index 4*(strand-1)+{R1 left,R1 right,R2 left,R2 right} */
    int32_t absoluteBounds[16];          /* --nOT/--nOB/--nCTOT/--nCTOB, same indexing */
    int32_t tile;                        /* reference positions per LDS tile; 0 = library default */
    int32_t n_slots;                     /* batches that may be in flight at once; 0 = 2 (double buffering) */
    int32_t n_streams;                   /* 0 = a stream per slot; k > 0 = k streams, slots 8j .. 8j+7 work on stream j % k: the slots of one
                                            md_dev_launch_group can share a stream -- creating one costs the runtime ~5 ms */
} md_dev_cfg;

/* The device sees every admitted alignment as one or more gapless SEGMENTS: the CIGAR is expanded on the host
 * (reference <-> query map), so the kernel never walks a CIGAR.  A segment is a run of M/=/X bases; it is split
 * further so that the read it is overlap-resolved against (overlaps.c:54-119) either covers the whole segment with
 * one of ITS gapless runs, or does not touch it.  32 bytes, coalesced one per lane.
 * The payload of a read lives at blob + 4*off4:
 *   uint8 seq[(l_qseq+1)/2]   BAM 4-bit codes, high nibble = even query index; padded to a multiple of 4 bytes
 *   uint8 qual[l_qseq]        raw phred bytes; padded to a multiple of 4 bytes
 * The host preparation emits segments in file (coordinate) order of their reads, ascending within a read; the device does not rely
 * on it.  What a caller-built batch may hold (tests/test_gpu_pileup_kernel.py pins it):
 *   - segments in any order, any number of them on one position; a tile works through the run of the array between the first and the
 *     last segment that touches it and passes over what lies between them without touching it;
 *   - rpos >= 0, len >= 1, q0 + len <= l_qseq and, with MDK_SF_PARTNER, m_q0 + len <= m_l_qseq: every payload index a segment can name
 *     lies inside the payload, which lies inside the blob.  Nothing else is required of q0, m_q0 or the two reads' lengths;
 *   - a segment may start before beg, end after end or run past the contig's end: only its positions p with beg <= p < end and
 *     p < contig length are counted.  A segment with none, n_segs == 0 and beg == end are all fine and give no sites;
 *   - trimming windows (md_dev_cfg bounds / absoluteBounds) may be empty or wider than the read; a base outside its read's window, own
 *     or partner's, reads as N with quality 0 -- the partner's window is that of the partner's strand and read number (msf);
 *   - a segment of strand 0 (undeterminable) has no trimming window and matches no '+' or '-' run of md_dev_set_regions.  Where it
 *     covers a position at which its own strand would be called -- a G site, as for OB/CTOB -- the launch fails with MDK_ERR_STRAND0,
 *     whatever the base and its quality; over C sites it is opposite-strand evidence when minOppositeDepth > 0, and nothing otherwise.
 *     The error belongs to that launch: md_dev_download returns it once and the slot takes the next batch as any other. */
typedef struct {
    int32_t  rpos;       /* reference position of the segment's first base */
    uint32_t off4;       /* payload of the read the segment belongs to */
    uint32_t l_qseq;     /* length of that READ (trimming bounds are defined on the whole read, common.c:137-208) */
    uint32_t q0;         /* query index of the segment's first base */
    uint16_t len;        /* bases in the segment, >= 1 */
    uint8_t  sf;         /* MDK_SF_*: strand of origin (getStrand, common.c:84-116) and flags */
    uint8_t  msf;        /* partner: strand (bits 0-2) and read #2 (bit 3); valid iff sf & MDK_SF_PARTNER */
    uint32_t m_off4;     /* partner read's payload */
    uint32_t m_l_qseq;   /* partner read's length */
    uint32_t m_q0;       /* partner's query index of the base aligned to rpos */
} md_seg;
#define MDK_SF_STRAND  7u     /* bits 0-2: 1 OT, 2 OB, 3 CTOT, 4 CTOB, 0 undeterminable */
#define MDK_SF_READ2   8u     /* read #2 (BAM flag 0x80) */
#define MDK_SF_SECOND  16u    /* this read is the LATER-in-file member of its pair ('b' of overlaps.c:54) */
#define MDK_SF_PARTNER 32u    /* m_* valid: the partner covers the whole segment gaplessly */

/* The admitted reads of ONE interval [beg,end) of one contig -- what one chunk of extractCalls sees.
 * Host-owned; must stay valid until the slot is downloaded, waited for or synced (copies are asynchronous). */
typedef struct {
    int32_t  tid;
    int64_t  beg, end;          /* columns counted: beg <= pos < end (extract.c:400) */
    int32_t  n_segs;
    const md_seg *seg;          /* [n_segs] */
    const uint8_t *blob;
    uint64_t blob_bytes;
    int32_t  n_reads;           /* informational: admitted alignments behind the segments */
    uint64_t algo_bytes;        /* informational: sum over those reads of 16 + 4*n_cigar + ceil(l/2) + l */
} md_read_batch;

/* Result of one interval: every position with nmeth+nunmeth > 0 (or nOff > 0 when minOppositeDepth > 0),
 * ascending.  Pointers are host memory owned by the library, valid until the slot is reused. */
typedef struct { uint32_t pos, nmeth, nunmeth, meta; } md_site;   /* meta bit 0: reference base is G/g; bits 1-2: context 0 CpG / 1 CHG / 2 CHH */
typedef struct { uint32_t noff, nvar; } md_site_var;              /* opposite-strand depth / variant evidence (extract.c:225-239) */
typedef struct {
    int64_t n_sites;
    const md_site *site;
    const md_site_var *var;          /* NULL unless minOppositeDepth > 0 */
} md_sites;

/* Device-resident result of one interval, as the kernel leaves it: tile t's sites (ascending) occupy
 * site[seg[t].off .. seg[t].off + seg[t].cnt).  Tiles are in position order but their segments are not: a tile
 * reserves room for one site per kept context position with a single atomic, so segments appear in completion order
 * and a segment may be followed by unused slots.  Used for device-to-device exchange (RCCL gather). */
typedef struct { uint32_t off, cnt; } md_tile_seg;
typedef struct {
    int64_t n_slots;                 /* slots of d_site in use (>= number of sites) */
    int32_t n_tiles;
    const md_site *d_site; const md_site_var *d_var; const md_tile_seg *d_seg;   /* DEVICE pointers */
} md_sites_dev;

/* ---- chunk preparation on the device ----
 * Instead of a host-built md_read_batch the device can take the records of a chunk as they lie in the inflated BAM stream and
 * do the reference's per-record work itself: filter_func's admission tests (common.c:416-444) with the NH / XG aux walk,
 * getStrand (common.c:84-116), the mappability windows (common.c:277-335), the BED span test (common.c:432-439), the
 * conversion-efficiency filter (common.c:338-404), the read-name pairing of the overlap constructor/destructor callbacks
 * (overlaps.c:121-147, with htslib's buffer eviction) and the CIGAR -> segment expansion (overlaps.c:27-52).
 * md_prep_cfg: the part of `Config` those steps read (MethylDackel.h:90-126). */
typedef struct {
    int32_t min_mapq, ignore_flags, require_flags, keep_dupes, ignore_nh, keep_singleton, keep_discordant;
    int32_t min_phred;            /* -p, for the conversion-efficiency filter */
    float   min_conv_eff;         /* --minConversionEfficiency, 0 = off */
    int32_t map_on, min_mappable; /* -M/-B given; --minMappableBases */
    int32_t no_pairing;           /* mbias: no overlap handler is installed (MBias.c:158-161) */
    int32_t perread;              /* perRead: a record is kept iff it STARTS inside the chunk and passes -R / -F / -q (perRead.c:178-183) */
} md_prep_cfg;
/* whole records back to back, each as in the file: uint32 block_size, then block_size bytes.  Where the records of a range start is told in one
 * of three ways:
 *   d_rec_off != NULL   the range lies in DEVICE memory -- a run of members of a piece inflated on the device (md_piece_*): ptr and d_rec_off are
 *                       device pointers, d_rec_off[i] - rec_delta is the offset of the range's record i from ptr;
 *   h_rec_off != NULL   host memory with a table of its own (what the thread that inflated the bytes noted): h_rec_off[i] - rec_delta is the
 *                       offset of record i from ptr (host memory, read before md_dev_upload_raw returns or asynchronously when it is staging memory);
 *   neither             host memory; its records' offsets are the next n_records entries of the batch's rec_off array.
 * n_records must be filled in for every range as soon as one range has a table of either kind; a batch without any may leave it 0. */
typedef struct { const uint8_t *ptr; uint64_t bytes; const uint32_t *d_rec_off; uint32_t n_records, rec_delta; const uint32_t *h_rec_off; } md_raw_range;
/* The candidate records of ONE chunk: everything the region query [beg,end) of the chunk's contig returns (pos < end,
 * bam_endpos > beg), in file order.  Host ranges hold exactly those; a range in device memory is a run of whole BGZF members and may hold
 * records of the neighbouring chunk or contig at its ends, which the preparation drops (it redoes the query per record).  rec_off = for the records
 * of the ranges WITHOUT a table of their own, in order: offset of the record's block_size word in the concatenation of all ranges (less than 4 GiB in total).  woff/wlen: the reference window the chunk fetches (extract.c:381), which the
 * conversion-efficiency filter classifies inside.  Host-owned; valid until the slot is waited for. */
typedef struct {
    int32_t tid; int64_t beg, end;
    int32_t n_ranges; const md_raw_range *range;
    int32_t n_records; const uint32_t *rec_off;
    int64_t woff, wlen;
} md_raw_batch;
int  md_dev_set_prep(md_dev *h, const md_prep_cfg *cfg);
/* mappability of a contig, 1 bit per base (bit i%32 of word i/32; 1 = mappable), for the admission windows */
int  md_dev_set_mappability(md_dev *h, int32_t tid, const uint32_t *bits, int64_t n_bases);
/* md_dev_upload_raw = H2D of the ranges + the preparation kernels; the slot is then in the same state as after md_dev_upload
 * (launch / download / wait / bench work on it).  md_dev_submit_raw = upload_raw + launch.  md_dev_download / md_dev_wait
 * return MDK_ERR_PREP_HOST when the preparation gave up on the chunk (see above). */
int  md_dev_upload_raw(md_dev *h, int slot, const md_raw_batch *b);
/* The same for a caller that can keep its device memory: a batch that is ONE device-resident range (the usual chunk of a file inflated on the
 * device: a run of members of one piece) is not copied at all -- the preparation and the pileup read the records where md_piece_* left them,
 * with the piece's own record table.  Returns 1 then, and the range (the piece's buffers) must stay as it is until the slot's results have been
 * collected (md_dev_download / md_dev_download_group / md_dev_wait); 0 = copied as md_dev_upload_raw does (the memory may be reused after
 * md_dev_upload_wait); < 0 an error.  MDK_NO_INPLACE=1 in the environment: always copies. */
int  md_dev_upload_raw_inplace(md_dev *h, int slot, const md_raw_batch *b);
/* waits until the copies md_dev_upload_raw (or md_dev_upload) queued for the slot have read their host memory, which may then be reused */
int  md_dev_upload_wait(md_dev *h, int slot);
/* the same without waiting: 1 = they have, 0 = not yet, < 0 error */
int  md_dev_upload_done(md_dev *h, int slot);
int  md_dev_submit_raw(md_dev *h, int slot, const md_raw_batch *b);
/* the records of an uploaded slot back on the host, as the device holds them: the concatenation of the batch's ranges (bytes)
 * and every record's offset in it (rec_off[n_records]); for a chunk the device preparation gives up on (MDK_ERR_PREP_HOST)
 * whose records were inflated on the device and so never existed in host memory.  bytes/n_records: capacities in, sizes out. */
int  md_dev_read_raw(md_dev *h, int slot, uint8_t *bytes, uint64_t *n_bytes, uint32_t *rec_off, uint32_t *n_records);
/* The preparation kernels of a slot uploaded with md_dev_upload_raw, re-run `iters` times on the resident records and timed
 * with HIP events (the slot's segments are the same afterwards). */
int  md_dev_bench_prep(md_dev *h, int slot, int warmup, int iters, float *ms_per_chunk);
/* the same over `n` uploaded raw slots holding different intervals, `per_launch` chunks per launch of each preparation kernel (as
 * md_dev_launch_group prepares them), round robin on one stream: ms per LAUNCH when the records stream from HBM */
int  md_dev_bench_prep_rotate(md_dev *h, const int *slots, int n, int per_launch, int warmup, int iters, float *ms_per_launch);
/* Test hook: the segments the device built for an uploaded slot (off4 / m_off4 are BYTE offsets into the uploaded records,
 * qualities follow the sequence without padding), their number, and the number of admitted reads. */
int  md_dev_debug_segments(md_dev *h, int slot, md_seg *out, int64_t cap, int64_t *n_segs, int64_t *n_reads);

/* ---- BGZF inflate and BAM record framing on the device ----
 * What the reference gets from htslib inside sam_itr_next (common.c:413): bgzf_read_block's inflate of each <= 64 KiB member and
 * bam_read1's framing of the records in it.  The host hands over a PIECE of the file -- a run of whole BGZF members, compressed,
 * as they lie in the file -- with a table of its members (found by walking the 18-byte BGZF headers: BSIZE, and ISIZE from each
 * member's trailer); the device inflates every member (one wavefront each), checks its CRC32, walks the records of every member from its first
 * byte, and leaves: the inflated bytes, a table with the offset of every record, and per member a DIGEST (first/last record,
 * extent of the read ends, coordinate order inside) from which the host applies the reference's chunk schedule
 * (extract.c:325-350) without ever seeing a record.  Inflated bytes and record table stay in device memory; a chunk's records
 * are then handed to md_dev_upload_raw as device-resident ranges (md_raw_range.d_rec_off != NULL). */
typedef struct { uint64_t in_off; uint32_t in_len, out_len; uint64_t out_off; uint32_t crc32, reserved; } md_inf_member;   /* deflate stream at comp + in_off, in_len bytes; ISIZE; where its bytes go (running sum of ISIZE); the CRC32 of the member's trailer, checked on the device as htslib's bgzf_read_block checks it */
typedef struct {
    uint32_t n_rec, first_rec;           /* records in the member; index of its first record in the piece's record table */
    int32_t tid0, pos0, tidN, posN;      /* first and last record */
    int32_t min_endp, max_endp;          /* extent of bam_endpos over the member's records */
    int32_t ok, sorted;                  /* ok: the member starts and ends on record boundaries; sorted: placed records in coordinate order, none unplaced */
} md_inf_digest;
typedef struct md_piece md_piece;
typedef struct {
    int32_t n_mem; const md_inf_digest *digest;      /* host memory owned by the piece, valid until its next submit */
    uint32_t n_records; uint64_t out_bytes;
    const uint8_t *d_out; const uint32_t *d_rec_off;  /* DEVICE pointers: inflated bytes; offset (in d_out) of every record's block_size word */
} md_piece_info;
/* how many members the device inflates at once (the wavefronts k_inflate keeps resident, each on one member): a piece of a whole multiple of this
 * many members leaves no last, nearly empty round of them; <= 0: unknown */
int  md_piece_members_per_round(md_dev *h);
int  md_piece_create(md_dev *h, md_piece **out);     /* buffers grown on demand; its work is queued on one of a few streams the pieces of a handle share (four; MDK_PIECE_STREAMS=0: a stream of its own) */
void md_piece_destroy(md_piece *p);
/* asynchronous: H2D of `comp` (pinned memory makes it a DMA) and the member table, the kernels, D2H of the digests.  The member
 * table must be contiguous (out_off = running sum of out_len), out_len <= 65536.  comp/mem must stay valid until md_piece_wait. */
int  md_piece_submit(md_piece *p, const uint8_t *comp, uint64_t comp_bytes, const md_inf_member *mem, int32_t n_mem);
int  md_piece_wait(md_piece *p, md_piece_info *info);
/* inflated bytes / record offsets copied back to the host (tests; files whose records straddle members) */
int  md_piece_read(md_piece *p, uint64_t off, uint64_t bytes, uint8_t *dst);
int  md_piece_read_records(md_piece *p, uint32_t first, uint32_t n, uint32_t *dst);
/* inflated bytes copied to other DEVICE memory (text files read back: the bytes are parsed on the device, md_text_parse_*) */
int  md_piece_copy(md_piece *p, uint64_t off, uint64_t bytes, void *d_dst);
/* the kernels alone, re-run on the resident piece and timed with HIP events on its stream */
int  md_piece_bench(md_piece *p, int iters, float *ms_inflate, float *ms_walk);
int  md_piece_bench_crc(md_piece *p, int iters, float *ms_crc);      /* k_crc32 alone on the resident piece (and its verdict) */

typedef struct {
    float ms_total;      /* one launch bracketed by HIP events on the slot's stream (includes lone-launch dispatch latency), mean over iters */
    float ms_pileup;     /* the pileup kernel: `iters` launches back to back between two HIP events, divided by iters */
    uint64_t algo_bytes; /* algorithmic bytes of one launch (SURVEY.md 8d formula) */
    uint64_t n_sites;
    int32_t tile, n_tiles, lds_bytes;   /* geometry the launch used: positions per tile, tiles, LDS bytes per workgroup */
} md_bench_result;

int  md_dev_count(void);                                       /* number of HIP devices, <0 on error */
/* optional: create the device context and load the kernels ahead of md_dev_open (e.g. on a thread, while options and
 * input headers are still being read) */
int  md_dev_warm(int device);
/* for a process about to leave without closing its handle (the command's _exit; also run at exit): joins the helper threads md_dev_warm started
 * (registration of staging blocks, streams and device blocks made ahead) and starts none again.  md_dev_close joins them too, but a later
 * md_dev_warm / md_dev_open in the same process starts its own again.  Idempotent. */
void md_dev_quiesce(void);
/* How much device memory the caller expects to use (inflated pieces, chunk slots, contigs), told as early as it knows (the size of the BAM):
 * md_dev_warm's helper thread makes that much carved memory ahead, while the copy engines are still idle.  An allocation made later, next to
 * the pieces' copies, costs its caller 10-30 ms and holds up every other call into the runtime meanwhile (profiles/r06pf_*).  No handle
 * needed; may be called before, during or after md_dev_warm; without it memory is made when first asked for. */
void md_dev_reserve_hint(uint64_t device_bytes);
int  md_dev_open(int device, const md_dev_cfg *cfg, md_dev **out);
/* room for the references of contigs 0..n-1, so that a thread may upload the next contig (md_dev_set_reference and what goes with it) while
 * others work on slots of contigs already uploaded; without it md_dev_set_reference must not run next to other calls on the handle */
int  md_dev_reserve_contigs(md_dev *h, int32_t n);
void md_dev_close(md_dev *h);
const char *md_dev_last_error(void);
int  md_dev_tile(const md_dev *h);

/* Upload (once) the bases of a contig; letters verbatim from the FASTA (case matters: C/c, G/g). */
int  md_dev_set_reference(md_dev *h, int32_t tid, const char *seq, int64_t len);

/* -l/--keepStrand: restrict the sites of a contig (whose reference is already uploaded) to these runs -- sorted,
 * disjoint, half-open, strand 0 = either, 1 = '+' (only OT/CTOT reads are seen there), 2 = '-' (only OB/CTOB reads).
 * Replaces posOverlapsBED + readStrandOverlapsBED inside the column loop (extract.c:402-405,425; bed.c:46-64).
 * n = 0 leaves the contig without sites.  Calling it again replaces the previous restriction only where a position
 * is still a site, so set_reference again first to widen. */
typedef struct { int32_t start, end, strand; } md_region;
int  md_dev_set_regions(md_dev *h, int32_t tid, const md_region *runs, int64_t n);

/* mbias (MBias.c:57-230): histogram of calls over (strand, read number, position in read) instead of per-position
 * counts; the reference keeps it as strandMeth{meth1,unmeth1,meth2,unmeth2}[qpos] per strand (MethylDackel.h:171-176).
 * count[q*16 + (strand-1)*4 + (read 2 ? 2 : 0) + (unmethylated ? 1 : 0)], 0 <= q < len; strand 1..4 = OT, OB, CTOT, CTOB.
 * md_dev_mbias_submit = md_dev_upload + the histogram kernel; the batch (built WITHOUT mate pairing: mbias installs no
 * overlap handler, MBias.c:159) must stay valid until md_dev_slot_sync(slot) or the next submit on that slot returns.
 * The histogram accumulates over submits in device memory; md_dev_mbias_read waits for all of them and returns it
 * (memory owned by the handle, valid until the next read/reset/close). */
typedef struct { int32_t len; const uint32_t *count; } md_mbias;
int  md_dev_mbias_submit(md_dev *h, int slot, const md_read_batch *b);
/* the same from the chunk's raw records (md_dev_set_prep with no_pairing = 1 first): H2D + device preparation are queued and the call
 * returns; the histogram kernel follows once the preparation has reported the longest admitted read (which sizes the histogram rows
 * kept in LDS) -- at the next submit on another slot, at md_dev_slot_sync or at md_dev_mbias_read, whichever comes first.  The ranges
 * must stay valid until md_dev_slot_sync(slot) or the next submit on that slot returns; MDK_ERR_PREP_HOST is not possible here (no
 * pairing). */
int  md_dev_mbias_submit_raw(md_dev *h, int slot, const md_raw_batch *b);
int  md_dev_mbias_read(md_dev *h, md_mbias *out);
int  md_dev_mbias_reset(md_dev *h);
int  md_dev_slot_sync(md_dev *h, int slot);
/* Group launches (k_mbias_multi): up to md_dev_group_max() slots, each freshly uploaded with md_dev_upload_raw / _inplace (md_dev_set_prep with
 * no_pairing first, the contigs' references resident), get their preparation and their histogram with one launch per kernel on the first
 * slot's stream (with CHG or CHH on, the histogram gets one launch per chunk instead, queued by the same call: eight dense chunks in one launch
 * were measured slower).  The call queues and returns: the host does not wait between preparation and histogram kernel -- how many histogram rows a
 * chunk keeps in LDS, and whether it may count at all, the kernel reads from the chunk's status block on the device.  A chunk adds its counts
 * exactly once: one whose preparation did not end cleanly, or whose longest admitted read has more positions than the histogram has rows, adds
 * nothing and says so in its status.  md_dev_mbias_collect(the same slots) waits for the launch; rc[i] is 0 or what the chunk's preparation
 * reported (MDK_ERR_PREP_HOST: prepare it on the host and give it to md_dev_mbias_submit; MDK_ERR_STRAND0; MDK_ERR_ARG for a malformed record),
 * and the chunks the device skipped for want of room go through the single-chunk path there and then (their preparation again, the histogram
 * grown with the device drained, k_mbias), so the records must stay valid until it returns.  md_dev_mbias_redone: how many chunks that were,
 * since the last reset / md_dev_bias_finish.  md_dev_mbias_group and md_dev_mbias_collect may be called by two threads (one each). */
int  md_dev_mbias_group(md_dev *h, const int *slots, int n);
int  md_dev_mbias_collect(md_dev *h, const int *slots, int n, int *rc);
int  md_dev_mbias_redone(const md_dev *h);

/* The methylation-bias table on the device (csrc/mdk_bias.hip): what a resident session returns for an `mbias` run.  md_dev_bias_finish waits
 * for every histogram kernel (MDK_ERR_STRAND0 as md_dev_mbias_read) and turns the histogram into a md_bias_set (k_bias_rows):
 *   - the rows of the command's table in the order it prints them (strand OT, OB, CTOT, CTOB; ascending position; read 1 then read 2; only
 *     where nmeth || nunmeth): MD_BIAS_STRAND int8 0..3, MD_BIAS_READ int8 1|2, MD_BIAS_POS int32 1-based, MD_BIAS_NMETH / MD_BIAS_NUNMETH int64;
 *   - MD_BIAS_COUNTS: the dense histogram, int64 [len][4][2][2] (position, strand, read, methylated/unmethylated), len = the longest admitted read;
 *   - the histogram on the host (md_bias_set_hist: memory of the set), from which the caller computes the inclusion bounds.
 * The set owns its device memory at its exact size, independent of the handle (it may outlive it), until md_bias_set_free.  The handle's
 * histogram stays as it is (md_dev_reset / md_dev_mbias_reset drop it). */
typedef struct md_bias_set md_bias_set;
enum { MD_BIAS_STRAND = 0, MD_BIAS_READ, MD_BIAS_POS, MD_BIAS_NMETH, MD_BIAS_NUNMETH, MD_BIAS_COUNTS };
int  md_dev_bias_finish(md_dev *h, md_bias_set **out);
int64_t md_bias_set_count(const md_bias_set *b);          /* rows */
int  md_bias_set_len(const md_bias_set *b);               /* positions of the dense histogram */
int  md_bias_set_redone(const md_bias_set *b);            /* chunks of the run that went through the single-chunk path after a group launch */
int  md_bias_set_hist(const md_bias_set *b, md_mbias *out);
/* synchronous copy of one column (count entries; MD_BIAS_COUNTS: 16 * len) into DEVICE memory of the set's device (to_host = 0) or host memory */
int  md_bias_set_copy(const md_bias_set *b, int column, void *dst, int to_host);
void md_bias_set_free(md_bias_set *b);

/* perRead (perRead.c): per-read CpG methylation.  One md_pr_read per alignment the command keeps (start inside the chunk,
 * -F/-R/-q passed), in file order; `cigar` holds the BAM CIGAR words of all reads back to back (cig_off/n_cigar index it);
 * the payload in `blob` is laid out as for md_read_batch (4*off4: seq nibbles padded to 4 bytes, then qualities).
 * Replaces processRead (perRead.c:38-94) for every read of a chunk; counts[i] belongs to read[i].
 * The reference must be resident WITHOUT md_dev_set_regions: perRead uses -l only to pass over whole chunks. */
typedef struct { int32_t pos; uint32_t off4, l_qseq, cig_off; uint16_t n_cigar; uint8_t strand, reserved; } md_pr_read;
typedef struct { int32_t tid; int64_t beg, end; int32_t n_reads; const md_pr_read *read; const uint32_t *cigar; uint64_t n_cigar;
                 const uint8_t *blob; uint64_t blob_bytes; } md_pr_batch;
typedef struct { uint32_t nmeth, nunmeth; } md_pr_count;
int  md_dev_perread_submit(md_dev *h, int slot, const md_pr_batch *b);                 /* H2D + kernel + D2H enqueued on the slot's stream */
int  md_dev_perread_download(md_dev *h, int slot, const md_pr_count **counts, int64_t *n);   /* waits; memory owned by the slot */
/* the same from the chunk's raw records (md_dev_set_prep with perread = 1): the device selects the reads (kept[i] = index into
 * the batch's rec_off of the i-th kept read, ascending) and walks them; n kept reads, counts[i] belongs to kept[i] */
int  md_dev_perread_submit_raw(md_dev *h, int slot, const md_raw_batch *b);
int  md_dev_perread_download_raw(md_dev *h, int slot, const uint32_t **kept, const md_pr_count **counts, int64_t *n);

/* slot in [0, n_slots): upload is H2D on the slot's stream; launch enqueues the kernels; download waits for
 * the slot and returns the sites.  md_dev_submit = upload + launch. */
int  md_dev_upload(md_dev *h, int slot, const md_read_batch *b);
int  md_dev_launch(md_dev *h, int slot);
int  md_dev_submit(md_dev *h, int slot, const md_read_batch *b);
/* One launch of each kernel over several uploaded slots (at most md_dev_group_max() = 8, all different): a 1 Mb chunk alone is
 * fewer than two workgroups per CU, so chunks are launched together -- the preparation kernels of the slots uploaded with
 * md_dev_upload_raw (queued here, not at upload) and the pileup; each chunk keeps its own reads, outputs and site counter, and
 * download / wait are per slot as after md_dev_launch. */
int  md_dev_launch_group(md_dev *h, const int *slots, int n);
int  md_dev_group_max(void);
int  md_dev_download(md_dev *h, int slot, md_sites *out);
/* md_dev_download for the slots of ONE md_dev_launch_group, with one wait and one round of copies for all of them instead of one per slot:
 * rc[i] is what md_dev_download(slots[i]) would have returned (0, MDK_ERR_PREP_HOST, MDK_ERR_STRAND0, ...) and out[i] its sites.  Returns 0 when
 * the collection itself worked, whatever the rc[i]. */
int  md_dev_download_group(md_dev *h, const int *slots, int n, md_sites *out, int *rc);
int  md_dev_sync(md_dev *h);

/* Make the kernels of `slot` write their result into caller-provided DEVICE buffers (e.g. torch tensors that are
 * then exchanged over RCCL) instead of library memory: d_site[cap_sites] (md_site), d_var[cap_sites] (md_site_var,
 * may be NULL when minOppositeDepth == 0), d_seg[cap_tiles] (md_tile_seg).  Pass all-NULL to unbind.
 * md_dev_wait then reports how many slots/tiles were used; MDK_ERR_ARG if a capacity was too small (cap_sites must
 * be at least the number of kept context positions of the interval; the interval length always suffices). */
int  md_dev_bind_output(md_dev *h, int slot, void *d_site, void *d_var, void *d_seg, int64_t cap_sites, int64_t cap_tiles);
/* wait for the slot's kernels; fills the device view (library or bound buffers) */
int  md_dev_wait(md_dev *h, int slot, md_sites_dev *out);
/* host-side helper: put a segmented result (copied to host memory, n_slots slots) into ascending order;
 * returns the number of sites written to out_site (>= 0) or a negative error */
int64_t md_sites_order(const md_site *site, const md_site_var *var, const md_tile_seg *seg, int32_t n_tiles, int64_t n_slots,
                       md_site *out_site, md_site_var *out_var);

/* ---- calls on the device (a resident extract session: include/mdk_extract.h mdk_session_*) ----
 * What the text post-pass (csrc/host/mdk_emit.c emit_format) makes of a chunk's sites -- the variant filter, --mergeContext, the depth
 * test, the contexts switched on -- done on the device (k_calls_compact), and the rows kept there as columns instead of printed:
 *   start, end  (int32)  bedGraph columns 2 and 3: end = start + 1, or + 2 / + 3 for a merged CpG / CHG row
 *   nmeth, nunmeth (int32)
 *   context     (uint8)  0 CpG, 1 CHG, 2 CHH
 *   strand      (int8)   +1 a C, -1 a G, 0 a --mergeContext CpG / CHG row (keyed at its C, whichever members survived)
 *   contig      (int32)  the chunk's tid (BAM header order)
 * Rows come in schedule order of the chunks (the keys given to md_dev_calls_group) and, within a chunk, in the order of the sites that
 * make them: for each context that is ascending `start`, exactly the order of that context's bedGraph lines.  --cytosine_report rows are
 * not made here.
 * Sequence: md_dev_calls_begin, then for every collected group md_dev_calls_group in place of md_dev_download_group (a slot answered
 * with MDK_ERR_PREP_HOST is prepared on the host, submitted again and passed to md_dev_calls_group alone, with its key), then
 * md_dev_calls_finish.  Between begin and finish, group launches leave their sites on the device (no copy to pinned host memory), so
 * md_dev_download_group must not be used on the handle meanwhile.  Single caller thread for the calls_* functions of a handle.
 * Ownership: the handle keeps a row arena and a tile table in device memory (plain hipMalloc, grown by doubling, kept until
 * md_dev_reset / md_dev_close); md_dev_calls_finish returns a md_calls_set that owns its own device memory, independent of the handle
 * (it may outlive it), until md_calls_set_free. */
typedef struct {
    int32_t min_depth;             /* -d, >= 1 */
    int32_t merge;                 /* --mergeContext */
    int32_t min_opposite_depth;    /* --minOppositeDepth (0: no variant filter; the handle's cfg.minOppositeDepth must match) */
    double  max_variant_frac;      /* --maxVariantFrac */
    int32_t ctx_on[3];             /* CpG, CHG, CHH rows wanted */
} md_calls_cfg;
typedef struct md_calls_set md_calls_set;
/* destination of md_calls_set_copy: n entries each; a NULL column is not copied */
typedef struct { int32_t *contig, *start, *end, *nmeth, *nunmeth; uint8_t *context; int8_t *strand; } md_calls_cols;
int  md_dev_calls_begin(md_dev *h, const md_calls_cfg *cfg);
/* waits for the group (as md_dev_download_group), reserves each chunk's room and queues k_calls_compact on the handle's own stream; the
 * slots' streams wait for it before their next work.  keys[i]: the chunk's place in the output order (its schedule index).  rc[i]: what
 * md_dev_download would have returned for slots[i] (0, MDK_ERR_PREP_HOST, MDK_ERR_STRAND0, ...); only rc 0 chunks are compacted.
 * Returns 0 when the collection itself worked. */
int  md_dev_calls_group(md_dev *h, const int *slots, const uint32_t *keys, int n, int *rc);
/* waits for every compaction, closes the gaps between the chunks' reservations (k_calls_gather) and hands the rows over */
int  md_dev_calls_finish(md_dev *h, md_calls_set **out);
int64_t md_calls_set_count(const md_calls_set *c);
/* synchronous copies of the columns into DEVICE memory of the set's device (to_host = 0) or host memory (to_host = 1) */
int  md_calls_set_copy(const md_calls_set *c, const md_calls_cols *dst, int to_host);
void md_calls_set_free(md_calls_set *c);

/* ---- reads on the device (a resident perRead session: include/mdk_extract.h mdk_session_perread) ----
 * The rows `perRead` prints (addRead, perRead.c:16-36), kept as columns instead of text:
 *   contig (int32) the chunk's tid; pos (int32) the record's pos; nmeth, nunmeth (int32) the read's CpG calls;
 *   name_off (int64, n + 1 entries, the first 0) and name bytes (uint8): the read names back to back, each the record's l_read_name
 *   bytes up to the first NUL (what %s prints).
 * Rows come in the order of the calls below, which the caller makes in schedule order; within a device-selected chunk, the kept reads
 * in file order.
 * Sequence: md_dev_reads_begin; then per chunk either
 *   - md_dev_perread_submit_raw + md_dev_reads_slot (queued on the slot's stream behind k_perread_raw, no host wait), later
 *     md_dev_reads_collect, which waits for the slot and appends its rows.  Between begin and finish md_dev_perread_submit_raw copies
 *     nothing of the reads back (md_dev_perread_download_raw must not be used); or
 *   - md_dev_reads_host for a chunk whose reads the host listed (counts NULL: all zero);
 * then md_dev_reads_finish.  Single caller thread for the reads_* functions of a handle.
 * Ownership: the handle keeps a row arena and per-slot staging in device memory (grown by doubling, kept until md_dev_reset /
 * md_dev_close); md_dev_reads_finish returns a md_reads_set that owns its device memory at its exact size, independent of the handle
 * (it may outlive it), until md_reads_set_free. */
typedef struct md_reads_set md_reads_set;
/* destination of md_reads_set_copy: n entries each (name_off: n + 1, name_bytes: md_reads_set_name_bytes); a NULL column is not copied */
typedef struct { int32_t *contig, *pos, *nmeth, *nunmeth; int64_t *name_off; uint8_t *name_bytes; } md_reads_cols;
int  md_dev_reads_begin(md_dev *h);
/* after md_dev_perread_submit_raw on `slot`: the kept reads' name lengths and their scan, queued on the slot's stream */
int  md_dev_reads_slot(md_dev *h, int slot);
/* waits for the slot; appends its rows (its kept reads, their counts and names) to the run's rows; *n: how many.  Returns what
 * md_dev_perread_download_raw would have returned (MDK_ERR_ARG for a malformed record: nothing is appended then). */
int  md_dev_reads_collect(md_dev *h, int slot, int64_t *n);
/* n reads of contig tid listed by the host: pos[i], counts[i] (NULL: no calls), name i = names[name_off[i] .. name_off[i + 1]) */
int  md_dev_reads_host(md_dev *h, int32_t tid, int64_t n, const int32_t *pos, const md_pr_count *counts, const uint64_t *name_off, const uint8_t *names);
int  md_dev_reads_finish(md_dev *h, md_reads_set **out);
int64_t md_reads_set_count(const md_reads_set *r);
int64_t md_reads_set_name_bytes(const md_reads_set *r);
/* synchronous copies of the columns into DEVICE memory of the set's device (to_host = 0) or host memory (to_host = 1) */
int  md_reads_set_copy(const md_reads_set *r, const md_reads_cols *dst, int to_host);
void md_reads_set_free(md_reads_set *r);

/* ---- the cytosine report on the device (a resident session: include/mdk_extract.h mdk_session_cytosines) ----
 * What `extract --cytosine_report` prints (csrc/host/mdk_emit.c emit_format + put_blanks), kept as columns: one row for EVERY cytosine of the
 * reference in the contexts switched on, covered or not, inside the chunks the caller names --
 *   contig (int32) the chunk's tid; pos (int32) 1-BASED, the line's column 2; strand (int8) +1 a C, -1 a G; nmeth, nunmeth (int32), 0 where the
 *   position has no site or its site is dropped by the variant filter (no depth test: -d does not apply to this format); context (uint8)
 *   0 CpG, 1 CHG, 2 CHH; trinucleotide (uint8 x 3) the line's column 7: 'C' and the two following bases, for a G of the reverse complement,
 *   each of ACGT after case folding or 'N' (anything else, and anything past a contig end).
 * Rows come in the order of the chunks' keys and ascending position inside a chunk.  Which rows there are depends on the contig's BASES, the
 * contexts and the chunks alone (the context codes md_dev_set_regions masked are not used): two runs over the same reference and
 * schedule give columns that line up row for row, whatever their reads.
 * Sequence: md_dev_cytosines_begin; for every collected group md_dev_cytosines_group in place of md_dev_download_group; md_dev_cytosines_finish.
 * As with the calls, group launches leave their sites on the device meanwhile.  Single caller thread for these functions of a handle.
 * Sizing: a chunk's row count is not bounded by anything the slot knows, so it is COUNTED first (k_cyto_count over the bases of the group's
 * chunks, queued before the wait for the group and read back after it), the run's arena is reserved for exactly that many rows more, and
 * k_cyto_fill writes them.  Ownership as for the calls: the handle keeps the arena (grown by doubling, kept until md_dev_reset /
 * md_dev_close); md_dev_cytosines_finish returns a set that owns its device memory at its exact size until md_cytosines_set_free. */
typedef struct {
    int32_t min_opposite_depth;    /* --minOppositeDepth (0: no variant filter; the handle's cfg.minOppositeDepth must match) */
    double  max_variant_frac;      /* --maxVariantFrac */
    int32_t ctx_on[3];             /* CpG, CHG, CHH rows wanted */
} md_cyto_cfg;
/* one chunk of the schedule: its place in the output order, its contig (reference resident) and [beg, end); rows stop at the contig's end */
typedef struct { uint32_t key; int32_t tid; int64_t beg, end; } md_cyto_chunk;
typedef struct md_cytosines_set md_cytosines_set;
/* destination of md_cytosines_set_copy: n entries each (trinucleotide: 3 n bytes); a NULL column is not copied */
typedef struct { int32_t *contig, *pos; int8_t *strand; int32_t *nmeth, *nunmeth; uint8_t *context, *trinucleotide; } md_cytosines_cols;
int  md_dev_cytosines_begin(md_dev *h, const md_cyto_cfg *cfg);
/* n <= md_dev_group_max() chunks.  slots[i] >= 0: the launched slot that holds chunk i (same contig and interval) -- waited for as
 * md_dev_download_group waits, rc[i] what md_dev_download would have returned; only rc 0 chunks get rows (one answered with MDK_ERR_PREP_HOST
 * is prepared on the host, submitted again and passed here alone).  slots[i] < 0: a chunk of the schedule that produced no launched slot:
 * every row of it has zero counts, rc[i] = 0.  Returns 0 when the collection itself worked. */
int  md_dev_cytosines_group(md_dev *h, const int *slots, const md_cyto_chunk *chunks, int n, int *rc);
/* waits for every fill, puts the chunks in key order (k_cyto_gather) and hands the rows over */
int  md_dev_cytosines_finish(md_dev *h, md_cytosines_set **out);
int64_t md_cytosines_set_count(const md_cytosines_set *c);
/* synchronous copies of the columns into DEVICE memory of the set's device (to_host = 0) or host memory (to_host = 1) */
int  md_cytosines_set_copy(const md_cytosines_set *c, const md_cytosines_cols *dst, int to_host);
void md_cytosines_set_free(md_cytosines_set *c);

/* ---- text on the device: the lines of `extract`'s and `perRead`'s files from columns (csrc/mdk_text.hip, csrc/mdk_text_core.h) ----
 * A renderer turns rows held as DEVICE-resident columns in the layouts above (md_calls_cols, md_cytosines_cols, md_reads_cols: a session's result, or any
 * arrays of those types -- filtered, re-ordered, concatenated) into the bytes csrc/host/mdk_emit.c put_site prints for them:
 *   MD_TEXT_BEDGRAPH   chrom start end (int)(100 m / cov) m u        MD_TEXT_FRACTION   chrom start end %f of m / cov
 *   MD_TEXT_COUNTS     chrom start end cov                           MD_TEXT_METHYLKIT  chrom.start+1 chrom start+1 F|R cov %6.2f %6.2f
 *   MD_TEXT_CYTOSINE_REPORT (md_text_measure_cytosines)  chrom pos +|- m u CG|CHG|CHH trinucleotide
 *   MD_TEXT_PERREAD (md_text_measure_reads)  name chrom pos V cov, as csrc/host/mdk_cmd_perread.c prints a read: cov = m + u, V = %f of
 *                      100 m / cov, or the characters 0.0 when cov == 0.  Every row has a line, covered or not
 * byte for byte what the command writes, %f and %6.2f included (exact, from integer arithmetic).  --logit has no format here: its value goes
 * through log(), which neither glibc nor the device library rounds correctly, so equal bytes cannot be promised.  Headers are not written.
 * A renderer belongs to a device and a contig name table (copied to the device once, by md_text_open; a name longer than 255 bytes is refused
 * with MDK_ERR_ARG -- the command's cut of a line at 10000 bytes is not reproduced).  Two steps per range of rows [r0, r1), at most 2^30 rows:
 *   md_text_measure_*  the length of every row's line, scanned; *bytes = the size of the text.  `context` 0 / 1 / 2: rows of other contexts give
 *                      no line (-1: every row); in the four call formats a row with nmeth + nunmeth == 0 gives none either (the command prints
 *                      none).  MDK_ERR_ARG, with md_dev_last_error, for a contig index outside the name table, a MD_TEXT_METHYLKIT row with
 *                      strand 0 (a --mergeContext row: the command refuses that combination) or a report row whose context is above 2;
 *   md_text_measure_reads  the same for rows [r0, r1) of md_reads_cols, whose name_off holds at least r1 + 1 entries and whose name_bytes holds
 *                      n_name_bytes bytes.  MDK_ERR_ARG for a contig index outside the name table, a name offset outside [0, n_name_bytes],
 *                      offsets that decrease inside the range, or a name longer than 255 bytes: no name is read before these are checked;
 *   md_text_fill       the text of the range measured last into `dst`, DEVICE memory of exactly *bytes bytes (any alignment).  Columns that
 *                      changed since the measure are detected per workgroup and end the call with MDK_ERR_ARG; nothing is written past dst.
 * Both work on the renderer's own stream and are synchronous: the columns must be complete when md_text_measure_* is called (a caller that
 * filled them on a stream of its own waits for that stream first), and dst holds the text when md_text_fill returns.  One thread at a time
 * per renderer.  The renderer owns the name table and a table of one entry per 256 rows, until md_text_close.
 *   md_text_gather_names  the ragged gather of read names (no text): name index[i] of the source -- src_bytes[src_off[j] .. src_off[j + 1]),
 *                      n_src names in n_src_bytes bytes -- to dst_bytes[dst_off[i] .. dst_off[i + 1]) for i in [0, n).  index has n int64
 *                      entries in any order, repeats allowed; dst_off has n + 1 entries, the scan of the selected lengths, made by the
 *                      caller; every array is DEVICE memory.  Same stream, same rules.  MDK_ERR_ARG for an index outside [0, n_src), source
 *                      offsets as refused above, or destination offsets that are not that scan inside [0, n_dst_bytes]; a workgroup with
 *                      such a row writes nothing, and nothing is read or written outside the arrays. */
#ifndef MD_TEXT_FORMATS
#define MD_TEXT_FORMATS
enum { MD_TEXT_BEDGRAPH = 0, MD_TEXT_FRACTION, MD_TEXT_COUNTS, MD_TEXT_METHYLKIT, MD_TEXT_CYTOSINE_REPORT, MD_TEXT_PERREAD, MD_TEXT_N_FORMATS };
#endif
typedef struct md_text md_text;
int  md_text_open(int device, int32_t n_contigs, const char *const *names, md_text **out);
int  md_text_measure_calls(md_text *t, const md_calls_cols *cols, int64_t r0, int64_t r1, int fmt, int context, int64_t *bytes);
int  md_text_measure_cytosines(md_text *t, const md_cytosines_cols *cols, int64_t r0, int64_t r1, int context, int64_t *bytes);
int  md_text_measure_reads(md_text *t, const md_reads_cols *cols, int64_t n_name_bytes, int64_t r0, int64_t r1, int64_t *bytes);
int  md_text_fill(md_text *t, void *dst, int64_t bytes);
int  md_text_gather_names(md_text *t, const int64_t *src_off, const uint8_t *src_bytes, int64_t n_src, int64_t n_src_bytes,
                          const int64_t *index, int64_t n, const int64_t *dst_off, uint8_t *dst_bytes, int64_t n_dst_bytes);
void md_text_close(md_text *t);

/* ---- mergeContext on the device: per-strand rows folded into per-CpG / per-CHG rows (csrc/mdk_merge.hip, csrc/mdk_merge_core.h) ----
 * What the `mergeContext` command does to the lines of a bedGraph, done to rows held as DEVICE-resident md_calls_cols -- which carry the
 * context and the strand the command looks up in the FASTA.  The n rows must be strictly ascending in (contig, start), each one cytosine:
 * end == start + 1, strand +1 (a C) or -1 (a G), context 0 / 1 / 2.  With d = context + 1:
 *   context 2             the row as it is, strand kept;
 *   context < 2, a C at p (contig, p, p + d + 1, its counts plus those of the next row if that is the G of the same contig and context at p + d,
 *                         context, strand 0), at the C's place;
 *   context < 2, a G at q no row if the row before it is its C; otherwise (contig, q - d, q + 1, its counts, context, 0);
 * and a row whose nmeth + nunmeth < min_depth is dropped (min_depth 0: none is).  Two steps on a renderer (its stream, its table of one entry
 * per 256 rows, its contig count; the same rules: synchronous, one thread at a time, the columns complete when the call is made):
 *   md_text_merge_measure  *rows = the number of rows of the result.  n at most 2^30.  MDK_ERR_ARG, with md_dev_last_error naming it, for a
 *                          CpG / CHG row with strand 0 or a row with end != start + 1 (merged already), a context above 2, a contig index
 *                          outside the name table, rows not strictly ascending, a G without its C at q < d, counts that add up to more than
 *                          INT32_MAX.  A measure of either kind voids the renderer's earlier one: there is one table;
 *   md_text_merge_fill     the seven columns of the result into `dst`, DEVICE memory of the caller of exactly *rows entries each, apart from
 *                          the measured columns.  Columns that changed since the measure are detected per workgroup and end the call with
 *                          MDK_ERR_ARG; nothing is written past dst. */
int  md_text_merge_measure(md_text *t, const md_calls_cols *cols, int64_t n, int32_t min_depth, int64_t *rows);
int  md_text_merge_fill(md_text *t, const md_calls_cols *dst, int64_t rows);

/* ---- sums over intervals: rows added up per island, promoter, candidate DMR or tile (csrc/mdk_regions.hip, csrc/mdk_region_core.h) ----
 * The n rows of DEVICE-resident md_calls_cols (n at most 2^30; `end` is not read and may be NULL) must be strictly ascending in (contig,
 * start).  The k intervals (k at most 2^30) are three int32 DEVICE columns, half-open and 0-based as BED lines, in any order; they may
 * overlap, nest or repeat.  With lo_j the number of rows whose (contig, start) < (iv_contig[j], iv_start[j]) and hi_j the number whose
 * (contig, start) < (iv_contig[j], iv_end[j]), the rows of interval j are [lo_j, hi_j): a row belongs to the interval that holds its
 * start, a merged row wider than one base included, so the windows of a tiling count every row exactly once.  A row counts if bit `context`
 * of context_mask (3 bits) is set, its strand is allowed by strand_mask (bit 0: +1, bit 1: -1, bit 2: 0, a merged row) and nmeth + nunmeth,
 * formed in 64 bits, is at least min_depth (not negative).  Per interval, in the intervals' own order, into DEVICE memory of k entries each:
 * nsites (the rows counted), nmeth and nunmeth (their counts added, int64).  An empty interval and one without rows give zeros.
 * MDK_ERR_ARG, with md_dev_last_error naming it, for rows not strictly ascending, a row's contig outside the name table, a context above 2,
 * an interval's contig outside the name table, an interval with start < 0 or end < start; the contents of the outputs are unspecified
 * then, and nothing is written past them.  One call, synchronous on the renderer's stream, with the rules of the sections above (one thread
 * at a time, the columns complete when the call is made).  It keeps a table of its own on the renderer (20 bytes per 256 rows, until
 * md_text_close) and voids nothing: a text, merge or parse measure that waits for its fill on the same renderer stays valid. */
int  md_text_regions(md_text *t, const md_calls_cols *cols, int64_t n,
                     const int32_t *iv_contig, const int32_t *iv_start, const int32_t *iv_end, int64_t k,
                     uint32_t context_mask, uint32_t strand_mask, int32_t min_depth,
                     int32_t *nsites, int64_t *nmeth, int64_t *nunmeth);

/* ---- samples joined into one site table: methylKit's `unite` (csrc/mdk_unite.hip, csrc/mdk_unite_core.h) ----
 * n_samples (1 to 1024) tables of DEVICE-resident md_calls_cols, sample s of n_rows[s] rows (at most 2^30), each strictly ascending in
 * (contig, start), with starts that are not negative.  A row is present in its sample if nmeth + nunmeth, formed in 64 bits, is at least
 * min_depth (not negative; 0: every row is).  A site is a (contig, start) of which some sample holds a present row; the result is the
 * sites at least min_samples (1 to n_samples) samples hold, ascending in (contig, start), with every sample's counts.  No key per row
 * and no sort: the sites are the bits of a bitmap over the contigs' covered extents -- per contig the largest start + 1 of any sample,
 * rounded up to 32 --, a site's number is the rank of its bit.  Two steps on a renderer (its stream, its status block, its contig count;
 * the same rules: synchronous, one thread at a time, the columns complete when the call is made):
 *   md_text_unite_measure  *n_union = the sites of the union (what min_samples 1 would give), *n_out = the sites of the result.
 *                          MDK_ERR_ARG, with md_dev_last_error naming it, for rows of a sample not strictly ascending, a contig index
 *                          outside the name table, a context above 2, a negative start, covered extents that add up to more than 2^35
 *                          bits (refused before the bitmap is allocated), more than 2^30 sites in the union.  The samples' columns must
 *                          stay alive and unchanged until the fill.  Temporaries, kept on the renderer until md_text_close: the extents
 *                          / 4 bytes (bitmap and ranks) and 12 bytes per site of the union;
 *   md_text_unite_fill     into DEVICE memory of the caller: contig, start, end, context, strand and nsamples (the samples that hold the
 *                          site) of n_out entries, nmeth and nunmeth of n_samples x n_out entries, sample-major -- row s is sample s --,
 *                          which the call sets to zero first: a sample that does not hold a site has 0 0 there.  n_out must be the
 *                          measured number.  The site's end, context and strand are those of one of the samples' rows, and every other
 *                          present row of the site is compared with them: MDK_ERR_ARG "samples disagree about a site" for a difference
 *                          (tables made against one reference never differ).  Columns that changed since the measure end the call with
 *                          MDK_ERR_ARG or give other numbers; nothing is written outside the outputs.
 * The tables are this section's own: a text, merge or parse measure that waits for its fill on the same renderer stays valid. */
int  md_text_unite_measure(md_text *t, const md_calls_cols *samples, int32_t n_samples, const int64_t *n_rows, int32_t min_samples, int32_t min_depth,
                           int64_t *n_union, int64_t *n_out);
int  md_text_unite_fill(md_text *t, int32_t *contig, int32_t *start, int32_t *end, uint8_t *context, int8_t *strand, int32_t *nsamples,
                        int32_t *nmeth, int32_t *nunmeth, int64_t n_out);

/* ---- two groups compared: Fisher's exact test of two groups of samples, site by site (csrc/mdk_diff.hip, csrc/mdk_diff_core.h) ----
 * nmeth and nunmeth are two DEVICE matrices of n_samples x n entries, sample-major and contiguous -- row s is sample s, as
 * md_text_unite_fill writes them --, of int32 (elem_bytes 4) or int64 (elem_bytes 8: sums of md_text_regions stacked); n at most 2^30,
 * n_samples 1 to 1024.  group holds n_samples DEVICE marks: 0 the sample is in group A, 1 in group B, -1 not used; each group needs a
 * sample.  Per site i the entries of each group are added in 64 bits into nmeth_a, nunmeth_a, nmeth_b, nunmeth_b (a, b, c, d), and
 *   meth_diff[i] = 100.0 * (double(c) / double(c + d) - double(a) / double(a + b)), B minus A; 0.0 where a group has no coverage
 *   pvalue[i]    = the two-sided p-value of Fisher's exact test of the table (a b / c d): the weight of the tables with its margins that
 *                  are no likelier than it (at most 1 + 1e-7 times as likely: the tie rule of R and scipy) over the weight of all.  1.0
 *                  where only one table has the margins (a group without coverage is such a site); 0.0 where the table is less than
 *                  2^-960 as likely as the likeliest, which puts the p-value below 1e-280
 * by the rule csrc/mdk_diff_core.h states in full: IEEE doubles, a multiplication and a division per table of the support, added in a
 * fixed order, no lgamma, log or exp -- so the bits are those of a host build of that header (tools/diff_emu), on any device, whatever lane
 * a site runs on.  MDK_ERR_ARG, with md_dev_last_error naming the condition and the first site that has it, for an entry that is negative,
 * an entry of 2^26 or more and a pooled margin (a + b, c + d, a + c, b + d) of 2^26 or more; also for a mark other than -1, 0 and 1 and a
 * group without a sample.  The outputs hold no result then; nothing is written outside them, and the inputs are only read.  One call,
 * synchronous on the renderer's stream, with the rules of the sections above (one thread at a time, the matrices complete when the call is
 * made).  It keeps nothing on the renderer and voids nothing: a text, merge, parse or unite measure that waits for its fill stays valid.
 * Not here: one-sided tests, more than two groups, a model of the replicates' over-dispersion (logistic regression), and any p-value
 * that needs lgamma. */
int  md_text_diff(md_text *t, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n, const int32_t *group,
                  int64_t *nmeth_a, int64_t *nunmeth_a, int64_t *nmeth_b, int64_t *nunmeth_b, double *meth_diff, double *pvalue);

/* ---- sites joined into regions: significant neighbouring rows of a comparison chained into DMRs (csrc/mdk_dmr.hip, csrc/mdk_dmr_core.h) ----
 * The n rows (at most 2^30) are DEVICE columns, strictly ascending in (contig, start): contig, start, end (int32), the groups' pooled
 * counts nmeth_a, nunmeth_a, nmeth_b, nunmeth_b (a, b, c, d: int64, as md_text_diff writes them) and `significant` (uint8; nonzero: the
 * caller calls the row significant).  context and strand are a comparison's other two columns: they are not read and may be NULL.  No
 * double of the rows is read.  dir(i) = the sign of c (a + b) - a (c + d), +1 where group B is the more methylated.  A row is a CANDIDATE
 * if it is significant, a + b > 0, c + d > 0 and dir != 0.  With p the candidate before candidate i, i continues p's region iff
 * contig[i] == contig[p], dir(i) == dir(p), start[i] - start[p] <= max_gap (bases) and i - p - 1 <= max_skip (rows that are no
 * candidates between them); otherwise i begins a region, as the first candidate does.  A region runs from its first candidate f to its
 * last l and reports contig[f], start[f], end[l], nsites = l - f + 1 (every row of the span), nsig (its candidates), direction = dir(f),
 * the sums of the four counts over ALL rows f .. l, and meth_diff and pvalue of these four sums exactly as md_text_diff gives them.  It is
 * kept iff nsig >= min_sites, |meth_diff| >= min_diff and the sign of the pooled c (a + b) - a (c + d) is its direction (pooled sums can
 * reverse the sign of every one of their rows; such a region is dropped).  max_gap >= 0, max_skip >= 0, min_sites >= 1, min_diff finite
 * and >= 0.  Two steps on a renderer (its stream and its status block; the same rules: synchronous, one thread at a time, the columns
 * complete when the call is made):
 *   md_text_dmr_measure  *n_regions = the kept regions.  MDK_ERR_ARG, with md_dev_last_error naming the condition and the first row that
 *                        has it, for rows not strictly ascending, a contig index outside 0 .. n_contigs - 1, a negative count, a count
 *                        of 2^26 or more; and, where no row is refused, for a region -- kept or not -- with a pooled margin (a + b, c + d,
 *                        a + c, b + d) of 2^26 or more, naming the region's first row.  The columns must stay alive until the fill.
 *                        Temporaries, kept on the renderer until md_text_close: 1 1/8 bytes per row, 56 per 256 rows, 48 per region
 *                        before the filter;
 *   md_text_dmr_fill     the twelve columns into DEVICE memory of the caller of n_regions entries each, in ascending order of the
 *                        regions.  n_regions must be the measured number: a fill without a measure, or with another count, is
 *                        MDK_ERR_ARG.  The rows a fill reads are the ones the measure chose: columns that changed since give other
 *                        numbers, never a read outside the n rows or a write outside the outputs.
 * The tables are this section's own: a text, merge, parse or unite measure that waits for its fill on the same renderer stays valid. */
int  md_text_dmr_measure(md_text *t, const int32_t *contig, const int32_t *start, const int32_t *end, const uint8_t *context, const int8_t *strand,
                         const int64_t *nmeth_a, const int64_t *nunmeth_a, const int64_t *nmeth_b, const int64_t *nunmeth_b, const uint8_t *significant,
                         int64_t n, int32_t n_contigs, int32_t max_gap, int32_t max_skip, int32_t min_sites, double min_diff, int64_t *n_regions);
int  md_text_dmr_fill(md_text *t, int32_t *contig, int32_t *start, int32_t *end, int32_t *nsites, int32_t *nsig, int8_t *direction,
                      int64_t *nmeth_a, int64_t *nunmeth_a, int64_t *nmeth_b, int64_t *nunmeth_b, double *meth_diff, double *pvalue, int64_t n_regions);

/* ---- text read back into columns: a bedGraph or a cytosine report parsed on the device (csrc/mdk_parse.hip, csrc/mdk_parse_core.h) ----
 * The way back from md_text_fill: `bytes` bytes of text in DEVICE memory become rows in the layouts above, without the host looking at a line.
 * A line starts at byte 0 and after every '\n' and ends before the next '\n' or at the end of the text; one '\r' before the '\n' is dropped; a
 * line that begins with `track` is skipped wherever it stands; every other line is a row.  A line is at most 512 bytes, its '\n' included.
 *   MD_PARSE_BEDGRAPH         chrom start end pct nmeth nunmeth, six fields separated by single tabs, into md_calls_cols.  chrom is looked up
 *                             in the renderer's names (a binary search per line; of equal names the first), the four numbers are 1 to 10 decimal
 *                             digits at most INT32_MAX, pct is not looked at.  end must be start + 1: per-cytosine files only.  The strand
 *                             (+1 a C, -1 a G) and the context (0 CpG, 1 CHG, 2 CHH) come from the contig's bases around start, by the rule of
 *                             the `mergeContext` command and of a session's own classification, so the contig must be resident:
 *   md_text_reference         copies the `len` bases of contig `contig` from HOST memory to the renderer's device, where they stay until they
 *                             are replaced, dropped (bases = NULL) or the renderer is closed.  Synchronous.  Case as in the FASTA.
 *   MD_PARSE_CYTOSINE_REPORT  chrom pos +|- nmeth nunmeth CG|CHG|CHH tri, seven fields, into md_cytosines_cols; pos stays 1-based and is at
 *                             least 1, tri is three letters of ACGTN.  No reference is needed.
 * Stricter than the command on purpose: signs, blanks, doubled tabs, trailing columns and numbers past INT32_MAX, which its strtoll / strtok
 * take, are refused.  What is accepted gives, after md_text_merge_*, what the command prints for the file.  Two steps, with the rules of this
 * section -- synchronous on the renderer's stream, one thread at a time, the text complete when the call is made, a measure of any kind voids
 * the renderer's earlier one:
 *   md_text_parse_measure     *rows = the number of rows.  `text` is 16-byte aligned device memory, bytes at most 2^31 - 1.  Nothing is
 *                             validated yet;
 *   md_text_parse_fill_*      the seven columns into `dst`, DEVICE memory of exactly *rows entries each (3 * rows bytes of trinucleotide), the
 *                             one that matches the measured format.  Every line is validated here: MDK_ERR_ARG, with md_dev_last_error naming
 *                             the refusal of the offending line that starts earliest -- an empty line, too few / too many / empty fields, a
 *                             non-digit, an overflow, an unknown contig, end != start + 1, a position outside the contig, a base that is neither
 *                             C nor G, a bad strand / context / trinucleotide, a line longer than 512 bytes, a contig without resident bases --
 *                             and md_text_parse_error_offset giving that line's first byte (-1: none, or the text changed since the measure,
 *                             which is detected per 4096 bytes).  The contents of dst are unspecified then; nothing is written past dst. */
#ifndef MD_PARSE_FORMATS
#define MD_PARSE_FORMATS
enum { MD_PARSE_BEDGRAPH = 0, MD_PARSE_CYTOSINE_REPORT = 1 };
#endif
int  md_text_reference(md_text *t, int32_t contig, const char *bases, int64_t len);
int  md_text_parse_measure(md_text *t, const uint8_t *text, int64_t bytes, int fmt, int64_t *rows);
int  md_text_parse_fill_calls(md_text *t, const md_calls_cols *dst, int64_t rows);
int  md_text_parse_fill_cytosines(md_text *t, const md_cytosines_cols *dst, int64_t rows);
int64_t md_text_parse_error_offset(const md_text *t);

/* BGZF made on the device (csrc/mdk_deflate.hip, csrc/mdk_deflate_core.h): `n` bytes of DEVICE memory -- the text md_text_fill left there, or any
 * bytes -- compressed into complete BGZF members in device memory, so that a block of text crosses to the host once and compressed.  Member i holds
 * input bytes [65280 i, min(65280 (i + 1), n)), bgzip's cut: the 18-byte header (1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, "BC", BSIZE), one raw
 * RFC 1951 stream ending in a final block -- LZ77 matches (4 to 258 bytes, up to 32768 back) and Huffman codes fitted to the member (a dynamic block), or
 * a stored block where that is no larger --, CRC32 and ISIZE.  No member is longer than 65536 bytes or than its stored form, 18 + 5 + input + 8 bytes.
 * The bytes are a function of the input alone (tools/deflate_emu.cpp makes the same ones on the host); gzip, zcat, bgzip, tabix and R read them.
 * There are no compression levels.  Synchronous on the renderer's stream, one thread at a time, as the calls above:
 *   md_text_deflate_measure   compresses (n at most 2^31 - 1; the input must be complete when the call is made) and gives *out_bytes: the members'
 *                             lengths added up, plus the 28-byte EOF member if `eof` is not 0.  n == 0 gives the EOF member alone, or nothing;
 *   md_text_deflate_fill      the members back to back, then the EOF member, into DEVICE memory of exactly out_bytes bytes (any alignment).
 * The compressed members wait in memory of the renderer's between the two calls, 64 KiB per member, kept for the next call. */
int  md_text_deflate_measure(md_text *t, const uint8_t *d_in, int64_t n, int eof, int64_t *out_bytes);
int  md_text_deflate_fill(md_text *t, void *d_out, int64_t out_bytes);

/* An idle handle (nothing uploaded or launched that has not been collected) back to the state md_dev_open left it in, with `cfg`
 * (same n_slots and n_streams): contigs, -l runs, mappability tracks, the preparation settings, the mbias histogram, the calls and reads state
 * are dropped, every slot's buffers are given back.  Pointers the library returned for the handle before (md_sites, md_sites_dev,
 * md_mbias) are void afterwards; md_piece objects must have been destroyed first.  When no other handle is open, the carved device
 * memory is reused from its start (a handle used for run after run would otherwise keep taking more). */
int  md_dev_reset(md_dev *h, const md_dev_cfg *cfg);

/* Re-run the kernels of an uploaded slot `iters` times (inputs stay resident in HBM; results are identical
 * every time) and time them with HIP events on the slot's stream. */
int  md_dev_bench(md_dev *h, int slot, int warmup, int iters, md_bench_result *out);

/* The same for `n` uploaded slots holding DIFFERENT intervals, launched `per_launch` at a time (1 = md_dev_launch, more =
 * md_dev_launch_group; n must be a multiple) round robin on one stream, `iters` launches in all: with enough slots the
 * working set exceeds the 256 MiB Infinity Cache and every launch streams its inputs from HBM.  algo_bytes / n_sites /
 * n_tiles are per LAUNCH, averaged over the rotation; ms_total == ms_pileup. */
int  md_dev_bench_rotate(md_dev *h, const int *slots, int n, int per_launch, int warmup, int iters, md_bench_result *out);

/* ---- multi-GPU: the exchange step of the interval-sharded path (SURVEY.md 8b last row, 8e) ----
 * Chunk k of the reference's schedule belongs to GPU k mod N; per-interval site buffers travel to rank 0 (whose host writes
 * the files) with ncclSend/ncclRecv groups over xGMI -- a gather, never a reduction.  RCCL is loaded on first use.
 *   md_comm_open_rank   one process per GPU (torchrun-style launch, or the command's own ranks mode, csrc/host/mdk_ranks.c):
 *                       rank 0 makes an id, every rank gets it out of band
 * md_comm_gather: d_send/send_bytes have one entry (this rank's buffer), d_recv/recv_bytes are indexed by rank and only read
 * on rank 0 (entry 0 may be NULL to leave rank 0's own buffer where it is).  Sizes must agree on both sides.  Asynchronous:
 * the send buffers must be complete before the call, and md_comm_wait must return before either side is touched again. */
#define MD_COMM_ID_BYTES 128
typedef struct md_comm md_comm;
int  md_comm_unique_id(uint8_t *id /* [MD_COMM_ID_BYTES] */);
int  md_comm_open_rank(md_dev *h, int rank, int world, const uint8_t *id, md_comm **out);
/* one process per rank where ranks SHARE a physical device (tests of the multi-process path on a single GPU: RCCL refuses two ranks
 * on one device): no RCCL; rank 0's receive buffers are mapped into the peers with HIP IPC and a "send" is a device copy into the
 * mapping.  `oob` is the caller's out-of-band all-gather (every rank contributes `bytes` bytes, receives world*bytes in rank order;
 * bench.py gives torch.distributed over gloo), used to agree on sizes and to pass the IPC handles round.  Only md_bench_* uses such
 * a communicator. */
typedef int (*md_comm_oob_fn)(void *ctx, const void *send, void *recv, uint64_t bytes);
int  md_comm_open_rank_shared(md_dev *h, int rank, int world, md_comm_oob_fn oob, void *ctx, md_comm **out);
void md_comm_close(md_comm *c);
int  md_comm_world(const md_comm *c);
int  md_comm_gather(md_comm *c, const void *const *d_send, const uint64_t *send_bytes, void *const *d_recv, const uint64_t *recv_bytes);
int  md_comm_wait(md_comm *c);
/* One process per GPU (md_comm_open_rank): a finished chunk's result travels from the rank that computed it to rank 0, which writes the
 * files.  The sizes go first, out of band (the command's TCP connection between the ranks): md_comm_result_header waits for the slot's
 * kernels and describes what will be sent (rc = what md_dev_download would have returned: 0, MDK_ERR_PREP_HOST, MDK_ERR_STRAND0 ...);
 * md_comm_result_send then posts the ncclSend of the three arrays (site records, variant evidence, tile segments) and
 * md_comm_result_recv, on rank 0 with the header it was given, the matching ncclRecv, waits, copies to the host and orders the sites.
 * The returned arrays belong to the communicator and stay valid until the next md_comm_result_recv from the same rank. */
typedef struct { int64_t n_slots; int32_t n_tiles, variant, rc, reserved; } md_result_hdr;
int  md_comm_result_header(md_dev *h, int slot, md_result_hdr *hdr);
int  md_comm_result_send(md_comm *c, int slot, const md_result_hdr *hdr);
int  md_comm_result_recv(md_comm *c, int src, const md_result_hdr *hdr, md_sites *out);
/* PCI bus id of the handle's device ("0000:c1:00.0"): two ranks on the same physical device cannot be RCCL peers */
int  md_dev_pci_bus_id(const md_dev *h, char *buf, int cap);

/* The resident-input benchmark loop of bench.py: `n` uploaded slots holding different intervals are launched `group` at a
 * time (md_dev_launch_group; n a multiple of group, at least two groups) round robin, two launches in flight (launch g is
 * issued, then launch g-1 is collected, as extract_main does); the kernels write straight into a send buffer and, with a
 * communicator, the results of a launch travel to rank 0 in one exchange while the next launch is computed.
 * md_bench_run(launches): that many kernel launches.  md_bench_verify compares what the last launch left in the send buffer
 * with md_dev_download of the same intervals (and, on rank 0, checks that every peer's data arrived). */
typedef struct md_bench md_bench;
typedef struct { uint64_t launches, slots_last, exchanges, bytes_per_exchange; } md_bench_run_result;
int  md_bench_open(md_dev *h, md_comm *comm /* NULL: one GPU */, const int *slots, int n, int group, md_bench **out);
int  md_bench_run(md_bench *b, int64_t launches, md_bench_run_result *out);
/* on = 1 (default when the slots hold raw records): every launch of md_bench_run prepares its chunks again from their resident
 * records before the pileup -- the whole device work `extract` does per chunk; on = 0: the pileup alone over the resident segments */
int  md_bench_set_prep(md_bench *b, int on);
int  md_bench_verify(md_bench *b);
int64_t md_bench_region_bytes(const md_bench *b);
void md_bench_close(md_bench *b);

/* Test hook: effective (post-trim, post-overlap-resolution) base code and quality of every query base of
 * every read of an uploaded slot, written to host arrays laid out like the blob's qual/seq (one byte per
 * base, concatenated in read order; out_off[i] = start of read i). */
int  md_dev_debug_effective(md_dev *h, int slot, uint8_t *out_base, uint8_t *out_qual, const uint64_t *out_off);

/* Pinned host memory for staging buffers (so the C host never includes HIP headers). */
void *md_host_alloc(uint64_t bytes);
/* Pinning costs ~0.3 s per GB up front and again at process exit; a pageable buffer costs ~5 ms per 55 MB upload instead.
 * on = 0 makes later md_host_alloc calls return pageable memory (the host does this for inputs of a few dozen chunks). */
void  md_host_set_pinned(int on);
void  md_host_free(void *p);
/* what registering staging blocks has cost so far (seconds on the uploading threads, calls, bytes) */
void  md_host_profile(double *seconds, uint64_t *calls, uint64_t *bytes);
/* MDK_HOST_PROFILE=1: seconds and calls the host threads have spent inside the library per site (waiting for a slot, allocating, queueing
 * copies, launching, waiting for results, copying them back, ...), as one line of text */
int   md_dev_profile_text(char *buf, int cap);
/* a staging block is registered with the runtime (hipHostRegister) the first time an upload reads from it; a thread that has just FILLED
 * one may do that itself once a device is open (h: that device), so that the thread submitting uploads does not have to.  ptr: anywhere
 * inside the block */
void  md_host_register(md_dev *h, const void *ptr);
/* register every staging block that is not registered yet, with `threads` threads; returns how many there were.  For the moment the device
 * comes up: the blocks filled until then would otherwise be registered one by one by the thread that uploads from them */
int   md_host_register_all(md_dev *h, int threads);

#ifdef __cplusplus
}
#endif
#endif
