/*
 * mdk_extract.h -- C ABI of the host side of the MI355X `extract` path (libmdk_extract.so).
 *
 * Drop-in symbol (what the reference's main.c:18,49-50 binds):
 *     int extract_main(int argc, char *argv[]);            reference: extract.c:706
 * Same argv contract (argv[0] == "extract"), option surface, validation order, messages, output
 * file naming/format and return codes as the reference; the per-chunk work (extractCalls,
 * extract.c:247-560) runs on the GPU through include/mdk_hip.h.  There is no CPU fallback: without
 * a usable device extract_main prints the HIP error and returns -20.
 *
 * The staged API below exposes the same pipeline one reference chunk at a time (used by the
 * parity tests, bench.py and the multi-GPU sharded driver).
 */
#ifndef MDK_EXTRACT_H
#define MDK_EXTRACT_H
#include <stdint.h>
#include "mdk_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MDK_RC_NODEVICE (-20)   /* GPU path unavailable */
#define MDK_RC_DEVICE   (-21)   /* a device operation failed mid-run */
#define MDK_RC_OUTPUT   (-22)   /* writing an output file failed (message on stderr) */

int extract_main(int argc, char *argv[]);

typedef struct mdk_plan mdk_plan;
#define MDK_CHUNK_NOREF   1   /* contig missing from the FASTA -> the reference skips the chunk; nothing is emitted */
#define MDK_CHUNK_BED     4   /* -l: no BED region touches the chunk -> the reference passes it over (extract.c:352-369) */
#define MDK_CHUNK_FOREIGN 2   /* interval sharding: another rank owns this chunk; its sites arrive through the gather */

/* One chunk of the reference's schedule (extract.c:325-350 + adjustBounds) with its admitted reads packed
 * for the device.  `batch` arrays are owned by the plan and stay valid until the second-next
 * mdk_plan_next_chunk call (two rotating pinned buffers). */
typedef struct {
    uint32_t index;            /* localBin: output order */
    int32_t  tid;
    int64_t  beg, end;         /* [localPos, localEnd) */
    int32_t  skipped;          /* MDK_CHUNK_* flags; non-zero: nothing was packed for this chunk */
    md_read_batch batch;
    uint64_t n_records_seen;   /* BAM records examined for this chunk (before admission) */
    md_pr_batch pr;            /* perRead plans: the reads that start in the chunk (batch is unused then) */
    const void *host;          /* perRead plans: the plan's own record of those reads (names), for mdk_plan_emit_perread */
    int32_t  prep;             /* 1: device preparation -- `raw` describes the chunk's records for md_dev_submit_raw and `batch` is empty
                                  (until mdk_plan_host_prepare) */
    md_raw_batch raw;
} mdk_chunk;

/* Parse an `extract` command line (argv[0] = "extract"), open inputs.  rc follows extract_main:
 * *out is NULL with rc==0 when the command line only asked for help/version. */
int  mdk_plan_open(int argc, char *argv[], mdk_plan **out);
void mdk_plan_close(mdk_plan *p);
/* device configuration implied by the options */
void mdk_plan_dev_cfg(const mdk_plan *p, md_dev_cfg *cfg);
/* upload the contig a chunk needs (no-op if already resident on that device handle) */
int  mdk_plan_ensure_reference(mdk_plan *p, md_dev *dev, int32_t tid);
/* 1: chunk produced; 0: schedule finished; <0: error */
int  mdk_plan_next_chunk(mdk_plan *p, mdk_chunk *c);
/* the same without waiting: 2 (nothing handed out) when the next chunk of the schedule is not ready yet */
int  mdk_plan_try_next_chunk(mdk_plan *p, mdk_chunk *c);
/* Where a chunk's per-record work happens.  mode 0 (what mdk_plan_open gives): on the host -- chunks carry `batch`.
 * mode 1 (what the commands use): on the device -- chunks carry `raw`, and md_dev_set_prep must be given
 * mdk_plan_prep_cfg's configuration (plus md_dev_set_mappability per contig, done by mdk_plan_ensure_reference).
 * Must be called before the first mdk_plan_next_chunk.  mdk_plan_host_prepare fills `batch` of a mode-1 chunk after all
 * (for a chunk the device answered with MDK_ERR_PREP_HOST); valid until the second-next mdk_plan_next_chunk. */
int  mdk_plan_set_prep(mdk_plan *p, int mode);
/* how many of the chunks handed out last stay valid (default 2: a chunk's arrays live until the second-next
 * mdk_plan_next_chunk); a caller that keeps more chunks in flight (several GPUs) raises it first.  2..40. */
int  mdk_plan_set_hold(mdk_plan *p, int n);
void mdk_plan_prep_cfg(const mdk_plan *p, md_prep_cfg *cfg);
int  mdk_plan_host_prepare(mdk_plan *p, mdk_chunk *c);
/* the same when the chunk was uploaded to `slot` of `dev` and some of its records were inflated on the device (they are read back) */
int  mdk_plan_host_prepare_from(mdk_plan *p, mdk_chunk *c, md_dev *dev, int slot);
/* the host memory behind a mode-1 chunk's record ranges is no longer needed (its upload has completed: md_dev_upload_wait): the inflate
 * teams may reuse it now instead of when the chunk is recycled.  The chunk stays valid otherwise; mdk_plan_host_prepare_from then reads
 * all of its records back from the device. */
int  mdk_plan_release_records(mdk_plan *p, const mdk_chunk *c);
/* BGZF inflate of the plan's BAM on this device as well (include/mdk_hip.h md_piece_*): from now on pieces of the
 * file are inflated by whoever is free, a host inflate team or the device, and chunks may name device-resident ranges.  Only for
 * plans in device-preparation mode of the `extract` command; mdk_plan_detach_device must precede md_dev_close. */
int  mdk_plan_attach_device(mdk_plan *p, md_dev *dev);
void mdk_plan_detach_device(mdk_plan *p);
/* host post-pass for one chunk (variant filter, --mergeContext, formats; extract.c:443-510), appended to
 * the plan's output files.  Chunks must be emitted in index order. */
int  mdk_plan_emit(mdk_plan *p, const mdk_chunk *c, const md_sites *sites);
/* print the variant-position line (extract.c:1489), close outputs */
int  mdk_plan_finish(mdk_plan *p);
/* interval sharding over `world` processes (one per GPU): this process admits and packs only the chunks whose index
 * is congruent to `rank`; every process still walks the whole schedule, so chunk indices agree everywhere. */
int  mdk_plan_set_shard(mdk_plan *p, int rank, int world);
int  mdk_plan_n_targets(const mdk_plan *p);
/* -l: the disjoint runs (include/mdk_hip.h: md_region) the sites of a contig are restricted to, as handed to
 * md_dev_set_regions by mdk_plan_ensure_reference; *n = -1 when no BED file was given.  Replaces the cursor walk over
 * config->bed in extractCalls (extract.c:352-369,402-405; bed.c:22-53). */
int  mdk_plan_regions(const mdk_plan *p, int32_t tid, const md_region **runs, int64_t *n);
const char *mdk_plan_target_name(const mdk_plan *p, int32_t tid);
int64_t mdk_plan_target_len(const mdk_plan *p, int32_t tid);

/* ---- `mbias` (MBias.c; main.c:17,51-52 dispatches to mbias_main) ----
 * mbias_main: drop-in for the reference symbol (argv[0] = "mbias"); same options, messages, return codes, SVG / --txt
 * output and "Suggested inclusion options" line; -20/-21 when the GPU is unavailable/fails.
 * mdk_plan_open_mbias: the same plan object for an `mbias` command line: chunks come out of mdk_plan_next_chunk with
 * batches built WITHOUT mate pairing (mbias installs no overlap handler, MBias.c:158-161), to be fed to
 * md_dev_mbias_submit.  mdk_plan_mbias_outputs tells what the command line asked to be written (prefix is NULL with
 * --noSVG; which = keepCpG + 2 keepCHG + 4 keepCHH as passed to makeSVGs, MBias.c:556).
 * mdk_mbias_report: makeSVGs + makeTXT (svg.c:300-454) over the histogram the device returns. */
int  mbias_main(int argc, char *argv[]);
/* for a caller that leaves with _exit after one of the entry points has returned (the `MethylDackel` command): joins the thread that brings the
 * HIP runtime up and the device library's helper threads, so that none of them is inside the runtime when the process goes */
void mdk_cli_quiesce(void);
int  mdk_plan_open_mbias(int argc, char *argv[], mdk_plan **out);
int  mdk_plan_mbias_outputs(const mdk_plan *p, const char **opref, int *svg, int *txt, int *which);
int  mdk_mbias_report(const md_mbias *hist, const char *opref, int svg, int txt, int which);
/* the report's inclusion bounds on their own (getThresholds, svg.c:239-294): bounds[4 * strand + {0,1,2,3}] = read 1 left, right, read 2 left,
 * right and has[strand] = 1 for every strand (0..3 = OT, OB, CTOT, CTOB) that has a call -- the numbers mdk_mbias_report prints behind
 * "Suggested inclusion options:" when it draws the plots.  Returns 0, -1 for a bad argument. */
int  mdk_mbias_suggest(const md_mbias *hist, int bounds[16], int has[4]);

/* ---- `perRead` (perRead.c; main.c:20,55-56 dispatches to perRead_main) ----
 * perRead_main: drop-in for the reference symbol (argv[0] = "perRead").  mdk_plan_open_perread: chunks without
 * adjustBounds, `pr` filled with the alignments that start in the chunk and pass -F/-R/-q (perRead.c:178-183), for
 * md_dev_perread_submit; a chunk of a contig the FASTA lacks comes out with MDK_CHUNK_NOREF set AND its reads listed
 * (the reference prints them with zero calls).  mdk_plan_emit_perread writes addRead's lines (perRead.c:16-36) for a
 * chunk, in chunk order; counts may be NULL for a MDK_CHUNK_NOREF chunk. */
int  perRead_main(int argc, char *argv[]);
int  mdk_plan_open_perread(int argc, char *argv[], mdk_plan **out);
int  mdk_plan_emit_perread(mdk_plan *p, const mdk_chunk *c, const md_pr_count *counts, int64_t n);
/* the same for a chunk handed out as raw records (mdk_plan_set_prep(p, 1)): kept[i] = index into c->raw.rec_off of the i-th kept
 * read, counts[i] its calls (md_dev_perread_download_raw); names and positions are read from the records themselves */
int  mdk_plan_emit_perread_raw(mdk_plan *p, const mdk_chunk *c, const uint32_t *kept, const md_pr_count *counts, int64_t n);

/* Bind the calling thread, and every thread it creates from now on, to the CPUs next to the index-th AMD GPU (sysfs
 * local_cpulist, GPUs in PCI order), if that leaves at least half of the CPUs the process may use.  Returns the number of CPUs
 * bound to, 0 if nothing was changed (no such GPU, one NUMA node, MDK_NO_BIND set).  The `MethylDackel` command calls it for
 * its single-GPU commands; a library caller decides for itself.  No counterpart in the reference. */
int  mdk_bind_to_device_node(int index);

/* ---- a resident extract session: the calls as device-resident columns, one process across many runs ----
 * mdk_session_extract takes the argv of extract_main (argv[0] = "extract"), parses it with the same code and returns the same codes for
 * the same errors.  Instead of bedGraph files it returns the rows those files would hold (include/mdk_hip.h "calls on the device":
 * contig, start, end, nmeth, nunmeth, context, strand).  Differences from the command:
 *   - --fraction, --counts, --logit, --methylKit and --cytosine_report are refused with MDK_RC_UNSUPPORTED (the first four only shape text; the
 *     report's rows are another table: mdk_session_cytosines, below);
 *   - -o is ignored and no output file is written; -O / -N (writing a BBM file) behave as in the command;
 *   - MDK_RANK / MDK_WORLD are ignored: one device;
 *   - the process is never left through _exit, and the HIP runtime and the device handle stay up between runs (md_dev_reset before
 *     every run after the first: nothing of one run -- contigs, -l runs, mappability -- reaches the next).
 * Ownership and lifetimes: a session owns its device handle until mdk_session_close.  Each successful mdk_session_extract returns a new
 * mdk_calls (*out; NULL on error) that owns its rows in device memory and its contig names; it does not depend on the session and
 * stays valid, also after mdk_session_close, until mdk_calls_free.  The calls of one session must come from one thread at a time.
 * mdk_calls_contig_name's string belongs to the mdk_calls.  mdk_calls_copy is synchronous: `dst` (device memory of the session's device
 * when to_host = 0, host memory when 1) holds mdk_calls_count entries of the column's type when it returns. */
#define MDK_RC_UNSUPPORTED (-23)  /* an option a session does not take */
typedef struct mdk_session mdk_session;
typedef struct mdk_calls mdk_calls;
enum { MDK_CALLS_CONTIG = 0, MDK_CALLS_START, MDK_CALLS_END, MDK_CALLS_NMETH, MDK_CALLS_NUNMETH, MDK_CALLS_CONTEXT, MDK_CALLS_STRAND };   /* int32 x5, uint8, int8 */
int  mdk_session_open(int device, mdk_session **out);
int  mdk_session_extract(mdk_session *s, int argc, char *argv[], mdk_calls **out);
void mdk_session_close(mdk_session *s);
int64_t mdk_calls_count(const mdk_calls *c);
int  mdk_calls_n_contigs(const mdk_calls *c);
const char *mdk_calls_contig_name(const mdk_calls *c, int i);
/* what the run's command line said, for whoever writes the command's files from the rows (include/mdk_hip.h md_text_*): 1 when --mergeContext
 * was on (the bedGraph header then says " merged"), and the contexts switched on as a bitmask (bit 0 CpG, 1 CHG, 2 CHH) -- the command writes a
 * file, header only, also for a context that is on and has no row.  0 for the empty result of -h / --version; -1 for NULL */
int  mdk_calls_merged(const mdk_calls *c);
int  mdk_calls_contexts(const mdk_calls *c);
int  mdk_calls_copy(const mdk_calls *c, int column, void *dst, int to_host);
void mdk_calls_free(mdk_calls *c);

/* ---- the same session's perRead: per-read methylation as device-resident columns ----
 * mdk_session_perread takes the argv of perRead_main (argv[0] = "perRead"), parses it with the same code and returns the same codes for the
 * same errors.  Instead of text it returns one row per line the command would print, in the same order (chunks in schedule order, reads
 * within a chunk in file order) -- include/mdk_hip.h "reads on the device":
 *   contig (int32, BAM header index), pos (int32, the line's column 3), nmeth, nunmeth (int32: the line prints 100*nmeth/(nmeth+nunmeth)
 *   and the sum), name_offsets (int64, count + 1 entries, the first 0) and name_bytes (uint8: the names back to back, each what %s prints
 *   of the record's name).
 * Differences from the command: -o is ignored and nothing is opened for writing; the process is never left through _exit.  -h / --version
 * return 0 and an empty mdk_reads (no device memory: its one name offset, 0, can be copied to the host only).  A run uses the device handle
 * with the slots and streams of an extract run, so extract and perRead runs alternate on one handle (md_dev_reset between runs).
 * Ownership and lifetimes are those of mdk_calls: each successful mdk_session_perread returns a new mdk_reads (*out; NULL on error) that owns
 * its rows in device memory and its contig names, does not depend on the session and stays valid, also after mdk_session_close, until
 * mdk_reads_free.  mdk_reads_copy is synchronous: `dst` (device memory of the session's device when to_host = 0, host memory when 1) holds
 * the column when it returns -- mdk_reads_count entries, count + 1 for MDK_READS_NAME_OFFSETS, mdk_reads_name_bytes for MDK_READS_NAME_BYTES. */
typedef struct mdk_reads mdk_reads;
enum { MDK_READS_CONTIG = 0, MDK_READS_POS, MDK_READS_NMETH, MDK_READS_NUNMETH, MDK_READS_NAME_OFFSETS, MDK_READS_NAME_BYTES };   /* int32 x4, int64, uint8 */
int  mdk_session_perread(mdk_session *s, int argc, char *argv[], mdk_reads **out);
int64_t mdk_reads_count(const mdk_reads *r);
int64_t mdk_reads_name_bytes(const mdk_reads *r);
int  mdk_reads_n_contigs(const mdk_reads *r);
const char *mdk_reads_contig_name(const mdk_reads *r, int i);
int  mdk_reads_copy(const mdk_reads *r, int column, void *dst, int to_host);
void mdk_reads_free(mdk_reads *r);

/* ---- the same session's mbias: the methylation-bias table as device-resident columns ----
 * mdk_session_mbias takes the argv of mbias_main (argv[0] = "mbias"), parses it with the same code and returns the same codes for the same
 * errors -- a command line without --noSVG still needs its output prefix (rc -1 without it).  The prefix is ignored: no SVG is written,
 * nothing is printed to stdout, --txt changes nothing.  What comes back (include/mdk_hip.h "the methylation-bias table on the device"):
 *   the table's rows in the order the command prints them -- MDK_BIAS_STRAND (int8, 0..3 = OT, OB, CTOT, CTOB), MDK_BIAS_READ (int8, 1 or 2),
 *   MDK_BIAS_POSITION (int32, 1-based), MDK_BIAS_NMETH, MDK_BIAS_NUNMETH (int64) --, MDK_BIAS_COUNTS, the dense histogram as int64
 *   [mdk_bias_len][4][2][2] (position, strand, read, methylated/unmethylated), and the inclusion bounds the command suggests when it draws
 *   its plots, always computed here: mdk_bias_suggested(b, strand, bounds) returns 1 and the strand's four numbers when the strand has a call.
 * mdk_bias_resubmitted: chunks of the run whose group launch left them out (a read longer than the histogram, more segments than reserved)
 * and that were counted through the single-chunk path instead.  -h / --version return 0 and an empty mdk_bias.  A chunk of a contig the FASTA
 * lacks ends the run with -4, a read of unknown strand aborts, both as in mbias_main.  The run uses the slots and streams of an extract run
 * (groups of up to eight chunks per launch, md_dev_mbias_group), so the three commands alternate on one handle.
 * Ownership and lifetimes are those of mdk_calls; mdk_bias_copy is synchronous (mdk_bias_count entries, 16 * mdk_bias_len for MDK_BIAS_COUNTS). */
typedef struct mdk_bias mdk_bias;
enum { MDK_BIAS_STRAND = 0, MDK_BIAS_READ, MDK_BIAS_POSITION, MDK_BIAS_NMETH, MDK_BIAS_NUNMETH, MDK_BIAS_COUNTS };   /* int8 x2, int32, int64 x3 */
int  mdk_session_mbias(mdk_session *s, int argc, char *argv[], mdk_bias **out);
int64_t mdk_bias_count(const mdk_bias *b);
int64_t mdk_bias_len(const mdk_bias *b);
int64_t mdk_bias_resubmitted(const mdk_bias *b);
int  mdk_bias_suggested(const mdk_bias *b, int strand, int bounds[4]);
int  mdk_bias_copy(const mdk_bias *b, int column, void *dst, int to_host);
void mdk_bias_free(mdk_bias *b);

/* ---- the same session's cytosine report: every cytosine of the reference as device-resident columns ----
 * mdk_session_cytosines takes the argv of extract_main (argv[0] = "extract") and runs it as `extract --cytosine_report`: the option is implied
 * and accepted if given.  Instead of <prefix>.cytosine_report.txt it returns one row per line that file would hold, in the file's order (the
 * chunks of the schedule, ascending position within a chunk) -- include/mdk_hip.h "the cytosine report on the device":
 *   MDK_CYTOSINES_CONTIG (int32, BAM header index), MDK_CYTOSINES_POS (int32, 1-BASED: the line's column 2), MDK_CYTOSINES_STRAND (int8, +1 a C,
 *   -1 a G), MDK_CYTOSINES_NMETH / _NUNMETH (int32), MDK_CYTOSINES_CONTEXT (uint8, 0 CG, 1 CHG, 2 CHH), MDK_CYTOSINES_TRINUCLEOTIDE (uint8, 3 per
 *   row: the letters of column 7).
 * The semantics are the command's, not those of mdk_session_extract's calls: -d does not apply, a site the variant filter drops is a 0 0 row,
 * and there is a row for every cytosine (in the contexts switched on) of every chunk of the schedule (-r, -l, --chunkSize) that is not passed
 * over -- MDK_CHUNK_NOREF and MDK_CHUNK_BED chunks give none --, covered or not, up to the contig's end.  Under -l a chunk that a BED
 * interval touches lists all its cytosines on both strands; only the counts are restricted.  The row set therefore depends on the reference,
 * the contexts and the schedule alone: runs over different BAM files with the same reference and options give columns that line up row for
 * row.  Differences from the command otherwise as for mdk_session_extract (-o ignored, nothing written or printed).  --fraction, --counts,
 * --logit and --methylKit are refused with MDK_RC_UNSUPPORTED; --mergeContext returns what the command returns for it next to
 * --cytosine_report.  mdk_session_extract keeps refusing --cytosine_report.  Ownership and lifetimes are those of mdk_calls; mdk_cytosines_copy
 * is synchronous (mdk_cytosines_count entries; 3 * count bytes for MDK_CYTOSINES_TRINUCLEOTIDE). */
typedef struct mdk_cytosines mdk_cytosines;
enum { MDK_CYTOSINES_CONTIG = 0, MDK_CYTOSINES_POS, MDK_CYTOSINES_STRAND, MDK_CYTOSINES_NMETH, MDK_CYTOSINES_NUNMETH, MDK_CYTOSINES_CONTEXT, MDK_CYTOSINES_TRINUCLEOTIDE };   /* int32 x2, int8, int32 x2, uint8, uint8 x3 */
int  mdk_session_cytosines(mdk_session *s, int argc, char *argv[], mdk_cytosines **out);
int64_t mdk_cytosines_count(const mdk_cytosines *c);
int  mdk_cytosines_n_contigs(const mdk_cytosines *c);
const char *mdk_cytosines_contig_name(const mdk_cytosines *c, int i);
int  mdk_cytosines_contexts(const mdk_cytosines *c);      /* as mdk_calls_contexts: the contexts whose cytosines are rows (--mergeContext never reaches a report) */
int  mdk_cytosines_copy(const mdk_cytosines *c, int column, void *dst, int to_host);
void mdk_cytosines_free(mdk_cytosines *c);

/* ---- the reference genome for callers that parse text (include/mdk_hip.h md_text_reference): the FASTA reader every command uses ----
 * mdk_reference_load reads the whole file (names cut at the first blank, the printable characters of the sequence lines, case kept) and
 * returns 0 and *out, or -1 and NULL.  Names and bases belong to the object until mdk_reference_free; mdk_reference_bases is
 * mdk_reference_length bytes without a terminator.  An index outside [0, n_contigs) gives NULL / -1. */
typedef struct mdk_reference mdk_reference;
int  mdk_reference_load(const char *fasta, mdk_reference **out);
int  mdk_reference_n_contigs(const mdk_reference *r);
const char *mdk_reference_name(const mdk_reference *r, int i);
int64_t mdk_reference_length(const mdk_reference *r, int i);
const char *mdk_reference_bases(const mdk_reference *r, int i);
void mdk_reference_free(mdk_reference *r);

/* ---- `mergeContext` (mergeContext.c; main.c:19,53-54): text-to-text host tool, no device work ---- */
int  mergeContext_main(int argc, char *argv[]);

#ifdef __cplusplus
}
#endif
#endif
