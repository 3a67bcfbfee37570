"""methyldackel_amd -- MI355X-native `MethylDackel extract` hot path.

The product is native code: ``csrc/mdk_hip.hip`` (HIP kernels + device C-ABI, ``include/mdk_hip.h``) and
``csrc/host/*.c`` (C host: BGZF/BAM decode, admission, pairing, chunk schedule, text emitters;
``include/mdk_extract.h``).  This package is only the ctypes view of those two C-ABIs that the tests, bench.py
and the multi-GPU driver use; it contains no compute and no fallback -- importing works anywhere, but every
device call fails loudly when ``libmdk_hip.so`` is missing or no GPU is visible.

Reference interface mirrored: ``extract_main(argc, argv)`` (reference extract.c:706) and the per-chunk
pipeline of ``extractCalls`` (reference extract.c:247-560).
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
import struct
import subprocess
import threading
from pathlib import Path

ROOT = Path(__file__).resolve().parent
REPO = ROOT.parent
BUILD = Path(os.environ["MDK_BUILD_DIR"]) if os.environ.get("MDK_BUILD_DIR") else ROOT / "_build"      # MDK_BUILD_DIR: experiment builds (tools/kbench.py)
LIB_HIP = BUILD / "libmdk_hip.so"
LIB_EXTRACT = BUILD / "libmdk_extract.so"
LIB_INDEX = BUILD / "libmdk_index.so"                          # tabix indexes: a library of its own, loaded at the first index call
LIB_STATS = BUILD / "libmdk_stats.so"                          # the replicates' F test: likewise, loaded at the first diff_replicates call
LIB_SMOOTH = BUILD / "libmdk_smooth.so"                        # smoothing: likewise, loaded at the first smooth call
LIB_COHORT = BUILD / "libmdk_cohort.so"                        # the united table as text and its sums over intervals: likewise, loaded at the first Cohort.write / render / read / regions call
LIB_TRACK = BUILD / "libmdk_track.so"                         # the bigWig track: likewise, loaded at the first render_bigwig / write_bigwig call
CLI = BUILD / "MethylDackel"

CHUNK_NOREF, CHUNK_FOREIGN, CHUNK_BED = 1, 2, 4
CHUNK_EMPTY = CHUNK_NOREF | CHUNK_BED      # passed over by every rank: nothing is packed and nothing is emitted
MDK_ERR = {-1: "HIP call failed", -2: "no device", -3: "bad argument", -4: "reference not uploaded",
           -5: "strand 0 read reached a call", -6: "out of memory"}


class MdkError(RuntimeError):
    pass


class md_dev_cfg(C.Structure):
    _fields_ = [("keepCpG", C.c_int32), ("keepCHG", C.c_int32), ("keepCHH", C.c_int32), ("minPhred", C.c_int32),
                ("minOppositeDepth", C.c_int32), ("bounds", C.c_int32 * 16), ("absoluteBounds", C.c_int32 * 16),
                ("tile", C.c_int32), ("n_slots", C.c_int32), ("n_streams", C.c_int32)]


class md_seg(C.Structure):
    _fields_ = [("rpos", C.c_int32), ("off4", C.c_uint32), ("l_qseq", C.c_uint32), ("q0", C.c_uint32), ("len", C.c_uint16),
                ("sf", C.c_uint8), ("msf", C.c_uint8), ("m_off4", C.c_uint32), ("m_l_qseq", C.c_uint32), ("m_q0", C.c_uint32)]


class md_read_batch(C.Structure):
    _fields_ = [("tid", C.c_int32), ("beg", C.c_int64), ("end", C.c_int64), ("n_segs", C.c_int32),
                ("seg", C.POINTER(md_seg)), ("blob", C.POINTER(C.c_uint8)), ("blob_bytes", C.c_uint64),
                ("n_reads", C.c_int32), ("algo_bytes", C.c_uint64)]


class md_prep_cfg(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("ignore_flags", C.c_int32), ("require_flags", C.c_int32), ("keep_dupes", C.c_int32), ("ignore_nh", C.c_int32),
                ("keep_singleton", C.c_int32), ("keep_discordant", C.c_int32), ("min_phred", C.c_int32), ("min_conv_eff", C.c_float),
                ("map_on", C.c_int32), ("min_mappable", C.c_int32), ("no_pairing", C.c_int32), ("perread", C.c_int32)]


class md_raw_range(C.Structure):
    _fields_ = [("ptr", C.POINTER(C.c_uint8)), ("bytes", C.c_uint64), ("d_rec_off", C.POINTER(C.c_uint32)), ("n_records", C.c_uint32), ("rec_delta", C.c_uint32), ("h_rec_off", C.POINTER(C.c_uint32))]


class md_raw_batch(C.Structure):
    _fields_ = [("tid", C.c_int32), ("beg", C.c_int64), ("end", C.c_int64), ("n_ranges", C.c_int32), ("range", C.POINTER(md_raw_range)),
                ("n_records", C.c_int32), ("rec_off", C.POINTER(C.c_uint32)), ("woff", C.c_int64), ("wlen", C.c_int64)]


class md_inf_member(C.Structure):
    _fields_ = [("in_off", C.c_uint64), ("in_len", C.c_uint32), ("out_len", C.c_uint32), ("out_off", C.c_uint64), ("crc32", C.c_uint32), ("reserved", C.c_uint32)]


class md_inf_digest(C.Structure):
    _fields_ = [("n_rec", C.c_uint32), ("first_rec", C.c_uint32), ("tid0", C.c_int32), ("pos0", C.c_int32), ("tidN", C.c_int32), ("posN", C.c_int32),
                ("min_endp", C.c_int32), ("max_endp", C.c_int32), ("ok", C.c_int32), ("sorted", C.c_int32)]


class md_piece_info(C.Structure):
    _fields_ = [("n_mem", C.c_int32), ("digest", C.POINTER(md_inf_digest)), ("n_records", C.c_uint32), ("out_bytes", C.c_uint64),
                ("d_out", C.c_void_p), ("d_rec_off", C.c_void_p)]


class md_region(C.Structure):
    _fields_ = [("start", C.c_int32), ("end", C.c_int32), ("strand", C.c_int32)]


class md_pr_read(C.Structure):
    _fields_ = [("pos", C.c_int32), ("off4", C.c_uint32), ("l_qseq", C.c_uint32), ("cig_off", C.c_uint32), ("n_cigar", C.c_uint16),
                ("strand", C.c_uint8), ("reserved", C.c_uint8)]


class md_pr_batch(C.Structure):
    _fields_ = [("tid", C.c_int32), ("beg", C.c_int64), ("end", C.c_int64), ("n_reads", C.c_int32), ("read", C.POINTER(md_pr_read)),
                ("cigar", C.POINTER(C.c_uint32)), ("n_cigar", C.c_uint64), ("blob", C.POINTER(C.c_uint8)), ("blob_bytes", C.c_uint64)]


class md_pr_count(C.Structure):
    _fields_ = [("nmeth", C.c_uint32), ("nunmeth", C.c_uint32)]


class md_mbias(C.Structure):
    _fields_ = [("len", C.c_int32), ("count", C.POINTER(C.c_uint32))]


class md_site(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("nmeth", C.c_uint32), ("nunmeth", C.c_uint32), ("meta", C.c_uint32)]


class md_site_var(C.Structure):
    _fields_ = [("noff", C.c_uint32), ("nvar", C.c_uint32)]


class md_tile_seg(C.Structure):
    _fields_ = [("off", C.c_uint32), ("cnt", C.c_uint32)]


class md_sites(C.Structure):
    _fields_ = [("n_sites", C.c_int64), ("site", C.POINTER(md_site)), ("var", C.POINTER(md_site_var))]


class md_sites_dev(C.Structure):
    _fields_ = [("n_slots", C.c_int64), ("n_tiles", C.c_int32), ("d_site", C.c_void_p), ("d_var", C.c_void_p), ("d_seg", C.c_void_p)]


class md_text_cols(C.Structure):
    """md_calls_cols and md_cytosines_cols alike: seven device pointers, in the order of CALL_COLUMNS / CYTOSINE_COLUMNS"""
    _fields_ = [(f"c{i}", C.c_void_p) for i in range(7)]


class md_reads_cols(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("contig", "pos", "nmeth", "nunmeth", "name_off", "name_bytes")]


class md_bench_result(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_pileup", C.c_float), ("algo_bytes", C.c_uint64), ("n_sites", C.c_uint64),
                ("tile", C.c_int32), ("n_tiles", C.c_int32), ("lds_bytes", C.c_int32)]


class mdk_chunk(C.Structure):
    _fields_ = [("index", C.c_uint32), ("tid", C.c_int32), ("beg", C.c_int64), ("end", C.c_int64), ("skipped", C.c_int32),
                ("batch", md_read_batch), ("n_records_seen", C.c_uint64), ("pr", md_pr_batch), ("host", C.c_void_p),
                ("prep", C.c_int32), ("raw", md_raw_batch)]


class md_bench_run_result(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("slots_last", C.c_uint64), ("exchanges", C.c_uint64), ("bytes_per_exchange", C.c_uint64)]


COMM_ID_BYTES = 128
md_comm_oob_fn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)      # out-of-band all-gather for md_comm_open_rank_shared

def raw_record_offsets(raw):
    """offset, in the concatenation of the batch's ranges, of every record of an md_raw_batch whose ranges all lie in HOST memory: from each
    range's own table (h_rec_off) or, for ranges without one, from the batch's rec_off array (include/mdk_hip.h md_raw_range)"""
    out, o, hidx = [], 0, 0
    tables = any(bool(raw.range[i].h_rec_off) or bool(raw.range[i].d_rec_off) for i in range(raw.n_ranges))
    if not tables:
        return [raw.rec_off[i] for i in range(raw.n_records)]
    for i in range(raw.n_ranges):
        r = raw.range[i]
        if r.d_rec_off:
            raise MdkError("raw_record_offsets: a range lies in device memory")
        if r.h_rec_off:
            out += [r.h_rec_off[k] - r.rec_delta + o for k in range(r.n_records)]
        else:
            out += [raw.rec_off[hidx + k] for k in range(r.n_records)]; hidx += r.n_records
        o += r.bytes
    return out


HIP_SYMBOLS = ["md_dev_count", "md_dev_warm", "md_dev_quiesce", "md_dev_reserve_hint", "md_dev_open", "md_dev_close", "md_dev_last_error", "md_dev_tile", "md_dev_set_reference", "md_dev_set_regions",
               "md_dev_upload", "md_dev_launch", "md_dev_submit", "md_dev_download", "md_dev_sync", "md_dev_bind_output", "md_dev_wait", "md_sites_order",
               "md_dev_bench", "md_dev_bench_rotate", "md_dev_launch_group", "md_dev_group_max", "md_dev_download_group", "md_dev_reserve_contigs", "md_comm_unique_id", "md_comm_open_rank", "md_comm_open_rank_shared", "md_comm_close", "md_comm_world", "md_comm_gather", "md_comm_wait", "md_comm_result_header", "md_comm_result_send", "md_comm_result_recv", "md_dev_pci_bus_id",
               "md_bench_open", "md_bench_run", "md_bench_verify", "md_bench_region_bytes", "md_bench_close", "md_dev_debug_effective", "md_host_alloc", "md_host_free", "md_host_set_pinned", "md_host_profile", "md_dev_profile_text", "md_host_register", "md_host_register_all",
               "md_dev_set_prep", "md_dev_set_mappability", "md_dev_upload_raw", "md_dev_upload_raw_inplace", "md_dev_upload_wait", "md_dev_upload_done", "md_dev_submit_raw", "md_dev_debug_segments", "md_dev_bench_prep", "md_dev_bench_prep_rotate", "md_bench_set_prep",
               "md_dev_mbias_submit", "md_dev_mbias_submit_raw", "md_dev_mbias_read", "md_dev_mbias_reset", "md_dev_slot_sync",
               "md_dev_mbias_group", "md_dev_mbias_collect", "md_dev_mbias_redone", "md_dev_bias_finish", "md_bias_set_count", "md_bias_set_len", "md_bias_set_redone", "md_bias_set_hist", "md_bias_set_copy", "md_bias_set_free",
               "md_dev_perread_submit", "md_dev_perread_download", "md_dev_perread_submit_raw", "md_dev_perread_download_raw", "md_dev_read_raw",
               "md_piece_members_per_round", "md_piece_create", "md_piece_destroy", "md_piece_submit", "md_piece_wait", "md_piece_read", "md_piece_read_records", "md_piece_copy", "md_piece_bench", "md_piece_bench_crc",
               "md_dev_calls_begin", "md_dev_calls_group", "md_dev_calls_finish", "md_calls_set_count", "md_calls_set_copy", "md_calls_set_free", "md_dev_reset",
               "md_dev_reads_begin", "md_dev_reads_slot", "md_dev_reads_collect", "md_dev_reads_host", "md_dev_reads_finish", "md_reads_set_count", "md_reads_set_name_bytes", "md_reads_set_copy", "md_reads_set_free",
               "md_dev_cytosines_begin", "md_dev_cytosines_group", "md_dev_cytosines_finish", "md_cytosines_set_count", "md_cytosines_set_copy", "md_cytosines_set_free",
               "md_text_open", "md_text_measure_calls", "md_text_measure_cytosines", "md_text_measure_reads", "md_text_fill", "md_text_gather_names", "md_text_close", "md_text_merge_measure", "md_text_merge_fill", "md_text_regions", "md_text_unite_measure", "md_text_unite_fill", "md_text_diff", "md_text_dmr_measure", "md_text_dmr_fill",
               "md_text_reference", "md_text_parse_measure", "md_text_parse_fill_calls", "md_text_parse_fill_cytosines", "md_text_parse_error_offset", "md_text_deflate_measure", "md_text_deflate_fill"]
EXTRACT_SYMBOLS = ["extract_main", "mdk_plan_open", "mdk_plan_close", "mdk_plan_dev_cfg", "mdk_plan_ensure_reference",
                   "mdk_plan_next_chunk", "mdk_plan_try_next_chunk", "mdk_plan_emit", "mdk_plan_finish", "mdk_plan_set_shard", "mdk_plan_n_targets", "mdk_plan_target_name",
                   "mdk_plan_target_len", "mdk_plan_regions", "mdk_plan_set_prep", "mdk_plan_set_hold", "mdk_plan_prep_cfg", "mdk_plan_host_prepare",
                   "mdk_plan_host_prepare_from", "mdk_plan_release_records", "mdk_plan_attach_device", "mdk_plan_detach_device",
                   "mbias_main", "mdk_cli_quiesce", "mdk_plan_open_mbias", "mdk_plan_mbias_outputs", "mdk_mbias_report",
                   "perRead_main", "mdk_plan_open_perread", "mdk_plan_emit_perread", "mdk_plan_emit_perread_raw", "mergeContext_main", "mdk_bind_to_device_node",
                   "mdk_session_open", "mdk_session_extract", "mdk_session_close", "mdk_calls_count", "mdk_calls_n_contigs", "mdk_calls_contig_name", "mdk_calls_merged", "mdk_calls_contexts", "mdk_calls_copy", "mdk_calls_free",
                   "mdk_session_perread", "mdk_reads_count", "mdk_reads_name_bytes", "mdk_reads_n_contigs", "mdk_reads_contig_name", "mdk_reads_copy", "mdk_reads_free",
                   "mdk_mbias_suggest", "mdk_session_mbias", "mdk_bias_count", "mdk_bias_len", "mdk_bias_resubmitted", "mdk_bias_suggested", "mdk_bias_copy", "mdk_bias_free",
                   "mdk_session_cytosines", "mdk_cytosines_count", "mdk_cytosines_n_contigs", "mdk_cytosines_contig_name", "mdk_cytosines_contexts", "mdk_cytosines_copy", "mdk_cytosines_free",
                   "mdk_reference_load", "mdk_reference_n_contigs", "mdk_reference_name", "mdk_reference_length", "mdk_reference_bases", "mdk_reference_free"]

_hip = None
_ext = None


def build(verbose: bool = False) -> None:
    """Compile everything in-tree (hipcc --offload-arch=gfx950 for the kernels, gcc for the host)."""
    r = subprocess.run(["make", "-C", str(REPO), "all"], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode:
        raise MdkError("build failed")


def lib_hip():
    global _hip
    if _hip is None:
        if not LIB_HIP.exists():
            raise MdkError(f"{LIB_HIP} is missing: the HIP extension was not built (run `make` / __graft_entry__.build()); there is no fallback")
        L = C.CDLL(str(LIB_HIP), mode=C.RTLD_GLOBAL)
        L.md_dev_last_error.restype = C.c_char_p
        L.md_dev_open.argtypes = [C.c_int, C.POINTER(md_dev_cfg), C.POINTER(C.c_void_p)]
        L.md_dev_close.argtypes = [C.c_void_p]
        L.md_dev_tile.argtypes = [C.c_void_p]
        L.md_dev_set_reference.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int64]
        L.md_dev_set_regions.argtypes = [C.c_void_p, C.c_int32, C.POINTER(md_region), C.c_int64]
        for f in ("md_dev_upload", "md_dev_submit"):
            getattr(L, f).argtypes = [C.c_void_p, C.c_int, C.POINTER(md_read_batch)]
        L.md_dev_launch.argtypes = [C.c_void_p, C.c_int]
        L.md_dev_download.argtypes = [C.c_void_p, C.c_int, C.POINTER(md_sites)]
        L.md_dev_sync.argtypes = [C.c_void_p]
        L.md_dev_bind_output.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
        L.md_dev_wait.argtypes = [C.c_void_p, C.c_int, C.POINTER(md_sites_dev)]
        L.md_sites_order.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
        L.md_sites_order.restype = C.c_int64
        L.md_dev_bench.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(md_bench_result)]
        L.md_dev_bench_rotate.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(md_bench_result)]
        L.md_dev_launch_group.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
        L.md_comm_unique_id.argtypes = [C.c_char_p]
        L.md_comm_open_rank.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]
        L.md_comm_open_rank_shared.argtypes = [C.c_void_p, C.c_int, C.c_int, md_comm_oob_fn, C.c_void_p, C.POINTER(C.c_void_p)]
        L.md_bench_set_prep.argtypes = [C.c_void_p, C.c_int]
        L.md_dev_bench_prep_rotate.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.md_comm_close.argtypes = [C.c_void_p]; L.md_comm_close.restype = None
        L.md_comm_world.argtypes = [C.c_void_p]
        L.md_comm_gather.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.md_comm_wait.argtypes = [C.c_void_p]
        L.md_bench_open.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.md_bench_run.argtypes = [C.c_void_p, C.c_int64, C.POINTER(md_bench_run_result)]
        L.md_bench_verify.argtypes = [C.c_void_p]
        L.md_bench_region_bytes.argtypes = [C.c_void_p]; L.md_bench_region_bytes.restype = C.c_int64
        L.md_bench_close.argtypes = [C.c_void_p]; L.md_bench_close.restype = None
        L.md_dev_debug_effective.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.md_dev_set_prep.argtypes = [C.c_void_p, C.POINTER(md_prep_cfg)]
        L.md_dev_set_mappability.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        L.md_dev_upload_raw.argtypes = [C.c_void_p, C.c_int, C.POINTER(md_raw_batch)]
        L.md_dev_submit_raw.argtypes = [C.c_void_p, C.c_int, C.POINTER(md_raw_batch)]
        L.md_dev_bench_prep.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.md_dev_debug_segments.argtypes = [C.c_void_p, C.c_int, C.POINTER(md_seg), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.md_dev_mbias_submit.argtypes = [C.c_void_p, C.c_int, C.POINTER(md_read_batch)]
        L.md_dev_mbias_submit_raw.argtypes = [C.c_void_p, C.c_int, C.POINTER(md_raw_batch)]
        L.md_dev_mbias_read.argtypes = [C.c_void_p, C.POINTER(md_mbias)]
        L.md_dev_mbias_reset.argtypes = [C.c_void_p]
        L.md_dev_slot_sync.argtypes = [C.c_void_p, C.c_int]
        L.md_dev_mbias_group.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
        L.md_dev_mbias_collect.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
        L.md_dev_mbias_redone.argtypes = [C.c_void_p]
        L.md_dev_perread_submit.argtypes = [C.c_void_p, C.c_int, C.POINTER(md_pr_batch)]
        L.md_dev_perread_download.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(md_pr_count)), C.POINTER(C.c_int64)]
        L.md_dev_perread_submit_raw.argtypes = [C.c_void_p, C.c_int, C.POINTER(md_raw_batch)]
        L.md_dev_read_raw.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint32)]
        L.md_piece_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.md_piece_destroy.argtypes = [C.c_void_p]; L.md_piece_destroy.restype = None
        L.md_piece_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(md_inf_member), C.c_int32]
        L.md_piece_wait.argtypes = [C.c_void_p, C.POINTER(md_piece_info)]
        L.md_piece_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.md_piece_read_records.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.md_piece_copy.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.md_piece_bench.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.md_dev_perread_download_raw.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(md_pr_count)), C.POINTER(C.c_int64)]
        L.md_host_alloc.restype = C.c_void_p
        L.md_host_alloc.argtypes = [C.c_uint64]
        L.md_host_free.argtypes = [C.c_void_p]
        _hip = L
    return _hip


def lib_extract():
    global _ext
    if _ext is None:
        lib_hip()
        if not LIB_EXTRACT.exists():
            raise MdkError(f"{LIB_EXTRACT} is missing (run `make`)")
        L = C.CDLL(str(LIB_EXTRACT))
        L.extract_main.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
        L.mdk_plan_open.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
        L.mdk_plan_close.argtypes = [C.c_void_p]
        L.mdk_plan_dev_cfg.argtypes = [C.c_void_p, C.POINTER(md_dev_cfg)]
        L.mdk_plan_ensure_reference.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.mdk_plan_next_chunk.argtypes = [C.c_void_p, C.POINTER(mdk_chunk)]
        L.mdk_plan_emit.argtypes = [C.c_void_p, C.POINTER(mdk_chunk), C.POINTER(md_sites)]
        L.mdk_plan_finish.argtypes = [C.c_void_p]
        L.mdk_plan_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mdk_plan_n_targets.argtypes = [C.c_void_p]
        L.mdk_plan_target_name.argtypes = [C.c_void_p, C.c_int32]
        L.mdk_plan_target_name.restype = C.c_char_p
        L.mdk_plan_target_len.argtypes = [C.c_void_p, C.c_int32]
        L.mdk_plan_target_len.restype = C.c_int64
        L.mbias_main.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
        L.mdk_plan_open_mbias.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
        L.mdk_plan_mbias_outputs.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mdk_mbias_report.argtypes = [C.POINTER(md_mbias), C.c_char_p, C.c_int, C.c_int, C.c_int]
        L.mdk_mbias_suggest.argtypes = [C.POINTER(md_mbias), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.perRead_main.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
        L.mergeContext_main.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
        L.mdk_plan_open_perread.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
        L.mdk_plan_emit_perread.argtypes = [C.c_void_p, C.POINTER(mdk_chunk), C.POINTER(md_pr_count), C.c_int64]
        L.mdk_plan_emit_perread_raw.argtypes = [C.c_void_p, C.POINTER(mdk_chunk), C.POINTER(C.c_uint32), C.POINTER(md_pr_count), C.c_int64]
        L.mdk_plan_regions.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(md_region)), C.POINTER(C.c_int64)]
        L.mdk_plan_set_prep.argtypes = [C.c_void_p, C.c_int]
        L.mdk_plan_prep_cfg.argtypes = [C.c_void_p, C.POINTER(md_prep_cfg)]; L.mdk_plan_prep_cfg.restype = None
        L.mdk_plan_host_prepare.argtypes = [C.c_void_p, C.POINTER(mdk_chunk)]
        L.mdk_plan_host_prepare_from.argtypes = [C.c_void_p, C.POINTER(mdk_chunk), C.c_void_p, C.c_int]
        L.mdk_plan_attach_device.argtypes = [C.c_void_p, C.c_void_p]
        L.mdk_plan_detach_device.argtypes = [C.c_void_p]; L.mdk_plan_detach_device.restype = None
        _ext = L
    return _ext


def _argv(args):
    arr = (C.c_char_p * (len(args) + 1))()
    for i, a in enumerate(args):
        arr[i] = os.fsencode(str(a))
    return arr


class Device:
    """One GPU handle (md_dev_open).  Raises MdkError when no device / no HIP library: there is no CPU path."""

    def __init__(self, cfg: md_dev_cfg, device: int = 0):
        L = lib_hip()
        self.h = C.c_void_p()
        rc = L.md_dev_open(device, C.byref(cfg), C.byref(self.h))
        if rc:
            raise MdkError(f"md_dev_open failed ({rc}): {L.md_dev_last_error().decode()}")
        self.L = L

    def _chk(self, rc, what):
        if rc:
            raise MdkError(f"{what} failed ({rc}): {self.L.md_dev_last_error().decode()}")

    def set_reference(self, tid: int, seq: bytes):
        self._chk(self.L.md_dev_set_reference(self.h, tid, seq, len(seq)), "md_dev_set_reference")

    def set_regions(self, tid: int, runs):
        """runs: [(start, end, strand)], sorted and disjoint (-l/--keepStrand)"""
        arr = (md_region * max(len(runs), 1))(*[md_region(*r) for r in runs])
        self._chk(self.L.md_dev_set_regions(self.h, tid, arr, len(runs)), "md_dev_set_regions")

    def submit(self, slot: int, batch: md_read_batch):
        self._chk(self.L.md_dev_submit(self.h, slot, C.byref(batch)), "md_dev_submit")

    def set_prep(self, cfg: "md_prep_cfg"):
        self._chk(self.L.md_dev_set_prep(self.h, C.byref(cfg)), "md_dev_set_prep")

    def upload_raw(self, slot: int, raw: "md_raw_batch"):
        """H2D of a chunk's BAM records + the device preparation (admission, pairing, segments)"""
        self._chk(self.L.md_dev_upload_raw(self.h, slot, C.byref(raw)), "md_dev_upload_raw")

    def submit_raw(self, slot: int, raw: "md_raw_batch"):
        self._chk(self.L.md_dev_submit_raw(self.h, slot, C.byref(raw)), "md_dev_submit_raw")

    def debug_segments(self, slot: int):
        """-> (list of md_seg as the device preparation built them, number of admitted reads)"""
        n, nr = C.c_int64(), C.c_int64()
        self._chk(self.L.md_dev_debug_segments(self.h, slot, None, 0, C.byref(n), C.byref(nr)), "md_dev_debug_segments")
        arr = (md_seg * max(1, n.value))()
        self._chk(self.L.md_dev_debug_segments(self.h, slot, arr, n.value, C.byref(n), C.byref(nr)), "md_dev_debug_segments")
        return arr, n.value, nr.value

    def upload(self, slot: int, batch: md_read_batch):
        self._chk(self.L.md_dev_upload(self.h, slot, C.byref(batch)), "md_dev_upload")

    def launch(self, slot: int):
        self._chk(self.L.md_dev_launch(self.h, slot), "md_dev_launch")

    def download(self, slot: int) -> md_sites:
        s = md_sites()
        self._chk(self.L.md_dev_download(self.h, slot, C.byref(s)), "md_dev_download")
        return s

    def wait(self, slot: int) -> md_sites_dev:
        s = md_sites_dev()
        self._chk(self.L.md_dev_wait(self.h, slot, C.byref(s)), "md_dev_wait")
        return s

    def bind_output(self, slot: int, d_site, d_var, d_seg, cap_sites: int, cap_tiles: int):
        self._chk(self.L.md_dev_bind_output(self.h, slot, d_site, d_var, d_seg, cap_sites, cap_tiles), "md_dev_bind_output")

    def bench_rotate(self, slots, warmup: int, iters: int, per_launch: int = 1) -> md_bench_result:
        """kernel time with HIP events while rotating over several resident intervals (working set beyond the Infinity Cache),
        `per_launch` intervals per kernel launch"""
        r = md_bench_result()
        arr = (C.c_int * len(slots))(*slots)
        self._chk(self.L.md_dev_bench_rotate(self.h, arr, len(slots), per_launch, warmup, iters, C.byref(r)), "md_dev_bench_rotate")
        return r

    def launch_group(self, slots):
        arr = (C.c_int * len(slots))(*slots)
        self._chk(self.L.md_dev_launch_group(self.h, arr, len(slots)), "md_dev_launch_group")

    def bench(self, slot: int, warmup: int, iters: int) -> md_bench_result:
        r = md_bench_result()
        self._chk(self.L.md_dev_bench(self.h, slot, warmup, iters, C.byref(r)), "md_dev_bench")
        return r

    def mbias_submit(self, slot: int, batch: md_read_batch):
        """accumulate the batch's calls into the device histogram; the batch must stay alive until slot_sync(slot)"""
        self._chk(self.L.md_dev_mbias_submit(self.h, slot, C.byref(batch)), "md_dev_mbias_submit")

    def mbias_submit_raw(self, slot: int, raw: "md_raw_batch"):
        self._chk(self.L.md_dev_mbias_submit_raw(self.h, slot, C.byref(raw)), "md_dev_mbias_submit_raw")

    def mbias_group(self, slots):
        """md_dev_mbias_group + md_dev_mbias_collect over freshly uploaded raw slots (upload_raw): their preparation and histogram with one launch
        per kernel, nothing waited for in between; returns the per-chunk codes and how many chunks the run has sent through the single-chunk path"""
        n = len(slots)
        arr = (C.c_int * n)(*slots)
        rcs = (C.c_int * n)()
        self._chk(self.L.md_dev_mbias_group(self.h, arr, n), "md_dev_mbias_group")
        self._chk(self.L.md_dev_mbias_collect(self.h, arr, n, rcs), "md_dev_mbias_collect")
        return list(rcs), int(self.L.md_dev_mbias_redone(self.h))

    def slot_sync(self, slot: int):
        self._chk(self.L.md_dev_slot_sync(self.h, slot), "md_dev_slot_sync")

    def mbias_read(self):
        """-> numpy uint32 array [len, 4 strands, 2 reads, (meth, unmeth)]"""
        import numpy as np
        m = md_mbias()
        self._chk(self.L.md_dev_mbias_read(self.h, C.byref(m)), "md_dev_mbias_read")
        if m.len <= 0:
            return np.zeros((0, 4, 2, 2), dtype=np.uint32)
        return np.ctypeslib.as_array(m.count, shape=(m.len * 16,)).reshape(m.len, 4, 2, 2).copy()

    def perread(self, slot: int, batch: md_pr_batch):
        """per-read CpG counts of a perRead chunk -> [(nmeth, nunmeth)] (submit + download)"""
        self._chk(self.L.md_dev_perread_submit(self.h, slot, C.byref(batch)), "md_dev_perread_submit")
        out, n = C.POINTER(md_pr_count)(), C.c_int64()
        self._chk(self.L.md_dev_perread_download(self.h, slot, C.byref(out), C.byref(n)), "md_dev_perread_download")
        return [(out[i].nmeth, out[i].nunmeth) for i in range(n.value)]

    def perread_raw(self, slot: int, raw: "md_raw_batch"):
        """perRead from a chunk's raw records: -> (kept record indices, [(nmeth, nunmeth)]) as the device selected and walked them"""
        self._chk(self.L.md_dev_perread_submit_raw(self.h, slot, C.byref(raw)), "md_dev_perread_submit_raw")
        kept, out, n = C.POINTER(C.c_uint32)(), C.POINTER(md_pr_count)(), C.c_int64()
        self._chk(self.L.md_dev_perread_download_raw(self.h, slot, C.byref(kept), C.byref(out), C.byref(n)), "md_dev_perread_download_raw")
        return [kept[i] for i in range(n.value)], [(out[i].nmeth, out[i].nunmeth) for i in range(n.value)]

    def mbias_reset(self):
        self._chk(self.L.md_dev_mbias_reset(self.h), "md_dev_mbias_reset")

    def sync(self):
        self._chk(self.L.md_dev_sync(self.h), "md_dev_sync")

    def close(self):
        if self.h:
            self.L.md_dev_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan:
    """The host pipeline of one `extract` command line, a chunk at a time (mdk_plan_*)."""

    def __init__(self, args, command: str = "extract"):
        L = lib_extract()
        self.L = L
        self.command = command
        self.args = [command] + [str(a) for a in args]
        self._argv = _argv(self.args)
        self.p = C.c_void_p()
        opener = {"extract": L.mdk_plan_open, "mbias": L.mdk_plan_open_mbias, "perRead": L.mdk_plan_open_perread}[command]
        self.rc = opener(len(self.args), self._argv, C.byref(self.p))
        if self.rc or not self.p:
            raise MdkError(f"{opener.__name__} returned {self.rc}")

    def mbias_outputs(self):
        """(prefix or None, svg, txt, which) of an mbias plan"""
        pre, svg, txt, which = C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
        if self.L.mdk_plan_mbias_outputs(self.p, C.byref(pre), C.byref(svg), C.byref(txt), C.byref(which)):
            raise MdkError("not an mbias plan")
        return (pre.value.decode() if pre.value else None), svg.value, txt.value, which.value

    def dev_cfg(self) -> md_dev_cfg:
        cfg = md_dev_cfg()
        self.L.mdk_plan_dev_cfg(self.p, C.byref(cfg))
        return cfg

    def set_shard(self, rank: int, world: int):
        if self.L.mdk_plan_set_shard(self.p, rank, world):
            raise MdkError("mdk_plan_set_shard: bad rank/world")

    def set_prep(self, mode: int):
        """0: chunks are prepared on the host (`batch`); 1: they come as raw records for the device (`raw`)"""
        if self.L.mdk_plan_set_prep(self.p, mode):
            raise MdkError("mdk_plan_set_prep: not possible for this plan (already started, or a perRead/mbias plan)")

    def prep_cfg(self) -> "md_prep_cfg":
        c = md_prep_cfg()
        self.L.mdk_plan_prep_cfg(self.p, C.byref(c))
        return c

    def attach_device(self, dev: "Device"):
        """BGZF inflate on the device too (include/mdk_extract.h mdk_plan_attach_device); detach_device before the device is closed"""
        rc = self.L.mdk_plan_attach_device(self.p, dev.h)
        if rc != 0:
            raise MdkError(f"mdk_plan_attach_device rc={rc}")
        self._attached = True

    def detach_device(self):
        if getattr(self, "_attached", False) and self.p:
            self.L.mdk_plan_detach_device(self.p)
            self._attached = False

    def host_prepare_from(self, chunk: "mdk_chunk", dev: "Device", slot: int):
        rc = self.L.mdk_plan_host_prepare_from(self.p, C.byref(chunk), dev.h, slot)
        if rc != 0:
            raise MdkError(f"mdk_plan_host_prepare_from rc={rc}")

    def host_prepare(self, chunk: "mdk_chunk"):
        rc = self.L.mdk_plan_host_prepare(self.p, C.byref(chunk))
        if rc:
            raise MdkError(f"mdk_plan_host_prepare failed ({rc})")

    def next_chunk(self):
        c = mdk_chunk()
        rc = self.L.mdk_plan_next_chunk(self.p, C.byref(c))
        if rc < 0:
            raise MdkError(f"mdk_plan_next_chunk failed ({rc})")
        return c if rc == 1 else None

    def ensure_reference(self, dev: Device, tid: int):
        rc = self.L.mdk_plan_ensure_reference(self.p, dev.h, tid)
        if rc:
            raise MdkError(f"mdk_plan_ensure_reference failed ({rc}): {lib_hip().md_dev_last_error().decode()}")

    def emit(self, chunk: mdk_chunk, sites: md_sites):
        rc = self.L.mdk_plan_emit(self.p, C.byref(chunk), C.byref(sites))
        if rc:
            raise MdkError(f"mdk_plan_emit failed ({rc})")

    def emit_perread(self, chunk: mdk_chunk, counts):
        """counts: [(nmeth, nunmeth)] per read of the chunk, or None for a chunk whose contig the FASTA lacks"""
        arr, n = None, 0
        if counts is not None:
            n = len(counts)
            arr = (md_pr_count * max(n, 1))(*[md_pr_count(m, u) for m, u in counts])
        rc = self.L.mdk_plan_emit_perread(self.p, C.byref(chunk), arr, n)
        if rc:
            raise MdkError(f"mdk_plan_emit_perread failed ({rc})")

    def finish(self):
        self.L.mdk_plan_finish(self.p)

    def regions(self, tid: int):
        """None without -l, else the [(start, end, strand)] runs the contig's sites are restricted to"""
        ptr, n = C.POINTER(md_region)(), C.c_int64()
        if self.L.mdk_plan_regions(self.p, tid, C.byref(ptr), C.byref(n)):
            raise MdkError("mdk_plan_regions failed")
        return None if n.value < 0 else [(ptr[i].start, ptr[i].end, ptr[i].strand) for i in range(n.value)]

    def target_name(self, tid: int) -> str:
        return self.L.mdk_plan_target_name(self.p, tid).decode()

    def close(self):
        if self.p:
            self.detach_device()
            self.L.mdk_plan_close(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mbias_report(hist, opref, svg: bool, txt: bool, which: int) -> int:
    """makeSVGs/makeTXT of the reference over a [len,4,2,2] uint32 histogram (writes <opref>_<strand>.svg, prints to
    the process's stdout/stderr)"""
    import numpy as np
    a = np.ascontiguousarray(hist, dtype=np.uint32).reshape(-1)
    m = md_mbias(len(a) // 16, a.ctypes.data_as(C.POINTER(C.c_uint32)))
    return lib_extract().mdk_mbias_report(C.byref(m), os.fsencode(str(opref)) if opref is not None else None, int(svg), int(txt), which)


def mbias_suggest(hist):
    """mdk_mbias_suggest over rows [q][16] (any integer array-like): {"OT": (a, b, c, d), ...} for the strands that have calls"""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(hist, dtype=np.uint32).reshape(-1))
    m = md_mbias(len(a) // 16, a.ctypes.data_as(C.POINTER(C.c_uint32)))
    bounds, has = (C.c_int * 16)(), (C.c_int * 4)()
    if lib_extract().mdk_mbias_suggest(C.byref(m), bounds, has):
        raise MdkError("mdk_mbias_suggest failed")
    return {STRANDS[k]: tuple(bounds[4 * k:4 * k + 4]) for k in range(4) if has[k]}


def sites_to_rows(s: md_sites):
    """md_sites -> list of (pos, type, isG, nmeth, nunmeth, noff, nvar) tuples (for tests)."""
    rows = []
    for i in range(s.n_sites):
        r = s.site[i]
        rows.append((r.pos, (r.meta >> 1) & 3, r.meta & 1, r.nmeth, r.nunmeth, s.var[i].noff if s.var else 0, s.var[i].nvar if s.var else 0))
    return rows


def run_cli(args, cwd=None, env=None, command="extract", ranks=None, timeout=None):
    """Run the `MethylDackel extract` (or `mbias`) command of this build; returns CompletedProcess.  `ranks=N` runs the command
    as N processes, one per GPU (csrc/host/mdk_ranks.c), and returns rank 0's."""
    if not CLI.exists():
        raise MdkError(f"{CLI} is missing (run `make`)")
    e = dict(os.environ)
    # a GPU exception in the command: the runtime prints what it was (address, reason) and aborts, instead of piping a GPU core dump to the
    # host's core_pattern helper, which no container holds (that attempt is all round 4's one faulting run left on stderr)
    e.setdefault("HSA_DISABLE_COREDUMP_ON_EXCEPTION", "1")
    if env:
        e.update(env)
    if ranks:
        return run_ranks(args, ranks, cwd=cwd, env=e, command=command, timeout=timeout or 900)
    if "MDK_WORLD" not in e:
        e["MDK_NO_RANKS"] = "1"        # a caller that is itself a torchrun rank (bench.py) runs the command alone, not as its rank
    return subprocess.run([str(CLI), command] + [str(a) for a in args], cwd=cwd, env=e, capture_output=True, text=True, timeout=timeout)


def run_ranks(args, n, cwd=None, env=None, command="extract", devices=None, timeout=900):
    """`MethylDackel extract` as N processes: rank k takes chunks k, k+N, ... of the one schedule every rank derives from the
    same inputs, and rank 0 collects and writes (csrc/host/mdk_ranks.c; the launcher a site would use is `torchrun
    --no-python` or tools/extract_ranks.sh).  `devices`: GPU ordinal per rank (default: rank k on GPU k modulo the visible
    GPUs).  Returns rank 0's CompletedProcess with `.rank_returncodes` and `.rank_stderr` of all ranks."""
    import socket
    if not CLI.exists():
        raise MdkError(f"{CLI} is missing (run `make`)")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(n):
        e = dict(os.environ if env is None else env)
        e.update({"MDK_RANK": str(r), "MDK_WORLD": str(n), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
        if devices is not None:
            e["MDK_DEVICE"] = str(devices[r])
        procs.append(subprocess.Popen([str(CLI), command] + [str(a) for a in args], cwd=cwd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        import threading
        res = [None] * n

        def drain(i):
            res[i] = procs[i].communicate(timeout=timeout)
        ths = [threading.Thread(target=drain, args=(i,)) for i in range(n)]
        [t.start() for t in ths]; [t.join() for t in ths]
        outs = res
    finally:
        for p_ in procs:
            if p_.poll() is None:
                p_.kill()
    out0 = outs[0] or ("", "")
    cp = subprocess.CompletedProcess(procs[0].args, procs[0].returncode, out0[0], out0[1])
    cp.rank_returncodes = [p_.returncode for p_ in procs]
    cp.rank_stderr = [(o or ("", ""))[1] for o in outs]
    return cp


# ---- a resident extract session: the calls as tensors (include/mdk_extract.h mdk_session_*) ----
RC_UNSUPPORTED = -23
CALL_COLUMNS = (("contig", "int32"), ("start", "int32"), ("end", "int32"), ("nmeth", "int32"), ("nunmeth", "int32"), ("context", "uint8"), ("strand", "int8"))
READ_COLUMNS = (("contig", "int32"), ("pos", "int32"), ("nmeth", "int32"), ("nunmeth", "int32"), ("name_offsets", "int64"), ("name_bytes", "uint8"))
BIAS_COLUMNS = (("strand", "int8"), ("read", "int8"), ("position", "int32"), ("nmeth", "int64"), ("nunmeth", "int64"), ("counts", "int64"))
CYTOSINE_COLUMNS = (("contig", "int32"), ("pos", "int32"), ("strand", "int8"), ("nmeth", "int32"), ("nunmeth", "int32"), ("context", "uint8"), ("trinucleotide", "uint8"))
STRANDS = ("OT", "OB", "CTOT", "CTOB")
CONTEXTS = ("CG", "CHG", "CHH")


CONTEXT_FILES = ("CpG", "CHG", "CHH")                         # as the command names its files and headers
TEXT_FORMATS = {"bedGraph": 0, "fraction": 1, "counts": 2, "methylKit": 3}       # MD_TEXT_* of include/mdk_hip.h
TEXT_CYTOSINE_REPORT = 4
TEXT_PERREAD = 5
TEXT_SUFFIX = (".bedGraph", ".meth.bedGraph", ".counts.bedGraph", ".methylKit")
TEXT_WHAT = ("levels", "fractions", "counts")
TEXT_BLOCK_ROWS = 1 << 22                                     # rows per block of `write` / `render`
PARSE_BEDGRAPH, PARSE_CYTOSINE_REPORT = 0, 1                  # MD_PARSE_* of include/mdk_hip.h
PARSE_BLOCK_BYTES = 256 << 20                                 # bytes of a file per piece of `read`


def _text_lib():
    """libmdk_hip.so with the md_text_* entry points typed: resolved here, at the first render, and not when the library is loaded"""
    L = lib_hip()
    if not getattr(L, "_text_types", False):
        L.md_text_open.argtypes = [C.c_int, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
        L.md_text_measure_calls.argtypes = [C.c_void_p, C.POINTER(md_text_cols), C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        L.md_text_measure_cytosines.argtypes = [C.c_void_p, C.POINTER(md_text_cols), C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_int64)]
        L.md_text_measure_reads.argtypes = [C.c_void_p, C.POINTER(md_reads_cols), C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        L.md_text_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.md_text_gather_names.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
        L.md_text_close.argtypes = [C.c_void_p]; L.md_text_close.restype = None
        L.md_text_merge_measure.argtypes = [C.c_void_p, C.POINTER(md_text_cols), C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.md_text_merge_fill.argtypes = [C.c_void_p, C.POINTER(md_text_cols), C.c_int64]
        L.md_text_regions.argtypes = [C.c_void_p, C.POINTER(md_text_cols), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.md_text_unite_measure.argtypes = [C.c_void_p, C.POINTER(md_text_cols), C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.md_text_unite_fill.argtypes = [C.c_void_p] + [C.c_void_p] * 8 + [C.c_int64]
        L.md_text_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_void_p] + [C.c_void_p] * 6
        L.md_text_dmr_measure.argtypes = [C.c_void_p] + [C.c_void_p] * 10 + [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_int64)]
        L.md_text_dmr_fill.argtypes = [C.c_void_p] + [C.c_void_p] * 12 + [C.c_int64]
        L.md_text_reference.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        L.md_text_parse_measure.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int64)]
        L.md_text_parse_fill_calls.argtypes = [C.c_void_p, C.POINTER(md_text_cols), C.c_int64]
        L.md_text_parse_fill_cytosines.argtypes = [C.c_void_p, C.POINTER(md_text_cols), C.c_int64]
        L.md_text_parse_error_offset.argtypes = [C.c_void_p]; L.md_text_parse_error_offset.restype = C.c_int64
        L.md_text_deflate_measure.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int64)]
        L.md_text_deflate_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L._text_types = True
    return L


class _TextRenderer:
    """one md_text: the contig names on the device (uploaded here, once) and the block table of the length scan"""

    def __init__(self, L, device, contigs):
        names = (C.c_char_p * max(len(contigs), 1))(*[os.fsencode(c) for c in contigs])
        self.L, self.h = L, C.c_void_p()
        rc = L.md_text_open(int(device), len(contigs), names, C.byref(self.h))
        if rc:
            self.h = None
            raise _rc_error("md_text_open", rc, L.md_dev_last_error().decode())

    def __del__(self):
        try:
            if self.h:
                self.L.md_text_close(self.h)
                self.h = None
        except Exception:
            pass


def _session_lib():
    L = lib_extract()
    if not getattr(L, "_session_types", False):
        L.mdk_session_open.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.mdk_session_close.argtypes = [C.c_void_p]
        for command, kind, counts in (("extract", "calls", ("count",)), ("perread", "reads", ("count", "name_bytes")), ("cytosines", "cytosines", ("count",))):
            getattr(L, f"mdk_session_{command}").argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
            for f in counts:
                getattr(L, f"mdk_{kind}_{f}").argtypes = [C.c_void_p]
                getattr(L, f"mdk_{kind}_{f}").restype = C.c_int64
            getattr(L, f"mdk_{kind}_n_contigs").argtypes = [C.c_void_p]
            getattr(L, f"mdk_{kind}_contig_name").argtypes = [C.c_void_p, C.c_int]
            getattr(L, f"mdk_{kind}_contig_name").restype = C.c_char_p
            getattr(L, f"mdk_{kind}_copy").argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            getattr(L, f"mdk_{kind}_free").argtypes = [C.c_void_p]
        for f in ("mdk_calls_merged", "mdk_calls_contexts", "mdk_cytosines_contexts"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.mdk_session_mbias.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
        for f in ("count", "len", "resubmitted"):
            getattr(L, f"mdk_bias_{f}").argtypes = [C.c_void_p]
            getattr(L, f"mdk_bias_{f}").restype = C.c_int64
        L.mdk_bias_suggested.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.mdk_bias_copy.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.mdk_bias_free.argtypes = [C.c_void_p]
        L._session_types = True
    return L


# ---- BGZF made on the device (include/mdk_hip.h md_text_deflate_*, csrc/mdk_deflate.hip) ----
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BGZF_MEMBER = 65280                                           # input bytes of a member: bgzip's cut
_BGZF_RENDERERS = {}                                          # device index -> the md_text `bgzf_compress` works on


def _deflate(L, text, data, eof):
    """``data`` (a contiguous uint8 tensor on the renderer's device) as BGZF members on that device, the EOF member behind them if asked for"""
    import torch
    torch.cuda.current_stream(data.device).synchronize()         # the bytes are complete, and nothing of torch's is queued on memory it hands out next
    size = C.c_int64()
    rc = L.md_text_deflate_measure(text.h, C.c_void_p(data.data_ptr() if data.numel() else 0), data.numel(), int(bool(eof)), C.byref(size))
    if rc:
        raise _rc_error("md_text_deflate_measure", rc, L.md_dev_last_error().decode())
    out = torch.empty(size.value, dtype=torch.uint8, device=data.device)
    rc = L.md_text_deflate_fill(text.h, C.c_void_p(out.data_ptr() if size.value else 0), size.value)
    if rc:
        raise _rc_error("md_text_deflate_fill", rc, L.md_dev_last_error().decode())
    return out


def bgzf_compress(data, eof=True):
    """``data``, a contiguous uint8 tensor on a device, as a BGZF file's bytes on that device (csrc/mdk_deflate.hip): members of 65280 input
    bytes, bgzip's cut, each compressed by one wavefront with LZ77 matches and Huffman codes fitted to it (stored where that is smaller:
    no member is longer than its input plus 31 bytes), then the 28-byte EOF member unless ``eof`` is false.  No bytes give the EOF member
    alone.  ``gzip.decompress`` of the result is ``data``; the bytes depend on ``data`` alone.  There are no compression levels.  A CPU
    tensor raises MdkError: there is no CPU path."""
    import torch
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise MdkError("bgzf_compress needs a contiguous one-dimensional uint8 tensor")
    if data.device.type != "cuda":
        raise MdkError(f"bytes are compressed on the device: the tensor is a {data.device.type} tensor, and there is no CPU path")
    if data.numel() > (1 << 31) - 1:
        raise MdkError("bgzf_compress takes at most 2^31 - 1 bytes a call")
    L, k = _text_lib(), data.device.index or 0
    if k not in _BGZF_RENDERERS:
        _BGZF_RENDERERS[k] = _TextRenderer(L, k, [])
    return _deflate(L, _BGZF_RENDERERS[k], data, eof)


def _region_filter(contigs, intervals, contexts, strand, min_depth):
    """what ``Calls.regions``, ``Cytosines.regions`` and ``Cohort.regions`` ask, checked before a tensor is looked at:
    (context_mask, strand_mask, min_depth) as csrc/mdk_region_core.h takes them"""
    if not isinstance(intervals, Intervals):
        raise MdkError("regions needs an Intervals (Intervals.read, Intervals.windows)")
    if list(intervals.contigs) != list(contigs):
        raise MdkError("the intervals' contigs are not the rows' contigs: their indices would name other sequences")
    if contexts is None:
        contexts = (0, 1, 2)
    context_mask = 0
    for x in ([contexts] if isinstance(contexts, (str, int)) else contexts):
        if x in CONTEXT_FILES:
            x = CONTEXT_FILES.index(x)
        if isinstance(x, bool) or x not in (0, 1, 2):
            raise MdkError(f"unknown context {x!r}: a subset of {CONTEXT_FILES}, or of the indices 0 to 2")
        context_mask |= 1 << x
    if strand not in (None, "+", "-"):
        raise MdkError(f"unknown strand {strand!r}: None (any), '+' or '-'")
    strand_mask = {None: 7, "+": 1, "-": 2}[strand]
    min_depth = int(min_depth)
    if not 0 <= min_depth <= 2 ** 31 - 1:
        raise MdkError("min_depth must be between 0 and 2^31 - 1")
    return context_mask, strand_mask, min_depth


def _region_intervals(intervals, dev):
    """``intervals`` on ``dev`` (itself if it is there already), its three columns checked"""
    import torch
    iv = intervals.to(dev)
    k = len(iv)
    for name in ("contig", "start", "end"):
        t = getattr(iv, name)
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.shape[0] != k:
            raise MdkError(f"the intervals' {name} column must be a contiguous int32 tensor with one entry per interval")
    return iv


class _Columns:
    """what a session run returns: ``contigs`` (names, BAM header order) and one tensor attribute per entry of COLUMNS"""
    COLUMNS = ()

    def __init__(self, contigs, columns):
        self.contigs = contigs
        for name, _ in self.COLUMNS:
            setattr(self, name, columns[name])

    def __len__(self):
        return int(getattr(self, self.COLUMNS[0][0]).shape[0])

    # what Session._run asks of a result kind: the entries of the columns that do not hold one per row, and the object from the filled columns
    KIND = ""
    ALWAYS = ()          # columns that hold entries even when there is no row

    @classmethod
    def _sizes(cls, L, out, n):
        return {}

    @classmethod
    def _build(cls, L, out, cols):
        k = cls.KIND
        return cls([getattr(L, f"mdk_{k}_contig_name")(out, i).decode() for i in range(getattr(L, f"mdk_{k}_n_contigs")(out))], cols)

    # ---- text on the device (include/mdk_hip.h md_text_*): Calls and Cytosines; Reads has a select and checks of its own ----
    def select(self, index):
        """a copy with the rows ``column[index]`` of every column (a boolean mask, an index tensor, a slice), same contigs and options:
        what ``render`` and ``write`` take just as they take the session's own result"""
        import copy
        c = copy.copy(self)
        c._text = None
        for name, _ in self.COLUMNS:
            setattr(c, name, getattr(self, name)[index].contiguous())
        return c

    def _text_blocks(self, fmt, context, block_rows):
        """the text of the rows, a block of at most ``block_rows`` rows at a time: uint8 tensors on the columns' device, made there by
        k_text_len / k_text_fill"""
        import torch
        cols = [getattr(self, name) for name, _ in self.COLUMNS]
        dev = cols[0].device
        for t, (name, dt) in zip(cols, self.COLUMNS):
            if t.device.type != "cuda":
                raise MdkError(f"text is made on the device: the {name} column is a {t.device.type} tensor, and there is no CPU path")
            if t.device != dev or t.dtype != getattr(torch, dt) or not t.is_contiguous() or t.shape[0] != cols[0].shape[0]:
                raise MdkError(f"the {name} column must be a contiguous {dt} tensor on {dev} with one entry per row")
        L = self._renderer(dev)
        view = md_text_cols(*[C.c_void_p(t.data_ptr()) for t in cols])
        return self._text_iter(L, view, dev, fmt, context, self._block_rows(block_rows))         # (checked before a file is opened; made block by block)

    @staticmethod
    def _block_rows(block_rows):
        block_rows = int(block_rows or os.environ.get("MDK_TEXT_BLOCK_ROWS") or TEXT_BLOCK_ROWS)        # (the variable is a test hook)
        if not 1 <= block_rows <= 1 << 30:
            raise MdkError("block_rows must be between 1 and 2^30")
        return block_rows

    def _renderer(self, dev):
        """libmdk_hip.so, and this object's md_text on the columns' device made if it is not there yet"""
        L = _text_lib()
        if getattr(self, "_text", None) is None:
            self._text = _TextRenderer(L, dev.index or 0, self.contigs)
        return L

    def _merged(self, cols, min_depth):
        """mergeContext over ``cols`` -- this object's rows as the seven tensors of CALL_COLUMNS -- on their device (k_merge_len /
        k_merge_fill, csrc/mdk_merge.hip): a Calls of new tensors, allocated by torch at the measured row count"""
        import torch
        min_depth = int(min_depth)
        if min_depth < 0:
            raise MdkError("min_depth must not be negative")
        dev, n = cols[0].device, int(cols[0].shape[0])
        for t, (name, dt) in zip(cols, CALL_COLUMNS):
            if t.device.type != "cuda":
                raise MdkError(f"rows are merged on the device: the {name} column is a {t.device.type} tensor, and there is no CPU path")
            if t.device != dev or t.dtype != getattr(torch, dt) or t.dim() != 1 or not t.is_contiguous() or t.shape[0] != n:
                raise MdkError(f"the {name} column must be a contiguous {dt} tensor on {dev} with one entry per row")
        L = self._renderer(dev)
        torch.cuda.current_stream(dev).synchronize()             # the columns are complete, and nothing of torch's is queued on memory it hands out next
        view, rows = md_text_cols(*[C.c_void_p(t.data_ptr()) for t in cols]), C.c_int64()
        rc = L.md_text_merge_measure(self._text.h, C.byref(view), n, min_depth, C.byref(rows))
        if rc:
            raise _rc_error("md_text_merge_measure", rc, L.md_dev_last_error().decode())
        out = {name: torch.empty(rows.value, dtype=getattr(torch, dt), device=dev) for name, dt in CALL_COLUMNS}
        rc = L.md_text_merge_fill(self._text.h, C.byref(md_text_cols(*[C.c_void_p(out[name].data_ptr()) for name, _ in CALL_COLUMNS])), rows.value)
        if rc:
            raise _rc_error("md_text_merge_fill", rc, L.md_dev_last_error().decode())
        return Calls(self.contigs, out, merged=True, contexts_on=self.contexts_on)

    def _regions(self, cols, intervals, contexts, strand, min_depth):
        """the sums of ``cols`` -- this object's rows as the seven tensors of CALL_COLUMNS -- over ``intervals`` on the rows' device
        (k_region_rows / k_region_blocks / k_region_sum, csrc/mdk_regions.hip): a Regions of the intervals' tensors and three new ones"""
        import torch
        context_mask, strand_mask, min_depth = _region_filter(self.contigs, intervals, contexts, strand, min_depth)
        dev, n = cols[0].device, int(cols[0].shape[0])
        for t, (name, dt) in zip(cols, CALL_COLUMNS):
            if t.device.type != "cuda":
                raise MdkError(f"regions are summed on the device: the {name} column is a {t.device.type} tensor, and there is no CPU path")
            if t.device != dev or t.dtype != getattr(torch, dt) or t.dim() != 1 or not t.is_contiguous() or t.shape[0] != n:
                raise MdkError(f"the {name} column must be a contiguous {dt} tensor on {dev} with one entry per row")
        iv = _region_intervals(intervals, dev)
        k = len(iv)
        L = self._renderer(dev)
        out = {"contig": iv.contig, "start": iv.start, "end": iv.end, "nsites": torch.empty(k, dtype=torch.int32, device=dev),
               "nmeth": torch.empty(k, dtype=torch.int64, device=dev), "nunmeth": torch.empty(k, dtype=torch.int64, device=dev)}
        torch.cuda.current_stream(dev).synchronize()             # the columns are complete, and nothing of torch's is queued on memory it hands out next
        view = md_text_cols(*[C.c_void_p(t.data_ptr()) for t in cols])
        rc = L.md_text_regions(self._text.h, C.byref(view), n, C.c_void_p(iv.contig.data_ptr()), C.c_void_p(iv.start.data_ptr()), C.c_void_p(iv.end.data_ptr()), k,
                               context_mask, strand_mask, min_depth, C.c_void_p(out["nsites"].data_ptr()), C.c_void_p(out["nmeth"].data_ptr()), C.c_void_p(out["nunmeth"].data_ptr()))
        if rc:
            raise _rc_error("md_text_regions", rc, L.md_dev_last_error().decode())
        return Regions(list(self.contigs), out)

    def _text_iter(self, L, view, dev, fmt, context, block_rows):
        import torch
        n = len(self)
        for r0 in range(0, max(n, 1), block_rows):
            r1 = min(n, r0 + block_rows)
            torch.cuda.current_stream(dev).synchronize()         # the columns are complete, and nothing of torch's is queued on memory it hands out next
            size = C.c_int64()
            if fmt == TEXT_PERREAD:
                rc = L.md_text_measure_reads(self._text.h, C.byref(view), int(self.name_bytes.shape[0]), r0, r1, C.byref(size))
            elif fmt == TEXT_CYTOSINE_REPORT:
                rc = L.md_text_measure_cytosines(self._text.h, C.byref(view), r0, r1, -1 if context is None else int(context), C.byref(size))
            else:
                rc = L.md_text_measure_calls(self._text.h, C.byref(view), r0, r1, fmt, -1 if context is None else int(context), C.byref(size))
            if rc:
                raise _rc_error("md_text_measure", rc, L.md_dev_last_error().decode())
            out = torch.empty(size.value, dtype=torch.uint8, device=dev)
            rc = L.md_text_fill(self._text.h, C.c_void_p(out.data_ptr()), size.value)
            if rc:
                raise _rc_error("md_text_fill", rc, L.md_dev_last_error().decode())
            yield out

    def _compressed(self, blocks, head, dev, feed=None):
        """the header line and every block of text as BGZF members on the device (a member never spans two blocks; the header's are its own).
        ``feed``: every piece of text is shown to it before it is deflated (the tabix indexer: the text is on the device just then)"""
        import torch
        L = _text_lib()
        if head:
            h = _device_bytes(head, dev)
            if feed:
                feed(h)
            yield _deflate(L, self._text, h, False)
        for b in blocks:
            if b.numel():
                if feed:
                    feed(b)
                yield _deflate(L, self._text, b, False)

    def _render(self, fmt, context, head, block_rows, compress=False):
        import torch
        blocks = self._text_blocks(fmt, context, block_rows)
        dev = getattr(self, self.COLUMNS[0][0]).device
        if compress:
            parts = list(self._compressed(blocks, head, dev)) + [_device_bytes(BGZF_EOF, dev)]
            return torch.cat(parts) if len(parts) > 1 else parts[0]
        parts = [b for b in blocks if b.numel()]
        if head:
            parts.insert(0, _device_bytes(head, dev))
        return torch.cat(parts) if len(parts) > 1 else parts[0] if parts else torch.empty(0, dtype=torch.uint8, device=dev)

    def _write_file(self, path, fmt, context, head, block_rows, compress=False, index=None):
        """the header, then every block of text: one device-to-host copy into a pinned buffer each, appended to the file.  ``compress``: the
        header and every block are BGZF members by then (k_deflate), and one EOF member ends the file.  ``index``: a tabix configuration;
        every piece of text is fed to the indexer on its way to the deflate, the member table is walked from the compressed bytes as
        they pass, and ``path + ".tbi"`` is written behind the file.  A refused row lets the data file finish, then raises"""
        import torch
        if index is not None and not compress:
            raise MdkError("index=True needs compress=True: a tabix index is the index of a BGZF file")
        write, blocks, ix = _file_writer(), self._text_blocks(fmt, context, block_rows), None
        try:
            if compress:
                dev = getattr(self, self.COLUMNS[0][0]).device
                if index is not None:
                    ix = _TabixIndexer(path, index, dev)
                blocks, head, tail = self._compressed(blocks, head, dev, ix.feed if ix else None), b"", BGZF_EOF
            else:
                tail = b""
            with open(path, "wb") as f:
                f.write(head)
                at = len(head)
                for b in blocks:
                    at += write(f, b, (lambda view: ix.members_of(view, at)) if ix else None)        # (the indexer sees a member before it is written)
                f.write(tail)
            if ix:
                ix.finish()
        finally:
            if ix:
                ix.close()
        return path


# ---- text read back into columns (include/mdk_hip.h md_text_parse_*, csrc/mdk_parse.hip): Calls.read, Cytosines.read ----
def _reference_lib():
    L = lib_extract()
    if not getattr(L, "_reference_types", False):
        L.mdk_reference_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.mdk_reference_n_contigs.argtypes = [C.c_void_p]
        L.mdk_reference_name.argtypes = [C.c_void_p, C.c_int]; L.mdk_reference_name.restype = C.c_char_p
        L.mdk_reference_length.argtypes = [C.c_void_p, C.c_int]; L.mdk_reference_length.restype = C.c_int64
        L.mdk_reference_bases.argtypes = [C.c_void_p, C.c_int]; L.mdk_reference_bases.restype = C.c_void_p
        L.mdk_reference_free.argtypes = [C.c_void_p]; L.mdk_reference_free.restype = None
        L._reference_types = True
    return L


class Reference:
    """A FASTA in host memory, read by the reader every command uses: ``contigs`` (names, file order) and ``lengths``.  What
    ``Calls.read`` looks a bedGraph line's strand and context up in: the bases go to a device once, at the first read there, and stay with
    this object's renderer for that device, so many files share one upload.  ``close()`` gives the host copy and the device copies back."""

    def __init__(self, path):
        self._L, self._h, self._text = _reference_lib(), C.c_void_p(), {}
        self.path = os.fspath(path)
        if self._L.mdk_reference_load(os.fsencode(self.path), C.byref(self._h)):
            self._h = None
            raise MdkError(f"cannot read the reference {self.path}")
        n = self._L.mdk_reference_n_contigs(self._h)
        self.contigs = [os.fsdecode(self._L.mdk_reference_name(self._h, i)) for i in range(n)]
        self.lengths = [int(self._L.mdk_reference_length(self._h, i)) for i in range(n)]

    def bases(self, i):
        """the bases of contig ``i`` as bytes, case as in the file"""
        if self._h is None:
            raise MdkError("the reference is closed")
        return C.string_at(self._L.mdk_reference_bases(self._h, i), self.lengths[i]) if self.lengths[i] else b""

    def _renderer(self, device):
        """this reference's md_text on ``device``: its names and, uploaded here at the first use, its bases"""
        if self._h is None:
            raise MdkError("the reference is closed")
        device = int(device)
        if device not in self._text:
            L = _text_lib()
            r = _TextRenderer(L, device, self.contigs)
            for i, n in enumerate(self.lengths):
                rc = L.md_text_reference(r.h, i, C.c_void_p(self._L.mdk_reference_bases(self._h, i)), n)
                if rc:
                    raise _rc_error("md_text_reference", rc, L.md_dev_last_error().decode())
            self._text[device] = r
        return self._text[device]

    def close(self):
        self._text = {}
        if self._h is not None:
            self._L.mdk_reference_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _parse_block_bytes(block_bytes):
    block_bytes = int(block_bytes or os.environ.get("MDK_PARSE_BLOCK_BYTES") or PARSE_BLOCK_BYTES)        # (the variable is a test hook)
    if not 1 <= block_bytes <= (1 << 31) - 1:
        raise MdkError("block_bytes must be between 1 and 2^31 - 1")
    return block_bytes


def _parse_device(device):
    """the torch device of a read; without a GPU an MdkError: there is no CPU path"""
    import torch
    if lib_hip().md_dev_count() <= 0 or not torch.cuda.is_available():
        raise MdkError("files are parsed on the device: no device is visible, and there is no CPU path")
    return torch.device("cuda", int(device))


def _last_newline(view, end):
    """the index of the last newline byte in view[:end], or -1 (searched backwards, 64 KiB at a time)"""
    while end > 0:
        lo = max(0, end - 65536)
        k = bytes(view[lo:end]).rfind(b"\n")
        if k >= 0:
            return lo + k
        end = lo
    return -1


def _parse_pieces(path, block_bytes):
    """(pinned uint8 tensor, bytes in it, offset in the file) for every piece of the file: at most ``block_bytes`` bytes, cut after its last
    newline or at the end of the file.  The tensor is reused: a piece is consumed before the next is asked for"""
    import torch
    size = os.path.getsize(path)
    pin = torch.empty(max(1, min(block_bytes, size)), dtype=torch.uint8, pin_memory=True)
    buf = pin.numpy()
    view = memoryview(buf)
    cap, keep, at = pin.numel(), 0, 0
    with open(path, "rb", buffering=0) as f:
        while True:
            end, eof = keep, False
            while end < cap:
                got = f.readinto(view[end:cap])
                if not got:
                    eof = True
                    break
                end += got
            if not eof and end == cap and size <= cap:
                eof = True                                   # the whole file is in the buffer
            if end == 0:
                return
            cut = end if eof else _last_newline(view, end) + 1
            if cut == 0:
                raise MdkError(f"{path}: a line longer than block_bytes ({block_bytes}) at byte {at}")
            yield pin, cut, at
            keep = end - cut
            if keep:
                buf[:keep] = buf[cut:end].copy()
            at += cut
            if eof and not keep:
                return


def _parse_line_number(path, offset):
    """the 1-based number of the line that holds byte ``offset`` of the file: the error path counts newlines on the host"""
    n, left = 1, offset
    with open(path, "rb") as f:
        while left > 0:
            b = f.read(min(left, 1 << 24))
            if not b:
                break
            n += b.count(b"\n"); left -= len(b)
    return n


def _parse_text(L, text, d, n, path, at, fmt, columns, dev, line_number):
    """the columns of the ``n`` bytes of text at the start of the device tensor ``d`` (the file's decompressed bytes from ``at``)"""
    import torch
    fill = L.md_text_parse_fill_cytosines if fmt == PARSE_CYTOSINE_REPORT else L.md_text_parse_fill_calls
    rows = C.c_int64()
    rc = L.md_text_parse_measure(text.h, C.c_void_p(d.data_ptr()), n, fmt, C.byref(rows))
    if rc:
        raise _rc_error("md_text_parse_measure", rc, L.md_dev_last_error().decode())
    cols = {name: torch.empty(rows.value * (3 if name == "trinucleotide" else 1), dtype=getattr(torch, dt), device=dev) for name, dt in columns}
    rc = fill(text.h, C.byref(md_text_cols(*[C.c_void_p(cols[name].data_ptr()) for name, _ in columns])), rows.value)
    if rc:
        detail, off = L.md_dev_last_error().decode(), int(L.md_text_parse_error_offset(text.h))
        if off >= 0:
            detail = f"{path}, line {line_number(path, at + off)}: {detail}"
        else:
            detail = f"{path}: {detail}"
        raise _rc_error("reading", rc, detail)
    return cols


def _parse_file(L, text, path, fmt, columns, dev, block_bytes):
    """the columns of one file, a list of dicts (one per piece), parsed on ``dev`` by k_parse_len / k_parse_fill.  A file that begins with
    the gzip magic is a BGZF file or refused (``_gz_kind``): its members are inflated on the device and parsed where they lie"""
    import torch
    kind = _gz_kind(path)
    if kind == "gzip":
        raise MdkError(f"{path}: a gzip file that is not BGZF (no BC subfield in its header): one member of any length is one wavefront's work. "
                       "Recompress it with bgzip (zcat file.gz | bgzip > file.bgz.gz), or decompress it")
    if kind == "bgzf":
        return _parse_bgzf(L, text, path, fmt, columns, dev, block_bytes)
    out = []
    for pin, n, at in _parse_pieces(path, block_bytes):
        d = torch.empty(n, dtype=torch.uint8, device=dev)
        d.copy_(pin[:n], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()             # the text is complete, and the pinned buffer may take the next piece
        out.append(_parse_text(L, text, d, n, path, at, fmt, columns, dev, _parse_line_number))
    return out


# ---- BGZF files read back (csrc/mdk_inflate.hip md_piece_*: the members are inflated and CRC32-checked on the device) ----
def _bgzf_bsize(buf, o, end):
    """the length of the BGZF member whose header stands at ``buf[o]`` -- the gzip magic, deflate, FLG = FEXTRA alone and a BC subfield of
    two bytes, which is BSIZE -- or 0: no such header there (or not all of it before ``end``)"""
    if o + 12 > end or buf[o] != 0x1f or buf[o + 1] != 0x8b or buf[o + 2] != 8 or buf[o + 3] != 4:
        return 0
    x, xe = o + 12, o + 12 + (buf[o + 10] | buf[o + 11] << 8)
    if xe > end:
        return 0
    while x + 4 <= xe:
        slen = buf[x + 2] | buf[x + 3] << 8
        if buf[x] == 66 and buf[x + 1] == 67 and slen == 2 and x + 6 <= xe:
            return (buf[x + 4] | buf[x + 5] << 8) + 1
        x += 4 + slen
    return 0


def _gz_kind(path):
    """what a file is by its content, not its name: "plain" (no gzip magic), "bgzf" (a BGZF header first) or "gzip" (any other gzip file)"""
    with open(path, "rb") as f:
        h = f.read(12 + 65535)
    if len(h) < 2 or h[0] != 0x1f or h[1] != 0x8b:
        return "plain"
    return "bgzf" if _bgzf_bsize(h, 0, len(h)) else "gzip"


def _bgzf_members(path, buf):
    """the member table of a BGZF file (``buf``: its bytes, a buffer), as the host walks a BAM's (csrc/host/mdk_io.c): [(file offset, stream
    offset, stream length, ISIZE, CRC32)], empty members -- the EOF member is one -- left out.  A last member that is cut short, bytes that
    are no BGZF header where one must stand and an ISIZE above 65536 raise MdkError; a missing EOF member does not (htslib warns and reads on)"""
    out, o, end = [], 0, len(buf)
    while o < end:
        bs = _bgzf_bsize(buf, o, end)
        if not bs:
            if end - o < 18 or (buf[o] == 0x1f and buf[o + 1] == 0x8b and buf[o + 2] == 8 and buf[o + 3] == 4 and o + 12 + (buf[o + 10] | buf[o + 11] << 8) > end):
                raise MdkError(f"{path}: the file is cut short inside the header of its last member (at byte {o})")
            raise MdkError(f"{path}: no BGZF member at byte {o}: a gzip member without a BC subfield, or not gzip at all")
        xlen = buf[o + 10] | buf[o + 11] << 8
        if o + bs > end:
            raise MdkError(f"{path}: the file is cut short inside its last member (at byte {o}: {bs} bytes by its header, {end - o} in the file)")
        if bs < 12 + xlen + 8:
            raise MdkError(f"{path}: the member at byte {o} is shorter than its own header and trailer")
        crc, isz = struct.unpack_from("<II", buf, o + bs - 8)
        if isz > 65536:
            raise MdkError(f"{path}: the member at byte {o} inflates to {isz} bytes: a BGZF member holds at most 65536")
        if isz:
            out.append((o, o + 12 + xlen, bs - 12 - xlen - 8, isz, crc))
        o += bs
    return out


def _gz_line_number(path, offset):
    """the 1-based number of the line that holds byte ``offset`` of the decompressed text: the error path inflates on the host and counts newlines"""
    import gzip
    n, left = 1, offset
    with gzip.open(path, "rb") as f:
        while left > 0:
            b = f.read(min(left, 1 << 24))
            if not b:
                break
            n += b.count(b"\n"); left -= len(b)
    return n


def _device_last_newline(d, end):
    """the index of the last newline in the device tensor ``d[:end]``, or -1 (searched backwards, 64 KiB at a time; one index crosses to the host)"""
    while end > 0:
        lo = max(0, end - 65536)
        k = (d[lo:end] == 10).nonzero()
        if k.numel():
            return lo + int(k[-1])
        end = lo
    return -1


def _parse_bgzf(L, text, path, fmt, columns, dev, block_bytes):
    """``_parse_file`` for a BGZF file.  The host walks the headers into a member table; pieces of whole members -- at most ``block_bytes``
    inflated bytes each, and at least one member -- go to the device through md_piece_submit (k_inflate, k_crc32), and their bytes are
    parsed there.  bgzip cuts members every 65280 bytes, not at newlines: the bytes behind a piece's last newline stay on the device and
    go in front of the next piece's.  No decompressed byte crosses to the host"""
    import contextlib
    import mmap
    out = []
    if os.path.getsize(path) == 0:
        return out
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as buf:
        with contextlib.closing(_bgzf_pieces(L, path, buf, _bgzf_members(path, buf), dev, block_bytes)) as pieces:
            for d, cut, at in pieces:
                out.append(_parse_text(L, text, d, cut, path, at, fmt, columns, dev, _gz_line_number))
    return out


def _bgzf_pieces(L, path, buf, members, dev, block_bytes, drop=0, limit=None):
    """the text of ``members`` (entries of ``_bgzf_members`` that follow each other in ``buf``, the file's bytes) as pieces of whole lines: a
    generator of (device tensor, the bytes at its start that are the piece, their offset in the text).  ``_parse_bgzf``'s pieces; a region
    read gives the members of one chunk, with ``drop`` bytes of the first member left out in front (the text begins there) and the text
    ended after ``limit`` bytes"""
    import re
    import torch
    cfg = md_dev_cfg(); cfg.keepCpG = 1; cfg.minPhred = 5          # (a handle for the pieces: none of its settings touches the inflate)
    handle, piece, stage, stage_cap = Device(cfg, device=dev.index or 0), C.c_void_p(), None, 0
    try:
        rc = L.md_piece_create(handle.h, C.byref(piece))
        if rc:
            raise _rc_error("md_piece_create", rc, L.md_dev_last_error().decode())
        tail, at, k = torch.empty(0, dtype=torch.uint8, device=dev), 0, 0
        while k < len(members) and (limit is None or at + tail.numel() < limit):
            k1, inflated = k, 0
            while k1 < len(members) and (k1 == k or inflated + members[k1][3] <= block_bytes):
                inflated += members[k1][3]; k1 += 1
            c0, c1 = members[k][1], members[k1 - 1][1] + members[k1 - 1][2]
            if c1 - c0 + 64 > stage_cap:
                if stage:
                    L.md_host_free(C.c_void_p(stage))
                stage_cap = c1 - c0 + (c1 - c0) // 8 + 64
                stage = L.md_host_alloc(stage_cap)
                if not stage:
                    raise MdkError("no pinned memory for a piece of the file")
            C.memmove(stage, buf[c0:c1], c1 - c0)
            tab, o = (md_inf_member * (k1 - k))(), 0
            for i in range(k, k1):
                _, so, sl, isz, crc = members[i]
                t = tab[i - k]
                t.in_off, t.in_len, t.out_len, t.out_off, t.crc32 = so - c0, sl, isz, o, crc
                o += isz
            info = md_piece_info()
            rc = L.md_piece_submit(piece, C.c_void_p(stage), c1 - c0, tab, k1 - k)
            if not rc:
                rc = L.md_piece_wait(piece, C.byref(info))
            if rc:
                detail = L.md_dev_last_error().decode()
                m = re.search(r"member (\d+) of the piece", detail)
                if m and int(m.group(1)) < k1 - k:
                    detail = f"the member at byte {members[k + int(m.group(1))][0]} of the file: {detail}"
                raise _rc_error("reading", rc, f"{path}: {detail}")
            keep, skip = tail.numel(), drop if k == 0 else 0
            take = max(0, inflated - skip)
            if limit is not None:
                take = min(take, limit - at - keep)
            d = torch.empty(keep + take, dtype=torch.uint8, device=dev)
            d[:keep] = tail
            torch.cuda.current_stream(dev).synchronize()         # the carried bytes are in place before the piece's are put behind them
            if take:
                rc = L.md_piece_copy(piece, skip, take, C.c_void_p(d.data_ptr() + keep))
                if rc:
                    raise _rc_error("md_piece_copy", rc, L.md_dev_last_error().decode())
            end = keep + take
            cut = end if k1 == len(members) or (limit is not None and at + end >= limit) else _device_last_newline(d, end) + 1
            if cut == 0:
                raise MdkError(f"{path}: a line longer than block_bytes ({block_bytes}) at byte {at} of the decompressed text")
            tail = d[cut:end].clone()
            torch.cuda.current_stream(dev).synchronize()
            yield d, cut, at
            at += cut; k = k1
    finally:
        if piece:
            L.md_piece_destroy(piece)
        if stage:
            L.md_host_free(C.c_void_p(stage))
        handle.close()


# ---- the side libraries: index, stats, smooth, cohort, track.  Each is one .hip file built into a .so of its own (csrc/mdk_side.hpp is
# the host layer they share), loaded at the first call that needs it: its code object's load is paid there and by no command ----
_side_handles = {}                                             # (library, device) -> its md_X handle, opened at the first use and kept
_side_locks = {name: threading.Lock() for name in ("stats", "smooth", "cohort", "track")}      # a handle's calls come from one thread at a time


def _load_side(name, path, noun):
    """``path`` as a CDLL with what every side library has: md_<name>_last_error, md_<name>_open(device, &handle), md_<name>_close"""
    if not path.exists():
        raise MdkError(f"{path} is missing: the {noun} library was not built (run `make` / __graft_entry__.build()); there is no fallback")
    L = C.CDLL(str(path))
    getattr(L, f"md_{name}_last_error").restype = C.c_char_p
    getattr(L, f"md_{name}_open").argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    close = getattr(L, f"md_{name}_close")
    close.argtypes, close.restype = [C.c_void_p], None
    return L


def _side_call(L, name, f, *args):
    """md_<name>_<f>(*args); a return code other than 0 raises with the library's text (the caller still holds the handle's lock)"""
    rc = getattr(L, f"md_{name}_{f}")(*args)
    if rc:
        raise _rc_error(f"md_{name}_{f}", rc, getattr(L, f"md_{name}_last_error")().decode())


def _side_handle(L, name, device):
    """the device's md_<name>, opened at its first use and kept; the caller holds ``_side_locks[name]``"""
    h = _side_handles.get((name, device))
    if h is None:
        h = C.c_void_p()
        _side_call(L, name, "open", device, C.byref(h))
        _side_handles[name, device] = h
    return h


def _side_limits(L, name, device, *limits):
    """md_<name>_limits on the device's handle: what ``smooth_limits``, ``cohort_limits`` and ``track_limits`` do"""
    with _side_locks[name]:
        _side_call(L, name, "limits", _side_handle(L, name, int(device)), *map(int, limits))


def _device_bytes(data, dev):
    """``data`` (bytes) as a uint8 tensor on ``dev``"""
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)


def _file_writer():
    """``write(f, t, seen=None)``: the device tensor ``t`` appended to the open file ``f`` through one pinned buffer, kept between the calls
    and grown by an eighth past the largest tensor: one copy to the host, waited for, then ``seen(bytes)`` if given, then the write.
    Returns the bytes written"""
    import torch
    pin = None

    def write(f, t, seen=None):
        nonlocal pin
        k = t.numel()
        if not k:
            return 0
        if pin is None or pin.numel() < k:
            pin = torch.empty(k + k // 8, dtype=torch.uint8, pin_memory=True)
        pin[:k].copy_(t, non_blocking=True)
        torch.cuda.current_stream(t.device).synchronize()
        view = memoryview(pin.numpy())[:k]
        if seen:
            seen(view)
        f.write(view)
        return k
    return write


# ---- tabix indexes (include/mdk_index.h, csrc/mdk_tabix.hip -> libmdk_index.so; the rule is csrc/mdk_tabix_core.h) ----
TABIX_UCSC = 0x10000
TABIX_PRESETS = {"bed": (TABIX_UCSC, 1, 2, 3, ord("#")), "methylKit": (0, 2, 3, 3, ord("#")), "cytosine_report": (0, 1, 2, 2, ord("#"))}
_index = None


class md_index_conf(C.Structure):
    _fields_ = [("format", C.c_int32), ("col_seq", C.c_int32), ("col_beg", C.c_int32), ("col_end", C.c_int32), ("meta", C.c_int32), ("skip", C.c_int32)]


class md_index_member(C.Structure):
    _fields_ = [("c_off", C.c_uint64), ("u_off", C.c_uint64), ("isize", C.c_uint32), ("pad", C.c_uint32)]


def lib_index():
    """libmdk_index.so, loaded at the first index call: its code object's load is paid there and by no command"""
    global _index
    if _index is None:
        L = _load_side("index", LIB_INDEX, "index")
        L.md_index_open.argtypes = [C.c_int, C.POINTER(md_index_conf), C.POINTER(C.c_void_p)]
        L.md_index_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.md_index_refusal.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.md_index_finish.argtypes = [C.c_void_p, C.POINTER(md_index_member), C.c_int64, C.c_uint64, C.POINTER(C.c_int64)]
        L.md_index_payload.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.md_index_count.argtypes = [C.c_void_p, C.c_int]; L.md_index_count.restype = C.c_int64
        _index = L
    return _index


def _tabix_conf(preset, skip):
    if preset not in TABIX_PRESETS:
        raise MdkError(f"unknown preset {preset!r}: one of {', '.join(TABIX_PRESETS)}")
    skip = int(skip)
    if not 0 <= skip <= 2 ** 31 - 1:
        raise MdkError("skip must be between 0 and 2^31 - 1")
    return TABIX_PRESETS[preset] + (skip,)


class _TabixIndexer:
    """one md_index: the text of the data file ``path`` is fed piece by piece (device tensors of whole lines), the members that hold bytes
    are noted as the compressed bytes pass, and ``finish`` writes ``path + ".tbi"``: the payload through ``bgzf_compress``"""

    def __init__(self, path, conf, dev):
        self.L, self.h, self.path, self.dev = lib_index(), C.c_void_p(), path, dev
        self.members, self.u, self.c_end, self.error, self.counts = [], 0, 0, None, None
        if os.path.exists(path + ".tbi"):
            os.remove(path + ".tbi")                                 # (an index of the file that stood here before is the index of another file)
        rc = self.L.md_index_open(dev.index or 0, C.byref(md_index_conf(*conf)), C.byref(self.h))
        if rc:
            self.h = None
            raise _rc_error("md_index_open", rc, self.L.md_index_last_error().decode())

    def feed(self, t):
        import torch
        if self.error is not None or not t.numel():
            return
        torch.cuda.current_stream(t.device).synchronize()            # the text is complete
        rc = self.L.md_index_feed(self.h, C.c_void_p(t.data_ptr()), t.numel())
        if rc == 1:
            self.error = _rc_error("indexing", -3, f"{self.path}, {self.L.md_index_last_error().decode()}: no tabix index is written")
        elif rc:
            raise _rc_error("md_index_feed", rc, self.L.md_index_last_error().decode())

    def members_of(self, buf, at):
        """the members in ``buf``, whole BGZF members that stand at byte ``at`` of the file"""
        o, end = 0, len(buf)
        while o < end:
            if o + 18 <= end and buf[o + 12:o + 16] == b"BC\x02\x00" and buf[o:o + 4] == b"\x1f\x8b\x08\x04":      # k_deflate's header: BSIZE stands at 16
                bs = (buf[o + 16] | buf[o + 17] << 8) + 1
            else:
                bs = _bgzf_bsize(buf, o, end)
            if not bs or o + bs > end:
                raise MdkError(f"{self.path}: no whole BGZF member at byte {at + o}")
            self.member(at + o, bs, struct.unpack_from("<I", buf, o + bs - 4)[0])
            o += bs

    def member(self, c, bs, isize):
        if isize:
            self.members.append((c, self.u, isize))
            self.u += isize; self.c_end = c + bs

    def finish(self):
        import torch
        if self.error is not None:
            raise self.error
        tab, size = (md_index_member * max(1, len(self.members)))(), C.c_int64()
        for t, (c, u, n) in zip(tab, self.members):
            t.c_off, t.u_off, t.isize = c, u, n
        rc = self.L.md_index_finish(self.h, tab, len(self.members), self.c_end, C.byref(size))
        if rc:
            raise _rc_error("md_index_finish", rc, f"{self.path}: {self.L.md_index_last_error().decode()}")
        payload = bytearray(size.value)
        _side_call(self.L, "index", "payload", self.h, (C.c_char * size.value).from_buffer(payload), size.value)
        self.counts = {k: int(self.L.md_index_count(self.h, i)) for i, k in enumerate(("lines", "entries", "records", "names", "pieces"))}
        data = bgzf_compress(_device_bytes(payload, self.dev))
        with open(self.path + ".tbi", "wb") as f:
            f.write(bytes(data.cpu().numpy()))
        return self.path + ".tbi"

    def close(self):
        if self.h:
            self.L.md_index_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tabix_index(path, preset="bed", skip=None, device=0, block_bytes=None):
    """``path + ".tbi"``: the tabix index of any BGZF table -- ``write(compress=True)``'s, bgzip's, last week's, the command line's output
    compressed afterwards --, what `tabix -p bed` would be run for.  The file's members are inflated and CRC32-checked on the device in
    pieces (as ``Calls.read`` reads them), every line is parsed there (csrc/mdk_tabix.hip), and the few records that are left become the
    index on the host; it is written as BGZF made on the device.  ``preset``: "bed" (columns 1, 2, 3, 0-based half-open: the bedGraph,
    --fraction and --counts files), "methylKit" (columns 2 and 3) or "cytosine_report" (columns 1 and 2).  ``skip``: the number of lines
    at the file's start that are no rows; by default 1 for a methylKit file, 0 for a report and, for "bed", 1 if the text begins with
    `track`.  Lines that begin with '#' are passed over.  The bytes of the index depend on the data file alone (csrc/mdk_tabix_core.h
    fixes what the specification leaves open).  Refused, with MdkError naming the path and the line, and no .tbi left behind: rows that
    are not sorted by (contig, begin), a contig that appears in two places, an interval past 2^29 (a .tbi ends at 512 Mb; CSI is not
    written), malformed coordinates, lines longer than 512 bytes, empty lines; and, as ``Calls.read`` refuses it, a gzip file that is
    not BGZF.  perRead files, ``Regions`` / ``Diff`` / ``Dmrs`` files and the `MethylDackel` command line are out of scope.  Returns
    the index's path.  There is no CPU path."""
    import contextlib
    import mmap
    import zlib
    path = os.fsdecode(path)
    dev = _parse_device(device)
    block_bytes = _parse_block_bytes(block_bytes)
    kind = _gz_kind(path)
    if kind != "bgzf":
        raise MdkError(f"{path}: " + ("a gzip file that is not BGZF (no BC subfield in its header): recompress it with bgzip" if kind == "gzip" else
                                      "not a BGZF file: a tabix index is the index of a BGZF file (write(compress=True), bgzip)"))
    L = _text_lib()
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as buf:
        members = _bgzf_members(path, buf)
        if skip is None:
            skip = {"methylKit": 1, "cytosine_report": 0}.get(preset)
            if skip is None:
                first = b""                                          # the text's first five bytes: members may be as short as one byte
                for _, so, sl, _, _ in members:
                    if len(first) >= 5:
                        break
                    first += zlib.decompress(buf[so:so + sl], -15)
                skip = 1 if first[:5] == b"track" else 0
        ix = _TabixIndexer(path, _tabix_conf(preset, skip), dev)
        try:
            for o, so, sl, isz, _ in members:
                ix.member(o, so + sl + 8 - o, isz)
            with contextlib.closing(_bgzf_pieces(L, path, buf, members, dev, block_bytes)) as pieces:
                for d, cut, _ in pieces:
                    ix.feed(d[:cut])
            return ix.finish()
        finally:
            ix.close()


def _tabix_chunks(path, name, beg, end):
    """the chunks of the .tbi ``path`` that may hold a line overlapping name:[beg, end), as [[begin, end]] virtual offsets, ascending,
    neighbours joined: those of the region's bins (reg2bins of the specification) that end above the linear index's offset for the
    region's first window.  The index is read on the host (it is small, and the gzip module does); only the asked name's bins are
    looked at, with numpy where every bin has one chunk, as the bins of ``write``'s and ``tabix_index``'s files have"""
    import gzip
    import zlib
    import numpy as np
    try:
        with open(path, "rb") as f:
            p = gzip.decompress(f.read())
    except FileNotFoundError:
        raise MdkError(f"{path}: no tabix index: a region is read through the index (write(..., compress=True, index=True), tabix_index)") from None
    except (OSError, EOFError, zlib.error) as e:
        raise MdkError(f"{path}: not a tabix index: {e}") from None
    try:
        if p[:4] != b"TBI\x01":
            raise ValueError("no TBI magic")
        n_ref, l_nm = struct.unpack_from("<i", p, 4)[0], struct.unpack_from("<i", p, 32)[0]
        names, o = [os.fsdecode(x) for x in p[36:36 + l_nm].split(b"\0")[:-1]], 36 + l_nm
        if len(names) != n_ref:
            raise ValueError("the names do not match n_ref")
        if name not in names:
            return []
        tid, wanted, found, head = names.index(name), _tabix_bins(beg, end), [], struct.Struct("<Ii").unpack_from
        for t in range(tid + 1):
            n_bin, = struct.unpack_from("<i", p, o); o += 4
            k = 0
            if n_bin > 1 and o + 24 * (n_bin - 1) <= len(p):
                words = np.frombuffer(p, dtype="<u4", count=6 * (n_bin - 1), offset=o)
                if bool((words[1::6] == 1).all()):               # one chunk in each of the first n_bin - 1 bins: they stand 24 bytes apart
                    k = n_bin - 1
                    if t == tid:
                        for i in np.nonzero(np.isin(words[0::6], np.asarray(wanted, dtype=np.uint32)))[0].tolist():
                            found.append(struct.unpack_from("<QQ", p, o + 24 * i + 8))
                    o += 24 * k
            wanted_set = set(wanted) if t == tid and k < n_bin else ()
            for _ in range(k, n_bin):
                b, n_chunk = head(p, o); o += 8
                if n_chunk < 0:
                    raise ValueError("a negative chunk count")
                if b in wanted_set:
                    found += [struct.unpack_from("<QQ", p, o + 16 * c) for c in range(n_chunk)]
                o += 16 * n_chunk
            n_intv, = struct.unpack_from("<i", p, o); o += 4
            if t == tid:
                if beg >> 14 >= n_intv:
                    return []
                low, = struct.unpack_from("<Q", p, o + 8 * (beg >> 14))
            o += 8 * n_intv
            if o > len(p):
                raise ValueError("cut short")
    except (struct.error, ValueError) as e:
        raise MdkError(f"{path}: not a tabix index: {e}") from None
    chunks = []
    for vb, ve in sorted(ch for ch in found if ch[1] > low):
        if chunks and vb <= chunks[-1][1]:
            chunks[-1][1] = max(chunks[-1][1], ve)
        else:
            chunks.append([vb, ve])
    return chunks


def _tabix_bins(beg, end):
    """the bins that may hold an interval overlapping [beg, end): reg2bins of the specification"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def _region_check(region):
    try:
        name, beg, end = region
        beg, end = int(beg), int(end)
    except (TypeError, ValueError):
        raise MdkError("region must be (name, beg, end): a contig name and a 0-based half-open interval") from None
    if not 0 <= beg < end:
        raise MdkError("region must be (name, beg, end) with 0 <= beg < end")
    return str(name), beg, min(end, 1 << 29)


def _parse_region(L, text, path, fmt, columns, dev, block_bytes, region, stats):
    """``_parse_file`` for the lines a tabix index says may overlap ``region``: the chunks of the region's bins that end above the linear
    index's offset for the region's first window, neighbours joined; of the file only the members those chunks span are inflated, and only
    the text between a chunk's begin and end is parsed; the member headers of those chunks alone are walked.  ``stats`` takes the count
    of members inflated"""
    import contextlib
    import mmap
    if isinstance(path, (list, tuple)):
        raise MdkError("a region is read from one file: every file has an index of its own")
    path = os.fsdecode(path)
    name, beg, end = region
    kind = _gz_kind(path)
    if kind != "bgzf":
        raise MdkError(f"{path}: a region is read through a tabix index, which only a BGZF file has (write(..., compress=True, index=True))")
    chunks = _tabix_chunks(path + ".tbi", name, beg, end)
    out, stats["members_inflated"] = [], 0
    if not chunks:
        return out
    misfit = MdkError(f"{path}.tbi: the index does not fit the file: no member where a chunk begins or ends. Index it again (tabix_index)")
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as buf:
        for vb, ve in chunks:
            c0, c1 = vb >> 16, ve >> 16
            if ve & 0xffff:                                           # the chunk ends inside the member at c1: that member too
                bs = _bgzf_bsize(buf, c1, len(buf)) if c1 < len(buf) else 0
                if not bs:
                    raise misfit
                c1 += bs
            if not c0 < c1 <= len(buf) or not _bgzf_bsize(buf, c0, len(buf)):
                raise misfit
            members = [(c0 + o, c0 + so, sl, isz, crc) for o, so, sl, isz, crc in _bgzf_members(path, buf[c0:c1])]      # the chunk's members alone are walked
            if not members or members[0][0] != c0 or vb & 0xffff >= members[0][3] or (ve & 0xffff and (members[-1][0] != ve >> 16 or ve & 0xffff > members[-1][3])):
                raise misfit
            limit = sum(m[3] for m in members) - (vb & 0xffff) - (members[-1][3] - (ve & 0xffff) if ve & 0xffff else 0)
            stats["members_inflated"] += len(members)
            with contextlib.closing(_bgzf_pieces(L, path, buf, members, dev, block_bytes, drop=vb & 0xffff, limit=limit)) as pieces:
                for d, cut, at in pieces:
                    out.append(_parse_text(L, text, d, cut, path, at, fmt, columns, dev, lambda p, o, vb=vb: _region_line_number(p, vb, o)))
    return out


def _region_line_number(path, vb, offset):
    """the 1-based line that holds the byte ``offset`` bytes behind virtual offset ``vb``: the error path walks the file on the host"""
    import gzip
    with open(path, "rb") as f:
        raw = f.read()
    before = gzip.decompress(raw[:vb >> 16]) if vb >> 16 else b""
    return _gz_line_number(path, len(before) + (vb & 0xffff) + offset)


def _parse_cat(pieces, columns, dev):
    import torch
    cols = {}
    for name, dt in columns:
        parts = [p[name] for p in pieces]
        cols[name] = parts[0] if len(parts) == 1 else torch.cat(parts) if parts else torch.empty(0, dtype=getattr(torch, dt), device=dev)
    return cols


def _contexts_present(context):
    import torch
    return tuple(int(k) for k in torch.unique(context).cpu().tolist())


class Calls(_Columns):
    """The rows `extract` would print, as columns (one entry per call, in the order of the chunks of the schedule; within a context,
    ascending `start`): ``contig`` (int32, index into ``contigs``, BAM header order), ``start``/``end`` (int32, bedGraph columns 2-3),
    ``nmeth``/``nunmeth`` (int32), ``context`` (uint8: 0 CpG, 1 CHG, 2 CHH) and ``strand`` (int8: +1 C, -1 G, 0 a --mergeContext row)."""
    COLUMNS = CALL_COLUMNS
    KIND = "calls"

    def __init__(self, contigs, columns, merged=False, contexts_on=(0, 1, 2)):
        super().__init__(contigs, columns)
        self.merged = bool(merged)                  # --mergeContext was on: the bedGraph headers say " merged"
        self.contexts_on = tuple(contexts_on)       # the contexts switched on (0 CpG, 1 CHG, 2 CHH): `write` makes a file for each, rows or not

    @classmethod
    def _build(cls, L, out, cols):
        c = super()._build(L, out, cols)
        c.merged = L.mdk_calls_merged(out) == 1
        c.contexts_on = tuple(k for k in range(3) if L.mdk_calls_contexts(out) >> k & 1)
        return c

    @staticmethod
    def _format(fmt):
        if fmt == "logit":
            raise _rc_error("rendering --logit", RC_UNSUPPORTED, "its value goes through log(), which neither the host's nor the device's library rounds correctly: the command's bytes cannot be promised")
        if fmt not in TEXT_FORMATS:
            raise MdkError(f"unknown format {fmt!r}: one of {', '.join(TEXT_FORMATS)}")
        return TEXT_FORMATS[fmt]

    def header(self, fmt, context, prefix):
        """the first line of the command's file for that format and context (csrc/host/mdk_plan.c), as bytes"""
        code = self._format(fmt)
        if fmt == "methylKit":
            return b"chrBase\tchr\tbase\tstrand\tcoverage\tfreqC\tfreqT\n"
        if prefix is None:
            raise MdkError("the bedGraph header quotes the output prefix: give prefix=, or header=False")
        return f'track type="bedGraph" description="{prefix} {CONTEXT_FILES[context]}{" merged" if self.merged else ""} methylation {TEXT_WHAT[code]}"\n'.encode()

    def render(self, fmt="bedGraph", context=0, prefix=None, header=True, block_rows=None, compress=False):
        """The bytes of the file `extract -o prefix` writes for one context (0 CpG, 1 CHG, 2 CHH), as a uint8 tensor on the columns' device,
        made there (csrc/mdk_text.hip) from whatever the columns hold now -- the session's rows, or a filtered or re-ordered ``select``.
        ``fmt``: "bedGraph" (the default output), "fraction" (--fraction), "counts" (--counts) or "methylKit" (--methylKit); byte for byte the
        command's text, %f and %6.2f included.  "logit" raises MdkError with rc -23: --logit's value goes through log(), which is not
        correctly rounded on either side, so its bytes cannot be promised.  Rows of other contexts and rows without coverage give no line;
        a methylKit line of a --mergeContext row (strand 0) is an error, as the combination is for the command.  ``header=False`` leaves the
        first line out.  ``compress=True`` gives the bytes of the .gz file instead: BGZF made on the device (``bgzf_compress``), the header
        line and every block of ``block_rows`` rows in members of their own, one EOF member at the end; ``gzip.decompress`` of it is the
        uncompressed result, whatever ``block_rows`` is.  CPU tensors raise MdkError: there is no CPU path."""
        code = self._format(fmt)
        return self._render(code, int(context), self.header(fmt, int(context), prefix) if header else b"", block_rows, compress)

    def write(self, prefix, fmt="bedGraph", directory=None, block_rows=None, compress=False, index=False):
        """The command's file set under the command's names -- <prefix>_CpG.bedGraph, .meth.bedGraph (fraction), .counts.bedGraph,
        .methylKit --, one file per context in ``contexts_on``, header-only where there is no row; in ``directory`` if given.  The text is
        made on the device in blocks of ``block_rows`` rows (default 2^22), each copied to the host once and appended: the extra device and
        pinned memory is one block's text, not the file's.  ``compress=True`` writes BGZF files under the same names with ``.gz`` appended:
        every block is compressed on the device (csrc/mdk_deflate.hip) before its one copy to the host, so about a third of the bytes
        cross; ``gzip``, ``zcat``, ``bgzip -d``, tabix and R read them, and ``gzip.decompress`` gives the uncompressed file byte for byte.
        A header-only file is the header's member and the EOF member.  There are no compression levels.
        ``index=True`` (with ``compress=True``; without it MdkError) writes <file>.gz.tbi next to every .gz: the tabix index methylKit's
        tabix-backed objects, IGV and `tabix file.gz chr2:1-2000000` open first, and the one ``read(region=)`` reads through; for a
        header-only file too (no names in it).  The text is indexed on the device (csrc/mdk_tabix.hip) on its way to the deflate --
        nothing is inflated again --, the member table is walked from the compressed bytes that cross to the host anyway, and the index
        is that of ``tabix_index`` for the same file, byte for byte (the bedGraph kinds as `-p bed` with the header line skipped,
        methylKit by its chr and base columns).  Rows the rule refuses -- out of order after a ``select``, a contig in two places, a row
        past 2^29: a .tbi ends at 512 Mb, and CSI is not written -- raise MdkError (rc -3) with the file and the line after the data
        file is complete, and no .tbi is left behind.
        Returns the paths."""
        code = self._format(fmt)
        gz = ".gz" if compress else ""
        if index and not compress:
            raise MdkError("index=True needs compress=True: a tabix index is the index of a BGZF file")
        conf = _tabix_conf("methylKit" if fmt == "methylKit" else "bed", 1) if index else None
        return [self._write_file(os.path.join(directory, f"{prefix}_{CONTEXT_FILES[k]}{TEXT_SUFFIX[code]}{gz}") if directory is not None else f"{prefix}_{CONTEXT_FILES[k]}{TEXT_SUFFIX[code]}{gz}",
                                 code, k, self.header(fmt, k, prefix), block_rows, compress, conf) for k in self.contexts_on]

    def merge_context(self, min_depth=1):
        """The rows the `mergeContext` command makes of these: a new Calls (``merged`` true, same ``contigs`` and ``contexts_on``, new tensors
        on this one's device) in which a CpG's or CHG's C and G are ONE row -- ``start`` the C, ``end`` one past the G, the counts added,
        ``strand`` 0 --, a C or G whose partner is no row is that row alone, and CHH rows are as they were.  Rows whose nmeth + nunmeth is
        below ``min_depth`` are then dropped (CHH rows too, as `extract -d` does; 0 keeps every row).  Made on the device from the columns
        alone (csrc/mdk_merge.hip): ``context`` and ``strand`` are what the command looks up in the FASTA.  The rows must be strictly
        ascending in (contig, start), as a session returns them and as ``select`` with a mask or an ascending index keeps them; rows in
        another order, rows merged already, a context above 2, a contig index outside ``contigs``, a G without its C closer to the
        contig's start than its site is long, and counts adding up past 2^31 - 1 raise MdkError (rc -3); so do CPU tensors: there is no
        CPU path.  One `extract` run at -d 1 thus gives the per-strand tables, the merged ones at any depth, and the files of both.
        What always holds, at the default ``min_depth``: ``m.write(p)`` is, after the header line, what `MethylDackel mergeContext` prints for the file ``self.write``
        made.  It equals `extract --mergeContext [-d D]` (``min_depth=D``) too, for runs without the variant filter (--minOppositeDepth)
        and without -l: under the first the command zeroes a C's counts when its G is a variant, under the second its pending sites
        never cross a chunk, and rows made afterwards cannot know either."""
        if self.merged:
            raise MdkError("merge_context: these rows are merged already (merged is true)")
        return self._merged([getattr(self, name) for name, _ in CALL_COLUMNS], min_depth)

    def profile(self, by="context", min_depth=1, depth_bins=1024, level_bins=20):
        """The first look at a sample -- methylKit's ``getCoverageStats`` and ``getMethylationStats``: a ``CountProfile`` of these rows as
        one sample, the counts viewed as ``[1, n]`` and not copied, made on the device by ``count_profile``, which documents the rule.
        ``by="context"`` groups the rows by their ``context`` column, three groups named CpG, CHG and CHH -- ``profile().rate()[0, 2]``,
        the methylated fraction of the CHH reads, is the usual estimate of the bisulfite non-conversion rate --; ``by=None`` is one
        group.  The order of the rows does not matter."""
        group, n_groups, group_names = _profile_by(by, self.context)
        return count_profile(self.nmeth.unsqueeze(0), self.nunmeth.unsqueeze(0), group, n_groups, min_depth, depth_bins, level_bins, group_names=group_names)

    def filter_depth(self, lo=10, hi_quantile=0.999, depth_bins=4096):
        """The rows deep enough to trust and not so deep that they are pile-ups of PCR duplicates or repeats -- the place of methylKit's
        ``filterByCoverage(lo.count=10, hi.perc=99.9)``: ``select`` of the rows with ``lo <= nmeth + nunmeth <= hi``, where ``hi`` is
        ``self.profile(min_depth=lo, depth_bins=depth_bins).depth_quantile(hi_quantile)`` of the row's own context -- the percentile
        of the depths of the rows that pass ``lo``, as ``CountProfile.depth_quantile`` defines it in integers: always a depth some
        row has, and not R's interpolated type 7 quantile, from which it may differ by the gap between two neighbouring depths.
        ``hi_quantile=None`` cuts only below.  A percentile at ``depth_bins`` or beyond raises MdkError: raise ``depth_bins``."""
        if isinstance(lo, bool) or not isinstance(lo, int) or not 1 <= lo < 1 << 26:
            raise MdkError(f"filter_depth: lo must be an integer within 1 and 2^26 - 1, not {lo!r}")
        depth = self.nmeth.long() + self.nunmeth.long()
        keep = depth >= lo
        if hi_quantile is not None:
            hi = self.profile("context", lo, depth_bins, 1).depth_quantile(hi_quantile)[0]
            keep &= depth <= hi[self.context.long()]
        return self.select(keep)

    def regions(self, intervals, contexts=None, strand=None, min_depth=1):
        """These rows added up per interval -- CpG islands, promoters, a BED of candidate DMRs, the tiles every DMR tool starts from --: a
        ``Regions`` with, per interval and in the intervals' own order, ``nsites`` (the rows counted), ``nmeth`` and ``nunmeth`` (int64),
        made on the rows' device (csrc/mdk_regions.hip) from the columns as they are: no file, no key per row, no prefix sum per row.
        ``intervals`` is an ``Intervals`` over the same ``contigs`` (on the CPU it is moved to the rows' device); its intervals may come
        in any order and overlap, nest or repeat.  A row belongs to the interval that holds its ``start`` -- a ``merge_context`` row,
        wider than one base, too --, so the windows of a tiling count every row exactly once.  A row counts if its context is in
        ``contexts`` (any subset of ("CpG", "CHG", "CHH") or of the indices 0 to 2; default: all), its strand is ``strand`` (``None``:
        any, merged rows included; "+" or "-") and nmeth + nunmeth >= ``min_depth``.  The rows must be strictly ascending in (contig,
        start), as a session returns them: rows in another order, a context above 2, a contig index outside ``contigs`` and an
        interval with a contig outside them, ``start < 0`` or ``end < start`` raise MdkError (rc -3); so do CPU tensors: there is no CPU
        path."""
        return self._regions([getattr(self, name) for name, _ in CALL_COLUMNS], intervals, contexts, strand, min_depth)

    def smooth(self, half_bases=1000, min_sites=70, kernel="tricube"):
        """``Cohort.smooth`` for this one sample: a ``Smoothed`` with ``n_samples`` 1 and these rows' ``contig``, ``start``, ``end``,
        ``context`` and ``strand`` (the same tensors).  The rows must be strictly ascending in (contig, start): one context of a
        session's calls, or ``merge_context`` rows of one context."""
        out = smooth_counts(self.contig, self.start, self.nmeth.unsqueeze(0), self.nunmeth.unsqueeze(0), half_bases, min_sites, kernel)
        return Smoothed(self.contigs, {name: getattr(self, name) for name, _ in DIFF_SITE_COLUMNS}, *out, half_bases, min_sites, kernel, merged=self.merged)

    # ---- the bigWig track (include/mdk_track.h, csrc/mdk_bigwig.hip -> libmdk_track.so; the rule is csrc/mdk_bigwig_core.h) ----
    def _track_arguments(self, lengths, value, context):
        """the checks of ``render_bigwig`` and ``write_bigwig``, made before anything is opened: (the five columns, the lengths as a C
        array, the value's code, the device)"""
        import torch
        if value not in TRACK_VALUES:
            raise MdkError(f"unknown value {value!r}: one of {', '.join(TRACK_VALUES)}")
        if isinstance(lengths, Reference):
            if list(lengths.contigs) != list(self.contigs):
                raise MdkError("the reference's contigs are not the rows' contigs: its lengths would be those of other sequences")
            lengths = lengths.lengths
        try:
            lengths = list(lengths)
        except TypeError:
            raise MdkError("lengths is a Reference, or a sequence of one int per contig") from None
        if len(lengths) != len(self.contigs):
            raise MdkError(f"lengths has {len(lengths)} entries, the rows have {len(self.contigs)} contigs")
        for name, l in zip(self.contigs, lengths):
            if isinstance(l, bool) or not isinstance(l, int) or not 0 <= l <= 2 ** 31 - 1:
                raise MdkError(f"the length of {name} must be an int between 0 and 2^31 - 1, not {l!r}")
        if context is not None:
            if context in CONTEXT_FILES:
                context = CONTEXT_FILES.index(context)
            if isinstance(context, bool) or context not in (0, 1, 2):
                raise MdkError(f"unknown context {context!r}: None, one of {CONTEXT_FILES}, or an index 0 to 2")
        cols = [getattr(self, name) for name in TRACK_COLUMNS] + [self.context]
        dev, n = cols[0].device, int(cols[0].shape[0])
        for t, name in zip(cols, TRACK_COLUMNS + ("context",)):
            dt = "uint8" if name == "context" else "int32"
            if t.device.type != "cuda":
                raise MdkError(f"the track is made on the device: the {name} column is a {t.device.type} tensor, and there is no CPU path")
            if t.device != dev or t.dtype != getattr(torch, dt) or t.dim() != 1 or not t.is_contiguous() or t.shape[0] != n:
                raise MdkError(f"the {name} column must be a contiguous {dt} tensor on {dev} with one entry per row")
        if context is not None:
            keep = cols[5] == context
            cols = [t[keep].contiguous() for t in cols[:5]]
        return cols[:5], (C.c_int64 * len(lengths))(*lengths), TRACK_VALUES[value], dev

    def _track_measure(self, L, h, cols, lengths, value):
        """md_track_bigwig_measure over the columns, under the handle's lock: the file's size"""
        names = (C.c_char_p * len(self.contigs))(*[os.fsencode(s) for s in self.contigs])
        size = C.c_int64()
        _side_call(L, "track", "bigwig_measure", h, *[C.c_void_p(t.data_ptr()) for t in cols], int(cols[0].shape[0]), len(self.contigs), names, lengths, value, C.byref(size))
        return size.value

    def render_bigwig(self, lengths, value="percent", context=None):
        """These rows as a bigWig track -- what IGV and the UCSC browser open, and what `bedGraphToBigWig` makes of the bedGraph --: the
        file's bytes as a uint8 tensor on the columns' device, made there (csrc/mdk_bigwig.hip) by the rule of csrc/mdk_bigwig_core.h: bbi
        version 4, sections of 1024 rows compressed as zlib streams, the R-tree index, up to eight zoom levels of 1024 * 4^k bases and the
        total summary.  ``lengths``: a ``Reference`` over the same ``contigs``, or one int per contig (0 to 2^31 - 1): a bigWig lists
        every contig with its length.  ``value``: "percent", (float)(100 nmeth / (nmeth + nunmeth)) as the bedGraph's fourth column, or
        "coverage", nmeth + nunmeth.  ``context``: ``None`` takes the rows as they are; 0, 1, 2 or "CpG", "CHG", "CHH" takes that
        context's rows.  The rows must be strictly ascending in (contig, start) and must not overlap: a session run with several
        contexts is not, as a whole, so pass one context.  A row outside its contig, a negative count, a row without coverage under
        "percent", rows out of order and rows that overlap raise MdkError (rc -3) naming the first such row; so do CPU tensors: there
        is no CPU path.  The bytes are a function of the columns and the arguments alone: the same on every run and every device, and
        those of tools/bigwig_emu.  Not here: reading a bigWig back, bigBed, compression levels, UCSC's own zoom widths."""
        import torch
        cols, lengths, value, dev = self._track_arguments(lengths, value, context)
        L = lib_track()
        torch.cuda.current_stream(dev).synchronize()             # the columns are complete, and nothing of torch's is queued on memory it hands out next
        with _side_locks["track"]:                               # a handle per device, kept: the measured file stays on it until it is filled
            h = _side_handle(L, "track", dev.index or 0)
            size = self._track_measure(L, h, cols, lengths, value)
            out = torch.empty(size, dtype=torch.uint8, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            _side_call(L, "track", "bigwig_fill_range", h, C.c_void_p(out.data_ptr()), 0, size)
        return out

    def write_bigwig(self, path, lengths, value="percent", context=None, piece_bytes=None):
        """``render_bigwig``'s bytes written to ``path``, the arguments as there.  The table is measured first -- all of the device work --
        and the file is opened only then: a refused table leaves no file.  The file then passes through one device buffer of
        ``piece_bytes`` (default 64 MiB), laid out there a piece at a time (md_track_bigwig_fill_range), each piece copied to the host
        once and appended.  Returns the path."""
        import torch
        piece_bytes = int(piece_bytes or TRACK_PIECE_BYTES)
        if not 1 <= piece_bytes <= (1 << 31) - 1:
            raise MdkError("piece_bytes must be between 1 and 2^31 - 1")
        cols, lengths, value, dev = self._track_arguments(lengths, value, context)
        L = lib_track()
        torch.cuda.current_stream(dev).synchronize()
        with _side_locks["track"]:
            h = _side_handle(L, "track", dev.index or 0)
            size = self._track_measure(L, h, cols, lengths, value)
            piece_bytes = min(piece_bytes, max(size, 1))
            buf, write = torch.empty(piece_bytes, dtype=torch.uint8, device=dev), _file_writer()
            torch.cuda.current_stream(dev).synchronize()
            with open(path, "wb") as f:
                for at in range(0, size, piece_bytes):
                    n = min(piece_bytes, size - at)
                    _side_call(L, "track", "bigwig_fill_range", h, C.c_void_p(buf.data_ptr()), at, n)
                    write(f, buf[:n])
        return path

    @classmethod
    def read(cls, paths, reference, device=0, contexts_on=None, block_bytes=None, region=None):
        """The rows of per-cytosine bedGraph files -- what ``write`` made, last week's run, the command-line tool's output -- as a Calls on
        ``device``, parsed there (csrc/mdk_parse.hip): no line passes through Python.  ``paths`` is one path or a list; the rows come in the
        order of the paths, then of the lines (``sorted()`` makes the three per-context files of one run the ascending table
        ``merge_context`` wants).  ``reference`` is a ``Reference``: ``contigs`` is its names, and every row's ``strand`` and ``context``
        come from its bases at the line's start by the rule of the `mergeContext` command, which is a session's own.  ``merged`` is False;
        ``contexts_on`` defaults to the contexts that have rows.  The result shares the reference's renderer, so ``write`` and
        ``merge_context`` need no second one: ``Calls.read(f, ref).merge_context().write(p)`` is the `mergeContext` command.
        A file is read in pieces of ``block_bytes`` (default 256 MiB), each cut after its last newline, put into a pinned buffer and copied
        to the device once; a line longer than a piece raises MdkError.  `track` lines are skipped wherever they stand.  The parser is
        stricter than the command (signs, blanks, doubled tabs, extra columns, numbers past INT32_MAX, merged files and lines longer than
        512 bytes are refused): MdkError with ``rc == -3`` names the refusal, the path and the line.  Only bedGraph files hold both counts:
        --fraction, --counts and --methylKit files cannot be read.  There is no CPU path.
        BGZF files -- ``write(compress=True)``'s, bgzip's -- are read too, recognised by content (the gzip magic with FEXTRA and a BC
        subfield), not by name: the host walks the 18-byte headers, pieces of whole members (``block_bytes`` counts inflated bytes) are
        inflated and CRC32-checked on the device (csrc/mdk_inflate.hip) and parsed where they lie; a line may straddle members and
        pieces, and no decompressed byte crosses to the host.  Refused, with MdkError naming the path: a gzip file that is not BGZF (one
        member of any length is one wavefront's work: recompress it with bgzip), a member whose CRC32 or ISIZE does not check (with
        the member's file offset), a last member that is cut short.  A missing EOF member is accepted, as htslib accepts it with a
        warning.  A refused line's number is that of the decompressed text.
        ``region=(name, beg, end)``, 0-based and half-open, reads one BGZF file at random through ``path + ".tbi"`` (``write(...,
        compress=True, index=True)``, ``tabix_index``): the index is read on the host, the chunks of the region's bins that end above
        the linear index's offset are taken, only the members they span are inflated, only the text between a chunk's begin and end is
        parsed, and the rows that overlap the region are kept -- ``read(path, ref).select(mask)`` of the whole file, for the price of
        the region.  The result's ``members_inflated`` says how many of the file's members were touched.  A name the index
        does not hold gives an empty table; a missing .tbi, a plain-text path and a list of several paths raise MdkError."""
        dev = _parse_device(device)
        if not isinstance(reference, Reference):
            raise MdkError("Calls.read needs a Reference: a bedGraph line's strand and context come from its bases")
        block_bytes = _parse_block_bytes(block_bytes)
        if region is not None:
            region, stats = _region_check(region), {}
            if not isinstance(paths, (str, bytes, os.PathLike)):
                raise MdkError("a region is read from one file: every file has an index of its own")
            text = reference._renderer(device)
            cols = _parse_cat(_parse_region(text.L, text, paths, PARSE_BEDGRAPH, CALL_COLUMNS, dev, block_bytes, region, stats), CALL_COLUMNS, dev)
            names = list(reference.contigs)
            keep = (cols["contig"] == (names.index(region[0]) if region[0] in names else -1)) & (cols["start"] < region[2]) & (cols["end"] > region[1])
            cols = {n: t[keep].contiguous() for n, t in cols.items()}
            c = cls(names, cols, merged=False, contexts_on=_contexts_present(cols["context"]) if contexts_on is None else contexts_on)
            c._text, c.members_inflated = text, stats["members_inflated"]
            return c
        paths = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)
        text = reference._renderer(device)
        pieces = []
        for p in paths:
            pieces += _parse_file(text.L, text, os.fspath(p), PARSE_BEDGRAPH, CALL_COLUMNS, dev, block_bytes)
        cols = _parse_cat(pieces, CALL_COLUMNS, dev)
        c = cls(list(reference.contigs), cols, merged=False, contexts_on=_contexts_present(cols["context"]) if contexts_on is None else contexts_on)
        c._text = text
        return c

    def sorted(self):
        """the rows in ascending (contig, start): a ``select`` by the stable argsort of contig << 32 | start, in torch"""
        import torch
        key = (self.contig.to(torch.int64) << 32) | self.start.to(torch.int64)
        c = self.select(torch.argsort(key, stable=True))
        c._text = getattr(self, "_text", None)
        return c

    def rows(self, context=None):
        """(chrom, start, end, nmeth, nunmeth) tuples on the host, optionally of one context -- the bedGraph lines' columns 1, 2, 3, 5, 6"""
        cols = [getattr(self, n).cpu().tolist() for n in ("contig", "start", "end", "nmeth", "nunmeth", "context")]
        return [(self.contigs[c], a, b, m, u) for c, a, b, m, u, x in zip(*cols) if context is None or x == context]


class Reads(_Columns):
    """The lines `perRead` would print, as columns (one row per line, in the command's order: chunks of the schedule, reads of a chunk in
    file order): ``contig`` (int32, index into ``contigs``), ``pos`` (int32, the line's column 3), ``nmeth``/``nunmeth`` (int32: the line
    prints 100*nmeth/(nmeth+nunmeth) and the sum), ``name_offsets`` (int64, len + 1 entries, the first 0) and ``name_bytes`` (uint8, the read
    names packed without separators: name i is name_bytes[name_offsets[i]:name_offsets[i + 1]])."""
    COLUMNS = READ_COLUMNS
    KIND = "reads"

    @classmethod
    def _sizes(cls, L, out, n):
        return {"name_offsets": n + 1, "name_bytes": int(L.mdk_reads_name_bytes(out))}

    def _checked(self):
        """the columns, after the checks of the ragged layout: one entry per row, ``len + 1`` offsets, all on one device"""
        import torch
        cols = [getattr(self, name) for name, _ in self.COLUMNS]
        dev, n = cols[0].device, len(self)
        for t, (name, dt) in zip(cols, self.COLUMNS):
            want = n + 1 if name == "name_offsets" else None if name == "name_bytes" else n
            if t.device != dev or t.dtype != getattr(torch, dt) or t.dim() != 1 or not t.is_contiguous() or (want is not None and t.shape[0] != want):
                raise MdkError(f"the {name} column must be a contiguous {dt} tensor on {dev}" + ("" if want is None else " with len + 1 entries" if want == n + 1 else " with one entry per row"))
        return cols, dev

    def _text_blocks(self, fmt, context, block_rows):
        cols, dev = self._checked()
        if dev.type != "cuda":
            raise MdkError(f"text is made on the device: the columns are {dev.type} tensors, and there is no CPU path")
        L = self._renderer(dev)
        view = md_reads_cols(*[C.c_void_p(t.data_ptr()) for t in cols])
        return self._text_iter(L, view, dev, TEXT_PERREAD, None, self._block_rows(block_rows))

    def render(self, block_rows=None, compress=False):
        """The bytes of the file `perRead -o` writes (no header: the command prints none), as a uint8 tensor on the columns' device, made
        there (k_rtext_len / k_rtext_fill, csrc/mdk_text.hip) from whatever the columns hold now: one line per row, covered or not.  A contig
        index outside ``contigs``, offsets that decrease or leave ``name_bytes``, and a name longer than 255 bytes raise MdkError; so do
        CPU tensors: there is no CPU path.  ``compress=True``: the bytes of the BGZF file, as ``Calls.render``."""
        return self._render(TEXT_PERREAD, None, b"", block_rows, compress)

    def write(self, path, block_rows=None, compress=False):
        """The file `perRead -o path` writes (``path`` is the file's name, not a prefix, as the command's -o is); blocks as ``Calls.write``.
        No rows give an empty file.  ``compress=True`` writes BGZF, compressed on the device as ``Calls.write`` does, to ``path`` as it is
        given (nothing is appended); no rows give the EOF member alone.  Returns the path."""
        return self._write_file(os.fspath(path), TEXT_PERREAD, None, b"", block_rows, compress)

    def select(self, index):
        """a copy with the rows ``index`` names -- a boolean mask, an int64 index tensor (any order, repeats allowed) or a slice --, same
        contigs: the per-row columns indexed with torch, ``name_offsets`` the scan of the selected names' lengths, ``name_bytes`` re-packed
        (on the device by k_rtext_gather, a workgroup per 256 names; on CPU tensors with torch)"""
        import copy
        import torch
        cols, dev = self._checked()
        n = len(self)
        if isinstance(index, slice):
            idx = torch.arange(*index.indices(n), device=dev)          # (a negative step too, which torch's own indexing refuses)
        else:
            index = torch.as_tensor(index, device=dev)
            if index.dtype == torch.bool:
                if index.shape != (n,):
                    raise MdkError("a mask must have one entry per row")
                idx = index.nonzero().reshape(-1)
            elif index.dtype == torch.int64 and index.dim() == 1:
                idx = torch.where(index < 0, index + n, index)
                if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
                    raise MdkError("an index is not a row")
            else:
                raise MdkError("select takes a boolean mask, an int64 index tensor or a slice")
        idx = idx.contiguous()
        c = copy.copy(self)
        c._text = None
        for name in ("contig", "pos", "nmeth", "nunmeth"):
            setattr(c, name, getattr(self, name)[idx].contiguous())
        off = self.name_offsets
        lens = off[idx + 1] - off[idx]
        new_off = torch.zeros(idx.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=new_off[1:])
        total = int(new_off[-1]) if idx.numel() else 0
        if total < 0 or (idx.numel() and int(lens.min()) < 0):
            raise MdkError("the name offsets decrease")
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        if dev.type != "cuda":
            if total:          # byte k of the result lies lens-scan[k's row] past its row's start in the source
                row = torch.repeat_interleave(torch.arange(idx.numel()), lens)
                out = self.name_bytes[off[idx][row] + (torch.arange(total) - new_off[:-1][row])].contiguous()
        elif idx.numel():
            L = self._renderer(dev)
            torch.cuda.current_stream(dev).synchronize()
            rc = L.md_text_gather_names(self._text.h, C.c_void_p(off.data_ptr()), C.c_void_p(self.name_bytes.data_ptr()), n, int(self.name_bytes.shape[0]),
                                        C.c_void_p(idx.data_ptr()), idx.numel(), C.c_void_p(new_off.data_ptr()), C.c_void_p(out.data_ptr()), total)
            if rc:
                raise _rc_error("md_text_gather_names", rc, L.md_dev_last_error().decode())
        c.name_offsets, c.name_bytes = new_off, out
        return c

    def names(self):
        """the read names on the host, as str"""
        off, b = self.name_offsets.cpu().tolist(), self.name_bytes.cpu().numpy().tobytes()
        return [b[off[i]:off[i + 1]].decode("latin-1") for i in range(len(self))]

    def rows(self):
        """(name, chrom, pos, nmeth, nunmeth) tuples on the host"""
        cols = [getattr(self, n).cpu().tolist() for n in ("contig", "pos", "nmeth", "nunmeth")]
        return [(q, self.contigs[c], p, m, u) for q, c, p, m, u in zip(self.names(), *cols)]


class Bias(_Columns):
    """What `mbias` would print, as columns: one row per line of its table, in the command's order (strand OT, OB, CTOT, CTOB; ascending
    position; read 1 then read 2; only positions with a call) -- ``strand`` (int8, index into STRANDS), ``read`` (int8, 1 or 2), ``position``
    (int32, 1-based), ``nmeth``/``nunmeth`` (int64) -- and ``counts``, the dense histogram, int64 [len, 4, 2, 2] (position, strand, read,
    methylated/unmethylated; len = the longest admitted read).  On the host: ``suggested``, the inclusion bounds the command prints behind
    "Suggested inclusion options:" when it draws its plots ({"OT": (a, b, c, d), ...}, the strands that have calls, in STRANDS order), and
    ``resubmitted``, the chunks whose group launch left them out and that were counted by a launch of their own.  No ``contigs``."""
    COLUMNS = BIAS_COLUMNS
    KIND = "bias"
    ALWAYS = ("counts",)

    @classmethod
    def _sizes(cls, L, out, n):
        return {"counts": 16 * int(L.mdk_bias_len(out))}

    @classmethod
    def _build(cls, L, out, cols):
        suggested, b4 = {}, (C.c_int * 4)()
        for k, name in enumerate(STRANDS):
            if L.mdk_bias_suggested(out, k, b4) == 1:
                suggested[name] = tuple(b4)
        cols["counts"] = cols["counts"].reshape(-1, 4, 2, 2)
        return cls(cols, suggested, int(L.mdk_bias_resubmitted(out)))

    def __init__(self, columns, suggested, resubmitted=0):
        for name, _ in self.COLUMNS:
            setattr(self, name, columns[name])
        self.suggested = suggested
        self.resubmitted = resubmitted

    def options(self):
        """the suggestion as argv tokens, ["--OT", "a,b,c,d", "--OB", ...]: ready to append to an extract command line"""
        return [t for k, v in self.suggested.items() for t in ("--" + k, ",".join(str(x) for x in v))]

    def render(self):
        """The `mbias --txt` table as the command prints it (csrc/host/mdk_mbias.c mdk_mbias_report), as bytes: the header line, then one
        line per row.  Made on the host from the row columns, CPU tensors or device ones: the table has at most 8 x read length rows, so
        a kernel would be complexity without a payoff."""
        return ("Strand\tRead\tPosition\tnMethylated\tnUnmethylated\n" + "".join("%s\t%i\t%i\t%u\t%u\n" % r for r in self.rows())).encode()

    def write(self, path):
        """``render()`` into the file ``path``; returns the path"""
        with open(path, "wb") as f:
            f.write(self.render())
        return path

    def rows(self):
        """(strand name, read, position, nmeth, nunmeth) tuples on the host: the lines of the --txt table"""
        cols = [getattr(self, n).cpu().tolist() for n in ("strand", "read", "position", "nmeth", "nunmeth")]
        return [(STRANDS[s], r, p, m, u) for s, r, p, m, u in zip(*cols)]


class Cytosines(_Columns):
    """The lines `extract --cytosine_report` would write, as columns: one row for EVERY cytosine of the reference in the contexts switched
    on, covered or not, in the file's order (the chunks of the schedule, ascending position within a chunk) -- ``contig`` (int32, index into
    ``contigs``), ``pos`` (int32, 1-based: the line's column 2), ``strand`` (int8: +1 a C, -1 a G), ``nmeth``/``nunmeth`` (int32),
    ``context`` (uint8: 0 CG, 1 CHG, 2 CHH) and ``trinucleotide`` (uint8 [len, 3]: the ASCII letters of column 7).  Which rows there are
    depends on the reference, the contexts and the schedule (-r, -l, --chunkSize) alone, never on the reads: the results of two BAM files
    run against one reference with the same options line up row for row, so ``torch.stack([a.nmeth, b.nmeth])`` is a samples x cytosines
    matrix."""
    COLUMNS = CYTOSINE_COLUMNS
    KIND = "cytosines"
    contexts_on = (0, 1, 2)

    @classmethod
    def _sizes(cls, L, out, n):
        return {"trinucleotide": 3 * n}

    @classmethod
    def _build(cls, L, out, cols):
        cols["trinucleotide"] = cols["trinucleotide"].reshape(-1, 3)
        c = super()._build(L, out, cols)
        c.contexts_on = tuple(k for k in range(3) if L.mdk_cytosines_contexts(out) >> k & 1)      # the contexts whose cytosines are rows
        return c

    def render(self, block_rows=None, compress=False):
        """The bytes of <prefix>.cytosine_report.txt (no header), as a uint8 tensor on the columns' device, made there from whatever the
        columns hold now.  ``compress=True``: the bytes of the BGZF file, as ``Calls.render``.  CPU tensors raise MdkError."""
        return self._render(TEXT_CYTOSINE_REPORT, None, b"", block_rows, compress)

    def write(self, prefix, directory=None, block_rows=None, compress=False, index=False):
        """<prefix>.cytosine_report.txt as the command writes it, in ``directory`` if given; blocks as ``Calls.write``.  ``compress=True``
        writes <prefix>.cytosine_report.txt.gz, BGZF compressed on the device as ``Calls.write`` does; ``index=True`` with it writes
        <prefix>.cytosine_report.txt.gz.tbi next to it (columns 1 and 2, no line skipped), made on the device from the text on its way to
        the deflate, and refuses what ``Calls.write`` refuses.  Returns the path."""
        name = f"{prefix}.cytosine_report.txt" + (".gz" if compress else "")
        if index and not compress:
            raise MdkError("index=True needs compress=True: a tabix index is the index of a BGZF file")
        return self._write_file(os.path.join(directory, name) if directory is not None else name, TEXT_CYTOSINE_REPORT, None, b"", block_rows, compress,
                                _tabix_conf("cytosine_report", 0) if index else None)

    @classmethod
    def read(cls, path, contigs, device=0, contexts_on=None, block_bytes=None, region=None):
        """The rows of a <prefix>.cytosine_report.txt as a Cytosines on ``device``, parsed there (csrc/mdk_parse.hip), in the file's order.
        ``contigs`` is the list of names the lines' first column is looked up in (a session result's ``contigs``, a ``Reference``'s); no
        reference is needed: strand, context and trinucleotide are in the file.  ``contexts_on`` defaults to the contexts that have rows.
        Pieces, refusals and errors as ``Calls.read``, BGZF files (``write(compress=True)``'s, bgzip's) and what is refused of .gz files
        included; there is no CPU path.  Reports of several samples
        read this way stack as a session's do: ``torch.stack([a.nmeth, b.nmeth])``.  ``region=(name, beg, end)``, 0-based and half-open:
        the cytosines of that region alone, read through ``path + ".tbi"`` as ``Calls.read`` reads a region (a cytosine at ``pos`` is the
        interval [pos - 1, pos)); ``members_inflated`` as there."""
        dev = _parse_device(device)
        block_bytes = _parse_block_bytes(block_bytes)
        contigs = list(contigs)
        L = _text_lib()
        text = _TextRenderer(L, int(device), contigs)
        stats = {}
        if region is not None:
            region = _region_check(region)
            if not isinstance(path, (str, bytes, os.PathLike)):
                raise MdkError("a region is read from one file: every file has an index of its own")
            cols = _parse_cat(_parse_region(L, text, path, PARSE_CYTOSINE_REPORT, CYTOSINE_COLUMNS, dev, block_bytes, region, stats), CYTOSINE_COLUMNS, dev)
            cols["trinucleotide"] = cols["trinucleotide"].reshape(-1, 3)
            keep = (cols["contig"] == (contigs.index(region[0]) if region[0] in contigs else -1)) & (cols["pos"] - 1 < region[2]) & (cols["pos"] > region[1])
            cols = {n: t[keep].contiguous() for n, t in cols.items()}
        else:
            cols = _parse_cat(_parse_file(L, text, os.fspath(path), PARSE_CYTOSINE_REPORT, CYTOSINE_COLUMNS, dev, block_bytes), CYTOSINE_COLUMNS, dev)
            cols["trinucleotide"] = cols["trinucleotide"].reshape(-1, 3)
        c = cls(contigs, cols)
        if stats:
            c.members_inflated = stats["members_inflated"]
        c.contexts_on = _contexts_present(cols["context"]) if contexts_on is None else tuple(contexts_on)
        c._text = text
        return c

    def merge_context(self):
        """The report per CpG / CHG site: a Calls (``merged`` true) with a row for every CpG and CHG site and every CHH cytosine of the
        reference, covered or not -- ``Calls.merge_context`` at ``min_depth=0`` over a view of these columns (``start`` = pos - 1, ``end`` =
        pos; counts, contig, context and strand are not copied).  Which rows there are depends on the reference and the schedule alone,
        so two samples' results line up row for row: ``torch.stack([a.merge_context().nmeth, b.merge_context().nmeth])`` is the samples x
        CpGs matrix.  ``Calls.render`` prints no line for an uncovered row."""
        return self._merged([self.contig, self.pos - 1, self.pos, self.nmeth, self.nunmeth, self.context, self.strand], 0)

    def regions(self, intervals, contexts=None, strand=None, min_depth=0):
        """The report added up per interval: ``Calls.regions`` over a view of these columns (``start`` = pos - 1, ``end`` = pos; counts,
        contig, context and strand are not copied).  At the default ``min_depth=0`` ``nsites`` is the number of cytosines of the
        interval, at ``min_depth=1`` the number covered; with ``Intervals.windows`` two samples' results line up window for window."""
        return self._regions([self.contig, self.pos - 1, self.pos, self.nmeth, self.nunmeth, self.context, self.strand], intervals, contexts, strand, min_depth)

    def profile(self, by="context", min_depth=1, depth_bins=1024, level_bins=20):
        """``Calls.profile`` of the report, every cytosine of the reference a cell: bin 0 of ``depth_hist`` holds the cytosines no read
        covers, ``sites()`` is the cytosines of the reference in the contexts switched on, and ``breadth()`` the share of them
        covered at ``min_depth``."""
        group, n_groups, group_names = _profile_by(by, self.context)
        return count_profile(self.nmeth.unsqueeze(0), self.nunmeth.unsqueeze(0), group, n_groups, min_depth, depth_bins, level_bins, group_names=group_names)

    def rows(self):
        """(chrom, pos, "+"/"-", nmeth, nunmeth, "CG"/"CHG"/"CHH", trinucleotide) tuples on the host: the seven fields of a line"""
        cols = [getattr(self, n).cpu().tolist() for n in ("contig", "pos", "strand", "nmeth", "nunmeth", "context")]
        tri = self.trinucleotide.cpu().numpy().tobytes().decode("latin-1")
        return [(self.contigs[c], p, "+" if s > 0 else "-", m, u, CONTEXTS[x], tri[3 * i:3 * i + 3]) for i, (c, p, s, m, u, x) in enumerate(zip(*cols))]


REGION_COLUMNS = (("contig", "int32"), ("start", "int32"), ("end", "int32"), ("nsites", "int32"), ("nmeth", "int64"), ("nunmeth", "int64"))
MAX_INTERVALS = 1 << 30


class Intervals:
    """Half-open, 0-based intervals as a BED file has them, for ``Calls.regions`` / ``Cytosines.regions``: ``contigs`` (the names the
    indices mean) and three int32 tensors of one entry per interval, ``contig`` (index into ``contigs``), ``start`` and ``end``, in any
    order; intervals may overlap, nest or repeat."""

    def __init__(self, contigs, contig, start, end):
        self.contigs = list(contigs)
        self.contig, self.start, self.end = contig, start, end

    def __len__(self):
        return int(self.contig.shape[0])

    def to(self, device):
        """the same intervals with their three tensors on ``device`` (this object if they are there already)"""
        cols = [t.to(device) for t in (self.contig, self.start, self.end)]
        if all(a is b for a, b in zip(cols, (self.contig, self.start, self.end))):
            return self
        return Intervals(self.contigs, *cols)

    @classmethod
    def read(cls, bed_path, contigs):
        """The intervals of a BED file, on the CPU, in the file's order.  ``contigs`` is the list of names column 1 is looked up in (a
        session result's ``contigs``, a ``Reference``'s).  Fields are separated by tabs or blanks and only the first three are used;
        empty lines and lines that begin with ``#``, ``track`` or ``browser`` are skipped.  A contig that is not in ``contigs``, a
        field that is not a decimal number, ``end < start`` and a value above 2^31 - 1 raise MdkError with the path and the line
        number.  Parsed on the host, line by line: a BED of islands or promoters has a few 10^5 lines.  A file that begins with the gzip
        magic -- plain gzip or BGZF -- is decompressed by the host's ``gzip`` module as it is read; one that does not inflate raises
        MdkError with the path."""
        import torch
        path, contigs = os.fspath(bed_path), list(contigs)
        index = {}
        for i, name in enumerate(contigs):
            index.setdefault(name, i)
        cols = ([], [], [])
        with open(path, "rb") as f:
            data = f.read()
        if data[:2] == b"\x1f\x8b":
            import gzip
            import zlib
            try:
                data = gzip.decompress(data)
            except (OSError, EOFError, zlib.error) as e:
                raise MdkError(f"{path}: not a readable gzip file: {e}") from None
        for ln, raw in enumerate(data.split(b"\n")[:-1] if data.endswith(b"\n") else data.split(b"\n"), 1):
            fields = raw.decode("latin-1").split()
            if not fields or fields[0].startswith("#") or fields[0] in ("track", "browser"):
                continue
            if len(fields) < 3:
                raise MdkError(f"{path}:{ln}: a BED line has at least three fields")
            if fields[0] not in index:
                raise MdkError(f"{path}:{ln}: the contig {fields[0]!r} is not among the contig names")
            for v in fields[1:3]:
                if not (v.isascii() and v.isdigit()):
                    raise MdkError(f"{path}:{ln}: {v!r} is not a decimal number")
            s, e = int(fields[1]), int(fields[2])
            if s > 2 ** 31 - 1 or e > 2 ** 31 - 1:
                raise MdkError(f"{path}:{ln}: a position above 2^31 - 1")
            if e < s:
                raise MdkError(f"{path}:{ln}: end {e} < start {s}")
            cols[0].append(index[fields[0]]); cols[1].append(s); cols[2].append(e)
        return cls(contigs, *[torch.tensor(c, dtype=torch.int32) for c in cols])

    @classmethod
    def windows(cls, lengths, width, step=None, contigs=None):
        """Every window ``[i * step, min(i * step + width, length))`` of every contig, in contig order, on the CPU -- the tiles of
        methylKit's ``tileMethylCounts`` (``step == width``, the default) or sliding windows (``step < width``).  ``lengths`` is a
        ``Reference``, or a list of contig lengths with their names as ``contigs``.  The windows depend on the lengths alone, covered or
        not, so two samples' ``regions`` line up window for window, as ``cytosine_report`` rows do.  ``width < 1``, ``step < 1`` and
        more than 2^30 windows raise MdkError."""
        import torch
        if isinstance(lengths, Reference):
            lengths, contigs = lengths.lengths, lengths.contigs if contigs is None else contigs
        lengths = [int(x) for x in lengths]
        if contigs is None or len(list(contigs)) != len(lengths):
            raise MdkError("windows needs a Reference, or a list of lengths and contigs= with a name for each")
        width, step = int(width), int(width if step is None else step)
        if width < 1 or step < 1:
            raise MdkError("width and step must be at least 1")
        if any(x < 0 or x > 2 ** 31 - 1 for x in lengths):
            raise MdkError("a contig length must be between 0 and 2^31 - 1")
        counts = [(x + step - 1) // step for x in lengths]
        if sum(counts) > MAX_INTERVALS:
            raise MdkError(f"{sum(counts)} windows: more than 2^30")
        counts = torch.tensor(counts, dtype=torch.int64)
        contig = torch.repeat_interleave(torch.arange(len(lengths), dtype=torch.int64), counts)
        first = torch.cumsum(counts, 0) - counts
        start = (torch.arange(int(counts.sum()), dtype=torch.int64) - first[contig]) * step
        end = torch.minimum(start + width, torch.tensor(lengths, dtype=torch.int64)[contig])
        return cls(contigs, contig.to(torch.int32), start.to(torch.int32), end.to(torch.int32))


class Regions(_Columns):
    """What ``Calls.regions`` / ``Cytosines.regions`` return, one entry per interval in the intervals' own order, on the rows' device:
    ``contig``, ``start``, ``end`` (int32: the intervals' own tensors), ``nsites`` (int32: the rows counted), ``nmeth`` and ``nunmeth``
    (int64: their counts added).  ``select`` takes a mask, an index or a slice, as for the other results."""
    COLUMNS = REGION_COLUMNS

    def rows(self):
        """(chrom, start, end, nsites, nmeth, nunmeth) tuples on the host"""
        cols = [getattr(self, n).cpu().tolist() for n, _ in REGION_COLUMNS]
        return [(self.contigs[c], a, b, k, m, u) for c, a, b, k, m, u in zip(*cols)]

    def write(self, path):
        """the six columns, tab-separated, the contig by its name, without a header; formatted on the host.  Returns the path."""
        with open(path, "w") as f:
            f.writelines("%s\t%d\t%d\t%d\t%d\t%d\n" % r for r in self.rows())
        return path


SITE_COLUMNS = (("contig", "int32"), ("start", "int32"), ("end", "int32"), ("context", "uint8"), ("strand", "int8"), ("nsamples", "int32"))
MAX_SAMPLES = 1024


class Cohort:
    """What ``unite`` returns: the sites several samples hold, one entry per site, ascending in (contig, start), on the samples' device.
    ``contig``, ``start``, ``end`` (int32), ``context`` (uint8) and ``strand`` (int8) describe the site as a Calls row does; ``nsamples``
    (int32) is the number of samples that hold it after the depth cut; ``nmeth`` and ``nunmeth`` are int32 matrices ``[S, n]``, row s the
    counts of sample s, zeros where it does not hold the site.  ``contigs`` and ``merged`` are the samples', ``contexts_on`` the union of
    theirs; ``n_union`` is the number of sites any sample holds, which ``min_samples=1`` would have given.  ``names`` is a tuple of S
    sample names (1 to 255 bytes of 0x21 to 0x7e each, no two alike) or None: ``unite`` leaves it None, ``select`` carries it, ``read``
    sets it from the file, and ``write`` puts it into the file's second line."""

    def __init__(self, contigs, columns, nmeth, nunmeth, merged=False, contexts_on=(0, 1, 2), n_union=None, names=None):
        self.contigs = contigs
        for name, _ in SITE_COLUMNS:
            setattr(self, name, columns[name])
        self.nmeth, self.nunmeth = nmeth, nunmeth
        self.merged, self.contexts_on = bool(merged), tuple(contexts_on)
        self.n_union = len(self) if n_union is None else int(n_union)
        self.names = None if names is None else _cohort_sample_names(names, int(nmeth.shape[0]))
        self._text = None

    def __len__(self):
        return int(self.start.shape[0])

    @property
    def n_samples(self):
        return int(self.nmeth.shape[0])

    def select(self, index):
        """a copy with the sites ``column[index]`` (a boolean mask, an index tensor, a slice): of the site columns, and of the matrices
        along their site axis"""
        cols = {name: getattr(self, name)[index].contiguous() for name, _ in SITE_COLUMNS}
        c = Cohort(self.contigs, cols, self.nmeth[:, index].contiguous(), self.nunmeth[:, index].contiguous(), self.merged, self.contexts_on, self.n_union, self.names)
        c._text = self._text
        return c

    def sample(self, i):
        """Sample ``i`` over ALL the sites of the table, as a Calls: the site columns and row ``i`` of the two matrices -- views, not
        copies.  A site the sample does not hold is a ``0 0`` row, which ``regions`` (at ``min_depth`` >= 1), ``write`` and
        ``merge_context`` pass over as they pass over any such row; so ``cohort.sample(i).regions(tiles)`` lines up across samples."""
        i = int(i)
        if not 0 <= i < self.n_samples:
            raise MdkError(f"sample {i}: the table holds samples 0 to {self.n_samples - 1}")
        cols = {name: getattr(self, name) for name, _ in CALL_COLUMNS if name not in ("nmeth", "nunmeth")}
        cols["nmeth"], cols["nunmeth"] = self.nmeth[i], self.nunmeth[i]
        c = Calls(self.contigs, cols, merged=self.merged, contexts_on=self.contexts_on)
        c._text = self._text
        return c

    def rows(self):
        """(chrom, start, end, context, strand, nsamples, (nmeth, nunmeth) of sample 0, of sample 1, ...) tuples on the host"""
        cols = [getattr(self, n).cpu().tolist() for n, _ in SITE_COLUMNS]
        m, u = self.nmeth.t().cpu().tolist(), self.nunmeth.t().cpu().tolist()
        return [(self.contigs[c], a, b, x, s, k) + tuple(zip(mm, uu)) for (c, a, b, x, s, k), mm, uu in zip(zip(*cols), m, u)]

    def diff(self, a, b):
        """Two groups of the table's samples compared site by site -- what methylKit calls ``calculateDiffMeth``: ``a`` and ``b`` are
        sequences of sample indices (control and treatment; disjoint, neither empty; the other samples are ignored).  A ``Diff`` with
        this table's site columns (the same tensors) and, per site, the groups' pooled counts, ``meth_diff`` (percent, b minus a) and
        ``pvalue``, the two-sided p-value of Fisher's exact test of the pooled 2 x 2 table, made on the device by ``diff_counts``."""
        out = diff_counts(self.nmeth, self.nunmeth, a, b, _text=self._text)          # (on the table's renderer, if it has one)
        cols = {name: getattr(self, name) for name, _ in DIFF_SITE_COLUMNS}
        cols.update(zip((name for name, _ in DIFF_RESULT_COLUMNS), out))
        return Diff(self.contigs, cols, merged=self.merged)

    def diff_replicates(self, a, b, min_dispersion=1.0):
        """``diff`` for groups of REPLICATES, which is what most experiments have: the quasi-binomial F test of ``diff_replicates`` in
        the place of Fisher's test of the pooled table, which takes every read of a group for an independent draw and rejects far too
        often when the samples of a group differ by more than that.  ``a`` and ``b`` as for ``diff``.  A ``ReplicateDiff`` with this
        table's site columns (the same tensors), the groups' pooled counts and ``meth_diff`` as ``diff`` gives them, ``pvalue`` the F
        test's, and ``df``, ``dispersion`` and ``statistic``.  With one sample a group there is nothing to estimate a dispersion
        from: every site has p 1.0 and df 0, and ``diff`` is the test for that experiment."""
        out = diff_replicates(self.nmeth, self.nunmeth, a, b, min_dispersion=min_dispersion)
        cols = {name: getattr(self, name) for name, _ in DIFF_SITE_COLUMNS}
        cols.update(zip((name for name, _ in REPLICATE_RESULT_COLUMNS), out))
        return ReplicateDiff(self.contigs, cols, merged=self.merged)

    def diff_groups(self, groups, min_dispersion=1.0, names=None):
        """``diff_replicates`` for THREE OR MORE groups of replicates -- a time course, several tissues, a dose series: the omnibus F
        test of ``diff_groups`` on the table's matrices, one pass whatever the number of groups.  ``groups`` is a sequence of
        sequences of sample indices (disjoint, none empty; the other samples are not read), ``names`` the groups' names for ``write``
        (``g0``, ``g1``, ... by default).  A ``GroupDiff`` with this table's site columns (the same tensors), the groups' pooled counts
        as two ``[G, n]`` matrices, ``meth_diff`` between the most and the least methylated group, which two these are, and the
        test's ``pvalue``, ``df``, ``df_groups``, ``dispersion`` and ``statistic``.  ``GroupDiff.contrast(i, j)`` is the ``Diff`` of
        two of the groups, one call away.  With one sample a group every site has p 1.0 and df 0."""
        out = diff_groups(self.nmeth, self.nunmeth, groups, min_dispersion=min_dispersion)
        cols = {name: getattr(self, name) for name, _ in DIFF_SITE_COLUMNS}
        cols.update(zip((name for name, _ in GROUP_RESULT_COLUMNS), out[2:]))
        return GroupDiff(self.contigs, cols, out[0], out[1], merged=self.merged, names=names, _text=self._text)

    def diff_model(self, design, test, samples=None, min_dispersion=1.0, names=None):
        """The site-by-site test WITH COVARIATES: the table's counts regressed on a design matrix and some of its columns tested given
        the others by ``diff_model`` -- a paired design (a dummy per patient beside the group), a batch, sex or age beside the variable
        of interest, the slope of a dose or a time.  ``design`` is ``[S', p]`` (anything that converts to float64 on the host), a row
        per used sample, ``samples`` the table's sample of every row (default: all of them in order; the others are not read), ``test``
        a column index or a sequence of them, ``names`` the columns' names for ``write`` (``x0``, ``x1``, ... by default).  A
        ``ModelDiff`` with this table's site columns (the same tensors), the used samples' pooled counts, the coefficients ``[p, n]``
        and the test's ``pvalue``, ``df``, ``dispersion``, ``statistic``, ``flags`` and ``iterations``.  Regions are joined on a pair's
        direction: ``cohort.diff(a, b).dmrs(model.qvalue() < 0.05)``."""
        out = diff_model(self.nmeth, self.nunmeth, design, test, samples=samples, min_dispersion=min_dispersion)
        cols = {name: getattr(self, name) for name, _ in DIFF_SITE_COLUMNS}
        cols.update(zip((name for name, _ in MODEL_RESULT_COLUMNS), out[1:]))
        tested = _model_arguments("diff_model", self.nmeth, self.nunmeth, design, test, samples)[7]
        return ModelDiff(self.contigs, cols, out[0], tested, merged=self.merged, names=names)

    def moments(self, min_depth=1):
        """How alike the table's samples are, the first look after ``unite`` -- methylKit's ``getCorrelation``: a ``SampleMoments`` of
        the two matrices with the table's ``names``, made on the device by ``sample_moments``, which documents the rule.  A site a
        sample does not hold (``0 0``) is not covered there and takes part in no pair with that sample.
        ``cohort.moments().correlation()`` is the samples' correlation matrix, ``.distance()`` what ``clusterSamples`` clusters on."""
        return sample_moments(self.nmeth, self.nunmeth, min_depth, names=self.names)

    def profile(self, by="context", min_depth=1, depth_bins=1024, level_bins=20):
        """Every sample's depth and level histograms in one pass -- ``Calls.profile`` for the whole table: a ``CountProfile`` of the two
        matrices with the table's ``names``, grouped by the ``context`` column (``by=None``: one group), made on the device by
        ``count_profile``.  Row s is, bit for bit, ``cohort.sample(s).profile(...)``; a site a sample does not hold is a ``0 0`` cell
        and counts in bin 0 of its ``depth_hist``."""
        group, n_groups, group_names = _profile_by(by, self.context)
        return count_profile(self.nmeth, self.nunmeth, group, n_groups, min_depth, depth_bins, level_bins, names=self.names, group_names=group_names)

    def smooth(self, half_bases=1000, min_sites=70, kernel="tricube"):
        """Every sample's counts smoothed along the genome, the step between ``unite`` and a test or a plot at low coverage -- what
        bsseq's BSmooth and DSS's ``smoothing=TRUE`` do first: a site's window reaches at least ``half_bases`` to either side AND holds
        at least ``min_sites`` sites of its contig (BSmooth's ``h`` and ``ns``; all of a shorter contig), every row of the window
        weighs by the tricube kernel of its distance (``kernel="flat"``: 1, a moving sum), and a sample's ``level`` is its weighted
        methylated count over its weighted depth.  A ``Smoothed`` with this table's site columns (the same tensors), made on the device
        by ``smooth_counts``, which documents the rule."""
        out = smooth_counts(self.contig, self.start, self.nmeth, self.nunmeth, half_bases, min_sites, kernel)
        return Smoothed(self.contigs, {name: getattr(self, name) for name, _ in SITE_COLUMNS}, *out, half_bases, min_sites, kernel, merged=self.merged)

    def regions(self, intervals, contexts=None, strand=None, min_depth=1):
        """Every sample's sums over ``intervals`` in one pass on the device -- methylKit's ``tileMethylCounts`` on a united object; CpG
        islands, promoters, tiles (``Intervals.windows``) or the regions ``Diff.dmrs`` has just reported (``dmrs.intervals()``).  The
        arguments are ``Calls.regions``': an ``Intervals`` over the same ``contigs``, a subset of the contexts by name or index,
        ``strand`` None, ``"+"`` or ``"-"``, and ``min_depth`` (0 to 2^31 - 1), which cuts CELL by cell: site i counts for sample s if its
        context and strand pass and ``nmeth[s, i] + nunmeth[s, i] >= min_depth`` (formed in 64 bits).  A ``CohortRegions`` whose
        ``nsites`` (int32), ``nmeth`` and ``nunmeth`` (int64) are ``[S, k]`` in the intervals' own order: cell (s, j) is, by definition
        and bit for bit, what ``cohort.sample(s).regions(intervals, contexts, strand, min_depth)`` gives for interval j -- without the
        loop, its S checks of the same rows, its S searches per interval and the ``torch.stack`` behind it (csrc/mdk_cregion.hip:
        k_cregion_sites, k_cregion_ranges, k_cregion_totals, k_cregion_scan, k_cregion_sum).  The matrices go as they come into
        ``mdk.diff_counts(r.nmeth, r.nunmeth, a, b)`` and ``mdk.diff_replicates(r.nmeth, r.nunmeth, a, b)``: the test of the regions.
        An empty table, no intervals, empty intervals and intervals without rows give zeros.  Rows that are not strictly ascending, a
        row's contig outside the names or context above 2, an interval's contig outside the names, ``start < 0`` or ``end < start``
        raise MdkError (rc -3); so do, before the library is touched, CPU tensors (there is no CPU path), matrices that are not
        contiguous int32 ``[S, n]`` on the site columns' device, S outside 1 to 1024, more than 2^30 sites or intervals, and intervals
        over other contigs."""
        import torch
        context_mask, strand_mask, min_depth = _region_filter(self.contigs, intervals, contexts, strand, min_depth)
        S, n = int(self.nmeth.shape[0]) if self.nmeth.dim() == 2 else -1, len(self)
        if not 1 <= S <= MAX_SAMPLES:
            raise MdkError(f"regions are summed for 1 to {MAX_SAMPLES} samples: nmeth must be a [samples, sites] tensor")
        tensors = [(name, getattr(self, name), dt, (n,)) for name, dt in SITE_COLUMNS if name in ("contig", "start", "context", "strand")]
        tensors += [("nmeth", self.nmeth, "int32", (S, n)), ("nunmeth", self.nunmeth, "int32", (S, n))]
        for name, t, dt, shape in tensors:
            if t.dtype != getattr(torch, dt) or tuple(t.shape) != shape or not t.is_contiguous():
                raise MdkError(f"the {name} column must be a contiguous {dt} tensor of shape {shape}")
        for name, t, dt, shape in tensors:
            if t.device.type != "cuda":
                raise MdkError(f"regions are summed on the device: the {name} column is a {t.device.type} tensor, and there is no CPU path")
        dev = self.start.device
        for name, t, dt, shape in tensors:
            if t.device != dev:
                raise MdkError(f"the {name} column must be on the site columns' device, {dev}")
        iv = _region_intervals(intervals, dev)
        k = len(iv)
        if n > MAX_INTERVALS or k > MAX_INTERVALS:
            raise MdkError(f"{n} sites and {k} intervals: more than 2^30")
        out = [torch.empty((S, k), dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int64)]
        L = lib_cohort()
        torch.cuda.current_stream(dev).synchronize()             # the columns are complete, and nothing of torch's is queued on memory it hands out next
        with _side_locks["cohort"]:                              # a handle per device, kept: its calls come from one thread at a time
            h = _cohort_handle(L, dev.index or 0, self.contigs)
            _side_call(L, "cohort", "regions", h, *[C.c_void_p(t.data_ptr()) for _, t, _, _ in tensors], S, n,
                       *[C.c_void_p(getattr(iv, name).data_ptr()) for name in ("contig", "start", "end")], k, context_mask, strand_mask, min_depth,
                       *[C.c_void_p(t.data_ptr()) for t in out])
        return CohortRegions(list(self.contigs), iv.contig, iv.start, iv.end, *out, names=self.names)

    # ---- the table as text and back (include/mdk_cohort.h, csrc/mdk_cohort.hip -> libmdk_cohort.so; the formats are csrc/mdk_cohort_core.h's) ----
    def _text_arguments(self, fmt, names, piece_bytes):
        """what ``write`` and ``render`` ask, checked before the library is touched or a file opened: (format code, header bytes, piece_bytes, device)"""
        import torch
        if not isinstance(fmt, str) or fmt not in COHORT_FORMATS:
            raise MdkError(f"unknown format {fmt!r}: one of {', '.join(COHORT_FORMATS)}")
        S, n = int(self.nmeth.shape[0]) if self.nmeth.dim() == 2 else -1, len(self)
        if not 1 <= S <= MAX_SAMPLES:
            raise MdkError(f"a table is written with 1 to {MAX_SAMPLES} samples: nmeth must be a [samples, sites] tensor")
        names = _cohort_sample_names(names if names is not None else self.names if self.names is not None else [f"s{i}" for i in range(S)], S)
        piece_bytes = int(piece_bytes or COHORT_PIECE_BYTES)
        if not 1 <= piece_bytes <= (1 << 31) - 1:
            raise MdkError("piece_bytes must be between 1 and 2^31 - 1")
        tensors = [(name, getattr(self, name), dt, (n,)) for name, dt in SITE_COLUMNS] + [("nmeth", self.nmeth, "int32", (S, n)), ("nunmeth", self.nunmeth, "int32", (S, n))]
        for name, t, dt, shape in tensors:
            if t.device.type != "cuda":
                raise MdkError(f"text is made on the device: the {name} column is a {t.device.type} tensor, and there is no CPU path")
        dev = self.nmeth.device
        for name, t, dt, shape in tensors:
            if t.device != dev or t.dtype != getattr(torch, dt) or tuple(t.shape) != shape or not t.is_contiguous():
                raise MdkError(f"the {name} column must be a contiguous {dt} tensor of shape {shape} on {dev}")
        if n > 1 << 30:
            raise MdkError(f"{n} sites: more than 2^30")
        return COHORT_FORMATS[fmt], _cohort_header(fmt, names, self.merged, self.contexts_on, self.n_union), piece_bytes, dev

    def _text_stream(self, fmt, names, piece_bytes, compress, opened, sink):
        """the table's text, block by block: ``opened()`` is called once the table is measured and no row refused, then ``sink(t)`` for the
        header and for every block -- ``t`` a uint8 tensor on the device that is the library's one buffer (or its BGZF members): the sink
        uses it before it returns"""
        import torch
        code, head, piece_bytes, dev = self._text_arguments(fmt, names, piece_bytes)
        S, n = self.n_samples, len(self)
        L = lib_cohort()
        torch.cuda.current_stream(dev).synchronize()             # the columns are complete, and nothing of torch's is queued on memory it hands out next
        with _side_locks["cohort"]:                              # a handle per device, kept: its calls come from one thread at a time
            h = _cohort_handle(L, dev.index or 0, self.contigs)
            sites = md_cohort_sites(*[C.c_void_p(getattr(self, name).data_ptr()) for name, _ in SITE_COLUMNS])
            total = C.c_int64()
            _side_call(L, "cohort", "measure", h, code, C.byref(sites), C.c_void_p(self.nmeth.data_ptr()), C.c_void_p(self.nunmeth.data_ptr()), S, n, C.byref(total))
            opened()
            emit = (lambda t: sink(bgzf_compress(t, eof=False))) if compress else sink
            emit(_device_bytes(head, dev))
            buf, r0 = None, 0
            while r0 < n:
                r1, size = C.c_int64(), C.c_int64()
                _side_call(L, "cohort", "cut", h, r0, piece_bytes, C.byref(r1), C.byref(size))
                if buf is None or buf.numel() < size.value:
                    buf = None
                    buf = torch.empty(max(size.value, min(piece_bytes, total.value)), dtype=torch.uint8, device=dev)
                    torch.cuda.current_stream(dev).synchronize()
                _side_call(L, "cohort", "fill", h, r0, r1.value, C.c_void_p(buf.data_ptr()), size.value)
                emit(buf[:size.value])
                torch.cuda.current_stream(dev).synchronize()     # the sink's copies have left the buffer before the next block is made in it
                r0 = r1.value
            if compress:
                sink(_device_bytes(BGZF_EOF, dev))

    def render(self, fmt="cohort", names=None, compress=False, piece_bytes=None):
        """the bytes ``write`` would put into a file, as a uint8 tensor on the table's device"""
        import torch
        parts = []
        self._text_stream(fmt, names, piece_bytes, compress, lambda: None, lambda t: parts.append(t.clone()))
        return torch.cat(parts) if len(parts) > 1 else parts[0]

    def write(self, path, fmt="cohort", names=None, compress=False, piece_bytes=None):
        """The table as a text file, made on the device (csrc/mdk_cohort.hip); returns ``path``.  ``fmt="cohort"`` is the format
        ``Cohort.read`` takes back exactly: two ``#`` lines (the version-1 signature with the samples, ``merged``, the contexts and
        ``n_union``; then the column names, ``NAME.nmeth`` and ``NAME.nunmeth`` per sample), then one BED-like line per site, ``0 0``
        cells included: chrom, start, end (0-based, half open), CG|CHG|CHH, ``+``, ``-`` or ``.`` (strand 0), nsamples, then nmeth and
        nunmeth of every sample, tab-separated.  ``fmt="methylBase"`` is write-only: the columns of methylKit's ``getData(methylBase)``
        as ``write.table(sep="\\t", quote=FALSE, row.names=FALSE)`` lays them out -- chr, start + 1 twice, ``+`` (strand >= 0) or ``-``,
        then coverage, numCs and numTs per sample.  ``names``: the samples' names (default ``self.names``, or ``s0`` ... ``s{S-1}``).
        ``compress``: BGZF made on the device; the header is a member of its own, every block of ``piece_bytes`` (default 64 MiB; the
        longest run of whole rows that fits, at least one) is deflated by ``bgzf_compress``, and one EOF member ends the file.  Plain
        bytes depend on the table alone, compressed ones also on ``piece_bytes``; ``gzip.decompress`` of the compressed file is the
        plain one.  A negative count, a negative contig or start, a contig index outside ``contigs``, ``end <= start`` and a context
        above 2 raise MdkError (rc -3) naming the first such site (and sample) before the file is opened; so do CPU tensors: there is
        no CPU path.  Rows need not ascend to be written."""
        files, write = [], _file_writer()
        try:
            self._text_stream(fmt, names, piece_bytes, compress, lambda: files.append(open(path, "wb")), lambda t: write(files[0], t))
        finally:
            for f in files:
                f.close()
        return path

    @classmethod
    def read(cls, path, contigs, device=0, block_bytes=None):
        """A ``"cohort"`` file (``Cohort.write``) read back into a Cohort on ``device``, parsed there (k_cparse_len, k_cparse_fill):
        every column, ``names``, ``merged``, ``contexts_on`` and ``n_union`` as they were written.  ``contigs``: the contig names the
        file's first column is looked up in, in the order their indices shall have.  Plain text or BGZF, told apart by content as
        ``Calls.read`` tells them; BGZF members are inflated and CRC-checked on the device.  The file goes to the device in pieces of at
        most ``block_bytes`` bytes cut at line ends.  Strict, as ``Calls.read`` is: exactly 6 + 2S fields separated by single tabs,
        numbers of 1 to 10 digits up to INT32_MAX, a known contig, context and strand tokens, ``nsamples <= S``, ``end > start``, lines of
        at most 32768 bytes, one trailing ``\\r`` dropped, no further ``#`` line, and rows strictly ascending in (index in ``contigs``,
        start) -- a refused line raises MdkError with the path, the line's number and one reason."""
        import contextlib
        import mmap
        import torch
        contigs = list(contigs)
        block_bytes = _parse_block_bytes(block_bytes)
        kind = _gz_kind(path)
        if kind == "gzip":
            raise MdkError(f"{path}: a gzip file that is not BGZF (no BC subfield in its header): one member of any length is one wavefront's work. "
                           "Recompress it with bgzip (zcat file.gz | bgzip > file.bgz.gz), or decompress it")
        pieces = []
        with contextlib.ExitStack() as stack:
            if kind == "bgzf":
                f = stack.enter_context(open(path, "rb"))
                buf = stack.enter_context(mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ))
                members = _bgzf_members(path, buf)
                S, merged, contexts_on, n_union, names, hdr = _cohort_read_header(path, kind, buf, members)
                dev = _parse_device(device)
                source = stack.enter_context(contextlib.closing(_bgzf_pieces(_text_lib(), path, buf, members, dev, block_bytes)))
                number = _gz_line_number
            else:
                S, merged, contexts_on, n_union, names, hdr = _cohort_read_header(path, kind)
                dev = _parse_device(device)
                source, number = _parse_pieces(path, block_bytes), _parse_line_number
            L = lib_cohort()
            prev = None
            for t, cut, at in source:
                if at + cut <= hdr:
                    continue
                if kind == "bgzf":
                    d = t
                else:
                    d = torch.empty(cut, dtype=torch.uint8, device=dev)
                    d.copy_(t[:cut], non_blocking=True)
                torch.cuda.current_stream(dev).synchronize()     # the text is complete, and the pinned buffer may take the next piece
                if d.data_ptr() & 15:
                    d = d.clone()
                    torch.cuda.current_stream(dev).synchronize()
                with _side_locks["cohort"]:
                    h = _cohort_handle(L, dev.index or 0, contigs)
                    rows = C.c_int64()
                    _side_call(L, "cohort", "parse_measure", h, C.c_void_p(d.data_ptr()), cut, max(0, hdr - at), S, C.byref(rows))
                    k = rows.value
                    cols = {name: torch.empty(k, dtype=getattr(torch, dt), device=dev) for name, dt in SITE_COLUMNS}
                    m, u = (torch.empty((S, k), dtype=torch.int32, device=dev) for _ in range(2))
                    torch.cuda.current_stream(dev).synchronize()
                    sites = md_cohort_sites(*[C.c_void_p(cols[name].data_ptr()) for name, _ in SITE_COLUMNS])
                    rc = L.md_cohort_parse_fill(h, C.byref(sites), C.c_void_p(m.data_ptr()), C.c_void_p(u.data_ptr()), k, 0, k,
                                                int(prev is not None), *(prev or (0, 0)))
                    detail, off = (L.md_cohort_last_error().decode(), int(L.md_cohort_parse_error_offset(h))) if rc else (None, -1)
                if rc:
                    raise _rc_error("reading", rc, f"{path}, line {number(path, at + off)}: {detail}" if off >= 0 else f"{path}: {detail}")
                if k:
                    prev = (int(cols["contig"][-1]), int(cols["start"][-1]))
                    pieces.append((cols, m, u))
        if len(pieces) == 1:
            cols, m, u = pieces[0]
        elif pieces:
            cols = {name: torch.cat([p[0][name] for p in pieces]) for name, _ in SITE_COLUMNS}
            m, u = (torch.cat([p[i] for p in pieces], dim=1).contiguous() for i in (1, 2))
        else:
            cols = {name: torch.empty(0, dtype=getattr(torch, dt), device=dev) for name, dt in SITE_COLUMNS}
            m, u = (torch.empty((S, 0), dtype=torch.int32, device=dev) for _ in range(2))
        return cls(contigs, cols, m, u, merged, contexts_on, n_union, names)


class CohortRegions:
    """What ``Cohort.regions`` returns, on the table's device: ``contig``, ``start``, ``end`` (int32, one entry per interval: the
    intervals' own tensors, in their own order) and the matrices ``nsites`` (int32), ``nmeth`` and ``nunmeth`` (int64), ``[S, k]``
    contiguous, row s the sums of sample s.  ``contigs`` are the table's and ``names`` its sample names (or None).  There is no
    ``diff`` here: ``mdk.diff_counts(r.nmeth, r.nunmeth, a, b)`` and ``mdk.diff_replicates(r.nmeth, r.nunmeth, a, b)`` take the
    matrices as they come."""

    def __init__(self, contigs, contig, start, end, nsites, nmeth, nunmeth, names=None):
        self.contigs = contigs
        self.contig, self.start, self.end = contig, start, end
        self.nsites, self.nmeth, self.nunmeth = nsites, nmeth, nunmeth
        self.names = None if names is None else _cohort_sample_names(names, int(nmeth.shape[0]))

    def __len__(self):
        return int(self.start.shape[0])

    @property
    def n_samples(self):
        return int(self.nmeth.shape[0])

    def select(self, index):
        """a copy with the intervals ``column[index]`` (a boolean mask, an index tensor, a slice): of the three interval columns, and of
        the matrices along their interval axis"""
        return CohortRegions(self.contigs, *[t[index].contiguous() for t in (self.contig, self.start, self.end)],
                             *[t[:, index].contiguous() for t in (self.nsites, self.nmeth, self.nunmeth)], names=self.names)

    def sample(self, i):
        """sample ``i`` as a ``Regions``: the interval columns and row ``i`` of the three matrices -- views, not copies"""
        i = int(i)
        if not 0 <= i < self.n_samples:
            raise MdkError(f"sample {i}: the result holds samples 0 to {self.n_samples - 1}")
        return Regions(self.contigs, {"contig": self.contig, "start": self.start, "end": self.end, "nsites": self.nsites[i], "nmeth": self.nmeth[i], "nunmeth": self.nunmeth[i]})

    def intervals(self):
        """the intervals as an ``Intervals`` (the same tensors)"""
        return Intervals(self.contigs, self.contig, self.start, self.end)

    def moments(self, min_depth=1):
        """``Cohort.moments`` of the intervals' sums: a ``SampleMoments`` over the intervals, an interval covered for a sample if its
        ``nmeth + nunmeth >= min_depth``.  A sum of 2^26 or more is refused, as ``diff_counts`` refuses it."""
        return sample_moments(self.nmeth, self.nunmeth, min_depth, names=self.names)

    def rows(self):
        """(chrom, start, end, (nsites, nmeth, nunmeth) of sample 0, of sample 1, ...) tuples on the host"""
        cols = [t.cpu().tolist() for t in (self.contig, self.start, self.end)]
        k, m, u = (t.t().cpu().tolist() for t in (self.nsites, self.nmeth, self.nunmeth))
        return [(self.contigs[c], a, b) + tuple(zip(kk, mm, uu)) for (c, a, b), kk, mm, uu in zip(zip(*cols), k, m, u)]

    def write(self, path, names=None):
        """One ``#chrom start end NAME.nsites NAME.nmeth NAME.nunmeth ...`` line, then a line per interval, tab-separated, the contig by
        its name; formatted on the host, as ``Regions.write``.  ``names``: the samples' names (default ``self.names``, or ``s0`` ...).
        Returns the path."""
        S = self.n_samples
        names = _cohort_sample_names(names if names is not None else self.names if self.names is not None else [f"s{i}" for i in range(S)], S)
        with open(path, "w") as f:
            f.write("\t".join(["#chrom", "start", "end"] + [f"{v}.{w}" for v in names for w in ("nsites", "nmeth", "nunmeth")]) + "\n")
            f.writelines("\t".join([r[0]] + [str(v) for v in r[1:3]] + [str(v) for cell in r[3:] for v in cell]) + "\n" for r in self.rows())
        return path


DIFF_SITE_COLUMNS = (("contig", "int32"), ("start", "int32"), ("end", "int32"), ("context", "uint8"), ("strand", "int8"))
DIFF_RESULT_COLUMNS = (("nmeth_a", "int64"), ("nunmeth_a", "int64"), ("nmeth_b", "int64"), ("nunmeth_b", "int64"), ("meth_diff", "float64"), ("pvalue", "float64"))


def _diff_arguments(what, nmeth, nunmeth, a, b):
    """what ``diff_counts`` and ``diff_replicates`` ask of their arguments, checked before a library is touched: (S, n, the samples'
    marks -- 0: group a, 1: group b, -1: not used --, the matrices' device)"""
    import torch
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in (torch.int32, torch.int64):
            raise MdkError(f"{what}: {name} must be a [samples, sites] tensor of int32 or int64")
    if nmeth.dtype != nunmeth.dtype or nmeth.shape != nunmeth.shape:
        raise MdkError(f"{what}: nmeth is {nmeth.dtype} {tuple(nmeth.shape)}, nunmeth {nunmeth.dtype} {tuple(nunmeth.shape)}: one dtype and one shape")
    S, n = int(nmeth.shape[0]), int(nmeth.shape[1])
    if not 1 <= S <= MAX_SAMPLES:
        raise MdkError(f"{what} takes 1 to {MAX_SAMPLES} samples, not {S}")
    if n > 1 << 30:
        raise MdkError(f"{n} sites: more than 2^30")
    marks = [-1] * S
    for g, (label, group) in enumerate((("a", a), ("b", b))):
        group = [group] if isinstance(group, int) else list(group)
        if not group:
            raise MdkError(f"{what}: group {label} is empty")
        for i in group:
            if isinstance(i, bool) or not hasattr(i, "__index__") or not 0 <= int(i) < S:
                raise MdkError(f"{what}: group {label} names sample {i!r}: the matrices hold samples 0 to {S - 1}")
            i = int(i)
            if marks[i] == 1 - g:
                raise MdkError(f"{what}: sample {i} is in both groups")
            marks[i] = g
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if not t.is_contiguous():
            raise MdkError(f"{what}: {name} must be contiguous, sample-major")
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if t.device.type != "cuda":
            raise MdkError(f"groups are compared on the device: {name} is a {t.device.type} tensor, and there is no CPU path")
    dev = nmeth.device
    if nunmeth.device != dev:
        raise MdkError(f"{what}: nmeth is on {dev}, nunmeth on {nunmeth.device}")
    return S, n, marks, dev


def diff_counts(nmeth, nunmeth, a, b, _text=None):
    """Two groups of samples compared site by site on the device (csrc/mdk_diff.hip).  ``nmeth`` and ``nunmeth`` are two ``[S, n]``
    device tensors of one dtype, int32 or int64, contiguous, row s the counts of sample s -- a ``Cohort``'s matrices, or per-sample
    ``Regions`` sums stacked with ``torch.stack``; ``a`` and ``b`` are sequences of row indices, disjoint, neither empty; rows in
    neither are ignored.  Returns six new tensors of n entries: ``nmeth_a``, ``nunmeth_a``, ``nmeth_b``, ``nunmeth_b`` (int64: the
    groups' entries added), ``meth_diff`` (float64: 100 * (b's methylated fraction - a's), 0.0 where a group has no coverage) and
    ``pvalue`` (float64: Fisher's exact test of the pooled table, two-sided, ties as R and scipy break them; 1.0 where a group has no
    coverage, 0.0 where it would be below about 1e-280).  The p-value is made of IEEE multiplications, divisions and additions in a
    fixed order (csrc/mdk_diff_core.h): the same bits on every run and every device, exact to about (4 * support + 8) * 2^-53.  A
    negative entry, an entry of 2^26 or more and a pooled margin of 2^26 or more raise MdkError (rc -3) naming the first such site; so do
    CPU tensors: there is no CPU path.  Not here: one-sided tests; more than two groups are ``diff_groups``', the over-dispersion
    between replicates is ``diff_replicates``'s."""
    import torch
    S, n, marks, dev = _diff_arguments("diff_counts", nmeth, nunmeth, a, b)
    L = _text_lib()
    if _text is None:
        _text = _TextRenderer(L, dev.index or 0, [])         # this call's own: a stream and a status block, closed when the call returns
    text = _text
    group = torch.tensor(marks, dtype=torch.int32, device=dev)
    out = [torch.empty(n, dtype=getattr(torch, dt), device=dev) for _, dt in DIFF_RESULT_COLUMNS]
    torch.cuda.current_stream(dev).synchronize()             # the matrices are complete, and nothing of torch's is queued on memory it hands out next
    rc = L.md_text_diff(text.h, C.c_void_p(nmeth.data_ptr()), C.c_void_p(nunmeth.data_ptr()), nmeth.element_size(), S, n, C.c_void_p(group.data_ptr()),
                        *[C.c_void_p(t.data_ptr()) for t in out])
    if rc:
        raise _rc_error("md_text_diff", rc, L.md_dev_last_error().decode())
    return tuple(out)


# ---- the replicates' F test (include/mdk_stats.h, csrc/mdk_qdiff.hip -> libmdk_stats.so; the rule is csrc/mdk_qdiff_core.h) ----
REPLICATE_RESULT_COLUMNS = DIFF_RESULT_COLUMNS + (("df", "int32"), ("dispersion", "float64"), ("statistic", "float64"))
_stats = None


def lib_stats():
    """libmdk_stats.so, loaded at the first ``diff_replicates`` call: its code object's load is paid there and by no command"""
    global _stats
    if _stats is None:
        L = _load_side("stats", LIB_STATS, "statistics")
        L.md_stats_qdiff.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_double] + [C.c_void_p] * 10
        _stats = L
    return _stats


def diff_replicates(nmeth, nunmeth, a, b, min_dispersion=1.0, steps=False):
    """Two groups of REPLICATE samples compared site by site on the device (csrc/mdk_qdiff.hip): the quasi-binomial F test, where
    ``diff_counts`` has Fisher's test of the pooled table.  The arguments are ``diff_counts``'s, checked as it checks them: two ``[S,
    n]`` device tensors of one dtype, int32 or int64, contiguous, and two disjoint sequences of row indices, neither empty; rows in
    neither are not read.  Per site a sample with ``nmeth + nunmeth == 0`` is not covered and is left out; ka and kb are the covered
    samples of the groups, nu = ka + kb - 2.  The statistic is Pearson's chi-square of the pooled table divided by the dispersion:
    Pearson's residuals of the covered samples around their group's pooled fraction, squared, added and divided by nu (McCullagh and
    Nelder's estimate; methylKit's ``overdispersion="MN", test="F"`` with the score statistic in the place of the deviance), and
    ``min_dispersion`` where that is smaller -- 1.0: replicates are never taken for less variable than independent draws.  The p-value
    is P(F(1, nu) > statistic).  Returns nine new tensors of n entries: ``nmeth_a``, ``nunmeth_a``, ``nmeth_b``, ``nunmeth_b``
    (int64) and ``meth_diff`` (float64) as ``diff_counts`` gives them, ``pvalue`` (float64), ``df`` (int32: nu, 0 below 1),
    ``dispersion`` and ``statistic`` (float64); with ``steps=True`` a tenth, uint32: the terms the tail's series took.  A site with
    nothing to test -- a group without a covered sample, nu < 1 (one sample a group), nothing or everything methylated in both -- has
    pvalue 1.0, dispersion 1.0 and statistic 0.0.  All of it is IEEE multiplications, divisions and additions in one order
    (csrc/mdk_qdiff_core.h): the same bits on every run and every device; the p-value's relative error is bounded by (4 steps + 12 nu +
    32) * 2^-53 from 1e-280 up, and it is 0.0 below that.  ``min_dispersion`` is a finite float within [2^-55, 2^800].  A negative
    entry, an entry of 2^26 or more and a pooled margin of 2^26 or more raise MdkError (rc -3) naming the first such site; so do CPU
    tensors: there is no CPU path.  Not here: one-sided tests, the deviance statistic; more than two groups are ``diff_groups``',
    covariates, pairs and trends ``diff_model``'s."""
    import torch
    if isinstance(min_dispersion, bool) or not isinstance(min_dispersion, (int, float)) or not 2.0 ** -55 <= min_dispersion <= 2.0 ** 800:         # (a NaN is in no range)
        raise MdkError(f"diff_replicates: min_dispersion must be a finite number within 2^-55 and 2^800, not {min_dispersion!r}")
    S, n, marks, dev = _diff_arguments("diff_replicates", nmeth, nunmeth, a, b)
    groups = [[s for s in range(S) if marks[s] == g] for g in (0, 1)]           # each ascending: the rule's visiting order
    order = (C.c_int32 * (len(groups[0]) + len(groups[1])))(*(groups[0] + groups[1]))
    L = lib_stats()
    out = [torch.empty(n, dtype=getattr(torch, dt), device=dev) for _, dt in REPLICATE_RESULT_COLUMNS]
    if steps:
        out.append(torch.empty(n, dtype=torch.uint32, device=dev))
    torch.cuda.current_stream(dev).synchronize()             # the matrices are complete, and nothing of torch's is queued on memory it hands out next
    with _side_locks["stats"]:                               # a handle per device, kept: its calls come from one thread at a time
        h = _side_handle(L, "stats", dev.index or 0)
        _side_call(L, "stats", "qdiff", h, C.c_void_p(nmeth.data_ptr()), C.c_void_p(nunmeth.data_ptr()), nmeth.element_size(), S, n, order, len(groups[0]), len(groups[1]),
                   float(min_dispersion), *([C.c_void_p(t.data_ptr()) for t in out] + ([] if steps else [None])))
    return tuple(out)


# ---- three or more groups of replicates (include/mdk_gdiff.h, csrc/mdk_gdiff.hip in libmdk_stats.so; the rule is csrc/mdk_gdiff_core.h) ----
GROUP_RESULT_COLUMNS = (("meth_diff", "float64"), ("group_lo", "int32"), ("group_hi", "int32"), ("pvalue", "float64"), ("df", "int32"), ("df_groups", "int32"),
                        ("dispersion", "float64"), ("statistic", "float64"))


def lib_groups():
    """``lib_stats()``'s library with ``diff_groups``' call bound, at the first call that needs it: the one library and the one handle
    per device of ``diff_replicates``, ``sample_moments`` and ``count_profile``"""
    L = lib_stats()
    if "md_stats_gdiff" not in vars(L):
        L.md_stats_gdiff.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_double] + [C.c_void_p] * 11
    return L


def _group_arguments(what, nmeth, nunmeth, groups):
    """what ``diff_groups`` asks of its arguments, checked before the library is touched, in ``_diff_arguments``' words: (S, n, the groups
    as lists of row indices, each ascending -- the rule's visiting order --, the matrices' device)"""
    import torch
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in (torch.int32, torch.int64):
            raise MdkError(f"{what}: {name} must be a [samples, sites] tensor of int32 or int64")
    if nmeth.dtype != nunmeth.dtype or nmeth.shape != nunmeth.shape:
        raise MdkError(f"{what}: nmeth is {nmeth.dtype} {tuple(nmeth.shape)}, nunmeth {nunmeth.dtype} {tuple(nunmeth.shape)}: one dtype and one shape")
    S, n = int(nmeth.shape[0]), int(nmeth.shape[1])
    if not 1 <= S <= MAX_SAMPLES:
        raise MdkError(f"{what} takes 1 to {MAX_SAMPLES} samples, not {S}")
    if n > 1 << 30:
        raise MdkError(f"{n} sites: more than 2^30")
    if isinstance(groups, (str, bytes)) or not hasattr(groups, "__iter__"):
        raise MdkError(f"{what}: groups must be a sequence of 2 to {S} sequences of sample indices, not {groups!r}")
    groups = list(groups)
    if not 2 <= len(groups) <= S:
        raise MdkError(f"{what}: {len(groups)} groups: 2 to {S}, the samples of the matrices")
    marks, out = [-1] * S, []
    for g, group in enumerate(groups):
        if isinstance(group, (str, bytes)) or not (hasattr(group, "__iter__") or hasattr(group, "__index__")):
            raise MdkError(f"{what}: group {g} must be a sequence of sample indices, not {group!r}")
        group = [group] if hasattr(group, "__index__") and not hasattr(group, "__iter__") else list(group)
        if not group:
            raise MdkError(f"{what}: group {g} is empty")
        for i in group:
            if isinstance(i, bool) or not hasattr(i, "__index__") or not 0 <= int(i) < S:
                raise MdkError(f"{what}: group {g} names sample {i!r}: the matrices hold samples 0 to {S - 1}")
            i = int(i)
            if marks[i] not in (-1, g):
                raise MdkError(f"{what}: sample {i} is in both groups {marks[i]} and {g}")
            marks[i] = g
        out.append([s for s in range(S) if marks[s] == g])
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if not t.is_contiguous():
            raise MdkError(f"{what}: {name} must be contiguous, sample-major")
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if t.device.type != "cuda":
            raise MdkError(f"groups are compared on the device: {name} is a {t.device.type} tensor, and there is no CPU path")
    dev = nmeth.device
    if nunmeth.device != dev:
        raise MdkError(f"{what}: nmeth is on {dev}, nunmeth on {nunmeth.device}")
    return S, n, out, dev


def diff_groups(nmeth, nunmeth, groups, min_dispersion=1.0, steps=False):
    """THREE OR MORE groups of replicate samples compared site by site on the device (csrc/mdk_gdiff.hip): the omnibus test "some group
    differs" -- a time course, several tissues, a dose series, control / het / hom --, where ``diff_replicates`` has two groups.
    ``nmeth`` and ``nunmeth`` are ``diff_counts``' matrices, checked as it checks them -- a ``Cohort``'s, or a ``CohortRegions``' --;
    ``groups`` is a sequence of 2 to S sequences of row indices, disjoint, none empty; rows in none are not read.  Per site a sample
    with ``nmeth + nunmeth == 0`` is not covered and is left out, and so is a group without a covered sample; with g covered groups
    and k covered samples in them, q = g - 1 and nu = k - g.  The statistic is Pearson's chi-square of the pooled g x 2 table over q
    times the dispersion -- ``diff_replicates``' estimate, Pearson's residuals of the covered samples around their group's pooled
    fraction, squared, added and divided by nu, and ``min_dispersion`` where that is smaller --, and the p-value is P(F(q, nu) >
    statistic): methylKit's ``calculateDiffMeth`` for several treatment levels with ``overdispersion="MN", test="F"``, the score
    statistic in the place of the deviance.  Returns ``nmeth`` and ``nunmeth`` (int64 ``[G, n]``: the groups' entries added),
    ``meth_diff`` (float64: the most methylated covered group's percentage less the least methylated one's, never negative, which is
    what methylKit reports for several groups), ``group_lo`` and ``group_hi`` (int32: these two groups, a tie to the lower index; -1
    where no group is covered), ``pvalue`` (float64), ``df`` (int32: nu, 0 below 1), ``df_groups`` (int32: q), ``dispersion`` and
    ``statistic`` (float64); with ``steps=True`` one more, uint32: the terms the tail's series took.  A site with nothing to test --
    fewer than two covered groups, nu < 1 (one sample a group: a design without replicates), nothing or everything methylated -- has
    pvalue 1.0, dispersion 1.0 and statistic 0.0.  A site with two covered groups has ``diff_replicates``' pvalue, df, dispersion and
    statistic of them bit for bit, and so has every site of a call with two groups.  All of it is IEEE multiplications, divisions
    and additions in one order (csrc/mdk_gdiff_core.h): the same bits on every run and every device; the p-value's relative error is
    bounded by (4 steps + 12 (nu + q) + 32) * 2^-53 from 1e-280 up, and it may be 0.0 below that.  Refusals are ``diff_replicates``':
    a negative entry, an entry of 2^26 or more and a pooled margin -- a group's depth, the methylated or the unmethylated of all
    groups -- of 2^26 or more raise MdkError (rc -3) naming the first such site; so do CPU tensors: there is no CPU path.  Not here:
    the deviance statistic, one-sided tests, a chi-square p-value for designs without replicates; covariates, pairs and trend tests
    are ``diff_model``'s."""
    import torch
    if isinstance(min_dispersion, bool) or not isinstance(min_dispersion, (int, float)) or not 2.0 ** -55 <= min_dispersion <= 2.0 ** 800:         # (a NaN is in no range)
        raise MdkError(f"diff_groups: min_dispersion must be a finite number within 2^-55 and 2^800, not {min_dispersion!r}")
    S, n, groups, dev = _group_arguments("diff_groups", nmeth, nunmeth, groups)
    G = len(groups)
    flat = [s for group in groups for s in group]
    ends, at = [], 0
    for group in groups:
        at += len(group)
        ends.append(at)
    order, group_end = (C.c_int32 * len(flat))(*flat), (C.c_int32 * G)(*ends)
    L = lib_groups()
    out = [torch.empty((G, n), dtype=torch.int64, device=dev) for _ in range(2)] + [torch.empty(n, dtype=getattr(torch, dt), device=dev) for _, dt in GROUP_RESULT_COLUMNS]
    if steps:
        out.append(torch.empty(n, dtype=torch.uint32, device=dev))
    torch.cuda.current_stream(dev).synchronize()             # the matrices are complete, and nothing of torch's is queued on memory it hands out next
    with _side_locks["stats"]:                               # the handle of diff_replicates: its calls come from one thread at a time
        h = _side_handle(L, "stats", dev.index or 0)
        _side_call(L, "stats", "gdiff", h, C.c_void_p(nmeth.data_ptr()), C.c_void_p(nunmeth.data_ptr()), nmeth.element_size(), S, n, order, group_end, G,
                   float(min_dispersion), *([C.c_void_p(t.data_ptr()) for t in out] + ([] if steps else [None])))
    return tuple(out)


# ---- a design matrix: covariates, pairs, slopes (include/mdk_mdiff.h, csrc/mdk_mdiff.hip in libmdk_stats.so; the rule is csrc/mdk_mdiff_core.h) ----
MODEL_RESULT_COLUMNS = (("nmeth", "int64"), ("nunmeth", "int64"), ("pvalue", "float64"), ("df", "int32"), ("dispersion", "float64"), ("statistic", "float64"),
                        ("flags", "uint8"), ("iterations", "int32"))
MODEL_MAX_COLUMNS = 8
MODEL_FLAGS = {"rank": 1, "numeric": 2, "reduced": 4, "full": 8}          # MD_STATS_MDIFF_* of include/mdk_mdiff.h


def lib_model():
    """``lib_stats()``'s library with ``diff_model``'s call bound, at the first call that needs it: the one library and the one handle
    per device of ``diff_replicates``, ``diff_groups``, ``sample_moments`` and ``count_profile``"""
    L = lib_stats()
    if "md_stats_mdiff" not in vars(L):
        L.md_stats_mdiff.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_double), C.c_int32, C.c_int32,
                                     C.c_double] + [C.c_void_p] * 10
    return L


def _model_arguments(what, nmeth, nunmeth, design, test, samples):
    """what ``diff_model`` asks of its arguments, checked before the library is touched, in ``_diff_arguments``' words: (S, n, the used
    samples ascending, their design rows as lists with the tested columns last, p, q, the place of every column of the caller's in
    these rows, the tested columns as the caller named them, the matrices' device)"""
    import math
    import torch
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in (torch.int32, torch.int64):
            raise MdkError(f"{what}: {name} must be a [samples, sites] tensor of int32 or int64")
    if nmeth.dtype != nunmeth.dtype or nmeth.shape != nunmeth.shape:
        raise MdkError(f"{what}: nmeth is {nmeth.dtype} {tuple(nmeth.shape)}, nunmeth {nunmeth.dtype} {tuple(nunmeth.shape)}: one dtype and one shape")
    S, n = int(nmeth.shape[0]), int(nmeth.shape[1])
    if not 1 <= S <= MAX_SAMPLES:
        raise MdkError(f"{what} takes 1 to {MAX_SAMPLES} samples, not {S}")
    if n > 1 << 30:
        raise MdkError(f"{n} sites: more than 2^30")
    try:
        rows = design.detach().to("cpu", torch.float64) if isinstance(design, torch.Tensor) else torch.tensor(design, dtype=torch.float64)
    except (TypeError, ValueError, RuntimeError) as e:
        raise MdkError(f"{what}: design must be a [samples, columns] matrix of numbers: {e}") from None
    if rows.dim() != 2:
        raise MdkError(f"{what}: design must be a [samples, columns] matrix, not of the shape {tuple(rows.shape)}")
    rows = rows.tolist()
    used, p = len(rows), len(rows[0]) if rows else 0
    if not 2 <= p <= MODEL_MAX_COLUMNS:
        raise MdkError(f"{what}: a design of {p} columns: 2 to {MODEL_MAX_COLUMNS}")
    if samples is None:
        samples = range(S)
    elif isinstance(samples, (str, bytes)) or not hasattr(samples, "__iter__"):
        raise MdkError(f"{what}: samples must be a sequence of sample indices, a row of the design each, not {samples!r}")
    samples = list(samples)
    if len(samples) != used:
        raise MdkError(f"{what}: the design has {used} rows for {len(samples)} samples: a row each")
    seen = set()
    for i in samples:
        if isinstance(i, bool) or not hasattr(i, "__index__") or not 0 <= int(i) < S:
            raise MdkError(f"{what}: samples names sample {i!r}: the matrices hold samples 0 to {S - 1}")
        if int(i) in seen:
            raise MdkError(f"{what}: sample {int(i)} is named twice")
        seen.add(int(i))
    samples = [int(i) for i in samples]
    if isinstance(test, (str, bytes)) or not (hasattr(test, "__iter__") or hasattr(test, "__index__")):
        raise MdkError(f"{what}: test must be a column index of the design or a sequence of them, not {test!r}")
    tested = [test] if hasattr(test, "__index__") and not hasattr(test, "__iter__") else list(test)
    for j in tested:
        if isinstance(j, bool) or not hasattr(j, "__index__") or not 0 <= int(j) < p:
            raise MdkError(f"{what}: test names column {j!r}: the design has columns 0 to {p - 1}")
    tested = [int(j) for j in tested]
    if len(set(tested)) != len(tested):
        raise MdkError(f"{what}: test names a column twice: {tested}")
    q = len(tested)
    if not 1 <= q < p:
        raise MdkError(f"{what}: {q} tested columns of {p}: 1 to {p - 1}, a reduced model is left")
    for k, row in enumerate(rows):
        for j, v in enumerate(row):
            if not (math.isfinite(v) and abs(v) <= 2.0 ** 20):
                raise MdkError(f"{what}: the design's entry in row {k}, column {j} is {v!r}: a finite number of at most 2^20 in magnitude")
    columns = [j for j in range(p) if j not in tested] + tested          # the reduced columns first, then the tested ones: the rule's order
    by_sample = sorted(range(used), key=lambda k: samples[k])           # ascending sample index: the rule's visiting order
    rows = [[rows[k][j] for j in columns] for k in by_sample]
    place = [columns.index(j) for j in range(p)]
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if not t.is_contiguous():
            raise MdkError(f"{what}: {name} must be contiguous, sample-major")
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if t.device.type != "cuda":
            raise MdkError(f"a design is fitted on the device: {name} is a {t.device.type} tensor, and there is no CPU path")
    dev = nmeth.device
    if nunmeth.device != dev:
        raise MdkError(f"{what}: nmeth is on {dev}, nunmeth on {nunmeth.device}")
    return S, n, [samples[k] for k in by_sample], rows, p, q, place, tuple(tested), dev


def diff_model(nmeth, nunmeth, design, test, samples=None, min_dispersion=1.0, steps=False):
    """A site's counts regressed on a DESIGN MATRIX on the device (csrc/mdk_mdiff.hip), and some of its columns tested given the others:
    what ``diff_replicates`` and ``diff_groups`` cannot do -- a paired design (a dummy per patient beside the group), a batch, sex, age or
    a cell-type fraction beside the variable of interest, the slope of a dose or a time (the trend test) --, methylKit's
    ``calculateDiffMeth(covariates=...)`` with ``overdispersion="MN", test="F"``, the score statistic in the place of the deviance.
    ``nmeth`` and ``nunmeth`` are ``diff_counts``' matrices, checked as it checks them -- a ``Cohort``'s, or a ``CohortRegions``' --;
    ``design`` is anything ``[S', p]`` that converts to float64 on the host (lists, an array, a tensor), a row per used sample and 2 to
    8 columns, an intercept among them if the model is to have one; ``samples`` names the row of the matrices of every design row
    (default: rows 0 .. S' - 1 are all S samples); rows it does not name are not read.  ``test`` is a column index or a sequence of
    them: the q tested columns, 1 <= q < p; the others are the reduced model.  Per site a sample with ``nmeth + nunmeth == 0`` is not
    covered and is left out; with k covered samples nu = k - p.  The model is a binomial GLM with logit link, fitted by Newton's method
    (at most 40 passes a fit, no sample's linear predictor moved by more than 4 in a pass); the statistic is Rao's score statistic of
    the reduced model against the full one over q times the dispersion -- Pearson's sum of the FULL fit over nu, and ``min_dispersion``
    where that is smaller --, and the p-value is P(F(q, nu) > statistic).  On an intercept and group dummies that is ``diff_groups``'
    test, within the two error bounds.  Returns ``coef`` (float64 ``[p, n]``: the full model's coefficients in the design's column
    order, on the logit scale), ``nmeth`` and ``nunmeth`` (int64: the used samples' entries added), ``pvalue`` (float64), ``df``
    (int32: nu, 0 below 1), ``dispersion`` and ``statistic`` (float64), ``flags`` (uint8: the bits of ``MODEL_FLAGS``) and
    ``iterations`` (int32: the passes of both fits); with ``steps=True`` one more, uint32: the terms the tail's series took.  A site
    with nothing to test -- nu < 1, nothing or everything methylated -- has pvalue 1.0, dispersion 1.0, statistic 0.0 and coefficients
    0.0; so has a site whose covered samples leave a column of the design dependent on the others or empty (``flags & 1``, df 0) and
    one where a fit lost a pivot (``flags & 2``).  A fit that did not converge within its 40 passes is reported all the same, with
    ``flags & 4`` (the reduced fit) or ``flags & 8`` (the full one): a deep sample without a methylated read that has a column to
    itself does that.  All of it is IEEE arithmetic in one order (csrc/mdk_mdiff_core.h): the same bits on every run and every device;
    the error bound is the header's.  Refusals are ``diff_replicates``': a negative entry, an entry of 2^26 or more and a pooled
    margin of 2^26 or more raise MdkError (rc -3) naming the first such site; so do a design whose columns are dependent over its
    samples, and CPU tensors: there is no CPU path.  Not here: the deviance statistic, offsets, interactions or a formula parser, a
    meth_diff column, shrinkage, more than 8 columns."""
    import torch
    if isinstance(min_dispersion, bool) or not isinstance(min_dispersion, (int, float)) or not 2.0 ** -55 <= min_dispersion <= 2.0 ** 800:         # (a NaN is in no range)
        raise MdkError(f"diff_model: min_dispersion must be a finite number within 2^-55 and 2^800, not {min_dispersion!r}")
    S, n, used, rows, p, q, place, _, dev = _model_arguments("diff_model", nmeth, nunmeth, design, test, samples)
    order = (C.c_int32 * len(used))(*used)
    flat = (C.c_double * (len(used) * p))(*[v for row in rows for v in row])
    L = lib_model()
    coef = torch.empty((p, n), dtype=torch.float64, device=dev)
    out = [torch.empty(n, dtype=getattr(torch, dt), device=dev) for _, dt in MODEL_RESULT_COLUMNS]
    if steps:
        out.append(torch.empty(n, dtype=torch.uint32, device=dev))
    torch.cuda.current_stream(dev).synchronize()             # the matrices are complete, and nothing of torch's is queued on memory it hands out next
    with _side_locks["stats"]:                               # the handle of diff_replicates: its calls come from one thread at a time
        h = _side_handle(L, "stats", dev.index or 0)
        _side_call(L, "stats", "mdiff", h, C.c_void_p(nmeth.data_ptr()), C.c_void_p(nunmeth.data_ptr()), nmeth.element_size(), S, n, order, len(used), flat, p, q,
                   float(min_dispersion), C.c_void_p(coef.data_ptr()), *([C.c_void_p(t.data_ptr()) for t in out] + ([] if steps else [None])))
    if place != list(range(p)):
        coef = coef[torch.tensor(place, dtype=torch.int64, device=dev)].contiguous()          # the caller's column order
    return (coef,) + tuple(out)


# ---- the pairwise sample moments (include/mdk_moments.h, csrc/mdk_moments.hip in libmdk_stats.so; the rule is csrc/mdk_moments_core.h) ----
MOMENTS_WHAT = ("correlation", "covariance", "n")
MOMENTS_SHAPES = {"auto": 0, "lanes": 1, "staged": 2}          # MOM_SHAPE_* of csrc/mdk_moments.hip


def lib_moments():
    """``lib_stats()``'s library with the moments' three calls bound, at the first call that needs them: the one library and the one
    handle per device of ``diff_replicates``"""
    L = lib_stats()
    if "md_stats_moments" not in vars(L):
        L.md_stats_center.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 2
        L.md_stats_moments_limits.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.md_stats_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_int64] + [C.c_void_p] * 4
    return L


def moments_limits(device=0, shape=0, chunk_sites=0, pair_tile=0, max_workgroups=0):
    """A test hook (md_stats_moments_limits): the kernel shape (0 by S, 1 a lane per site, 2 staged in LDS; or a name of
    ``MOMENTS_SHAPES``), the sites of a staged chunk, a lane's pairs a side and the most workgroups of a launch for the
    ``sample_moments`` calls on ``device`` from now on; 0 is the default of each.  The results do not depend on them."""
    L = lib_moments()
    with _side_locks["stats"]:
        _side_call(L, "stats", "moments_limits", _side_handle(L, "stats", int(device)), int(MOMENTS_SHAPES.get(shape, shape)), int(chunk_sites), int(pair_tile), int(max_workgroups))


def _moments_arguments(nmeth, nunmeth, min_depth):
    """what ``sample_moments`` asks of its arguments, checked before the library is touched, the way ``_diff_arguments`` checks: (S, n,
    the matrices' device)"""
    import torch
    what = "sample_moments"
    if isinstance(min_depth, bool) or not isinstance(min_depth, int) or not 1 <= min_depth < 1 << 26:
        raise MdkError(f"{what}: min_depth must be an integer within 1 and 2^26 - 1, not {min_depth!r}")
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in (torch.int32, torch.int64):
            raise MdkError(f"{what}: {name} must be a [samples, sites] tensor of int32 or int64")
    if nmeth.dtype != nunmeth.dtype or nmeth.shape != nunmeth.shape:
        raise MdkError(f"{what}: nmeth is {nmeth.dtype} {tuple(nmeth.shape)}, nunmeth {nunmeth.dtype} {tuple(nunmeth.shape)}: one dtype and one shape")
    S, n = int(nmeth.shape[0]), int(nmeth.shape[1])
    if not 1 <= S <= MAX_SAMPLES:
        raise MdkError(f"{what} takes 1 to {MAX_SAMPLES} samples, not {S}")
    if n > 1 << 30:
        raise MdkError(f"{n} sites: more than 2^30")
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if not t.is_contiguous():
            raise MdkError(f"{what}: {name} must be contiguous, sample-major")
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if t.device.type != "cuda":
            raise MdkError(f"moments are summed on the device: {name} is a {t.device.type} tensor, and there is no CPU path")
    dev = nmeth.device
    if nunmeth.device != dev:
        raise MdkError(f"{what}: nmeth is on {dev}, nunmeth on {nunmeth.device}")
    return S, n, dev


def _moments_center(sums):
    """``cxy`` and ``vxx`` of the four int64 ``[S, S]`` device matrices (n, sx, sxx, sxy): md_stats_center"""
    import torch
    S, dev = int(sums[0].shape[0]), sums[0].device
    out = [torch.empty((S, S), dtype=torch.float64, device=dev) for _ in range(2)]
    L = lib_moments()
    torch.cuda.current_stream(dev).synchronize()             # the sums are complete, and nothing of torch's is queued on memory it hands out next
    with _side_locks["stats"]:
        h = _side_handle(L, "stats", dev.index or 0)
        _side_call(L, "stats", "center", h, *[C.c_void_p(t.data_ptr()) for t in sums], S, *[C.c_void_p(t.data_ptr()) for t in out])
    return out


def sample_moments(nmeth, nunmeth, min_depth=1, names=None):
    """How alike the samples of a table are -- what methylKit's ``getCorrelation``, ``clusterSamples`` and ``PCASamples`` start from --,
    summed on the device (csrc/mdk_moments.hip).  ``nmeth`` and ``nunmeth`` are two ``[S, n]`` device tensors of one dtype, int32 or
    int64, contiguous, row s the counts of sample s: a ``Cohort``'s matrices or a ``CohortRegions``'.  A cell is covered if ``nmeth +
    nunmeth >= min_depth`` (1 to 2^26 - 1); its level is the methylated fraction in units of 2^-16, rounded half up.  A ``SampleMoments``:
    over the sites where samples i and j are BOTH covered (pairwise-complete observations) their number ``n``, the sums ``sx`` of i's
    levels, ``sxx`` of their squares and ``sxy`` of the products of i's and j's -- exact integers, the same bits on every run, device
    and blocking of the kernels --, and ``cxy = n sxy - sx sx^T`` and ``vxx = n sxx - sx^2``, formed in 128-bit integers and rounded once.
    The matrices are not changed.  A negative entry and an entry of 2^26 or more raise MdkError (rc -3) naming the first such site; so do
    CPU tensors: there is no CPU path.  Not here: Spearman's correlation, weights by depth, PCA and clustering
    (``torch.linalg.eigh(moments.covariance())`` is the first of them)."""
    import torch
    S, n, dev = _moments_arguments(nmeth, nunmeth, min_depth)
    if names is not None:
        names = _cohort_sample_names(names, S)
    L = lib_moments()
    sums = [torch.empty((S, S), dtype=torch.int64, device=dev) for _ in range(4)]
    torch.cuda.current_stream(dev).synchronize()             # the matrices are complete, and nothing of torch's is queued on memory it hands out next
    with _side_locks["stats"]:                               # a handle per device, kept: its calls come from one thread at a time
        h = _side_handle(L, "stats", dev.index or 0)
        _side_call(L, "stats", "moments", h, C.c_void_p(nmeth.data_ptr()), C.c_void_p(nunmeth.data_ptr()), nmeth.element_size(), S, n, min_depth,
                   *[C.c_void_p(t.data_ptr()) for t in sums])
    return SampleMoments(*sums, *_moments_center(sums), min_depth, names)


class SampleMoments:
    """What ``sample_moments``, ``Cohort.moments`` and ``CohortRegions.moments`` return, on the table's device: ``n``, ``sx``, ``sxx``,
    ``sxy`` (int64 ``[S, S]``) and ``cxy``, ``vxx`` (float64 ``[S, S]``) as ``sample_moments`` documents them, ``min_depth``, and
    ``names``, a tuple of S sample names or None.  Row i, column j is about sample i over the sites it shares with sample j; ``n``,
    ``sxy`` and ``cxy`` are symmetric, the diagonals each sample's own.  The methods work in torch on the device from these matrices.
    ``a + b`` is the moments of two disjoint sets of sites -- chromosomes, batches -- of the same samples: the integers add, and the
    sum is centred again."""

    def __init__(self, n, sx, sxx, sxy, cxy, vxx, min_depth=1, names=None):
        self.n, self.sx, self.sxx, self.sxy, self.cxy, self.vxx = n, sx, sxx, sxy, cxy, vxx
        self.min_depth = int(min_depth)
        self.names = None if names is None else _cohort_sample_names(names, int(n.shape[0]))

    @property
    def n_samples(self):
        return int(self.n.shape[0])

    def mean(self):
        """float64 ``[S, S]``: the mean level of sample i over the sites it shares with j, ``sx / n / 65536`` -- the correctly rounded
        quotient, both integers being exact as doubles; NaN where n is 0"""
        return self.sx.double() / self.n.double() / 65536.0

    def covariance(self):
        """float64 ``[S, S]``: the sample covariance of the levels as fractions, ``cxy / (n (n - 1)) / 2^32``, within 4 * 2^-53 of the
        exact quotient; NaN where n < 2"""
        import torch
        n = self.n.double()
        c = self.cxy / (n * (n - 1.0)) / 4294967296.0
        return torch.where(self.n >= 2, c, torch.full_like(c, float("nan")))

    def correlation(self):
        """float64 ``[S, S]``: Pearson's correlation over the shared sites, ``cxy / sqrt(vxx * vxx^T)``, within 8 * 2^-53 of exact
        arithmetic and clamped to [-1, 1]; NaN where n < 2 or either sample is constant over the shared sites; the diagonal exactly
        1.0 where it is defined"""
        import torch
        vt = self.vxx.t()
        r = torch.clamp(self.cxy / torch.sqrt(self.vxx * vt), -1.0, 1.0)
        r = torch.where((self.n >= 2) & (self.vxx > 0) & (vt > 0), r, torch.full_like(r, float("nan")))
        d = torch.diagonal(r)                                 # (a view)
        d.copy_(torch.where(torch.isnan(d), d, torch.ones_like(d)))
        return r

    def distance(self):
        """``1 - correlation()``: what methylKit's ``clusterSamples`` clusters on"""
        return 1.0 - self.correlation()

    def __add__(self, other):
        import torch
        if not isinstance(other, SampleMoments):
            return NotImplemented
        if other.n_samples != self.n_samples or other.names != self.names or other.min_depth != self.min_depth:
            raise MdkError(f"moments add over the same samples and min_depth: {self.n_samples} samples {self.names} at {self.min_depth}, and {other.n_samples} {other.names} at {other.min_depth}")
        if other.n.device != self.n.device:
            raise MdkError(f"moments add on one device: {self.n.device} and {other.n.device}")
        sums = [(a + b).contiguous() for a, b in zip((self.n, self.sx, self.sxx, self.sxy), (other.n, other.sx, other.sxx, other.sxy))]
        most = int(sums[0].max())
        if most > 1 << 30:
            raise MdkError(f"{most} sites in all: more than 2^30")
        return SampleMoments(*sums, *_moments_center(sums), self.min_depth, self.names)

    def _what(self, what):
        if what not in MOMENTS_WHAT:
            raise MdkError(f"unknown matrix {what!r}: one of {', '.join(MOMENTS_WHAT)}")
        return self.n if what == "n" else getattr(self, what)()

    def rows(self, what="correlation"):
        """(name, value for sample 0, for sample 1, ...) tuples on the host, a tuple per sample: ``what`` is ``"correlation"``,
        ``"covariance"`` (floats) or ``"n"`` (ints); the names are ``self.names``, or ``s0`` ..."""
        names = self.names if self.names is not None else tuple(f"s{i}" for i in range(self.n_samples))
        return [(name,) + tuple(row) for name, row in zip(names, self._what(what).cpu().tolist())]

    def write(self, path, what="correlation"):
        """A square table as text: one ``#sample NAME ...`` line, then a line per sample, its name and its row of the matrix, tab-separated;
        doubles as ``%.17g`` (``nan`` where undefined), formatted on the host.  Returns the path."""
        rows = self.rows(what)
        with open(path, "w") as f:
            f.write("\t".join(["#sample"] + [r[0] for r in rows]) + "\n")
            f.writelines("\t".join([r[0]] + [str(v) if isinstance(v, int) else "%.17g" % v for v in r[1:]]) + "\n" for r in rows)
        return path


# ---- the count profile (include/mdk_profile.h, csrc/mdk_profile.hip in libmdk_stats.so; the rule is csrc/mdk_profile_core.h) ----
PROFILE_WHAT = ("summary", "depth", "level")
PROFILE_MAX_GROUPS, PROFILE_MAX_DEPTH_BINS, PROFILE_MAX_LEVEL_BINS = 4, 4096, 256         # PROF_MAX_* of csrc/mdk_profile_core.h
PROFILE_SUMMARY_COLUMNS = ("sample", "group", "sites", "covered", "nmeth", "nunmeth", "rate", "mean_depth", "median_depth", "max_depth")


def lib_profile():
    """``lib_stats()``'s library with the profile's two calls bound, at the first call that needs them: the one library and the one
    handle per device of ``diff_replicates`` and ``sample_moments``"""
    L = lib_stats()
    if "md_stats_profile" not in vars(L):
        L.md_stats_profile_limits.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.md_stats_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 5
    return L


def profile_limits(device=0, range_sites=0, band_samples=0, max_workgroups=0):
    """A test hook (md_stats_profile_limits): the sites of a workgroup's range (a multiple of 64), the samples of a band (1, 2 or 4)
    and the most workgroups of a launch for the ``count_profile`` calls on ``device`` from now on; 0 is the default of each.  The
    results do not depend on them."""
    L = lib_profile()
    with _side_locks["stats"]:
        _side_call(L, "stats", "profile_limits", _side_handle(L, "stats", int(device)), int(range_sites), int(band_samples), int(max_workgroups))


def _profile_arguments(nmeth, nunmeth, group, n_groups, min_depth, depth_bins, level_bins):
    """what ``count_profile`` asks of its arguments, checked before the library is touched, the way ``_moments_arguments`` checks: (S, n,
    the matrices' device)"""
    import torch
    what = "count_profile"
    for name, v, most in (("min_depth", min_depth, (1 << 26) - 1), ("n_groups", n_groups, PROFILE_MAX_GROUPS), ("depth_bins", depth_bins, PROFILE_MAX_DEPTH_BINS),
                          ("level_bins", level_bins, PROFILE_MAX_LEVEL_BINS)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= most:
            raise MdkError(f"{what}: {name} must be an integer within 1 and {'2^26 - 1' if name == 'min_depth' else most}, not {v!r}")
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in (torch.int32, torch.int64):
            raise MdkError(f"{what}: {name} must be a [samples, sites] tensor of int32 or int64")
    if nmeth.dtype != nunmeth.dtype or nmeth.shape != nunmeth.shape:
        raise MdkError(f"{what}: nmeth is {nmeth.dtype} {tuple(nmeth.shape)}, nunmeth {nunmeth.dtype} {tuple(nunmeth.shape)}: one dtype and one shape")
    S, n = int(nmeth.shape[0]), int(nmeth.shape[1])
    if not 1 <= S <= MAX_SAMPLES:
        raise MdkError(f"{what} takes 1 to {MAX_SAMPLES} samples, not {S}")
    if n > 1 << 30:
        raise MdkError(f"{n} sites: more than 2^30")
    if group is not None and (not isinstance(group, torch.Tensor) or group.dim() != 1 or group.dtype != torch.uint8 or int(group.shape[0]) != n):
        raise MdkError(f"{what}: group must be a uint8 tensor of {n} entries, one per site")
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth), ("group", group)):
        if t is not None and not t.is_contiguous():
            raise MdkError(f"{what}: {name} must be contiguous" + ("" if name == "group" else ", sample-major"))
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth), ("group", group)):
        if t is not None and t.device.type != "cuda":
            raise MdkError(f"counts are profiled on the device: {name} is a {t.device.type} tensor, and there is no CPU path")
    dev = nmeth.device
    for name, t in (("nunmeth", nunmeth), ("group", group)):
        if t is not None and t.device != dev:
            raise MdkError(f"{what}: nmeth is on {dev}, {name} on {t.device}")
    return S, n, dev


def _profile_group_names(group_names, G):
    """``group_names`` as a tuple of G names, 1 to 255 bytes of 0x21 to 0x7e each, no two alike; None stays None"""
    if group_names is None:
        return None
    try:
        return _cohort_sample_names(group_names, G)
    except MdkError as e:
        raise MdkError("group_names: " + str(e).replace("samples", "groups").replace("sample", "group")) from None


def count_profile(nmeth, nunmeth, group=None, n_groups=1, min_depth=1, depth_bins=1024, level_bins=20, names=None, group_names=None):
    """The first look at a table of counts, before ``unite`` -- what methylKit's ``getCoverageStats``, ``getMethylationStats`` and
    ``filterByCoverage`` start from: per sample and group of sites the histogram of the depths, the histogram of the methylation
    levels, the sums and the largest depth, in one pass on the device (csrc/mdk_profile.hip).  ``nmeth`` and ``nunmeth`` are two
    ``[S, n]`` device tensors of one dtype, int32 or int64, contiguous, row s the counts of sample s.  ``group`` is a contiguous uint8
    device tensor of n entries, the group of each site, every one below ``n_groups`` (1 to 4) -- a ``context`` column with
    ``n_groups=3`` --, or None: every site is in group 0.  With d = nmeth + nunmeth of a cell, a ``CountProfile`` of five int64 tensors:
    ``depth_hist`` ``[S, G, depth_bins + 1]`` counts EVERY cell, d = 0 included, bin b the cells of depth exactly b and the last,
    the overflow bin, those of ``depth_bins`` (1 to 4096) or more; ``max_depth`` ``[S, G]`` is the largest d.  A cell with d >=
    ``min_depth`` (1 to 2^26 - 1) is covered: ``level_hist`` ``[S, G, level_bins]`` counts it in bin ``min(level_bins - 1, floor(nmeth *
    level_bins / d))`` (``level_bins`` 1 to 256: equal bins of the methylated fraction, a cell all methylated in the last), and
    ``nmeth_sum`` and ``nunmeth_sum`` ``[S, G]`` add its counts.  Exact integers, the same bits on every run, device and blocking of
    the kernel; the matrices are not changed.  A negative entry, an entry of 2^26 or more and a group of ``n_groups`` or more raise
    MdkError (rc -3) naming the first such site; so do CPU tensors: there is no CPU path.  Not here: groups by strand or contig, a joint
    depth x level histogram, a level quantile, ``normalizeCoverage``."""
    import torch
    S, n, dev = _profile_arguments(nmeth, nunmeth, group, n_groups, min_depth, depth_bins, level_bins)
    if names is not None:
        names = _cohort_sample_names(names, S)
    group_names = _profile_group_names(group_names, n_groups)
    L = lib_profile()
    out = [torch.empty(shape, dtype=torch.int64, device=dev) for shape in ((S, n_groups, depth_bins + 1), (S, n_groups, level_bins), (S, n_groups), (S, n_groups), (S, n_groups))]
    torch.cuda.current_stream(dev).synchronize()             # the matrices are complete, and nothing of torch's is queued on memory it hands out next
    with _side_locks["stats"]:                               # a handle per device, kept: its calls come from one thread at a time
        h = _side_handle(L, "stats", dev.index or 0)
        _side_call(L, "stats", "profile", h, C.c_void_p(nmeth.data_ptr()), C.c_void_p(nunmeth.data_ptr()), nmeth.element_size(), S, n,
                   None if group is None else C.c_void_p(group.data_ptr()), n_groups, min_depth, depth_bins, level_bins, *[C.c_void_p(t.data_ptr()) for t in out])
    return CountProfile(*out, min_depth, names, group_names)


def _profile_by(by, context):
    """(group, n_groups, group_names) of a ``profile`` method's ``by``"""
    if by is None:
        return None, 1, None
    if by == "context":
        return context, 3, CONTEXT_FILES
    raise MdkError(f"profile: by must be \"context\" or None, not {by!r}")


class CountProfile:
    """What ``count_profile`` and the ``profile`` methods return, on the table's device: ``depth_hist`` ``[S, G, depth_bins + 1]``,
    ``level_hist`` ``[S, G, level_bins]``, ``nmeth_sum``, ``nunmeth_sum`` and ``max_depth`` ``[S, G]`` (int64) as ``count_profile``
    documents them, ``min_depth``, ``depth_bins``, ``level_bins``, ``n_samples``, ``n_groups``, and ``names`` and ``group_names``,
    tuples of S sample names and of G group names, or None.  The methods work in torch on the device from these tensors.
    ``a + b`` is the profile of two disjoint sets of sites -- chromosomes, batches -- of the same samples: the integers add, and
    ``max_depth`` is the larger."""

    def __init__(self, depth_hist, level_hist, nmeth_sum, nunmeth_sum, max_depth, min_depth=1, names=None, group_names=None):
        shape = tuple(depth_hist.shape)
        if len(shape) != 3 or shape[2] < 2 or level_hist.dim() != 3 or tuple(level_hist.shape[:2]) != shape[:2] or level_hist.shape[2] < 1 or \
                any(tuple(t.shape) != shape[:2] for t in (nmeth_sum, nunmeth_sum, max_depth)):
            raise MdkError("a CountProfile is made of [S, G, depth_bins + 1], [S, G, level_bins] and three [S, G] tensors")
        self.depth_hist, self.level_hist, self.nmeth_sum, self.nunmeth_sum, self.max_depth = depth_hist, level_hist, nmeth_sum, nunmeth_sum, max_depth
        self.min_depth = int(min_depth)
        self.names = None if names is None else _cohort_sample_names(names, shape[0])
        self.group_names = _profile_group_names(group_names, shape[1])

    @property
    def n_samples(self):
        return int(self.depth_hist.shape[0])

    @property
    def n_groups(self):
        return int(self.depth_hist.shape[1])

    @property
    def depth_bins(self):
        return int(self.depth_hist.shape[2]) - 1

    @property
    def level_bins(self):
        return int(self.level_hist.shape[2])

    def sites(self):
        """int64 ``[S, G]``: the cells counted, covered or not -- for a ``Cytosines`` the cytosines of the reference"""
        return self.depth_hist.sum(2)

    def covered(self):
        """int64 ``[S, G]``: the cells with a depth of ``min_depth`` or more"""
        return self.level_hist.sum(2)

    def breadth(self):
        """float64 ``[S, G]``: ``covered / sites``, the correctly rounded quotient; NaN where there is no site"""
        return self.covered().double() / self.sites().double()

    def mean_depth(self):
        """float64 ``[S, G]``: the mean depth of the covered cells, ``(nmeth_sum + nunmeth_sum) / covered`` -- the correctly rounded
        quotient while the sum is below 2^53; NaN where nothing is covered"""
        return (self.nmeth_sum + self.nunmeth_sum).double() / self.covered().double()

    def rate(self):
        """float64 ``[S, G]``: the methylated fraction of the covered cells' reads, ``nmeth_sum / (nmeth_sum + nunmeth_sum)`` -- the
        correctly rounded quotient while the sums are below 2^53; NaN where that is 0.  In CHH this is the usual estimate of the
        bisulfite non-conversion rate."""
        return self.nmeth_sum.double() / (self.nmeth_sum + self.nunmeth_sum).double()

    def _label(self, s, g):
        return (self.names[s] if self.names is not None else f"s{s}"), (self.group_names[g] if self.group_names is not None else "all" if self.n_groups == 1 else f"g{g}")

    def depth_quantile(self, q):
        """int64 ``[S, G]``: a percentile of the covered cells' depths, read from ``depth_hist`` without a sort and defined in integers.
        With N the covered count and k = max(1, ceil(Fraction(q) * N)) -- Fraction(q) the exact value of the float ``q``, within [0,
        1] --, the smallest depth v such that at least k covered cells have a depth of v or less, counted from bin ``min_depth`` up;
        -1 where N is 0.  So q = 0 is the smallest covered depth, q = 1 the largest, and the result is always a depth some cell has:
        the rule is not R's interpolated type 7.  If a result would lie in the overflow bin -- with ``min_depth >= depth_bins`` every
        covered cell does -- MdkError names the sample, the group and its ``max_depth``: raise ``depth_bins``."""
        import math
        from fractions import Fraction
        import torch
        if isinstance(q, bool) or not isinstance(q, (int, float)) or not 0 <= q <= 1:        # (a NaN is in no range)
            raise MdkError(f"depth_quantile: q must be a number within 0 and 1, not {q!r}")
        fq, B = Fraction(q), self.depth_bins
        hist = self.depth_hist.clone()
        hist[:, :, :min(self.min_depth, B)] = 0                                            # (at min_depth >= B every covered cell is in bin B)
        N = hist.sum(2)
        k = torch.tensor([[max(1, math.ceil(fq * v)) for v in row] for row in N.cpu().tolist()], dtype=torch.int64, device=N.device).reshape(N.shape)
        v = (hist.cumsum(2) < k.unsqueeze(2)).sum(2)                                       # the first bin at which the running count reaches k
        over = ((N > 0) & (v >= B)).nonzero()
        if over.shape[0]:
            s, g = (int(x) for x in over[0].cpu().tolist())
            name, group = self._label(s, g)
            raise MdkError(f"depth_quantile({q!r}): for sample {name}, group {group}, it lies in the overflow bin, depth {B} or more (max_depth {int(self.max_depth[s, g])}): raise depth_bins")
        return torch.where(N > 0, v, torch.full_like(v, -1))

    def median_depth(self):
        """``depth_quantile(0.5)``"""
        return self.depth_quantile(0.5)

    def __add__(self, other):
        import torch
        if not isinstance(other, CountProfile):
            return NotImplemented
        mine = (tuple(self.depth_hist.shape), tuple(self.level_hist.shape), self.min_depth, self.names, self.group_names)
        theirs = (tuple(other.depth_hist.shape), tuple(other.level_hist.shape), other.min_depth, other.names, other.group_names)
        if mine != theirs:
            raise MdkError(f"profiles add over the same samples, groups, bins and min_depth: {mine}, and {theirs}")
        if other.depth_hist.device != self.depth_hist.device:
            raise MdkError(f"profiles add on one device: {self.depth_hist.device} and {other.depth_hist.device}")
        return CountProfile(self.depth_hist + other.depth_hist, self.level_hist + other.level_hist, self.nmeth_sum + other.nmeth_sum, self.nunmeth_sum + other.nunmeth_sum,
                            torch.maximum(self.max_depth, other.max_depth), self.min_depth, self.names, self.group_names)

    def rows(self, what="summary"):
        """Tuples on the host, sample-major, then by group.  ``what="summary"``, one per (sample, group): (sample, group, sites, covered,
        nmeth_sum, nunmeth_sum, rate, mean_depth, median_depth, max_depth) -- ints but for ``rate`` and ``mean_depth``, floats that are
        NaN where nothing is covered; ``median_depth`` is -1 there, and raises as ``depth_quantile`` does where it lies in the overflow
        bin.  ``"depth"``, one per bin: (sample, group, depth, count), the last bin's ``depth`` being ``depth_bins``: that or more.
        ``"level"``, one per bin: (sample, group, bin, lower, upper, count) with the bin's bounds ``bin / level_bins`` and ``(bin + 1) /
        level_bins`` as floats.  The names are ``names`` and ``group_names``, or ``s0`` ... and ``g0`` ... (``all`` for one group)."""
        if what not in PROFILE_WHAT:
            raise MdkError(f"unknown table {what!r}: one of {', '.join(PROFILE_WHAT)}")
        S, G = self.n_samples, self.n_groups
        cells = [(s, g) + self._label(s, g) for s in range(S) for g in range(G)]
        if what == "summary":
            cols = [t.cpu().tolist() for t in (self.sites(), self.covered(), self.nmeth_sum, self.nunmeth_sum, self.rate(), self.mean_depth(), self.median_depth(), self.max_depth)]
            return [(name, group) + tuple(c[s][g] for c in cols) for s, g, name, group in cells]
        if what == "depth":
            hist = self.depth_hist.cpu().tolist()
            return [(name, group, b, v) for s, g, name, group in cells for b, v in enumerate(hist[s][g])]
        hist, L = self.level_hist.cpu().tolist(), self.level_bins
        return [(name, group, l, l / L, (l + 1) / L, v) for s, g, name, group in cells for l, v in enumerate(hist[s][g])]

    def write(self, path, what="summary"):
        """A small table as text, formatted on the host: a first line ``#count_profile WHAT min_depth=M depth_bins=B level_bins=L``, a
        second of the column names -- ``#sample group sites covered nmeth nunmeth rate mean_depth median_depth max_depth``, ``#sample
        group depth count`` or ``#sample group bin lower upper count`` --, then ``rows(what)``, a line each; all tab-separated, ints
        as they are, doubles as ``%.17g`` (``nan`` where undefined).  Returns the path."""
        rows = self.rows(what)
        columns = PROFILE_SUMMARY_COLUMNS if what == "summary" else ("sample", "group", "depth", "count") if what == "depth" else ("sample", "group", "bin", "lower", "upper", "count")
        with open(path, "w") as f:
            f.write(f"#count_profile\t{what}\tmin_depth={self.min_depth}\tdepth_bins={self.depth_bins}\tlevel_bins={self.level_bins}\n")
            f.write("#" + "\t".join(columns) + "\n")
            f.writelines("\t".join("%.17g" % v if isinstance(v, float) else str(v) for v in r) + "\n" for r in rows)
        return path


# ---- smoothing (include/mdk_smooth.h, csrc/mdk_smooth.hip -> libmdk_smooth.so; the rule is csrc/mdk_smooth_core.h) ----
SMOOTH_KERNELS = {"tricube": 0, "flat": 1}                     # SMO_* of csrc/mdk_smooth_core.h
_smooth = None


def lib_smooth():
    """libmdk_smooth.so, loaded at the first ``smooth`` call: its code object's load is paid there and by no command"""
    global _smooth
    if _smooth is None:
        L = _load_side("smooth", LIB_SMOOTH, "smoothing")
        L.md_smooth_run.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 4
        L.md_smooth_limits.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        _smooth = L
    return _smooth


def smooth_limits(device=0, tile_sites=0, chunk_sites=0, sample_batch=0, max_workgroups=0):
    """A test hook (md_smooth_limits): the sites of a workgroup's tile, the rows of a chunk it stages, the samples of a batch and the most
    workgroups of a launch for the smooth calls on ``device`` from now on; 0 is the default of each.  The results do not depend on them."""
    _side_limits(lib_smooth(), "smooth", device, tile_sites, chunk_sites, sample_batch, max_workgroups)


def _smooth_arguments(contig, start, nmeth, nunmeth, half_bases, min_sites, kernel):
    """what ``smooth_counts`` asks of its arguments, checked before the library is touched, the way ``_diff_arguments`` checks: (S, n, the
    kernel's code, the tensors' device)"""
    import torch
    what = "smooth_counts"
    for name, v, lo, hi in (("half_bases", half_bases, 0, 1 << 20), ("min_sites", min_sites, 1, 1 << 16)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise MdkError(f"{what}: {name} must be an integer within {lo} and {hi}, not {v!r}")
    if not isinstance(kernel, str) or kernel not in SMOOTH_KERNELS:
        raise MdkError(f"{what}: unknown kernel {kernel!r}: one of {', '.join(SMOOTH_KERNELS)}")
    for name, t in (("contig", contig), ("start", start)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.int32:
            raise MdkError(f"{what}: {name} must be a tensor of int32, one entry per site")
    for name, t in (("nmeth", nmeth), ("nunmeth", nunmeth)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in (torch.int32, torch.int64):
            raise MdkError(f"{what}: {name} must be a [samples, sites] tensor of int32 or int64")
    if nmeth.dtype != nunmeth.dtype or nmeth.shape != nunmeth.shape:
        raise MdkError(f"{what}: nmeth is {nmeth.dtype} {tuple(nmeth.shape)}, nunmeth {nunmeth.dtype} {tuple(nunmeth.shape)}: one dtype and one shape")
    S, n = int(nmeth.shape[0]), int(nmeth.shape[1])
    if contig.shape != (n,) or start.shape != (n,):
        raise MdkError(f"{what}: the matrices hold {n} sites, contig {tuple(contig.shape)} and start {tuple(start.shape)}")
    if not 1 <= S <= MAX_SAMPLES:
        raise MdkError(f"{what} takes 1 to {MAX_SAMPLES} samples, not {S}")
    if n > 1 << 30:
        raise MdkError(f"{n} sites: more than 2^30")
    tensors = (("contig", contig), ("start", start), ("nmeth", nmeth), ("nunmeth", nunmeth))
    for name, t in tensors:
        if not t.is_contiguous():
            raise MdkError(f"{what}: {name} must be contiguous" + (", sample-major" if t.dim() == 2 else ""))
    for name, t in tensors:
        if t.device.type != "cuda":
            raise MdkError(f"counts are smoothed on the device: {name} is a {t.device.type} tensor, and there is no CPU path")
    dev = nmeth.device
    for name, t in tensors:
        if t.device != dev:
            raise MdkError(f"{what}: nmeth is on {dev}, {name} on {t.device}")
    return S, n, SMOOTH_KERNELS[kernel], dev


def smooth_counts(contig, start, nmeth, nunmeth, half_bases=1000, min_sites=70, kernel="tricube"):
    """Kernel-weighted methylation levels of every site, per sample, on the device (csrc/mdk_smooth.hip).  ``contig`` and ``start`` are
    int32 device tensors of n sites, strictly ascending in (contig, start); ``nmeth`` and ``nunmeth`` two ``[S, n]`` device tensors of one
    dtype, int32 or int64, contiguous, row s the counts of sample s.  The window of site i reaches at least ``half_bases`` (0 to 2^20) to
    either side and holds at least ``min_sites`` (1 to 2^16) sites: with k = min(min_sites, the sites of i's contig) and d_k the distance
    to i's k-th nearest site of the contig (i itself the first), half = max(half_bases, d_k), and the window's rows are those of the
    contig within half of start[i]; a window never crosses a contig.  A row at distance d weighs (1 - (d / half)^3)^3 (``"tricube"``; 0
    at d = half, 1 where half is 0) or 1 (``"flat"``).  Returns four new tensors: ``level`` and ``depth`` (float64 ``[S, n]``: the
    weighted methylated count over the weighted depth -- NaN where that depth is 0 --, and the weighted depth), ``nsites`` and ``half``
    (int32 ``[n]``: the window's rows and its half-width).  IEEE multiplications, divisions and additions in one order, the window's
    rows ascending (csrc/mdk_smooth_core.h): the same bits on every run, every device and every blocking of the kernels; with the flat
    kernel the sums are exact integers and level the correctly rounded quotient, with tricube level is within (2 nsites + 2) * 2^-53 of
    exact arithmetic over the weights.  Rows out of order, a negative contig or start, a negative entry and an entry of 2^26 or more
    (``diff_counts``' limit) raise MdkError (rc -3) naming the first such site; so do CPU tensors: there is no CPU path.  Not here:
    local linear or quadratic fits (BSmooth's degree 2), other kernels, windows across contigs."""
    import torch
    S, n, code, dev = _smooth_arguments(contig, start, nmeth, nunmeth, half_bases, min_sites, kernel)
    L = lib_smooth()
    level, depth = (torch.empty((S, n), dtype=torch.float64, device=dev) for _ in range(2))
    nsites, half = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.current_stream(dev).synchronize()             # the columns are complete, and nothing of torch's is queued on memory it hands out next
    with _side_locks["smooth"]:                              # a handle per device, kept: its calls come from one thread at a time
        h = _side_handle(L, "smooth", dev.index or 0)
        _side_call(L, "smooth", "run", h, C.c_void_p(contig.data_ptr()), C.c_void_p(start.data_ptr()), C.c_void_p(nmeth.data_ptr()), C.c_void_p(nunmeth.data_ptr()),
                   nmeth.element_size(), S, n, int(half_bases), int(min_sites), code, *[C.c_void_p(t.data_ptr()) for t in (level, depth, nsites, half)])
    return level, depth, nsites, half


# ---- the united table as text (include/mdk_cohort.h, csrc/mdk_cohort.hip -> libmdk_cohort.so; the formats are csrc/mdk_cohort_core.h's) ----
COHORT_FORMATS = {"cohort": 0, "methylBase": 1}                # COH_FMT_* of csrc/mdk_cohort_core.h
COHORT_PIECE_BYTES = 64 << 20
COHORT_SIGNATURE = "#methyldackel_amd cohort 1"
COHORT_SITE_NAMES = ("#chrom", "start", "end", "context", "strand", "nsamples")
_cohort, _cohort_contigs = None, {}


class md_cohort_sites(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _ in (("contig", 0), ("start", 0), ("end", 0), ("context", 0), ("strand", 0), ("nsamples", 0))]


def lib_cohort():
    """libmdk_cohort.so, loaded at the first ``Cohort.write`` / ``render`` / ``read`` / ``regions`` call: its code object's load is paid there and by no command"""
    global _cohort
    if _cohort is None:
        L = _load_side("cohort", LIB_COHORT, "cohort text")
        L.md_cohort_limits.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.md_cohort_names.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_int32]
        L.md_cohort_measure.argtypes = [C.c_void_p, C.c_int, C.POINTER(md_cohort_sites), C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]
        L.md_cohort_cut.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.md_cohort_fill.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]
        L.md_cohort_parse_measure.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.md_cohort_parse_fill.argtypes = [C.c_void_p, C.POINTER(md_cohort_sites), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int32, C.c_int32]
        L.md_cohort_parse_error_offset.argtypes = [C.c_void_p]; L.md_cohort_parse_error_offset.restype = C.c_int64
        L.md_cohort_regions.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 3 + [C.c_int64, C.c_uint32, C.c_uint32, C.c_int32] + [C.c_void_p] * 3
        _cohort = L
    return _cohort


def _cohort_handle(L, device, contigs=None):
    """the device's md_cohort, opened at its first use and kept, with ``contigs`` as its contig names (uploaded when they change); the
    caller holds ``_side_locks["cohort"]``"""
    h = _side_handle(L, "cohort", device)
    if contigs is not None and _cohort_contigs.get(device) != tuple(contigs):
        blobs = [str(c).encode() for c in contigs]
        off = (C.c_uint32 * (len(blobs) + 1))(*([0] + list(itertools.accumulate(len(b) for b in blobs))))
        _cohort_contigs.pop(device, None)
        _side_call(L, "cohort", "names", h, b"".join(blobs), off, len(blobs))
        _cohort_contigs[device] = tuple(contigs)
    return h


def cohort_limits(device=0, tile_sites=0, sample_block=0, max_workgroups=0):
    """A test hook (md_cohort_limits): the sites of a tile, the samples of a block and the most workgroups of a launch for the
    ``Cohort.write`` / ``render`` / ``read`` / ``regions`` calls on ``device`` from now on; 0 is the default of each.  No byte, no column and
    no sum depends on them."""
    _side_limits(lib_cohort(), "cohort", device, tile_sites, sample_block, max_workgroups)


def _cohort_sample_names(names, S):
    """``names`` as a tuple of S sample names: 1 to 255 bytes of 0x21 to 0x7e each, no two alike"""
    if isinstance(names, (str, bytes)) or not hasattr(names, "__iter__"):
        raise MdkError("names must be a sequence of sample names")
    names = tuple(names)
    if len(names) != S:
        raise MdkError(f"{len(names)} names for {S} samples")
    for k, v in enumerate(names):
        if not isinstance(v, str) or not 1 <= len(v) <= 255 or any(not 0x21 <= ord(c) <= 0x7e for c in v):
            raise MdkError(f"the name of sample {k}, {v!r}, is not 1 to 255 bytes of 0x21 to 0x7e")
    if len(set(names)) != S:
        raise MdkError("two samples have the same name")
    return names


def _cohort_header(fmt, names, merged, contexts_on, n_union):
    """the lines in front of a table's rows, formatted on the host"""
    if fmt == "methylBase":
        return ("\t".join(["chr", "start", "end", "strand"] + [f"{w}{k + 1}" for k in range(len(names)) for w in ("coverage", "numCs", "numTs")]) + "\n").encode()
    first = "\t".join([COHORT_SIGNATURE, f"samples={len(names)}", f"merged={int(bool(merged))}", "contexts=" + ",".join(str(int(x)) for x in contexts_on), f"n_union={int(n_union)}"])
    second = "\t".join(list(COHORT_SITE_NAMES) + [f"{v}.{w}" for v in names for w in ("nmeth", "nunmeth")])
    return (first + "\n" + second + "\n").encode()


def _cohort_read_header(path, kind, buf=None, members=()):
    """the two ``#`` lines of a "cohort" file, read on the host: (S, merged, contexts_on, n_union, names, the bytes the two lines take).
    Of a BGZF file (``buf``: its bytes, ``members``: its table) the first members are inflated here until they hold two lines, unchecked:
    the device inflates and checks every member when the rows are read"""
    import re
    import zlib
    if kind == "bgzf":
        head = b""
        for _, so, sl, _, _ in members:
            if head.count(b"\n") >= 2:
                break
            try:
                head += zlib.decompressobj(-15).decompress(bytes(buf[so:so + sl]))
            except zlib.error:
                break
        lines = head.split(b"\n", 2)
        first, second = (lines[0] + b"\n" if len(lines) > 1 else lines[0]), (lines[1] + b"\n" if len(lines) > 2 else lines[1] if len(lines) > 1 else b"")
    else:
        with open(path, "rb") as f:
            first, second = f.readline(), f.readline()
    m = re.fullmatch(re.escape(COHORT_SIGNATURE) + r"\tsamples=([0-9]{1,4})\tmerged=([01])\tcontexts=((?:[012](?:,[012])*)?)\tn_union=([0-9]{1,18})\r?\n", first.decode("latin-1"))
    if not m or not 1 <= int(m.group(1)) <= MAX_SAMPLES:
        raise MdkError(f"{path}, line 1: not the signature of a version-1 cohort file ({COHORT_SIGNATURE!r}, then samples=, merged=, contexts= and n_union=)")
    S = int(m.group(1))
    fields = second.decode("latin-1").rstrip("\n").rstrip("\r").split("\t") if second.endswith(b"\n") else []
    names = [v[:-len(".nmeth")] for v in fields[6::2]]
    if len(fields) != 6 + 2 * S or tuple(fields[:6]) != COHORT_SITE_NAMES or any(a != f"{v}.nmeth" or b != f"{v}.nunmeth" for v, a, b in zip(names, fields[6::2], fields[7::2])):
        raise MdkError(f"{path}, line 2: the column names of {S} samples are {6 + 2 * S} fields, the six site columns and NAME.nmeth, NAME.nunmeth per sample")
    try:
        names = _cohort_sample_names(names, S)
    except MdkError as e:
        raise MdkError(f"{path}, line 2: {e}") from None
    return S, bool(int(m.group(2))), tuple(int(x) for x in m.group(3).split(",") if x), int(m.group(4)), names, len(first) + len(second)


class Smoothed:
    """What ``Cohort.smooth`` and ``Calls.smooth`` return, on the table's device: ``contigs``, the table's site columns (the same
    tensors: ``contig``, ``start``, ``end``, ``context``, ``strand``, and a cohort's ``nsamples``), ``level`` and ``depth`` (float64
    ``[S, n]``), ``nsites`` and ``half`` (int32 ``[n]``) as ``smooth_counts`` gives them, and the parameters ``half_bases``,
    ``min_sites`` and ``kernel`` they were made with.  ``level`` is NaN where a sample has no depth in the whole window; NaN compares
    false, so a threshold on a statistic made of levels passes such sites over."""

    def __init__(self, contigs, columns, level, depth, nsites, half, half_bases, min_sites, kernel, merged=False):
        self.contigs = contigs
        self._site_columns = tuple(columns)
        for name, t in columns.items():
            setattr(self, name, t)
        self.level, self.depth, self.nsites, self.half = level, depth, nsites, half
        self.half_bases, self.min_sites, self.kernel = int(half_bases), int(min_sites), kernel
        self.merged = bool(merged)

    def __len__(self):
        return int(self.start.shape[0])

    @property
    def n_samples(self):
        return int(self.level.shape[0])

    def select(self, index):
        """a copy with the sites ``column[index]`` (a boolean mask, an index tensor, a slice): of the site columns, of ``nsites`` and
        ``half``, and of ``level`` and ``depth`` along their site axis.  The values stay those of the whole table's windows"""
        cols = {name: getattr(self, name)[index].contiguous() for name in self._site_columns}
        return Smoothed(self.contigs, cols, self.level[:, index].contiguous(), self.depth[:, index].contiguous(), self.nsites[index].contiguous(),
                        self.half[index].contiguous(), self.half_bases, self.min_sites, self.kernel, self.merged)

    def rows(self):
        """(chrom, start, end, nsites, half, (level, depth) of sample 0, of sample 1, ...) tuples on the host"""
        cols = [getattr(self, n).cpu().tolist() for n in ("contig", "start", "end", "nsites", "half")]
        lv, dp = self.level.t().cpu().tolist(), self.depth.t().cpu().tolist()
        return [(self.contigs[c], a, b, k, h) + tuple(zip(ll, dd)) for (c, a, b, k, h), ll, dd in zip(zip(*cols), lv, dp)]


# ---- the bigWig track (include/mdk_track.h, csrc/mdk_bigwig.hip -> libmdk_track.so): Calls.render_bigwig, Calls.write_bigwig ----
TRACK_COLUMNS = ("contig", "start", "end", "nmeth", "nunmeth")
TRACK_VALUES = {"percent": 0, "coverage": 1}                   # BW_VALUE_* of csrc/mdk_bigwig_core.h
TRACK_PIECE_BYTES = 64 << 20
_track = None


def lib_track():
    """libmdk_track.so, loaded at the first ``render_bigwig`` / ``write_bigwig`` call: its code object's load is paid there and by no command"""
    global _track
    if _track is None:
        L = _load_side("track", LIB_TRACK, "track")
        L.md_track_limits.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.md_track_bigwig_measure.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int64, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64)]
        L.md_track_bigwig_fill_range.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
        _track = L
    return _track


def track_limits(device=0, max_workgroups=0, batch_sections=0):
    """A test hook (md_track_limits): at most ``max_workgroups`` workgroups per launch and ``batch_sections`` sections per batch for the
    bigWig calls on ``device`` from now on; 0 is the default of either.  The bytes do not depend on them."""
    _side_limits(lib_track(), "track", device, max_workgroups, batch_sections)


def _benjamini_hochberg(p):
    """what ``Diff.qvalue`` and ``Dmrs.qvalue`` return for the p-values ``p``: a new tensor beside it, in its order"""
    import torch
    n = int(p.shape[0])
    if not n:
        return p.clone()
    ascending, order = torch.sort(p)
    rank = torch.searchsorted(ascending, ascending, right=True)           # the rows with a p-value at most this one's
    q = ascending * float(n) / rank.to(torch.float64)
    q = torch.flip(torch.cummin(torch.flip(q, (0,)), 0).values, (0,)).clamp(max=1.0)
    out = torch.empty_like(p)
    out[order] = q
    return out


class Diff(_Columns):
    """What ``Cohort.diff`` returns, one entry per site of the cohort, on its device: ``contig``, ``start``, ``end`` (int32), ``context``
    (uint8) and ``strand`` (int8) are the cohort's own tensors; ``nmeth_a``, ``nunmeth_a``, ``nmeth_b``, ``nunmeth_b`` (int64) the
    groups' pooled counts, ``meth_diff`` (float64) the difference of their methylation in percent, b minus a, ``pvalue`` (float64)
    Fisher's exact test of the pooled table.  ``contigs`` and ``merged`` are the cohort's.  ``select`` takes a mask, an index or a slice,
    as for the other results."""
    COLUMNS = DIFF_SITE_COLUMNS + DIFF_RESULT_COLUMNS

    def __init__(self, contigs, columns, merged=False):
        super().__init__(contigs, columns)
        self.merged = bool(merged)

    def qvalue(self):
        """The p-values of the table's rows adjusted as Benjamini and Hochberg do (R's ``p.adjust(method="BH")``): in descending order of
        p, ``p * n / rank``, the running minimum, capped at 1.  A float64 tensor on the device, in the rows' order, made with torch:
        it is a sort, not a hot path.  Rows with equal p-values have the rank of the last of them, so they get equal q-values."""
        return _benjamini_hochberg(self.pvalue)

    def dmrs(self, significant, max_gap=300, max_skip=0, min_sites=3, min_diff=0.0):
        """Significant neighbouring rows joined into differentially methylated regions on the rows' device (csrc/mdk_dmr.hip; the rule
        in full: csrc/mdk_dmr_core.h) -- what DSS ``callDMR`` and metilene report.  ``significant`` is a ``torch.bool`` tensor of one
        entry per row on the rows' device, for example ``d.qvalue() < 0.01``.  A row is a candidate if it is significant, both groups
        cover it and their fractions differ; its direction is the sign of b's fraction minus a's, from the four counts alone.  A
        candidate continues the region of the candidate before it if both are on one contig and of one direction, their starts at
        most ``max_gap`` bases apart and at most ``max_skip`` rows that are no candidates between them; otherwise it begins a region.
        A region reports its span, ``nsites`` (every row of the span), ``nsig`` (its candidates), ``direction``, the four counts added
        over ALL rows of the span, and ``meth_diff`` and ``pvalue`` of these sums, bit for bit what ``diff_counts`` gives for them.
        It is kept if ``nsig >= min_sites``, ``abs(meth_diff) >= min_diff`` (percent) and the pooled difference has the direction of
        its rows (pooling can reverse it: such a region is dropped).  Returns a ``Dmrs``, ascending.  The defaults are conventions,
        not measurements: 300 bases is metilene's distance, three sites DSS's minimum.  Rows not strictly ascending in (contig,
        start), a contig index outside ``contigs``, a negative count, a count of 2^26 or more and a region whose pooled margins reach
        2^26 raise MdkError (rc -3) naming the first such row; so do CPU tensors: there is no CPU path.  Not here: smoothing, a
        minimum length in bases (``select((r.end - r.start) >= L)`` does it), merging regions of opposite direction.

        On a ``ReplicateDiff`` the joining is the same -- it takes the mask and the pooled counts, whatever test made the mask --, and
        a region's own ``pvalue`` stays Fisher's test of the pooled sums: it does not know the replicates.  The replicates' test of
        the regions is one more call, on every sample's sums over them::

            r = d.dmrs(d.qvalue() < 0.01)
            per = cohort.regions(r.intervals())
            test = mdk.diff_replicates(per.nmeth, per.nunmeth, a, b)"""
        import math
        import torch
        names = [n for n, _ in DIFF_SITE_COLUMNS[:3] + DIFF_RESULT_COLUMNS[:4]]
        cols = [getattr(self, n) for n in names]
        n = len(self)
        for what, v, low in (("max_gap", max_gap, 0), ("max_skip", max_skip, 0), ("min_sites", min_sites, 1)):
            if isinstance(v, bool) or not hasattr(v, "__index__") or not low <= int(v) <= 2 ** 31 - 1:
                raise MdkError(f"dmrs: {what} must be an integer between {low} and 2^31 - 1, not {v!r}")
        if isinstance(min_diff, bool) or not isinstance(min_diff, (int, float)) or not math.isfinite(min_diff) or min_diff < 0:
            raise MdkError(f"dmrs: min_diff must be a finite number of percent, 0 or more, not {min_diff!r}")
        if not isinstance(significant, torch.Tensor) or significant.dtype != torch.bool:
            raise MdkError("dmrs: significant must be a torch.bool tensor with one entry per row, such as d.qvalue() < 0.01")
        if significant.dim() != 1 or significant.shape[0] != n:
            raise MdkError(f"dmrs: significant has the shape {tuple(significant.shape)}: one entry per row, ({n},)")
        for t, name in zip(cols + [significant], names + ["significant"]):
            if t.device.type != "cuda":
                raise MdkError(f"regions are joined on the device: {'the ' + name + ' column' if name != 'significant' else name} is a {t.device.type} tensor, and there is no CPU path")
        dev = cols[0].device
        if significant.device != dev:
            raise MdkError(f"dmrs: significant is on {significant.device}, the rows on {dev}")
        for t, name, (_, dt) in zip(cols, names, DIFF_SITE_COLUMNS[:3] + DIFF_RESULT_COLUMNS[:4]):
            if t.device != dev or t.dtype != getattr(torch, dt) or t.dim() != 1 or not t.is_contiguous() or t.shape[0] != n:
                raise MdkError(f"dmrs: the {name} column must be a contiguous {dt} tensor on {dev} with one entry per row")
        if not significant.is_contiguous():
            raise MdkError("dmrs: significant must be contiguous")
        if n > 1 << 30:
            raise MdkError(f"{n} rows: more than 2^30")
        if not n:
            return Dmrs(list(self.contigs), {name: torch.empty(0, dtype=getattr(torch, dt), device=dev) for name, dt in DMR_COLUMNS}, merged=self.merged)
        L = self._renderer(dev)
        mask = significant.view(torch.uint8)                     # (a bool tensor holds a byte of 0 or 1 per entry)
        torch.cuda.current_stream(dev).synchronize()             # the columns are complete, and nothing of torch's is queued on memory it hands out next
        p = [C.c_void_p(t.data_ptr()) for t in cols]
        count = C.c_int64()
        rc = L.md_text_dmr_measure(self._text.h, p[0], p[1], p[2], None, None, p[3], p[4], p[5], p[6], C.c_void_p(mask.data_ptr()), n, len(self.contigs),
                                   int(max_gap), int(max_skip), int(min_sites), float(min_diff), C.byref(count))
        if rc:
            raise _rc_error("md_text_dmr_measure", rc, L.md_dev_last_error().decode())
        out = {name: torch.empty(count.value, dtype=getattr(torch, dt), device=dev) for name, dt in DMR_COLUMNS}
        rc = L.md_text_dmr_fill(self._text.h, *[C.c_void_p(out[name].data_ptr()) for name, _ in DMR_COLUMNS], count.value)
        if rc:
            raise _rc_error("md_text_dmr_fill", rc, L.md_dev_last_error().decode())
        return Dmrs(list(self.contigs), out, merged=self.merged)

    def rows(self):
        """(chrom, start, end, context, strand, nmeth_a, nunmeth_a, nmeth_b, nunmeth_b, meth_diff, pvalue) tuples on the host"""
        cols = [getattr(self, n).cpu().tolist() for n, _ in self.COLUMNS]
        return [(self.contigs[r[0]],) + r[1:] for r in zip(*cols)]

    def write(self, path):
        """the eleven columns, tab-separated, the contig by its name, without a header; formatted on the host, the two doubles with
        %.17g, which reads back to the same bits.  Returns the path."""
        with open(path, "w") as f:
            f.writelines("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.17g\t%.17g\n" % r for r in self.rows())
        return path


class ReplicateDiff(Diff):
    """What ``Cohort.diff_replicates`` returns: a ``Diff`` whose ``pvalue`` is the quasi-binomial F test's, with three columns more
    behind it -- ``df`` (int32: the covered samples of both groups less two, 0 below 1), ``dispersion`` (float64: the estimate, or the
    floor where that is larger) and ``statistic`` (float64: F).  The pooled counts and ``meth_diff`` are ``Cohort.diff``'s, bit for
    bit, so ``qvalue``, ``select`` and ``dmrs`` are ``Diff``'s own, unchanged."""
    COLUMNS = DIFF_SITE_COLUMNS + REPLICATE_RESULT_COLUMNS

    def rows(self):
        """(chrom, start, end, context, strand, nmeth_a, nunmeth_a, nmeth_b, nunmeth_b, meth_diff, pvalue, df, dispersion, statistic)
        tuples on the host"""
        return super().rows()

    def write(self, path):
        """the fourteen columns, tab-separated, the contig by its name, without a header; formatted on the host, the four doubles
        with %.17g, which reads back to the same bits.  Returns the path."""
        with open(path, "w") as f:
            f.writelines("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.17g\t%.17g\t%d\t%.17g\t%.17g\n" % r for r in self.rows())
        return path


class GroupDiff:
    """What ``Cohort.diff_groups`` returns, one entry per site of the cohort, on its device: ``contig``, ``start``, ``end`` (int32),
    ``context`` (uint8) and ``strand`` (int8) are the cohort's own tensors; ``nmeth`` and ``nunmeth`` (int64 ``[G, n]``) the groups'
    pooled counts, row g group g's; ``meth_diff`` (float64) the most methylated covered group's percentage less the least methylated
    one's, ``group_lo`` and ``group_hi`` (int32) these two groups; ``pvalue`` (float64) the quasi-binomial F test's, ``df`` and
    ``df_groups`` (int32) its degrees of freedom, ``dispersion`` and ``statistic`` (float64).  ``contigs`` and ``merged`` are the
    cohort's, ``n_groups`` is G and ``names`` the groups' names.  It is not a ``Diff``: more than two groups have no direction to join
    regions on -- ``contrast(i, j)`` gives the ``Diff`` of a pair, with its direction, Fisher's p and ``dmrs``."""
    COLUMNS = DIFF_SITE_COLUMNS + GROUP_RESULT_COLUMNS

    def __init__(self, contigs, columns, nmeth, nunmeth, merged=False, names=None, _text=None):
        self.contigs = contigs
        for name, _ in self.COLUMNS:
            setattr(self, name, columns[name])
        self.nmeth, self.nunmeth = nmeth, nunmeth
        self.merged = bool(merged)
        G = int(nmeth.shape[0])
        self.names = _cohort_sample_names(names if names is not None else [f"g{g}" for g in range(G)], G)
        self._text = _text

    def __len__(self):
        return int(self.start.shape[0])

    @property
    def n_groups(self):
        return int(self.nmeth.shape[0])

    def qvalue(self):
        """the omnibus p-values adjusted as Benjamini and Hochberg do, over the sites of this table: ``Diff.qvalue``'s rule"""
        return _benjamini_hochberg(self.pvalue)

    def select(self, index):
        """a copy with the sites ``column[index]`` (a boolean mask, an index tensor, a slice): of every column, and of the two matrices
        along their site axis"""
        cols = {name: getattr(self, name)[index].contiguous() for name, _ in self.COLUMNS}
        return GroupDiff(self.contigs, cols, self.nmeth[:, index].contiguous(), self.nunmeth[:, index].contiguous(), self.merged, self.names, self._text)

    def contrast(self, i, j):
        """Groups ``i`` and ``j`` compared as ``Cohort.diff`` compares them, from their pooled counts: a ``Diff`` with this table's site
        columns (the same tensors), group i as a and group j as b -- ``meth_diff`` j minus i, ``pvalue`` Fisher's exact test of the
        pooled 2 x 2 table --, made on the device by ``diff_counts(self.nmeth, self.nunmeth, [i], [j])``.  So a pair's direction and
        ``dmrs`` are one call away: ``g.contrast(0, 2).dmrs(g.qvalue() < 0.01)``."""
        out = diff_counts(self.nmeth, self.nunmeth, [i], [j], _text=self._text)
        cols = {name: getattr(self, name) for name, _ in DIFF_SITE_COLUMNS}
        cols.update(zip((name for name, _ in DIFF_RESULT_COLUMNS), out))
        return Diff(self.contigs, cols, merged=self.merged)

    def rows(self):
        """(chrom, start, end, context, strand, (nmeth, nunmeth) of group 0, of group 1, ..., meth_diff, group_lo, group_hi, pvalue, df,
        df_groups, dispersion, statistic) tuples on the host"""
        site = [getattr(self, n).cpu().tolist() for n, _ in DIFF_SITE_COLUMNS]
        result = [getattr(self, n).cpu().tolist() for n, _ in GROUP_RESULT_COLUMNS]
        m, u = self.nmeth.t().cpu().tolist(), self.nunmeth.t().cpu().tolist()
        return [(self.contigs[s[0]],) + s[1:] + tuple(zip(mm, uu)) + r for s, mm, uu, r in zip(zip(*site), m, u, zip(*result))]

    def write(self, path):
        """a header line -- ``#chrom start end context strand``, then ``NAME.nmeth NAME.nunmeth`` for every group, then the eight result
        columns' names --, then a line per site, tab-separated, the contig by its name; formatted on the host, the four doubles with
        %.17g, which reads back to the same bits.  Returns the path."""
        head = ["#chrom", "start", "end", "context", "strand"] + [f"{v}.{w}" for v in self.names for w in ("nmeth", "nunmeth")] + [n for n, _ in GROUP_RESULT_COLUMNS]
        G = self.n_groups
        with open(path, "w") as f:
            f.write("\t".join(head) + "\n")
            for r in self.rows():
                cells = ["%s" % r[0]] + ["%d" % v for v in r[1:5]] + ["%d" % v for pair in r[5:5 + G] for v in pair]
                d, lo, hi, p, df, dfg, phi, stat = r[5 + G:]
                f.write("\t".join(cells + ["%.17g" % d, "%d" % lo, "%d" % hi, "%.17g" % p, "%d" % df, "%d" % dfg, "%.17g" % phi, "%.17g" % stat]) + "\n")
        return path


class ModelDiff:
    """What ``Cohort.diff_model`` returns, one entry per site of the cohort, on its device: ``contig``, ``start``, ``end`` (int32),
    ``context`` (uint8) and ``strand`` (int8) are the cohort's own tensors; ``nmeth`` and ``nunmeth`` (int64) the used samples' pooled
    counts; ``coef`` (float64 ``[p, n]``) the full model's coefficients on the logit scale, row j the design's column j; ``pvalue``
    (float64) the quasi-binomial F test's of the tested columns, ``df`` (int32), ``dispersion`` and ``statistic`` (float64), ``flags``
    (uint8: the bits of ``MODEL_FLAGS``) and ``iterations`` (int32).  ``contigs`` and ``merged`` are the cohort's; ``n_columns`` is p,
    ``tested`` the tested columns as the call named them and ``names`` the columns' names.  It is not a ``Diff``: a model has no pair
    of groups to take a direction from -- ``cohort.diff(a, b).dmrs(model.qvalue() < 0.05)`` joins regions on a pair's."""
    COLUMNS = DIFF_SITE_COLUMNS + MODEL_RESULT_COLUMNS

    def __init__(self, contigs, columns, coef, tested, merged=False, names=None):
        self.contigs = contigs
        for name, _ in self.COLUMNS:
            setattr(self, name, columns[name])
        self.coef = coef
        self.merged = bool(merged)
        p = int(coef.shape[0])
        self.tested = tuple(int(j) for j in tested)
        self.names = _cohort_sample_names(names if names is not None else [f"x{j}" for j in range(p)], p)

    def __len__(self):
        return int(self.start.shape[0])

    @property
    def n_columns(self):
        return int(self.coef.shape[0])

    def qvalue(self):
        """the p-values adjusted as Benjamini and Hochberg do, over the sites of this table: ``Diff.qvalue``'s rule"""
        return _benjamini_hochberg(self.pvalue)

    def select(self, index):
        """a copy with the sites ``column[index]`` (a boolean mask, an index tensor, a slice): of every column, and of the coefficients
        along their site axis"""
        cols = {name: getattr(self, name)[index].contiguous() for name, _ in self.COLUMNS}
        return ModelDiff(self.contigs, cols, self.coef[:, index].contiguous(), self.tested, self.merged, self.names)

    def rows(self):
        """(chrom, start, end, context, strand, nmeth, nunmeth, the p coefficients as a tuple, pvalue, df, dispersion, statistic, flags,
        iterations) tuples on the host"""
        site = [getattr(self, n).cpu().tolist() for n, _ in DIFF_SITE_COLUMNS + MODEL_RESULT_COLUMNS[:2]]
        result = [getattr(self, n).cpu().tolist() for n, _ in MODEL_RESULT_COLUMNS[2:]]
        coef = self.coef.t().cpu().tolist()
        return [(self.contigs[s[0]],) + s[1:] + (tuple(c),) + r for s, c, r in zip(zip(*site), coef, zip(*result))]

    def write(self, path):
        """a header line -- ``#chrom start end context strand nmeth nunmeth``, then ``coef.NAME`` for every column of the design, then the
        six result columns' names --, then a line per site, tab-separated, the contig by its name; formatted on the host, the doubles
        with %.17g, which reads back to the same bits.  Returns the path."""
        head = ["#chrom", "start", "end", "context", "strand", "nmeth", "nunmeth"] + [f"coef.{v}" for v in self.names] + [n for n, _ in MODEL_RESULT_COLUMNS[2:]]
        with open(path, "w") as f:
            f.write("\t".join(head) + "\n")
            for r in self.rows():
                p, df, phi, stat, flags, its = r[8:]
                f.write("\t".join(["%s" % r[0]] + ["%d" % v for v in r[1:7]] + ["%.17g" % v for v in r[7]] +
                                  ["%.17g" % p, "%d" % df, "%.17g" % phi, "%.17g" % stat, "%d" % flags, "%d" % its]) + "\n")
        return path


DMR_COLUMNS = (("contig", "int32"), ("start", "int32"), ("end", "int32"), ("nsites", "int32"), ("nsig", "int32"), ("direction", "int8"),
               ("nmeth_a", "int64"), ("nunmeth_a", "int64"), ("nmeth_b", "int64"), ("nunmeth_b", "int64"), ("meth_diff", "float64"), ("pvalue", "float64"))


class Dmrs(_Columns):
    """What ``Diff.dmrs`` returns, one entry per region, ascending, on the rows' device: ``contig``, ``start``, ``end`` (int32: from
    the start of the region's first significant row to the end of its last), ``nsites`` (int32: the rows of the span, significant or
    not), ``nsig`` (int32: the significant rows that made it), ``direction`` (int8: +1 where group b is the more methylated, -1 where
    a is), ``nmeth_a``, ``nunmeth_a``, ``nmeth_b``, ``nunmeth_b`` (int64: the groups' counts added over every row of the span),
    ``meth_diff`` and ``pvalue`` (float64: of these sums, as ``diff_counts`` gives them).  ``contigs`` and ``merged`` are the rows'.
    ``select`` takes a mask, an index or a slice, as for the other results."""
    COLUMNS = DMR_COLUMNS

    def __init__(self, contigs, columns, merged=False):
        super().__init__(contigs, columns)
        self.merged = bool(merged)

    def qvalue(self):
        """the regions' p-values adjusted as Benjamini and Hochberg do, over the regions of this table: ``Diff.qvalue``'s rule"""
        return _benjamini_hochberg(self.pvalue)

    def intervals(self):
        """the regions as an ``Intervals`` on their device (the same three tensors): ``calls.regions(dmrs.intervals())`` gives a
        sample's own sums over the regions -- a row belongs to the region that holds its start, so every row of a span is counted"""
        return Intervals(self.contigs, self.contig, self.start, self.end)

    def rows(self):
        """(chrom, start, end, nsites, nsig, direction, nmeth_a, nunmeth_a, nmeth_b, nunmeth_b, meth_diff, pvalue) tuples on the host"""
        cols = [getattr(self, n).cpu().tolist() for n, _ in DMR_COLUMNS]
        return [(self.contigs[r[0]],) + r[1:] for r in zip(*cols)]

    def write(self, path):
        """the twelve columns, tab-separated, the contig by its name, without a header; formatted on the host, the two doubles with
        %.17g, which reads back to the same bits.  Returns the path."""
        with open(path, "w") as f:
            f.writelines("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.17g\t%.17g\n" % r for r in self.rows())
        return path


def unite(samples, min_samples=None, min_depth=1):
    """Several samples' calls joined into one table of sites -- what methylKit calls ``unite`` and every comparison of samples starts
    from: a ``Cohort`` of the sites at least ``min_samples`` of the samples hold (default: all of them; 1: the union), with every
    sample's counts per site, made on the samples' device (csrc/mdk_unite.hip) from the columns as they are: no key per row, no sort.
    ``samples`` is a sequence of 1 to 1024 ``Calls`` on one device with the same ``contigs`` and the same ``merged``; a row whose
    nmeth + nunmeth is below ``min_depth`` counts as absent from its sample (0 keeps ``0 0`` rows).  Every sample must be strictly
    ascending in (contig, start), as a session returns it, and the samples must agree about a site: for one (contig, start) the same
    ``end``, ``context`` and ``strand`` -- runs against one reference do; a merged CpG table and a merged CHG table do not, and cannot
    be united into one (nor can either be with per-strand rows: ``merged`` must be the same).  Rows in another order, a context above
    2, a contig index outside ``contigs``, a negative start, samples that disagree about a site of the result, and sites spread over
    more than 2^35 bases of covered extent raise MdkError (rc -3); so do CPU tensors: there is no CPU path."""
    import torch
    samples = list(samples)
    S = len(samples)
    if not 1 <= S <= MAX_SAMPLES:
        raise MdkError(f"unite takes 1 to {MAX_SAMPLES} samples, not {S}")
    if not all(isinstance(c, Calls) for c in samples):
        raise MdkError("unite takes Calls (Session.extract, Calls.read, merge_context, select)")
    first = samples[0]
    for k, c in enumerate(samples):
        if list(c.contigs) != list(first.contigs):
            raise MdkError(f"sample {k}'s contigs are not sample 0's: their indices would name other sequences")
        if c.merged != first.merged:
            raise MdkError(f"sample {k} has merged={c.merged}, sample 0 merged={first.merged}: merged and per-strand rows describe different sites")
    min_samples = S if min_samples is None else int(min_samples)
    if not 1 <= min_samples <= S:
        raise MdkError(f"min_samples must be between 1 and the number of samples, {S}")
    min_depth = int(min_depth)
    if not 0 <= min_depth <= 2 ** 31 - 1:
        raise MdkError("min_depth must be between 0 and 2^31 - 1")
    dev = first.start.device
    for k, c in enumerate(samples):
        n = int(c.start.shape[0]) if c.start.dim() else -1
        for name, dt in CALL_COLUMNS:
            t = getattr(c, name)
            if t.dtype != getattr(torch, dt) or t.dim() != 1 or not t.is_contiguous() or t.shape[0] != n:
                raise MdkError(f"sample {k}: the {name} column must be a contiguous {dt} tensor with one entry per row")
    for k, c in enumerate(samples):
        for name, _ in CALL_COLUMNS:
            t = getattr(c, name)
            if t.device.type != "cuda":
                raise MdkError(f"samples are united on the device: the {name} column of sample {k} is a {t.device.type} tensor, and there is no CPU path")
            if t.device != dev:
                raise MdkError(f"sample {k}: the {name} column is on {t.device}, sample 0 on {dev}")
    L = first._renderer(dev)
    text = first._text
    torch.cuda.current_stream(dev).synchronize()             # the columns are complete, and nothing of torch's is queued on memory it hands out next
    views = (md_text_cols * S)(*[md_text_cols(*[C.c_void_p(getattr(c, name).data_ptr()) for name, _ in CALL_COLUMNS]) for c in samples])
    n_rows = (C.c_int64 * S)(*[len(c) for c in samples])
    n_union, n_out = C.c_int64(), C.c_int64()
    rc = L.md_text_unite_measure(text.h, views, S, n_rows, min_samples, min_depth, C.byref(n_union), C.byref(n_out))
    if rc:
        raise _rc_error("md_text_unite_measure", rc, L.md_dev_last_error().decode())
    n = n_out.value
    cols = {name: torch.empty(n, dtype=getattr(torch, dt), device=dev) for name, dt in SITE_COLUMNS}
    nmeth, nunmeth = (torch.empty((S, n), dtype=torch.int32, device=dev) for _ in range(2))
    rc = L.md_text_unite_fill(text.h, *[C.c_void_p(cols[name].data_ptr()) for name, _ in SITE_COLUMNS], C.c_void_p(nmeth.data_ptr()), C.c_void_p(nunmeth.data_ptr()), n)
    if rc:
        raise _rc_error("md_text_unite_fill", rc, L.md_dev_last_error().decode())
    out = Cohort(list(first.contigs), cols, nmeth, nunmeth, first.merged, sorted(set().union(*[c.contexts_on for c in samples])), n_union.value)
    out._text = text
    return out


class Session:
    """One process, one device handle, many `extract` runs: ``Session(device=0).extract(args) -> Calls``.  ``args`` is the extract
    command line as for run_cli (without the command name).  The rows never pass through text: they are compacted on the device
    (k_calls_compact) and copied device to device into tensors torch allocated on ``torch.device("cuda", device)``; with
    ``device_tensors=False`` into CPU tensors instead.  --fraction/--counts/--logit/--methylKit/--cytosine_report are refused (rc -23),
    -o is ignored; any non-zero return code raises MdkError with ``.rc``.  The files come from the result: ``Calls.write(prefix, fmt)`` and
    ``Cytosines.write(prefix)`` make the command's text on the device, byte for byte (the format is chosen there, not on the command line).  ``perread(args) -> Reads`` runs `perRead` command lines on the
    same handle, ``mbias(args) -> Bias`` `mbias` ones, and ``cytosine_report(args) -> Cytosines`` gives the one output of `extract` that
    ``extract`` refuses: a row for every cytosine of the reference."""

    def __init__(self, device: int = 0):
        self.device = device
        self._L = _session_lib()
        h = C.c_void_p()
        rc = self._L.mdk_session_open(int(device), C.byref(h))
        if rc:
            raise _rc_error("mdk_session_open", rc)
        self._h = h

    def _run(self, command, result, args, device_tensors, entry=None):
        """one run of `command` on the handle: its mdk_<kind> object copied, column by column, into tensors -- device to device into
        tensors torch allocated on the session's device, or into CPU tensors -- and freed"""
        import torch
        if self._h is None:
            raise MdkError("the session is closed")
        L, kind = self._L, result.KIND
        argv = [command] + [str(a) for a in args]
        arr = (C.c_char_p * (len(argv) + 1))(*[os.fsencode(a) for a in argv], None)
        out = C.c_void_p()
        rc = getattr(L, f"mdk_session_{entry or command.lower()}")(self._h, len(argv), arr, C.byref(out))
        if rc:
            raise _rc_error(entry or command, rc)
        try:
            n = int(getattr(L, f"mdk_{kind}_count")(out))
            size = result._sizes(L, out, n)                     # every other column: n
            dev = torch.device("cuda", self.device) if device_tensors else torch.device("cpu")
            cols = {}
            for k, (name, dt) in enumerate(result.COLUMNS):
                m = size.get(name, n)
                t = (torch.empty if n else torch.zeros)(m, dtype=getattr(torch, dt), device=dev)
                if m and (n or name in result.ALWAYS):
                    rc = getattr(L, f"mdk_{kind}_copy")(out, k, C.c_void_p(t.data_ptr()), 0 if device_tensors else 1)
                    if rc:
                        raise _rc_error(f"copying the {name} column", rc)
                cols[name] = t
            return result._build(L, out, cols)
        finally:
            getattr(L, f"mdk_{kind}_free")(out)

    def extract(self, args, device_tensors: bool = True) -> Calls:
        return self._run("extract", Calls, args, device_tensors)

    def perread(self, args, device_tensors: bool = True) -> Reads:
        """The `perRead` command line (without the command name) on the same handle: the rows it would print, as Reads.  -o is ignored;
        any non-zero return code raises MdkError with ``.rc``.  Extract and perRead runs may alternate on one session."""
        return self._run("perRead", Reads, args, device_tensors)

    def mbias(self, args, device_tensors: bool = True) -> Bias:
        """The `mbias` command line (without the command name) on the same handle: its table, the dense histogram and the suggested inclusion
        bounds, as Bias.  Parsed as the command parses it (without --noSVG the output prefix is still required), but the prefix is ignored:
        no SVG is written and nothing is printed.  ``s.extract(args + b.options())`` is the run the suggestion is for."""
        return self._run("mbias", Bias, args, device_tensors)

    def cytosine_report(self, args, device_tensors: bool = True) -> Cytosines:
        """The `extract` command line (without the command name) run as `extract --cytosine_report` on the same handle: the rows of
        <prefix>.cytosine_report.txt as Cytosines.  --cytosine_report is implied (and accepted if given), -o is ignored, nothing is written
        or printed.  The command's semantics, not those of ``extract``'s Calls: -d does not apply, a site the variant filter drops is a
        0 0 row, uncovered cytosines are rows.  --fraction/--counts/--logit/--methylKit are refused (rc -23); --mergeContext returns what
        the command returns for it."""
        return self._run("extract", Cytosines, args, device_tensors, entry="cytosines")

    def close(self):
        if self._h is not None:
            self._L.mdk_session_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _rc_error(what, rc, detail=None):
    msg = detail or ("option not available through a session" if rc == RC_UNSUPPORTED else MDK_ERR.get(rc, "see stderr"))
    e = MdkError(f"{what} failed: rc {rc} ({msg})")
    e.rc = rc
    return e
