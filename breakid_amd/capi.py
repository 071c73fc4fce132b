"""ctypes binding of libbreakid_hip.so (include/breakid_hip.h).  The host-side mirror of the
reference's stage functions: names and argument meaning follow BreakID.cc's free functions
(get_mean_insert_size, scan_discordant_pairs, remove_isolated_pairs + find_cluster_pairs_enspan_*,
findClusterBreakPointInfoSaTag).  There is NO CPU fallback: without the built extension or without a
gfx950 device every entry point raises."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbreakid_hip.so")
_LIB = None


class BreakIDError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libbreakid_hip error %d: %s" % (code, msg))
        self.code = code


def build(verbose=False):
    """Compile the HIP extension in-tree for gfx950 (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    r = subprocess.run(cmd, capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libbreakid_hip.so failed:\n" + (r.stdout or "")[-4000:] + (r.stderr or "")[-4000:])


EXPORTS = ["bk_init", "bk_prepare_process", "bk_free", "bk_last_error", "bk_set_stream", "bk_sync", "bk_get_stream", "bk_upload_records", "bk_records", "bk_exclude_regions", "bk_isize_stats",
           "bk_discordant_pairs", "bk_mask_and_cluster", "bk_split_evidence", "bk_cluster_summary",
           "bk_split_breakpoints", "bk_normal_support", "bk_ref_support", "bk_genotype_call", "bk_clip_support", "bk_clip_reads", "bk_base_depth", "bk_clip_rescue", "bk_junctions", "bk_junction_sides", "bk_vcf_breakend_alt", "bk_evidence", "bk_unique_support", "bk_clip_consensus", "bk_junction_fit", "bk_locus_similarity", "bk_sequence_match", "bk_site_complexity", "bk_window_coverage", "bk_window_context", "bk_call_windows", "bk_fusion_frame", "bk_link_calls", "bk_locus_partners", "bk_call_partner_sites", "bk_fragment_sizes", "bk_fragment_bounds", "bk_known_calls", "bk_split_junctions", "bk_split_junction_counts", "bk_debug_split_junctions", "bk_cigar_gaps", "bk_cigar_gap_counts", "bk_clip_loci", "bk_clip_locus_counts", "bk_run", "bk_fetch", "bk_timing", "bk_timing_enable", "bk_timing_touched", "bk_group_stats", "bk_qname_hash", "bk_qname_check",
           "bk_bam_open", "bk_bam_header", "bk_bam_decode", "bk_bam_close", "bk_bam_extract", "bk_bam_names_free", "bk_bam_reads", "bk_reads_free", "bk_bam_decode_device", "bk_bam_decode_device_part", "bk_bam_decode_device_ctx", "bk_bam_dev_free", "bk_feed_release_caches", "bk_debug_bgzf_inflate", "bk_debug_bgzf_inflate_form", "bk_debug_bgzf_info", "bk_debug_std_sort", "bk_debug_scan", "bk_debug_radix_sort", "bk_debug_prims_info", "bk_sort_forms", "bk_debug_sort_info", "bk_debug_ahc", "bk_debug_points", "bk_debug_points_groups", "bk_debug_cluster_info", "bk_debug_stream_info", "bk_debug_stream_blocks", "bk_debug_cigar", "bk_debug_vote", "bk_debug_region", "bk_shard_begin", "bk_shard_get_stats", "bk_shard_set_stats",
           "bk_shard_sd_local", "bk_shard_sd_finish", "bk_shard_buffer", "bk_shard_set_buffer", "bk_shard_group_sizes",
           "bk_shard_own_groups", "bk_shard_route_candidates", "bk_shard_group_keys", "bk_shard_route_pairs", "bk_shard_group_pairs", "bk_shard_bp_cov", "bk_shard_bp_vote", "bk_shard_bp_vote_slice", "bk_shard_bp_set_voted", "bk_shard_bp_depth", "bk_shard_bp_finish"]


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise BreakIDError(abi.BK_ERR_NO_DEVICE, "libbreakid_hip.so is not built (run __graft_entry__.build()); "
                                                     "there is no CPU fallback")
        try:
            # when PyTorch-ROCm lives in the same process it must load its HIP runtime first: two copies of
            # libamdhip64 (torch's bundled one and /opt/rocm's) cannot both own the device
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        vp, u64p, dp = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)
        L.bk_init.argtypes = [C.c_int, vp, C.POINTER(C.c_char_p), C.c_int, C.POINTER(vp)]
        L.bk_free.argtypes = [vp]
        L.bk_last_error.restype = C.c_char_p
        L.bk_last_error.argtypes = [vp]
        L.bk_set_stream.argtypes = [vp, vp]
        L.bk_sync.argtypes = [vp]
        L.bk_upload_records.argtypes = [vp, C.POINTER(abi.Soa), C.c_int]
        L.bk_records.argtypes = [vp, C.POINTER(abi.Soa)]
        L.bk_exclude_regions.argtypes = [vp, C.POINTER(abi.Regions), u64p]
        L.bk_isize_stats.argtypes = [vp, dp, dp]
        L.bk_discordant_pairs.argtypes = [vp, C.c_int, C.c_double, u64p, C.POINTER(C.c_uint32)]
        L.bk_mask_and_cluster.argtypes = [vp, C.c_double, C.c_int, u64p]
        L.bk_split_evidence.argtypes = [vp, u64p]
        L.bk_cluster_summary.argtypes = [vp, C.c_double, u64p]
        L.bk_split_breakpoints.argtypes = [vp, C.c_double, u64p]
        L.bk_run.argtypes = [vp, C.c_int, C.c_int, dp, u64p]
        L.bk_normal_support.argtypes = [vp, vp, C.c_double, C.POINTER(vp), u64p]
        L.bk_ref_support.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.POINTER(vp), u64p]
        L.bk_genotype_call.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_float)]
        L.bk_clip_support.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.POINTER(vp), u64p]
        L.bk_clip_reads.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.bk_base_depth.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(vp)]
        L.bk_clip_rescue.argtypes = [vp, vp, vp, C.c_uint32] + [C.POINTER(C.c_uint32)] * 4
        L.bk_junctions.argtypes = [vp, C.POINTER(vp), u64p]
        L.bk_junction_sides.argtypes = [vp, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]
        L.bk_vcf_breakend_alt.argtypes = [C.c_char, C.c_int, C.c_char_p, C.c_uint32, C.c_int, C.c_char_p, C.c_size_t]
        L.bk_evidence.argtypes = [vp, C.POINTER(vp), u64p, C.POINTER(C.POINTER(C.c_uint64))]
        L.bk_unique_support.argtypes = [vp, C.POINTER(vp), u64p, C.POINTER(C.POINTER(C.c_uint64)), u64p]
        L.bk_clip_consensus.argtypes = [vp, C.POINTER(abi.Reads), vp, C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.bk_junction_fit.argtypes = [vp, C.POINTER(abi.RefSeq), vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.bk_locus_similarity.argtypes = [vp, C.POINTER(abi.RefSeq), vp, C.c_uint64, C.c_uint32, C.POINTER(vp)]
        L.bk_sequence_match.argtypes = [vp, C.POINTER(abi.SeqPanel), vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.bk_site_complexity.argtypes = [vp, C.POINTER(abi.RefSeq), vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.bk_window_coverage.argtypes = [vp, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
        L.bk_window_context.argtypes = [vp, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
        L.bk_call_windows.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, vp, vp]
        L.bk_fusion_frame.argtypes = [vp, C.POINTER(abi.TxModel), vp, C.c_uint64, C.POINTER(vp)]
        L.bk_link_calls.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.POINTER(vp)]
        L.bk_locus_partners.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.POINTER(vp)]
        L.bk_call_partner_sites.argtypes = [vp, C.c_double, vp]
        L.bk_fragment_sizes.argtypes = [vp, vp, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(vp)]
        L.bk_fragment_bounds.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.bk_known_calls.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, C.POINTER(vp)]
        L.bk_split_junctions.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(vp), u64p]
        L.bk_split_junction_counts.argtypes = [vp, u64p]
        L.bk_debug_split_junctions.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, vp, C.c_uint64, C.POINTER(vp), u64p]
        L.bk_cigar_gaps.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp), u64p]
        L.bk_cigar_gap_counts.argtypes = [vp, u64p]
        L.bk_clip_loci.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp), u64p]
        L.bk_clip_locus_counts.argtypes = [vp, u64p]
        L.bk_fetch.argtypes = [vp, C.c_int, C.POINTER(vp), u64p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint32)]
        L.bk_timing.argtypes = [vp, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(C.c_float)),
                                C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_int)]
        L.bk_timing_enable.argtypes = [vp, C.c_int]
        L.bk_timing_touched.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_int)]
        L.bk_debug_std_sort.argtypes = [vp, vp, vp, C.c_uint32, vp]
        L.bk_debug_scan.argtypes = [vp, C.c_int, vp, C.c_uint64, C.c_int, vp]
        L.bk_debug_radix_sort.argtypes = [vp, vp, vp, C.c_uint64, C.c_int, C.c_int, vp, vp]
        L.bk_debug_prims_info.argtypes = [u64p]
        L.bk_sort_forms.argtypes = [vp, u64p]
        L.bk_debug_sort_info.argtypes = [vp, u64p]
        L.bk_debug_ahc.argtypes = [vp, vp, vp, C.c_uint32, C.c_double, vp, vp, C.POINTER(C.c_uint32)]
        L.bk_debug_points.argtypes = [vp, C.c_int, vp, vp, C.c_uint32, C.c_double, vp, vp, C.POINTER(C.c_uint32)]
        L.bk_debug_points_groups.argtypes = [vp, C.c_int, vp, vp, vp, C.c_uint32, C.c_double, vp, vp, vp, C.POINTER(C.c_uint32)]
        L.bk_debug_cluster_info.argtypes = [u64p]
        L.bk_debug_stream_info.argtypes = [u64p]
        L.bk_debug_stream_blocks.argtypes = [C.c_uint]
        L.bk_debug_cigar.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
        L.bk_debug_vote.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_int32, C.c_int32, vp]
        L.bk_debug_region.argtypes = [vp, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32)]
        L.bk_shard_begin.argtypes = [vp, C.c_uint64, C.c_int]
        L.bk_shard_get_stats.argtypes = [vp, C.POINTER(abi.ShardStats)]
        L.bk_shard_set_stats.argtypes = [vp, C.POINTER(abi.ShardStats)]
        L.bk_shard_sd_local.argtypes = [vp, u64p, C.POINTER(vp), u64p]
        L.bk_shard_sd_finish.argtypes = [vp, vp, C.c_uint64, C.c_uint64, dp, dp]
        L.bk_shard_buffer.argtypes = [vp, C.c_int, C.POINTER(vp), u64p, C.POINTER(C.c_uint32)]
        L.bk_shard_set_buffer.argtypes = [vp, C.c_int, vp, C.c_uint64]
        L.bk_shard_group_sizes.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint32)]
        L.bk_shard_own_groups.argtypes = [vp, vp, C.c_uint32]
        L.bk_shard_route_candidates.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.POINTER(C.c_uint64))]
        L.bk_shard_group_keys.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)]
        L.bk_shard_route_pairs.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(C.POINTER(C.c_uint64))]
        L.bk_shard_group_pairs.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32]
        L.bk_shard_bp_cov.argtypes = [vp, C.c_double, C.POINTER(vp), u64p]
        L.bk_shard_bp_vote.argtypes = [vp, C.c_double, vp]
        L.bk_shard_bp_vote_slice.argtypes = [vp, C.c_double, vp, C.c_uint64, C.c_uint64, C.POINTER(vp), C.POINTER(vp)]
        L.bk_shard_bp_set_voted.argtypes = [vp, vp]
        L.bk_shard_bp_depth.argtypes = [vp, C.POINTER(vp), u64p]
        L.bk_shard_bp_finish.argtypes = [vp, vp]
        L.bk_qname_hash.restype = C.c_uint64
        L.bk_qname_hash.argtypes = [C.c_char_p, C.c_size_t]
        L.bk_qname_check.restype = C.c_uint32
        L.bk_qname_check.argtypes = [C.c_char_p, C.c_size_t]
        L.bk_bam_open.argtypes = [C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_size_t]
        L.bk_bam_header.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(C.c_uint32))]
        L.bk_bam_decode.argtypes = [vp, C.POINTER(abi.Soa), C.c_char_p, C.c_size_t]
        L.bk_bam_close.argtypes = [vp]
        L.bk_bam_extract.argtypes = [C.c_char_p, C.c_char_p, vp, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(vp), u64p, C.c_char_p, C.c_size_t]
        L.bk_bam_names_free.argtypes = [vp]
        L.bk_bam_reads.argtypes = [C.c_char_p, vp, C.c_uint64, C.POINTER(abi.Reads), C.c_char_p, C.c_size_t]
        L.bk_reads_free.argtypes = [C.POINTER(abi.Reads)]
        L.bk_reads_free.restype = None
        L.bk_bam_names_free.restype = None
        L.bk_bam_decode_device.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(abi.Soa), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_char_p)),
                                           C.POINTER(C.POINTER(C.c_uint32)), C.c_char_p, C.c_size_t]
        L.bk_bam_decode_device_part.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(abi.Soa), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_char_p)),
                                           C.POINTER(C.POINTER(C.c_uint32)), C.c_char_p, C.c_size_t]
        L.bk_bam_dev_free.argtypes = [vp]
        L.bk_feed_release_caches.argtypes = []
        L.bk_feed_release_caches.restype = None
        L.bk_bam_decode_device_ctx.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_char_p)),
                                               C.POINTER(C.POINTER(C.c_uint32)), C.c_char_p, C.c_size_t]
        L.bk_debug_bgzf_inflate.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.c_char_p, C.c_size_t]
        L.bk_debug_bgzf_inflate_form.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), C.c_int, C.c_uint64, C.c_char_p, C.c_size_t]
        L.bk_debug_bgzf_info.argtypes = [u64p]
        _LIB = L
    return _LIB


MULTI_LIB_PATH = os.path.join(_HERE, "libbreakid_rccl.so")
_MULTI = None
TRANSPORT_AUTO, TRANSPORT_RCCL, TRANSPORT_LOCAL = 0, 1, 2


def multi_lib():
    """libbreakid_rccl.so (include/breakid_multi.h), loaded behind lib(): the process then has torch's HIP runtime and RCCL, and
    the library's own references to them resolve to those copies."""
    global _MULTI
    if _MULTI is None:
        lib()
        if not os.path.exists(MULTI_LIB_PATH):
            raise BreakIDError(abi.BK_ERR_NO_DEVICE, "libbreakid_rccl.so is not built (run __graft_entry__.build())")
        M = C.CDLL(MULTI_LIB_PATH)
        vp, dp = C.c_void_p, C.POINTER(C.c_double)
        M.bk_multi_run.argtypes = [C.POINTER(abi.Soa), vp, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, C.POINTER(C.c_uint64), C.POINTER(vp),
                                   C.c_char_p, C.c_size_t]
        M.bk_multi_stats.argtypes = [vp, dp, dp, C.POINTER(vp), C.POINTER(C.c_uint32)]
        M.bk_multi_free.argtypes = [vp]
        M.bk_multi_free.restype = None
        _MULTI = M
    return _MULTI


def multi_run(contigs, cols, n_gpus, transport=TRANSPORT_LOCAL, qual=20, fast=True):
    """bk_multi_run on a host table (dict of numpy arrays as for Context.upload) -> dict with w, n_clustered, mean, sd (bk_multi_stats)
    and the cluster table of rank 0's context; the context is released (bk_multi_free) before this returns."""
    M = multi_lib()
    qc = cols.get("qcheck")
    cols = {k: np.ascontiguousarray(cols[k], dtype=dt) for k, dt in abi.SOA_COLS}
    if qc is not None:
        cols["qcheck"] = np.ascontiguousarray(qc, dtype=np.uint32)
    for k in ("cigar", "aux"):
        if cols[k].size == 0:
            cols[k] = np.zeros(1, cols[k].dtype)
    soa = abi.soa_from_numpy(cols)
    lens = np.asarray([l for _, l in contigs], dtype=np.uint32)
    names = (C.c_char_p * len(contigs))(*[n.encode() for n, _ in contigs])
    w, ncl, h = C.c_double(), C.c_uint64(), C.c_void_p()
    err = C.create_string_buffer(512)
    rc = M.bk_multi_run(C.byref(soa), lens.ctypes.data, names, len(contigs), int(n_gpus), int(transport), int(qual), int(fast), C.byref(w), C.byref(ncl), C.byref(h), err, 512)
    if rc != 0:
        raise BreakIDError(rc, err.value.decode())
    try:
        mean, sd = C.c_double(), C.c_double()
        rc = M.bk_multi_stats(h, C.byref(mean), C.byref(sd), None, None)
        if rc != 0:
            raise BreakIDError(rc, "bk_multi_stats")
        L = lib()
        clusters, _ = abi.fetch_array(L, h, lambda hh, st, d, c, g, ng: L.bk_fetch(hh, st, d, c, g, ng), abi.STAGE_CLUSTERS)
        return {"w": w.value, "n_clustered": ncl.value, "mean": mean.value, "sd": sd.value, "clusters": clusters}
    finally:
        M.bk_multi_free(h)


def prims_info():
    """The tile constants of the built primitives (bk_debug_prims_info; no GPU): BLOCK, SCAN_TILE, SCAN_ONE_MAX, RS_TILE."""
    out = (C.c_uint64 * 4)()
    rc = lib().bk_debug_prims_info(out)
    if rc != 0:
        raise BreakIDError(rc, "bk_debug_prims_info")
    return dict(zip(("BLOCK", "SCAN_TILE", "SCAN_ONE_MAX", "RS_TILE"), (int(v) for v in out)))


def bgzf_info():
    """The constants of the built GPU inflate (bk_debug_bgzf_info; no GPU), named as in abi.BGZF_INFO."""
    out = (C.c_uint64 * len(abi.BGZF_INFO))()
    rc = lib().bk_debug_bgzf_info(out)
    if rc != 0:
        raise BreakIDError(rc, "bk_debug_bgzf_info")
    return dict(zip(abi.BGZF_INFO, (int(v) for v in out)))


def bgzf_inflate_form(data, form, out_align=256):
    """A whole BGZF file image inflated on the GPU by the decoder and in the output layout named (bk_debug_bgzf_inflate_form; form:
    a sum of abi.BGZF_FORM_ROUNDS and abi.BGZF_FORM_SHARED, out_align 256 or 1): (rc, the blocks' bytes back to back or None when
    rc != 0, the error text).  No exception for a malformed stream: the return code is what the tests look at."""
    src = np.frombuffer(bytes(data), np.uint8)
    olen, err = C.c_uint64(), C.create_string_buffer(256)
    total = 0
    off = 0
    while off + 18 <= len(src):  # the sum of the blocks' ISIZE fields sizes the buffer; the library validates the headers itself
        bsize = int(src[off + 16]) | (int(src[off + 17]) << 8)
        if off + bsize + 1 > len(src):
            break
        total += int.from_bytes(src[off + bsize - 3:off + bsize + 1].tobytes(), "little")
        off += bsize + 1
    out = np.zeros(total + 16, np.uint8)
    rc = lib().bk_debug_bgzf_inflate_form(src.ctypes.data, len(src), out.ctypes.data, len(out), C.byref(olen), int(form), int(out_align), err, 256)
    if rc != 0:
        return rc, None, err.value.decode()
    return 0, out[:olen.value].tobytes(), ""


def cluster_info():
    """The constants of the built fast clustering (bk_debug_cluster_info; no GPU): FW_TILE, FW_LEVELS."""
    out = (C.c_uint64 * 2)()
    rc = lib().bk_debug_cluster_info(out)
    if rc != 0:
        raise BreakIDError(rc, "bk_debug_cluster_info")
    return dict(zip(("FW_TILE", "FW_LEVELS"), (int(v) for v in out)))


def stream_info():
    """The constants of the built stream pass (bk_debug_stream_info): STREAM_V, ST_CAND_CAP, ST_SA_CAP and RESIDENT, the number of
    blocks launch_stream takes for one resident set (0 in a process without a device; the other three need none)."""
    out = (C.c_uint64 * 4)()
    rc = lib().bk_debug_stream_info(out)
    if rc != 0:
        raise BreakIDError(rc, "bk_debug_stream_info")
    return dict(zip(("STREAM_V", "ST_CAND_CAP", "ST_SA_CAP", "RESIDENT"), (int(v) for v in out)))


def stream_blocks(blocks):
    """Cap the grid of k_stream for the whole process (bk_debug_stream_blocks); 0 = no cap, the default.  Tests only: set it back."""
    rc = lib().bk_debug_stream_blocks(int(blocks))
    if rc != 0:
        raise BreakIDError(rc, "bk_debug_stream_blocks")


def w_from(mean, sd):
    times = 2
    return times * math.sqrt(times) * (mean + 3 * sd)  # BreakID.cc:103


def genotype_call(alt, ref):
    """The library's genotype model (bk_genotype_call; no GPU): (gt, gq, vaf) with gt 0 = 0/0, 1 = 0/1, 2 = 1/1, 255 = ./.;
    vaf is a numpy float32 (NaN without evidence)."""
    gt, gq, vaf = C.c_uint8(), C.c_uint8(), C.c_float()
    rc = lib().bk_genotype_call(int(alt), int(ref), C.byref(gt), C.byref(gq), C.byref(vaf))
    if rc != 0:
        raise BreakIDError(rc, "bk_genotype_call")
    return gt.value, gq.value, np.float32(vaf.value)


def junction_sides(row):
    """The library's side rule (bk_junction_sides; no GPU) for one abi.JUNCTION row: (right1, right2, source), source 2 = split
    reads, 1 = pairs, 0 = no evidence."""
    a = np.zeros(1, abi.JUNCTION)
    a[0] = row
    r1, r2, src = C.c_uint8(), C.c_uint8(), C.c_uint8()
    rc = lib().bk_junction_sides(a.ctypes.data, C.byref(r1), C.byref(r2), C.byref(src))
    if rc != 0:
        raise BreakIDError(rc, "bk_junction_sides")
    return r1.value, r2.value, src.value


def clip_rescue(cluster, junction, clip, min_support=3):
    """The library's rescue rule (bk_clip_rescue; no GPU) for one abi.CLUSTER row with its abi.JUNCTION and abi.CLIP_SUPPORT rows:
    (pos1, pos2, n1, n2) when the unvoted cluster has a clip peak of at least min_support reads on both sides, in the directions
    its pairs give; None otherwise.  min_support = 0 raises BreakIDError(BK_ERR_ARG)."""
    c, j, s = np.zeros(1, abi.CLUSTER), np.zeros(1, abi.JUNCTION), np.zeros(1, abi.CLIP_SUPPORT)
    c[0], j[0], s[0] = cluster, junction, clip
    out = [C.c_uint32() for _ in range(4)]
    rc = lib().bk_clip_rescue(c.ctypes.data, j.ctypes.data, s.ctypes.data, int(min_support), *[C.byref(o) for o in out])
    if rc < 0:
        raise BreakIDError(rc, "bk_clip_rescue")
    return tuple(o.value for o in out) if rc == 1 else None


def call_windows(cluster, right1, right2, flank, target_len):
    """The coverage windows of one call (bk_call_windows; no GPU) for one abi.CLUSTER row, the sides bk_junction_sides gives it, the
    flank length and the reference list's lengths: five abi.COV_WINDOW rows (left and right of either cut, then the span between
    the cuts).  flank = 0 raises BreakIDError(BK_ERR_ARG)."""
    c = np.zeros(1, abi.CLUSTER)
    c[0] = cluster
    lens = np.ascontiguousarray(target_len, np.uint32)
    out = np.zeros(5, abi.COV_WINDOW)
    rc = lib().bk_call_windows(c.ctypes.data, int(right1), int(right2), int(flank), lens.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise BreakIDError(rc, "bk_call_windows")
    return out


def call_partner_sites(cluster, w):
    """The two sites of one call for Context.locus_partners (bk_call_partner_sites; no GPU) for one abi.CLUSTER row and the run's
    distance w: side s has the window [max(1, ps_min - W), ps_max + W], W = int(w), and the other side's as its partner window.
    Returns two abi.PARTNER_SITE rows."""
    c = np.zeros(1, abi.CLUSTER)
    c[0] = cluster
    out = np.zeros(2, abi.PARTNER_SITE)
    rc = lib().bk_call_partner_sites(c.ctypes.data, float(w), out.ctypes.data)
    if rc != 0:
        raise BreakIDError(rc, "bk_call_partner_sites")
    return out


def fragment_bounds(mean, sd):
    """The library's bounds for Context.fragment_sizes (bk_fragment_bounds; no GPU): (max(0, floor(mean - 3 sd)), ceil(mean + 3 sd)), both
    clamped to int32.  A non-finite value or sd < 0 raises BreakIDError(BK_ERR_ARG)."""
    lo, hi = C.c_int32(), C.c_int32()
    rc = lib().bk_fragment_bounds(float(mean), float(sd), C.byref(lo), C.byref(hi))
    if rc != 0:
        raise BreakIDError(rc, "bk_fragment_bounds")
    return lo.value, hi.value


def vcf_breakend_alt(ref_base, own_right, mate_chr, mate_pos, mate_right, cap=None):
    """The ALT text of one VCF breakend (bk_vcf_breakend_alt; no GPU).  cap: the buffer size handed to the library (default: large
    enough); a buffer that is too small raises BreakIDError(BK_ERR_ARG)."""
    chrom = mate_chr.encode()
    if cap is None:
        cap = len(chrom) + 32
    buf = C.create_string_buffer(max(int(cap), 1))
    rc = lib().bk_vcf_breakend_alt(ref_base.encode(), int(bool(own_right)), chrom, int(mate_pos), int(bool(mate_right)), buf, int(cap))
    if rc != 0:
        raise BreakIDError(rc, "bk_vcf_breakend_alt")
    return buf.value.decode()


class Context:
    """One GPU context = the state the reference keeps in main() between BreakID.cc:93 and :167."""

    def __init__(self, contigs, device=0):
        self.L = lib()
        self.contigs = list(contigs)
        lens = np.asarray([l for _, l in contigs], dtype=np.uint32)
        names = (C.c_char_p * len(contigs))(*[n.encode() for n, _ in contigs])
        h = C.c_void_p()
        rc = self.L.bk_init(device, lens.ctypes.data, names, len(contigs), C.byref(h))
        if rc != 0:
            raise BreakIDError(rc, (self.L.bk_last_error(None) or b"").decode())
        self.h = h
        self._keep = None

    def close(self):
        if self.h:
            self.L.bk_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise BreakIDError(rc, (self.L.bk_last_error(self.h) or b"").decode())

    def set_stream(self, hip_stream_handle):
        self._check(self.L.bk_set_stream(self.h, C.c_void_p(hip_stream_handle)))

    def sync(self):
        self._check(self.L.bk_sync(self.h))

    def upload(self, cols):
        """cols: dict of numpy arrays (host) laid out as abi.SOA_COLS."""
        qc = cols.get("qcheck")
        cols = {k: np.ascontiguousarray(cols[k], dtype=dt) for k, dt in abi.SOA_COLS}
        if qc is not None:
            cols["qcheck"] = np.ascontiguousarray(qc, dtype=np.uint32)
        for k in ("cigar", "aux"):
            if cols[k].size == 0:
                cols[k] = np.zeros(1, cols[k].dtype)
        soa = abi.soa_from_numpy(cols)
        self._keep = (cols, soa)
        self._check(self.L.bk_upload_records(self.h, C.byref(soa), abi.BK_MEM_HOST))

    def attach_device_table(self, table):
        """table: DeviceBamTable; the columns are used in place (BK_MEM_DEVICE)"""
        self._keep = table
        self._check(self.L.bk_upload_records(self.h, C.byref(table.soa), abi.BK_MEM_DEVICE))

    def upload_soa(self, handle):
        """handle: BamTable from decode_bam(keep=True); the decoder's (pinned) columns go straight to bk_upload_records."""
        self._keep = handle
        self._check(self.L.bk_upload_records(self.h, C.byref(handle.soa), abi.BK_MEM_HOST))

    def attach_device(self, ptrs, n, n_cigar_words, n_aux_bytes):
        """ptrs: dict name -> device pointer (int) of columns already resident in HBM."""
        s = abi.Soa()
        s.n = n
        for name, _ in abi.SOA_COLS:
            setattr(s, name, ptrs[name])
        if ptrs.get("qcheck"):
            s.qcheck = ptrs["qcheck"]
        if ptrs.get("side"):
            s.side = ptrs["side"]
        s.n_cigar_words = n_cigar_words
        s.n_aux_bytes = n_aux_bytes
        self._keep = (ptrs, s)
        self._check(self.L.bk_upload_records(self.h, C.byref(s), abi.BK_MEM_DEVICE))

    def exclude_regions(self, tid, beg, end):
        """Take the records that overlap any interval [beg[k], end[k]) on contig tid[k] out of the uploaded table (bk_exclude_regions:
        after upload / attach, before isize_stats).  Returns the number of records removed."""
        tid, beg, end = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (tid, beg, end))
        if not len(tid) == len(beg) == len(end):
            raise ValueError("exclude_regions: tid, beg and end differ in length")
        r = abi.Regions(tid.ctypes.data, beg.ctypes.data, end.ctypes.data, len(tid))
        n = C.c_uint64()
        self._check(self.L.bk_exclude_regions(self.h, C.byref(r), C.byref(n)))
        return n.value

    def isize_stats(self):
        m, s = C.c_double(), C.c_double()
        self._check(self.L.bk_isize_stats(self.h, C.byref(m), C.byref(s)))
        return m.value, s.value

    # ---- one sample over several contexts: the statistics steps of the bk_shard_* sequence (sharded.py drives the whole of it) ----
    def shard_begin(self, rec_base, qual=20):
        """the stream pass of a context that holds records [rec_base, rec_base + n) of the sample"""
        self._check(self.L.bk_shard_begin(self.h, int(rec_base), int(qual)))

    def shard_get_stats(self):
        st = abi.ShardStats()
        self._check(self.L.bk_shard_get_stats(self.h, C.byref(st)))
        return st

    def shard_set_stats(self, st):
        """st: abi.ShardStats with the sums (isize_sum, isize_n, sumsq) and maxima (vmax, max_span) over all shards"""
        self._check(self.L.bk_shard_set_stats(self.h, C.byref(st)))

    def shard_sd_local(self):
        """(sum of floor(d) over this shard, device pointer of its exception list, its length); an exception is 16 bytes: l_before
        (uint64, relative to this shard) and d (double)"""
        lt, ex, nex = C.c_uint64(), C.c_void_p(), C.c_uint64()
        self._check(self.L.bk_shard_sd_local(self.h, C.byref(lt), C.byref(ex), C.byref(nex)))
        return lt.value, ex.value, nex.value

    def shard_sd_finish(self, all_ex_ptr, n_all, l_grand):
        """replays the exceptions of all shards (device memory, sample order, l_before made global) -> (mean, sd)"""
        m, s = C.c_double(), C.c_double()
        self._check(self.L.bk_shard_sd_finish(self.h, C.c_void_p(all_ex_ptr or 0), int(n_all), int(l_grand), C.byref(m), C.byref(s)))
        return m.value, s.value

    def discordant_pairs(self, qual, w):
        n, g = C.c_uint64(), C.c_uint32()
        self._check(self.L.bk_discordant_pairs(self.h, qual, w, C.byref(n), C.byref(g)))
        return n.value, g.value

    def mask_and_cluster(self, w, fast):
        n = C.c_uint64()
        self._check(self.L.bk_mask_and_cluster(self.h, w, int(fast), C.byref(n)))
        return n.value

    def split_evidence(self):
        n = C.c_uint64()
        self._check(self.L.bk_split_evidence(self.h, C.byref(n)))
        return n.value

    def cluster_summary(self, w):
        n = C.c_uint64()
        self._check(self.L.bk_cluster_summary(self.h, w, C.byref(n)))
        return n.value

    def split_breakpoints(self, w, count=True):
        n = C.c_uint64()
        self._check(self.L.bk_split_breakpoints(self.h, w, C.byref(n) if count else None))
        return n.value

    def normal_support(self, normal, w):
        """Matched-normal evidence of this (tumour) context's clusters: one abi.NORMAL_SUPPORT row per STAGE_CLUSTERS row.
        `normal`: a Context on the same device and reference list, after isize_stats, discordant_pairs(same qual, w) and
        split_evidence; `w`: the tumour's distance."""
        data, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bk_normal_support(self.h, normal.h, w, C.byref(data), C.byref(n)))
        if not n.value:
            return np.zeros(0, abi.NORMAL_SUPPORT)
        buf = (C.c_char * (n.value * abi.NORMAL_SUPPORT.itemsize)).from_address(data.value)
        return np.frombuffer(buf, dtype=abi.NORMAL_SUPPORT, count=n.value).copy()

    def junctions(self):
        """Junction evidence of this context's clusters (bk_junctions): one abi.JUNCTION row per STAGE_CLUSTERS row, same order."""
        data, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bk_junctions(self.h, C.byref(data), C.byref(n)))
        if not n.value:
            return np.zeros(0, abi.JUNCTION)
        buf = (C.c_char * (n.value * abi.JUNCTION.itemsize)).from_address(data.value)
        return np.frombuffer(buf, dtype=abi.JUNCTION, count=n.value).copy()

    def evidence(self):
        """The reads behind this context's clusters (bk_evidence): (rows, call_off) with one abi.EVIDENCE row per member pair and per
        matching split tuple, ordered by call, and call_off[c] .. call_off[c + 1] the rows of STAGE_CLUSTERS row c."""
        data, n, off = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint64)()
        self._check(self.L.bk_evidence(self.h, C.byref(data), C.byref(n), C.byref(off)))
        rows = np.zeros(0, abi.EVIDENCE)
        if n.value:
            buf = (C.c_char * (n.value * abi.EVIDENCE.itemsize)).from_address(data.value)
            rows = np.frombuffer(buf, dtype=abi.EVIDENCE, count=n.value).copy()
        d2, ncl = C.c_void_p(), C.c_uint64()  # call_off has one entry more than STAGE_CLUSTERS has rows
        self._check(self.L.bk_fetch(self.h, abi.STAGE_CLUSTERS, C.byref(d2), C.byref(ncl), None, None))
        return rows, np.ctypeslib.as_array(off, shape=(ncl.value + 1,)).copy()

    def unique_support(self, listing=True):
        """The unique fragments behind this context's clusters (bk_unique_support): one abi.UNIQUE_SUPPORT row per STAGE_CLUSTERS row
        and, with `listing`, first[r] = the smallest row of evidence() that is the same fragment as row r: (rows, first), or rows."""
        data, n, first, n_rows = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint64)(), C.c_uint64()
        if listing:
            self._check(self.L.bk_unique_support(self.h, C.byref(data), C.byref(n), C.byref(first), C.byref(n_rows)))
        else:
            self._check(self.L.bk_unique_support(self.h, C.byref(data), C.byref(n), None, None))
        rows = np.zeros(0, abi.UNIQUE_SUPPORT)
        if n.value:
            buf = (C.c_char * (n.value * abi.UNIQUE_SUPPORT.itemsize)).from_address(data.value)
            rows = np.frombuffer(buf, dtype=abi.UNIQUE_SUPPORT, count=n.value).copy()
        if not listing:
            return rows
        return rows, (np.ctypeslib.as_array(first, shape=(n_rows.value,)).copy() if n_rows.value else np.zeros(0, np.uint64))

    def clip_consensus(self, reads, sites, mapq_min, min_clip, max_len=64, min_depth=2, col_depth=True):
        """The clipped bases of `reads` piled up at `sites` (bk_clip_consensus).  reads: a dict of the bk_reads columns (abi.READS_COLS;
        `key` may be missing), as bam_reads returns it or built by hand; sites: abi.CLIP_SITE rows with tol 0.  Returns (rows, bases,
        depth): one abi.CONSENSUS row per site, bases as uint8 [n_sites, max_len] (0 behind a site's len) and, with `col_depth`, the
        depth of every column as uint32 [n_sites, max_len] (None without)."""
        sites = np.ascontiguousarray(sites, abi.CLIP_SITE)
        assert sites.ndim == 1
        n = len(sites)
        t, keep = reads_struct(reads)
        out, bases, depth = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.L.bk_clip_consensus(self.h, C.byref(t), sites.ctypes.data if n else None, n, int(mapq_min), int(min_clip), int(max_len), int(min_depth),
                                             C.byref(out), C.byref(bases), C.byref(depth) if col_depth else None))
        del keep
        if not n:
            return np.zeros(0, abi.CONSENSUS), np.zeros((0, int(max_len)), np.uint8), (np.zeros((0, int(max_len)), np.uint32) if col_depth else None)
        buf = (C.c_char * (n * abi.CONSENSUS.itemsize)).from_address(out.value)
        rows = np.frombuffer(buf, dtype=abi.CONSENSUS, count=n).copy()
        b = np.ctypeslib.as_array(C.cast(bases, C.POINTER(C.c_uint8)), shape=(n, int(max_len))).copy()
        d = np.ctypeslib.as_array(C.cast(depth, C.POINTER(C.c_uint32)), shape=(n, int(max_len))).copy() if col_depth else None
        return rows, b, d

    def junction_fit(self, ref, probes, query, max_shift=32, max_ins=32, max_hom=32):
        """The queries of `probes` fitted to the reference at the other side of their calls (bk_junction_fit).  ref: a dict of the
        bk_refseq columns (abi.REFSEQ_COLS); probes: abi.JUNCTION_PROBE rows; query: uint8 [n, max_len], ASCII, as clip_consensus
        returns its bases.  Returns one abi.JUNCTION_FIT row per probe."""
        probes = np.ascontiguousarray(probes, abi.JUNCTION_PROBE)
        query = np.ascontiguousarray(query, np.uint8)
        assert probes.ndim == 1 and query.ndim == 2 and query.shape[0] == len(probes)
        n, max_len = len(probes), query.shape[1]
        t, keep = refseq_struct(ref)
        out = C.c_void_p()
        self._check(self.L.bk_junction_fit(self.h, C.byref(t), probes.ctypes.data if n else None, n, query.ctypes.data if n else None, max_len, int(max_shift), int(max_ins),
                                           int(max_hom), C.byref(out)))
        del keep
        if not n:
            return np.zeros(0, abi.JUNCTION_FIT)
        buf = (C.c_char * (n * abi.JUNCTION_FIT.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.JUNCTION_FIT, count=n).copy()

    def locus_similarity(self, ref, pairs, flank=150):
        """The reference windows of `flank` bases either side of the two positions of every pair compared with each other
        (bk_locus_similarity).  ref: a dict of the bk_refseq columns (abi.REFSEQ_COLS), as junction_fit takes it; pairs:
        abi.LOCUS_PAIR rows.  Returns one abi.LOCUS_SIM row per pair."""
        pairs = np.ascontiguousarray(pairs, abi.LOCUS_PAIR)
        assert pairs.ndim == 1
        n = len(pairs)
        t, keep = refseq_struct(ref)
        out = C.c_void_p()
        self._check(self.L.bk_locus_similarity(self.h, C.byref(t), pairs.ctypes.data if n else None, n, int(flank), C.byref(out)))
        del keep
        if not n:
            return np.zeros(0, abi.LOCUS_SIM)
        buf = (C.c_char * (n * abi.LOCUS_SIM.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.LOCUS_SIM, count=n).copy()

    def sequence_match(self, panel, probes, query, seed=12):
        """The queries of `probes` searched in the sequences of `panel`, forward and reverse-complemented (bk_sequence_match).  panel:
        (off, bases), uint64 [n_seqs + 1] from 0 and uint8 ASCII A C G T N, or a list of str / bytes, one per sequence; probes:
        abi.SEQ_PROBE rows; query: uint8 [n, max_len], ASCII, as clip_consensus returns its bases.  Returns one abi.SEQ_HIT row per
        probe."""
        if isinstance(panel, (list, tuple)) and not (len(panel) == 2 and isinstance(panel[0], np.ndarray)):
            seqs = [x.encode() if isinstance(x, str) else bytes(x) for x in panel]
            panel = (np.cumsum([0] + [len(x) for x in seqs]), np.frombuffer(b"".join(seqs), np.uint8))
        off = np.ascontiguousarray(panel[0], np.uint64)
        bases = np.ascontiguousarray(panel[1], np.uint8)
        probes = np.ascontiguousarray(probes, abi.SEQ_PROBE)
        query = np.ascontiguousarray(query, np.uint8)
        assert off.ndim == 1 and len(off) >= 1 and bases.ndim == 1 and probes.ndim == 1 and query.ndim == 2 and query.shape[0] == len(probes)
        n, max_len = len(probes), query.shape[1]
        t = abi.SeqPanel()
        t.n_seqs = len(off) - 1
        t.off = off.ctypes.data
        t.bases = bases.ctypes.data if bases.size else None
        out = C.c_void_p()
        self._check(self.L.bk_sequence_match(self.h, C.byref(t), probes.ctypes.data if n else None, n, query.ctypes.data if n else None, max_len, int(seed), C.byref(out)))
        if not n:
            return np.zeros(0, abi.SEQ_HIT)
        buf = (C.c_char * (n * abi.SEQ_HIT.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.SEQ_HIT, count=n).copy()

    def site_complexity(self, ref, sites, flank=32, max_period=6):
        """The reference window of `flank` bases either side of every site described by itself: soft-mask, trinucleotide counts and
        exact tandem tracts of a period up to `max_period` (bk_site_complexity).  ref: a dict of the bk_refseq columns
        (abi.REFSEQ_COLS), as junction_fit takes it; sites: abi.REF_SITE rows.  Returns one abi.SITE_CPLX row per site."""
        sites = np.ascontiguousarray(sites, abi.REF_SITE)
        assert sites.ndim == 1
        n = len(sites)
        t, keep = refseq_struct(ref)
        out = C.c_void_p()
        self._check(self.L.bk_site_complexity(self.h, C.byref(t), sites.ctypes.data if n else None, n, int(flank), int(max_period), C.byref(out)))
        del keep
        if not n:
            return np.zeros(0, abi.SITE_CPLX)
        buf = (C.c_char * (n * abi.SITE_CPLX.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.SITE_CPLX, count=n).copy()

    def ref_support(self, records, mapq_min, anchor, w):
        """Reference-allele evidence of this context's calls on the record table of `records` (bk_ref_support): one abi.REF_SUPPORT
        row per STAGE_CLUSTERS row.  `records`: this context itself, or a Context on the same device and reference list (the
        matched normal), after isize_stats; `w`: this context's distance."""
        data, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bk_ref_support(self.h, records.h, int(mapq_min), int(anchor), w, C.byref(data), C.byref(n)))
        if not n.value:
            return np.zeros(0, abi.REF_SUPPORT)
        buf = (C.c_char * (n.value * abi.REF_SUPPORT.itemsize)).from_address(data.value)
        return np.frombuffer(buf, dtype=abi.REF_SUPPORT, count=n.value).copy()

    def clip_support(self, records, mapq_min, min_clip, w):
        """Soft-clip evidence of this context's clusters on the record table of `records` (bk_clip_support): one abi.CLIP_SUPPORT
        row per STAGE_CLUSTERS row, voted or not.  `records`: this context itself, or a Context on the same device and reference
        list (the matched normal), after isize_stats; `w`: this context's distance."""
        data, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bk_clip_support(self.h, records.h, int(mapq_min), int(min_clip), w, C.byref(data), C.byref(n)))
        if not n.value:
            return np.zeros(0, abi.CLIP_SUPPORT)
        buf = (C.c_char * (n.value * abi.CLIP_SUPPORT.itemsize)).from_address(data.value)
        return np.frombuffer(buf, dtype=abi.CLIP_SUPPORT, count=n.value).copy()

    def clip_reads(self, sites, mapq_min, min_clip, listing=True):
        """The clip events of this context's records at `sites` (bk_clip_reads; abi.CLIP_SITE rows, or anything np.asarray turns into
        them): (counts, rows, site_off) with one uint32 per site, one abi.CLIP_READ row per event ordered by site and record, and
        site_off[k] .. site_off[k + 1] the rows of site k; with listing=False the counts alone (no listing is made).  After
        isize_stats."""
        sites = np.ascontiguousarray(sites, abi.CLIP_SITE)
        assert sites.ndim == 1
        n = len(sites)
        counts, rows, off = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.L.bk_clip_reads(self.h, sites.ctypes.data if n else None, n, int(mapq_min), int(min_clip), C.byref(counts),
                                         C.byref(rows) if listing else None, C.byref(off) if listing else None))
        cnt = np.ctypeslib.as_array(C.cast(counts, C.POINTER(C.c_uint32)), shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        if not listing:
            return cnt
        site_off = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        out = np.zeros(0, abi.CLIP_READ)
        if site_off[-1]:
            buf = (C.c_char * (int(site_off[-1]) * abi.CLIP_READ.itemsize)).from_address(rows.value)
            out = np.frombuffer(buf, dtype=abi.CLIP_READ, count=int(site_off[-1])).copy()
        return cnt, out, site_off

    def base_depth(self, tid, pos):
        """cal_single_base_depth on this context's records at arbitrary 1-based positions (bk_base_depth): one uint32 per entry."""
        tid = np.ascontiguousarray(tid, np.int32)
        pos = np.ascontiguousarray(pos, np.uint32)
        assert tid.shape == pos.shape and tid.ndim == 1
        data = C.c_void_p()
        self._check(self.L.bk_base_depth(self.h, tid.ctypes.data, pos.ctypes.data, len(tid), C.byref(data)))
        if not len(tid):
            return np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint32)), shape=(len(tid),)).copy()

    def window_coverage(self, windows, mapq_min=0):
        """The aligned bases of this context's eligible records inside arbitrary windows (bk_window_coverage).  windows:
        abi.COV_WINDOW rows, 0-based and half-open.  Returns one abi.WINDOW_COV row per window."""
        windows = np.ascontiguousarray(windows, abi.COV_WINDOW)
        assert windows.ndim == 1
        n = len(windows)
        out = C.c_void_p()
        self._check(self.L.bk_window_coverage(self.h, windows.ctypes.data if n else None, n, int(mapq_min), C.byref(out)))
        if not n:
            return np.zeros(0, abi.WINDOW_COV)
        buf = (C.c_char * (n * abi.WINDOW_COV.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.WINDOW_COV, count=n).copy()

    def window_context(self, windows, mapq_min=0):
        """The record classes and the mapping quality of this context's records that start inside arbitrary windows
        (bk_window_context).  windows: abi.COV_WINDOW rows, 0-based and half-open; mapq_min: the threshold of `lowq`.  Returns one
        abi.WINDOW_CTX row per window."""
        windows = np.ascontiguousarray(windows, abi.COV_WINDOW)
        assert windows.ndim == 1
        n = len(windows)
        out = C.c_void_p()
        self._check(self.L.bk_window_context(self.h, windows.ctypes.data if n else None, n, int(mapq_min), C.byref(out)))
        if not n:
            return np.zeros(0, abi.WINDOW_CTX)
        buf = (C.c_char * (n * abi.WINDOW_CTX.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.WINDOW_CTX, count=n).copy()

    def fusion_frame(self, model, sites):
        """The 5' / 3' partners and the reading frame of every site (bk_fusion_frame).  model: a TxModel, or a dict of the bk_txmodel
        columns (abi.TXMODEL_COLS); sites: abi.FRAME_SITE rows.  Returns one abi.FRAME_CALL row per site."""
        sites = np.ascontiguousarray(sites, abi.FRAME_SITE)
        assert sites.ndim == 1
        n = len(sites)
        t, keep = txmodel_struct(model.cols if isinstance(model, TxModel) else model)
        out = C.c_void_p()
        self._check(self.L.bk_fusion_frame(self.h, C.byref(t), sites.ctypes.data if n else None, n, C.byref(out)))
        del keep
        if not n:
            return np.zeros(0, abi.FRAME_CALL)
        buf = (C.c_char * (n * abi.FRAME_CALL.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.FRAME_CALL, count=n).copy()

    def link_calls(self, sites, max_dist=1000):
        """Reciprocal partners, duplicates and events of a list of calls (bk_link_calls).  sites: abi.LINK_SITE rows; max_dist: the
        distance up to which two breakends are near.  Returns one abi.CALL_LINK row per site."""
        sites = np.ascontiguousarray(sites, abi.LINK_SITE)
        assert sites.ndim == 1
        n = len(sites)
        out = C.c_void_p()
        self._check(self.L.bk_link_calls(self.h, sites.ctypes.data if n else None, n, max_dist, C.byref(out)))
        if not n:
            return np.zeros(0, abi.CALL_LINK)
        buf = (C.c_char * (n * abi.CALL_LINK.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.CALL_LINK, count=n).copy()

    def locus_partners(self, sites, max_gap):
        """Where the discordant pairs inside arbitrary windows point to (bk_locus_partners).  sites: abi.PARTNER_SITE rows; max_gap: the
        distance up to which two neighbouring mates belong to one locus.  Returns one abi.LOCUS_PARTNERS row per site."""
        sites = np.ascontiguousarray(sites, abi.PARTNER_SITE)
        assert sites.ndim == 1
        n = len(sites)
        out = C.c_void_p()
        self._check(self.L.bk_locus_partners(self.h, sites.ctypes.data if n else None, n, max_gap, C.byref(out)))
        if not n:
            return np.zeros(0, abi.LOCUS_PARTNERS)
        buf = (C.c_char * (n * abi.LOCUS_PARTNERS.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.LOCUS_PARTNERS, count=n).copy()

    def fragment_sizes(self, sites, lo, hi):
        """The fragment lengths the member pairs of every call imply across its junction (bk_fragment_sizes).  sites: abi.FRAG_SITE rows,
        one per BK_STAGE_CLUSTERS row; lo, hi: the library's bounds (capi.fragment_bounds).  Returns one abi.FRAG_SIZES row per site."""
        sites = np.ascontiguousarray(sites, abi.FRAG_SITE)
        assert sites.ndim == 1
        n = len(sites)
        out = C.c_void_p()
        self._check(self.L.bk_fragment_sizes(self.h, sites.ctypes.data if n else None, n, lo, hi, C.byref(out)))
        if not n:
            return np.zeros(0, abi.FRAG_SIZES)
        buf = (C.c_char * (n * abi.FRAG_SIZES.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.FRAG_SIZES, count=n).copy()

    def known_calls(self, entries, sites, slop=100):
        """Every call of a list against a panel of pairs of intervals (bk_known_calls).  entries: abi.KNOWN_ENTRY rows; sites:
        abi.KNOWN_SITE rows; slop: the distance up to which a breakend falls into an interval.  Returns one abi.KNOWN_CALL row per site."""
        entries = np.ascontiguousarray(entries, abi.KNOWN_ENTRY)
        sites = np.ascontiguousarray(sites, abi.KNOWN_SITE)
        assert entries.ndim == 1 and sites.ndim == 1
        n = len(sites)
        out = C.c_void_p()
        self._check(self.L.bk_known_calls(self.h, entries.ctypes.data if len(entries) else None, len(entries), sites.ctypes.data if n else None, n, slop, C.byref(out)))
        if not n:
            return np.zeros(0, abi.KNOWN_CALL)
        buf = (C.c_char * (n * abi.KNOWN_CALL.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.KNOWN_CALL, count=n).copy()

    def split_junctions(self, mapq_min=20, tol=2, min_reads=3):
        """Junction calls from the split-evidence tuples alone (bk_split_junctions), after split_evidence().  Returns the
        abi.SPLIT_JUNCTION rows of the calls with at least min_reads distinct reads."""
        out, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bk_split_junctions(self.h, mapq_min, tol, min_reads, C.byref(out), C.byref(n)))
        if not n.value:
            return np.zeros(0, abi.SPLIT_JUNCTION)
        buf = (C.c_char * (n.value * abi.SPLIT_JUNCTION.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.SPLIT_JUNCTION, count=n.value).copy()

    def debug_split_junctions(self, mapq_min, tol, min_reads, clusters):
        """split_junctions() with the claimed row looked up in `clusters` (abi.CLUSTER rows) instead of the context's own table"""
        clusters = np.ascontiguousarray(clusters, abi.CLUSTER)
        out, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bk_debug_split_junctions(self.h, mapq_min, tol, min_reads, clusters.ctypes.data if len(clusters) else None, len(clusters), C.byref(out), C.byref(n)))
        if not n.value:
            return np.zeros(0, abi.SPLIT_JUNCTION)
        buf = (C.c_char * (n.value * abi.SPLIT_JUNCTION.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.SPLIT_JUNCTION, count=n.value).copy()

    def split_junction_counts(self):
        """What the last split_junctions() counted (bk_split_junction_counts): tuples, eligible tuples, exact junctions, calls before
        min_reads, returned calls that a voted row claims, rounds of label propagation."""
        out = (C.c_uint64 * 6)()
        self._check(self.L.bk_split_junction_counts(self.h, out))
        return dict(zip(("tuples", "eligible", "exact", "calls", "claimed", "rounds"), (int(v) for v in out)))

    def cigar_gaps(self, mapq_min=20, min_len=20, anchor=10, tol=2, min_reads=3):
        """Deletions and insertions from the CIGAR gaps of the context's record table (bk_cigar_gaps); no stage need have run.  Returns
        the abi.CIGAR_GAP rows of the calls with at least min_reads distinct reads."""
        out, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bk_cigar_gaps(self.h, mapq_min, min_len, anchor, tol, min_reads, C.byref(out), C.byref(n)))
        if not n.value:
            return np.zeros(0, abi.CIGAR_GAP)
        buf = (C.c_char * (n.value * abi.CIGAR_GAP.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.CIGAR_GAP, count=n.value).copy()

    def cigar_gap_counts(self):
        """What the last cigar_gaps() counted (bk_cigar_gap_counts): records, eligible records, events, events beyond a contig's end,
        exact events, loci, calls before min_reads, returned rows."""
        out = (C.c_uint64 * 8)()
        self._check(self.L.bk_cigar_gap_counts(self.h, out))
        return dict(zip(("records", "eligible", "events", "beyond", "exact", "loci", "calls", "written"), (int(v) for v in out)))

    def clip_loci(self, calls=None, mapq_min=20, min_clip=10, tol=2, pair_dist=50, min_reads=3):
        """Soft-clip pile-ups of the context's record table (bk_clip_loci); no stage need have run.  calls: None, or the Context (this one
        or another) whose voted rows may claim a locus.  Returns the abi.CLIP_LOCUS rows of the loci with at least min_reads distinct
        reads."""
        out, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bk_clip_loci(self.h, calls.h if calls is not None else None, mapq_min, min_clip, tol, pair_dist, min_reads, C.byref(out), C.byref(n)))
        if not n.value:
            return np.zeros(0, abi.CLIP_LOCUS)
        buf = (C.c_char * (n.value * abi.CLIP_LOCUS.itemsize)).from_address(out.value)
        return np.frombuffer(buf, dtype=abi.CLIP_LOCUS, count=n.value).copy()

    def clip_locus_counts(self):
        """What the last clip_loci() counted (bk_clip_locus_counts): records, eligible records, events, events beyond a contig's end,
        exact sites, loci, loci with a mutual partner, returned rows."""
        out = (C.c_uint64 * 8)()
        self._check(self.L.bk_clip_locus_counts(self.h, out))
        return dict(zip(("records", "eligible", "events", "beyond", "exact", "loci", "mutual", "written"), (int(v) for v in out)))

    def run(self, qual=20, fast=True):
        w, n = C.c_double(), C.c_uint64()
        self._check(self.L.bk_run(self.h, qual, int(fast), C.byref(w), C.byref(n)))
        return w.value, n.value

    def fetch(self, stage):
        def fn(h, st, d, c, g, ng):
            return self.L.bk_fetch(h, st, d, c, g, ng)
        try:
            return abi.fetch_array(self.L, self.h, fn, stage)
        except RuntimeError:
            self._check(-1 if not self.L.bk_last_error(self.h) else abi.BK_ERR_ARG)
            raise

    def debug_std_sort(self, key, group_off):
        key = np.ascontiguousarray(key, np.uint32)
        group_off = np.ascontiguousarray(group_off, np.uint64)
        perm = np.zeros(len(key), np.uint32)
        self._check(self.L.bk_debug_std_sort(self.h, key.ctypes.data, group_off.ctypes.data, len(group_off) - 1, perm.ctypes.data))
        return perm

    def debug_scan(self, values, in_place=False):
        """prims::exclusive_scan of a uint32 or uint64 array (bk_debug_scan): n + 1 entries of the same type, the total last."""
        values = np.ascontiguousarray(values)
        assert values.ndim == 1 and values.dtype in (np.uint32, np.uint64), values.dtype
        out = np.zeros(len(values) + 1, values.dtype)
        self._check(self.L.bk_debug_scan(self.h, values.dtype.itemsize, values.ctypes.data if len(values) else None, len(values), int(in_place), out.ctypes.data))
        return out

    def debug_radix_sort(self, keys, vals, begin_bit, end_bit):
        """prims::radix_sort_pairs (bk_debug_radix_sort): (keys, vals) in the stable order of bits [begin_bit, end_bit) of the keys."""
        keys = np.ascontiguousarray(keys, np.uint64)
        vals = np.ascontiguousarray(vals, np.uint32)
        assert keys.ndim == 1 and keys.shape == vals.shape
        n = len(keys)
        ko, vo = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        self._check(self.L.bk_debug_radix_sort(self.h, keys.ctypes.data if n else None, vals.ctypes.data if n else None, n, int(begin_bit), int(end_bit),
                                               ko.ctypes.data if n else None, vo.ctypes.data if n else None))
        return ko, vo

    def sort_forms(self):
        """How this context's std::sort replays ran so far: (service jobs, task dispatches, chains of launches)."""
        out = (C.c_uint64 * 3)()
        self._check(self.L.bk_sort_forms(self.h, out))
        return tuple(int(v) for v in out)

    SORT_INFO = ("FIN_MAX", "HEAP_BIG_MIN", "HEAP_RANKED_MAX", "HEAP_LARGE", "SVC_WIDE_MIN", "F2_HB", "F2_EXT", "HEAP_PAD", "SJ_MAX_WIDE", "SJ_MAX_NARROW",
                 "cap32", "max_heap", "n_heap")

    def debug_sort_info(self):
        """The sizes at which the std::sort replay changes its code path in this build, cap32 of the task dispatch on this device,
        and max_heap / n_heap of this context's last debug_std_sort (bk_debug_sort_info; 0xFFFFFFFF each: a job of the service)."""
        out = (C.c_uint64 * len(self.SORT_INFO))()
        self._check(self.L.bk_debug_sort_info(self.h, out))
        return dict(zip(self.SORT_INFO, (int(v) for v in out)))

    def debug_ahc(self, x, y, w):
        x = np.ascontiguousarray(x, np.uint32)
        y = np.ascontiguousarray(y, np.uint32)
        n = len(x)
        idx = np.zeros(max(n, 1), np.uint32)
        cl = np.zeros(max(n, 1), np.int32)
        m = C.c_uint32()
        self._check(self.L.bk_debug_ahc(self.h, x.ctypes.data, y.ctypes.data, n, float(w), idx.ctypes.data, cl.ctypes.data, C.byref(m)))
        return idx[:m.value].copy(), cl[:m.value].copy()

    def debug_points(self, mode, x, y, w):
        """mode: 'mask' | 'iso' | 'fast' (see include/breakid_hip.h: bk_debug_points)."""
        x = np.ascontiguousarray(x, np.uint32)
        y = np.ascontiguousarray(y, np.uint32)
        n = len(x)
        idx = np.zeros(max(n, 1), np.uint32)
        cl = np.zeros(max(n, 1), np.int32)
        m = C.c_uint32()
        self._check(self.L.bk_debug_points(self.h, {"mask": 0, "iso": 1, "fast": 2}[mode], x.ctypes.data, y.ctypes.data, n, float(w), idx.ctypes.data,
                                           cl.ctypes.data, C.byref(m)))
        return idx[:m.value].copy(), cl[:m.value].copy()

    def debug_points_groups(self, mode, x, y, group_off, w):
        """bk_debug_points for several groups in one list (group_off: n_groups + 1 ascending offsets into x / y): indices into x / y,
        cluster numbers (zeros unless mode is 'fast') and the list's group offsets afterwards."""
        x = np.ascontiguousarray(x, np.uint32)
        y = np.ascontiguousarray(y, np.uint32)
        group_off = np.ascontiguousarray(group_off, np.uint64)
        n = len(x)
        assert len(y) == n and len(group_off) >= 1 and int(group_off[-1]) == n
        idx = np.zeros(2 * n + 1, np.uint32)
        cl = np.zeros(2 * n + 1, np.int32)
        goff = np.zeros(len(group_off), np.uint64)
        m = C.c_uint32()
        self._check(self.L.bk_debug_points_groups(self.h, {"mask": 0, "iso": 1, "fast": 2}[mode], x.ctypes.data, y.ctypes.data, group_off.ctypes.data,
                                                  len(group_off) - 1, float(w), idx.ctypes.data, cl.ctypes.data, goff.ctypes.data, C.byref(m)))
        return idx[:m.value].copy(), cl[:m.value].copy(), goff

    def debug_cigar(self, rows):
        """rows: (kind 't'|'b', c1 text or list of BAM words, c2 text, e) -> int32 array (n, 6)."""
        kind = np.asarray([1 if r[0] == "b" else 0 for r in rows], np.uint8)
        c1 = bytearray()
        o1 = [0]
        for r in rows:
            while r[0] == "b" and len(c1) % 4:
                c1 += b"\0"            # word rows start 4-byte aligned (the padding belongs to no row)
                o1[-1] = len(c1)
            c1 += np.asarray(r[1], np.uint32).tobytes() if r[0] == "b" else r[1].encode()
            o1.append(len(c1))
        c2 = bytearray()
        o2 = [0]
        for r in rows:
            c2 += r[2].encode()
            o2.append(len(c2))
        # rows keep their own start: offsets are (start_i, end_i) pairs flattened as start of i = o[i], end of i = o[i+1] (padding shifted the start)
        o1a, o2a = np.asarray(o1, np.uint32), np.asarray(o2, np.uint32)
        b1 = np.frombuffer(bytes(c1) + b"\0" * 16, np.uint8)
        b2 = np.frombuffer(bytes(c2) + b"\0" * 16, np.uint8)
        e = np.asarray([r[3] for r in rows], np.int32)
        out = np.zeros((len(rows), 6), np.int32)
        self._check(self.L.bk_debug_cigar(self.h, len(rows), kind.ctypes.data, o1a.ctypes.data, b1.ctypes.data, o2a.ctypes.data, b2.ctypes.data, e.ctypes.data,
                                          out.ctypes.data))
        return out

    def debug_vote(self, s1, s2, p1_tid, p2_tid):
        s1 = np.ascontiguousarray(s1, abi.SPLIT)
        s2 = np.ascontiguousarray(s2, abi.SPLIT)
        out = np.zeros(3, np.int32)
        self._check(self.L.bk_debug_vote(self.h, s1.ctypes.data, len(s1), s2.ctypes.data, len(s2), p1_tid, p2_tid, out.ctypes.data))
        return tuple(int(v) for v in out)

    def debug_region(self, tid, start, end, depth_pos, cap=4096):
        out = np.zeros(cap, abi.SPLIT)
        n, cov, depth = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self.L.bk_debug_region(self.h, tid, start, end, depth_pos, out.ctypes.data, cap, C.byref(n), C.byref(cov), C.byref(depth)))
        return out[:min(n.value, cap)].copy(), n.value, cov.value, depth.value

    def timing_enable(self, on=True):
        self._check(self.L.bk_timing_enable(self.h, int(on)))

    def timing(self):
        names = C.POINTER(C.c_char_p)()
        ms = C.POINTER(C.c_float)()
        by = C.POINTER(C.c_uint64)()
        n = C.c_int()
        self._check(self.L.bk_timing(self.h, C.byref(names), C.byref(ms), C.byref(by), C.byref(n)))
        return [(names[i].decode(), float(ms[i]), int(by[i])) for i in range(n.value)]

    def timing_touched(self):
        """bytes the kernels of each timed stage load + store themselves (call after timing(); same order)"""
        t = C.POINTER(C.c_uint64)()
        n = C.c_int()
        self._check(self.L.bk_timing_touched(self.h, C.byref(t), C.byref(n)))
        return [int(t[i]) for i in range(n.value)]


class DeviceBamTable:
    """Record table decoded on the GPU (bk_bam_decode_device): device-resident columns owned by the library."""

    def __init__(self, L, h, soa, contigs):
        self.L, self.h, self.soa, self.contigs = L, h, soa, contigs

    def close(self):
        if self.h:
            self.L.bk_bam_dev_free(self.h)
            self.h = None


def decode_bam_device(path, device=0):
    """GPU BGZF inflate + BAM decode -> DeviceBamTable; raises BreakIDError(BK_ERR_IO) for files that are not block aligned."""
    L = lib()
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    s = abi.Soa()
    nt = C.c_int()
    names = C.POINTER(C.c_char_p)()
    lens = C.POINTER(C.c_uint32)()
    rc = L.bk_bam_decode_device(path.encode(), device, C.byref(h), C.byref(s), C.byref(nt), C.byref(names), C.byref(lens), err, 512)
    if rc != 0:
        raise BreakIDError(rc, err.value.decode())
    contigs = [(names[i].decode(), int(lens[i])) for i in range(nt.value)]
    return DeviceBamTable(L, h, s, contigs)


def decode_bam_device_part(path, part, parts, device=0):
    """The records of part `part` of `parts` of a block-aligned BAM (bk_bam_decode_device_part): one rank's record range of a
    sharded run, decoded on its own GPU."""
    L = lib()
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    s = abi.Soa()
    nt = C.c_int()
    names = C.POINTER(C.c_char_p)()
    lens = C.POINTER(C.c_uint32)()
    rc = L.bk_bam_decode_device_part(path.encode(), device, part, parts, C.byref(h), C.byref(s), C.byref(nt), C.byref(names), C.byref(lens), err, 512)
    if rc != 0:
        raise BreakIDError(rc, err.value.decode())
    contigs = [(names[i].decode(), int(lens[i])) for i in range(nt.value)]
    return DeviceBamTable(L, h, s, contigs)


def decode_bam_device_ctx(path, qual=20, device=0):
    """File -> device table with the stream pass of the hot path overlapped with the feed (bk_bam_decode_device_ctx):
    returns (Context with the table attached and the stream pass done, DeviceBamTable owning the columns)."""
    L = lib()
    hb, hc = C.c_void_p(), C.c_void_p()
    err = C.create_string_buffer(512)
    nt = C.c_int()
    names = C.POINTER(C.c_char_p)()
    lens = C.POINTER(C.c_uint32)()
    rc = L.bk_bam_decode_device_ctx(path.encode(), device, qual, C.byref(hb), C.byref(hc), C.byref(nt), C.byref(names), C.byref(lens), err, 512)
    if rc != 0:
        raise BreakIDError(rc, err.value.decode())
    contigs = [(names[i].decode(), int(lens[i])) for i in range(nt.value)]
    ctx = Context.__new__(Context)
    ctx.L, ctx.contigs, ctx.h = L, contigs, hc
    table = DeviceBamTable(L, hb, None, contigs)
    ctx._keep = table
    s = abi.Soa()
    ctx._check(L.bk_records(hc, C.byref(s)))  # the columns the table owns, as the context holds them
    table.soa = s
    return ctx, table


def bam_extract(in_bam, out_bam, keys, tags):
    """Read names back from their hashes, and the reads themselves (bk_bam_extract; host code, no GPU).  keys: abi.READ_KEY array
    (qcheck 0 = compare qhash alone; tag indexes `tags`); out_bam: path or None (names only).  Returns (names, n_written): one
    name per key, "" for a key no record matched."""
    keys = np.ascontiguousarray(keys, abi.READ_KEY)
    tag_arr = (C.c_char_p * max(len(tags), 1))(*[t.encode() for t in tags])
    names, n = C.c_void_p(), C.c_uint64()
    err = C.create_string_buffer(512)
    L = lib()
    rc = L.bk_bam_extract(os.fsencode(in_bam), None if out_bam is None else os.fsencode(out_bam), keys.ctypes.data if len(keys) else None, len(keys),
                          tag_arr if len(tags) else None, len(tags), C.byref(names), C.byref(n), err, 512)
    if rc != 0:
        raise BreakIDError(rc, err.value.decode())
    try:
        out, p = [], names.value
        for _ in range(len(keys)):
            t = C.string_at(p)
            out.append(t.decode())
            p += len(t) + 1
    finally:
        L.bk_bam_names_free(names)
    return out, n.value


def reads_struct(reads):
    """A dict of bk_reads columns as (abi.Reads, the arrays that back it).  n is len(reads["tid"])."""
    t, keep = abi.Reads(), []
    t.n = len(reads["tid"])
    for name, dt in abi.READS_COLS:
        if name not in reads:
            continue
        a = np.ascontiguousarray(reads[name], dt)
        keep.append(a)
        setattr(t, name, a.ctypes.data if a.size else None)
    return t, keep


def refseq_struct(ref):
    """A dict of bk_refseq columns as (abi.RefSeq, the arrays that back it).  n_segs is len(ref["tid"])."""
    t, keep = abi.RefSeq(), []
    t.n_segs = len(ref["tid"])
    for name, dt in abi.REFSEQ_COLS:
        a = np.ascontiguousarray(ref[name], dt)
        keep.append(a)
        setattr(t, name, a.ctypes.data if a.size else None)
    return t, keep


def txmodel_struct(cols):
    """A dict of bk_txmodel columns as (abi.TxModel, the arrays that back it).  n_tx is len(cols["tid"]), n_parts len(cols["ex_start"])."""
    t, keep = abi.TxModel(), []
    t.n_tx, t.n_parts = len(cols["tid"]), len(cols["ex_start"])
    for name, dt in abi.TXMODEL_COLS:
        a = np.ascontiguousarray(cols[name], dt)
        keep.append(a)
        setattr(t, name, a.ctypes.data if a.size else None)
    return t, keep


class TxModel:
    """A transcript model for Context.fusion_frame, built from (tid, tx_start, tx_end, strand, parts, name, gene) rows: strand is
    "+" / "-" or 0 / 1, parts a list of (start, end) coding parts, 0-based and half-open.  The rows are sorted by (tid, tx_start),
    stably, as bk_txmodel asks; `names` and `genes` follow the sorted order, so that FRAME_CALL["tx"] indexes them."""

    def __init__(self, rows):
        rows = sorted(rows, key=lambda r: (r[0], r[1]))
        self.names = [r[5] if len(r) > 5 else "" for r in rows]
        self.genes = [r[6] if len(r) > 6 else "" for r in rows]
        off, starts, ends = [0], [], []
        for r in rows:
            starts += [p[0] for p in r[4]]
            ends += [p[1] for p in r[4]]
            off.append(len(starts))
        self.cols = {"tid": np.asarray([r[0] for r in rows], np.int32), "tx_start": np.asarray([r[1] for r in rows], np.uint32),
                     "tx_end": np.asarray([r[2] for r in rows], np.uint32),
                     "strand": np.asarray([{"+": 0, "-": 1}.get(r[3], r[3]) for r in rows], np.uint8),
                     "ex_off": np.asarray(off if rows else [], np.uint32), "ex_start": np.asarray(starts, np.uint32), "ex_end": np.asarray(ends, np.uint32)}

    def __len__(self):
        return len(self.names)

    @classmethod
    def from_refgene(cls, lines, contig_names):
        """The model the command line builds from refGene rows: NR_ rows skipped, the coding parts CDS n exons, transcripts on
        contigs that `contig_names` lacks dropped.  Returns (model, dropped)."""
        tid_of = {n: i for i, n in enumerate(contig_names)}
        rows, dropped = [], 0
        for line in lines:
            f = line.rstrip("\n").split("\t")
            if "NR_" in f[1]:
                continue
            if f[2] not in tid_of:
                dropped += 1
                continue
            cs, ce, ne = int(f[6]), int(f[7]), int(f[8])
            xs = [int(v) for v in f[9].split(",") if v][:ne]
            xe = [int(v) for v in f[10].split(",") if v][:ne]
            parts = [(max(s, cs), min(e, ce)) for s, e in zip(xs, xe) if cs != ce and s < ce and e > cs]
            rows.append((tid_of[f[2]], int(f[4]), int(f[5]), f[3], parts, f[1], f[12]))
        return cls(rows), dropped


def bam_reads(path, keys):
    """The alignments of named reads with their bases (bk_bam_reads; host code, no GPU).  keys: abi.READ_KEY array (tag is not
    read).  Returns a dict of numpy copies of the bk_reads columns (abi.READS_COLS), rows in file order."""
    keys = np.ascontiguousarray(keys, abi.READ_KEY)
    L = lib()
    t = abi.Reads()
    err = C.create_string_buffer(512)
    rc = L.bk_bam_reads(os.fsencode(path), keys.ctypes.data if len(keys) else None, len(keys), C.byref(t), err, 512)
    if rc != 0:
        raise BreakIDError(rc, err.value.decode())
    try:
        n = t.n
        cols = {}

        def col(name, dt, cnt):
            ptr = getattr(t, name)
            if cnt == 0 or not ptr:
                return np.zeros(0, dt)
            buf = (C.c_char * (cnt * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt, count=cnt).copy()
        for name, dt in abi.READS_COLS:
            if name in ("cigar", "seq"):
                continue
            cols[name] = col(name, dt, n + 1 if name in ("cigar_off", "seq_off") else n)
        cols["cigar"] = col("cigar", np.uint32, int(cols["cigar_off"][-1]))
        cols["seq"] = col("seq", np.uint8, int(cols["seq_off"][-1]))
        return cols
    finally:
        L.bk_reads_free(C.byref(t))


class BamTable:
    """Decoded record table still owned by the C++ reader (pinned host columns); close() releases it."""

    def __init__(self, L, h, soa):
        self.L, self.h, self.soa = L, h, soa
        n = soa.n
        self.nbytes = n * (4 * 5 + 2 + 1 + 8) + (n + 1) * 8 + soa.n_cigar_words * 4 + soa.n_aux_bytes

    def close(self):
        if self.h:
            self.L.bk_bam_close(self.h)
            self.h = None


def decode_bam(path, keep=False):
    """C++ BGZF/BAM decoder -> (contigs, SoA dict of numpy copies); keep=True also returns the live BamTable."""
    L = lib()
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = L.bk_bam_open(path.encode(), C.byref(h), err, 512)
    if rc != 0:
        raise BreakIDError(rc, err.value.decode())
    try:
        nt = C.c_int()
        names = C.POINTER(C.c_char_p)()
        lens = C.POINTER(C.c_uint32)()
        L.bk_bam_header(h, C.byref(nt), C.byref(names), C.byref(lens))
        contigs = [(names[i].decode(), int(lens[i])) for i in range(nt.value)]
        s = abi.Soa()
        rc = L.bk_bam_decode(h, C.byref(s), err, 512)
        if rc != 0:
            raise BreakIDError(rc, err.value.decode())
        n = s.n
        sizes = {"cigar_off": n + 1, "aux_off": n + 1, "cigar": max(1, s.n_cigar_words), "aux": max(1, s.n_aux_bytes)}
        cols = {}
        for name, dt in abi.SOA_COLS_ALL:
            cnt = sizes.get(name, n)
            ptr = getattr(s, name)
            if cnt == 0 or not ptr:
                cols[name] = np.zeros(0, dt)
                continue
            buf = (C.c_char * (cnt * np.dtype(dt).itemsize)).from_address(ptr)
            cols[name] = np.frombuffer(buf, dtype=dt, count=cnt).copy()
        cols["cigar"] = cols["cigar"][: s.n_cigar_words]
        cols["aux"] = cols["aux"][: s.n_aux_bytes]
        if keep:
            t = BamTable(L, h, s)
            h = None
            return contigs, cols, t
        return contigs, cols
    finally:
        if h:
            L.bk_bam_close(h)
