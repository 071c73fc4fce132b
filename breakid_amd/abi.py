"""numpy / ctypes mirror of include/breakid_hip.h (POD layouts and stage ids)."""
import ctypes as C

import numpy as np

BK_OK = 0
BK_ERR_ARG, BK_ERR_HIP, BK_ERR_NO_DEVICE, BK_ERR_UNSORTED, BK_ERR_CIGAR, BK_ERR_IO, BK_ERR_LIMIT, BK_ERR_COLLISION = -1, -2, -3, -4, -5, -6, -7, -8
BK_MEM_HOST, BK_MEM_DEVICE = 0, 1
STAGE_SCAN, STAGE_ISO, STAGE_CLUSTERED, STAGE_SPLITS, STAGE_CLUSTERS, STAGE_GROUP_KEYS = range(6)

PAIR = np.dtype([("x", "<u4"), ("y", "<u4"), ("p1_pos", "<u4"), ("p2_pos", "<u4"), ("p1_tid", "<i4"),
                 ("p2_tid", "<i4"), ("p1_flag", "<u2"), ("p2_flag", "<u2"), ("p1_mapq", "u1"), ("p2_mapq", "u1"),
                 ("p1_rev", "u1"), ("p2_rev", "u1"), ("rec", "<u8"), ("id", "<u4"), ("cluster", "<i4"),
                 ("group", "<u4"), ("reserved", "<u4")])
SPLIT = np.dtype([("rec", "<u8"), ("tid", "<i4"), ("pos", "<i4"), ("endpos", "<i4"), ("reserved", "<u4"), ("qhash", "<u8"),
                  ("prim_chr", "<i4"), ("sec_chr", "<i4"), ("prim_start", "<u4"), ("prim_end", "<u4"),
                  ("prim_bp", "<u4"), ("sec_start", "<u4"), ("sec_end", "<u4"), ("sec_bp", "<u4"),
                  ("prim_cigar", "<u8"), ("sec_cigar", "<u8"), ("flags", "<u4"), ("qcheck", "<u4")])
CLUSTER = np.dtype([("group", "<u4"), ("id", "<i4"), ("p1_tid", "<i4"), ("p2_tid", "<i4"), ("p1_mean", "<u4"),
                    ("p2_mean", "<u4"), ("p1_min", "<u4"), ("p1_max", "<u4"), ("p2_min", "<u4"), ("p2_max", "<u4"),
                    ("p1_exact", "<u4"), ("p2_exact", "<i4"), ("n_drp", "<u4"), ("n_sr", "<u4"), ("depth1", "<u4"),
                    ("depth2", "<u4"), ("type_mask", "<u4"), ("flags", "<u4")])
GROUP_KEY = np.dtype([("p1_tid", "<i4"), ("p2_tid", "<i4")])
NORMAL_SUPPORT = np.dtype([("n_drp", "<u4"), ("n_sr", "<u4"), ("depth1", "<u4"), ("depth2", "<u4")])  # struct bk_normal_support
REF_SUPPORT = np.dtype([("ref_pairs1", "<u4"), ("ref_pairs2", "<u4"), ("ref_reads1", "<u4"), ("ref_reads2", "<u4")])  # struct bk_ref_support
JUNCTION = np.dtype([("pairs", "<u4", (4,)), ("splits", "<u4", (4,)), ("mapq_sum1", "<u8"), ("mapq_sum2", "<u8")])  # struct bk_junction
assert JUNCTION.itemsize == 48
CLIP_LEFT, CLIP_RIGHT = 0, 1
CLIP_SUPPORT = np.dtype([("at", "<u4", (2, 2)), ("peak_pos", "<u4", (2, 2)), ("peak_n", "<u4", (2, 2)), ("events", "<u4", (2, 2))])  # struct bk_clip_support, [side][dir]
assert CLIP_SUPPORT.itemsize == 64
CLIP_SITE = np.dtype([("tid", "<i4"), ("pos", "<u4"), ("tol", "<u4"), ("dir", "<u4")])  # struct bk_clip_site; pos 1-based, dir CLIP_LEFT / CLIP_RIGHT
CLIP_READ = np.dtype([("rec", "<u8"), ("qhash", "<u8"), ("qcheck", "<u4"), ("site", "<u4"), ("tid", "<i4"), ("p", "<u4"), ("clip_len", "<u4"), ("flag", "<u2"),
                      ("mapq", "u1"), ("dir", "u1")])  # struct bk_clip_read
assert CLIP_SITE.itemsize == 16 and CLIP_READ.itemsize == 40
EV_PAIR, EV_SPLIT = 1, 2
EVIDENCE = np.dtype([("rec", "<u8"), ("qhash", "<u8"), ("qcheck", "<u4"), ("call", "<u4"), ("tid1", "<i4"), ("pos1", "<u4"), ("tid2", "<i4"),
                     ("pos2", "<u4"), ("flag1", "<u2"), ("flag2", "<u2"), ("mapq1", "u1"), ("mapq2", "u1"), ("kind", "u1"), ("sides", "u1")])  # struct bk_evidence
UNIQUE_SUPPORT = np.dtype([("uniq_pairs", "<u4"), ("top_pairs", "<u4"), ("uniq_splits", "<u4"), ("top_splits", "<u4")])  # struct bk_unique_support
assert UNIQUE_SUPPORT.itemsize == 16
CONSENSUS = np.dtype([("n_reads", "<u4"), ("len", "<u4"), ("match", "<u4"), ("total", "<u4")])  # struct bk_consensus
assert CONSENSUS.itemsize == 16
# the columns of a bk_reads table, in the struct's order (cigar_off and seq_off have n + 1 entries)
READS_COLS = [("tid", np.int32), ("pos", np.int32), ("flag", np.uint16), ("mapq", np.uint8), ("key", np.uint32), ("cigar_off", np.uint32), ("cigar", np.uint32),
              ("l_seq", np.uint32), ("seq_off", np.uint64), ("seq", np.uint8)]
JUNCTION_PROBE = np.dtype([("tid_own", "<i4"), ("pos_own", "<u4"), ("dir_own", "<u4"), ("tid_mate", "<i4"), ("pos_mate", "<u4"), ("dir_mate", "<u4"), ("qlen", "<u4"),
                           ("reserved", "<u4")])  # struct bk_junction_probe
JUNCTION_FIT = np.dtype([("shift", "<i4"), ("ins", "<u4"), ("aligned", "<u4"), ("mism", "<u4"), ("hom_fwd", "<u4"), ("hom_back", "<u4"), ("score", "<i4"),
                         ("placed", "<u4")])  # struct bk_junction_fit
assert JUNCTION_PROBE.itemsize == 32 and JUNCTION_FIT.itemsize == 32
LOCUS_PAIR = np.dtype([("tid_a", "<i4"), ("pos_a", "<u4"), ("tid_b", "<i4"), ("pos_b", "<u4")])  # struct bk_locus_pair; pos 1-based
LOCUS_SIM = np.dtype([("score", "<u4"), ("len", "<u4"), ("mism", "<u4"), ("run", "<u4"), ("diag", "<i4"), ("start", "<u4"), ("orient", "<u4"),
                      ("found", "<u4")])  # struct bk_locus_sim
assert LOCUS_PAIR.itemsize == 16 and LOCUS_SIM.itemsize == 32
SEQ_PROBE = np.dtype([("qlen", "<u4"), ("reversed", "<u4")])  # struct bk_seq_probe
SEQ_HIT = np.dtype([("found", "<u4"), ("seq", "<i4"), ("orient", "<u4"), ("score", "<u4"), ("len", "<u4"), ("mism", "<u4"), ("run", "<u4"), ("q_start", "<u4"),
                    ("s_start", "<u4"), ("n_seeds", "<u4"), ("seq2", "<i4"), ("score2", "<u4")])  # struct bk_seq_hit; s_start 0-based
assert SEQ_PROBE.itemsize == 8 and SEQ_HIT.itemsize == 48
REF_SITE = np.dtype([("tid", "<i4"), ("pos", "<u4")])  # struct bk_ref_site; pos 1-based
SITE_CPLX = np.dtype([("covered", "<u4"), ("valid", "<u4"), ("gc", "<u4"), ("masked", "<u4"), ("mask_run", "<u4"), ("tri_total", "<u4"), ("tri_pairs", "<u4"),
                      ("tri_distinct", "<u4"), ("bp_period", "<u4"), ("bp_len", "<u4"), ("bp_start", "<u4"), ("max_period", "<u4"), ("max_len", "<u4"),
                      ("max_start", "<u4"), ("reserved", "<u4", (2,))])  # struct bk_site_cplx
assert REF_SITE.itemsize == 8 and SITE_CPLX.itemsize == 64
COV_WINDOW = np.dtype([("tid", "<i4"), ("beg", "<u4"), ("end", "<u4"), ("reserved", "<u4")])  # struct bk_cov_window; 0-based, half-open
WINDOW_COV = np.dtype([("bases", "<u8"), ("reads", "<u4"), ("reserved", "<u4")])  # struct bk_window_cov
WINDOW_CTX = np.dtype([("mapq_sum", "<u8"), ("reads", "<u4"), ("mq0", "<u4"), ("lowq", "<u4"), ("clipped", "<u4"), ("improper", "<u4"), ("orphan", "<u4"), ("dup", "<u4"),
                       ("secsup", "<u4")])  # struct bk_window_ctx; records by start, not by overlap
assert WINDOW_CTX.itemsize == 40
assert COV_WINDOW.itemsize == 16 and WINDOW_COV.itemsize == 16
FRAME_SITE = np.dtype([("tid1", "<i4"), ("pos1", "<u4"), ("tid2", "<i4"), ("pos2", "<u4"), ("right1", "u1"), ("right2", "u1"), ("reserved", "u1", (6,))])  # struct bk_frame_site; pos 1-based
FRAME_CALL = np.dtype([("cls", "u1"), ("order", "u1"), ("loc", "u1", (2,)), ("role", "u1", (2,)), ("exon", "<u2", (2,)), ("reserved", "<u2"), ("tx", "<i4", (2,)),
                       ("cod", "<u4", (2,)), ("n_tx", "<u4", (2,)), ("n_inframe", "<u4"), ("n_compatible", "<u4"), ("reserved2", "<u4")])  # struct bk_frame_call
assert FRAME_SITE.itemsize == 24 and FRAME_CALL.itemsize == 48
FRAME_CLASSES = ["none", "antisense", "truncating", "promoter", "outframe", "inframe"]  # BK_FRAME_*
FRAME_HEAD, FRAME_TAIL = 1, 2
FRAME_CHUNK = 128  # csrc/frame.h: the overlapping transcripts of one side that the kernel stages at a time
FRAME_LOCS = [".", "noncoding", "5UTR", "CDS", "intron", "3UTR"]  # BK_LOC_*
LINK_SITE = np.dtype([("tid1", "<i4"), ("pos1", "<u4"), ("tid2", "<i4"), ("pos2", "<u4"), ("right1", "u1"), ("right2", "u1"), ("reserved", "u1", (6,))])  # struct bk_link_site; pos 1-based
CALL_LINK = np.dtype([("n_dup", "<u4"), ("n_recip", "<u4"), ("n_adj", "<u4"), ("dup_of", "<i4"), ("mate", "<i4"), ("off", "<i4", (2,)), ("event", "<u4"), ("event_size", "<u4"),
                      ("mate_crossed", "u1"), ("reserved", "u1", (3,))])  # struct bk_call_link
assert LINK_SITE.itemsize == 24 and CALL_LINK.itemsize == 40
LINK_RELATIONS = ["none", "duplicate", "reciprocal", "adjacent"]  # BK_LINK_*
LINK_MAX_DIST = 1000000  # BK_LINK_MAX_DIST
PARTNER_SITE = np.dtype([("tid", "<i4"), ("beg", "<u4"), ("end", "<u4"), ("mtid", "<i4"), ("mbeg", "<u4"), ("mend", "<u4"), ("reserved", "<u4", (2,))])  # struct bk_partner_site; 1-based, inclusive
LOCUS_PARTNERS = np.dtype([("ends", "<u4"), ("to_partner", "<u4"), ("loci", "<u4"), ("top_n", "<u4"), ("top_tid", "<i4"), ("top_beg", "<u4"), ("top_end", "<u4"), ("reserved", "<u4")])  # struct bk_locus_partners
assert PARTNER_SITE.itemsize == 32 and LOCUS_PARTNERS.itemsize == 32
FRAG_SITE = np.dtype([("pos1", "<u4"), ("pos2", "<u4"), ("right1", "u1"), ("right2", "u1"), ("skip", "u1"), ("reserved", "u1", (5,))])  # struct bk_frag_site; pos 1-based
FRAG_SIZES = np.dtype([("n_used", "<u4"), ("n_off", "<u4"), ("n_lost", "<u4"), ("n_short", "<u4"), ("n_long", "<u4"), ("min", "<i4"), ("max", "<i4"), ("reserved", "<u4"), ("sum", "<i8"), ("abs_dev", "<u8")])  # struct bk_frag_sizes
assert FRAG_SITE.itemsize == 16 and FRAG_SIZES.itemsize == 48
KNOWN_ENTRY = np.dtype([("tid1", "<i4"), ("beg1", "<u4"), ("end1", "<u4"), ("tid2", "<i4"), ("beg2", "<u4"), ("end2", "<u4"), ("name", "<u4"), ("score", "<i4"),
                        ("strand1", "u1"), ("strand2", "u1"), ("reserved", "u1", (6,))])  # struct bk_known_entry; [beg, end) 0-based
KNOWN_SITE = np.dtype([("tid1", "<i4"), ("pos1", "<u4"), ("tid2", "<i4"), ("pos2", "<u4"), ("right1", "u1"), ("right2", "u1"), ("reserved", "u1", (6,))])  # struct bk_known_site; pos 1-based
KNOWN_CALL = np.dtype([("n_hits", "<u4"), ("n_oriented", "<u4"), ("n_opposed", "<u4"), ("n_names", "<u4"), ("n_side", "<u4", (2,)), ("best", "<i4"), ("best_score", "<i4"),
                       ("best_dist", "<u4"), ("best_crossed", "u1"), ("best_oriented", "u1"), ("reserved", "u1", (2,))])  # struct bk_known_call
assert KNOWN_ENTRY.itemsize == 40 and KNOWN_SITE.itemsize == 24 and KNOWN_CALL.itemsize == 40
KNOWN_MAX_SLOP = 1000000  # BK_KNOWN_MAX_SLOP
KNOWN_NO_SCORE = -2147483648  # BK_KNOWN_NO_SCORE
SPLIT_JUNCTION = np.dtype([("tid1", "<i4"), ("pos1", "<u4"), ("tid2", "<i4"), ("pos2", "<u4"), ("n_reads", "<u4"), ("n_tuples", "<u4"), ("n_exact", "<u4"), ("lo1", "<u4"), ("hi1", "<u4"),
                           ("lo2", "<u4"), ("hi2", "<u4"), ("n_own", "<u4", (2,)), ("mapq_sum", "<u4", (2,)), ("call", "<i4"), ("right1", "u1"), ("right2", "u1"), ("call_crossed", "u1"),
                           ("reserved", "u1"), ("top_reads", "<u4")])  # struct bk_split_junction; pos 1-based
assert SPLIT_JUNCTION.itemsize == 72
SJ_MAX_TOL = 100  # BK_SJ_MAX_TOL
CIGAR_GAP = np.dtype([("tid", "<i4"), ("start", "<u4"), ("len", "<u4"), ("kind", "<u4"), ("n_reads", "<u4"), ("n_rows", "<u4"), ("n_exact", "<u4"), ("top_reads", "<u4"),
                      ("lo_start", "<u4"), ("hi_start", "<u4"), ("lo_len", "<u4"), ("hi_len", "<u4"), ("n_fwd", "<u4"), ("n_rev", "<u4"), ("mapq_sum", "<u8")])  # struct bk_cigar_gap; start 1-based
assert CIGAR_GAP.itemsize == 64
GAP_DEL, GAP_INS = 0, 1  # BK_GAP_DEL, BK_GAP_INS
GAP_MAX_TOL = 100  # BK_GAP_MAX_TOL
GAP_MAX_LEN = 1000000  # BK_GAP_MAX_LEN
CLIP_LOCUS = np.dtype([("tid", "<i4"), ("pos", "<u4"), ("dir", "<u4"), ("flags", "<u4"), ("n_reads", "<u4"), ("n_rows", "<u4"), ("n_exact", "<u4"), ("top_reads", "<u4"),
                       ("lo_pos", "<u4"), ("hi_pos", "<u4"), ("n_fwd", "<u4"), ("n_rev", "<u4"), ("max_clip", "<u4"), ("n_orphan", "<u4"), ("clip_sum", "<u8"), ("mapq_sum", "<u8"),
                       ("n_improper", "<u4"), ("claim", "<u4"), ("mate", "<u4"), ("mate_pos", "<u4"), ("mate_reads", "<u4"), ("mate_off", "<i4")])  # struct bk_clip_locus; pos 1-based
assert CLIP_LOCUS.itemsize == 96
CLIPLOCI_MAX_TOL = 100  # BK_CLIPLOCI_MAX_TOL
CLIPLOCI_MAX_PAIR = 100000  # BK_CLIPLOCI_MAX_PAIR
STRAND_NONE, STRAND_LEFT, STRAND_RIGHT = 0, 1, 2  # BK_STRAND_*
BGZF_FORM_ROUNDS, BGZF_FORM_SHARED = 1, 2  # BK_BGZF_FORM_*: the form bits of bk_debug_bgzf_inflate_form
# the words of bk_debug_bgzf_info, in its order
BGZF_INFO = ("LIT_FAST", "DIST_FAST", "LANE_PART_BITS", "LANE_CHECK_BITS", "LANE_FULL_WALKS", "CHUNK_DW", "RES_WIN", "RESOLVE_THREADS", "BGZF_BATCH_BLOCKS",
             "BGZF_TOKENS_PER_BLOCK", "BGZF_MAX_DEFLATE_BLOCKS")
# the columns of a bk_txmodel, in the struct's order (ex_off has n_tx + 1 entries, ex_start / ex_end n_parts)
TXMODEL_COLS = [("tid", np.int32), ("tx_start", np.uint32), ("tx_end", np.uint32), ("strand", np.uint8), ("ex_off", np.uint32), ("ex_start", np.uint32), ("ex_end", np.uint32)]
# the columns of a bk_refseq table, in the struct's order (off has n_segs + 1 entries)
REFSEQ_COLS = [("tid", np.int32), ("start", np.uint32), ("len", np.uint32), ("off", np.uint64), ("bases", np.uint8)]
READ_KEY = np.dtype([("qhash", "<u8"), ("qcheck", "<u4"), ("tag", "<u4")])  # bk_read_key
assert EVIDENCE.itemsize == 48 and READ_KEY.itemsize == 16
assert PAIR.itemsize == 56 and SPLIT.itemsize == 88 and CLUSTER.itemsize == 72 and NORMAL_SUPPORT.itemsize == 16 and REF_SUPPORT.itemsize == 16

STAGE_DTYPE = {STAGE_SCAN: PAIR, STAGE_ISO: PAIR, STAGE_CLUSTERED: PAIR, STAGE_SPLITS: SPLIT,
               STAGE_CLUSTERS: CLUSTER, STAGE_GROUP_KEYS: GROUP_KEY}


class Reads(C.Structure):  # bk_reads
    _fields_ = [("n", C.c_uint64)] + [(name, C.c_void_p) for name, _ in READS_COLS] + [("owner", C.c_void_p)]


class RefSeq(C.Structure):  # bk_refseq
    _fields_ = [("n_segs", C.c_uint64)] + [(name, C.c_void_p) for name, _ in REFSEQ_COLS]


class SeqPanel(C.Structure):  # bk_seq_panel
    _fields_ = [("n_seqs", C.c_uint64), ("off", C.c_void_p), ("bases", C.c_void_p)]


class TxModel(C.Structure):  # bk_txmodel
    _fields_ = [("n_tx", C.c_uint64), ("n_parts", C.c_uint64)] + [(name, C.c_void_p) for name, _ in TXMODEL_COLS]


class Soa(C.Structure):
    _fields_ = [("n", C.c_uint64), ("tid", C.c_void_p), ("pos", C.c_void_p), ("mtid", C.c_void_p),
                ("mpos", C.c_void_p), ("isize", C.c_void_p), ("flag", C.c_void_p), ("mapq", C.c_void_p),
                ("qhash", C.c_void_p), ("cigar_off", C.c_void_p), ("cigar", C.c_void_p),
                ("aux_off", C.c_void_p), ("aux", C.c_void_p), ("n_cigar_words", C.c_uint64),
                ("n_aux_bytes", C.c_uint64), ("qcheck", C.c_void_p), ("side", C.c_void_p)]


class Regions(C.Structure):
    """bk_regions: the exclude list of bk_exclude_regions (host arrays, [beg, end) 0-based)"""
    _fields_ = [("tid", C.c_void_p), ("beg", C.c_void_p), ("end", C.c_void_p), ("n", C.c_uint64)]


SOA_COLS = [("tid", np.int32), ("pos", np.int32), ("mtid", np.int32), ("mpos", np.int32), ("isize", np.int32),
            ("flag", np.uint16), ("mapq", np.uint8), ("qhash", np.uint64), ("cigar_off", np.uint32),
            ("cigar", np.uint32), ("aux_off", np.uint32), ("aux", np.uint8)]


SOA_COLS_ALL = SOA_COLS + [("qcheck", np.uint32)]  # with the optional second read-name hash (the BAM decoders fill it)


def soa_from_numpy(cols) -> Soa:
    """cols: dict of contiguous numpy arrays (host).  The dict must outlive the returned struct."""
    s = Soa()
    s.n = len(cols["tid"])
    for name, dt in SOA_COLS:
        a = cols[name]
        assert a.dtype == dt and a.flags["C_CONTIGUOUS"], name
        setattr(s, name, a.ctypes.data if a.size else 0)
    assert len(cols["cigar_off"]) == s.n + 1 and len(cols["aux_off"]) == s.n + 1
    s.n_cigar_words = int(cols["cigar_off"][-1]) if s.n else 0
    s.n_aux_bytes = int(cols["aux_off"][-1]) if s.n else 0
    q = cols.get("qcheck")  # optional column: second hash of the read names
    if q is not None and s.n:
        assert q.dtype == np.uint32 and q.flags["C_CONTIGUOUS"] and len(q) == s.n
        s.qcheck = q.ctypes.data
    return s


def fetch_array(lib, handle, fn, stage):
    """Generic `*_fetch` caller -> (structured array copy, group offsets or None)."""
    data = C.c_void_p()
    count = C.c_uint64()
    goff = C.POINTER(C.c_uint64)()
    ng = C.c_uint32()
    rc = fn(handle, stage, C.byref(data), C.byref(count), C.byref(goff), C.byref(ng))
    if rc != 0:
        raise RuntimeError("fetch(stage=%d) failed rc=%d" % (stage, rc))
    dt = STAGE_DTYPE[stage]
    n = count.value
    if n:
        buf = (C.c_char * (n * dt.itemsize)).from_address(data.value)
        arr = np.frombuffer(buf, dtype=dt, count=n).copy()
    else:
        arr = np.zeros(0, dt)
    off = None
    if ng.value or bool(goff):
        off = np.ctypeslib.as_array(goff, shape=(ng.value + 1,)).copy() if bool(goff) else None
    return arr, off


class ShardStats(C.Structure):
    _fields_ = [("isize_sum", C.c_uint64), ("isize_n", C.c_uint64), ("sumsq", C.c_double), ("vmax", C.c_uint32),
                ("max_span", C.c_uint32), ("n_cand", C.c_uint64), ("n_split", C.c_uint64)]


BUF_CANDIDATES, BUF_TUPLES, BUF_CLUSTERS = 0, 1, 2
# struct Cand (csrc/bk_common.h): a row of BUF_CANDIDATES
CAND = np.dtype([("qhash", "<u8"), ("rec", "<u8"), ("tid", "<i4"), ("pos", "<i4"), ("mtid", "<i4"), ("mpos", "<i4"), ("flag", "<u2"), ("mapq", "u1"), ("pad", "u1"),
                 ("qcheck", "<u4")])
assert CAND.itemsize == 40


def device_ptrs(cols):
    """torch column dict (breakid_amd.synth_gpu) -> name -> device pointer, incl. the optional qcheck column"""
    p = {k: cols[k].data_ptr() for k, _ in SOA_COLS}
    if "qcheck" in cols:
        p["qcheck"] = cols["qcheck"].data_ptr()
    if "side" in cols:  # bk_side rows (include/breakid_hip.h): qhash, mtid, mpos, qcheck of a record in one 32-byte row
        p["side"] = cols["side"].data_ptr()
    return p
