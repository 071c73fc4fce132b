/*
 * breakid_hip.h — C ABI of libbreakid_hip.so, the MI355X (gfx950) implementation of BreakID's hot
 * path: discordant-pair scan + clustering and the split-read (SA-tag / CIGAR) breakpoint scan.
 *
 * The reference (SinOncology/BreakID) has no plugin / FFI layer: its hot path is a chain of free
 * functions called from main() (src/BreakID.cc:93-167).  Each entry point below replaces one link of
 * that chain; the reference call it stands in for is cited next to it.  A reference maintainer binds
 * them from main() as shown in INTEGRATION.md.
 *
 * Conventions: plain C, no exceptions across the boundary; every call returns BK_OK (0) or a negative
 * error code and bk_last_error() gives the text.  The caller owns all inputs; the library owns every
 * output until bk_free().  One host thread per context; the context owns one HIP stream (or uses the
 * one given to bk_set_stream).  Record columns may live in host memory (copied to HBM by
 * bk_upload_records) or already in HBM (BK_MEM_DEVICE: used in place, zero copy).
 */
#ifndef BREAKID_HIP_H
#define BREAKID_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BK_OK 0
#define BK_ERR_ARG (-1)       /* bad argument / call order */
#define BK_ERR_HIP (-2)       /* HIP runtime error (text in bk_last_error) */
#define BK_ERR_NO_DEVICE (-3) /* no gfx950 device / code object missing: the product never falls back to CPU */
#define BK_ERR_UNSORTED (-4)  /* records are not coordinate sorted (the reference needs a .bai, i.e. a sorted BAM) */
#define BK_ERR_CIGAR (-5)     /* the reference's "error cigar" exit(-1) (src/BreakID.cc:954-968) */
#define BK_ERR_IO (-6)        /* BAM decode errors (bk_bam_*) */
#define BK_ERR_LIMIT (-7)     /* an internal capacity was exceeded (text says which) */
#define BK_ERR_COLLISION (-8) /* two different read names (or contig names) share a hash: the call would not be the reference's */

#define BK_MEM_HOST 0
#define BK_MEM_DEVICE 1

typedef struct bk_ctx bk_ctx;

/* Columnar record table (structure of arrays).  One row per BAM alignment record, in file order.
 * Field meaning = bam1_core_t (thirdparty/.../htslib/sam.h:148-181): pos/mpos 0-based.
 *   cigar_off[i]..cigar_off[i+1]  BAM-encoded CIGAR words (len<<4|op) of record i
 *   aux_off[i]..aux_off[i+1]      aux blob of record i: empty when the record has no SA:Z tag,
 *                                 else the SA text, or  OC-text '\t' SA-text  when an OC:Z tag exists
 *   qhash                         64-bit hash of the read name (bk_qname_hash) used for the qname joins
 *   qcheck                        optional (may be NULL): second, independent 32-bit hash of the read name
 *                                 (bk_qname_check, never 0).  The reference compares read names as strings
 *                                 (BreakID.cc:1424, :627-637); with this column every equal-qhash decision of the mate join
 *                                 and of the breakpoint vote is verified, and a mismatch ends the run with BK_ERR_COLLISION
 *                                 instead of a silently different call.  The BAM decoders (bk_bam_*) fill it.
 * A table handed over in device memory (BK_MEM_DEVICE) is used in place: tid, pos, isize, flag, mapq, cigar_off and aux_off
 * must be 16-byte aligned there (the streaming kernels read them as vectors); BK_ERR_ARG otherwise.
 */
typedef struct bk_soa {
  uint64_t n;
  const int32_t *tid, *pos, *mtid, *mpos, *isize;
  const uint16_t *flag;
  const uint8_t *mapq;
  const uint64_t *qhash;
  const uint32_t *cigar_off; /* n+1 */
  const uint32_t *cigar;     /* cigar_off[n] words */
  const uint32_t *aux_off;   /* n+1 */
  const uint8_t *aux;        /* aux_off[n] bytes */
  uint64_t n_cigar_words;    /* = cigar_off[n] (given so that device-resident tables need no read-back) */
  uint64_t n_aux_bytes;      /* = aux_off[n] */
  const uint32_t *qcheck;    /* n entries or NULL */
  const struct bk_side *side; /* n entries or NULL: see bk_side */
} bk_soa;

/* Optional device layout of the four columns only discordant candidates and SA-bearing records need (about 5 % of the records
 * of a WGS sample): qhash, mtid, mpos and qcheck of a record in ONE 32-byte row, so that the streaming pass fetches one sector
 * per candidate instead of one per column (four scattered 4-8-byte reads cost four 64-byte fetches).  A producer that writes a
 * table in device memory may fill it (the synthetic generator does); a host table gets it when it is uploaded; when `side` is
 * given the library reads those four values from it and never touches the qhash / mtid / mpos / qcheck columns. */
typedef struct bk_side {
  uint64_t qhash;
  int32_t mtid, mpos;
  uint32_t qcheck;           /* 0 = the table has no second read-name hash */
  uint32_t reserved[3];      /* 0 */
} bk_side;                   /* 32 bytes */

/* One discordant pair = the numeric content of `discordant_pair` (src/BreakID.h:39-58). */
typedef struct bk_pair {
  uint32_t x, y;             /* p1_chr_pos, p2_chr_pos (genome-wide, util_bam.cc:57-68) */
  uint32_t p1_pos, p2_pos;   /* 1-based */
  int32_t p1_tid, p2_tid;    /* chromosome of each side (-1 = "*") */
  uint16_t p1_flag, p2_flag;
  uint8_t p1_mapq, p2_mapq, p1_rev, p2_rev;
  uint64_t rec;              /* index, in the whole sample, of the record that completed the pair (discovery order); 64 bits like the
                                reference's own counters (long / size_t, BreakID.cc:1379,1911-1913): a shard's records are numbered
                                rec_base + i, and a sample may hold more than 2^32 records even though one context does not */
  uint32_t id;               /* "pair_No_<id>": index inside its group at add_enspan_point_id time */
  int32_t cluster;           /* cluster number inside the group, -1 before clustering */
  uint32_t group;            /* group ordinal, groups ordered like std::map<string> on "chrA_chrB" */
  uint32_t reserved;         /* 0 */
} bk_pair;                   /* 56 bytes */

/* One split-read evidence tuple = numeric content of `split_align_pair` (src/BreakID.h:116-133).
 * Chromosome names are interned (ids < n_targets are header names).  CIGAR strings are only compared for equality by the
 * reference, so they travel as 64-bit codes: a text of the form <n><M|S><n><M|S> (every text that can reach a tuple: both
 * sides pass the ([0-9]+[MS]){2} gate, CigarRoller.cc:326) is encoded EXACTLY (bit 63 set; counts < 2^28, up to 3 leading
 * zeros per count), anything else as a 63-bit hash of the text (bit 63 clear). */
typedef struct bk_split {
  uint64_t rec;              /* index of the record in the whole sample (rec_base + i) */
  int32_t tid, pos, endpos;  /* of the record itself: 0-based pos, bam_endpos (sam.c:344-350) */
  uint32_t reserved;         /* second hash (bk_qname_check of the text) of an SA contig name that is neither in the header nor chr1..22,X,Y
                                (such a name is a 30-bit hash id in prim_chr / sec_chr); 0 otherwise */
  uint64_t qhash;
  int32_t prim_chr, sec_chr;
  uint32_t prim_start, prim_end, prim_bp, sec_start, sec_end, sec_bp;
  uint64_t prim_cigar, sec_cigar;
  uint32_t flags;            /* bit0 = secondary (flag & 0x100); bit1 = "error cigar" record */
  uint32_t qcheck;           /* bk_qname_check of the read name (0 when the table has no qcheck column) */
} bk_split;                  /* 88 bytes */

#define BK_TYPE_DIFF_CHR 1u
#define BK_TYPE_SAME_ORIENT 2u
#define BK_TYPE_ABS_REVERSE 4u
#define BK_TYPE_DEFAULT_ORIENT 8u

/* One cluster = numeric content of `cluster_info` (src/BreakID.h:60-113) that the txt writer needs. */
typedef struct bk_cluster {
  uint32_t group;
  int32_t id;
  int32_t p1_tid, p2_tid;
  uint32_t p1_mean, p2_mean, p1_min, p1_max, p2_min, p2_max;
  uint32_t p1_exact;
  int32_t p2_exact;
  uint32_t n_drp, n_sr;
  uint32_t depth1, depth2;
  uint32_t type_mask;        /* BK_TYPE_* : drp_type_set */
  uint32_t flags;            /* bit0 passed the near-diagonal filter (:348); bit1 valid (:446) */
} bk_cluster;

/* stage ids for bk_fetch */
#define BK_STAGE_SCAN 0      /* bk_pair[]  after scan_discordant_pairs, grouped            */
#define BK_STAGE_ISO 1       /* bk_pair[]  after remove_isolated_pairs                     */
#define BK_STAGE_CLUSTERED 2 /* bk_pair[]  after find_cluster_pairs_enspan_{fast,ahc}      */
#define BK_STAGE_SPLITS 3    /* bk_split[] every accepted split-evidence tuple, record order */
#define BK_STAGE_CLUSTERS 4  /* bk_cluster[] every cluster that passed :348, group/id order */
#define BK_STAGE_GROUP_KEYS 5 /* int32 pairs (p1_tid,p2_tid) per group ordinal               */

/* ---- lifetime ------------------------------------------------------------------------------- */
/* Replaces: samopen + header parsing (BreakID.cc:1391,1410).  target_name[i] NUL-terminated. */
int bk_init(int device, const uint32_t *target_len, const char *const *target_name, int n_targets, bk_ctx **out);
/* Optional, once per process and before its first HIP call: notes the hardware-queue count the runtime starts with (GPU_MAX_HW_QUEUES,
   default 4; the lanes of bk_mask_and_cluster, the resident sort service and the GPU feed each want a hardware queue of their own and
   share one when there are too few).  bk_init calls it; a caller with threads of its own calls it before it starts them. */
void bk_prepare_process(void);
void bk_free(bk_ctx *ctx);
const char *bk_last_error(const bk_ctx *ctx); /* ctx may be NULL: error of the failed bk_init */
int bk_set_stream(bk_ctx *ctx, void *hip_stream); /* optional: run on the caller's hipStream_t */
int bk_sync(bk_ctx *ctx);
int bk_get_stream(bk_ctx *ctx, void **hip_stream); /* the hipStream_t the context runs on (collectives of a sharded run are queued on it) */

/* Replaces: the two sequential BAM passes' record access (BreakID.cc:1414, :1929). */
int bk_upload_records(bk_ctx *ctx, const bk_soa *cols, int mem_space);

/* ---- exclude list ------------------------------------------------------------------------------------------------------
 * Every stage then behaves as if the table had no record that overlaps an excluded interval.  Overlap is htslib's region
 * predicate, the one the breakpoint stage uses: a record is excluded when tid == T && pos < end && bam_endpos > beg for an interval
 * [beg, end) on contig T, bam_endpos = pos + the reference length of the CIGAR (M, D, N, =, X), or pos + 1 for a record without
 * CIGAR or with flag 0x4.  A record with tid == -1 is never excluded.  What follows from that definition, with no special case:
 * insert-size statistics (and so w) come from the kept records only; a pair with either mate excluded does not form at the mate
 * join (its other record has no partner); excluded records give no split-evidence tuples and add nothing to depth; the kept
 * records are renumbered in file order as in a filtered file, and join order, sort ties and the 64-bit record indices of a sharded
 * run follow from that numbering.  The result equals that of bk_upload_records on the table without those records.
 * Call order: after bk_upload_records and before the stream pass; BK_ERR_ARG otherwise, with the context unchanged (after
 * bk_isize_stats or any stage, after bk_shard_begin, and on a context of bk_bam_decode_device_ctx, which has streamed already).
 * Intervals: host arrays; 0 <= tid < n_targets and 0 <= beg < end, BK_ERR_ARG otherwise; unsorted and overlapping intervals are
 * merged.  n_removed (may be NULL) receives the number of records taken out.
 * Memory: the kept records are copied, in order, into columns the context owns (the layout of a device table, bk_side rows
 * included).  After the call the context never reads the caller's BK_MEM_DEVICE table again (the caller may free it); for a
 * host upload the uploaded columns are released, so peak device memory is one table plus its kept part.  An empty list leaves a
 * host upload as it is and copies a device table. */
typedef struct bk_regions {
  const int32_t *tid, *beg, *end; /* n entries each (host memory); [beg, end) 0-based, half-open */
  uint64_t n;
} bk_regions;
int bk_exclude_regions(bk_ctx *ctx, const bk_regions *r, uint64_t *n_removed);

/* ---- stages (call in this order) ------------------------------------------------------------ */
/* get_mean_insert_size (BreakID.cc:1909-1954): bit-exact mean and sd. */
int bk_isize_stats(bk_ctx *ctx, double *mean, double *sd);
/* scan_discordant_pairs (BreakID.cc:1362-1515): filter, qname mate join, grouping. */
int bk_discordant_pairs(bk_ctx *ctx, int mapq_min, double w, uint64_t *n_pairs, uint32_t *n_groups);
/* remove_isolated_pairs (:1271) + find_cluster_pairs_enspan_fast (:1046) or _ahc (:1304), all groups. */
int bk_mask_and_cluster(bk_ctx *ctx, double w, int fast, uint64_t *n_clustered);
/* per-read SA-tag/CIGAR evidence of find_sa_reads (:892-1030) for every record, once. */
int bk_split_evidence(bk_ctx *ctx, uint64_t *n_tuples);
/* findClusterBreakPointInfoSaTag summary part (:225-352). */
int bk_cluster_summary(bk_ctx *ctx, double w, uint64_t *n_clusters);
/* findEncompassingReadsAndBreakPointInfo (:390-490): region select, find_bp_pair, depth, type. */
int bk_split_breakpoints(bk_ctx *ctx, double w, uint64_t *n_valid);

/* Whole hot path = body of main() between BreakID.cc:98 and :167 (annotation excluded).
 * w_out receives times*sqrt(times)*(mean+3sd) (:103). */
int bk_run(bk_ctx *ctx, int mapq_min, int fast, double *w_out, uint64_t *n_valid);

/* ---- matched normal --------------------------------------------------------------------------------------------------
 * Evidence for every tumour cluster in a second sample (the patient's normal), one row per BK_STAGE_CLUSTERS row, same order.
 * W = (int) w, the tumour's distance (the integer the breakpoint stage uses).
 *   n_drp   the normal's discordant pairs (its BK_STAGE_SCAN table) with the cluster's p1_tid / p2_tid, p1_pos in
 *           [p1_min - W, p1_max + W], p2_pos in [p2_min - W, p2_max + W] and an orientation bit (BK_TYPE_*, computed as for the
 *           cluster's type_mask) in the cluster's type_mask
 *   n_sr    voted clusters only (flags bit 1; 0 otherwise): the normal's split-evidence tuples (BK_STAGE_SPLITS) whose own
 *           record lies on p1_tid or p2_tid (the tuples the vote itself looks at), without the "error cigar" flag, and whose
 *           (prim_chr, prim_bp, sec_chr, sec_bp) is (p1 chromosome, p1_exact, p2 chromosome, p2_exact) or (p2 chromosome,
 *           p2_exact, p1 chromosome, p1_exact), each breakpoint within +-2 bp; chromosomes compared as the vote compares them
 *           (interned ids: the header name's for the call, and for a tuple's own side the id the stream pass gives it).  The unit
 *           is tuples, not read names: a read whose two alignments both carry SA tags counts twice, as in BK_STAGE_SPLITS.
 *   depth1, depth2  voted clusters only: cal_single_base_depth at p1_exact / p2_exact on the normal's records.
 * The struct has no typedef: the name belongs to the call below (as with `struct stat` and stat()). */
struct bk_normal_support { uint32_t n_drp, n_sr, depth1, depth2; }; /* 16 bytes */
/* tumor: after bk_split_breakpoints.  normal: after bk_isize_stats, bk_discordant_pairs(same mapq_min, tumour's w) and
 * bk_split_evidence; w = the tumour's own distance (its bk_discordant_pairs w); same device, identical reference list (names and
 * lengths); neither may be a shard (bk_shard_*).  *out: one row
 * per BK_STAGE_CLUSTERS row, library-owned until the next call or bk_free(tumor).  BK_ERR_ARG (with the reason in bk_last_error)
 * when one of these does not hold.  A normal without pairs or tuples is no error: its counts are 0. */
int bk_normal_support(bk_ctx *tumor, bk_ctx *normal, double w, const struct bk_normal_support **out, uint64_t *count);

/* ---- genotype: reference-allele evidence -------------------------------------------------------------------------------
 * Only voted clusters (flags bit 1) get counts; the rows of all others are zero.  For a voted cluster and each of its two sides s
 * (chromosome T = ps_tid, exact 1-based breakpoint e = ps_exact), let b = e - 1 (0-based), A = anchor >= 0, W = (int) w.  A record
 * i of the `records` context is eligible when
 *   - tid[i] == T, flag has 0x1, flag has none of 0x4 0x100 0x200 0x400 0x800, mapq[i] >= mapq_min,
 *   - its aux blob is empty (aux_off[i+1] == aux_off[i]: a read with an SA tag is junction evidence, never reference evidence),
 *   - pos[i] <= b - A.
 * Then
 *   ref_reads_s = eligible records with bam_endpos(i) >= b + 1 + A (bam_endpos as in bk_exclude_regions: the aligned reference
 *                 interval covers the breakpoint base with at least A bases on either side; soft clips do not count, D and N do),
 *   ref_pairs_s = eligible records that also have flag 0x2, lack 0x8, and have 0 < isize[i] <= W and
 *                 pos[i] + isize[i] >= b + 1 + A (the left mate of a properly paired fragment that spans the breakpoint;
 *                 isize > 0 counts a fragment once; only the left mate's own mapq and aux are looked at).
 * All comparisons in signed 64-bit.  A read can count in both.  T < 0 gives zeros.
 * The struct has no typedef: the name belongs to the call below. */
struct bk_ref_support { uint32_t ref_pairs1, ref_pairs2, ref_reads1, ref_reads2; }; /* 16 bytes */
/* calls: after bk_split_breakpoints.  records: after bk_isize_stats (the stream pass gives the longest alignment); records == calls
 * genotypes the sample itself, another context on the same device with an identical reference list (names and lengths) is the
 * matched normal.  Neither may be a shard (bk_shard_*).  *out: one row per BK_STAGE_CLUSTERS row, same order, library-owned until
 * the next call or bk_free(calls).  BK_ERR_ARG (with the reason in bk_last_error) for wrong call order, anchor < 0, mapq_min < 0,
 * differing reference lists, shards.  It changes nothing a later bk_fetch or stage returns, and works on every table form the
 * context can hold (host upload, BK_MEM_DEVICE with and without `side`, the table bk_exclude_regions left behind, the context of
 * bk_bam_decode_device_ctx while its bk_bam_dev lives). */
int bk_ref_support(bk_ctx *calls, bk_ctx *records, int mapq_min, int anchor, double w, const struct bk_ref_support **out, uint64_t *count);
/* The genotype model, a pure host function (no context, no GPU).  With k = alt, r = ref and c = (log10 0.05, log10 0.5, log10 0.95)
 * (a 5 % error rate, as SV genotypers use: the model's constants, not measurements): L[g] = k * c[g] + r * c[2 - g] for g = 0, 1, 2
 * in double precision, each product rounded on its own; gt = the g with the largest L (the smaller g on a tie; 0 = 0/0, 1 = 0/1,
 * 2 = 1/1); gq = min(99, floor(10 * (L[best] - L[second]) + 0.5)); vaf = (float) k / (float) ((uint64_t) k + r).  k + r == 0:
 * gt = 255 ("./."), gq = 0, vaf = NaN.  A call is genotyped on its junction reads: alt = n_sr, ref = (ref_reads1 + ref_reads2 + 1) / 2;
 * the pair counts stand beside it: n_drp against (ref_pairs1 + ref_pairs2 + 1) / 2.  BK_ERR_ARG for a null output. */
int bk_genotype_call(uint32_t alt, uint32_t ref, uint8_t *gt, uint8_t *gq, float *vaf);

/* ---- junction evidence: which side of each breakpoint the retained sequence lies on (what a VCF breakend must say) -------
 * One row per BK_STAGE_CLUSTERS row, same order.
 *   Member pairs of a cluster c are the rows of BK_STAGE_CLUSTERED with group == c.group && cluster == c.id.
 *     pairs[2 * p1_rev + p2_rev] counts them, mapq_sum1 / mapq_sum2 add their p1_mapq / p2_mapq.  Every row gets these, voted or
 *     not, so pairs[0] + pairs[1] + pairs[2] + pairs[3] == n_drp.  A forward-strand read lies left of its breakpoint, a
 *     reverse-strand read right of it.
 *   Matching tuples, voted clusters only (flags bit 1; zeros otherwise): exactly the set bk_normal_support.n_sr is defined over,
 *     but on the context's own BK_STAGE_SPLITS: tuples whose own record lies on p1_tid or p2_tid, without the "error cigar" flag,
 *     whose (prim_chr, prim_bp, sec_chr, sec_bp) is within +-2 bp of (p1 chromosome, p1_exact, p2 chromosome, p2_exact) - then side
 *     1 is prim and side 2 is sec - or else of (p2 chromosome, p2_exact, p1 chromosome, p1_exact) - then side 1 is sec and side 2
 *     is prim; chromosomes compared as interned ids, as there; when both hold the first wins; the unit is tuples, each counted once.
 *     A side is RIGHT when its *_bp == *_start (the alignment begins at the breakpoint and extends to the right: a leading clip),
 *     otherwise LEFT (*_bp == *_end).  splits[2 * right1 + right2] counts them, so the four bins sum to the n_sr that
 *     bk_normal_support reports for a normal that holds the same table.
 * The struct has no typedef: the name belongs to the call below. */
struct bk_junction {
  uint32_t pairs[4];    /* member pairs of the cluster by strands, index = 2 * p1_rev + p2_rev */
  uint32_t splits[4];   /* matching split tuples by clip side, index = 2 * right1 + right2; voted clusters only, else 0 */
  uint64_t mapq_sum1, mapq_sum2;   /* sums of p1_mapq / p2_mapq over the member pairs */
};                      /* 48 bytes */
/* ctx: after bk_split_breakpoints, with the lists of its bk_mask_and_cluster / bk_cluster_summary still in place; not a shard
 * (bk_shard_*).  *out: library-owned until the next call or bk_free(ctx).  BK_ERR_ARG (with the reason in bk_last_error) for wrong
 * call order, null outputs and shards.  It changes nothing a later bk_fetch or stage returns, and works on every table form the
 * context can hold.  A context without clusters is no error: *count = 0. */
int bk_junctions(bk_ctx *ctx, const struct bk_junction **out, uint64_t *count);
/* Pure host functions (no context, no GPU), so that every caller shares one rule.
 * bk_junction_sides: which side of each breakpoint the retained sequence lies on.  If any splits[] is non-zero: the index of the
 * largest splits[] bin, *source = 2; else if any pairs[] is non-zero: the index of the largest pairs[] bin, *source = 1 (the index
 * means the same: forward = left, reverse = right); else index 1, *source = 0.  The smallest index wins a tie.
 * *right1 = index >> 1, *right2 = index & 1.  BK_ERR_ARG for a null argument. */
int bk_junction_sides(const struct bk_junction *j, uint8_t *right1, uint8_t *right2, uint8_t *source);
/* bk_vcf_breakend_alt: the ALT text of one breakend (VCF 4.2, section 5.4) into buf, NUL-terminated.  Own side left: the base
 * comes first; mate right: '[', mate left: ']'.  (own, mate) = (left, right): N[chr:pos[, (left, left): N]chr:pos], (right, left):
 * ]chr:pos]N, (right, right): [chr:pos[N.  BK_ERR_ARG for a null mate_chr or buf, or a buffer too small for the text and its NUL. */
int bk_vcf_breakend_alt(char ref_base, int own_right, const char *mate_chr, uint32_t mate_pos, int mate_right, char *buf, size_t cap);

/* ---- soft-clip evidence: clipped reads without an SA tag, at every cluster ----------------------------------------------------
 * The vote (bk_split_breakpoints) sees only reads with an SA tag.  A read that is soft-clipped at the junction but carries none (a
 * clip too short to place, an aligner that writes no SA, a second segment in a repeat) is counted here, for every row of
 * BK_STAGE_CLUSTERS, voted or not, same order.  Parameters: mapq_min >= 0, min_clip >= 1, W = (int) w (the integer the breakpoint
 * stage uses).  All comparisons in signed 64-bit.
 * Clip events of a record i of the `records` context.  The record is eligible when tid[i] >= 0, flag has none of 0x4 0x100 0x200
 * 0x400 0x800 (0x1 is not required), mapq[i] >= mapq_min, its aux blob is empty (aux_off[i+1] == aux_off[i]: a read with an SA tag
 * is split-read evidence already, so clip evidence and N_SR stay disjoint) and its CIGAR has a reference length > 0 (M, D, N, =, X).
 * It gives up to two events (tid, p, dir), p 1-based as p1_exact / prim_bp are, dir 0 = LEFT, 1 = RIGHT as right1 / right2 of
 * bk_junction_sides:
 *   leading   after skipping leading H ops the first op is S with length >= min_clip: (tid, pos + 1, RIGHT) - the alignment starts
 *             at the breakpoint and extends right;
 *   trailing  after skipping trailing H ops the last op is S with length >= min_clip: (tid, bam_endpos, LEFT), bam_endpos as in
 *             bk_exclude_regions (the 1-based last aligned base equals the 0-based exclusive end).
 * Per row and side s (0 = p1, 1 = p2): T = ps_tid, window [max(1, ps_min - W), ps_max + W] (the window of bk_normal_support.n_drp);
 * T < 0 gives zeros.  For each dir:
 *   events[s][dir]    events on T with p in the window
 *   peak_n, peak_pos  the largest number of events of that direction that share one exact p in the window, and that p (the
 *                     smallest p on a tie); both 0 without an event
 *   at[s][dir]        voted rows only (flags bit 1; 0 otherwise): events on T with |p - ps_exact| <= 2, the +-2 bp of the tuple
 *                     matching of bk_normal_support / bk_junctions (counted wherever ps_exact lies, inside the window or not)
 * The struct has no typedef: the name belongs to the call below. */
struct bk_clip_support { uint32_t at[2][2], peak_pos[2][2], peak_n[2][2], events[2][2]; }; /* [side][dir], 64 bytes */
/* calls: after bk_split_breakpoints.  records: after bk_isize_stats (the stream pass gives the longest alignment); records == calls
 * is the sample itself, another context on the same device with an identical reference list (names and lengths) is the matched
 * normal.  Neither may be a shard (bk_shard_*).  *out: one row per BK_STAGE_CLUSTERS row, same order, library-owned until the next
 * call or bk_free(calls).  BK_ERR_ARG (with the reason in bk_last_error) for wrong call order, min_clip < 1, mapq_min < 0, differing
 * reference lists, shards, null outputs.  It changes nothing a later bk_fetch or stage returns, and works on every table form the
 * context can hold (host upload, BK_MEM_DEVICE with and without `side`, the table bk_exclude_regions left behind, the context of
 * bk_bam_decode_device_ctx while its bk_bam_dev lives).  A context without clusters is no error: *count = 0. */
int bk_clip_support(bk_ctx *calls, bk_ctx *records, int mapq_min, int min_clip, double w, const struct bk_clip_support **out, uint64_t *count);
/* cal_single_base_depth (the count behind depth1 / depth2) at n arbitrary 1-based positions; tid and pos are host arrays, tid < 0
 * gives 0.  records: after bk_isize_stats, not a shard.  *out: n counts, library-owned until the next call or bk_free(records). */
int bk_base_depth(bk_ctx *records, const int32_t *tid, const uint32_t *pos, uint64_t n, const uint32_t **out);
/* The rescue rule, a pure host function (no context, no GPU), so that every caller shares it.  Returns 1 and fills the outputs when
 * the row is unvoted (!(flags & 2)), both tids are >= 0, and with (d1, d2) the sides bk_junction_sides(j) gives (for an unvoted row
 * they come from the strands of its pairs) peak_n[0][d1] >= min_support and peak_n[1][d2] >= min_support; then pos_s =
 * peak_pos[s][d_s] and n_s = peak_n[s][d_s].  Returns 0 otherwise, BK_ERR_ARG for a null argument or min_support == 0.  The command
 * line's min_support is 3: one more than the vote's own threshold of 2 (BreakID.cc:446), because no second alignment verifies a
 * clip position - a constant of the model, not a measurement. */
int bk_clip_rescue(const bk_cluster *c, const struct bk_junction *j, const struct bk_clip_support *s, uint32_t min_support, uint32_t *pos1, uint32_t *pos2, uint32_t *n1,
                   uint32_t *n2);

/* ---- the clipped reads at a site ------------------------------------------------------------------------------------------
 * bk_clip_support counts the clip events of every cluster window; bk_clip_reads counts, and lists, the clip events at sites the
 * caller names, on any records context.  Which records are eligible and which events (tid, p, dir) a record has is exactly what
 * bk_clip_support (above) defines, with the same mapq_min and min_clip; nothing of it is restated here.  An event (tid, p, d) belongs
 * to site k when, compared in signed 64-bit,
 *   tid == sites[k].tid,  d == sites[k].dir,  |p - sites[k].pos| <= sites[k].tol.
 * counts[k] is the number of such events; a site with tid < 0 gives 0.  Two sites may overlap or be equal: an event is then counted,
 * and its record listed, under each.
 * rows lists the events, one bk_clip_read each.  Order (part of the contract; two runs give the same bytes): by site ascending,
 * within a site by `rec` ascending - a record has at most one event per direction, so this is a total order.
 * site_off[k] .. site_off[k + 1] bounds site k; site_off has n_sites + 1 entries.  A read name is not kept on the device: a row
 * carries the two hashes of its record, which bk_bam_extract turns back into names and records.
 * Two identities tie the call to bk_clip_support(calls, records, mapq_min, min_clip, w): for every row c, side s and direction d
 *   a site (ps_tid, peak_pos[s][d], 0, d) counts peak_n[s][d], and
 *   for a voted row a site (ps_tid, ps_exact, 2, d) counts at[s][d].
 * Neither struct has a typedef: the names belong to the call below. */
struct bk_clip_site { int32_t tid; uint32_t pos; uint32_t tol; uint32_t dir; }; /* 16 bytes; pos 1-based, dir 0 = LEFT, 1 = RIGHT */
struct bk_clip_read {
  uint64_t rec;               /* index of the record in the context's table, as bk_evidence.rec is */
  uint64_t qhash;             /* qhash of record `rec` */
  uint32_t qcheck;            /* likewise (0 when the table has no qcheck) */
  uint32_t site;              /* k */
  int32_t tid; uint32_t p;    /* the event's own contig and position (1-based) */
  uint32_t clip_len;          /* length of the S op that made the event */
  uint16_t flag;              /* of the record */
  uint8_t mapq;               /* of the record */
  uint8_t dir;                /* 0 = LEFT, 1 = RIGHT */
};                            /* 40 bytes */
/* records: after bk_isize_stats (the stream pass gives the longest alignment), not a shard (bk_shard_*).  sites: a host array.
 * *counts (n_sites entries), *rows (site_off[n_sites] rows) and *site_off are library-owned until the next call or bk_free(records).
 * rows == NULL && site_off == NULL asks for the counts only: no listing is made (this is how a matched normal is counted).
 * BK_ERR_ARG (with the reason in bk_last_error) for wrong call order, shards, min_clip < 1, mapq_min < 0, a dir above 1, null counts,
 * exactly one of rows / site_off null, null sites with n_sites > 0, and for a listing asked of a table that has neither a qhash
 * column nor `side` rows.  BK_ERR_LIMIT beyond 2^30 sites or 2^32 rows.  n_sites == 0 is no error: site_off has its one entry, 0.
 * It changes nothing a later bk_fetch or stage returns, and works on every table form the context can hold (host upload,
 * BK_MEM_DEVICE with and without `side`, the table bk_exclude_regions left behind, the context of bk_bam_decode_device_ctx while its
 * bk_bam_dev lives). */
int bk_clip_reads(bk_ctx *records, const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, const uint32_t **counts,
                  const struct bk_clip_read **rows, const uint64_t **site_off);

/* ---- evidence export: the reads behind every call -----------------------------------------------------------------------
 * bk_junctions counts a cluster's member pairs and, for a voted cluster, its matching tuples; bk_evidence lists the same rows, one
 * bk_evidence row each.  Membership is exactly that of bk_junctions (above): a BK_EV_PAIR row for every member pair of every
 * BK_STAGE_CLUSTERS row, voted or not, and a BK_EV_SPLIT row for every matching tuple of a voted one, side 1 and side 2 assigned
 * as there (the first orientation wins when both hold).  So, per call, the BK_EV_PAIR rows number n_drp, their histogram over
 * `sides` is bk_junction.pairs, and that of the BK_EV_SPLIT rows is bk_junction.splits.
 * Order (part of the contract; two runs give the same bytes): by `call` ascending, within a call pairs before splits, pairs in
 * ascending BK_STAGE_CLUSTERED row, splits in ascending BK_STAGE_SPLITS row.  call_off[c] .. call_off[c + 1] bounds call c.
 * A read name is not kept on the device: a row carries its two hashes (qhash, qcheck), which bk_bam_extract turns back into names
 * and records.  The struct has no typedef: the name belongs to the call below. */
#define BK_EV_PAIR 1
#define BK_EV_SPLIT 2
struct bk_evidence {
  uint64_t rec;               /* pair: bk_pair.rec; split: bk_split.rec */
  uint64_t qhash;             /* pair: qhash of record `rec` of the context's table; split: bk_split.qhash */
  uint32_t qcheck;            /* likewise (0 when the table has no qcheck) */
  uint32_t call;              /* row in BK_STAGE_CLUSTERS */
  int32_t tid1; uint32_t pos1; /* pair: p1_tid, p1_pos (1-based); split: the call's p1_tid and the tuple's breakpoint on side 1 */
  int32_t tid2; uint32_t pos2; /* pair: p2_tid, p2_pos; split: p2_tid and the tuple's breakpoint on side 2 */
  uint16_t flag1, flag2;      /* pair: p1_flag, p2_flag; split: low 16 bits of bk_split.flags, and 1 if (prim, sec) = (side 2, side 1) else 0 */
  uint8_t mapq1, mapq2;       /* pair: p1_mapq, p2_mapq; split: mapq of record `rec`, 0 */
  uint8_t kind;               /* BK_EV_PAIR / BK_EV_SPLIT */
  uint8_t sides;              /* pair: 2 * p1_rev + p2_rev; split: 2 * right1 + right2, as bk_junction.splits is indexed */
};                            /* 48 bytes */
/* ctx: as for bk_junctions (after bk_split_breakpoints, the lists still in place, not a shard).  *out (count rows) and *call_off
 * (n_clusters + 1 entries) are library-owned until the next call or bk_free(ctx).  BK_ERR_ARG (with the reason in bk_last_error) for
 * wrong call order, null arguments and shards.  It changes nothing a later bk_fetch or stage returns, and works on every table
 * form the context can hold (host upload, BK_MEM_DEVICE with and without `side`, the table bk_exclude_regions left behind, the
 * context of bk_bam_decode_device_ctx while its bk_bam_dev lives).  A context without clusters is no error: *count = 0 and
 * call_off has its one entry, 0. */
int bk_evidence(bk_ctx *ctx, const struct bk_evidence **out, uint64_t *count, const uint64_t **call_off);

/* ---- unique support: how many different fragments stand behind every call ---------------------------------------------------
 * n_drp and n_sr count rows: a PCR duplicate that the BAM does not mark (0x400) counts again, the isolation and clustering stages
 * keep some pairs twice, and a split read whose two alignments both carry an SA tag gives two tuples.  bk_unique_support groups the
 * rows of bk_evidence by fragment.  Membership, order and side assignment are exactly those of bk_evidence (above); row r below
 * is row r of what bk_evidence would return.
 * Fragment key, compared as exact integers (no hash decides that two rows are equal):
 *   BK_EV_PAIR row of member pair p    (p1_pos, p2_pos, p1_rev != 0, p2_rev != 0)
 *   BK_EV_SPLIT row of tuple t         (A1_start, A1_end, A2_start, A2_end, mtid[t.rec], mpos[t.rec]): A1, A2 = the tuple's prim_* and
 *                                      sec_* start and end, A1 = prim unless the row is swapped (the row's flag2); mtid / mpos of
 *                                      record t.rec of the context's table (from the bk_side row when the table has them).  Both
 *                                      tuples of one read give the same key; the mate position separates fragments that share a
 *                                      read start.
 * Two rows are the same fragment when they have the same call, the same kind and equal keys.  first[r] = the smallest row index of
 * r's fragment (first[first[r]] == first[r] <= r); n_rows = bk_evidence's count.
 * Per BK_STAGE_CLUSTERS row, for pair rows and for split rows: uniq_* = the number of fragments (rows with first[r] == r), top_* =
 * the rows of the largest fragment (0 without rows).  An unvoted row has no split rows: uniq_splits = top_splits = 0.
 * Limits: positions are leftmost alignment starts, not unclipped 5' ends, so duplicates that differ in soft clipping stay apart
 * (the count errs towards more fragments); a pair row and a split row of one fragment are counted each in its own column.
 * The struct has no typedef: the name belongs to the call below. */
struct bk_unique_support { uint32_t uniq_pairs, top_pairs, uniq_splits, top_splits; }; /* 16 bytes */
/* ctx, call order, errors and table forms: as for bk_evidence; it needs no earlier bk_evidence call, leaves the buffers bk_evidence
 * returned valid and unchanged, and changes nothing a later bk_fetch or stage returns.  *out (*count = n_clusters rows) and *first
 * (*n_rows entries) are library-owned until the next bk_unique_support or bk_free(ctx).  first == NULL and n_rows == NULL asks for
 * the counts alone; exactly one of them null is BK_ERR_ARG, as are null out / count, shards, wrong call order, and a table with
 * clusters but neither mtid / mpos columns nor bk_side rows.  A context without clusters is no error: *count = 0, *n_rows = 0. */
int bk_unique_support(bk_ctx *ctx, const struct bk_unique_support **out, uint64_t *count, const uint64_t **first, uint64_t *n_rows);

/* ---- junction consensus: what the clipped reads read across a breakpoint ------------------------------------------------------
 * bk_clip_reads says which reads are clipped at a site; bk_clip_consensus says what their clipped bases are: per site the clipped
 * bases are piled up column by column, counting away from the junction, and every column votes one base.  No layer of a context
 * carries SEQ, so the alignments come as a table of their own, bk_reads, in host memory: what bk_bam_reads (below, with the host
 * feed) brings back for a set of read names, or columns the caller built.  Base q of read i is in byte seq_off[i] + q / 2 of seq,
 * the high nibble when q is even, in BAM's 4-bit codes (=ACMGRSVTWYHKDBN); every read starts on a byte. */
typedef struct bk_reads {       /* a table of its own, not a context's record table; host memory */
  uint64_t n;
  const int32_t *tid, *pos;     /* pos 0-based */
  const uint16_t *flag;
  const uint8_t *mapq;
  const uint32_t *key;          /* index of the bk_read_key that selected the alignment (bk_bam_reads; bk_clip_consensus does not read it) */
  const uint32_t *cigar_off;    /* n + 1 */
  const uint32_t *cigar;        /* BAM words, len << 4 | op */
  const uint32_t *l_seq;
  const uint64_t *seq_off;      /* n + 1, in bytes */
  const uint8_t *seq;
  void *owner;                  /* bk_reads_free */
} bk_reads;
/* All comparisons in signed 64-bit.
 * Eligible alignment i of `reads`: tid[i] >= 0, flag has none of 0x4 0x200 0x400 (0x100 and 0x800 are allowed: the second part of a
 * chimeric read is what the far side needs, and a hard-clipped one has no S op and so no event), mapq[i] >= mapq_min, its CIGAR has
 * a reference length > 0, l_seq[i] > 0 and l_seq[i] equals the CIGAR's query length (M, I, S, =, X).
 * Events: (tid, p, dir) and the clip length c = the length of the S op are those bk_clip_support (above) defines, leading and
 * trailing, with min_clip; nothing of it is restated here.  The one difference: there is no aux condition (a bk_reads table has no
 * aux column), so reads with an SA tag count here.
 * Membership: an event belongs to site k when tid == sites[k].tid, dir == sites[k].dir and p == sites[k].pos (sites[k].tol must be 0).
 * Equal sites each get the event; a site with tid < 0 gets nothing.
 * Columns count bases away from the junction, 0 <= j < min(c, max_len): of a trailing clip (LEFT) column j is base l_seq - c + j, of
 * a leading clip (RIGHT) base c - 1 - j (leading H ops hold no bases).
 * Per site k and column j: depth[j] = the number of events with c > j (it does not increase with j); counts are kept for A, C, G, T
 * (codes 1, 2, 4, 8), every other code counts in depth only.
 *   len                      the number of columns with depth[j] >= min_depth
 *   bases[k * max_len + j]   j < len: the most frequent of A, C, G, T, on a tie the smaller in the order A < C < G < T, 'N' when all
 *                            four counts are 0; j >= len: 0
 *   match, total             sums over j < len of the winning count and of depth[j]
 *   n_reads                  the number of events of the site
 *   col_depth[k * max_len + j] = depth[j] for every j < max_len
 * Every output is an integer sum or an argmax with a fixed tie rule: two runs, and any permutation of the rows of `reads`, give the
 * same bytes.  The struct has no typedef: the name belongs to the call below. */
struct bk_consensus { uint32_t n_reads, len, match, total; };   /* 16 bytes */
/* ctx: any live context that is not a shard (bk_shard_*); it gives the device, the stream, the buffers and bk_timing (scope
 * `consensus`).  No stage needs to have run and nothing a later bk_fetch or stage returns changes.  reads, sites: host memory.
 * *out (n_sites rows), *bases and *col_depth (n_sites * max_len entries each) are library-owned until the next call or bk_free(ctx);
 * col_depth may be NULL: not wanted.  BK_ERR_ARG (with the reason in bk_last_error) for shards, null ctx / reads / out / bases, null
 * sites with n_sites > 0, a null column of a table with n > 0, max_len outside 1..256, min_depth == 0, min_clip < 1, mapq_min < 0, a
 * dir above 1, tol != 0, cigar_off or seq_off that do not ascend, and a seq_off span shorter than (l_seq + 1) / 2 bytes.
 * BK_ERR_LIMIT beyond 2^32 reads, 2^30 sites or 2^32 events that belong to a site.  n_sites == 0 or reads->n == 0 is no error. */
int bk_clip_consensus(bk_ctx *ctx, const bk_reads *reads, const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, uint32_t max_len,
                      uint32_t min_depth, const struct bk_consensus **out, const uint8_t **bases, const uint32_t **col_depth);

/* ---- junction fit: the voted sequence of a side against the reference at the other side -----------------------------------------
 * bk_clip_consensus says what the clipped reads of a side read across the junction; bk_junction_fit says where that sequence lies in
 * the partner locus: how much of it continues there (aligned, mism), where exactly the continuation starts (shift), how many bases
 * that neither side templates lie in between (ins), and how many bases both sides share at the junction (hom_fwd, hom_back).
 * All comparisons in signed 64-bit.
 * Reference: bk_refseq, host memory, uploaded per call as bk_reads is.  Base i of segment g is nibble i of the bytes from off[g], the
 * high nibble first; every segment starts on a byte.  The nibbles are in nib encoding: T = 0, C = 1, A = 2, G = 3, the codes 4..7 are
 * N, bit 3 is the soft-mask and is ignored; the payload of a .nib file behind its 8-byte header is a valid segment as it lies.
 * Segments are sorted by (tid, start) and do not overlap (start[g] + len[g] <= start[g + 1] on one tid); they may abut and may leave
 * gaps.  ref(t, p), the base at the 1-based position p of contig t, is N when t < 0, p < 1 or no segment covers p (segment g covers
 * start[g] < p <= start[g] + len[g]).  comp() complements a base; comp(N) = N. */
typedef struct bk_refseq {
  uint64_t n_segs;
  const int32_t *tid;
  const uint32_t *start;        /* 0-based */
  const uint32_t *len;          /* bases */
  const uint64_t *off;          /* n_segs + 1, in bytes */
  const uint8_t *bases;
} bk_refseq;
/* Probe k: its own side (tid_own, pos_own, dir_own), the other side of the call (tid_mate, pos_mate, dir_mate), dir 0 = LEFT and
 * 1 = RIGHT as everywhere else, and its query query[k * max_len + j], j < qlen <= max_len: ASCII A C G T N, column j counting away
 * from the junction.  That is the layout and the stride of `bases` from bk_clip_consensus (with qlen = len): one call's output is
 * the next call's input without repacking. */
struct bk_junction_probe { int32_t tid_own; uint32_t pos_own, dir_own; int32_t tid_mate; uint32_t pos_mate, dir_mate; uint32_t qlen, reserved; };  /* 32 bytes */
/* Walks, for any integer index:
 *   own   O[j] = ref(tid_own, pos_own + 1 + j) for LEFT, ref(tid_own, pos_own - 1 - j) for RIGHT; never complemented.  O[0], O[1], ..
 *         is what the reads would read had they gone on in their own locus; O[-1], O[-2], .. are the last bases they retain.
 *   mate  M[i] = ref(tid_mate, pos_mate + i) when dir_mate is RIGHT, ref(tid_mate, pos_mate - i) when it is LEFT; complemented iff
 *         dir_own == dir_mate.  M[0], M[1], .. is the retained sequence of the partner as this side's reads read it.
 * Placements: 0 <= ins <= min(max_ins, qlen - 1), -max_shift <= shift <= max_shift; column j >= ins is compared with
 * M[j - ins + shift].  A column matches iff the query byte is one of A C G T and equals the walk's base; everything else is a
 * mismatch, N on either side included.  aligned = qlen - ins, mism = the mismatching columns, score = aligned - 2 * mism: a match
 * +1, a mismatch -1, an inserted column 0.  Chosen is the placement with the largest score; on a tie the smaller ins, then the
 * smaller |shift|, then shift >= 0 before shift < 0.
 * Why this score: with ins + mism as a cost no insertion is ever reported, since a few random inserted bases cost less as mismatches
 * on the neighbouring diagonal than as an insertion.  With an inserted column at 0 and a mismatch at 2 relative to a match, a single
 * mismatch in column 0 reads as ins 1, shift 1 (one non-templated base), and a mismatch in column 1 or later stays a mismatch.  Both
 * are intended.
 * Microhomology, counted only when the chosen ins == 0 (else both are 0):
 *   hom_fwd   the number of leading columns j = 0, 1, .. < qlen with query[j] == O[j] == M[j + shift], all of A C G T
 *   hom_back  the number of leading i = 0, 1, .. < max_hom with O[-1 - i] == M[shift - 1 - i], both of A C G T
 * (leading: the count stops at the first index that fails).  placed = 1 iff qlen >= 1 and both tids are >= 0; an unplaced row is
 * all zeros.  Every output is an integer count or an argmax with a fixed tie rule: two runs, and any permutation of the probes, give
 * the same bytes row for row.  The structs have no typedef: bk_junction_fit names the call below. */
struct bk_junction_fit { int32_t shift; uint32_t ins, aligned, mism, hom_fwd, hom_back; int32_t score; uint32_t placed; };  /* 32 bytes */
/* ctx: any live context that is not a shard (bk_shard_*); it gives the device, the stream, the buffers and bk_timing (scope
 * `junction_fit`).  No stage needs to have run and nothing a later bk_fetch or stage returns changes.  ref, probes, query: host
 * memory.  *out (n rows) is library-owned until the next call or bk_free(ctx).  BK_ERR_ARG (with the reason in bk_last_error) for
 * shards, null ctx / ref / out, null probes or query with n > 0, max_len outside 1..256, max_shift, max_ins or max_hom above 64, a
 * dir above 1, qlen > max_len, a query byte outside ACGTN within qlen, a null column of a table with n_segs > 0, segments out of
 * order or overlapping, off that does not ascend, and an off span shorter than (len + 1) / 2 bytes.  BK_ERR_LIMIT beyond 2^30
 * probes or 2^20 segments.  n == 0 is no error, and neither is n_segs == 0 (every walk is then N). */
int bk_junction_fit(bk_ctx *ctx, const bk_refseq *ref, const struct bk_junction_probe *probes, uint64_t n, const uint8_t *query, uint32_t max_len, uint32_t max_shift,
                    uint32_t max_ins, uint32_t max_hom, const struct bk_junction_fit **out);

/* ---- locus similarity: the reference at one breakpoint of a call against the reference at the other ------------------------------
 * Two paralogous genes, a processed pseudogene and its parent, or two copies of a segmental duplication share a stretch of sequence;
 * reads of one copy align to the other and a call forms between them.  bk_locus_similarity says how alike the two loci of a call are:
 * the best ungapped stretch that window A, the reference around one breakpoint, shares with window B around the other, forward or
 * reverse-complemented, and the longest exact common substring.  It reads nothing but the reference (bk_refseq, ref() and comp()
 * as above; the soft-mask bit is ignored).  All arithmetic in signed 64-bit.
 * Pair k: (tid_a, pos_a) and (tid_b, pos_b), pos 1-based.  R = flank, L = 2 R + 1.
 *   window A                 a[i]  = ref(tid_a, pos_a - R + i), 0 <= i < L
 *   window B, orientation 0  b0[j] = ref(tid_b, pos_b - R + j)
 *   window B, orientation 1  b1[j] = comp(ref(tid_b, pos_b + R - j)): the reverse complement
 * Cell (o, i, j) matches iff a[i] is one of A C G T and equals b_o[j].  A segment (o, d, i0, n), n >= 1, covers the columns
 * i0 .. i0 + n - 1 of A against b_o[i + d], all inside both windows; its score is matches - 2 * mismatches, and every column that
 * does not match is a mismatch, N on either side included.  The weights are a constant of the model: a stretch below two thirds
 * identity does not grow, which is about where reads begin to mis-align between two copies.
 * Excluded diagonal: when tid_a == tid_b, the diagonal d = pos_a - pos_b of orientation 0 compares every base with itself; it is left
 * out entirely, of the best segment and of `run`.  (Without this every call whose breakpoints lie within 2 R of each other, a small
 * deletion or duplication, would score its own overlap.)
 * Best segment: the largest key (score, -n, -o, -|d|, [d >= 0], -i0): the highest score, then the shortest, orientation 0 first, the
 * diagonal nearest 0, d >= 0 before d < 0, the smallest start.  When its score is > 0: found = 1, score, len = n,
 * mism = (len - score) / 3, diag = d, start = i0, orient = o; otherwise the row is all zeros (tid < 0, windows of N, n_segs == 0).
 * run: the longest stretch of consecutive matching cells on any diagonal of either orientation but the excluded one: the longest
 * exact common substring.  found == 1 iff run >= 1.
 * One pass finds the best segment of a diagonal: a running sum of +1 / -2 that restarts wherever it is <= 0, every end position
 * offering (sum, length since the restart).
 * Among random windows the best score is about 8 to 11 and run 8 to 10 (L = 301 and 511): orientation for the reader, no threshold.
 * Every output is an integer count or an argmax with a fixed tie rule: two runs, and any permutation of the pairs, give the same bytes
 * row for row.  The structs have no typedef. */
struct bk_locus_pair { int32_t tid_a; uint32_t pos_a; int32_t tid_b; uint32_t pos_b; };              /* 16 bytes, pos 1-based */
struct bk_locus_sim  { uint32_t score, len, mism, run; int32_t diag; uint32_t start, orient, found; }; /* 32 bytes */
/* ctx: any live context that is not a shard (bk_shard_*); it gives the device, the stream, the buffers and bk_timing (scope
 * `locus_similarity`; bk_timing_touched is n * (48 + L): the pair row, the result row and L nibbles of each window).  No stage needs
 * to have run and nothing a later bk_fetch or stage returns changes.  ref, pairs: host memory.  *out (n rows) is library-owned until
 * the next call or bk_free(ctx).  BK_ERR_ARG (with the reason in bk_last_error) for shards, null ctx / ref / out, null pairs with
 * n > 0, flank outside 1..255, and every defect of the reference table that bk_junction_fit rejects.  BK_ERR_LIMIT beyond 2^30 pairs
 * or 2^20 segments, looked at before any array is read.  n == 0 is no error, and neither is n_segs == 0 (every row is then zero). */
int bk_locus_similarity(bk_ctx *ctx, const bk_refseq *ref, const struct bk_locus_pair *pairs, uint64_t n, uint32_t flank, const struct bk_locus_sim **out);

/* ---- sequence match: short queries searched in a library of sequences the caller supplies -----------------------------------------
 * bk_junction_fit and bk_locus_similarity read the sample's own reference at positions the caller knows.  bk_sequence_match answers
 * the other question: which sequence of a panel (Alu / L1 / SVA consensus sequences, a viral genome, a vector) does a read-derived
 * sequence such as a clip consensus continue into, on which strand and where.  The contract below describes results only; how they
 * are found (a k-mer index, seeded ungapped extension) is the library's business, and a brute force over every diagonal gives the
 * same bytes.  All comparisons in signed 64-bit.
 * Panel: host memory, uploaded and indexed per call.  Sequence s is P_s = bases[off[s] .. off[s + 1]), ASCII, only A C G T N (lower
 * case is the caller's to fold); len_s = off[s + 1] - off[s].  A sequence's neighbours in `bases` are not part of it. */
typedef struct bk_seq_panel {
  uint64_t n_seqs;
  const uint64_t *off;          /* n_seqs + 1, in bases; off[0] == 0 */
  const uint8_t *bases;
} bk_seq_panel;
/* Probe k has qlen <= max_len bytes at query[k * max_len ..], ASCII A C G T N: the layout and the stride of `bases` from
 * bk_clip_consensus (with qlen = len).  Its string is q[i] = query[k * max_len + i], or query[k * max_len + qlen - 1 - i] when
 * `reversed` is set: that is for a RIGHT site, whose columns count backwards, so that q reads in BAM orientation and one call's
 * output is the next call's input without repacking (reversed = dir). */
struct bk_seq_probe { uint32_t qlen, reversed; };   /* 8 bytes */
/* Orientations: q_0 = q, q_1[i] = comp(q[qlen - 1 - i]), comp(N) = N.
 * A diagonal (s, o, d) holds the cells i with 0 <= i < qlen and 0 <= i + d < len_s.  A cell matches iff q_o[i] is one of A C G T and
 * equals P_s[i + d]; N never matches, on either side.
 * A run is a maximal stretch of consecutive matching cells of one diagonal.  A diagonal is seeded when it has a run of at least `seed`
 * cells.  n_seeds = the runs of at least `seed` cells over all diagonals of all sequences in both orientations (saturating at
 * 2^32 - 1).  found = 1 iff n_seeds > 0; otherwise the row is all zeros but seq = seq2 = -1.
 * Best segment, over the seeded diagonals only: a segment (i0, n), n >= 1, of a diagonal scores matches - 2 * mismatches, every
 * cell that does not match being a mismatch: the rule of bk_locus_similarity, and its one pass, a running sum of +1 / -2 that
 * restarts wherever it is <= 0, every matching cell offering (sum, length since the restart).  The winner has the largest key
 * (score, -n, -s, -o, -(i0 + d), -i0): the highest score, then the shortest, the smallest sequence index, orientation 0, the smallest
 * start on the panel, the smallest i0.  Reported of it: seq = s, orient = o, score, len = n, mism = (len - score) / 3,
 * s_start = i0 + d (0-based and forward on the panel sequence in both orientations), q_start = the segment's first base in q (i0 for
 * orientation 0, qlen - i0 - n for orientation 1).
 * run = the longest run on any seeded diagonal.  score2 = the best segment score over the seeded diagonals of sequences other than
 * seq, seq2 = the smallest such index that reaches it; 0 and -1 without one.  score2 is what tells "AluYa5 or AluYb8" from "HPV16
 * and nothing else".
 * Hand examples, seed 12, checked with the brute force of tests/seqmatchcases.py.  Panel:
 *   0  GGCCGGGCGCGGTGGCTCACGCCTGTAATCCCAGCA
 *   1  TTGACCATGGCTAGCATCGGATTACAGGCGTGAGCCACCAAAAAAAAAAAA
 *   2  GGCCGGGCGCGGTGGCTCATGCCTGTAAT
 *   TTTTTTTTTGGTGGCTCACGCCTGTAATCC  -> seq 1, orient 1, score 30, len 30, mism 0, run 30, q_start 0, s_start 18, n_seeds 2, seq2 0,
 *                                      score2 21 (sequence 2 has one mismatch that leaves two runs of 9 and is never seeded)
 *   GGTGGCTCACGC                    -> seq 0 by the index tie, s_start 10, score 12, n_seeds 2, seq2 1, score2 12
 *   GGTGGCTCACG                     -> not found
 *   A x 15 against the one sequence C + A x 20 + G -> score 15, s_start 1, n_seeds 12: six full diagonals and runs of 14, 13 and 12
 *                                      at either end
 * Cost: nothing is capped.  A k-mer that occurs R times in the panel costs R per query k-mer that equals it, so a poly-A panel makes
 * a poly-A query expensive; a panel of consensus sequences with tails of 10 to 30 A is the intended use.
 * Every output is a count or an argmax with a fixed tie rule: two runs, and any permutation of the probes, give the same bytes row for
 * row.  The structs have no typedef. */
struct bk_seq_hit { uint32_t found; int32_t seq; uint32_t orient, score, len, mism, run, q_start, s_start, n_seeds; int32_t seq2; uint32_t score2; };  /* 48 bytes */
/* ctx: any live context that is not a shard (bk_shard_*); it gives the device, the stream, the buffers and bk_timing: scope
 * `sequence_match` with `sequence_match_index` and `sequence_match_probes` inside it.  bk_timing_touched, with B = off[n_seqs],
 * M = the k-mers of the panel (positions p whose `seed` bases hold no N and end inside p's sequence) and
 * passes = (2 * seed + 7) / 8:
 *   sequence_match_index   B + 36 * M * passes   the panel bytes; a radix pass reads a key for the histogram, reads and writes key and
 *                                                value for the scatter and is credited 36 bytes an item as everywhere in the library
 *   sequence_match_probes  n * (56 + max_len)    the probe row, the query and the result row
 *   sequence_match         the sum of the two
 * The panel reads of the extension are not modelled.  No stage needs to have run and nothing a later bk_fetch or stage returns
 * changes.  panel, probes, query: host memory.  *out (n rows) is library-owned until the next call or bk_free(ctx).  BK_ERR_ARG
 * (with the reason in bk_last_error) for shards, null ctx / panel / out, null probes or query with n > 0, max_len outside 1..256,
 * seed outside 8..16, qlen > max_len, reversed > 1, a query byte outside ACGTN within qlen, a panel byte outside ACGTN, null off with
 * n_seqs > 0, null bases with B > 0, and off that does not ascend from 0.  BK_ERR_LIMIT beyond 2^30 probes, 2^20 sequences or 2^28
 * panel bases, looked at before any other entry of an array is read.  No errors: n == 0, n_seqs == 0 (off and bases may then be
 * NULL), sequences shorter than seed, empty sequences. */
int bk_sequence_match(bk_ctx *ctx, const bk_seq_panel *panel, const struct bk_seq_probe *probes, uint64_t n, const uint8_t *query, uint32_t max_len, uint32_t seed,
                      const struct bk_seq_hit **out);

/* ---- site complexity: what the reference looks like at one position ---------------------------------------------------------------
 * Aligners clip and split reads in microsatellites, low-complexity stretches and annotated repeats for reasons that have nothing to do
 * with a rearrangement.  bk_site_complexity describes the reference window around one position by itself: how much of it is
 * soft-masked (bit 3 of the nibble, which nothing else reads), its trinucleotide counts (the DUST score of the window) and its exact
 * tandem tracts.  It reads nothing but the reference (bk_refseq as above).  All arithmetic is integer.
 * Site k: (tid, pos), pos 1-based.  R = flank, L = 2 R + 1.  Column i, 0 <= i < L, is position pos - R + i of contig tid, and nib[i]
 * the raw nibble there when a segment of `ref` holds the position.  Column i is
 *   covered  when a segment holds the position (never before position 1, outside every segment, or on tid < 0),
 *   masked   when covered and nib[i] & 8,
 *   valid    when covered and (nib[i] & 4) == 0; its base is then w[i] in A C G T = 0 1 2 3 (nib T C A G = 0 1 2 3 -> 3 1 0 2).
 * Counts: covered, valid, masked are the numbers of such columns; gc the valid columns with C or G.  mask_run is the length of the
 * maximal run of consecutive masked columns that contains column R, 0 when column R is not masked; a run that reaches an end of the
 * window is a lower bound of the interval's length.
 * Trinucleotides: column i <= L - 3 starts triplet t = 16 w[i] + 4 w[i + 1] + w[i + 2] when i, i + 1 and i + 2 are all valid; c_t is
 * the count of triplet t.  tri_total = sum c_t, tri_pairs = sum c_t (c_t - 1) / 2, tri_distinct = the number of t with c_t > 0.
 * sdust's score of the whole window is tri_pairs / (tri_total - 1).
 * Tandem tracts: for a period p, 1 <= p <= max_period and p < L, m_p[i] = 1 for 0 <= i < L - p when columns i and i + p are both
 * valid and w[i] == w[i + p].  A maximal run of n >= p consecutive ones of m_p that starts at i0 (two full copies at least) is a
 * tract of period p, start i0 and length n + p: it covers the columns i0 .. i0 + n + p - 1.  Tracts are exact; one N or one mismatch
 * ends a tract.  They are ordered by the key (-length, period, start): the longest first, then the shortest period, then the
 * smallest start, so that a homopolymer is reported with period 1 and not with 2 or 3.  max_period / max_len / max_start is the first
 * tract of the window in that order; bp_period / bp_len / bp_start the first tract whose columns intersect [R - 1, R + 1], the base
 * at `pos` and its two neighbours (a junction lies on one side of the base or the other).  All three fields are 0 without a tract.
 * By hand, R = 3 on GTACACA: w = 2 3 0 1 0 1 0.  m_2 = 0 0 1 1 1: one run of n = 3 >= 2 from i0 = 2, the tract (period 2, start 2,
 * length 5), columns 2 .. 6.  m_1 has no one and m_3 = 0 0 0 0, so max_* = bp_* = (2, 5, 2) (the tract holds column 2 = R - 1).  The
 * triplets are GTA TAC ACA CAC ACA: tri_total 5, tri_pairs 1 (ACA twice), tri_distinct 4; gc = 3.
 * Every output is an integer count or an argmax with a fixed tie rule: two runs, and any permutation of the sites, give the same bytes
 * row for row.  The structs have no typedef. */
struct bk_ref_site   { int32_t tid; uint32_t pos; };                       /* 8 bytes, pos 1-based */
struct bk_site_cplx  { uint32_t covered, valid, gc, masked, mask_run,
                       tri_total, tri_pairs, tri_distinct,
                       bp_period, bp_len, bp_start,
                       max_period, max_len, max_start, reserved[2]; };     /* 64 bytes, reserved = 0 */
/* ctx: any live context that is not a shard (bk_shard_*); it gives the device, the stream, the buffers and bk_timing (scope
 * `site_complexity`; bk_timing_touched is n * (72 + L): the site row, the result row and L nibbles).  No stage needs to have run and
 * nothing a later bk_fetch or stage returns changes.  ref, sites: host memory.  *out (n rows) is library-owned until the next call or
 * bk_free(ctx).  BK_ERR_ARG (with the reason in bk_last_error) for shards, null ctx / ref / out, null sites with n > 0, flank outside
 * 1..255, max_period outside 1..64, and every defect of the reference table that bk_junction_fit rejects.  BK_ERR_LIMIT beyond 2^30
 * sites or 2^20 segments, looked at before any array is read.  n == 0 is no error, and neither is n_segs == 0 (every row is then
 * zero).  A period at or above L has no tract and is no error. */
int bk_site_complexity(bk_ctx *ctx, const bk_refseq *ref, const struct bk_ref_site *sites, uint64_t n, uint32_t flank, uint32_t max_period, const struct bk_site_cplx **out);

/* ---- window coverage: the aligned bases inside arbitrary windows of the record table --------------------------------------------
 * Whether copy number changes at a breakpoint: the depth between the two breakpoints of a deletion drops, that of a tandem
 * duplication rises, an unbalanced translocation shows a step at one breakpoint only.  depth1 / depth2 are the count at the
 * breakpoint base itself and say nothing about either side of it.  bk_window_coverage answers any number of windows of any length,
 * each in time that does not depend on its length.  All arithmetic in signed 64-bit.
 * Record i of the `records` context is eligible when tid[i] >= 0, its flag has none of 0x4 0x100 0x200 0x400 0x800 (0x1 is not
 * required), mapq[i] >= mapq_min and its CIGAR has a reference length > 0 (M, D, N, =, X).  Its interval is [pos[i], bam_endpos(i)),
 * bam_endpos as in bk_exclude_regions and bk_ref_support: D and N count, soft clips do not, and a read with an SA tag counts like
 * any other.  For window k = (T, a, b), 0-based and half-open:
 *   bases  the sum over the eligible records on T of |[pos, bam_endpos) n [a, b)|
 *   reads  the number of eligible records on T for which that overlap is not empty
 * T < 0, T >= n_targets and b <= a give a zero row.  A window is not clamped against the contig length: no record lies beyond it.
 * With mapq_min = 0, on a table without supplementary records (0x800, which the reference's filter lets through), `bases` is the
 * `coverage` of the reference's cal_mean_depth (util_bed.cc:18-70) for the 1-based inclusive region [a + 1, b].
 * How: one streaming pass sums the eligible lengths of every tile of 256 records; an exclusive scan makes them prefixes S (lengths)
 * and C (records).  With h(x) = the first record of T with pos >= x, the records that start before x are a prefix of the table, and
 * only those within max_span (the longest alignment, from bk_isize_stats) of x can reach beyond it:
 *   bases = (S(h(b)) - over(b)) - (S(h(a)) - over(a)),  over(x) = the sum of bam_endpos - x over the eligible records with pos < x < bam_endpos
 *   reads = C(h(b)) - C(h(a)) + the number of eligible records with pos < a < bam_endpos
 * The tile sums depend on mapq_min and are rebuilt by every call.  Every output is an integer: two runs, and any permutation of the
 * windows, give the same bytes row for row.  The structs have no typedef. */
struct bk_cov_window { int32_t tid; uint32_t beg, end; uint32_t reserved; };   /* 16 bytes; 0-based, half-open; reserved = 0 */
struct bk_window_cov { uint64_t bases; uint32_t reads; uint32_t reserved; };   /* 16 bytes; reserved = 0 */
/* records: after bk_isize_stats (the stream pass gives max_span), not a shard (bk_shard_*).  windows: host memory.  *out (n rows) is
 * library-owned until the next call or bk_free(records).  BK_ERR_ARG (with the reason in bk_last_error) for a null out, null windows
 * with n > 0, wrong call order, shards, mapq_min < 0 and a window whose reserved is not 0; BK_ERR_LIMIT beyond 2^30 windows.  n == 0
 * and a table without records are no errors (every row is then zero).  It changes nothing a later bk_fetch or stage returns, and
 * works on every table form the context can hold (host upload, BK_MEM_DEVICE with and without `side`, the table bk_exclude_regions
 * left behind, where the excluded records simply do not count, the context of bk_bam_decode_device_ctx while its bk_bam_dev lives).
 * bk_timing: scope `window_coverage`, with `window_coverage_tiles` (the tile pass and its scans) and `window_coverage_windows` (the
 * window kernel) inside it.  bk_timing_touched of `window_coverage`: 11 bytes of every record (flag, mapq, tid, cigar_off) and its
 * CIGAR words, 16 bytes per tile, 32 bytes per window; the records the windows' edges visit are not modelled. */
int bk_window_coverage(bk_ctx *records, const struct bk_cov_window *windows, uint64_t n, int mapq_min, const struct bk_window_cov **out);
/* The windows of one call, a pure host function (no context, no GPU), so that every caller shares one rule.  Side s (0 = p1, 1 = p2)
 * has the exact 1-based breakpoint e = ps_exact and a direction right_s from bk_junction_sides (0 = LEFT, 1 = RIGHT).  Its cut is
 * k_s = e for a LEFT side and e - 1 for a RIGHT side, so the breakpoint base (0-based e - 1) always lies in the window on the
 * retained side.  out[2 s] = [k_s - flank, k_s) and out[2 s + 1] = [k_s, k_s + flank), both clamped to [0, target_len[ps_tid]); a
 * clamped window with end <= beg is written as (ps_tid, 0, 0).  out[4] = [min(k_1, k_2), max(k_1, k_2)), clamped likewise, when
 * p1_tid == p2_tid >= 0, and (-1, 0, 0) otherwise.  A negative tid gives (tid, 0, 0).  reserved = 0 everywhere.  target_len is the reference
 * list of bk_init (it must cover both tids).  Returns BK_OK, or BK_ERR_ARG for a null argument or flank == 0. */
int bk_call_windows(const bk_cluster *c, int right1, int right2, uint32_t flank, const uint32_t *target_len, struct bk_cov_window out[5]);

/* ---- window context: record classes and mapping quality of the records that start inside arbitrary windows ------------------------
 * What the alignments around a breakpoint looked like before any filter: every record-level call above applies its mapping-quality
 * and flag filter first and reports what survived.  A locus where a third of the reads have mapping quality 0 is a paralogue or a
 * repeat whatever its read support says; unmapped mates mark an insertion site.  bk_window_context answers any number of windows of
 * any length, each in time that does not depend on its length.  Every output is an integer.
 * Membership is by leftmost aligned position, NOT by overlap: record i belongs to window k = (T, a, b), 0-based and half-open, when
 * tid[i] == T and a <= pos[i] < b.  Adjacent half-open windows are therefore disjoint and their rows add: the row of [a, b) is the
 * sum of the rows of [a, m) and [m, b).  (bk_window_coverage counts aligned bases by overlap; this call counts records by start.)
 * Record i is mapped when tid[i] >= 0 and flag 0x4 is clear.  The base set: mapped records with none of 0x100 0x200 0x400 0x800.
 * 0x1 is not required and neither is a reference length, so a record with an empty CIGAR or with 100S is in it.  A row counts:
 *   reads     the base set
 *   mapq_sum  the sum of mapq over the base set, in 64 bits
 *   mq0       base set, mapq == 0
 *   lowq      base set, mapq < mapq_min: 0 for mapq_min == 0, and mq0 is among them otherwise
 *   clipped   base set, CIGAR not empty, and the first or the last operation is S after one leading and one trailing H have been
 *             skipped: H S ... and ... S H count, a hard clip alone does not, an S inside the CIGAR does not, H alone is not clipped
 *   improper  base set, 0x1 set, 0x8 clear, 0x2 clear
 *   orphan    base set, 0x1 and 0x8 set: reads whose mate is unmapped
 *   dup       mapped, 0x400 set, none of 0x100 0x200 0x800
 *   secsup    mapped, 0x100 or 0x800 set; 0x200 and 0x400 do not matter
 * A record with tid >= 0 and 0x4 set (an unmapped mate placed beside its partner) counts nowhere.  T < 0, T >= n_targets and
 * b <= a give a zero row.  A window is not clamped against the contig length: no record lies beyond it.
 * How: one streaming pass classifies every record and sums the nine counters of every tile of 256 records; exclusive scans in 64
 * bits make them prefixes.  With h(x) = the first record of T with pos >= x, the records in front of h(x) are a prefix of the table:
 * a counter's value there is the prefix of tile h / 256 plus the at most 255 records of that tile in front of h, classified by the
 * same function.  A row is the value at h(b) less the value at h(a).  No atomics anywhere: two runs, and any permutation of the
 * windows, give the same bytes row for row.  lowq depends on mapq_min, so the tile sums are rebuilt by every call.  The struct has
 * no typedef. */
struct bk_window_ctx { uint64_t mapq_sum; uint32_t reads, mq0, lowq, clipped, improper, orphan, dup, secsup; };   /* 40 bytes */
/* records: a context that holds a record table, not a shard (bk_shard_*); bk_isize_stats need not have run, because no record
 * reaches across an edge here.  windows: host memory, struct bk_cov_window as above.  *out (n rows) is library-owned until the next
 * call or bk_free(records).  BK_ERR_ARG (with the reason in bk_last_error) for a null out, null windows with n > 0, a context
 * without a table, shards, mapq_min < 0 and a window whose reserved is not 0; BK_ERR_LIMIT beyond 2^30 windows.  n == 0 and a table
 * without records are no errors (every row is then zero).  It changes nothing a later bk_fetch or stage returns, and works on every
 * table form bk_window_coverage does.
 * bk_timing: scope `window_context`, with `window_context_tiles` (the tile pass and its scans) and `window_context_windows` (the
 * window kernel) inside it.  bk_timing_touched of `window_context`: 19 bytes of every record (flag 2, mapq 1, tid 4, cigar_off 4,
 * and 8 for the first and the last CIGAR word), 40 bytes per tile (five 64-bit words: mapq_sum, and the eight counts two to a
 * word), 16 + 40 bytes per window; the partial tiles the windows' edges visit are not modelled. */
int bk_window_context(bk_ctx *records, const struct bk_cov_window *windows, uint64_t n, int mapq_min, const struct bk_window_ctx **out);

/* ---- fusion frame: the 5' and 3' partner and the reading frame of every call ------------------------------------------------------
 * Whether two breakpoints, each with the side on which sequence is retained, can give a fusion transcript at all, which transcript
 * is its 5' partner and whether the reading frame is kept.  A frame call is a property of a pair of isoforms, so every transcript
 * that overlaps side 1 is paired with every transcript that overlaps side 2.  All arithmetic is integer.
 * Model: bk_txmodel, host memory, uploaded per call as bk_refseq is.  Transcript i lies on contig tid[i] >= 0, covers
 * [tx_start[i], tx_end[i]) and runs on strand[i] (0 = '+', 1 = '-'); its coding parts (CDS n exons) are the entries
 * ex_off[i] .. ex_off[i + 1] - 1 of ex_start / ex_end.  Every coordinate is 0-based and half-open.  The parts of one transcript
 * ascend, none is empty (ex_start < ex_end), none overlaps the one before it (they may abut) and all lie inside
 * [tx_start, tx_end).  L(i), the coding length, is the sum of the parts' lengths; L = 0 (no part) is a non-coding transcript.
 * cds_start / cds_end are the first start and the last end of the parts.  The rows ascend by (tid, tx_start); ex_off ascends from
 * ex_off[0] = 0 to ex_off[n_tx] = n_parts.
 * Site k: side 1 (tid1, pos1, right1) and side 2 (tid2, pos2, right2), pos 1-based as p1_exact is, right 0 = LEFT and 1 = RIGHT as
 * everywhere else (bk_junction_sides).  Transcript T overlaps the side (tid, P) when T.tid == tid && T.tx_start < P && P <= T.tx_end;
 * a side with tid < 0 overlaps nothing.
 * Per transcript and side, with b = P - 1 the 0-based breakpoint base:
 *   retained  the bases b' <= b of a LEFT side, b' >= b of a RIGHT side (the breakpoint base is retained, as p_exact means)
 *   role      BK_FRAME_HEAD when (strand == '+') == (the side is LEFT): the retained part holds the transcript's 5' end and
 *             transcription runs towards the junction; BK_FRAME_TAIL otherwise
 *   r         the coding bases that are retained
 *   cod       r for a head (the coding bases it contributes), L - r for a tail (the coding bases lost in front of the junction)
 *   exon      counted over the coding parts in transcription order from 1 (part g of m in genomic order is g + 1 on '+' and m - g
 *             on '-'): for a head the last part that has a retained base, for a tail the first one; 0 when no part has one
 *   loc       of the base b: BK_LOC_NONCODING when L == 0; BK_LOC_CDS inside a part; BK_LOC_INTRON inside [cds_start, cds_end) but
 *             in no part; BK_LOC_5UTR / BK_LOC_3UTR in front of / behind the CDS in transcription order (b < cds_start is 5' on
 *             '+' and 3' on '-'; b >= cds_end the other way round).  An intron between two UTR exons counts as UTR.
 * Per pair (A overlaps side 1, B overlaps side 2; A and B may be the same transcript), the class is
 *   BK_FRAME_ANTISENSE (1)  the roles are equal: both promoters retained, or both lost
 *   otherwise, with H the head, T the tail, h = cod(H), t = cod(T):
 *   BK_FRAME_INFRAME (5)    0 < h < L(H), 0 < t < L(T) and h % 3 == t % 3
 *   BK_FRAME_OUTFRAME (4)   the same bounds, different remainders
 *   BK_FRAME_PROMOTER (3)   h == 0 && t == 0 && L(H) > 0 && L(T) > 0: a 5' UTR in front of the tail's whole CDS
 *   BK_FRAME_TRUNCATING (2) everything else (the head's stop codon retained, the tail's start lost behind a non-coding head, a
 *                           breakpoint in the tail's 3' UTR, a non-coding partner)
 * An intragenic deletion on a '+' gene (A == B) is in frame exactly when the coding bases it removes are a multiple of 3; that
 * needs no special case.
 * Per call: n_tx[s] = the transcripts that overlap side s + 1, and n_pairs = n_tx[0] * n_tx[1] (not stored).  n_inframe counts the
 * pairs of class 5, n_compatible those of classes 2..5, both over all pairs (they stop at 2^32 - 1).  The reported pair is the one
 * with the largest class; ties go to the larger L(A) + L(B), then the smaller model index of A, then of B.  cls is its class,
 * tx[] the model indices of A and B, and role / loc / exon / cod describe A on side 1 and B on side 2.  order is 1 when side 1 is
 * the head, 2 when side 2 is, 0 for BK_FRAME_ANTISENSE and BK_FRAME_NONE.  With n_tx[0] == 0 or n_tx[1] == 0 the class is
 * BK_FRAME_NONE (0); a side that has transcripts still reports the one with the largest L (the smallest index on a tie) with its
 * role / loc / exon / cod.  A side without a transcript has tx = -1 and role = loc = exon = cod = 0.  Every output is a count or
 * an argmax with a fixed tie rule: two runs, and any permutation of the sites, give the same bytes row for row.
 * Hand example (the G1 fixture): GENEA '+' with the parts [40500, 41000) [50000, 51000) [58000, 59500), side 1 = 50099 LEFT: a head,
 * r = cod = 500 + 99 = 599, CDS, exon 2.  GENEB '-' with the parts [70500, 71000) [80100, 89500), L = 9900, side 2 = 80200 RIGHT:
 * also a head, cod = 89500 - 80199 = 9301; the class is antisense.  GENEB on '+' instead is a tail with cod = 9900 - 9301 = 599,
 * CDS, exon 2, and the call is in frame (599 % 3 == 599 % 3), order 1. */
#define BK_FRAME_NONE 0
#define BK_FRAME_ANTISENSE 1
#define BK_FRAME_TRUNCATING 2
#define BK_FRAME_PROMOTER 3
#define BK_FRAME_OUTFRAME 4
#define BK_FRAME_INFRAME 5
#define BK_FRAME_HEAD 1 /* role; 0 = the side has no transcript */
#define BK_FRAME_TAIL 2
#define BK_LOC_NONCODING 1 /* loc; 0 = the side has no transcript */
#define BK_LOC_5UTR 2
#define BK_LOC_CDS 3
#define BK_LOC_INTRON 4
#define BK_LOC_3UTR 5
typedef struct bk_txmodel {
  uint64_t n_tx, n_parts;
  const int32_t *tid;
  const uint32_t *tx_start, *tx_end;
  const uint8_t *strand;        /* 0 = '+', 1 = '-' */
  const uint32_t *ex_off;       /* n_tx + 1 */
  const uint32_t *ex_start, *ex_end; /* n_parts each */
} bk_txmodel;
struct bk_frame_site { int32_t tid1; uint32_t pos1; int32_t tid2; uint32_t pos2; uint8_t right1, right2; uint8_t reserved[6]; };   /* 24 bytes */
struct bk_frame_call { uint8_t cls, order, loc[2], role[2]; uint16_t exon[2]; uint16_t reserved; int32_t tx[2]; uint32_t cod[2], n_tx[2], n_inframe, n_compatible; uint32_t reserved2; };   /* 48 bytes; reserved = 0 */
/* ctx: any live context that is not a shard (bk_shard_*); no stage needs to have run, and nothing a later bk_fetch or stage returns
 * changes.  model and sites: host memory.  *out (n rows) is library-owned until the next call or bk_free(ctx).  BK_ERR_ARG (with
 * the reason in bk_last_error) for a null model or out, null sites with n > 0, a shard, a right above 1, a model that lacks a
 * column, rows that do not ascend by (tid, tx_start), a negative tid, tx_end < tx_start, a strand above 1, an ex_off that does not
 * ascend from 0 to n_parts, and coding parts that are empty, descend, overlap or reach outside [tx_start, tx_end).  BK_ERR_LIMIT
 * beyond 2^24 transcripts or 2^28 parts (looked at before any array is read) and beyond 2^30 sites.  n == 0 is no error, and
 * neither is n_tx == 0 (every row is then BK_FRAME_NONE with tx = -1).  exon stops at 65535.
 * How: on upload the device derives the exclusive prefix of the coding lengths over all parts and, per contig, the running maximum
 * of tx_end.  One wavefront per site: per side a binary search for U = #{tx_start < P} on the contig, then a walk backwards from
 * U - 1, 64 transcripts a step, until the running maximum falls below P; r / exon / loc of an overlapping transcript by a binary
 * search over its parts; the pairs dealt to the lanes and one key reduced by shuffles.
 * bk_timing: scope `fusion_frame` (the work on the device copy: the derived arrays and the site kernel).  bk_timing_touched: 21
 * bytes per transcript (tid and tx_start as one key, tx_end, its running maximum, strand, ex_off) and 16 per part (start, end, the
 * prefix), each once, and 72 per site (its row and its result); the transcripts a site's walk visits are not modelled. */
int bk_fusion_frame(bk_ctx *ctx, const bk_txmodel *model, const struct bk_frame_site *sites, uint64_t n, const struct bk_frame_call **out);

/* ---- linked calls: reciprocal partners, duplicates and events of a list of calls -------------------------------------------------
 * How the calls of one list relate to each other: which one is the reciprocal junction of which (der(A) and der(B) of a balanced
 * translocation, the two ends of an inversion), which junction was called twice, and which calls share a breakpoint region and so
 * form one event.  All arithmetic is integer.
 * Site k: side 1 (tid1, pos1, right1) and side 2 (tid2, pos2, right2), pos 1-based as p1_exact is, right 0 = LEFT and 1 = RIGHT as
 * everywhere else (bk_junction_sides); the layout of bk_frame_site.  Sides are numbered s = 0, 1 below.
 *   near       A breakend is (tid, P, right).  Two breakends of different sites are near when tid == tid' >= 0 and |P - P'| <= D,
 *              D = max_dist, compared in 64 bits (P may be 1 or 0xFFFFFFFF).  A side with tid < 0 is near nothing.
 *   N          for sites i != j: N[s][t] = side s of i is near side t of j.
 *   mappings   straight holds when N[0][0] && N[1][1] and pairs (0,0) and (1,1); crossed holds when N[0][1] && N[1][0] and pairs
 *              (0,1) and (1,0).  A mapping that holds is same when both of its pairs have equal right, opposite when both have
 *              different right (one of each is neither).
 *   relation   of (i, j), symmetric, the first that applies:
 *                BK_LINK_DUPLICATE (1)   a mapping holds and is same: the junction was called twice
 *                BK_LINK_RECIPROCAL (2)  a mapping holds and is opposite: the two derivative junctions
 *                BK_LINK_ADJACENT (3)    any N[s][t] is set (both pairs near with mixed sides are here)
 *                BK_LINK_NONE (0)        otherwise
 * Per site i: n_dup, n_recip and n_adj count the other sites in each relation, each other site once however many of its breakends
 * are near.  dup_of is the smallest index among the duplicates, -1 without one.  mate is the reciprocal partner with the smallest
 * |off[0]| + |off[1]|, ties to the smaller index; when both mappings of one partner are opposite the smaller sum wins, then
 * straight; -1 without one.  off[s] is the partner's paired position minus P of side s, and mate_crossed is 1 for the crossed
 * mapping; all three are 0 without a mate.  For a LEFT side (the bases up to and including P are retained) an offset of +1 is a
 * blunt break, above +1 means off - 1 bases lost, 0 or below 1 - off bases duplicated; for a RIGHT side the signs mirror (-1 is
 * blunt).
 * Event: the graph whose edges are every relation other than none.  event is the smallest site index in the component of i and
 * event_size its number of sites; a site alone has event == i and event_size == 1.  A site whose own two sides are near each other
 * (a 300-base deletion with D = 1000) is not its own partner: only i != j counts.
 * Every output is a count or an argmin with a fixed tie rule: two runs give the same bytes, and a permutation of the sites gives
 * the same rows with the indices mapped.
 * Hand example (D = 1000): site 0 = (chr1 300000 LEFT, chr2 700000 RIGHT), site 1 = (chr1 300021 RIGHT, chr2 699990 LEFT): straight
 * holds and is opposite, RECIPROCAL; site 0 has mate = 1, off = {+21, -10}, event = 0, event_size = 2 without site 2.  Site 2 =
 * (chr2 700400 LEFT, chr3 5000 RIGHT) is ADJACENT to both, so with it the event has size 3. */
#define BK_LINK_NONE 0
#define BK_LINK_DUPLICATE 1
#define BK_LINK_RECIPROCAL 2
#define BK_LINK_ADJACENT 3
#define BK_LINK_MAX_DIST 1000000u
struct bk_link_site { int32_t tid1; uint32_t pos1; int32_t tid2; uint32_t pos2; uint8_t right1, right2; uint8_t reserved[6]; };   /* 24 bytes, as bk_frame_site */
struct bk_call_link { uint32_t n_dup, n_recip, n_adj; int32_t dup_of, mate; int32_t off[2]; uint32_t event, event_size; uint8_t mate_crossed; uint8_t reserved[3]; };   /* 40 bytes; reserved = 0 */
/* ctx: any live context that is not a shard (bk_shard_*); no stage needs to have run, and nothing a later bk_fetch or stage returns
 * changes.  sites: host memory.  *out (n rows) is library-owned until the next call or bk_free(ctx).  BK_ERR_ARG (with the reason
 * in bk_last_error) for a null out, null sites with n > 0, a shard, a right above 1 and max_dist above BK_LINK_MAX_DIST.
 * BK_ERR_LIMIT beyond 2^30 sites.  n == 0 is no error; max_dist == 0 means exact coincidence.
 * How: the breakends with tid >= 0 are sorted by ((tid + 1) << 32) | pos over the bits in use.  A run ends where the sorted gap
 * exceeds D or the contig changes; two breakends are joined by near-steps exactly when they lie in one run, so the events are
 * the components of the graph whose vertices are runs and whose edges are the sites.  One wavefront per site searches, per side,
 * the first key >= (tid, P - D) and deals the breakends up to (tid, P + D) to its lanes 64 a step; a hit on site j computes the
 * whole N of (i, j) from the two rows and counts j only when the hit is the first set entry of N in the order (0,0) (0,1) (1,0)
 * (1,1).  A locus with k sites inside one window therefore costs k * k for those sites; nothing is capped.  The components are
 * min-label propagation with pointer jumping over the runs; the host reads a changed flag between rounds, and more than n + 1
 * rounds give BK_ERR_LIMIT (they cannot be needed: a label travels at least one site a round).
 * bk_timing: scope `link_calls` (the work on the device copy).  bk_timing_touched: 64 bytes per site (its row and its result) and,
 * per breakend with tid >= 0 (m of them), 24 (its key and value written, its run id, its run's label and the event's two
 * counters) + 24 per radix pass (key and value read and written), passes = ceil((32 + bits(max tid + 1)) / 8), bits(x) the
 * position of the highest set bit of x from 1; the rows a site reads of its neighbours and the component rounds are not modelled. */
int bk_link_calls(bk_ctx *ctx, const struct bk_link_site *sites, uint64_t n, uint32_t max_dist, const struct bk_call_link **out);

/* ---- partner loci: where the discordant pairs at a locus point to -------------------------------------------------------------------
 * A call reports the pairs that agree with each other (N_DRP).  The same window may hold hundreds of ends whose mates scatter over
 * many other places: the signature of a repeat, a collapsed duplication or an aligner's dumping ground.
 * All arithmetic is signed 64-bit.
 * The ends of a context are the 2 P sides of the P rows of its BK_STAGE_SCAN table.  Pair i gives two ends: end 2 i has own locus
 * (p1_tid, p1_pos) and mate locus (p2_tid, p2_pos); end 2 i + 1 is the same pair the other way round.  Positions are the table's own
 * (1-based).  For a site (T, a, b | MT, ma, mb) = (tid, beg, end | mtid, mbeg, mend):
 *   ends        the number of ends with own tid == T and a <= pos <= b.
 *   to_partner  the number of those whose mate has tid == MT and ma <= mpos <= mb.  MT < 0 or mb < ma means no end goes to the
 *               partner.
 *   elsewhere   the other ends.  Sort their mates ascending by (mtid, mpos); tid -1 sorts first.  A locus is a maximal run in which
 *               neighbours have equal mtid and mpos differing by at most max_gap.  loci is the number of runs.  top_* describes the
 *               run with the most ends; a tie goes to the first in sorted order.  top_n is its ends; top_tid, top_beg, top_end are
 *               its contig and its smallest and largest mpos.  With no end elsewhere: loci = top_n = 0, top_tid = -1, top_beg =
 *               top_end = 0; top_n == 0 is the "none" signal.
 * T < 0, T >= n_targets and b < a give a zero row with top_tid = -1.  An end elsewhere whose mate lies inside the site's own window
 * is a locus like any other: it is a local event, and worth seeing.  reserved = 0 everywhere.
 * Hand example: chr1 = 0, chr2 = 1, chr3 = 2, and ten pairs (p1 -> p2): five chr1:1000, 1010, 1020, 1030, 1040 -> chr2:5000, 5010,
 * 5020, 5030, 5040; three chr1:1100, 1110, 1120 -> chr3:9000, 9100, 9500; one chr1:1200 -> chr1:80000; one chr1:900 -> chr2:5600.
 * The site (0, 800, 1300 | 1, 4800, 5300) has ends = 10 and to_partner = 5.  With max_gap = 200 and 399 it has loci = 4 (chr1:80000,
 * chr2:5600, chr3:9000-9100, chr3:9500) and top = chr3:9000-9100 with top_n = 2; with max_gap = 400 it has loci = 3 and top =
 * chr3:9000-9500 with top_n = 3.  The mirror site (1, 4800, 5300 | 0, 800, 1300) has ends = 5, to_partner = 5, loci = 0, top_n = 0.
 * Every output is a count or an argmax with a fixed tie rule: two runs, and any permutation of the sites, give the same bytes row for
 * row.  The structs have no typedef. */
struct bk_partner_site { int32_t tid; uint32_t beg, end; int32_t mtid; uint32_t mbeg, mend; uint32_t reserved[2]; };   /* 32 bytes; 1-based, inclusive; reserved = 0 */
struct bk_locus_partners { uint32_t ends, to_partner, loci, top_n; int32_t top_tid; uint32_t top_beg, top_end, reserved; }; /* 32 bytes */
/* ctx: after bk_discordant_pairs and not a shard (bk_shard_*); any later stage may have run.  sites: host memory.  *out (n rows) is
 * library-owned until the next call or bk_free(ctx).  BK_ERR_ARG (with the reason in bk_last_error) for a null out, null sites with
 * n > 0, wrong call order, shards and a site whose reserved is not 0.  BK_ERR_LIMIT beyond 2^30 sites, or when the elsewhere ends of
 * all sites together exceed what the radix sort takes (2^32 - 16 rows).  n == 0 and a context without pairs are no errors.  It
 * changes nothing a later bk_fetch or stage returns, and works on every table form the context can hold (host upload, BK_MEM_DEVICE
 * with and without `side`, the table bk_exclude_regions left behind, the context of bk_bam_decode_device_ctx while its bk_bam_dev
 * lives): it reads the pair table alone.
 * How: the ends are sorted by ((tid + 1) << 32) | pos over the bits in use, 32 + bits(n_targets + 1), and the mates' keys gathered
 * into that order; the index is rebuilt by every call.  One wavefront per site finds its range [lo, hi) with two wave-wide lower
 * bounds and tests the mates 64 per ballot.  An exclusive scan of the elsewhere counts gives every site a segment of rows; the host
 * reads their total once.  One wavefront per site writes its elsewhere mates' keys there (a row's slot is the matches in front of
 * it: no atomic), the rows are sorted stably by the mate key's bits and then by the site's, and one wavefront per site walks its
 * sorted segment 64 rows a step for the runs.
 * bk_timing: scope `locus_partners` (the work on the device copy), with `locus_partners_index` and `locus_partners_sites` inside it.
 * bk_timing_touched of `locus_partners`: 56 bytes per pair row read and 12 bytes per end of the index (its key and its value), which
 * is `locus_partners_index`; 64 bytes per site (its row and its result) and 12 bytes per elsewhere row (its key and its value) per
 * sort pass, passes = ceil((32 + bits(n_targets + 1)) / 8) + ceil(bits(n - 1) / 8), bits(x) the position of the highest set bit of x
 * from 1, which is `locus_partners_sites`.  The passes of the index's own sort and the ends the sites read are not modelled. */
int bk_locus_partners(bk_ctx *ctx, const struct bk_partner_site *sites, uint64_t n, uint32_t max_gap, const struct bk_locus_partners **out);
/* The two sites of one call, a pure host function (no context, no GPU), so that every caller shares one rule.  With W = (int) w, side
 * s (0 = p1, 1 = p2) of a cluster has the own window [max(1, ps_min - W), ps_max + W] on ps_tid, the call's window as
 * bk_normal_support defines it, and the other side's window as its partner window.  out[s] is side s; a bound above 0xFFFFFFFF is
 * written as 0xFFFFFFFF and a window whose upper bound lies below its lower one as (1, 0).  Returns BK_OK, or BK_ERR_ARG for a null
 * argument. */
int bk_call_partner_sites(const bk_cluster *c, double w, struct bk_partner_site out[2]);   /* pure host function */

/* ---- fragment sizes: the fragment lengths the member pairs imply across each junction ------------------------------------------------
 * A pair supports a junction physically when the fragment, read through the junction, has a length the library could have produced:
 * the bases from read 1 to breakpoint 1 plus the bases from breakpoint 2 to read 2.  All arithmetic is signed 64-bit.
 * n must equal the number of BK_STAGE_CLUSTERS rows; site c belongs to call c.  A site with skip != 0 gives an all-zero row.  Otherwise
 * the rows of call c are its BK_EV_PAIR rows of bk_evidence, same membership and order, voted or not: the call works for any cluster
 * row a caller has positions for.  For one such row take (T_s, P_s, F_s) = (tid_s, pos_s, flag_s) for side s = 1, 2 and H = its qhash.
 *   off       the row is off when ((F_s & 0x10) != 0) != (right_s != 0) on either side: the read does not lie on the side of the
 *             breakpoint that the site keeps.  An off row is never looked up.
 *   lookup    R_s = the smallest index i of the context's record table with tid[i] == T_s, pos[i] == P_s - 1, flag[i] == F_s and
 *             qhash[i] == H (the qhash from the bk_side row where the table has them).  The mate join builds both sides from records
 *             of this table, so R_s exists; a row without one is lost and counted, never guessed.
 *   end       E_s = bam_endpos of R_s: pos + the reference length of its M, D, N, =, X operations, pos + 1 without a CIGAR (or with
 *             flag 0x4, as htslib has it).  Read as a 1-based coordinate it is the last aligned base.
 *   retained  the breakpoint base is retained on both kinds of side, as -consensus and -link read it:
 *             right_s == 0: a_s = site.pos_s - P_s + 1;   otherwise: a_s = E_s - site.pos_s + 1.
 *   length    L = a_1 + a_2, clamped to [-2^31 + 1, 2^31 - 1].  a_s may be negative when a read lies beyond the breakpoint; it is taken
 *             as it is.
 * Per call, over the used rows (neither off nor lost): n_used; n_short counts L < lo and n_long counts L > hi; min and max (both 0
 * without a used row); sum; abs_dev = the sum of |L - centre| with centre = floor((2 sum + n_used) / (2 n_used)), the floor towards
 * minus infinity.  n_used + n_off + n_lost equals the call's pair rows.
 * Limit: positions are aligned coordinates, so soft-clipped bases are not added back (as for bk_unique_support): a clipped read's
 * fragment reads short by its clip on the outer end.
 * Hand example: a library of mean 350 and sd 40 (bk_fragment_bounds: lo = 230, hi = 470); the site (pos1 = 10000, right1 = 0 | pos2 =
 * 50000, right2 = 1); four pairs whose read 1 is forward and starts at 9801, 9851, 9901, 9951.  Their mates: reverse at 50101 with
 * 100M (E = 50200); reverse at 50051 with 50M10D50M (E = 50160); reverse at 49991 with 40S60M (E = 50050); forward at 50201.  The
 * lengths are 200 + 201 = 401, 150 + 161 = 311 and 100 + 51 = 151; the fourth row is off.  So n_used = 3, n_off = 1, n_short = 1,
 * n_long = 0, min = 151, max = 401, sum = 863, centre = floor(1729 / 6) = 288, abs_dev = 113 + 23 + 137 = 273.
 * Every output is a count, an extreme or an integer sum: two runs give the same bytes.  The structs have no typedef. */
struct bk_frag_site  { uint32_t pos1, pos2; uint8_t right1, right2, skip; uint8_t reserved[5]; };   /* 16 bytes; pos 1-based; reserved = 0 */
struct bk_frag_sizes { uint32_t n_used, n_off, n_lost, n_short, n_long; int32_t min, max; uint32_t reserved; int64_t sum; uint64_t abs_dev; };  /* 48 bytes */
/* ctx, call order, table forms, shards and lifetime: as for bk_unique_support.  It runs after bk_split_breakpoints, needs no earlier
 * bk_evidence call, and leaves bk_evidence's buffers and every later bk_fetch unchanged.  sites: host memory.  *out (n rows) is
 * library-owned until the next bk_fragment_sizes or bk_free(ctx).  BK_ERR_ARG (with the reason in bk_last_error) for null arguments
 * (sites may be null when n == 0), n != the cluster count, lo > hi, a non-zero reserved, right* or skip above 1, shards and wrong
 * call order.  A context without clusters with n == 0 is no error.
 * How: the pair rows are listed per call as bk_unique_support lists them (the split rows are left out); one lane per (row, side)
 * finds the side's first record of equal (tid, pos) by a binary search over the sampled keys of every 1024th record and then the
 * stride, and walks the records of that position for flag and hash, 8 on its own, the rest by its whole wavefront 64 a step; one
 * wavefront per call reduces its rows in two passes.
 * bk_timing: scope `fragment_sizes`.  bk_timing_touched: per member pair what bk_evidence's listing reads and sorts; per pair row its
 * 48-byte row written and read and its 8-byte length written and read twice (120 bytes); per looked-up record ten probes of tid and
 * pos in its stride (80 bytes), per record its walk reads tid, pos, flag and hash (18 bytes), and per used side its two CIGAR offsets
 * (8 bytes); per site its 16 bytes, its two offsets and its 48-byte row (80 bytes).  The probes of the sampled keys (cache
 * resident) and the CIGAR words are not modelled. */
int bk_fragment_sizes(bk_ctx *ctx, const struct bk_frag_site *sites, uint64_t n, int32_t lo, int32_t hi, const struct bk_frag_sizes **out);
/* The library's bounds, a pure host function (no context, no GPU): lo = max(0, floor(mean - 3 sd)), hi = ceil(mean + 3 sd), both
 * clamped to int32.  Returns BK_OK, or BK_ERR_ARG for a null pointer, a non-finite value or sd < 0. */
int bk_fragment_bounds(double mean, double sd, int32_t *lo, int32_t *hi);   /* pure host function */

/* ---- known junctions: every call of a list against a panel of pairs of intervals (BEDPE) ------------------------------------------
 * What is already known about a junction: in how many entries of a panel of normals it was seen, or which entry of a catalogue of
 * known fusions it is.  Both are lists of pairs of genomic intervals.  All arithmetic is integer.
 * Site: breakend s = 0, 1 is (tid_s, P_s, right_s), P 1-based as p1_exact is, x = P - 1; the layout of bk_frame_site.  Entry:
 * interval k = 0, 1 is (tid, [beg, end)), 0-based and half-open as in BED, then a name id, a score and two strands.
 *   dist       dist(x, [b, e)) is 0 when b <= x < e, b - x below the interval and x - (e - 1) at or above end, compared in 64 bits
 *              (P may be 1 or 0xFFFFFFFF, beg may be 0).  A breakend falls into an interval when the tids are equal and >= 0 and
 *              dist <= slop.
 *   mappings   straight holds when breakend 0 falls into interval 0 and breakend 1 into interval 1; crossed holds when 0 falls into
 *              1 and 1 into 0.  A mapping's dist is the sum of its two distances.
 *   agree      a mapping agrees when the entry states both strands and each stated strand equals the side of the breakend paired
 *              with it (BK_STRAND_LEFT for right == 0, BK_STRAND_RIGHT for right == 1); it opposes when both strands are stated and
 *              it does not agree.  An entry with one strand stated counts as unstated.
 *   hit        an entry is a hit of the site when a mapping holds, once even when both hold.  The hit's mapping is the first by:
 *              agrees, then the smaller dist, then straight.
 * Per site: n_hits; n_oriented and n_opposed from the hit's mapping; n_names, the distinct `name` values among the hits;
 * n_side[s], the entries with at least one interval that breakend s falls into, whatever the other breakend does, each entry once.
 * best is the hit with the largest score (BK_KNOWN_NO_SCORE sorts below every score), ties to the smaller dist, then to the smaller
 * entry index; best_score, best_dist, best_crossed and best_oriented (1 when its mapping agrees) describe it.  Without a hit
 * best = -1, best_score = BK_KNOWN_NO_SCORE and the rest is 0.
 * Every output is a count or an argmax with a fixed tie rule: two runs give the same bytes, and a permutation of the sites permutes
 * the rows.
 * Hand example (chr1 = 0, chr2 = 1, slop 100; site = chr1 300000 LEFT, chr2 700000 RIGHT, so x = 299999 and 699999):
 *   e0 = chr1 [299950,300050) / chr2 [699900,700100), name 0, score 12, + -   straight holds and agrees, dist 0
 *   e1 = chr2 [700050,700060) / chr1 [299000,299990), name 1, score 40, - +   crossed holds with distances 51 and 10, and agrees
 *   e2 = chr1 [299990,300010) / chr1 [100,200), name 0                        no hit (breakend 0 alone)
 *   e3 = chr2 [699000,701000) / chr2 [699500,700500), name 2                  no hit (breakend 1 alone, through both intervals)
 *   row: n_hits 2, n_oriented 2, n_opposed 0, n_names 2, n_side {3, 3}, best 1, best_score 40, best_dist 61, best_crossed 1,
 *   best_oriented 1. */
#define BK_KNOWN_MAX_SLOP 1000000u
#define BK_KNOWN_NO_SCORE INT32_MIN
#define BK_STRAND_NONE 0   /* unstated */
#define BK_STRAND_LEFT 1   /* '+': the bases up to the breakpoint are retained (right == 0) */
#define BK_STRAND_RIGHT 2  /* '-': right == 1 */
struct bk_known_entry { int32_t tid1; uint32_t beg1, end1; int32_t tid2; uint32_t beg2, end2; uint32_t name; int32_t score; uint8_t strand1, strand2; uint8_t reserved[6]; };   /* 40 bytes */
struct bk_known_site  { int32_t tid1; uint32_t pos1; int32_t tid2; uint32_t pos2; uint8_t right1, right2; uint8_t reserved[6]; };   /* 24 bytes, as bk_frame_site */
struct bk_known_call  { uint32_t n_hits, n_oriented, n_opposed, n_names, n_side[2]; int32_t best, best_score; uint32_t best_dist; uint8_t best_crossed, best_oriented; uint8_t reserved[2]; };   /* 40 bytes; reserved = 0 */
/* ctx: any live context that is not a shard (bk_shard_*); no stage needs to have run, and nothing a later bk_fetch or stage returns
 * changes.  entries, sites: host memory.  *out (n rows) is library-owned until the next call or bk_free(ctx).  BK_ERR_ARG (with the
 * reason and the index in bk_last_error) for a null out, null sites with n > 0, null entries with n_entries > 0, a shard, slop
 * above BK_KNOWN_MAX_SLOP, a right above 1, a strand above 2, a non-zero reserved byte of a site or an entry, and an interval with
 * tid >= 0 and end <= beg.  BK_ERR_LIMIT beyond 2^30 sites, 2^30 entries or 2^32 - 16 listed hits (the sum of n_hits).  n == 0 and
 * n_entries == 0 are no errors; with no entries every row is the no-hit row.  An interval with tid < 0 holds nothing; its entry can
 * still count in n_side through its other interval.
 * How: the intervals with tid >= 0 (m of the 2 n_entries) are sorted by ((tid + 1) << 32) | beg over the bits in use, the value
 * being 2 * entry + k, and a running maximum of end is kept inside every contig's run.  One wavefront per site searches, per
 * breakend, the last key with beg <= x + slop and walks backwards 64 intervals a step while the running maximum still reaches
 * x - slop; each lane tests its own interval.  On a hold the lane reads the entry's row and computes the whole table of (breakend,
 * interval) from it.  An entry reached through both of its intervals is counted at the first of them that holds the breakend, in
 * the order (interval 0, interval 1); hits are found from breakend 0 only, n_side from both walks.  The counts and the best hit are
 * wave reductions.  For n_names the hits per site are scanned, a second walk lists (site << 32) | name at the site's offset, the
 * list is sorted over the name's and the site's bits in use, and one wavefront per site counts the run heads.  No atomics, and
 * nothing is capped: an entry that spans a whole contig makes every site on that contig walk that contig's whole run, because the
 * running maximum never drops below it.  The entries are uploaded and indexed per call; the buffers are the context's and are
 * reused when they are large enough.
 * bk_timing: scope `known_calls` (the work on the device copies) around `known_calls_index` and `known_calls_sites`.
 * bk_timing_touched, with bits(x) the position of the highest set bit of x from 1 (0 for 0):
 *   index  per entry 40 (its row) + 24 (two keys and values written) + 48 per radix pass (two keys and values read and written),
 *          passes = ceil((32 + bits(max tid + 1)) / 8), 0 without an interval with tid >= 0; per such interval 16 (its end
 *          gathered, its running maximum written)
 *   sites  per site 80 (its 24-byte row, its 40-byte result, its count and its offset); per listed hit 12 (its key and value
 *          written) + 24 per radix pass, passes = ceil(bits(max name) / 8) + ceil(bits(n - 1) / 8)
 *   known_calls is their sum.  The intervals and entries that a site's walks read are not modelled. */
int bk_known_calls(bk_ctx *ctx, const struct bk_known_entry *entries, uint64_t n_entries, const struct bk_known_site *sites, uint64_t n, uint32_t slop, const struct bk_known_call **out);

/* ---- split junctions: junction calls from the split-evidence tuples alone ------------------------------------------------------------
 * Every BK_STAGE_CLUSTERS row starts from a cluster of discordant pairs; a junction whose fragments are not discordant (a deletion
 * or duplication shorter than the library's spread, a small inversion) has no row however many split reads cross it.  This call
 * groups the tuples of BK_STAGE_SPLITS by the junction they state.  All arithmetic is integer, compared in signed 64-bit.
 *   ends        The own end of a tuple is sec_* when flags & 1, else prim_*; the other end is the remaining one.  An end's position is
 *               its *_bp; it is RIGHT (1) when *_bp == *_start, else LEFT (0), as for bk_junctions.  The own end's contig is the
 *               tuple's tid, the record's real contig, not the interned *_chr.  The other end's contig is its interned *_chr when
 *               0 <= chr < n_targets: the first header entry of that name.
 *   eligible    A tuple is eligible when !(flags & 2), tid >= 0, the other contig is a header id as above, both positions lie in
 *               1 .. target_len of their contig, the own record (row `rec` of the table, as bk_evidence.rec is) has neither 0x4 nor
 *               0x200 set and mapq >= mapq_min, and the two ends are not identical in (contig, pos, right).
 *   canonical   The two ends are ordered ascending by (contig, pos, right) and become end 1 and end 2; own_end (0 or 1) says which of
 *               them the own end became.
 *   exact       An exact junction is a maximal set of eligible tuples with equal (tid1, pos1, right1, tid2, pos2, right2).
 *   near        Two exact junctions are near when tid1, tid2, right1 and right2 are equal, |pos1 - pos1'| <= tol and
 *               |pos2 - pos2'| <= tol.
 *   call        A connected component of the exact junctions under near (single linkage; tol == 0 makes every exact junction a
 *               call).  Single linkage can chain: exact junctions each tol apart form one call however long the chain grows; lo / hi
 *               show its extent.
 *   reads       Read identity is qhash (64 bits) alone: n_reads counts the distinct qhash of a call's tuples.
 * Row: (tid1, pos1, right1, tid2, pos2, right2) is the representative, the call's exact junction with the most distinct reads
 * (top_reads of them), ties to the smallest in the order (tid1, tid2, right1, right2, pos1, pos2).  n_tuples and n_exact count the
 * call's tuples and exact junctions; lo1 .. hi2 are the extremes of pos1 and pos2 over its exact junctions; n_own[k] counts the tuples
 * with own_end == k and mapq_sum[k] adds their own records' mapq.  reserved = 0.
 *   call        -1 unless bk_split_breakpoints has run and the context has voted rows (flags bit 1).  Then the smallest voted
 *               BK_STAGE_CLUSTERS row that some exact junction of the call matches: straight, when tid1 == p1_tid, |pos1 - p1_exact|
 *               <= 2, tid2 == p2_tid and |pos2 - p2_exact| <= 2 (the +-2 of the vote), or crossed, when the same holds with p1 and p2
 *               exchanged.  Sides are not compared.  call_crossed = 0 when some exact junction matches that row straight, else 1 (0
 *               without a row).
 * Output: the calls with n_reads >= min_reads, ordered by their smallest exact junction in the order above.  Every output is a
 * count, a sum, an extreme or an argmax with a fixed tie rule: two runs give the same bytes, and a renaming of the reads that keeps
 * qhash equality gives the same rows.
 * Hand example (chr1 = 0, chr2 = 1, every flags 0, every mapq 60, tol 2, min_reads 1).  Reads a, b, c: own end chr1 5000 LEFT, other
 * end chr1 5250 RIGHT.  Read d, first alignment: own end chr1 5251 RIGHT, other end chr1 5001 LEFT (the own end becomes end 2); second
 * alignment: own end chr1 5001 LEFT, other end chr1 5251 RIGHT.  Read e: own end chr2 700 RIGHT, other end chr1 5000 LEFT.  The exact
 * junctions are (chr1 5000 L, chr1 5250 R) with 3 reads, (chr1 5001 L, chr1 5251 R) with 1 read in 2 tuples, and (chr1 5000 L,
 * chr2 700 R).  Row 0: 0 5000 0 5250, n_reads 4, n_tuples 5, n_exact 2, lo1 5000, hi1 5001, lo2 5250, hi2 5251, n_own {4, 1},
 * mapq_sum {240, 60}, call -1, right 0 1, top_reads 3.  Row 1: 0 5000 1 700, n_reads 1, n_tuples 1, n_exact 1, n_own {0, 1}, mapq_sum
 * {0, 60}, right 0 1, top_reads 1.  With tol 0 there are three rows; with min_reads 3 only row 0.
 * The struct has no typedef. */
#define BK_SJ_MAX_TOL 100u
struct bk_split_junction {
  int32_t tid1; uint32_t pos1; int32_t tid2; uint32_t pos2;   /* the representative exact junction */
  uint32_t n_reads, n_tuples, n_exact;   /* distinct qhash, tuples, exact junctions of the call */
  uint32_t lo1, hi1, lo2, hi2;           /* min / max of pos1 and pos2 over the call's exact junctions */
  uint32_t n_own[2];                     /* tuples whose own record carries end 1 / end 2 */
  uint32_t mapq_sum[2];                  /* sum of the own records' mapq, by own_end */
  int32_t call;                          /* BK_STAGE_CLUSTERS row that claims it, -1 without */
  uint8_t right1, right2, call_crossed, reserved;
  uint32_t top_reads;                    /* distinct reads of the representative */
};                                       /* 72 bytes */
/* ctx: after bk_split_evidence and not a shard (bk_shard_*); whether bk_split_breakpoints has run decides only `call`.  *out (*count
 * rows) is library-owned until the next call or bk_free(ctx).  BK_ERR_ARG (with the reason in bk_last_error) for wrong call order,
 * shards, null outputs, mapq_min < 0, tol > BK_SJ_MAX_TOL and min_reads == 0.  BK_ERR_LIMIT beyond 2^30 eligible tuples, and for a
 * reference list of more than 2^30 sequences (the group key holds two contig numbers and two sides in 64 bits).  A context
 * without tuples is no error: *count = 0.  It changes nothing a later bk_fetch or stage returns, and works on every table form the
 * context can hold (host upload, BK_MEM_DEVICE with and without `side`, the table bk_exclude_regions left behind, the context of
 * bk_bam_decode_device_ctx while its bk_bam_dev lives): of the records it reads flag and mapq alone.
 * How: one lane per tuple classifies it; a scan compacts the e eligible tuples into 32-byte canonical rows.  Three stable LSD stages
 * of the radix sort order them: by qhash (64 bits; run heads and a scan turn the hash into a dense rank), by (pos1, pos2) over
 * 2 * bits(longest contig) bits, by ((tid1 * n_targets + tid2) << 2 | right1 << 1 | right2) over its bits in use.  Run heads and
 * scans give the x exact junctions and their distinct reads; one wavefront per exact junction sums its tuples.  Components: one
 * wavefront per exact junction finds, by binary search, the first exact junction of its group with pos1' >= pos1 - tol and deals
 * the rows up to pos1 + tol to its lanes 64 a step, each lane testing pos2 and offering its row's label; the smallest becomes the
 * exact junction's own label and, by an integer atomic minimum, that of the exact junction it pointed to so far; pointer jumping
 * follows.  The host reads a changed flag between rounds; more than x + 1 rounds give
 * BK_ERR_LIMIT (they cannot be needed: a label travels at least one near-step a round).  Nothing is capped: a locus with k exact
 * junctions inside one window costs k * k for those, every round.  The exact junctions are then sorted by label and the tuples by
 * (label, read rank), which makes every call a contiguous range of both; one wavefront per call reduces them.  The claimed row: the
 * host sorts the voted rows' two orientations by ((tid + 1) << 32) | exact (they are few), one lane per exact junction searches
 * them.  A scan compacts the calls by min_reads.  No atomics on results: every result word has one writer; the labels alone take
 * atomic minima, whose outcome does not depend on the order.
 * bk_timing: scope `split_junctions`.  bk_timing_touched, with bits(x) the position of the highest set bit of x from 1 (0 for 0) and
 * a radix pass costing 36 bytes per item (key and value read by the histogram, read and written by the scatter): per tuple 96 (its
 * row, its flag written and scanned); per eligible tuple 123 (its row read again with the record's flag and mapq, the canonical row
 * written) + 36 * P1 + 132 (three key gathers) + 64 (the sorted copy) + 24 (heads, scans, ids) + 36 * P2 + 48 (the second key, its
 * heads and scans), P1 = 8 + ceil(2 * bits(longest contig) / 8) + ceil(bits(largest group key) / 8), P2 = ceil((bits(e) + bits(x))
 * / 8); per exact junction 80 (its row written and read) + 36 * ceil(bits(x) / 8) + 24; per call 84; per returned row 72.  The rows
 * the walks read and the rounds are not modelled. */
int bk_split_junctions(bk_ctx *ctx, int mapq_min, uint32_t tol, uint32_t min_reads, const struct bk_split_junction **out, uint64_t *count);
/* What the last bk_split_junctions of this context counted: out[0] tuples, [1] eligible tuples, [2] exact junctions, [3] calls before
 * min_reads, [4] returned calls that a voted row claims, [5] rounds of label propagation.  BK_ERR_ARG for a null argument. */
int bk_split_junction_counts(bk_ctx *ctx, uint64_t out[6]);
/* Test hook: bk_split_junctions with the claimed row looked up in `rows` (host memory, n_rows of them, any order of p1 and p2)
 * instead of the context's own table; bk_split_breakpoints need not have run.  A context's own rows put the lower (contig, position)
 * first, so only a caller's table reaches the crossed match.  Errors as bk_split_junctions, and BK_ERR_ARG for null rows with
 * n_rows > 0. */
int bk_debug_split_junctions(bk_ctx *ctx, int mapq_min, uint32_t tol, uint32_t min_reads, const bk_cluster *rows, uint64_t n_rows, const struct bk_split_junction **out,
                             uint64_t *count);

/* ---- CIGAR gaps: deletions and insertions the aligner wrote inside an alignment -------------------------------------------------------
 * An aligner writes a 30- to 100-base deletion in the middle of a read as 70M45D80M, not as a split read: such a record has no SA
 * tag, no soft clip and a proper pair, so no other call sees it.  This call walks the CIGAR of every record of the table and groups
 * the long D and I operations.  All arithmetic is integer.
 *   eligible    A record is eligible when tid >= 0, none of the flags 0x4 0x100 0x200 0x400 0x800 is set and mapq >= mapq_min.
 *   walk        p = pos (0-based) equals the 1-based coordinate of the last reference base consumed so far.  M = X add their length
 *               to p and to the matched count; D N add their length to p only; I S H P do not move p.
 *   event       An operation D (kind BK_GAP_DEL = 0) or I (kind BK_GAP_INS = 1) of length len >= min_len gives an event with start =
 *               p before the operation.  A deletion removes start + 1 .. start + len; its right end is start + len + 1.  An insertion
 *               lies between start and start + 1; its right end is start + 1.  N never gives an event: it is the aligner's statement
 *               of a splice.
 *   anchor      The M = X lengths of all operations in front of the event, and of all operations behind it, must each sum to at least
 *               `anchor`.  Other gaps in between do not reset the sums.
 *   beyond      An event whose right end exceeds the contig's length is dropped and counted as beyond.  (So is one with a start
 *               below 0, which needs pos < 0 on a mapped record, and every event of a tid at or above n_targets: neither is valid BAM.)
 *   read        A read is its qhash.  Two mates that both cross a gap are one read.
 *   exact       Equal (kind, tid, start, len) are one exact event.
 *   locus       A maximal run of exact events of one kind on one contig whose sorted starts differ by at most tol from one to the next.
 *   call        Within a locus, a maximal run of sorted lens that differ by at most tol from one to the next.
 * This is two one-dimensional single linkages, first on start, then on len inside the locus; both can chain, and the spans in the row
 * show the extent.  It is not the two-dimensional linkage of bk_split_junctions: two events 2 * tol apart in start with equal len are
 * one call when a third event of any other length bridges their starts.  Nothing is capped and nothing costs k * k.
 * Row: (tid, start, len, kind) is the representative, the call's exact event with the most distinct reads (top_reads of them), ties
 * to the smaller (start, len).  n_reads counts the distinct qhash of the call, n_rows its events (records x operations), n_exact its
 * exact events; lo_start .. hi_len are the extremes over its events; n_fwd / n_rev count the rows by flag 0x10 (one-strand support
 * is the classic gap artefact); mapq_sum adds the records' mapq over the rows.
 * Output: the calls with n_reads >= min_reads, ordered by (kind, tid, first start of the locus, lowest len of the call).  Every
 * output is a count, a sum, an extreme or an argmax with a fixed tie rule: two runs give the same bytes.
 * Hand example (one contig of 1 000 000 bases, mapq_min 20, min_len 20, anchor 10, tol 2, min_reads 1; pos 0-based; flag 0x10 = reverse):
 *   a, b, c   pos  999  70M45D80M    mapq 60            DEL start 1069 len 45 (removes 1070 .. 1114, right end 1115)
 *   d         pos 1000  70M46D79M    mapq 40, reverse   DEL start 1070 len 46
 *   d (mate)  pos 1039  30M45D120M   mapq 60            DEL start 1069 len 45
 *   e         pos 1059  10M30I110M   mapq 30            INS start 1069 len 30
 *   f         pos 1060  9M45D141M    mapq 60            none: 9 matched bases in front
 *   g         pos  999  70M45N80M    mapq 60            none: N
 * Counts: 8 records, 8 eligible, 6 events, 0 beyond, 3 exact, 2 loci, 2 calls, 2 written.  Row 0: tid 0 start 1069 len 45 kind 0,
 * n_reads 4, n_rows 5, n_exact 2, top_reads 4, lo_start 1069, hi_start 1070, lo_len 45, hi_len 46, n_fwd 4, n_rev 1, mapq_sum 280.
 * Row 1: tid 0 start 1069 len 30 kind 1, n_reads 1, n_rows 1, n_exact 1, top_reads 1, 1069 1069 30 30, n_fwd 1, n_rev 0, mapq_sum 30.
 * With tol 0 there are three calls; with min_reads 2 only row 0.
 * The struct has no typedef. */
#define BK_GAP_DEL 0u
#define BK_GAP_INS 1u
#define BK_GAP_MAX_TOL 100u
#define BK_GAP_MAX_LEN 1000000u
struct bk_cigar_gap {
  int32_t tid; uint32_t start; uint32_t len; uint32_t kind;   /* the representative exact event */
  uint32_t n_reads, n_rows, n_exact;     /* distinct qhash, events, exact events of the call */
  uint32_t top_reads;                    /* distinct reads of the representative */
  uint32_t lo_start, hi_start, lo_len, hi_len;   /* spans of the call */
  uint32_t n_fwd, n_rev;                 /* rows by flag 0x10 */
  uint64_t mapq_sum;                     /* over rows */
};                                       /* 64 bytes */
/* records: a context that holds a record table (host upload, BK_MEM_DEVICE with and without `side`, the table bk_exclude_regions
 * left behind - so excluded regions are honoured by themselves -, the context of bk_bam_decode_device_ctx while its bk_bam_dev
 * lives) and is not a shard (bk_shard_*); no stage need have run.  *out (*count rows) is library-owned until the next call or
 * bk_free.  BK_ERR_ARG (with the reason in bk_last_error) for null outputs, a sharded context, a context without a table, mapq_min
 * < 0, min_len, anchor or min_reads of 0, min_len > BK_GAP_MAX_LEN and tol > BK_GAP_MAX_TOL.  BK_ERR_LIMIT beyond 2^30 events.  A
 * table without events is no error: *count = 0.  It changes nothing a later bk_fetch or bk_run returns.
 * How: the record pass, one wavefront per tile of 256 records, four consecutive records a lane, cigar_off, flag and mapq read as
 * vectors; only a record whose flag and mapq pass and that has three or more operations (fewer cannot hold an anchored gap) has its
 * tid, pos and CIGAR words fetched, and one lane walks one CIGAR of any length.  Pass one sums the events per tile (it also reads
 * tid as a vector: the count of eligible records needs it and the table need not be sorted yet), a scan makes the sums offsets, pass
 * two walks the records of the tiles that hold an event again and writes the events in record order (32 bytes: qhash, start, len,
 * kind and contig, strand and mapq).  Then stable LSD stages of the radix sort by qhash (64 bits; run heads and a scan turn the hash
 * into a dense rank), by len (28 bits) and by (kind, tid, start) over 1 + bits(n_targets - 1) + bits(longest contig) bits; the
 * heads of the loci and a scan; one stage by (locus, len) over bits(loci) + 28 bits; the heads of the calls, of the exact events and
 * of the reads inside them, with their scans; one stage by (call, read rank), whose run heads are the distinct reads of a call; one
 * wavefront per call for its row; a scan compacts the calls by min_reads.  No atomic anywhere: every result word has one writer.
 * The host reads a count four times, where a buffer or a key must be sized: the events (with the eligible records and beyond), the
 * loci, the exact events with the calls, the returned rows.
 * bk_timing: scope `cigar_gaps`, and inside it `cigar_gaps_records` (the record pass) and `cigar_gaps_calls`.  bk_timing_touched,
 * with T = ceil(records / 256), bits(x) the position of the highest set bit of x from 1 (0 for 0) and a radix pass costing 36 bytes
 * per item: cigar_gaps_records = 11 * records (cigar_off, flag, mapq, tid) + 56 * T (the two tile words written, scanned and read)
 * + 1792 * min(events, T) (at most that many tiles are read again, 7 bytes a record) + 48 * events (tid, pos, qhash, the row);
 * cigar_gaps_calls = events * (36 * (P1 + P2 + P3) + 400) + 144 * calls + 128 * written, P1 = 8 + 4 + ceil((bits(longest contig) +
 * bits(n_targets - 1) + 1) / 8), P2 = ceil((bits(loci) + 28) / 8), P3 = ceil((bits(calls) + bits(events)) / 8); 400 = three key
 * gathers (132), the read ranks (24), two sorted copies (128), the loci (20), the three heads, scans and two start lists (60), the
 * read key with its heads and scan (36).  cigar_gaps is their sum.  The CIGAR words that the walks read are not modelled. */
int bk_cigar_gaps(bk_ctx *records, int mapq_min, uint32_t min_len, uint32_t anchor, uint32_t tol, uint32_t min_reads, const struct bk_cigar_gap **out, uint64_t *count);
/* What the last bk_cigar_gaps of this context counted: out[0] records, [1] eligible records, [2] events, [3] events beyond a contig's
 * end, [4] exact events, [5] loci, [6] calls before min_reads, [7] returned rows.  BK_ERR_ARG for a null argument. */
int bk_cigar_gap_counts(bk_ctx *records, uint64_t out[8]);

/* ---- soft-clip loci: pile-ups of clipped reads over the whole table ------------------------------------------------------------------
 * bk_clip_support counts clips inside the windows of the clusters and bk_clip_reads at sites the caller knows.  A breakpoint whose reads
 * are clipped without an SA tag and whose mates are unmapped or scattered (a mobile-element insertion, a viral integration site, novel
 * sequence) forms no cluster and is seen by neither.  This call groups the clip events of the whole table.  All arithmetic is integer.
 *   events      Which records are eligible and which events (tid, p, dir) a record has is exactly what bk_clip_support (above) defines,
 *               with the same mapq_min and min_clip; nothing of it is restated here.
 *   beyond      An event with p above the contig's length, or on a tid >= n_targets, is dropped and counted as beyond.  (So is one with
 *               p below 1, which needs pos < 0 on a mapped record: not valid BAM.)
 *   read        A read is its qhash.
 *   exact       Equal (dir, tid, p) are one exact site.
 *   locus       A maximal run of exact sites of one direction on one contig whose sorted p differ by at most tol from one to the next.
 * This is a single linkage, as in bk_cigar_gaps: it can chain, and the span in the row shows the extent.  Nothing is capped.
 * Row: (tid, pos, dir) is the representative, the locus's exact site with the most distinct reads (top_reads of them), ties to the
 * smaller p.  n_reads counts the distinct qhash of the locus, n_rows its events, n_exact its exact sites; lo_pos .. hi_pos is its span;
 * n_fwd / n_rev count the rows by flag 0x10; max_clip and clip_sum are over the lengths of the S ops that made the rows, mapq_sum adds
 * the records' mapq; n_orphan counts the rows with flags 0x1 and 0x8 (the mate is unmapped: the mark of inserted sequence), n_improper
 * those with 0x1 and neither 0x8 nor 0x2.
 *   facing      A LEFT locus with representative p and a RIGHT locus with representative q on one contig face each other when
 *               |q - p - 1| <= pair_dist; mate_off = q - p on both rows, read as bk_link_calls reads it: +1 is a blunt insertion point,
 *               more means bases lost, 0 or less means bases duplicated (a target-site duplication).  A locus's partner is the facing
 *               locus with the most n_reads, ties to the smaller |q - p - 1|, then to the smaller position.  flags bit 0 = the locus
 *               has a partner, bit 1 = the relation is mutual (each is the other's partner).  Facing is decided over all loci, before
 *               min_reads: mate is the partner's index among the returned rows, 0xFFFFFFFF when it is not returned; mate_pos and
 *               mate_reads (the partner's representative position and n_reads) and mate_off are filled whenever bit 0 is set, 0 otherwise.
 *   claim       With a `calls` context: the smallest voted row (flags bit 1) of its BK_STAGE_CLUSTERS with a side s such that ps_tid
 *               == tid and lo_pos - 2 <= ps_exact <= hi_pos + 2 (sides are not compared, as bk_split_junctions claims); 0xFFFFFFFF
 *               when there is none, and everywhere when calls is NULL.
 * Output: the loci with n_reads >= min_reads, ordered by (dir, tid, lo_pos).  Every output word is a count, a sum, an extreme or an
 * argmax with a fixed tie rule: two runs give the same bytes.
 * Hand example (one contig of 1 000 000 bases, mapq_min 20, min_clip 10, tol 2, pair_dist 50, min_reads 1; pos 0-based; proper pairs
 * unless said):
 *   a, b, c   pos  899  100M50S     mapq 60                    LEFT 999
 *   d         pos  900  101M49S     mapq 40, reverse           LEFT 1001
 *   e, f      pos  989  50S100M     mapq 60                    RIGHT 990
 *   g         pos  989  9S100M      mapq 60                    none: the clip is too short
 *   h         pos  989  50S100M     mapq 60, an SA tag         none: not eligible
 *   i         pos 5000  5H30S100M   mapq 60, flag 0x1 | 0x8    RIGHT 5001
 *   j         pos  899  100M50S     mapq 10                    none: not eligible
 * Counts: 10 records, 8 eligible, 7 events, 0 beyond, 4 exact, 3 loci, 2 with a mutual partner, 3 returned.  Row 0: tid 0 pos 999 LEFT,
 * n_reads 4, n_rows 4, n_exact 2, top_reads 3, lo_pos 999, hi_pos 1001, n_fwd 3, n_rev 1, max_clip 50, clip_sum 199, mapq_sum 220, mate 1,
 * mate_pos 990, mate_reads 2, mate_off -9 (ten bases duplicated), flags 3.  Row 1: tid 0 pos 990 RIGHT, n_reads 2, mate 0, mate_pos
 * 999, mate_reads 4, mate_off -9, flags 3.  Row 2: tid 0 pos 5001 RIGHT, n_reads 1, n_orphan 1, flags 0.
 * The struct has no typedef (bk_clip_site is the site of bk_clip_reads). */
#define BK_CLIP_LEFT 0u
#define BK_CLIP_RIGHT 1u
#define BK_CLIPLOCI_MAX_TOL 100u
#define BK_CLIPLOCI_MAX_PAIR 100000u
struct bk_clip_locus {
  int32_t tid; uint32_t pos; uint32_t dir;   /* the representative exact site; pos 1-based, dir 0 = LEFT, 1 = RIGHT */
  uint32_t flags;                        /* bit 0 has a facing locus, bit 1 the relation is mutual */
  uint32_t n_reads, n_rows, n_exact;     /* distinct qhash, events, exact sites of the locus */
  uint32_t top_reads;                    /* distinct reads of the representative */
  uint32_t lo_pos, hi_pos;               /* span of the locus */
  uint32_t n_fwd, n_rev;                 /* rows by flag 0x10 */
  uint32_t max_clip;                     /* the longest clip among the rows */
  uint32_t n_orphan;                     /* rows with 0x1 and 0x8 */
  uint64_t clip_sum, mapq_sum;           /* over rows */
  uint32_t n_improper;                   /* rows with 0x1 and neither 0x8 nor 0x2 */
  uint32_t claim;                        /* the claiming BK_STAGE_CLUSTERS row, 0xFFFFFFFF for none */
  uint32_t mate;                         /* the partner among the returned rows, 0xFFFFFFFF when it is not returned */
  uint32_t mate_pos, mate_reads;         /* the partner's representative position and distinct reads */
  int32_t mate_off;                      /* q - p */
};                                       /* 96 bytes */
/* records: a context that holds a record table (host upload, BK_MEM_DEVICE with and without `side`, the table bk_exclude_regions
 * left behind - so excluded regions are honoured by themselves -, the context of bk_bam_decode_device_ctx while its bk_bam_dev
 * lives) and is not a shard (bk_shard_*); no stage need have run on it.  calls: NULL, or a context (records itself, or another one on
 * the same device with an identical reference list) after bk_split_breakpoints, not a shard.  *out (*count rows) is library-owned until
 * the next call or bk_free(records).  BK_ERR_ARG (with the reason in bk_last_error) for null outputs, a sharded context, a context
 * without a table, mapq_min < 0, min_clip < 1, min_reads of 0, tol > BK_CLIPLOCI_MAX_TOL, pair_dist > BK_CLIPLOCI_MAX_PAIR, a calls
 * context before bk_split_breakpoints and differing reference lists.  BK_ERR_LIMIT beyond 2^30 events.  A table without events is no
 * error: *count = 0.  It changes nothing a later bk_fetch or bk_run returns.
 * How: the record pass, one wavefront per tile of 256 records, four consecutive records a lane, flag, mapq, cigar_off and aux_off read
 * as vectors; only a record whose flag, mapq and empty aux blob pass has its CIGAR words fetched (and its pos, when it has an event), and
 * the rule of bk_clip_support (one device function, shared with it) looks at its first and last words and walks the whole CIGAR only
 * where it does there; the count of eligible records reads on to the first word with a reference length, which is the first or second.  Pass one sums the events per tile (it also reads tid as a vector: the table need not be sorted), a scan makes the sums
 * offsets, pass two looks at the tiles that hold an event again and writes the events in record order (32 bytes: qhash, p, tid and
 * dir, the clip's length, flag bits and mapq).  Then stable LSD stages of the radix sort by qhash (64 bits; run heads and a scan turn
 * the hash into a dense rank) and by (dir, tid, p) over 1 + bits(n_targets - 1) + bits(longest contig) bits; the heads of the loci,
 * of the exact sites and of the reads inside them, with their scans; one stage by (locus, read rank), whose run heads are the distinct
 * reads of a locus; one wavefront per locus for its row.  The representatives ascend within a (dir, tid), so one wavefront per locus
 * searches the other direction's loci for the first one inside the facing window and walks the window 64 loci a step; a second kernel
 * sets the mutual bit.  The claim: the 2 x rows breakpoints of the calls are radix-sorted by (tid, pos) and one lane per locus walks
 * those inside its span.  A scan compacts the loci by min_reads and renumbers mate.  No atomic anywhere: every result word has one
 * writer.  The host reads a count three times, where a buffer or a key must be sized or a count is returned: the events (with the
 * eligible records and beyond), the exact sites with the loci, the mutual loci with the returned rows.
 * bk_timing: scope `clip_loci`, and inside it `clip_loci_records` (the record pass) and `clip_loci_calls`.  bk_timing_touched, with
 * T = ceil(records / 256), E = the events that are not beyond, bits(x) the position of the highest set bit of x from 1 (0 for 0) and a
 * radix pass costing 36 bytes per item: clip_loci_records = 15 * records (flag, mapq, cigar_off, aux_off, tid) + 56 * T (the two tile
 * words written, scanned and read) + 2816 * min(E, T) (at most that many tiles are read again, 11 bytes a record) + 48 * E (tid, pos,
 * qhash, the row); clip_loci_calls = E * (36 * (P1 + P2 + P3) + 376) + 176 * loci + 224 * returned + B * (36 * PB + 40), P1 = 8, P2 =
 * ceil((bits(longest contig) + bits(n_targets - 1) + 1) / 8), P3 = ceil((bits(loci) + bits(E)) / 8), B = 2 x the rows of the calls (0
 * without them), PB = ceil((33 + bits(n_targets - 1)) / 8); 376 = two key gathers (92), the read ranks (32), the sorted copy (68), the
 * three heads, scans and two start lists (76), the read key with its heads and scan (68), the rows' read of the sorted table (40).
 * clip_loci is their sum.  The CIGAR words and the searches are not modelled. */
int bk_clip_loci(bk_ctx *records, bk_ctx *calls, int mapq_min, int min_clip, uint32_t tol, uint32_t pair_dist, uint32_t min_reads, const struct bk_clip_locus **out,
                 uint64_t *count);
/* What the last bk_clip_loci of this context counted: out[0] records, [1] eligible records, [2] events (those beyond among them), [3]
 * events beyond a contig's end, [4] exact sites, [5] loci, [6] loci with a mutual partner, [7] returned rows.  BK_ERR_ARG for a null
 * argument. */
int bk_clip_locus_counts(bk_ctx *records, uint64_t out[8]);

/* Copy a stage's result to library-owned host memory.  *data stays valid until the next bk_fetch
 * of the same stage or bk_free.  group_off (may be NULL) receives n_groups+1 offsets for pair stages. */
int bk_fetch(bk_ctx *ctx, int stage, const void **data, uint64_t *count, const uint64_t **group_off, uint32_t *n_groups);

/* Per-group counts behind the reference's stage log and `_performance.txt` (BreakID.cc:119-191), groups in the reference's
 * std::map<string> order: pairs after scan_discordant_pairs, after remove_isolated_pairs (:123), after clustering (:129-137), and
 * one past the largest cluster number of the group (-fast numbers from 1: find_cluster_pairs_enspan_fast returned
 * cluster_id_end - 1; AHC from 0: #roots = cluster_id_end + n_isolated_removed - n_clustered).  Valid after bk_cluster_summary. */
typedef struct bk_group_stat {
  int32_t p1_tid, p2_tid;
  uint64_t n_scan, n_isolated_removed, n_clustered;
  uint32_t cluster_id_end;
  uint32_t ordinal;          /* of the group in the reference's std::map<string> order of "chrA_chrB" among ALL groups of the sample
                                (= bk_pair.group; on one GPU simply the row number) */
} bk_group_stat;
int bk_group_stats(bk_ctx *ctx, const bk_group_stat **out, uint32_t *n_groups);

/* per-kernel timing of the last stage calls: name/ms pairs, for bench.py's roofline leg */
int bk_timing(bk_ctx *ctx, const char *const **names, const float **ms, const uint64_t **bytes, int *n);
int bk_timing_enable(bk_ctx *ctx, int on);
/* after bk_timing: bytes each timed stage's own kernels load + store (0 = not modelled), same order and count as bk_timing */
int bk_timing_touched(bk_ctx *ctx, const uint64_t **touched, int *n);

/* ---- one sample sharded over several GPUs -----------------------------------------------------
 * One context per GPU holds a contiguous range of the sample's coordinate-sorted records.  The library does the
 * per-shard work; the caller moves the small tables between the contexts (RCCL all-gather / all-reduce over xGMI
 * from torch.distributed in breakid_amd/sharded.py).  Sequence:
 *   bk_upload_records; bk_shard_begin                       stream pass, record indices are global (rec_base + i)
 *   bk_shard_get_stats -> all-reduce -> bk_shard_set_stats  insert-size sums, spans
 *   bk_shard_sd_local -> all-gather -> bk_shard_sd_finish   bit-exact sd: exceptions replayed in global record order
 *   BK_BUF_CANDIDATES: bk_shard_buffer -> all-gather -> bk_shard_set_buffer; bk_discordant_pairs (replicated join)
 *   bk_shard_group_sizes -> owner per group -> bk_shard_own_groups; bk_mask_and_cluster; bk_cluster_summary
 *   BK_BUF_TUPLES, BK_BUF_CLUSTERS: gather as above
 *   bk_shard_bp_cov -> all-reduce(sum) -> bk_shard_bp_vote -> bk_shard_bp_depth -> all-reduce(sum) -> bk_shard_bp_finish
 * after which every context holds the complete cluster table (bk_fetch).  One CONTEXT holds fewer than 2^32 records; the sample
 * may hold more (record indices are 64-bit across the contexts: rec_base + i). */
typedef struct bk_shard_stats {
  uint64_t isize_sum, isize_n;
  double sumsq;
  uint32_t vmax, max_span;
  uint64_t n_cand, n_split;
} bk_shard_stats;
#define BK_BUF_CANDIDATES 0 /* 40-byte candidates of the discordant filter */
#define BK_BUF_TUPLES 1     /* bk_split, unsorted */
#define BK_BUF_CLUSTERS 2   /* bk_cluster of the groups this rank owns */
int bk_shard_begin(bk_ctx *ctx, uint64_t rec_base, int mapq_min);
int bk_shard_get_stats(bk_ctx *ctx, bk_shard_stats *out);
int bk_shard_set_stats(bk_ctx *ctx, const bk_shard_stats *total);
int bk_shard_sd_local(bk_ctx *ctx, uint64_t *l_total, void **ex_dev, uint64_t *n_ex); /* exceptions: 16 B {u64 l_before, f64 d}, device */
int bk_shard_sd_finish(bk_ctx *ctx, const void *all_ex_dev, uint64_t n_all, uint64_t l_grand, double *mean, double *sd);
int bk_shard_buffer(bk_ctx *ctx, int which, void **dev, uint64_t *count, uint32_t *elem_bytes);
int bk_shard_set_buffer(bk_ctx *ctx, int which, const void *dev, uint64_t count); /* gathered table, device, caller keeps it alive */
int bk_shard_group_sizes(bk_ctx *ctx, const uint64_t **starts, uint32_t *n_groups); /* n_groups+1 pair offsets, numeric key order */
int bk_shard_own_groups(bk_ctx *ctx, const uint8_t *own, uint32_t n_groups);
/* Routed exchange (scales with the number of GPUs: no rank joins or sorts more than its share).  Instead of the
 * replicated join above:
 *   bk_shard_route_candidates -> all-to-all -> bk_shard_set_buffer(BK_BUF_CANDIDATES); bk_discordant_pairs joins the
 *     read names this rank owns ((qhash >> 17) % world)
 *   bk_shard_group_keys + bk_shard_group_sizes -> all-gather of (key, size) -> owner per chr-pair key (LPT on the totals)
 *   bk_shard_route_pairs -> all-to-all -> bk_shard_group_pairs: the table of exactly the groups this rank owns, `group`
 *     ordinals global; then bk_mask_and_cluster, bk_cluster_summary and the gathers / reductions as above. */
int bk_shard_route_candidates(bk_ctx *ctx, uint32_t world, void **dev, const uint64_t **counts); /* 40-byte candidates ordered by destination; counts[world] */
int bk_shard_group_keys(bk_ctx *ctx, const uint32_t **keys, uint32_t *n_groups);                /* (p1_tid+1)*(n_targets+1)+(p2_tid+1) per group */
int bk_shard_route_pairs(bk_ctx *ctx, const uint32_t *dest_of_group, uint32_t n_groups, uint32_t world, void **dev, const uint64_t **counts); /* bk_pair rows ordered by destination */
int bk_shard_group_pairs(bk_ctx *ctx, const void *pairs_dev, uint64_t n, const uint32_t *all_keys, uint32_t n_all_keys);
int bk_shard_bp_cov(bk_ctx *ctx, double w, void **cov_dev, uint64_t *n);   /* u32[2*n_clusters] partial coverage counts */
int bk_shard_bp_vote(bk_ctx *ctx, double w, const void *cov_total_dev);
/* the vote of clusters [lo, hi) only (every rank takes a slice); the voted rows (72 B) and flags (u32) of the slices are
 * then all-gathered in rank order: BK_BUF_CLUSTERS via bk_shard_set_buffer, the flags via bk_shard_bp_set_voted */
int bk_shard_bp_vote_slice(bk_ctx *ctx, double w, const void *cov_total_dev, uint64_t lo, uint64_t hi, void **clusters_dev, void **voted_dev);
int bk_shard_bp_set_voted(bk_ctx *ctx, const void *voted_all_dev);
int bk_shard_bp_depth(bk_ctx *ctx, void **depth_dev, uint64_t *n);         /* u32[2*n_clusters] partial depth counts */
int bk_shard_bp_finish(bk_ctx *ctx, const void *depth_total_dev);

/* Test hook: orders every group [group_off[g], group_off[g+1]) of `key` exactly as
 * std::sort(first, last, [](a, b){ return a.key < b.key; }) of libstdc++ does (the reference's unstable sorts,
 * BreakID.cc:1274-1282,1091,1127) and returns the permutation (perm_out[p] = original index of the element now at p). */
int bk_debug_std_sort(bk_ctx *ctx, const uint32_t *key, const uint64_t *group_off, uint32_t n_groups, uint32_t *perm_out);

/* Test hooks of the two device-wide primitives every stage stands on (csrc/prims.h), on the context's stream and in buffers the
 * context keeps between calls (so what an earlier call of another size left behind is part of what a test sees):
 *   bk_debug_scan        prims::exclusive_scan of n elements of elem_bytes (4 or 8) bytes: out[0] = 0, out[i] = in[0] + .. +
 *                        in[i-1] modulo 2^32 / 2^64, out[n] = the total (n + 1 entries).  in_place != 0: input and output are
 *                        one device buffer of n + 1 entries, as the radix sort scans its histogram.
 *   bk_debug_radix_sort  prims::radix_sort_pairs: (keys, vals) ordered by bits [begin_bit, end_bit) of the key alone, stable;
 *                        begin_bit >= end_bit is the identity.  0 <= begin_bit and end_bit <= 64, else BK_ERR_ARG; more than
 *                        2^32 - 16 items give BK_ERR_LIMIT.
 *   bk_debug_prims_info  the tile constants of this build: BLOCK, SCAN_TILE, SCAN_ONE_MAX, RS_TILE (the sizes at which the
 *                        primitives change their form follow from them) */
int bk_debug_scan(bk_ctx *ctx, int elem_bytes, const void *in, uint64_t n, int in_place, void *out);
int bk_debug_radix_sort(bk_ctx *ctx, const uint64_t *keys, const uint32_t *vals, uint64_t n, int begin_bit, int end_bit, uint64_t *keys_out, uint32_t *vals_out);
int bk_debug_prims_info(uint64_t out[4]);

/* Test hook: how the std::sort replays of this context ran so far, summed over its lanes: out[0] jobs of the resident sort
 * service, out[1] task dispatches on the caller's stream.  out[2] is always 0: it counted a third form (chains of launches)
 * that no longer exists; the three-word signature stays. */
int bk_sort_forms(bk_ctx *ctx, uint64_t out[3]);

/* Test hook: the sizes at which the std::sort replay changes its code path in this build, and what the last sort through
 * bk_debug_std_sort met.  out[0..9] = FIN_MAX, HEAP_BIG_MIN, HEAP_RANKED_MAX, HEAP_LARGE, SVC_WIDE_MIN, F2_HB, F2_EXT, HEAP_PAD,
 * SJ_MAX_WIDE, SJ_MAX_NARROW; out[10] = cap32, the ranked heap entries that fit a wide workgroup's LDS in the task dispatch (from
 * the kernel's attributes on the context's device); out[11] = the longest heap segment and out[12] = the elements in heap
 * segments of the context's last debug sort, as its task dispatch counted them (0xFFFFFFFF each when that sort ran as a job of
 * the resident service, whose statistics are not read back; 0 before the first sort). */
int bk_debug_sort_info(bk_ctx *ctx, uint64_t out[13]);

/* Test hook: find_cluster_pairs_enspan_ahc (BreakID.cc:1304-1352) on one group of x-sorted points; returns the
 * surviving point indices in output order with their cluster numbers. */
int bk_debug_ahc(bk_ctx *ctx, const uint32_t *x, const uint32_t *y, uint32_t n, double w, uint32_t *idx_out, int32_t *cluster_out, uint32_t *n_out);

/* Test hooks that run the reference's unit vectors (tests/golden/units.json, *.regions.json) through the device code of the
 * product path - the same kernels / device functions the stages use:
 *   bk_debug_points  one group of points in the given order; mode 0 = mask_pairs_chr_pos (BreakID.cc:1813-1877), 1 =
 *                    remove_isolated_pairs (:1271-1285), 2 = find_cluster_pairs_enspan_fast (:1046-1160, x-sorted input):
 *                    surviving point indices in output order (+ cluster numbers for mode 2).  It is the one-group call of
 *   bk_debug_points_groups  the same for n_groups groups in ONE list, as the lanes hand it to the product functions (mask_list,
 *                    remove_isolated_all, fast_cluster_all with ng = n_groups): group_off has n_groups + 1 ascending entries
 *                    starting at 0 (equal neighbours = an empty group), the points of group g are x / y [group_off[g],
 *                    group_off[g+1]).  idx_out (room for 2 * n entries: masking can emit a group's element 1 twice) indexes x / y,
 *                    cluster_out (mode 2, may be NULL) restarts at 1 in every group, goff_out (n_groups + 1 entries, may be NULL)
 *                    receives the list's group offsets afterwards, *n_out its length.  BK_ERR_ARG for offsets that do not
 *                    ascend from 0.
 *   bk_debug_cluster_info  FW_TILE and FW_LEVELS of this build (csrc/cluster.h: the tile of the chain-following kernels of the fast
 *                    clustering and their rounds of pointer doubling); no GPU needed
 *   bk_debug_cigar   n rows of the CIGAR model (CigarRoller.cc / Cigar.cc): c1 = text (kind 0) or BAM words (kind 1, 4-byte
 *                    aligned rows), c2 = SA cigar text, e = tolerance; out6 = rolled op count, begin clips, end clips,
 *                    reference length, matches, is_complementary_cigar(c2, e) (CigarRoller.cc:323-346)
 *   bk_debug_vote    find_bp_pair (BreakID.cc:577-857) on two tuple tables: voted (p1_bp, p2_bp, count) or (-1, -1, 0) when the
 *                    best count stays below 2 (:446)
 *   bk_debug_region  find_sa_reads (:868-1037) on a raw region of the uploaded table: evidence tuples that survive the region
 *                    verdict, total_coverage capped at 5, and cal_single_base_depth (util_bed.cc:154-192) at depth_pos */
int bk_debug_points(bk_ctx *ctx, int mode, const uint32_t *x, const uint32_t *y, uint32_t n, double w, uint32_t *idx_out, int32_t *cluster_out, uint32_t *n_out);
int bk_debug_points_groups(bk_ctx *ctx, int mode, const uint32_t *x, const uint32_t *y, const uint64_t *group_off, uint32_t n_groups, double w, uint32_t *idx_out,
                           int32_t *cluster_out, uint64_t *goff_out, uint32_t *n_out);
int bk_debug_cluster_info(uint64_t out[2]);
/*   bk_debug_stream_info    the constants of the built stream pass (csrc/stream.hip): STREAM_V (records per lane and iteration), the
 *                    capacities of the LDS candidate bin and of the LDS bin of SA-bearing record indices, and the number of blocks
 *                    launch_stream takes for one resident set (0 in a process without a device; nothing else needs one)
 *   bk_debug_stream_blocks  a process-wide cap on the grid of k_stream, applied after the resident cap; 0 = none (the default).
 *                    With a cap of 1 .. 3 a table of a few thousand records runs many iterations per block, so the tests reach
 *                    the flush windows and the edges of the two bins at small sizes.  Set it back to 0 afterwards. */
int bk_debug_stream_info(uint64_t out[4]);
int bk_debug_stream_blocks(unsigned blocks);
int bk_debug_cigar(bk_ctx *ctx, uint32_t n, const uint8_t *kind, const uint32_t *c1_off, const uint8_t *c1, const uint32_t *c2_off, const uint8_t *c2, const int32_t *e,
                   int32_t *out6);
int bk_debug_vote(bk_ctx *ctx, const bk_split *side1, uint32_t n1, const bk_split *side2, uint32_t n2, int32_t p1_tid, int32_t p2_tid, int32_t *out3);
int bk_debug_region(bk_ctx *ctx, int32_t tid, uint32_t start, uint32_t end, uint64_t depth_pos, bk_split *out, uint32_t cap, uint32_t *n_out, uint32_t *cov_out,
                    uint32_t *depth_out);

/* ---- host feed (C++ BGZF/BAM decoder -> pinned SoA); replaces htslib's reader for this path --- */
typedef struct bk_bam bk_bam;
uint64_t bk_qname_hash(const char *name, size_t len);
uint32_t bk_qname_check(const char *name, size_t len); /* the qcheck column: independent of bk_qname_hash, folds the length in, never 0 */
int bk_bam_open(const char *path, bk_bam **out, char *err, size_t errlen);
int bk_bam_header(const bk_bam *b, int *n_targets, const char *const **names, const uint32_t **lens);
/* decode all records into a SoA owned by the bk_bam (pinned when a GPU is present) */
int bk_bam_decode(bk_bam *b, bk_soa *out, char *err, size_t errlen);
void bk_bam_close(bk_bam *b);
/* Read names back from their hashes, and the reads themselves: one streaming pass over in_bam (read in chunks, inflated block by
 * block, a record that crosses BGZF blocks carried over: both file layouts; memory is bounded by the chunk, the longest record and
 * the keys - the inflated file is never held).  A record is selected when its read name (the C string, as the decoders hash it) has
 * bk_qname_hash == keys[k].qhash and, unless keys[k].qcheck is 0, bk_qname_check == keys[k].qcheck: both mates and every secondary
 * and supplementary alignment of that name.  names_out (may be NULL) receives n_keys NUL-terminated names back to back in key order,
 * "" for a key no record matched; free it with bk_bam_names_free.  out_bam (may be NULL: names only, no file) receives the selected
 * records in file order (the output stays coordinate sorted) behind the input's header bytes, unchanged (text, reference names and
 * lengths); every record gets bk:Z:<tags[keys[k].tag]> appended to its aux data, its block_size corrected.  BGZF as htslib writes it:
 * at most 0xff00 payload bytes per block, a block is flushed before a record that would not fit, a longer record spans blocks, the
 * 28-byte EOF block comes last.  The file is written under a temporary name in the target directory and renamed on success; on any
 * failure no output file exists.  n_written (may be NULL): records selected.  An empty key set gives a header-only BAM.
 * BK_ERR_ARG: null in_bam, null keys or tags with a non-zero count, duplicate keys (equal qhash and qcheck), tag >= n_tags.
 * BK_ERR_IO: unreadable or truncated input, a bad BGZF block, a record longer than its stream, an unwritable output.  The text
 * is in err.  Limits: a record that already carries a bk tag gets a second one; two different names that agree in all 96 hash
 * bits are both written (and the key's name is that of the first of them in the file). */
typedef struct bk_read_key { uint64_t qhash; uint32_t qcheck; uint32_t tag; } bk_read_key; /* tag: index into tags[] */
int bk_bam_extract(const char *in_bam, const char *out_bam, const bk_read_key *keys, uint64_t n_keys, const char *const *tags, uint64_t n_tags, char **names_out,
                   uint64_t *n_written, char *err, size_t errlen);
void bk_bam_names_free(char *names);
/* The alignments of named reads with their bases: the pass of bk_bam_extract (selection by keys, streaming, both file layouts,
 * memory bound, error codes; keys[k].tag is not read) with a table as its result instead of a file.  Rows are in file order;
 * key[i] is the first key that selects row i, as bk_bam_extract picks its tag; a record with l_seq == 0 is kept with an empty
 * sequence; an empty key set gives n == 0 and is no error.  The table is host memory that bk_reads_free gives back (it zeroes the
 * struct; a table the call did not fill, or filled with an error, needs no free).  BK_ERR_ARG also for a null out, BK_ERR_LIMIT
 * beyond 2^32 keys or CIGAR words. */
int bk_bam_reads(const char *in_bam, const bk_read_key *keys, uint64_t n_keys, bk_reads *out, char *err, size_t errlen);
void bk_reads_free(bk_reads *r);

/* The same feed on the GPU: BGZF blocks are inflated on the device (bgzf_gpu.hip) and the records are decoded into
 * device-resident columns (cols holds device pointers: bk_upload_records(ctx, cols, BK_MEM_DEVICE)).
 * Files whose records stay inside their BGZF blocks (htslib / samtools writers) are streamed in chunks
 * (BREAKID_FEED_CHUNK_MB, default 32-64 MiB, four to eight in flight): device memory holds the chunks in flight and the
 * columns.  Files whose records run across blocks (htsjdk / Picard / GATK writers, long reads): record boundaries are
 * guessed per block and verified to chain, in chunks that start at the record carried over from the chunk before; a record
 * longer than 8 MiB that crosses a chunk sends the file to a one-batch variant (file image + inflated stream in HBM).
 * BK_ERR_IO when the boundaries cannot be established, BK_ERR_LIMIT when neither variant can take the file - take
 * bk_bam_open / bk_bam_decode then. */
typedef struct bk_bam_dev bk_bam_dev;
int bk_bam_decode_device(const char *path, int device, bk_bam_dev **out, bk_soa *cols, int *n_targets, const char *const **names, const uint32_t **lens,
                         char *err, size_t errlen);
/* One part of a file whose records stay inside their BGZF blocks: the blocks that start in [b(part), b(part + 1)), where b(k)
 * is the first block start at or behind k / parts of the file's bytes (found by hopping over the block headers, so every caller
 * finds the same boundaries and the parts tile the file) - the record range of one rank of a sharded run (bk_shard_*), decoded on
 * that rank's own GPU; the ranks' record counts give their rec_base.  The header is parsed by every part.  BK_ERR_IO for files
 * whose records run across blocks (they have no such cut points: take the host decoder). */
int bk_bam_decode_device_part(const char *path, int device, int part, int parts, bk_bam_dev **out, bk_soa *cols, int *n_targets, const char *const **names,
                              const uint32_t **lens, char *err, size_t errlen);
void bk_bam_dev_free(bk_bam_dev *h);
/* What the GPU feed keeps between files so that the second file of a process starts at full speed: three page-locked staging
 * buffers per chunk size (32 or 64 MiB each), and per device the feed slots of the last decode (streams, events, device buffers:
 * ~0.3 GB per slot, four to eight slots).  This call gives all of it back; no decode may be running.  The next file pays the
 * first-file cost again (~60 ms: registration of the staging buffers, allocations). */
void bk_feed_release_caches(void);
/* Feed and hot path overlapped: the reference reads the BAM twice, one pass after the other (BreakID.cc:1929,
 * :1414); here the file is read once, and the record-level kernel of the hot path (insert-size sums, discordant filter,
 * SA gate: k_stream) runs on the records of a feed chunk while the following chunks are still being copied and inflated.
 * Creates the context itself (the reference list comes out of the file), attaches the device table (BK_MEM_DEVICE) and
 * returns with the stream pass complete: continue with bk_isize_stats / bk_discordant_pairs(mapq_min) / ...  *bam_out owns
 * the columns and must outlive the context.  Same file support and errors as bk_bam_decode_device. */
int bk_bam_decode_device_ctx(const char *path, int device, int mapq_min, bk_bam_dev **bam_out, bk_ctx **ctx_out, int *n_targets, const char *const **names,
                             const uint32_t **lens, char *err, size_t errlen);
/* The record table a context holds, as device pointers (cols->n, n_cigar_words, n_aux_bytes say how much lies behind them): the
 * table of bk_bam_decode_device_ctx, which hands out no bk_soa of its own, a BK_MEM_DEVICE table as it was attached, or the device
 * copy of a BK_MEM_HOST upload.  The context's stream is synchronised first.  The columns belong to whoever owned them before
 * (the bk_bam_dev, the caller, the context).  BK_ERR_ARG when the context holds no table. */
int bk_records(bk_ctx *ctx, bk_soa *cols);
/* test / measurement hook: inflates a whole BGZF file image on the GPU, bytes back to the host */
int bk_debug_bgzf_inflate(const void *file, uint64_t n, void *out, uint64_t out_cap, uint64_t *out_len, float *kernel_ms, char *err, size_t errlen);
/* Test hooks of the GPU inflate alone (csrc/bgzf_gpu.hip; tests/inflatecases.py, tests/test_gpu_inflate.py):
 *   bk_debug_bgzf_inflate_form  bk_debug_bgzf_inflate with the decoder and the output layout named outright.  form: a sum of
 *                        BK_BGZF_FORM_ROUNDS (the decoder that takes 64 bit positions per round; without it the lanes decoder,
 *                        which leaves windows that do not synchronise to the rounds) and BK_BGZF_FORM_SHARED (the kernels the
 *                        streaming feed launches: another register allocation).  out_align: 256 (every block's output starts at a
 *                        multiple of 256, as the feed of block-aligned files lays it out) or 1 (the blocks abut, as the feed of
 *                        files whose records cross blocks lays them out: a block whose offset is no multiple of 4 takes the byte
 *                        stores of the resolve kernel).  out receives the blocks' bytes back to back either way.  BK_ERR_ARG for
 *                        another form or alignment; BK_ERR_IO "inflate failed" when any block is malformed or does not give isize
 *                        bytes (one flag per call: out is then not written).  A block's CRC32 is not looked at.
 *   bk_debug_bgzf_info   the constants of this build, no GPU needed: out[0..10] = LIT_FAST, DIST_FAST (bits of the direct tables),
 *                        LANE_PART_BITS, LANE_CHECK_BITS, LANE_FULL_WALKS (a lane's part of a window, its checkpoint, the long
 *                        passes after which a window goes to the rounds), CHUNK_DW (dwords the input window slides by), RES_WIN,
 *                        RESOLVE_THREADS (output positions per resolve window, threads of a resolve block), BGZF_BATCH_BLOCKS
 *                        (blocks per launch pair), BGZF_TOKENS_PER_BLOCK, BGZF_MAX_DEFLATE_BLOCKS (deflate blocks one BGZF block
 *                        may hold: one more is reported as malformed) */
#define BK_BGZF_FORM_ROUNDS 1
#define BK_BGZF_FORM_SHARED 2
int bk_debug_bgzf_inflate_form(const void *file, uint64_t n, void *out, uint64_t out_cap, uint64_t *out_len, int form, uint64_t out_align, char *err, size_t errlen);
int bk_debug_bgzf_info(uint64_t out[11]);

#ifdef __cplusplus
}
#endif
#endif
