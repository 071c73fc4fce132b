// Interface of cliploci.hip: soft-clip pile-ups called over the whole record table (bk_clip_loci).
#pragma once
#include "bk_common.h"
#include "bp.h"
#include "clip.h"
#include "prims.h"

struct ClipLociBufs
{
  DevBuf tile_ev, tile_eb, totals, ev, sorted, keys, vals, lhead, xhead, qhead, exl, exx, exq, exd, lstart, xstart, rows, lkey, partner, mutual, bkeys, bvals, claim, keep, out;
  DevBuf scan_tmp, scan_tmp64;
  prims::RadixBufs radix;
};

// the record table, where a record's read-name hash comes from (the bk_side row when the table has one, the column otherwise), and
// the reference list
struct ClipLociInput
{
  RecView rec;  // aux_off set
  uint64_t n_cigar_words = 0;
  const bk_side *side = nullptr;
  const uint64_t *qhash = nullptr;
  const uint32_t *tprefix = nullptr;  // nt + 1 prefix sums of the contig lengths (modulo 2^32: only differences are used)
  int nt = 0;
  uint32_t max_len = 0;  // the longest contig
};

struct ClipLociParams
{
  int mapq_min, min_clip;
  uint32_t tol, pair_dist, min_reads;
};

struct ClipLociStats
{
  uint64_t n = 0, eligible = 0, events = 0 /* kept: beyond is not among them */, beyond = 0, exact = 0, loci = 0, mutual = 0, written = 0, breakpoints = 0;
  int pos_bits = 0, tid_bits = 0;
  uint64_t touched_records() const;  // the record pass by the byte model of include/breakid_hip.h
  uint64_t touched_calls() const;    // everything behind it
};

// The record pass: counts the events of every tile of records, scans the tile counts and writes the events in record order into
// b.ev.  Waits for the stream once (the three totals).  Throws BK_ERR_LIMIT beyond 2^30 events.
void cliploci_events(const ClipLociInput &in, const ClipLociParams &p, ClipLociBufs &b, hipStream_t st, ClipLociStats *stats);
// The loci from the stats->events events of b.ev.  `cl` (may be null: no claim) is the device cluster table of ncl rows in which the
// claiming row is looked up.  Waits for the stream twice (exact sites and loci; mutual partners and written rows).  Device array
// owned by `b`: rows[stats->written].
void cliploci_calls(const ClipLociParams &p, const bk_cluster *cl, uint64_t ncl, ClipLociBufs &b, hipStream_t st, struct bk_clip_locus **rows, ClipLociStats *stats);
