// Interface of gaps.hip: deletions and insertions called from the CIGAR gaps of the record table (bk_cigar_gaps).
#pragma once
#include "bk_common.h"
#include "bp.h"
#include "prims.h"

constexpr int GAP_LEN_BITS = 28;  // a BAM CIGAR word holds its length in 28 bits

struct GapBufs
{
  DevBuf tile_ev, tile_eb, totals, ev, sorted, bylen, keys, vals, head, qhead, ex, exx, exq, exd, cstart, xstart, rows, keep, out;
  DevBuf scan_tmp, scan_tmp64;
  prims::RadixBufs radix;
};

// the record table, where a record's read-name hash comes from (the bk_side row when the table has one, the column otherwise), and
// the reference list
struct GapInput
{
  RecView rec;
  uint64_t n_cigar_words = 0;
  const bk_side *side = nullptr;
  const uint64_t *qhash = nullptr;
  const uint32_t *tprefix = nullptr;  // nt + 1 prefix sums of the contig lengths (modulo 2^32: only differences are used)
  int nt = 0;
  uint32_t max_len = 0;  // the longest contig
};

struct GapParams
{
  int mapq_min;
  uint32_t min_len, anchor, tol, min_reads;
};

struct GapStats
{
  uint64_t n = 0, eligible = 0, events = 0, beyond = 0, exact = 0, loci = 0, calls = 0, written = 0;
  int start_bits = 0, tid_bits = 0;
  uint64_t touched_records() const;  // the record pass by the byte model of include/breakid_hip.h
  uint64_t touched_calls() const;    // everything behind it
};

// The record pass: counts the events of every tile of records, scans the tile counts and writes the events in record order into
// b.ev.  Waits for the stream once (the three totals).  Throws BK_ERR_LIMIT beyond 2^30 events.
void gap_events(const GapInput &in, const GapParams &p, GapBufs &b, hipStream_t st, GapStats *stats);
// The calls from the stats->events events of b.ev.  Waits for the stream three times (loci; exact events and calls; written rows).
// Device array owned by `b`: rows[stats->written].
void gap_calls(const GapParams &p, GapBufs &b, hipStream_t st, struct bk_cigar_gap **rows, GapStats *stats);
