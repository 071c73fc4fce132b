// Interface of unique.hip: the unique fragments behind every call (bk_unique_support).
#pragma once
#include "bk_common.h"
#include "evidence.h"

// Rows of one (call, kind) a wavefront looks at per step of the last pass (k_uq_runs): a fragment with more rows than this spans
// several steps, its head carried from one to the next.  tests/dedupcases.py mirrors it (UNIQUE_TILE) to build calls that straddle it.
constexpr int UNIQUE_TILE = 64;

struct UniqueBufs
{
  EvidenceBufs ev;    // its own: bk_evidence's buffers stay as the caller last saw them
  EvidenceKeys keys;  // the fragment key words of every row (evidence.h)
  DevBuf differ, key_a, key_b, val_a, val_b, hist, scan_tmp, res, first;
};

// what the passes report (host side, for the byte model of bk_timing)
struct UniqueStat
{
  uint64_t n_rows = 0;
  uint32_t passes = 0;   // 8-bit radix passes that ran: the digits in which two rows differ at all
  uint32_t gathers = 0;  // key words that had such a digit
};

// One bk_unique_support row per row of `cl` in *res_out and, with listing, first[n_rows] in *first_out: device arrays owned by `b`.
// *ev_stat_out is evidence()'s own (device, one entry); its `bad` also reports a sorted row outside the range of its call.
void unique_support(const JunctionPairs &p, const TupleTable &tt, const bk_cluster *cl, uint64_t ncl, const EvidenceRecs &recs, bool listing, UniqueBufs &b, hipStream_t st,
                    struct bk_unique_support **res_out, uint64_t **first_out, EvidenceStat **ev_stat_out, UniqueStat *stat);
