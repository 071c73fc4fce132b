// Interface of fragsize.hip: the fragment lengths the member pairs imply across each call's junction (bk_fragment_sizes).
#pragma once
#include "bk_common.h"
#include "bp.h"
#include "evidence.h"

// Records of equal (tid, pos) a lane of k_fg_lengths looks at on its own before the wavefront takes the walk over, 64 records a step.
// tests/fragcases.py mirrors it (LANE_WALK) to build pile-ups on either side of it.
constexpr int FRAG_LANE_WALK = 8;

// one entry per pair row: its length, or why it has none
constexpr uint32_t FRAG_USED = 0, FRAG_OFF = 1, FRAG_LOST = 2, FRAG_SKIP = 3;
struct FragLen
{
  int32_t len;
  uint32_t mark;
};

// what the kernels report besides the rows (statistics for the byte model and BK_DEBUG=fragsize; no result depends on them)
struct FragStat
{
  uint32_t bad;      // != 0: a row outside the range of its call (nothing is written then)
  uint32_t longest;  // records of the longest equal-position walk
  unsigned long long lookups, walked, wave_walks;  // records looked up, records their walks read, walks a whole wavefront finished
};

struct FragBufs
{
  EvidenceBufs ev;  // its own: bk_evidence's buffers stay as the caller last saw them
  DevBuf sites, len, res, stat, samp;
};

// the sites in device memory (not part of the timed scope)
void fragsize_upload(const struct bk_frag_site *sites, uint64_t n, FragBufs &b, hipStream_t st);
// One bk_frag_sizes row per row of `cl` in *res_out, one FragLen per pair row in *len_out (pair_off_out[ncl + 1] bounds the calls): device
// arrays owned by `b`.  *ev_stat_out is evidence()'s own, *stat_out the one above (device, one entry each).
void fragment_sizes(const JunctionPairs &p, const TupleTable &tt, const bk_cluster *cl, uint64_t ncl, const EvidenceRecs &recs, const RecView &rec, int32_t lo, int32_t hi,
                    FragBufs &b, hipStream_t st, struct bk_frag_sizes **res_out, FragLen **len_out, uint64_t **pair_off_out, uint64_t *n_rows_out, EvidenceStat **ev_stat_out,
                    FragStat **stat_out);
