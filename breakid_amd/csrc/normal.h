// Interface of normal.hip: matched-normal evidence of the tumour's clusters (bk_normal_support).
#pragma once
#include "bk_common.h"
#include "prims.h"
#include "bp.h"
#include "tuple_match.h"

struct NormalBufs
{
  DevBuf key, val, key2, val2, flag, rank, gtab, rows, res;
  prims::RadixBufs radix;
  BpBufs bb;  // samp / voted / depth of the depth phase (bp_depth_partial)
};

// The normal side of one call: its discordant pairs (BK_STAGE_SCAN table), its record-ordered tuples and its record table.
struct NormalSide
{
  const bk_pair *pairs;
  uint64_t n_pairs;
  TupleTable tuples;
  RecView rec;
};

// out[c] = the four counts of tumour cluster c, row c of `cl` (BK_STAGE_CLUSTERS order: bp.hip, cluster_summary): a device array of
// ncl entries owned by `b`.
void normal_support(const NormalSide &n, const bk_cluster *cl, uint64_t ncl, double w, NormalBufs &b, hipStream_t st, struct bk_normal_support **out);
