// Interface of normal.hip: matched-normal evidence of the tumour's clusters (bk_normal_support).
#pragma once
#include "bk_common.h"
#include "prims.h"
#include "bp.h"

struct NormalBufs
{
  DevBuf key, val, key2, val2, flag, rank, gtab, rows, res, grp;
  prims::RadixBufs radix;
  BpBufs bb;  // samp / voted / depth of the depth phase (bp_depth_partial)
};

// The normal side of one call: its discordant pairs (BK_STAGE_SCAN table), its record-ordered tuples and its record table.
struct NormalSide
{
  const bk_pair *pairs;
  uint64_t n_pairs;
  const bk_split *sp;
  uint64_t n_split;
  RecView rec;
  int maxspan;
  const int32_t *hdr_id;  // interned chromosome id per tid + 1 (the vote's p1_chr, bp.hip: k_bp_vote)
  const int32_t *own_id;  // per tid: interned id a tuple of a record on that tid carries for its own side (stream.hip: own_chr)
  int32_t empty_id;       // ... and for a record outside the header
};

// out[c] = the four counts of tumour cluster c (device order of `cl`); grp_out[c] = its `group` (the caller restores BK_STAGE_CLUSTERS
// order).  Both are device arrays of ncl entries owned by `b`.
void normal_support(const NormalSide &n, const bk_cluster *cl, uint64_t ncl, int32_t nt, double w, NormalBufs &b, hipStream_t st, struct bk_normal_support **out,
                    uint32_t **grp_out);
