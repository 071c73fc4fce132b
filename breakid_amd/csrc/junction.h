// Interface of junction.hip: per-call junction evidence (bk_junctions).
#pragma once
#include "bk_common.h"
#include "bp.h"
#include "tuple_match.h"

struct JunctionBufs
{
  DevBuf res, visited;
};

// The clustered pair list (lanes.hip) and the slot -> cluster-row map cluster_summary left behind (bp.hip: slot = slotbase[group] +
// cluster number; a slot with keep != 0 is row off[slot] of the device cluster table).
struct JunctionPairs
{
  const bk_pair *pairs;
  const uint32_t *idx, *gof, *cl;
  uint64_t n;
  uint32_t ng;
  const uint32_t *slotbase, *keep, *off;
};

// out[c] = the junction evidence of cluster c, row c of `cl` (BK_STAGE_CLUSTERS order: bp.hip, cluster_summary); visited_out[c] =
// tuples its wave searched (the byte model).  Device arrays of ncl entries owned by `b`.  pairs_only: the member pairs alone are
// counted, no tuple is searched (splits and visited stay 0).
void junctions(const JunctionPairs &p, const TupleTable &tt, const bk_cluster *cl, uint64_t ncl, JunctionBufs &b, hipStream_t st, struct bk_junction **out,
               uint32_t **visited_out, bool pairs_only = false);
