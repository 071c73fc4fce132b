// Interface of junction.hip: per-call junction evidence (bk_junctions).
#pragma once
#include "bk_common.h"
#include "bp.h"

struct JunctionBufs
{
  DevBuf res, grp, visited;
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

// out[c] = the junction evidence of cluster c (device order of `cl`); grp_out[c] = its `group` (the caller restores BK_STAGE_CLUSTERS
// order); visited_out[c] = tuples its wave searched (the byte model).  Device arrays of ncl entries owned by `b`.
void junctions(const JunctionPairs &p, const bk_split *sp, uint64_t nsp, const bk_cluster *cl, uint64_t ncl, int maxspan, const int32_t *hdr_id, const int32_t *own_id,
               int32_t nt, int32_t empty_id, JunctionBufs &b, hipStream_t st, struct bk_junction **out, uint32_t **grp_out, uint32_t **visited_out);
