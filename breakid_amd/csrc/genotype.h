// Interface of genotype.hip: reference-allele evidence of every voted call (bk_ref_support).
#pragma once
#include "bk_common.h"
#include "bp.h"

struct RefBufs
{
  DevBuf samp, res, stat;
};

// per (call, side) wave, written only when a byte model is wanted: records of its window, CIGAR words walked
struct RefStat
{
  uint32_t visited, words;
};

// out[c] = the four counts of call c, row c of `cl` (BK_STAGE_CLUSTERS order: bp.hip, cluster_summary), on the record table `rec`
// (isize and aux_off set; maxspan = its max(bam_endpos - pos)).  stat_out (may be null) receives 2 * ncl RefStat rows,
// [2 * c + side].  Both are device arrays owned by `b`.
void ref_support(const RecView &rec, int maxspan, const bk_cluster *cl, uint64_t ncl, int mapq_min, int anchor, double w, RefBufs &b, hipStream_t st,
                 struct bk_ref_support **out, RefStat **stat_out);
