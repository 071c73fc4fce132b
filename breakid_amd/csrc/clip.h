// Interface of clip.hip: soft-clip evidence of every cluster (bk_clip_support).
#pragma once
#include "bk_common.h"
#include "bp.h"

// positions per tile of the window walk: one LDS counter per position and direction (2 * CLIP_TILE * 4 bytes per wave)
constexpr int CLIP_TILE = 1024;

struct ClipBufs
{
  DevBuf samp, res, stat;
};

// per (call, side) wave, written only when a byte model is wanted: records visited (a record that two neighbouring tiles look at
// counts twice), CIGAR words read, tiles walked
struct ClipStat
{
  uint32_t visited, words, tiles, pad;
};

// out[c] = the sixteen counts of row c of `cl` (BK_STAGE_CLUSTERS order) on the record table `rec` (aux_off set; maxspan = its
// max(bam_endpos - pos)).  stat_out (may be null) receives 2 * ncl ClipStat rows, [2 * c + side].  Both are device arrays owned by `b`.
void clip_support(const RecView &rec, int maxspan, const bk_cluster *cl, uint64_t ncl, int mapq_min, int min_clip, double w, ClipBufs &b, hipStream_t st,
                  struct bk_clip_support **out, ClipStat **stat_out);
