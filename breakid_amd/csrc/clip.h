// Interface of clip.hip: soft-clip evidence of every cluster (bk_clip_support) and the clip events at given sites (bk_clip_reads).
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

// ---- bk_clip_reads ----------------------------------------------------------------------------------------------------------------
struct ClipReadBufs
{
  DevBuf samp, sites, counts, counts64, site_off, rows, stat, bad, scan_tmp;
};

// where a listed row takes the read-name hashes of its record from: the bk_side row when the table has one, the columns otherwise
// (qcheck may be null); all null for a call that asks for the counts only
struct ClipNames
{
  const bk_side *side;
  const uint64_t *qhash;
  const uint32_t *qcheck;
};

// device arrays owned by the ClipReadBufs: counts[n_sites]; with a listing site_off[n_sites + 1] and rows[n_rows]; stat[n_sites]
// (visited and words of the count pass; the emit pass walks the same records) when asked for.  bad: the listing did not fill
// exactly the ranges of site_off (an internal error; the caller reports it).
struct ClipReadsOut
{
  uint32_t *counts;
  uint64_t *site_off;
  struct bk_clip_read *rows;
  uint64_t n_rows;
  ClipStat *stat;
  bool bad;
};

// `sites` is a host array.  With a listing the call synchronises the stream twice (the row count, then the check); without one it
// only queues the count pass.
void clip_reads(const RecView &rec, const ClipNames &nm, int maxspan, const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, bool listing,
                bool want_stat, ClipReadBufs &b, hipStream_t st, ClipReadsOut &o);
