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

// ---- the event rule, shared by clip.hip and cliploci.hip ---------------------------------------------------------------------------
constexpr uint16_t CLIP_FLAG_NEVER = 0x4 | 0x100 | 0x200 | 0x400 | 0x800;
constexpr uint32_t CIGAR_S = 4, CIGAR_H = 5;

__device__ __forceinline__ bool cigar_op_ref(uint32_t word) { return ((0x3C1A7u >> ((word & 15u) << 1)) & 2u) && (word >> 4); }

// The clip events of record i, whose flag, mapq and aux columns have passed: `lead` (at pos + 1) and `trail` (at *pt = bam_endpos).
// The first and the last CIGAR word decide (and the words behind hard clips); the whole CIGAR is walked only for a record with a
// trailing clip that qualifies, or with a leading one that no aligned base follows at once (the reference length must be > 0).
// len_lead / len_trail: the lengths of the two S ops (of use where the event is set).
__device__ __forceinline__ void clip_events(const RecView &r, uint64_t i, int32_t pos, int min_clip, bool &lead, bool &trail, long long &pt, uint32_t &words,
                                            uint32_t &len_lead, uint32_t &len_trail)
{
  lead = trail = false;
  pt = 0;
  len_lead = len_trail = 0;
  const uint32_t c0 = r.cigar_off[i], c1 = r.cigar_off[i + 1];
  words += 2;
  if (c1 <= c0) return;
  const uint32_t *__restrict__ cg = r.cigar;
  uint32_t a = c0, z = c1 - 1;
  uint32_t wa = cg[a], wz = cg[z];
  words += 2;
  while ((wa & 15u) == CIGAR_H && a < z) wa = cg[++a], ++words;
  while ((wz & 15u) == CIGAR_H && z > a) wz = cg[--z], ++words;
  const bool l = (wa & 15u) == CIGAR_S && (long long) (wa >> 4) >= min_clip;
  const bool t = (wz & 15u) == CIGAR_S && (long long) (wz >> 4) >= min_clip;
  if (!l && !t) return;
  len_lead = wa >> 4;
  len_trail = wz >> 4;
  if (!t && a + 1 < c1 && cigar_op_ref(cg[a + 1]))
  {
    ++words;
    lead = true;
    return;
  }
  const int32_t len = cigar_reflen_hts(cg + c0, c1 - c0);
  words += c1 - c0;
  if (len <= 0) return;
  lead = l;
  trail = t;
  pt = (long long) pos + len;
}
