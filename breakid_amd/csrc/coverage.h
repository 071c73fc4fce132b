// Interface of coverage.hip: the aligned bases inside arbitrary windows of the record table (bk_window_coverage).
#pragma once
#include "bp.h"

constexpr uint32_t COV_TILE_SHIFT = 8;  // a tile is 256 records: one wavefront, four records per lane

struct CovBufs
{
  DevBuf samp, len, cnt, scan_tmp, win, res;
};

// Tiles of a table of n records, and the entries of each prefix array (one more: the total)
static inline uint64_t cov_tiles(uint64_t n) { return (n + (1ull << COV_TILE_SHIFT) - 1) >> COV_TILE_SHIFT; }

// cov_tiles_build queues the tile pass and the two scans on `st`: b.len / b.cnt then hold, per tile, the eligible reference length and
// the eligible records in front of it (cov_tiles(n) + 1 entries each).  window_coverage queues the window kernel over the n device
// rows b.win; device array owned by `b`: res[n].  The caller has checked the windows (reserved == 0) and n <= 2^30.
void cov_tiles_build(const RecView &rec, int mapq_min, CovBufs &b, hipStream_t st);
void window_coverage(const RecView &rec, int32_t n_targets, int maxspan, uint64_t n, int mapq_min, CovBufs &b, hipStream_t st, struct bk_window_cov **res);
