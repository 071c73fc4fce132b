// Interface of context.hip: record classes and mapping quality inside arbitrary windows of the record table (bk_window_context).
#pragma once
#include "bp.h"

constexpr uint32_t CTX_TILE_SHIFT = 8;  // a tile is 256 records: one wavefront, four records per lane (the tile of coverage.h)
constexpr uint32_t CTX_ARRAYS = 5;      // prefix arrays per table: mapq_sum, and the eight counts two to a 64-bit word

struct CtxBufs
{
  DevBuf samp, pre, scan_tmp, win, res;
};

// Tiles of a table of n records; every prefix array has one entry more (the total)
static inline uint64_t ctx_tiles(uint64_t n) { return (n + (1ull << CTX_TILE_SHIFT) - 1) >> CTX_TILE_SHIFT; }
// Bytes the tile pass writes per tile: one 64-bit word per prefix array
constexpr uint64_t CTX_TILE_BYTES = 8ull * CTX_ARRAYS;

// ctx_tiles_build queues the tile pass and the scans on `st`: b.pre then holds CTX_ARRAYS arrays of ctx_tiles(n) + 1 prefixes each.
// window_context queues the window kernel over the n device rows b.win; device array owned by `b`: res[n].  The caller has checked
// the windows (reserved == 0) and n <= 2^30.
void ctx_tiles_build(const RecView &rec, int mapq_min, CtxBufs &b, hipStream_t st);
void window_context(const RecView &rec, int32_t n_targets, uint64_t n, int mapq_min, CtxBufs &b, hipStream_t st, struct bk_window_ctx **res);
