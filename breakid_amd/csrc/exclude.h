// Interface of exclude.hip (bk_exclude_regions: the records that overlap excluded intervals taken out of a context's table).
#pragma once
#include <functional>

#include "bk_common.h"

// merged exclude intervals on the device: those of contig t are [beg[k], end[k]) for k in [off[t], off[t + 1]), sorted and disjoint
struct ExclRegions
{
  const uint32_t *off;  // n_targets + 1
  const int32_t *beg, *end;
  int32_t n_targets;
};

// Stable, out-of-place compaction of `src` (device columns, the layout bk_upload_records demands of device tables) to the records
// that overlap no interval of `rg` (tid == T && pos < end && bam_endpos > beg).  dst[0..12] receive tid, pos, mtid, mpos, isize, flag,
// mapq, qhash, cigar_off, cigar, aux_off, aux, qcheck (the order of bk_ctx::col), each 16-byte aligned with a 16-byte tail pad;
// `out` describes the new table (side = nullptr: the caller makes the rows).  Synchronises the stream once (the kept counts size
// the outputs).  `tick(name, bytes, begin)` brackets the steps for the context's timers; `bytes` = what the step's kernels load + store.
void exclude_compact(const bk_soa &src, const ExclRegions &rg, DevBuf dst[13], bk_soa &out, hipStream_t st,
                     const std::function<void(const char *, uint64_t, bool)> &tick);
