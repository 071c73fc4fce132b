// Interface of locsim.hip: the reference around the two breakpoints of a call compared with itself (bk_locus_similarity).
#pragma once
#include "refseq_dev.h"

struct LocsimBufs
{
  // the reference and the pairs, uploaded per call
  RefseqBufs ref;
  DevBuf pairs;
  DevBuf res;
  const struct bk_locus_pair *d_pairs = nullptr;
};

// `ref` and `pairs` are host arrays that the caller has checked (include/breakid_hip.h: the segments ascend and do not overlap, every
// off span holds its bases, 1 <= flank <= 255).  locsim_upload queues the copies into `b` (the caller times locus_similarity alone,
// the work on the device copy); locus_similarity queues one kernel on `st`.  Device array owned by `b`: res[n].
void locsim_upload(const bk_refseq &ref, const struct bk_locus_pair *pairs, uint64_t n, LocsimBufs &b, hipStream_t st);
void locus_similarity(uint64_t n, uint32_t flank, LocsimBufs &b, hipStream_t st, struct bk_locus_sim **res);
