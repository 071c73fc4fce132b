// Interface of seqcx.hip: what the reference looks like at one position (bk_site_complexity): soft-mask, trinucleotides, tandem tracts.
#pragma once
#include "refseq_dev.h"

struct SeqcxBufs
{
  // the reference and the sites, uploaded per call
  RefseqBufs ref;
  DevBuf sites;
  DevBuf res;
  const struct bk_ref_site *d_sites = nullptr;
};

// `ref` and `sites` are host arrays that the caller has checked (include/breakid_hip.h: the segments ascend and do not overlap, every
// off span holds its bases, 1 <= flank <= 255, 1 <= max_period <= 64).  seqcx_upload queues the copies into `b` (the caller times
// site_complexity alone, the work on the device copy); site_complexity queues one kernel on `st`.  Device array owned by `b`: res[n].
void seqcx_upload(const bk_refseq &ref, const struct bk_ref_site *sites, uint64_t n, SeqcxBufs &b, hipStream_t st);
void site_complexity(uint64_t n, uint32_t flank, uint32_t max_period, SeqcxBufs &b, hipStream_t st, struct bk_site_cplx **res);
