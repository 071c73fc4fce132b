// Interface of jfit.hip: the voted sequence of a breakpoint side fitted to the reference at the other side (bk_junction_fit).
#pragma once
#include "refseq_dev.h"

struct JfitBufs
{
  // the reference, the probes and the queries, uploaded per call
  RefseqBufs ref;
  DevBuf probes, query;
  DevBuf res;
  const struct bk_junction_probe *d_probes = nullptr;
  const uint8_t *d_query = nullptr;
};

// `ref`, `probes` and `query` are host arrays that the caller has checked (include/breakid_hip.h: the segments ascend and do not
// overlap, every off span holds its bases, dir <= 1, qlen <= max_len <= 256, the three maxima <= 64).  jfit_upload queues the copies
// into `b` (the caller times junction_fit alone, the work on the device copy); junction_fit queues one kernel on `st`.
// Device array owned by `b`: res[n].
void jfit_upload(const bk_refseq &ref, const struct bk_junction_probe *probes, uint64_t n, const uint8_t *query, uint32_t max_len, JfitBufs &b, hipStream_t st);
void junction_fit(uint64_t n, uint32_t max_len, uint32_t max_shift, uint32_t max_ins, uint32_t max_hom, JfitBufs &b, hipStream_t st, struct bk_junction_fit **res);
