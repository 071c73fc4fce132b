// Interface of evidence.hip: the reads behind every call (bk_evidence).
#pragma once
#include "bk_common.h"
#include "bp.h"
#include "junction.h"

struct EvidenceBufs
{
  JunctionBufs jn;  // the counts come from junctions() itself (junction.hip)
  DevBuf cnt, npair, call_off, pair_off, keys, vals, rows, stat, scan_tmp;
  prims::RadixBufs radix;
};

// The columns a row gathers at `rec`: the read-name hashes of a pair row (from the bk_side row when the table has one, from the
// columns otherwise; qcheck may be null) and the mapq of a split row.
struct EvidenceRecs
{
  uint64_t n;
  const bk_side *side;
  const uint64_t *qhash;
  const uint32_t *qcheck;
  const uint8_t *mapq;
};

// what the kernels report besides the rows (read back after the call)
struct EvidenceStat
{
  uint32_t bad;      // != 0: a row fell outside the range its call was given, or a `rec` outside the table (nothing is written then)
  uint32_t pad;
  unsigned long long visited;  // tuples the split waves looked at (the byte model)
};

// Rows in their final order (include/breakid_hip.h) in *rows_out, call_off_out[ncl + 1] over the rows of `cl` (BK_STAGE_CLUSTERS
// order: bp.hip, cluster_summary), both device arrays owned by `b`.  *stat_out: device, one entry.
void evidence(const JunctionPairs &p, const TupleTable &tt, const bk_cluster *cl, uint64_t ncl, const EvidenceRecs &recs, EvidenceBufs &b, hipStream_t st,
              struct bk_evidence **rows_out, uint64_t **call_off_out, EvidenceStat **stat_out);
