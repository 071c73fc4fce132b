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
  const int32_t *mtid = nullptr, *mpos = nullptr;  // only the fragment keys read them (EvidenceKeys), and only without `side`
};

// The fragment key of every row (bk_unique_support, include/breakid_hip.h), written by the kernels that list the rows so that
// membership, order and side assignment are stated once.  Four columns of `n` words each at d + j * n, word j of row r:
//   pair   0: p1_pos << 32 | p2_pos   1: 2 * (p1_rev != 0) + (p2_rev != 0)   2: 0
//   split  0: A1_start << 32 | A1_end   1: A2_start << 32 | A2_end   2: mtid << 32 | mpos of record `rec` (A1 = prim unless swapped)
//   both   3: call << 1 | (kind == BK_EV_SPLIT): ascending in r
// evidence() sizes `w` once it knows the row count and leaves `d` and `n` behind; with keys_only the rows themselves are not written.
struct EvidenceKeys
{
  DevBuf w;
  uint64_t *d = nullptr;
  uint64_t n = 0;
  bool keys_only = true;
};

// what the kernels report besides the rows (read back after the call)
struct EvidenceStat
{
  uint32_t bad;      // != 0: a row fell outside the range its call was given, or a `rec` outside the table (nothing is written then)
  uint32_t pad;
  unsigned long long visited;  // tuples the split waves looked at (the byte model)
};

// Rows in their final order (include/breakid_hip.h) in *rows_out, call_off_out[ncl + 1] over the rows of `cl` (BK_STAGE_CLUSTERS
// order: bp.hip, cluster_summary), both device arrays owned by `b`.  *stat_out: device, one entry.  keys != nullptr: the fragment
// keys as well (above).  pairs_only: the BK_EV_PAIR rows alone, same order, packed, so that *call_off_out bounds a call's pair rows;
// the tuples are counted (junctions()) but not listed.
void evidence(const JunctionPairs &p, const TupleTable &tt, const bk_cluster *cl, uint64_t ncl, const EvidenceRecs &recs, EvidenceBufs &b, hipStream_t st,
              struct bk_evidence **rows_out, uint64_t **call_off_out, EvidenceStat **stat_out, EvidenceKeys *keys = nullptr, bool pairs_only = false);
