// Interface of sjcall.hip: junction calls from the split-evidence tuples alone (bk_split_junctions).
#pragma once
#include "bk_common.h"
#include "prims.h"

struct SjBufs
{
  DevBuf flag, tup, sorted, keys, vals, head, qhead, ex, xid, xstart, xrow, label, changed, xlist, cstart_x, cstart_t, claim, rows, keep, out, counts;
  DevBuf cent;  // the voted rows' breakpoints, sorted by the host
  DevBuf scan_tmp;
  prims::RadixBufs radix;
};

// the context's tuples, the two record columns the definition reads, and the reference list
struct SjInput
{
  const bk_split *split = nullptr;
  uint64_t n = 0;
  const uint16_t *flag = nullptr;
  const uint8_t *mapq = nullptr;
  uint64_t n_rec = 0;
  const uint32_t *tprefix = nullptr;  // nt + 1 prefix sums of the contig lengths (modulo 2^32: only differences are used)
  int nt = 0;
  uint32_t max_len = 0;  // the longest contig
};

// one end pair of a voted row, as the claimed-row search reads it: key = ((tid_a + 1) << 32) | pos_a, code = 2 * row + crossed.
// Sorted ascending by (key, code) by the caller.
struct SjClaim
{
  uint64_t key;
  int32_t tid_b;
  uint32_t pos_b, code, pad;
};

struct SjStats
{
  uint64_t n = 0, eligible = 0, exact = 0, calls = 0, claimed = 0, rounds = 0, written = 0;
  int pos_bits = 0, group_bits = 0;
  uint64_t touched() const;  // the byte model of include/breakid_hip.h
};

// Queues the kernels on `st` and waits for it where the host needs a count (eligible tuples, exact junctions, the changed flag of a
// round, calls, rows).  Throws BK_ERR_LIMIT beyond 2^30 eligible tuples and when the components need more than x + 1 rounds (x exact junctions).
// Device array owned by `b`: rows[stats.written].
void split_junctions(const SjInput &in, int mapq_min, uint32_t tol, uint32_t min_reads, const SjClaim *claims, uint64_t n_claims, SjBufs &b, hipStream_t st,
                     struct bk_split_junction **rows, SjStats *stats);
