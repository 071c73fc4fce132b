// The tuple search shared by bk_normal_support's n_sr (normal.hip), bk_junctions' splits[] (junction.hip) and bk_evidence's split rows
// (evidence.hip): the split-evidence tuples that carry a voted cluster's breakpoint pair.  One wavefront per cluster; every lane calls with the same arguments.
#pragma once
#include "bk_common.h"
#include "bp.h"

__device__ __forceinline__ bool near2(uint32_t bp, long long exact)
{
  const long long d = (long long) bp - exact;
  return d >= -2 && d <= 2;
}
// first tuple with (tid, pos) >= (T, P): the tuples are in record order = coordinate order (bp.hip: split_lower_pos)
__device__ __forceinline__ uint64_t tuple_lower(const bk_split *__restrict__ sp, uint64_t ns, int32_t T, long long P)
{
  const uint32_t Tu = (uint32_t) T;
  return wave_lower(0, ns, [&](uint64_t m) {
    const uint32_t t = (uint32_t) sp[m].tid;
    return t != Tu ? (t < Tu) : ((long long) sp[m].pos < P);
  });
}
// The record-ordered tuples of one context and what the search needs of its header (api.hip: tuple_table).
struct TupleTable
{
  const bk_split *sp;
  uint64_t n;
  int maxspan;            // max(bam_endpos - pos) of the context's records
  const int32_t *hdr_id;  // interned chromosome id per tid + 1 (the vote's p1_chr, bp.hip: k_bp_vote)
  const int32_t *own_id;  // per tid: interned id a tuple of a record on that tid carries for its own side (stream.hip: own_chr)
  int32_t nt, empty_id;   // ... and for a record outside the header's nt entries
};
// Only tuples whose own record lies on the call's chromosomes (p1_tid, p2_tid) count: the tuples the vote itself looks at.  A
// matching tuple's own alignment carries one of its two breakpoints (prim_* of a primary record, sec_* of a 0x100 one,
// stream.hip), and that breakpoint lies inside the alignment: the record starts in [e - 2 - maxspan, e + 2] around the exact
// breakpoint e it is compared with.  The own side's chromosome id is own_id[tid] (the reference's chromID2ChrName of the tid), so
// a record on chromosome T can stand for p1 (around p1_exact) when own_id[T] == c1 and for p2 (around p2_exact) when own_id[T] ==
// c2: up to four ranges, (p1_tid | p2_tid) x (p1_exact | p2_exact); two for a header that lists chr1..chr22, chrX, chrY first and
// in that order (own_id[T] == c(T)).  The ranges may overlap: whoever walks them visits a tuple once.
// The up to four index ranges of a cluster (empty: lo == hi) and the interned ids of its two chromosomes.
struct TupleRanges
{
  uint64_t lo[4], hi[4];
  int32_t c1, c2;
};
__device__ __forceinline__ TupleRanges tuple_ranges(const TupleTable &tt, const bk_cluster &k)
{
  TupleRanges r;
  const long long e1 = (long long) k.p1_exact, e2 = (long long) k.p2_exact;
  r.c1 = tt.hdr_id[k.p1_tid + 1];  // interned chromosome ids, as the vote compares them (k_bp_vote)
  r.c2 = tt.hdr_id[k.p2_tid + 1];
#pragma unroll
  for (int q = 0; q < 4; ++q)
  {
    const int32_t T = (q >> 1) ? k.p2_tid : k.p1_tid;  // the tuple's own record lies on T ...
    const long long e = (q & 1) ? e2 : e1;           // ... and its own breakpoint is compared with e
    const int32_t own = (T >= 0 && T < tt.nt) ? tt.own_id[T] : tt.empty_id;
    const bool on = own == ((q & 1) ? r.c2 : r.c1) && !((q >> 1) && k.p1_tid == k.p2_tid);  // (one chromosome: q = 2, 3 repeat q = 0, 1)
    r.lo[q] = r.hi[q] = 0;
    if (on)
    {
      r.lo[q] = tuple_lower(tt.sp, tt.n, T, e - 2 - tt.maxspan);
      r.hi[q] = tuple_lower(tt.sp, tt.n, T, e + 3);
    }
  }
  return r;
}
// 0: the tuple does not carry the breakpoint pair; 1: (prim, sec) is (p1, p2); 2: it is (p2, p1) and not also (p1, p2)
__device__ __forceinline__ int tuple_side(const bk_split &s, const TupleRanges &r, const bk_cluster &k)
{
  if (s.flags & 2u) return 0;  // "error cigar" tuple
  const long long e1 = (long long) k.p1_exact, e2 = (long long) k.p2_exact;
  const int32_t pc = s.prim_chr, sc = s.sec_chr;
  const uint32_t pb = s.prim_bp, sb = s.sec_bp;
  if (pc == r.c1 && sc == r.c2 && near2(pb, e1) && near2(sb, e2)) return 1;
  if (pc == r.c2 && sc == r.c1 && near2(pb, e2) && near2(sb, e1)) return 2;
  return 0;
}
// The clip sides of a matching tuple as a strand-bin index 2 * side1 + side2: a side is right (1) when its breakpoint is the
// alignment's start (a leading clip), else left; side 1 is prim unless the tuple names the pair the other way round.
__device__ __forceinline__ uint32_t split_sides(const bk_split &s, bool swapped)
{
  const uint32_t rp = s.prim_bp == s.prim_start ? 1u : 0u, rs = s.sec_bp == s.sec_start ? 1u : 0u;
  return swapped ? 2u * rs + rp : 2u * rp + rs;
}
// Walks the ranges, a range skipping the indices of the ranges before it.  `hit(s, swapped)` runs on the lane that holds a matching
// tuple s: swapped == false when (prim, sec) is (p1, p2), true when it is (p2, p1) and not also (p1, p2).  Returns the number of
// tuples the wave looked at (the same value on every lane).
template <class Hit> __device__ __forceinline__ uint32_t for_matching_tuples(const TupleTable &tt, const bk_cluster &k, Hit hit)
{
  const int lane = threadIdx.x & 63;
  const TupleRanges r = tuple_ranges(tt, k);
  uint32_t visited = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
  {
    visited += r.hi[q] > r.lo[q] ? (uint32_t) (r.hi[q] - r.lo[q]) : 0u;
    for (uint64_t t = r.lo[q] + lane; t < r.hi[q]; t += 64)
    {
      bool seen = false;
#pragma unroll
      for (int p = 0; p < q; ++p) seen |= t >= r.lo[p] && t < r.hi[p];
      if (seen) continue;
      const bk_split &s = tt.sp[t];
      const int side = tuple_side(s, r, k);
      if (side) hit(s, side == 2);
    }
  }
  return visited;
}
