// Junction evidence of every cluster (bk_junctions): its member pairs by strand combination with the sums of their
// mapping qualities, and, for a voted cluster, the split-evidence tuples that carry its breakpoint pair by clip side.  Both are
// what a VCF breakend needs to say on which side of each breakpoint the retained sequence lies.  One linear pass over the clustered
// pair list (the shape of k_accumulate, bp.hip) and one wavefront per voted cluster over the tuples (the search of k_normal_sr).
#include "junction.h"
#include "tuple_match.h"
#include <cstddef>

namespace
{
// p1_mapq, p2_mapq, p1_rev, p2_rev are four neighbouring bytes of a pair row: one 32-bit load instead of the 56-byte row
static_assert(offsetof(bk_pair, p1_mapq) % 4 == 0 && offsetof(bk_pair, p2_mapq) == offsetof(bk_pair, p1_mapq) + 1 &&
                  offsetof(bk_pair, p1_rev) == offsetof(bk_pair, p1_mapq) + 2 && offsetof(bk_pair, p2_rev) == offsetof(bk_pair, p1_mapq) + 3 && sizeof(bk_pair) % 4 == 0,
              "bk_pair: the mapq / rev bytes must form one aligned word");
static_assert(sizeof(struct bk_junction) == 48 && offsetof(struct bk_junction, splits) == 16 && offsetof(struct bk_junction, mapq_sum1) == 32, "bk_junction must be 48 bytes");

// A lane per list entry.  A wave holds at most 64 members of one cluster, so the four strand bins travel through the segmented scan
// as four bytes of one word and the two mapq sums (<= 64 * 255) as its two halves; only the last lane of a run of equal slots
// touches the cluster's row (members of a cluster are neighbours in the list, as in k_accumulate).
__global__ __launch_bounds__(256) void k_junction_pairs(JunctionPairs in, uint32_t ncl, struct bk_junction *__restrict__ res)
{
  const uint64_t p = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = p < in.n;
  uint32_t s = 0xFFFFFFFFu, bins = 0, mq = 0;
  if (live)
  {
    const uint32_t word = *reinterpret_cast<const uint32_t *>(&in.pairs[in.idx[p]].p1_mapq);
    s = in.slotbase[in.gof[p]] + in.cl[p];
    const uint32_t r1 = ((word >> 16) & 0xFFu) ? 1u : 0u, r2 = (word >> 24) ? 1u : 0u;
    bins = 1u << (8u * (2u * r1 + r2));
    mq = (word & 0xFFu) | (((word >> 8) & 0xFFu) << 16);
  }
  const uint32_t s_prev = __shfl_up(s, 1, 64), s_next = __shfl_down(s, 1, 64);
  bool head = lane == 0 || s_prev != s;
  const bool tail = lane == 63 || s_next != s;
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint32_t o_bins = __shfl_up(bins, d, 64), o_mq = __shfl_up(mq, d, 64);
    const int o_head = __shfl_up((int) head, d, 64);
    if (lane >= d && !head)
    {
      bins += o_bins;
      mq += o_mq;
      head = o_head != 0;
    }
  }
  if (!live || !tail) return;
  if (s >= in.slotbase[in.ng] || !in.keep[s]) return;  // the cluster did not pass the near-diagonal filter: it has no row
  const uint32_t row = in.off[s];
  if (row >= ncl) return;
  struct bk_junction *o = res + row;
#pragma unroll
  for (int i = 0; i < 4; ++i)
  {
    const uint32_t c = (bins >> (8 * i)) & 0xFFu;
    if (c) atomicAdd(&o->pairs[i], c);
  }
  atomicAdd(reinterpret_cast<unsigned long long *>(&o->mapq_sum1), (unsigned long long) (mq & 0xFFFFu));
  atomicAdd(reinterpret_cast<unsigned long long *>(&o->mapq_sum2), (unsigned long long) (mq >> 16));
}

// One wave per cluster; a voted one searches its tuples and bins every match by the clip sides of its two alignments (tuple_match.h).
__global__ __launch_bounds__(256) void k_junction_sr(TupleTable tt, const bk_cluster *__restrict__ cl, uint32_t ncl, struct bk_junction *__restrict__ res,
                                                     uint32_t *__restrict__ visited)
{
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= ncl) return;
  const bk_cluster k = cl[c];
  uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0, seen = 0;
  if (k.flags & 2u)
  {
    seen = for_matching_tuples(tt, k, [&](const bk_split &s, bool swapped) {
      const uint32_t b = split_sides(s, swapped);
      n0 += b == 0u;
      n1 += b == 1u;
      n2 += b == 2u;
      n3 += b == 3u;
    });
    n0 = wave_sum(n0);
    n1 = wave_sum(n1);
    n2 = wave_sum(n2);
    n3 = wave_sum(n3);
  }
  if (lane == 0)
  {
    // (the row was cleared before the two kernels: k_junction_pairs adds to the other fields, in any order)
    res[c].splits[0] = n0;
    res[c].splits[1] = n1;
    res[c].splits[2] = n2;
    res[c].splits[3] = n3;
    visited[c] = seen;
  }
}
}  // namespace

void junctions(const JunctionPairs &p, const TupleTable &tt, const bk_cluster *cl, uint64_t ncl, JunctionBufs &b, hipStream_t st, struct bk_junction **out,
               uint32_t **visited_out, bool pairs_only)
{
  struct bk_junction *res = b.res.as<struct bk_junction>(ncl + 1);
  uint32_t *visited = b.visited.as<uint32_t>(ncl + 1);
  *out = res;
  *visited_out = visited;
  if (ncl == 0) return;
  if (ncl > 0x7FFFFFFFull) throw bk_error(BK_ERR_LIMIT, "too many clusters");
  HIP_CHECK(hipMemsetAsync(res, 0, ncl * sizeof(struct bk_junction), st));
  if (p.n) hipLaunchKernelGGL(k_junction_pairs, dim3(cdiv(p.n, 256)), dim3(256), 0, st, p, (uint32_t) ncl, res);
  if (pairs_only)  // (no tuple is looked at: the split counts stay 0)
    HIP_CHECK(hipMemsetAsync(visited, 0, ncl * sizeof(uint32_t), st));
  else
    hipLaunchKernelGGL(k_junction_sr, dim3(cdiv(ncl, 4)), dim3(256), 0, st, tt, cl, (uint32_t) ncl, res, visited);
}
