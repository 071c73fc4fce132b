// Interface of bp.hip (cluster summary + split-read breakpoint stage).
#pragma once
#include "bk_common.h"
#include "prims.h"
#include "wave.h"

// Lower bound by a whole wavefront: every lookup of bp.hip and normal.hip is made by all 64 lanes of a wave with the same arguments (one
// wave per cluster), and a binary search is a chain of dependent memory round trips - 30 of them for a record lookup, ~22 for
// a tuple lookup, the better part of k_bp_cov / k_bp_regions / k_bp_depth.  64 probes per round trip cut the range 65-fold:
// `less(i)` = "element i orders before the target" (monotone over [lo, hi)); returns the first index for which it is false.
template <class Less> __device__ __forceinline__ uint64_t wave_lower(uint64_t lo, uint64_t hi, Less less)
{
  const uint32_t lane = threadIdx.x & 63;
  while (hi - lo > 64)
  {
    const uint64_t width = hi - lo;
    const uint64_t p = lo + width * (lane + 1) / 65;  // lo < p < hi
    const uint32_t c = (uint32_t) __popcll(__ballot(less(p)));  // the probes that order before the target are a prefix of the lanes
    const uint64_t nlo = c ? lo + width * c / 65 + 1 : lo;
    const uint64_t nhi = c < 64 ? lo + width * (c + 1) / 65 : hi;
    lo = nlo;
    hi = nhi;
  }
  const uint64_t i = lo + lane;
  return lo + (uint64_t) __popcll(__ballot(i < hi && less(i)));
}

struct ClusterAcc
{
  uint32_t *n;
  unsigned long long *sum1, *sum2;
  uint32_t *min1, *max1, *min2, *max2, *type;
};

// device view of the record columns the region queries touch
struct RecView
{
  uint64_t n;
  const int32_t *tid, *pos;
  const uint16_t *flag;
  const uint8_t *mapq;
  const uint32_t *cigar_off, *cigar;
  const unsigned long long *samp = nullptr;  // search keys of every 1024th record (rec_lower), or null
  uint64_t n_samp = 0;
  const int32_t *isize = nullptr;     // the two columns only bk_ref_support reads (genotype.hip)
  const uint32_t *aux_off = nullptr;
};

// first record index with (tid,pos) >= (T,P) in coordinate order (unmapped tid=-1 sorts last).  A search over the whole table
// is ~30 dependent HBM round trips per region; with the sampled keys of every REC_SAMPLE-th record (5 MB for 620 M records:
// cache resident) the first ~20 steps stay in the cache and only the last 10 touch the record columns.
constexpr uint32_t REC_SAMPLE_SHIFT = 10;
__device__ __forceinline__ unsigned long long rec_key(int32_t tid, long long pos) { return ((unsigned long long) (uint32_t) tid << 32) | (uint32_t) (pos + 0x80000000ll); }
__device__ inline uint64_t rec_lower(const RecView &r, int32_t T, long long P)
{
  uint64_t lo = 0, hi = r.n;
  if (r.samp)
  {
    // samp[j] = key of record j << REC_SAMPLE_SHIFT; first sample >= target bounds the answer to one stride
    const unsigned long long want = rec_key(T, P < -0x80000000ll ? -0x80000000ll : P);
    const unsigned long long *__restrict__ samp = r.samp;
    const uint64_t a = wave_lower(0, r.n_samp, [&](uint64_t m) { return samp[m] < want; });
    lo = a ? ((a - 1) << REC_SAMPLE_SHIFT) + 1 : 0;  // record (a-1)<<shift is < target, record a<<shift is >= target
    hi = a < r.n_samp ? (a << REC_SAMPLE_SHIFT) : r.n;
  }
  const uint32_t Tu = (uint32_t) T;
  return wave_lower(lo, hi, [&](uint64_t m) {
    const uint32_t t = (uint32_t) r.tid[m];
    return t != Tu ? (t < Tu) : ((long long) r.pos[m] < P);
  });
}

struct BpWork
{
  uint64_t t1lo, t1hi, t2lo, t2hi;
  uint32_t ok, pad;
};

struct BpBufs
{
  DevBuf samp, key, val, kmax, lexbase, slotbase, an, as1, as2, amin1, amax1, amin2, amax2, atype, keep, off, tmpc, work, nmatch, moff, err, emit, ecount, scan_tmp, cov, depth, voted, nvalid, maxrec;
  prims::RadixBufs radix;
};

// clusters with a voted breakpoint pair (flags bit 1), counted on the device
uint64_t count_valid_clusters(const bk_cluster *cl, uint64_t ncl, BpBufs &b, hipStream_t st);
// rec_bits = bits of the largest record index a tuple may carry (the sort key)
void sort_splits(bk_split *unsorted, uint64_t n, bk_split *sorted, BpBufs &b, hipStream_t st, int rec_bits);
// returns the number of clusters that passed the near-diagonal filter; clusters_out holds them in BK_STAGE_CLUSTERS order (the
// invariant: bp.hip).  lex_to_num[l] = numeric index of the group at position l of the context's lexicographic group order.
uint64_t cluster_summary(const bk_pair *pairs, const uint32_t *idx, const uint32_t *gof, const uint32_t *cl, uint64_t n, uint32_t ng, const uint32_t *gkey,
                         const uint32_t *glex, const uint32_t *lex_to_num, int32_t nt, double w, DevBuf &clusters_out, BpBufs &b, hipStream_t st);
// r with the sampled search keys of rec_lower, built into `samp` (tables of fewer than 64 strides are searched directly)
RecView rec_sampled(const RecView &r, DevBuf &samp, hipStream_t st);
// phases of the breakpoint stage (a sharded run sums `cov` and `depth` over the record shards between them)
uint32_t *bp_cov_partial(const RecView &r, const bk_cluster *cl, uint64_t ncl, double w, int maxspan, BpBufs &b, hipStream_t st);
void bp_vote(const bk_split *sp, uint64_t nsp, bk_cluster *cl, uint64_t ncl, double w, int maxspan, const uint32_t *cov, const int32_t *hdr_id, BpBufs &b, hipStream_t st);
uint32_t *bp_depth_partial(const RecView &r, const bk_cluster *cl, uint64_t ncl, int maxspan, BpBufs &b, hipStream_t st);
// cal_single_base_depth (base_depth_wave, the count behind depth1 / depth2) at n arbitrary 1-based positions: tid, pos and depth are
// device arrays of n entries, `samp` backs the sampled search keys
void base_depth_at(const RecView &r, const int32_t *tid, const uint32_t *pos, uint64_t n, int maxspan, DevBuf &samp, hipStream_t st, uint32_t *depth);
void bp_finish(bk_cluster *cl, uint64_t ncl, const uint32_t *depth, BpBufs &b, hipStream_t st);
void split_breakpoints(const RecView &r, const bk_split *sp, uint64_t nsp, bk_cluster *cl, uint64_t ncl, double w, int maxspan, const int32_t *hdr_id, BpBufs &b,
                       hipStream_t st);
// test hook: one raw region through the product's region / verdict / depth device code (res: n tuples, coverage capped at 5, depth, poison)
void debug_region(const RecView &r, const bk_split *sp, uint64_t nsp, int32_t tid, uint32_t start, uint32_t end, int maxspan, unsigned long long depth_pos, bk_split *out,
                  uint32_t cap, uint32_t *res, hipStream_t st);
