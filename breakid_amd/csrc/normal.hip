// Matched-normal evidence of every tumour cluster (bk_normal_support): how many of the normal's discordant
// pairs fall into the cluster's window, how many of its split-evidence tuples carry the voted breakpoint pair, and the normal's
// single-base depth at both breakpoints.  The normal has only been through the record-level stages (stream pass, mate join,
// split evidence); its pairs are indexed here by (chromosome pair, p1_pos) with the library's radix sort, and every count is a
// wave-wide window search - one wavefront per tumour cluster, as in bp.hip.
#include "normal.h"
#include "tuple_match.h"

namespace
{
// the orientation bit of one pair, exactly as k_accumulate (bp.hip) folds it into a cluster's type_mask
__device__ __forceinline__ uint32_t pair_type(const bk_pair &pr)
{
  uint32_t type = 0;
  if (pr.p1_tid != pr.p2_tid)
    type = BK_TYPE_DIFF_CHR;
  else
  {
    if (pr.p1_rev && !pr.p2_rev) type |= BK_TYPE_ABS_REVERSE;
    if (pr.p1_rev == pr.p2_rev) type |= BK_TYPE_SAME_ORIENT;
    if (!pr.p1_rev && pr.p2_rev) type |= BK_TYPE_DEFAULT_ORIENT;
  }
  return type;
}
__device__ __forceinline__ unsigned long long numeric_key(int32_t t1, int32_t t2, int32_t nt)
{
  return (unsigned long long) (uint32_t) (t1 + 1) * (unsigned long long) (nt + 1) + (unsigned long long) (uint32_t) (t2 + 1);
}
__device__ __forceinline__ unsigned long long tid_pair(int32_t t1, int32_t t2) { return ((unsigned long long) (uint32_t) (t1 + 1) << 32) | (uint32_t) (t2 + 1); }

// ---- pair index: sorted 64-bit keys (group << 32 | p1_pos) and one (p2_pos, orientation bit) row per key -----------------------
// group = the numeric chromosome-pair key while it fits in 32 bits (nt < 65535) ...
__global__ __launch_bounds__(256) void k_keys_numeric(const bk_pair *__restrict__ pairs, uint64_t n, int32_t nt, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
  const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bk_pair p = pairs[i];
  key[i] = (numeric_key(p.p1_tid, p.p2_tid, nt) << 32) | p.p1_pos;
  val[i] = (uint32_t) i;
}
// ... else the dense rank of the (p1_tid, p2_tid) pair: a sort by p1_pos, a stable sort by the 64-bit tid pair, a scan of the
// first element of every tid pair
__global__ __launch_bounds__(256) void k_keys_pos(const bk_pair *__restrict__ pairs, uint64_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
  const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  key[i] = pairs[i].p1_pos;
  val[i] = (uint32_t) i;
}
__global__ __launch_bounds__(256) void k_keys_tidpair(const bk_pair *__restrict__ pairs, const uint32_t *__restrict__ vin, uint64_t n, uint64_t *__restrict__ key,
                                                      uint32_t *__restrict__ val)
{
  const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t v = vin[j];
  key[j] = tid_pair(pairs[v].p1_tid, pairs[v].p2_tid);
  val[j] = v;
}
__global__ __launch_bounds__(256) void k_tp_flags(const uint64_t *__restrict__ tp, uint64_t n, uint32_t *__restrict__ flag)
{
  const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) flag[j] = (j == 0 || tp[j] != tp[j - 1]) ? 1u : 0u;
}
// gtab[rank] = the tid pair of that rank (ascending); key[j] = rank << 32 | p1_pos
__global__ __launch_bounds__(256) void k_tp_rank(const uint64_t *__restrict__ tp, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ scan,
                                                 const uint32_t *__restrict__ v, const bk_pair *__restrict__ pairs, uint64_t n, uint64_t *__restrict__ key,
                                                 unsigned long long *__restrict__ gtab)
{
  const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t rank = scan[j] + flag[j] - 1u;
  if (flag[j]) gtab[rank] = tp[j];
  key[j] = ((uint64_t) rank << 32) | pairs[v[j]].p1_pos;
}
__global__ __launch_bounds__(256) void k_rows(const bk_pair *__restrict__ pairs, const uint32_t *__restrict__ v, uint64_t n, uint2 *__restrict__ rows)
{
  const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const bk_pair p = pairs[v[j]];
  rows[j] = make_uint2(p.p2_pos, pair_type(p));
}

// ---- n_drp: one wave per tumour cluster --------------------------------------------------------------------------------------
// [lo, hi) = the rows of the cluster's chromosome pair with p1_pos in [p1_min - W, p1_max + W] (wave-wide lower bounds on the keys);
// the rows in between are tested on p2_pos and the orientation bit, 64 per ballot and four ballots' loads in flight at once: a dense
// same-chromosome group puts thousands of rows into one window.
constexpr int DRP_STEPS = 4;
__global__ __launch_bounds__(256) void k_normal_drp(const uint64_t *__restrict__ keys, const uint2 *__restrict__ rows, uint64_t nrows, int dense,
                                                    const unsigned long long *__restrict__ gtab, const uint32_t *__restrict__ ngtab_dev, int32_t nt,
                                                    const bk_cluster *__restrict__ cl, uint32_t ncl, int W, struct bk_normal_support *__restrict__ res,
                                                    uint32_t *__restrict__ voted)
{
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= ncl) return;
  const bk_cluster k = cl[c];
  uint32_t n = 0;
  const long long a1 = (long long) k.p1_min - W, b1 = (long long) k.p1_max + W;  // signed 64-bit window bounds
  const long long a2 = (long long) k.p2_min - W, b2 = (long long) k.p2_max + W;
  bool have = nrows > 0 && a1 <= b1 && b1 >= 0 && a1 <= 0xFFFFFFFFll && a2 <= b2;
  unsigned long long g = 0;
  if (have && !dense)
    g = numeric_key(k.p1_tid, k.p2_tid, nt);
  else if (have)
  {
    const uint32_t ng = *ngtab_dev;
    const unsigned long long tp = tid_pair(k.p1_tid, k.p2_tid);
    g = wave_lower(0, ng, [&](uint64_t m) { return gtab[m] < tp; });
    have = g < ng && gtab[g] == tp;
  }
  if (have)
  {
    const uint64_t klo = (g << 32) | (uint64_t) (a1 < 0 ? 0 : a1);
    const uint64_t khi = (g << 32) | (uint64_t) (b1 > 0xFFFFFFFFll ? 0xFFFFFFFFll : b1);
    const uint64_t lo = wave_lower(0, nrows, [&](uint64_t m) { return keys[m] < klo; });
    const uint64_t hi = wave_lower(lo, nrows, [&](uint64_t m) { return keys[m] <= khi; });
    for (uint64_t base = lo; base < hi; base += DRP_STEPS * 64)
    {
      uint2 r[DRP_STEPS];
#pragma unroll
      for (int s = 0; s < DRP_STEPS; ++s)
      {
        const uint64_t i = base + (uint64_t) s * 64 + lane;
        r[s] = i < hi ? rows[i] : make_uint2(0u, 0u);  // type 0 never intersects a mask
      }
#pragma unroll
      for (int s = 0; s < DRP_STEPS; ++s)
      {
        const bool hit = (r[s].y & k.type_mask) && (long long) r[s].x >= a2 && (long long) r[s].x <= b2;
        n += (uint32_t) __popcll(__ballot(hit));
      }
    }
  }
  if (lane == 0)
  {
    struct bk_normal_support o;
    o.n_drp = n;
    o.n_sr = o.depth1 = o.depth2 = 0;
    res[c] = o;
    voted[c] = (k.flags & 2u) ? 1u : 0u;
  }
}

// ---- n_sr: one wave per voted cluster -----------------------------------------------------------------------------------------
// (the range construction and the match: tuple_match.h, shared with bk_junctions)
__global__ __launch_bounds__(256) void k_normal_sr(TupleTable tt, const bk_cluster *__restrict__ cl, uint32_t ncl, struct bk_normal_support *__restrict__ res)
{
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= ncl) return;
  const bk_cluster k = cl[c];
  if (!(k.flags & 2u)) return;
  uint32_t n = 0;
  for_matching_tuples(tt, k, [&](const bk_split &, bool) { ++n; });
  n = wave_sum(n);
  if (lane == 0) res[c].n_sr = n;
}

// depth1/depth2: bp_depth_partial's counts (k_bp_depth / base_depth_wave on the normal's records)
__global__ __launch_bounds__(256) void k_normal_depth(const uint32_t *__restrict__ depth, uint32_t ncl, struct bk_normal_support *__restrict__ res)
{
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncl) return;
  res[c].depth1 = depth[2 * c];
  res[c].depth2 = depth[2 * c + 1];
}
}  // namespace

static inline unsigned nb(uint64_t n) { return cdiv(n ? n : 1, 256); }

void normal_support(const NormalSide &n, const bk_cluster *cl, uint64_t ncl, double w, NormalBufs &b, hipStream_t st, struct bk_normal_support **out)
{
  struct bk_normal_support *res = b.res.as<struct bk_normal_support>(ncl + 1);
  uint32_t *voted = b.bb.voted.as<uint32_t>(ncl + 1);
  *out = res;
  if (ncl == 0) return;
  if (ncl > 0x7FFFFFFFull) throw bk_error(BK_ERR_LIMIT, "too many clusters");
  const int W = (int) w;  // the integer the breakpoint stage passes as wi (bp.hip: bp_vote)
  const uint64_t np = n.n_pairs;
  const int32_t nt = n.tuples.nt;
  const bool dense = nt >= 65535;  // (nt + 1)^2 no longer fits in the 32 high bits of a key
  const uint64_t *keys = nullptr;
  const uint2 *rows = nullptr;
  const unsigned long long *gtab = nullptr;
  const uint32_t *ngtab = nullptr;
  if (np)
  {
    uint64_t *k0 = b.key.as<uint64_t>(np), *ks;
    uint32_t *v0 = b.val.as<uint32_t>(np), *vs;
    if (!dense)
    {
      int gbits = 1;
      while ((1ull << gbits) < (uint64_t) (nt + 1) * (uint64_t) (nt + 1)) ++gbits;
      hipLaunchKernelGGL(k_keys_numeric, dim3(nb(np)), dim3(256), 0, st, n.pairs, np, nt, k0, v0);
      prims::radix_sort_pairs(k0, v0, np, 0, 32 + gbits, b.radix, st, &ks, &vs);
    }
    else
    {
      hipLaunchKernelGGL(k_keys_pos, dim3(nb(np)), dim3(256), 0, st, n.pairs, np, k0, v0);
      prims::radix_sort_pairs(k0, v0, np, 0, 32, b.radix, st, &ks, &vs);
      uint64_t *k1 = b.key2.as<uint64_t>(np);
      uint32_t *v1 = b.val2.as<uint32_t>(np);
      hipLaunchKernelGGL(k_keys_tidpair, dim3(nb(np)), dim3(256), 0, st, n.pairs, vs, np, k1, v1);
      int tbits = 1;
      while ((1ull << tbits) <= (uint64_t) nt) ++tbits;  // p1_tid + 1 <= nt
      prims::radix_sort_pairs(k1, v1, np, 0, 32 + tbits, b.radix, st, &ks, &vs);
      uint32_t *flag = b.flag.as<uint32_t>(np + 1), *scan = b.rank.as<uint32_t>(np + 1);
      hipLaunchKernelGGL(k_tp_flags, dim3(nb(np)), dim3(256), 0, st, ks, np, flag);
      prims::exclusive_scan<uint32_t>(flag, scan, np, b.radix.scan_tmp, st);
      unsigned long long *gt = b.gtab.as<unsigned long long>(np);
      hipLaunchKernelGGL(k_tp_rank, dim3(nb(np)), dim3(256), 0, st, ks, flag, scan, vs, n.pairs, np, k0, gt);  // (k0 is free after the second sort)
      ks = k0;
      gtab = gt;
      ngtab = scan + np;
    }
    uint2 *rw = b.rows.as<uint2>(np);
    hipLaunchKernelGGL(k_rows, dim3(nb(np)), dim3(256), 0, st, n.pairs, vs, np, rw);
    keys = ks;
    rows = rw;
  }
  hipLaunchKernelGGL(k_normal_drp, dim3(cdiv(ncl, 4)), dim3(256), 0, st, keys, rows, np, dense ? 1 : 0, gtab, ngtab, nt, cl, (uint32_t) ncl, W, res, voted);
  hipLaunchKernelGGL(k_normal_sr, dim3(cdiv(ncl, 4)), dim3(256), 0, st, n.tuples, cl, (uint32_t) ncl, res);
  const uint32_t *depth = bp_depth_partial(n.rec, cl, ncl, n.tuples.maxspan, b.bb, st);
  hipLaunchKernelGGL(k_normal_depth, dim3(nb(ncl)), dim3(256), 0, st, depth, (uint32_t) ncl, res);
}
