// Junction calls from split reads alone (bk_split_junctions).  One lane per tuple classifies it; a scan compacts the
// eligible ones into 32-byte canonical rows; three stable LSD stages of the radix sort order them by (contigs + sides, pos1, pos2,
// qhash), the first of which also ranks the read hashes so that later keys carry a 30-bit rank instead of 64 bits.  Run heads and
// scans give the exact junctions; one wavefront per exact junction walks its pos1 window 64 a step for the smallest label among its
// near neighbours (min-label propagation with pointer jumping, the rounds counted by the host); a sort of the exact junctions by
// label and one of the tuples by (label, read rank) make every call a contiguous range, which one wavefront reduces.  Integer
// arithmetic only.  Every result word has one writer and no atomic; the labels alone take an integer atomic minimum (a root is hooked
// by whoever finds a smaller label), whose outcome does not depend on the order, and labels only fall.
#include "sjcall.h"
#include "runs.h"

using runs::bits_of;
using runs::NONE;

namespace
{
constexpr int JUMPS = 8;  // pointer jumps of one vertex in one round

struct SjTuple
{
  uint64_t g, qhash;  // g = ((tid1 * n_targets + tid2) << 2) | right1 << 1 | right2
  uint32_t pos1, pos2;
  uint32_t own_mapq;  // own_end << 8 | mapq
  uint32_t qrank;     // dense rank of qhash among the eligible tuples
};
struct SjExact
{
  uint64_t g;
  uint32_t pos1, pos2, n_reads, n_tuples, n_own[2], mapq_sum[2];
};
static_assert(sizeof(SjTuple) == 32 && sizeof(SjExact) == 40 && sizeof(SjClaim) == 24, "row sizes of sjcall.hip");

// ---- classification -----------------------------------------------------------------------------------------------------------------
// The definition of include/breakid_hip.h, one tuple.  Every read is inside its array: tid and the other contig are checked against
// n_targets before tprefix is read, rec against the table's rows before flag and mapq are.
__device__ __forceinline__ bool sj_classify(const SjInput &in, int mapq_min, const bk_split &s, SjTuple &t)
{
  if (s.flags & 2u) return false;
  if (s.tid < 0 || s.tid >= in.nt) return false;
  const bool sec = s.flags & 1u;
  const int32_t other_chr = sec ? s.prim_chr : s.sec_chr;
  if (other_chr < 0 || other_chr >= in.nt) return false;
  const uint32_t own_bp = sec ? s.sec_bp : s.prim_bp, own_start = sec ? s.sec_start : s.prim_start;
  const uint32_t oth_bp = sec ? s.prim_bp : s.sec_bp, oth_start = sec ? s.prim_start : s.sec_start;
  const uint32_t own_len = in.tprefix[s.tid + 1] - in.tprefix[s.tid], oth_len = in.tprefix[other_chr + 1] - in.tprefix[other_chr];
  if (own_bp < 1u || own_bp > own_len || oth_bp < 1u || oth_bp > oth_len) return false;
  if (s.rec >= in.n_rec) return false;
  if (in.flag[s.rec] & 0x204) return false;
  const uint32_t mq = in.mapq[s.rec];
  if ((long long) mq < (long long) mapq_min) return false;
  const uint32_t own_r = own_bp == own_start, oth_r = oth_bp == oth_start;
  const int32_t own_t = s.tid;
  if (own_t == other_chr && own_bp == oth_bp && own_r == oth_r) return false;
  const bool own_first = own_t < other_chr || (own_t == other_chr && (own_bp < oth_bp || (own_bp == oth_bp && own_r < oth_r)));
  const uint64_t t1 = own_first ? own_t : other_chr, t2 = own_first ? other_chr : own_t;
  const uint32_t r1 = own_first ? own_r : oth_r, r2 = own_first ? oth_r : own_r;
  t.g = ((t1 * (uint64_t) in.nt + t2) << 2) | (r1 << 1) | r2;
  t.qhash = s.qhash;
  t.pos1 = own_first ? own_bp : oth_bp;
  t.pos2 = own_first ? oth_bp : own_bp;
  t.own_mapq = ((own_first ? 0u : 1u) << 8) | mq;
  t.qrank = 0;
  return true;
}

__global__ __launch_bounds__(256) void k_sj_flag(SjInput in, int mapq_min, uint32_t *__restrict__ flag)
{
  const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= in.n) return;
  SjTuple t;
  flag[i] = sj_classify(in, mapq_min, in.split[i], t);
}

// ex = the exclusive scan of the flags (n + 1 entries): an eligible tuple's slot is ex[i] < ex[n] = e
__global__ __launch_bounds__(256) void k_sj_compact(SjInput in, int mapq_min, const uint32_t *__restrict__ ex, SjTuple *__restrict__ tup)
{
  const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= in.n) return;
  if (ex[i + 1] == ex[i]) return;
  SjTuple t;
  if (sj_classify(in, mapq_min, in.split[i], t)) tup[ex[i]] = t;
}

// ---- the sort stages ----------------------------------------------------------------------------------------------------------------
// keys[i] = the stage's key of tuple perm[i] (perm == nullptr: the identity); vals[i] = that tuple.  perm may be vals itself.
__global__ __launch_bounds__(256) void k_sj_keys(const SjTuple *__restrict__ tup, const uint32_t *perm, uint32_t e, int mode, int pos_bits, uint64_t *__restrict__ keys, uint32_t *vals)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  const uint32_t k = perm ? perm[i] : i;  // (k < e: perm is a permutation that the sort made of the identity)
  const SjTuple t = tup[k];
  keys[i] = mode == 0 ? t.qhash : mode == 1 ? ((uint64_t) t.pos1 << pos_bits) | t.pos2 : t.g;
  vals[i] = k;
}

// the heads of the exact junctions and of the reads inside them, over the sorted rows; both are 1 at i == 0
__global__ __launch_bounds__(256) void k_sj_heads(const SjTuple *__restrict__ sorted, uint32_t e, uint32_t *__restrict__ head, uint32_t *__restrict__ qhead)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  uint32_t h = 1, q = 1;
  if (i)
  {
    const SjTuple a = sorted[i - 1], b = sorted[i];
    h = a.g != b.g || a.pos1 != b.pos1 || a.pos2 != b.pos2;
    q = h | (a.qrank != b.qrank);
  }
  head[i] = h;
  qhead[i] = q;
}

// ---- the exact junctions ------------------------------------------------------------------------------------------------------------
// One wavefront per exact junction, four to a workgroup: its tuples are rows [xstart[j], xstart[j + 1]) of the sorted table.
__global__ __launch_bounds__(256) void k_sj_exact(const SjTuple *__restrict__ sorted, const uint32_t *__restrict__ xstart, const uint32_t *__restrict__ exq, uint32_t x,
                                                  SjExact *__restrict__ xrow, uint32_t *__restrict__ label)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= x) return;
  const uint32_t a = xstart[j], b = xstart[j + 1];  // (a < b <= e)
  uint32_t own1 = 0, mq0 = 0, mq1 = 0;
  for (uint32_t i = a + lane; i < b; i += 64)
  {
    const uint32_t om = sorted[i].own_mapq;
    const uint32_t o = om >> 8, mq = om & 255u;
    own1 += o;
    mq0 += o ? 0u : mq;
    mq1 += o ? mq : 0u;
  }
  own1 = wave_sum(own1);
  mq0 = wave_sum(mq0);
  mq1 = wave_sum(mq1);
  if (lane) return;
  const SjTuple t = sorted[a];
  SjExact r;
  r.g = t.g;
  r.pos1 = t.pos1;
  r.pos2 = t.pos2;
  r.n_reads = exq[b] - exq[a];
  r.n_tuples = b - a;
  r.n_own[0] = b - a - own1;
  r.n_own[1] = own1;
  r.mapq_sum[0] = mq0;
  r.mapq_sum[1] = mq1;
  xrow[j] = r;
  label[j] = j;
}

// the first exact junction whose (g, pos1) is >= (g, want) (x: none)
__device__ __forceinline__ uint32_t sj_lower(const SjExact *__restrict__ xrow, uint32_t x, uint64_t g, long long want)
{
  uint32_t lo = 0, hi = x;
  while (lo < hi)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    const uint64_t mg = xrow[mid].g;
    if (mg < g || (mg == g && (long long) xrow[mid].pos1 < want))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// One round of min-label propagation.  One wavefront per exact junction j: the exact junctions of its group with pos1' in
// [pos1 - tol, pos1 + tol] are a contiguous range of the table, dealt to the lanes 64 a step; a lane whose row is near j offers its
// label.  The smallest offer m goes to label[j] and to the label of what j pointed to so far (its root, or a member on the way to
// it): without that hook a small label that reaches a settled stretch from its far end would cross it one step a round.  A label
// read while another lane lowers it is still a member of the component.  Invariants: label[v] <= v and label[v] is in v's component.
// A round that changes nothing leaves every near pair with one label, and then that label is the component's smallest member.
__global__ __launch_bounds__(256) void k_sj_hook(const SjExact *__restrict__ xrow, uint32_t x, uint32_t tol, uint32_t *label, uint32_t *changed)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= x) return;
  const SjExact me = xrow[j];
  const long long T = tol, lo = (long long) me.pos1 - T, hi = (long long) me.pos1 + T;
  uint32_t m = NONE;
  for (uint32_t q0 = sj_lower(xrow, x, me.g, lo); q0 < x; q0 += 64)  // (q0 is the same on every lane)
  {
    const uint32_t q = q0 + lane;
    bool hit = false;
    if (q < x)
    {
      const SjExact o = xrow[q];
      hit = o.g == me.g && (long long) o.pos1 <= hi;
      if (hit)
      {
        const long long d = (long long) o.pos2 - (long long) me.pos2;
        if (d <= T && -d <= T)
        {
          const uint32_t l = label[q];
          m = l < m ? l : m;
        }
      }
    }
    if (!__all(hit)) break;  // the table is sorted: behind the first miss there is no hit
  }
  m = wave_min(m);
  if (lane == 0)
  {
    const uint32_t old = label[j];  // (old <= j < x)
    if (m < old)
    {
      atomicMin(&label[j], m);
      atomicMin(&label[old], m);
      *changed = 1u;
    }
  }
}

__global__ __launch_bounds__(256) void k_sj_jump(uint32_t *label, uint32_t x)
{
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= x) return;
  const uint32_t first = label[v];
  uint32_t l = first;
  for (int k = 0; k < JUMPS; ++k)
  {
    const uint32_t up = label[l];  // (l <= v < x)
    if (up == l) break;
    l = up;
  }
  if (l < first) atomicMin(&label[v], l);
}

__global__ __launch_bounds__(256) void k_sj_label_keys(const uint32_t *__restrict__ label, uint32_t x, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= x) return;
  keys[j] = label[j];
  vals[j] = j;
}

// (label of the tuple's exact junction) << rank_bits | read rank: equal keys are one read of one call
__global__ __launch_bounds__(256) void k_sj_tuple_keys(const SjTuple *__restrict__ sorted, const uint32_t *__restrict__ xid, const uint32_t *__restrict__ label, uint32_t e, int rank_bits,
                                                       uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  keys[i] = ((uint64_t) label[xid[i]] << rank_bits) | sorted[i].qrank;  // (xid[i] < x)
  vals[i] = i;
}

// ---- the claimed row ----------------------------------------------------------------------------------------------------------------
// One lane per exact junction: the entries with end a on tid1 within +-2 of pos1 are a range of the sorted entries (a handful: the
// voted rows are few); the smallest code whose end b is on tid2 within +-2 of pos2 wins.
__global__ __launch_bounds__(256) void k_sj_claim(const SjExact *__restrict__ xrow, uint32_t x, uint32_t nt, const SjClaim *__restrict__ ent, uint32_t nc, uint32_t *__restrict__ claim)
{
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= x) return;
  const SjExact me = xrow[j];
  const uint64_t t12 = me.g >> 2, tid1 = t12 / nt, tid2 = t12 % nt;
  const long long lo = (long long) me.pos1 - 2, hi = (long long) me.pos1 + 2;
  const uint64_t k_lo = ((tid1 + 1) << 32) | (uint64_t) (lo < 0 ? 0 : lo), k_hi = ((tid1 + 1) << 32) | (uint64_t) (hi > 0xFFFFFFFFll ? 0xFFFFFFFFll : hi);
  uint32_t a = 0, b = nc;
  while (a < b)
  {
    const uint32_t mid = a + (b - a) / 2;
    if (ent[mid].key < k_lo)
      a = mid + 1;
    else
      b = mid;
  }
  uint32_t best = NONE;
  for (uint32_t q = a; q < nc && ent[q].key <= k_hi; ++q)
  {
    const SjClaim c = ent[q];
    const long long d = (long long) c.pos_b - (long long) me.pos2;
    if ((uint64_t) (long long) c.tid_b == tid2 && d <= 2 && -d <= 2) best = c.code < best ? c.code : best;
  }
  claim[j] = best;
}

// ---- the calls ----------------------------------------------------------------------------------------------------------------------
// One wavefront per call c.  Its exact junctions are entries [cx[c], cx[c + 1]) of the list sorted by label (ascending inside a call,
// because the sort is stable), its tuples rows [ct[c], ct[c + 1]) of the list sorted by (label, read rank).
__global__ __launch_bounds__(256) void k_sj_calls(const SjExact *__restrict__ xrow, const uint32_t *__restrict__ xlist, const uint32_t *__restrict__ cx, const uint32_t *__restrict__ ct,
                                                  const uint32_t *__restrict__ exd, const uint32_t *__restrict__ claim, uint32_t n_calls, uint32_t nt, uint32_t min_reads,
                                                  struct bk_split_junction *__restrict__ rows, uint32_t *__restrict__ keep)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_calls) return;
  const uint32_t a = cx[c], b = cx[c + 1];
  uint32_t n_tuples = 0, own0 = 0, own1 = 0, mq0 = 0, mq1 = 0, lo1 = NONE, hi1 = 0, lo2 = NONE, hi2 = 0, cl = NONE;
  unsigned long long top = 0;  // n_reads << 32 | ~j: the most reads, then the smallest exact junction
  for (uint32_t i = a + lane; i < b; i += 64)
  {
    const uint32_t j = xlist[i];  // (j < x: a value of k_sj_label_keys)
    const SjExact r = xrow[j];
    n_tuples += r.n_tuples;
    own0 += r.n_own[0];
    own1 += r.n_own[1];
    mq0 += r.mapq_sum[0];
    mq1 += r.mapq_sum[1];
    lo1 = r.pos1 < lo1 ? r.pos1 : lo1;
    hi1 = r.pos1 > hi1 ? r.pos1 : hi1;
    lo2 = r.pos2 < lo2 ? r.pos2 : lo2;
    hi2 = r.pos2 > hi2 ? r.pos2 : hi2;
    const uint32_t k = claim[j];
    cl = k < cl ? k : cl;
    const unsigned long long key = ((unsigned long long) r.n_reads << 32) | (0xFFFFFFFFu - j);
    top = key > top ? key : top;
  }
  n_tuples = wave_sum(n_tuples);
  own0 = wave_sum(own0);
  own1 = wave_sum(own1);
  mq0 = wave_sum(mq0);
  mq1 = wave_sum(mq1);
  lo1 = wave_min(lo1);
  hi1 = wave_max(hi1);
  lo2 = wave_min(lo2);
  hi2 = wave_max(hi2);
  cl = wave_min(cl);
  top = wave_max(top);
  if (lane) return;
  const SjExact rep = xrow[0xFFFFFFFFu - (uint32_t) top];  // (a call has at least one exact junction, so top came from one)
  const uint64_t t12 = rep.g >> 2;
  struct bk_split_junction r;
  r.tid1 = (int32_t) (t12 / nt);
  r.pos1 = rep.pos1;
  r.tid2 = (int32_t) (t12 % nt);
  r.pos2 = rep.pos2;
  r.n_reads = exd[ct[c + 1]] - exd[ct[c]];
  r.n_tuples = n_tuples;
  r.n_exact = b - a;
  r.lo1 = lo1;
  r.hi1 = hi1;
  r.lo2 = lo2;
  r.hi2 = hi2;
  r.n_own[0] = own0;
  r.n_own[1] = own1;
  r.mapq_sum[0] = mq0;
  r.mapq_sum[1] = mq1;
  r.call = cl == NONE ? -1 : (int32_t) (cl >> 1);
  r.right1 = (uint8_t) ((rep.g >> 1) & 1u);
  r.right2 = (uint8_t) (rep.g & 1u);
  r.call_crossed = cl == NONE ? 0 : (uint8_t) (cl & 1u);
  r.reserved = 0;
  r.top_reads = rep.n_reads;
  rows[c] = r;
  keep[c] = r.n_reads >= min_reads;
}

// counts[0] = the kept calls a voted row claims, counts[1] = all claimed calls: one workgroup, no atomic
__global__ __launch_bounds__(256) void k_sj_count_claimed(const struct bk_split_junction *__restrict__ rows, const uint32_t *__restrict__ keep, uint32_t n_calls, uint32_t *__restrict__ counts)
{
  __shared__ uint32_t lds[prims::WAVES];
  uint32_t kept = 0, all = 0;
  for (uint32_t c = threadIdx.x; c < n_calls; c += 256)
  {
    const uint32_t cl = rows[c].call >= 0;
    all += cl;
    kept += cl & keep[c];
  }
  uint32_t tot;
  (void) prims::block_exclusive_scan(kept, lds, tot);
  if (threadIdx.x == 0) counts[0] = tot;
  (void) prims::block_exclusive_scan(all, lds, tot);
  if (threadIdx.x == 0) counts[1] = tot;
}

}  // namespace

uint64_t SjStats::touched() const
{
  const uint64_t rank_bits = bits_of(eligible), x_bits = bits_of(exact);
  const uint64_t p1 = 8 + ((uint64_t) 2 * pos_bits + 7) / 8 + ((uint64_t) group_bits + 7) / 8, p2 = (rank_bits + x_bits + 7) / 8, p3 = (x_bits + 7) / 8;
  return n * 96ull + eligible * (123ull + 36ull * p1 + 132ull + 64ull + 24ull + 36ull * p2 + 48ull) + exact * (80ull + 36ull * p3 + 24ull) + calls * 84ull + written * 72ull;
}

void split_junctions(const SjInput &in, int mapq_min, uint32_t tol, uint32_t min_reads, const SjClaim *claims, uint64_t n_claims, SjBufs &b, hipStream_t st,
                     struct bk_split_junction **rows_out, SjStats *stats)
{
  static_assert(sizeof(struct bk_split_junction) == 72, "bk_split_junction must be 72 bytes");
  SjStats s;
  s.n = in.n;
  s.pos_bits = bits_of(in.max_len);
  s.group_bits = in.nt > 0 ? bits_of(((((uint64_t) in.nt - 1) * (uint64_t) in.nt + (uint64_t) in.nt - 1) << 2) | 3ull) : 0;
  *rows_out = b.out.as<struct bk_split_junction>(1);
  *stats = s;
  if (in.n == 0) return;
  prims::radix_check_count(in.n);

  // 1, 2: classify, compact
  uint32_t *ex = b.flag.as<uint32_t>(in.n + 1);
  hipLaunchKernelGGL(k_sj_flag, dim3(cdiv(in.n, 256)), dim3(256), 0, st, in, mapq_min, ex);
  prims::exclusive_scan<uint32_t>(ex, ex, in.n, b.scan_tmp, st);
  const uint32_t e = runs::read_u32(ex + in.n, st);
  s.eligible = e;
  *stats = s;
  if (e == 0) return;
  if (e > 0x40000000u) throw bk_error(BK_ERR_LIMIT, "bk_split_junctions: more than 2^30 eligible tuples");
  SjTuple *tup = b.tup.as<SjTuple>(e);
  hipLaunchKernelGGL(k_sj_compact, dim3(cdiv(in.n, 256)), dim3(256), 0, st, in, mapq_min, ex, tup);

  // 3: stable LSD stages, least significant first: qhash (and its dense rank), (pos1, pos2), the group
  uint64_t *keys = b.keys.as<uint64_t>(e), *sk;
  uint32_t *vals = b.vals.as<uint32_t>(e), *sv;
  uint32_t *head = b.head.as<uint32_t>((uint64_t) e + 1), *qhead = b.qhead.as<uint32_t>((uint64_t) e + 1);
  const unsigned ge = cdiv(e, 256);
  hipLaunchKernelGGL(k_sj_keys, dim3(ge), dim3(256), 0, st, tup, (const uint32_t *) nullptr, e, 0, s.pos_bits, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, 64, b.radix, st, &sk, &sv);
  hipLaunchKernelGGL(runs::k_key_heads, dim3(ge), dim3(256), 0, st, sk, e, 0, 0u, head, (uint32_t *) nullptr);
  prims::exclusive_scan<uint32_t>(head, head, e, b.scan_tmp, st);
  hipLaunchKernelGGL(runs::k_dense_rank<SjTuple>, dim3(ge), dim3(256), 0, st, sv, head, e, tup);
  hipLaunchKernelGGL(k_sj_keys, dim3(ge), dim3(256), 0, st, tup, sv, e, 1, s.pos_bits, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, 2 * s.pos_bits, b.radix, st, &sk, &sv);
  hipLaunchKernelGGL(k_sj_keys, dim3(ge), dim3(256), 0, st, tup, sv, e, 2, s.pos_bits, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, s.group_bits, b.radix, st, &sk, &sv);
  SjTuple *sorted = b.sorted.as<SjTuple>(e);
  hipLaunchKernelGGL(runs::k_gather_rows<SjTuple>, dim3(ge), dim3(256), 0, st, tup, sv, e, sorted);

  // 4: the exact junctions
  uint32_t *exq = qhead, *xid = b.xid.as<uint32_t>(e), *xstart = b.xstart.as<uint32_t>((uint64_t) e + 1);
  hipLaunchKernelGGL(k_sj_heads, dim3(ge), dim3(256), 0, st, sorted, e, head, qhead);
  uint32_t *exh = b.ex.as<uint32_t>((uint64_t) e + 1);
  prims::exclusive_scan<uint32_t>(head, exh, e, b.scan_tmp, st);
  prims::exclusive_scan<uint32_t>(qhead, exq, e, b.scan_tmp, st);
  hipLaunchKernelGGL(runs::k_run_starts, dim3(ge), dim3(256), 0, st, exh, e, xstart, xid);
  const uint32_t x = runs::read_u32(exh + e, st);  // (1 <= x <= e)
  s.exact = x;
  SjExact *xrow = b.xrow.as<SjExact>(x);
  uint32_t *label = b.label.as<uint32_t>(x), *changed = b.changed.as<uint32_t>(1);
  hipLaunchKernelGGL(k_sj_exact, dim3(cdiv(x, 4)), dim3(256), 0, st, sorted, xstart, exq, x, xrow, label);

  // 5, 6: components.  The smallest label of a component travels at least one near-step a round and a component has at most x members:
  // x + 1 rounds settle every input, the last one changing nothing.  The loop is counted by the host, so it ends whatever the device does.
  uint32_t rounds = 0;
  for (;;)
  {
    if (rounds > x) throw bk_error(BK_ERR_LIMIT, "bk_split_junctions: the calls did not settle within x + 1 rounds of label propagation (x exact junctions)");
    ++rounds;
    HIP_CHECK(hipMemsetAsync(changed, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_sj_hook, dim3(cdiv(x, 4)), dim3(256), 0, st, xrow, x, tol, label, changed);
    hipLaunchKernelGGL(k_sj_jump, dim3(cdiv(x, 256)), dim3(256), 0, st, label, x);
    if (!runs::read_u32(changed, st)) break;
  }
  s.rounds = rounds;

  // the exact junctions by label: every call a contiguous range, calls in the order of their smallest exact junction
  const unsigned gx = cdiv(x, 256);
  const int x_bits = bits_of(x), rank_bits = bits_of(e);
  hipLaunchKernelGGL(k_sj_label_keys, dim3(gx), dim3(256), 0, st, label, x, keys, vals);
  prims::radix_sort_pairs(keys, vals, x, 0, x_bits, b.radix, st, &sk, &sv);
  uint32_t *xlist = b.xlist.as<uint32_t>(x), *cx = b.cstart_x.as<uint32_t>((uint64_t) x + 1), *ct = b.cstart_t.as<uint32_t>((uint64_t) x + 1);
  HIP_CHECK(hipMemcpyAsync(xlist, sv, (uint64_t) x * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(runs::k_key_heads, dim3(gx), dim3(256), 0, st, sk, x, 0, 1u, head, (uint32_t *) nullptr);
  prims::exclusive_scan<uint32_t>(head, exh, x, b.scan_tmp, st);
  hipLaunchKernelGGL(runs::k_run_starts, dim3(gx), dim3(256), 0, st, exh, x, cx, (uint32_t *) nullptr);
  const uint32_t n_calls = runs::read_u32(exh + x, st);  // (1 <= n_calls <= x)
  s.calls = n_calls;

  // 7: the tuples by (label, read rank): the heads of the sub-runs are the distinct reads of a call
  hipLaunchKernelGGL(k_sj_tuple_keys, dim3(ge), dim3(256), 0, st, sorted, xid, label, e, rank_bits, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, rank_bits + x_bits, b.radix, st, &sk, &sv);
  uint32_t *exd = qhead;
  hipLaunchKernelGGL(runs::k_key_heads, dim3(ge), dim3(256), 0, st, sk, e, rank_bits, 1u, head, qhead);
  prims::exclusive_scan<uint32_t>(head, exh, e, b.scan_tmp, st);
  prims::exclusive_scan<uint32_t>(qhead, exd, e, b.scan_tmp, st);
  hipLaunchKernelGGL(runs::k_run_starts, dim3(ge), dim3(256), 0, st, exh, e, ct, (uint32_t *) nullptr);  // (as many label runs as calls: ct[n_calls] = e)

  // 9: the claimed row of every exact junction
  uint32_t *claim = b.claim.as<uint32_t>(x);
  const SjClaim *d_ent = b.cent.as<SjClaim>(n_claims + 1);
  if (n_claims) HIP_CHECK(hipMemcpyAsync((void *) d_ent, claims, n_claims * sizeof(SjClaim), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_sj_claim, dim3(gx), dim3(256), 0, st, xrow, x, (uint32_t) in.nt, d_ent, (uint32_t) n_claims, claim);

  // 8, 10: the calls, and those with enough reads
  struct bk_split_junction *rows = b.rows.as<struct bk_split_junction>(n_calls);
  uint32_t *keep = b.keep.as<uint32_t>((uint64_t) n_calls + 1), *counts = b.counts.as<uint32_t>(2);
  hipLaunchKernelGGL(k_sj_calls, dim3(cdiv(n_calls, 4)), dim3(256), 0, st, xrow, xlist, cx, ct, exd, claim, n_calls, (uint32_t) in.nt, min_reads, rows, keep);
  hipLaunchKernelGGL(k_sj_count_claimed, dim3(1), dim3(256), 0, st, rows, keep, n_calls, counts);
  prims::exclusive_scan<uint32_t>(keep, keep, n_calls, b.scan_tmp, st);
  struct bk_split_junction *out = b.out.as<struct bk_split_junction>((uint64_t) n_calls + 1);
  hipLaunchKernelGGL(runs::k_keep_out<struct bk_split_junction>, dim3(cdiv(n_calls, 256)), dim3(256), 0, st, rows, keep, n_calls, out);
  s.written = runs::read_u32(keep + n_calls, st);
  s.claimed = runs::read_u32(counts, st);
  *rows_out = out;
  *stats = s;
}
