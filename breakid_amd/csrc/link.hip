// Linked calls (bk_link_calls): how the calls of one list relate to each other.  The breakends with a contig are sorted
// by ((tid + 1) << 32) | pos; one wavefront per site deals the breakends inside its two windows to the lanes and decides duplicate /
// reciprocal / adjacent from the two rows alone.  The events are the components of the graph whose vertices are the runs of the sorted
// table (a run ends where the gap exceeds D or the contig changes) and whose edges are the sites: min-label propagation with pointer
// jumping, the rounds counted by the host.  Integer arithmetic only; the atomics are integer min and add, whose results do not depend
// on the order.
#include "link.h"
#include "wave.h"

namespace
{
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int JUMPS = 8;  // pointer jumps of one vertex in one round

__device__ __forceinline__ unsigned long long link_key(int32_t tid, unsigned long long pos) { return ((unsigned long long) ((long long) tid + 1) << 32) | pos; }

// breakend 2 * i + s is side s of site i.  A side with tid < 0 gets the key of contig 0, which no side with a contig has: the sort puts
// these in front, and everything after the sort starts behind them.
__global__ __launch_bounds__(256) void k_link_keys(const struct bk_link_site *__restrict__ sites, uint32_t n, unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const struct bk_link_site s = sites[i];
  keys[2 * i] = s.tid1 < 0 ? 0ull : link_key(s.tid1, s.pos1);
  keys[2 * i + 1] = s.tid2 < 0 ? 0ull : link_key(s.tid2, s.pos2);
  vals[2 * i] = 2 * i;
  vals[2 * i + 1] = 2 * i + 1;
}

// flag[q] = 1 where sorted breakend q opens a run other than the first: the contig changes or the gap to q - 1 exceeds D
__global__ __launch_bounds__(256) void k_link_run_flags(const unsigned long long *__restrict__ keys, uint32_t m, uint32_t D, uint32_t *__restrict__ flag)
{
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= m) return;
  uint32_t f = 0;
  if (q)
  {
    const unsigned long long a = keys[q - 1], b = keys[q];  // a <= b
    f = (a >> 32) != (b >> 32) || b - a > (unsigned long long) D;
  }
  flag[q] = f;
}

// ex = the exclusive scan of the flags (m + 1 entries), so ex[q + 1] is the run of sorted breakend q.  run_of[breakend] = its run;
// every possible run id (there are at most m) starts as its own label, with no site and no count.
__global__ __launch_bounds__(256) void k_link_runs(const uint32_t *__restrict__ vals, const uint32_t *__restrict__ ex, uint32_t m, uint32_t *__restrict__ run_of,
                                                   uint32_t *__restrict__ label, uint32_t *__restrict__ ev_min, uint32_t *__restrict__ ev_cnt)
{
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= m) return;
  run_of[vals[q]] = ex[q + 1];  // (vals[q] < 2 n: a value that k_link_keys wrote)
  label[q] = q;
  ev_min[q] = NONE;
  ev_cnt[q] = 0;
}

// ---- one site against its neighbours --------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool link_near(int32_t ta, uint32_t pa, int32_t tb, uint32_t pb, long long D)
{
  const long long d = (long long) pa - (long long) pb;
  return ta == tb && ta >= 0 && d <= D && -d <= D;
}

// the first sorted breakend whose key is >= want (m: none)
__device__ __forceinline__ uint32_t link_lower(const unsigned long long *__restrict__ keys, uint32_t m, unsigned long long want)
{
  uint32_t lo = 0, hi = m;
  while (lo < hi)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < want)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

constexpr unsigned long long NO_KEY = ~0ull;
// The mate key, smallest wins: (|off0| + |off1|) << 31 | j << 1 | crossed.  The sum is at most 2 * BK_LINK_MAX_DIST < 2^21 and
// j < 2^30, so the key stays below 2^52 and NO_KEY is above every key.
__device__ __forceinline__ unsigned long long mate_key(long long o0, long long o1, uint32_t j, uint32_t crossed)
{
  const unsigned long long sum = (unsigned long long) (o0 < 0 ? -o0 : o0) + (unsigned long long) (o1 < 0 ? -o1 : o1);
  return (sum << 31) | ((unsigned long long) j << 1) | crossed;
}

// One wavefront per site, four to a workgroup; no LDS and no barrier.  Every sorted breakend read is q < m, every site read is
// j = vals[q] >> 1 < n.  The row is complete but for event / event_size, which start as "alone" and are set by k_link_event_out.
__global__ __launch_bounds__(256) void k_link_sites(const struct bk_link_site *__restrict__ sites, uint32_t n, const unsigned long long *__restrict__ keys,
                                                    const uint32_t *__restrict__ vals, uint32_t m, uint32_t max_dist, struct bk_call_link *__restrict__ res)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const struct bk_link_site me = sites[i];
  const int32_t tid[2] = {me.tid1, me.tid2};
  const uint32_t P[2] = {me.pos1, me.pos2};
  const uint32_t R[2] = {me.right1, me.right2};
  const long long D = max_dist;

  unsigned long long counts = 0;  // n_dup and n_recip of this lane, 32 bits each: a lane counts a site at most once, and n <= 2^30
  uint32_t n_adj = 0;
  unsigned long long dup_min = NO_KEY, mate_min = NO_KEY;
  for (int s = 0; s < 2; ++s)
  {
    if (tid[s] < 0) continue;
    const long long lo = (long long) P[s] - D, hi = (long long) P[s] + D;
    const unsigned long long k_lo = link_key(tid[s], lo < 0 ? 0ull : (unsigned long long) lo);
    const unsigned long long k_hi = link_key(tid[s], hi > 0xFFFFFFFFll ? 0xFFFFFFFFull : (unsigned long long) hi);
    for (uint32_t q0 = link_lower(keys, m, k_lo); q0 < m; q0 += 64)  // (q0 is the same on every lane)
    {
      const uint32_t q = q0 + lane;
      const bool hit = q < m && keys[q] <= k_hi;
      if (hit)
      {
        const uint32_t b = vals[q], j = b >> 1, t = b & 1u;
        if (j != i)
        {
          const struct bk_link_site o = sites[j];
          const int32_t otid[2] = {o.tid1, o.tid2};
          const uint32_t oP[2] = {o.pos1, o.pos2};
          const uint32_t oR[2] = {o.right1, o.right2};
          uint32_t N = 0;  // bit 2 * s' + t' = N[s'][t']
#pragma unroll
          for (int a = 0; a < 4; ++a) N |= (uint32_t) link_near(tid[a >> 1], P[a >> 1], otid[a & 1], oP[a & 1], D) << a;
          // this hit is entry (s, t) of N; the site is counted where its first set entry is found
          if (!(N & ((1u << (2 * s + (int) t)) - 1u)))
          {
            const bool straight = (N & 1u) && (N & 8u), crossed = (N & 2u) && (N & 4u);
            const bool st_same = R[0] == oR[0] && R[1] == oR[1], st_opp = R[0] != oR[0] && R[1] != oR[1];
            const bool cr_same = R[0] == oR[1] && R[1] == oR[0], cr_opp = R[0] != oR[1] && R[1] != oR[0];
            if ((straight && st_same) || (crossed && cr_same))
            {
              counts += 1ull;
              dup_min = j < dup_min ? j : dup_min;
            }
            else if ((straight && st_opp) || (crossed && cr_opp))
            {
              counts += 1ull << 32;
              if (straight && st_opp)
              {
                const unsigned long long k = mate_key((long long) oP[0] - (long long) P[0], (long long) oP[1] - (long long) P[1], j, 0);
                mate_min = k < mate_min ? k : mate_min;
              }
              if (crossed && cr_opp)
              {
                const unsigned long long k = mate_key((long long) oP[1] - (long long) P[0], (long long) oP[0] - (long long) P[1], j, 1);
                mate_min = k < mate_min ? k : mate_min;
              }
            }
            else
              ++n_adj;
          }
        }
      }
      if (!__all(hit)) break;  // the table is sorted: behind the first miss there is no hit
    }
  }
  counts = wave_sum(counts);
  const unsigned long long adj = wave_sum<unsigned long long>(n_adj);
  dup_min = wave_min(dup_min);
  mate_min = wave_min(mate_min);

  struct bk_call_link r;
  r.n_dup = (uint32_t) counts;
  r.n_recip = (uint32_t) (counts >> 32);
  r.n_adj = (uint32_t) adj;
  r.dup_of = dup_min == NO_KEY ? -1 : (int32_t) dup_min;
  r.mate = -1;
  r.off[0] = r.off[1] = 0;
  r.event = i;
  r.event_size = 1;
  r.mate_crossed = 0;
  r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
  if (mate_min != NO_KEY)
  {
    const uint32_t j = (uint32_t) (mate_min >> 1) & 0x3FFFFFFFu, crossed = (uint32_t) mate_min & 1u;
    const struct bk_link_site o = sites[j];  // (j < n: it came from a row of vals)
    const uint32_t oP[2] = {o.pos1, o.pos2};
    r.mate = (int32_t) j;
    r.mate_crossed = (uint8_t) crossed;
    r.off[0] = (int32_t) ((long long) oP[crossed] - (long long) P[0]);
    r.off[1] = (int32_t) ((long long) oP[1 - crossed] - (long long) P[1]);
  }
  if (lane == 0) res[i] = r;
}

// ---- the events: components over the runs ---------------------------------------------------------------------------------------------
// Invariants of label[]: label[v] <= v, label[v] is a run of v's component, and after k rounds label[v] is at most the smallest run
// within k sites of v.  A round that changes nothing leaves every site's two runs with one label, and then that label is the
// component's smallest run.
__global__ __launch_bounds__(256) void k_link_hook(const uint32_t *__restrict__ run_of, uint32_t n, uint32_t *label, uint32_t *changed)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = run_of[2 * i], b = run_of[2 * i + 1];
  if (a == NONE || b == NONE || a == b) return;
  const uint32_t la = label[a], lb = label[b];
  if (la == lb) return;
  const uint32_t lo = la < lb ? la : lb, hi = la < lb ? lb : la;
  atomicMin(&label[a], lo);
  atomicMin(&label[b], lo);
  atomicMin(&label[hi], lo);  // (hi is a run of the same component, and lo < hi)
  *changed = 1u;
}

__global__ __launch_bounds__(256) void k_link_jump(uint32_t *label, uint32_t m)
{
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= m) return;
  const uint32_t first = label[v];
  uint32_t l = first;
  for (int k = 0; k < JUMPS; ++k)
  {
    const uint32_t up = label[l];  // (l <= v < m)
    if (up == l) break;
    l = up;
  }
  if (l < first) atomicMin(&label[v], l);
}

// the run a site belongs to: that of its first side with a contig (both have one label by now)
__device__ __forceinline__ uint32_t link_site_run(const uint32_t *__restrict__ run_of, uint32_t i)
{
  const uint32_t a = run_of[2 * i];
  return a != NONE ? a : run_of[2 * i + 1];
}

__global__ __launch_bounds__(256) void k_link_event_acc(const uint32_t *__restrict__ run_of, uint32_t n, const uint32_t *__restrict__ label, uint32_t *ev_min, uint32_t *ev_cnt)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = link_site_run(run_of, i);
  if (r == NONE) return;
  const uint32_t root = label[r];
  atomicMin(&ev_min[root], i);
  atomicAdd(&ev_cnt[root], 1u);
}

__global__ __launch_bounds__(256) void k_link_event_out(const uint32_t *__restrict__ run_of, uint32_t n, const uint32_t *__restrict__ label,
                                                        const uint32_t *__restrict__ ev_min, const uint32_t *__restrict__ ev_cnt, struct bk_call_link *__restrict__ res)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = link_site_run(run_of, i);
  if (r == NONE) return;  // (no side has a contig: the site stays alone)
  const uint32_t root = label[r];
  res[i].event = ev_min[root];
  res[i].event_size = ev_cnt[root];
}
}  // namespace

int LinkShape::key_bits() const
{
  if (!m) return 0;
  int bits = 0;
  for (uint64_t v = (uint64_t) max_tid + 1; v; v >>= 1) ++bits;
  return 32 + bits;
}

uint64_t LinkShape::touched() const
{
  const uint64_t passes = ((uint64_t) key_bits() + 7) / 8;
  return n * (sizeof(struct bk_link_site) + sizeof(struct bk_call_link)) + m * (24ull + 24ull * passes);
}

void link_upload(const struct bk_link_site *sites, uint64_t n, LinkBufs &b, hipStream_t st) { b.d_sites = upload(b.sites, sites, n, st); }

void link_calls(const LinkShape &shape, uint32_t max_dist, LinkBufs &b, hipStream_t st, struct bk_call_link **res_out, uint32_t *rounds_out)
{
  static_assert(sizeof(struct bk_link_site) == 24 && sizeof(struct bk_call_link) == 40, "bk_link_site must be 24 bytes and bk_call_link 40");
  const uint32_t n = (uint32_t) shape.n, m = (uint32_t) shape.m;
  struct bk_call_link *res = b.res.as<struct bk_call_link>(shape.n + 1);
  *res_out = res;
  *rounds_out = 0;
  if (n == 0) return;

  // the sorted breakends with a contig: the 2 n - m others sort in front (key 0) and are left out from here on
  unsigned long long *keys = b.keys.as<unsigned long long>(2ull * n);
  uint32_t *vals = b.vals.as<uint32_t>(2ull * n);
  hipLaunchKernelGGL(k_link_keys, dim3(cdiv(n, 256)), dim3(256), 0, st, b.d_sites, n, keys, vals);
  uint64_t *sk;
  uint32_t *sv;
  prims::radix_sort_pairs((uint64_t *) keys, vals, 2ull * n, 0, shape.key_bits(), b.radix, st, &sk, &sv);
  const unsigned long long *skeys = (const unsigned long long *) sk + (2ull * n - m);
  const uint32_t *svals = sv + (2ull * n - m);

  hipLaunchKernelGGL(k_link_sites, dim3(cdiv(n, 4)), dim3(256), 0, st, b.d_sites, n, skeys, svals, m, max_dist, res);
  if (m == 0) return;

  uint32_t *ex = b.flags.as<uint32_t>((uint64_t) m + 1), *run_of = b.run_of.as<uint32_t>(2ull * n);
  uint32_t *label = b.label.as<uint32_t>(m), *ev_min = b.ev_min.as<uint32_t>(m), *ev_cnt = b.ev_cnt.as<uint32_t>(m);
  uint32_t *changed = b.changed.as<uint32_t>(1);
  hipLaunchKernelGGL(k_link_run_flags, dim3(cdiv(m, 256)), dim3(256), 0, st, skeys, m, max_dist, ex);
  prims::exclusive_scan<uint32_t>(ex, ex, m, b.scan_tmp, st);
  HIP_CHECK(hipMemsetAsync(run_of, 0xFF, 2ull * n * sizeof(uint32_t), st));  // NONE
  hipLaunchKernelGGL(k_link_runs, dim3(cdiv(m, 256)), dim3(256), 0, st, svals, ex, m, run_of, label, ev_min, ev_cnt);

  // A label travels at least one site a round, and a component has at most n of them: n + 1 rounds settle every input, the last one
  // changing nothing.  The loop is counted by the host, so it ends whatever the device does.
  uint32_t rounds = 0;
  for (;;)
  {
    if (rounds > n) throw bk_error(BK_ERR_LIMIT, "bk_link_calls: the events did not settle within n + 1 rounds of label propagation");
    ++rounds;
    uint32_t h_changed = 0;
    HIP_CHECK(hipMemsetAsync(changed, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_link_hook, dim3(cdiv(n, 256)), dim3(256), 0, st, run_of, n, label, changed);
    hipLaunchKernelGGL(k_link_jump, dim3(cdiv(m, 256)), dim3(256), 0, st, label, m);
    HIP_CHECK(hipMemcpyAsync(&h_changed, changed, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (!h_changed) break;
  }
  *rounds_out = rounds;
  hipLaunchKernelGGL(k_link_event_acc, dim3(cdiv(n, 256)), dim3(256), 0, st, run_of, n, label, ev_min, ev_cnt);
  hipLaunchKernelGGL(k_link_event_out, dim3(cdiv(n, 256)), dim3(256), 0, st, run_of, n, label, ev_min, ev_cnt, res);
}
