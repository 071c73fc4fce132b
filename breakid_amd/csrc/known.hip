// Known junctions (bk_known_calls): every call of a list against a panel of pairs of intervals.  The intervals with a
// contig are sorted by ((tid + 1) << 32) | beg, and a running maximum of `end` is kept inside every contig's run.  One wavefront per
// site searches, per breakend, the last interval that begins at or before x + slop and walks backwards 64 intervals a step while the
// running maximum still reaches x - slop.  A lane whose interval holds the breakend reads the entry's row, computes the whole 2 x 2
// table of (breakend, interval) from it and counts the entry only where it is reached through its first interval that holds.  The
// distinct names are counted without atomics: the hits per site are scanned, a second walk lists (site << 32) | name at the site's
// offset, the list is sorted and one wavefront per site counts the run heads.  Integer arithmetic only: two runs give the same bytes.
#include "known.h"
#include "runs.h"

namespace
{
constexpr uint32_t DIST_MASK = 0x1FFFFFu;  // a mapping's dist is at most 2 * BK_KNOWN_MAX_SLOP = 2 000 000 < 2^21 - 1
static_assert(2ull * BK_KNOWN_MAX_SLOP < DIST_MASK, "the best key keeps dist in 21 bits, and 0 is no key");

__device__ __forceinline__ unsigned long long known_key(int32_t tid, unsigned long long beg) { return ((unsigned long long) ((long long) tid + 1) << 32) | beg; }

// interval end 2 * e + k is interval k of entry e.  An interval with tid < 0 gets the key of contig 0, which no interval with a contig
// has: the sort puts these in front, and everything after the sort starts behind them.
__global__ __launch_bounds__(256) void k_known_keys(const struct bk_known_entry *__restrict__ entries, uint32_t n_entries, unsigned long long *__restrict__ keys,
                                                    uint32_t *__restrict__ vals)
{
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_entries) return;
  const struct bk_known_entry r = entries[e];
  keys[2 * e] = r.tid1 < 0 ? 0ull : known_key(r.tid1, r.beg1);
  keys[2 * e + 1] = r.tid2 < 0 ? 0ull : known_key(r.tid2, r.beg2);
  vals[2 * e] = 2 * e;
  vals[2 * e + 1] = 2 * e + 1;
}

// iend[q] = the end of the q-th interval in sorted order (vals[q] < 2 n_entries: a value that k_known_keys wrote)
__global__ __launch_bounds__(256) void k_known_ends(const struct bk_known_entry *__restrict__ entries, const uint32_t *__restrict__ vals, uint32_t m, uint32_t *__restrict__ iend)
{
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= m) return;
  const uint32_t v = vals[q];
  const struct bk_known_entry *r = entries + (v >> 1);
  iend[q] = (v & 1u) ? r->end2 : r->end1;
}

// The running maximum of `end` inside every contig's run, as the running maximum of (contig << 32) | end over the whole index: the
// contig ascends, so the largest value up to row q carries q's contig and the largest end of its run so far.  One workgroup walks the
// rows 256 at a time with the carry in a register (the shape of k_frame_run_max).
__global__ __launch_bounds__(256) void k_known_run_max(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ iend, uint32_t m, uint32_t *__restrict__ run_max)
{
  __shared__ unsigned long long wmax[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < m; base += 256)
  {
    const uint32_t q = base + threadIdx.x;
    unsigned long long v = q < m ? (keys[q] & 0xFFFFFFFF00000000ull) | iend[q] : 0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
      const unsigned long long o = __shfl_up(v, d, 64);
      if (lane >= d && o > v) v = o;
    }
    if (lane == 63) wmax[w] = v;
    __syncthreads();
    unsigned long long tot = carry;
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
      const unsigned long long s = wmax[k];
      if (k < w && s > v) v = s;
      tot = s > tot ? s : tot;
    }
    __syncthreads();
    if (carry > v) v = carry;
    if (q < m) run_max[q] = (uint32_t) v;
    carry = tot;
  }
}

// ---- one site against the panel ---------------------------------------------------------------------------------------------------------
// dist(x, [b, e)) in 64 bits; e > b >= 0 for every interval with a contig (the host's check)
__device__ __forceinline__ bool known_falls(int32_t ts, long long x, int32_t ti, uint32_t b, uint32_t e, long long slop, long long &d)
{
  d = 0;
  if (ts != ti || ts < 0) return false;
  d = x < (long long) b ? (long long) b - x : x >= (long long) e ? x - ((long long) e - 1) : 0ll;
  return d <= slop;
}

// how many sorted intervals have a key <= want
__device__ __forceinline__ uint32_t known_upper(const unsigned long long *__restrict__ keys, uint32_t m, unsigned long long want)
{
  uint32_t lo = 0, hi = m;
  while (lo < hi)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] <= want)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// what an entry is to a site: the table F (bit 2 * s + k = breakend s falls into interval k) and, where a mapping holds, the hit
struct KnownHit
{
  uint32_t F;
  bool hit, crossed, oriented, opposed;
  uint32_t dist;
};

__device__ __forceinline__ KnownHit known_entry(const int32_t tid[2], const long long x[2], const uint32_t side[2], const struct bk_known_entry &r, long long slop)
{
  const int32_t itid[2] = {r.tid1, r.tid2};
  const uint32_t ibeg[2] = {r.beg1, r.beg2}, iend[2] = {r.end1, r.end2};
  long long d[4];
  KnownHit h;
  h.F = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) h.F |= (uint32_t) known_falls(tid[a >> 1], x[a >> 1], itid[a & 1], ibeg[a & 1], iend[a & 1], slop, d[a]) << a;
  const bool straight = (h.F & 1u) && (h.F & 8u), cross = (h.F & 2u) && (h.F & 4u);
  const bool stated = r.strand1 != BK_STRAND_NONE && r.strand2 != BK_STRAND_NONE;
  const bool st_agree = stated && r.strand1 == side[0] && r.strand2 == side[1], cr_agree = stated && r.strand1 == side[1] && r.strand2 == side[0];
  const long long st_dist = d[0] + d[3], cr_dist = d[1] + d[2];
  h.hit = straight || cross;
  // the first by: agrees, then the smaller dist, then straight
  h.crossed = cross && (!straight || (cr_agree != st_agree ? cr_agree : cr_dist < st_dist));
  h.oriented = h.hit && (h.crossed ? cr_agree : st_agree);
  h.opposed = h.hit && stated && !h.oriented;
  h.dist = h.hit ? (uint32_t) (h.crossed ? cr_dist : st_dist) : 0u;
  return h;
}

// One wavefront per site, four to a workgroup; no LDS and no barrier.  Every read of the index is 0 <= q <= top < m, every entry read
// is vals[q] >> 1 < n_entries.  The loop's trip count and its exit are the same on every lane, so the ballots of the listing pass see
// the whole wavefront.
// LIST false: the row but for n_names (0), and cnt[i] = n_hits.  LIST true: (i << 32) | name of every hit at off[i] + its slot, the
// slot being the number of hits in front of it in the walk; the predicate is the first pass's on the same data, so the slots fill the
// segment exactly, and the bound is tested all the same.
template <bool LIST>
__global__ __launch_bounds__(256) void k_known_sites(const struct bk_known_site *__restrict__ sites, uint32_t n, const struct bk_known_entry *__restrict__ entries,
                                                     const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ iend,
                                                     const uint32_t *__restrict__ run_max, uint32_t m, uint32_t slop_u, struct bk_known_call *__restrict__ res,
                                                     unsigned long long *__restrict__ cnt, const unsigned long long *__restrict__ off, unsigned long long *__restrict__ nkey)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const struct bk_known_site me = sites[i];
  const int32_t tid[2] = {me.tid1, me.tid2};
  const long long x[2] = {(long long) me.pos1 - 1, (long long) me.pos2 - 1};
  const uint32_t side[2] = {me.right1 + 1u, me.right2 + 1u};  // BK_STRAND_LEFT / BK_STRAND_RIGHT
  const long long slop = slop_u;

  uint32_t n_hits = 0, n_oriented = 0, n_opposed = 0, n_side[2] = {0, 0};
  unsigned long long best_key = 0;  // (score biased to unsigned) << 21 | (DIST_MASK - dist): the largest wins; 0 = no hit
  uint32_t best_info = 0xFFFFFFFFu;  // entry << 2 | crossed << 1 | oriented: among equal keys the smallest entry wins
  unsigned long long seg = 0, seg_end = 0, filled = 0;
  if (LIST)
  {
    seg = off[i], seg_end = off[i + 1];
    if (seg == seg_end) return;
  }
  const unsigned long long below = (1ull << lane) - 1ull;

  for (int s = 0; s < (LIST ? 1 : 2); ++s)
  {
    if (tid[s] < 0 || m == 0) continue;
    long long hi = x[s] + slop;
    const long long lo = x[s] - slop;  // an interval reaches the breakend when end - 1 >= lo (and it begins at or before hi)
    if (hi < 0) continue;
    if (hi > 0xFFFFFFFFll) hi = 0xFFFFFFFFll;
    const unsigned long long contig = (unsigned long long) ((long long) tid[s] + 1);
    const uint32_t upto = known_upper(keys, m, (contig << 32) | (unsigned long long) hi);
    for (long long top = (long long) upto - 1; top >= 0; top -= 64)  // (top is the same on every lane)
    {
      if ((keys[top] >> 32) != contig || (long long) run_max[top] - 1 < lo) break;  // no interval of this contig up to `top` reaches
      const long long q = top - (long long) lane;
      bool mine = false;
      uint32_t name = 0;
      if (q >= 0 && (keys[q] >> 32) == contig && (long long) iend[q] - 1 >= lo)
      {
        const uint32_t v = vals[q], e = v >> 1, k = v & 1u;
        const struct bk_known_entry r = entries[e];
        const KnownHit h = known_entry(tid, x, side, r, slop);
        // breakend s falls into interval k of e; the entry is counted at the first interval that holds this breakend
        const bool first = !(k == 1u && (h.F & (1u << (2 * s))));
        if (first)
        {
          ++n_side[s];
          if (s == 0 && h.hit)
          {
            mine = true;
            name = r.name;
            ++n_hits;
            n_oriented += h.oriented;
            n_opposed += h.opposed;
            const unsigned long long key = ((unsigned long long) ((uint32_t) r.score ^ 0x80000000u) << 21) | (unsigned long long) (DIST_MASK - h.dist);
            const uint32_t info = (e << 2) | ((uint32_t) h.crossed << 1) | (uint32_t) h.oriented;
            if (key > best_key || (key == best_key && info < best_info)) best_key = key, best_info = info;
          }
        }
      }
      if (LIST)
      {
        const unsigned long long who = __ballot(mine);
        const unsigned long long at = seg + filled + (unsigned long long) __popcll(who & below);
        if (mine && at < seg_end) nkey[at] = ((unsigned long long) i << 32) | name;
        filled += (unsigned long long) __popcll(who);
      }
    }
  }
  if (LIST) return;

  n_hits = wave_sum(n_hits);
  n_oriented = wave_sum(n_oriented);
  n_opposed = wave_sum(n_opposed);
  n_side[0] = wave_sum(n_side[0]);
  n_side[1] = wave_sum(n_side[1]);
  const unsigned long long top_key = wave_max(best_key);
  const uint32_t top_info = wave_min(best_key == top_key && best_key ? best_info : 0xFFFFFFFFu);

  struct bk_known_call r;
  r.n_hits = n_hits, r.n_oriented = n_oriented, r.n_opposed = n_opposed, r.n_names = 0;
  r.n_side[0] = n_side[0], r.n_side[1] = n_side[1];
  r.best = -1, r.best_score = BK_KNOWN_NO_SCORE, r.best_dist = 0;
  r.best_crossed = r.best_oriented = 0;
  r.reserved[0] = r.reserved[1] = 0;
  if (top_key)
  {
    r.best = (int32_t) (top_info >> 2);
    r.best_score = (int32_t) ((uint32_t) (top_key >> 21) ^ 0x80000000u);
    r.best_dist = DIST_MASK - ((uint32_t) top_key & DIST_MASK);
    r.best_crossed = (uint8_t) ((top_info >> 1) & 1u);
    r.best_oriented = (uint8_t) (top_info & 1u);
  }
  if (lane == 0)
  {
    res[i] = r;
    cnt[i] = n_hits;
  }
}

// ---- the distinct names: one wavefront per site over its sorted segment, 64 rows a step -------------------------------------------------
// Row r opens a run when it is the segment's first or differs from row r - 1 (within a segment only the name can differ).  Every read is
// seg <= r - 1 < r < seg_end <= the listed hits.
__global__ __launch_bounds__(256) void k_known_name_heads(uint32_t n, const unsigned long long *__restrict__ nkey, const unsigned long long *__restrict__ off,
                                                          struct bk_known_call *__restrict__ res)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const unsigned long long seg = off[i], seg_end = off[i + 1];
  uint32_t heads = 0;
  for (unsigned long long r = seg + lane; r < seg_end; r += 64) heads += r == seg || nkey[r] != nkey[r - 1];
  heads = wave_sum(heads);
  if (lane == 0) res[i].n_names = heads;
}
}  // namespace

using runs::bits_of;

int KnownShape::key_bits() const { return m ? 32 + bits_of((uint64_t) max_tid + 1) : 0; }
int KnownShape::name_bits() const { return bits_of(max_name); }
int KnownShape::site_bits() const { return n ? bits_of(n - 1) : 0; }
uint32_t KnownShape::index_passes() const { return (uint32_t) ((key_bits() + 7) / 8); }
uint32_t KnownShape::name_passes() const { return (uint32_t) ((name_bits() + 7) / 8 + (site_bits() + 7) / 8); }
uint64_t KnownShape::touched_index() const { return n_entries * (sizeof(struct bk_known_entry) + 24ull + 48ull * index_passes()) + 16ull * m; }
uint64_t KnownShape::touched_sites(uint64_t hits) const { return n * (sizeof(struct bk_known_site) + sizeof(struct bk_known_call) + 16ull) + hits * (12ull + 24ull * name_passes()); }

void known_upload(const struct bk_known_entry *entries, uint64_t n_entries, const struct bk_known_site *sites, uint64_t n, KnownBufs &b, hipStream_t st)
{
  b.d_entries = upload(b.entries, entries, n_entries, st);
  b.d_sites = upload(b.sites, sites, n, st);
}

void known_index(const KnownShape &shape, KnownBufs &b, hipStream_t st)
{
  static_assert(sizeof(struct bk_known_entry) == 40 && sizeof(struct bk_known_site) == 24 && sizeof(struct bk_known_call) == 40, "bk_known_entry and bk_known_call must be 40 bytes, bk_known_site 24");
  b.ikeys = nullptr;
  b.ivals = nullptr;
  const uint32_t ne = (uint32_t) shape.n_entries, m = (uint32_t) shape.m;
  if (!ne) return;
  unsigned long long *keys = b.keys.as<unsigned long long>(2ull * ne);
  uint32_t *vals = b.vals.as<uint32_t>(2ull * ne);
  hipLaunchKernelGGL(k_known_keys, dim3(cdiv(ne, 256)), dim3(256), 0, st, b.d_entries, ne, keys, vals);
  if (!m) return;
  // the sorted intervals with a contig: the 2 ne - m others sort in front (key 0) and are left out from here on
  uint64_t *sk;
  uint32_t *sv;
  prims::radix_sort_pairs((uint64_t *) keys, vals, 2ull * ne, 0, shape.key_bits(), b.rx_index, st, &sk, &sv);
  b.ikeys = (const unsigned long long *) sk + (2ull * ne - m);
  b.ivals = sv + (2ull * ne - m);
  uint32_t *iend = b.iend.as<uint32_t>(m), *run_max = b.run_max.as<uint32_t>(m);
  hipLaunchKernelGGL(k_known_ends, dim3(cdiv(m, 256)), dim3(256), 0, st, b.d_entries, b.ivals, m, iend);
  hipLaunchKernelGGL(k_known_run_max, dim3(1), dim3(256), 0, st, b.ikeys, iend, m, run_max);
}

uint64_t known_count(const KnownShape &shape, uint32_t slop, KnownBufs &b, hipStream_t st, struct bk_known_call **res_out)
{
  const uint32_t n = (uint32_t) shape.n, m = b.ikeys ? (uint32_t) shape.m : 0u;
  struct bk_known_call *res = b.res.as<struct bk_known_call>(shape.n + 1);
  *res_out = res;
  if (!n) return 0;
  unsigned long long *cnt = b.cnt.as<unsigned long long>(n), *off = b.off.as<unsigned long long>((uint64_t) n + 1);
  hipLaunchKernelGGL(k_known_sites<false>, dim3(cdiv(n, 4)), dim3(256), 0, st, b.d_sites, n, b.d_entries, b.ikeys, b.ivals, b.iend.get<uint32_t>(), b.run_max.get<uint32_t>(), m, slop,
                     res, cnt, (const unsigned long long *) nullptr, (unsigned long long *) nullptr);
  prims::exclusive_scan<unsigned long long>(cnt, off, n, b.scan_tmp, st);
  unsigned long long total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, off + n, sizeof total, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));  // the only wait: the list of names is sized from the total
  return total;
}

void known_names(const KnownShape &shape, uint32_t slop, uint64_t hits, KnownBufs &b, hipStream_t st)
{
  const uint32_t n = (uint32_t) shape.n, m = (uint32_t) shape.m;
  if (!n || !hits) return;  // (every n_names is 0 already)
  struct bk_known_call *res = b.res.get<struct bk_known_call>();
  const unsigned long long *off = b.off.get<unsigned long long>();
  unsigned long long *nkey = b.nkey.as<unsigned long long>(hits);
  uint32_t *nval = b.nval.as<uint32_t>(hits);  // the sort carries a value; nothing reads it
  HIP_CHECK(hipMemsetAsync(nval, 0, hits * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_known_sites<true>, dim3(cdiv(n, 4)), dim3(256), 0, st, b.d_sites, n, b.d_entries, b.ikeys, b.ivals, b.iend.get<uint32_t>(), b.run_max.get<uint32_t>(), m, slop,
                     res, (unsigned long long *) nullptr, off, nkey);
  // stable: by the name's bits in use, then by the site's.  A site's rows end up where the scan put its segment.
  uint64_t *k1, *k2;
  uint32_t *v1, *v2;
  prims::radix_sort_pairs((uint64_t *) nkey, nval, hits, 0, shape.name_bits(), b.rx_name, st, &k1, &v1);
  prims::radix_sort_pairs(k1, v1, hits, 32, 32 + shape.site_bits(), b.rx_site, st, &k2, &v2);
  hipLaunchKernelGGL(k_known_name_heads, dim3(cdiv(n, 4)), dim3(256), 0, st, n, (const unsigned long long *) k2, off, res);
}
