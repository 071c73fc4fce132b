// Partner loci (bk_locus_partners): for arbitrary windows, how many ends of the sample's discordant pairs lie inside,
// how many of them have their mate inside the window's partner, and into how many loci the mates of the others fall.  The 2 P ends
// of the BK_STAGE_SCAN table are indexed by ((tid + 1) << 32) | pos with the library's radix sort, the mates' keys gathered into that
// order.  One wavefront per site searches its range of the index, counts, and writes the mates that go elsewhere into a segment of its
// own at scanned offsets; the rows are sorted by (site, mate key) and one wavefront per site walks its segment for the runs.  Integer
// arithmetic only, no atomics: two runs give the same bytes.
#include "partners.h"
#include "runs.h"

namespace
{
constexpr int PT_STEPS = 4;  // ballots of 64 mates whose loads are in flight together

__device__ __forceinline__ uint64_t locus_key(int32_t tid, uint32_t pos) { return ((uint64_t) ((long long) tid + 1) << 32) | pos; }

// end 2 i is side 1 of pair i, end 2 i + 1 side 2: the key of its own locus and its number
__global__ __launch_bounds__(256) void k_partner_keys(const bk_pair *__restrict__ pairs, uint64_t np, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
  const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  const bk_pair p = pairs[i];
  key[2 * i] = locus_key(p.p1_tid, p.p1_pos);
  key[2 * i + 1] = locus_key(p.p2_tid, p.p2_pos);
  val[2 * i] = (uint32_t) (2 * i);
  val[2 * i + 1] = (uint32_t) (2 * i + 1);
}

// mkey[q] = the key of the mate of the q-th end in sorted order (vals[q] < 2 np: a value that k_partner_keys wrote)
__global__ __launch_bounds__(256) void k_partner_mates(const bk_pair *__restrict__ pairs, const uint32_t *__restrict__ vals, uint64_t ne, uint64_t *__restrict__ mkey)
{
  const uint64_t q = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (q >= ne) return;
  const uint32_t e = vals[q];
  const bk_pair p = pairs[e >> 1];
  mkey[q] = (e & 1u) ? locus_key(p.p1_tid, p.p1_pos) : locus_key(p.p2_tid, p.p2_pos);
}

// the partner window of a site as a range of mate keys; lo > hi: no end goes to the partner
struct PartnerRange
{
  uint64_t lo, hi;
  __device__ __forceinline__ bool holds(uint64_t k) const { return k >= lo && k <= hi; }
};
__device__ __forceinline__ PartnerRange partner_range(const struct bk_partner_site &s)
{
  if (s.mtid < 0 || s.mend < s.mbeg) return PartnerRange{1ull, 0ull};
  return PartnerRange{locus_key(s.mtid, s.mbeg), locus_key(s.mtid, s.mend)};
}

// ---- count: one wavefront per site, four to a workgroup; no LDS and no barrier ----------------------------------------------------
// [lo, hi) = the ends of the index inside the site's own window.  info[i] = (lo, ends, to_partner, 0); cnt[i] = the ends that go
// elsewhere.  Every read of the index is q < hi <= ne.
__global__ __launch_bounds__(256) void k_partner_count(const struct bk_partner_site *__restrict__ sites, uint32_t n, int32_t nt, const uint64_t *__restrict__ ikeys,
                                                       const uint64_t *__restrict__ mkey, uint64_t ne, uint4 *__restrict__ info, uint64_t *__restrict__ cnt)
{
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (i >= n) return;
  const struct bk_partner_site s = sites[i];
  uint64_t lo = 0, hi = 0;
  uint32_t to_partner = 0;
  if (ne > 0 && s.tid >= 0 && s.tid < nt && s.beg <= s.end)
  {
    const uint64_t klo = locus_key(s.tid, s.beg), khi = locus_key(s.tid, s.end);
    lo = wave_lower(0, ne, [&](uint64_t m) { return ikeys[m] < klo; });
    hi = wave_lower(lo, ne, [&](uint64_t m) { return ikeys[m] <= khi; });
    const PartnerRange pr = partner_range(s);
    for (uint64_t base = lo; base < hi; base += PT_STEPS * 64)
    {
      uint64_t k[PT_STEPS];
      bool in[PT_STEPS];
#pragma unroll
      for (int t = 0; t < PT_STEPS; ++t)
      {
        const uint64_t q = base + (uint64_t) t * 64 + lane;
        in[t] = q < hi;
        k[t] = in[t] ? mkey[q] : 0ull;
      }
#pragma unroll
      for (int t = 0; t < PT_STEPS; ++t) to_partner += (uint32_t) __popcll(__ballot(in[t] && pr.holds(k[t])));
    }
  }
  if (lane == 0)
  {
    const uint32_t ends = (uint32_t) (hi - lo);  // (ne < 2^32: the sort's limit)
    info[i] = make_uint4((uint32_t) lo, ends, to_partner, 0u);
    cnt[i] = ends - to_partner;
  }
}

// ---- expand: the mates that go elsewhere, into the site's segment [off[i], off[i + 1]) ---------------------------------------------
// A row's slot is the number of such mates in front of it: those of the earlier ballots plus those of the lower lanes in its own.  The
// predicate is k_partner_count's on the same data, so the slots fill the segment exactly; the bound is tested all the same.
__global__ __launch_bounds__(256) void k_partner_expand(const struct bk_partner_site *__restrict__ sites, uint32_t n, const uint64_t *__restrict__ mkey,
                                                        const uint4 *__restrict__ info, const uint64_t *__restrict__ off, uint64_t *__restrict__ rkey,
                                                        uint32_t *__restrict__ rsite)
{
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (i >= n) return;
  const uint64_t seg = off[i], seg_end = off[i + 1];
  if (seg == seg_end) return;
  const uint4 f = info[i];
  const uint64_t lo = f.x, hi = (uint64_t) f.x + f.y;
  const PartnerRange pr = partner_range(sites[i]);
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t filled = 0;
  for (uint64_t base = lo; base < hi; base += PT_STEPS * 64)
  {
    uint64_t k[PT_STEPS];
    bool in[PT_STEPS];
#pragma unroll
    for (int t = 0; t < PT_STEPS; ++t)
    {
      const uint64_t q = base + (uint64_t) t * 64 + lane;
      in[t] = q < hi;
      k[t] = in[t] ? mkey[q] : 0ull;
    }
#pragma unroll
    for (int t = 0; t < PT_STEPS; ++t)
    {
      const bool mine = in[t] && !pr.holds(k[t]);
      const uint64_t who = __ballot(mine);
      const uint64_t at = seg + filled + (uint64_t) __popcll(who & below);
      if (mine && at < seg_end)
      {
        rkey[at] = k[t];
        rsite[at] = i;
      }
      filled += (uint64_t) __popcll(who);
    }
  }
}

// ---- between the two sorts of the rows -----------------------------------------------------------------------------------------------
// the rows are sorted by mate key; the second sort's key is the row's site, its value the row's place in that order
__global__ __launch_bounds__(256) void k_partner_site_keys(const uint32_t *__restrict__ site, uint64_t nr, uint64_t *__restrict__ skey, uint32_t *__restrict__ spos)
{
  const uint64_t j = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (j >= nr) return;
  skey[j] = site[j];
  spos[j] = (uint32_t) j;
}
// fkey[r] = the mate key of the r-th row in (site, mate key) order (spos[r] < nr: a value that k_partner_site_keys wrote)
__global__ __launch_bounds__(256) void k_partner_gather(const uint64_t *__restrict__ key_by_mate, const uint32_t *__restrict__ spos, uint64_t nr, uint64_t *__restrict__ fkey)
{
  const uint64_t r = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (r >= nr) return;
  fkey[r] = key_by_mate[spos[r]];
}

// ---- runs: one wavefront per site over its sorted segment, 64 rows a step -------------------------------------------------------------
// Row r opens a run when it is the segment's first, when its contig differs from row r - 1's, or when its position exceeds that row's
// by more than max_gap.  The open run is carried as its first row (`open`); a lane whose row opens a run closes the one before it,
// which started at the nearest opening row below the lane, or at `open`.  A closed run is the candidate (length << 32) | ~(first row
// in the segment): the largest candidate is the longest run, and among equals the first.  Every read is seg <= r < seg_end <= nr.
__global__ __launch_bounds__(256) void k_partner_runs(uint32_t n, const uint64_t *__restrict__ fkey, const uint64_t *__restrict__ off, const uint4 *__restrict__ info,
                                                      uint32_t max_gap, struct bk_locus_partners *__restrict__ res)
{
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (i >= n) return;
  const uint64_t seg = off[i], seg_end = off[i + 1];
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t best = 0, open = seg;
  uint32_t loci = 0;
  auto candidate = [&](uint64_t first, uint64_t len) { return (len << 32) | (0xFFFFFFFFull - (first - seg)); };  // (len and first - seg are below 2^32)
  for (uint64_t base = seg; base < seg_end; base += 64)
  {
    const uint64_t r = base + lane;
    bool opens = false;
    if (r < seg_end)
    {
      opens = r == seg;
      if (!opens)
      {
        const uint64_t a = fkey[r - 1], b = fkey[r];  // a <= b
        opens = (a >> 32) != (b >> 32) || b - a > (uint64_t) max_gap;
      }
    }
    const uint64_t who = __ballot(opens);
    if (opens && r != seg)
    {
      const uint64_t lower = who & below;
      const uint64_t first = lower ? base + (uint64_t) (63 - __clzll((long long) lower)) : open;
      const uint64_t c = candidate(first, r - first);
      best = c > best ? c : best;
    }
    if (who) open = base + (uint64_t) (63 - __clzll((long long) who));
    loci += (uint32_t) __popcll(who);
  }
  if (seg < seg_end)
  {
    const uint64_t c = candidate(open, seg_end - open);  // the run that the segment's end closes
    best = c > best ? c : best;
  }
  best = wave_max(best);
  if (lane == 0)
  {
    const uint4 f = info[i];
    uint4 head = make_uint4(f.y, f.z, loci, 0u), tail = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);  // (top_tid = -1)
    if (best)
    {
      const uint64_t len = best >> 32, first = seg + (0xFFFFFFFFull - (best & 0xFFFFFFFFull));
      const uint64_t a = fkey[first], b = fkey[first + len - 1];
      head.w = (uint32_t) len;
      tail = make_uint4((uint32_t) (a >> 32) - 1u, (uint32_t) a, (uint32_t) b, 0u);
    }
    uint4 *row = reinterpret_cast<uint4 *>(res + i);
    row[0] = head;
    row[1] = tail;
  }
}

using runs::bits_of;
int site_bits(uint64_t n_sites) { return n_sites ? bits_of(n_sites - 1) : 0; }
}  // namespace

int partners_key_bits(int32_t n_targets) { return 32 + bits_of((uint64_t) n_targets + 1); }

uint32_t partners_row_passes(int32_t n_targets, uint64_t n_sites) { return (uint32_t) ((partners_key_bits(n_targets) + 7) / 8 + (site_bits(n_sites) + 7) / 8); }

uint64_t partners_touched_index(uint64_t n_pairs) { return n_pairs * sizeof(bk_pair) + 2 * n_pairs * 12ull; }

uint64_t partners_touched_sites(int32_t n_targets, uint64_t n_sites, uint64_t n_rows) { return n_sites * 64ull + n_rows * 12ull * partners_row_passes(n_targets, n_sites); }

void partners_upload(const struct bk_partner_site *sites, uint64_t n, PartnerBufs &b, hipStream_t st)
{
  struct bk_partner_site *d = b.sites.as<struct bk_partner_site>(n + 1);
  if (n) HIP_CHECK(hipMemcpyAsync(d, sites, n * sizeof(struct bk_partner_site), hipMemcpyHostToDevice, st));
  b.d_sites = d;
}

void partners_index(const bk_pair *pairs, uint64_t n_pairs, int32_t n_targets, PartnerBufs &b, hipStream_t st)
{
  const uint64_t ne = 2 * n_pairs;
  b.ikeys = b.imates = nullptr;
  b.n_ends = ne;
  if (!ne) return;
  prims::radix_check_count(ne);
  uint64_t *key = b.key.as<uint64_t>(ne), *sk;
  uint32_t *val = b.val.as<uint32_t>(ne), *sv;
  hipLaunchKernelGGL(k_partner_keys, dim3(cdiv(n_pairs, 256)), dim3(256), 0, st, pairs, n_pairs, key, val);
  prims::radix_sort_pairs(key, val, ne, 0, partners_key_bits(n_targets), b.rx_index, st, &sk, &sv);
  uint64_t *mkey = b.mkey.as<uint64_t>(ne);
  hipLaunchKernelGGL(k_partner_mates, dim3(cdiv(ne, 256)), dim3(256), 0, st, pairs, sv, ne, mkey);
  b.ikeys = sk;
  b.imates = mkey;
}

uint64_t partners_count(int32_t n_targets, uint64_t n, PartnerBufs &b, hipStream_t st)
{
  if (!n) return 0;
  uint4 *info = b.info.as<uint4>(n);
  uint64_t *cnt = b.cnt.as<uint64_t>(n), *off = b.off.as<uint64_t>(n + 1);
  hipLaunchKernelGGL(k_partner_count, dim3(cdiv(n, 4)), dim3(256), 0, st, b.d_sites, (uint32_t) n, n_targets, b.ikeys, b.imates, b.n_ends, info, cnt);
  prims::exclusive_scan<uint64_t>(cnt, off, n, b.scan_tmp, st);
  uint64_t total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));  // the only wait: the row buffers are sized from the total
  return total;
}

void partners_rows(int32_t n_targets, uint64_t n, uint64_t nr, uint32_t max_gap, PartnerBufs &b, hipStream_t st, struct bk_locus_partners **res_out)
{
  static_assert(sizeof(struct bk_partner_site) == 32 && sizeof(struct bk_locus_partners) == 32, "bk_partner_site and bk_locus_partners must be 32 bytes");
  struct bk_locus_partners *res = b.res.as<struct bk_locus_partners>(n + 1);
  *res_out = res;
  if (!n) return;
  const uint4 *info = b.info.get<uint4>();
  const uint64_t *off = b.off.get<uint64_t>();
  const uint64_t *fkey = nullptr;
  if (nr)
  {
    uint64_t *rkey = b.rkey.as<uint64_t>(nr), *k1;
    uint32_t *rsite = b.rsite.as<uint32_t>(nr), *v1;
    hipLaunchKernelGGL(k_partner_expand, dim3(cdiv(n, 4)), dim3(256), 0, st, b.d_sites, (uint32_t) n, b.imates, info, off, rkey, rsite);
    // stable: by the mate key's bits, then by the site's.  A site's rows end up where the scan put its segment.
    prims::radix_sort_pairs(rkey, rsite, nr, 0, partners_key_bits(n_targets), b.rx_rows, st, &k1, &v1);
    uint64_t *skey = b.skey.as<uint64_t>(nr), *k2;
    uint32_t *spos = b.spos.as<uint32_t>(nr), *v2;
    hipLaunchKernelGGL(k_partner_site_keys, dim3(cdiv(nr, 256)), dim3(256), 0, st, v1, nr, skey, spos);
    prims::radix_sort_pairs(skey, spos, nr, 0, site_bits(n), b.rx_site, st, &k2, &v2);
    uint64_t *fk = b.fkey.as<uint64_t>(nr);
    hipLaunchKernelGGL(k_partner_gather, dim3(cdiv(nr, 256)), dim3(256), 0, st, k1, v2, nr, fk);
    fkey = fk;
  }
  hipLaunchKernelGGL(k_partner_runs, dim3(cdiv(n, 4)), dim3(256), 0, st, (uint32_t) n, fkey, off, info, max_gap, res);
}
