// Soft-clip evidence of every cluster (bk_clip_support): on each side of a cluster, the soft-clipped reads without an
// SA tag whose clip sits inside the cluster's window - how many, where they pile up, and how many sit at the voted breakpoint.  A
// window search over the resident, coordinate-sorted record table - one wavefront (a workgroup of its own) per (call, side).
#include "clip.h"
#include <cstddef>

namespace
{
constexpr int CLIP_STEPS = 4;

// a pos column is int32: beyond its range a bound is where the next chromosome begins
__device__ __forceinline__ uint64_t clip_lower(const RecView &r, int32_t T, long long P)
{
  return P <= 0x7FFFFFFFll ? rec_lower(r, T, P) : rec_lower(r, (int32_t) ((uint32_t) T + 1u), -0x80000000ll);
}

// The window [lo, hi] is data (p_max - p_min) plus a parameter (W): it has no upper bound, so it is walked in tiles of CLIP_TILE
// positions.  A tile [t0, t1) looks at the records with pos in [t0 - 1 - maxspan, t1 - 1] (a leading event lies at pos + 1, a trailing
// one at most maxspan further right) and counts only the events that fall into it, each into the LDS counter of its position and
// direction; a record that two neighbouring tiles see is so counted once.  After the tile every lane scans its share of the
// counters, and the largest (the smallest position on a tie) is folded into the running best: tiles ascend, so a later tile wins
// only with a larger count.  Tiles without records are skipped: the next record of the chromosome says where to go on.
__global__ __launch_bounds__(64) void k_clip_support(RecView r, const bk_cluster *__restrict__ cl, uint32_t ncl, int mapq_min, int min_clip, int W, int maxspan,
                                                     uint32_t *__restrict__ res, ClipStat *__restrict__ stat)
{
  __shared__ uint32_t hist[2][CLIP_TILE];
  const uint32_t c = blockIdx.x >> 1, side = blockIdx.x & 1u;
  const int lane = threadIdx.x;
  if (c >= ncl) return;
  const bk_cluster k = cl[c];
  const int32_t T = side ? k.p2_tid : k.p1_tid;
  const bool voted = (k.flags & 2u) != 0;
  const long long e = side ? (long long) k.p2_exact : (long long) k.p1_exact;
  const long long pmin = side ? k.p2_min : k.p1_min, pmax = side ? k.p2_max : k.p1_max;
  const long long lo = pmin - W > 1 ? pmin - W : 1, hi = pmax + W;
  uint32_t n_at[2] = {0, 0}, n_ev[2] = {0, 0};      // per lane
  uint32_t best_n[2] = {0, 0}, best_p[2] = {0, 0};  // the same on every lane
  uint32_t visited = 0, words = 0, tiles = 0;
  if (T >= 0 && r.n)
  {
    long long t0 = lo;
    while (t0 <= hi)
    {
      const long long t1 = hi - t0 >= CLIP_TILE ? t0 + CLIP_TILE : hi + 1;
      const uint64_t rlo = clip_lower(r, T, t0 - 1 - maxspan), rhi = clip_lower(r, T, t1);
      if (rlo >= rhi)
      {
        if (t1 > hi || rlo >= r.n || r.tid[rlo] != T) break;
        t0 += ((long long) r.pos[rlo] + 1 - t0) / CLIP_TILE * CLIP_TILE;  // (that record starts at or behind t1: at least one tile on)
        continue;
      }
      ++tiles;
      visited += (uint32_t) (rhi - rlo);
      for (int j = lane; j < 2 * CLIP_TILE; j += 64) (&hist[0][0])[j] = 0u;
      __syncthreads();
      for (uint64_t base = rlo; base < rhi; base += CLIP_STEPS * 64)
      {
        int32_t p[CLIP_STEPS];
        uint32_t a0[CLIP_STEPS], a1[CLIP_STEPS];
        uint16_t f[CLIP_STEPS];
        uint8_t q[CLIP_STEPS];
#pragma unroll
        for (int s = 0; s < CLIP_STEPS; ++s)
        {
          const uint64_t i = base + (uint64_t) s * 64 + lane;
          const bool in = i < rhi;
          p[s] = in ? r.pos[i] : 0;
          f[s] = in ? r.flag[i] : (uint16_t) 0x4;  // never eligible
          q[s] = in ? r.mapq[i] : (uint8_t) 0;
          a0[s] = in ? r.aux_off[i] : 0u;
          a1[s] = in ? r.aux_off[i + 1] : 0u;
        }
#pragma unroll
        for (int s = 0; s < CLIP_STEPS; ++s)
        {
          if ((f[s] & CLIP_FLAG_NEVER) || (int) q[s] < mapq_min || a1[s] != a0[s]) continue;
          bool lead, trail;
          long long pt;
          uint32_t ll, lt;
          clip_events(r, base + (uint64_t) s * 64 + lane, p[s], min_clip, lead, trail, pt, words, ll, lt);
          const long long pl = (long long) p[s] + 1;
          if (lead && pl >= t0 && pl < t1)
          {
            atomicAdd(&hist[1][pl - t0], 1u);
            ++n_ev[1];
            if (voted && pl >= e - 2 && pl <= e + 2) ++n_at[1];
          }
          if (trail && pt >= t0 && pt < t1)
          {
            atomicAdd(&hist[0][pt - t0], 1u);
            ++n_ev[0];
            if (voted && pt >= e - 2 && pt <= e + 2) ++n_at[0];
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int d = 0; d < 2; ++d)
      {
        uint32_t bn = 0, bp = 0;
        for (int j = lane; j < CLIP_TILE; j += 64)
        {
          const uint32_t v = hist[d][j];
          if (v > bn) bn = v, bp = (uint32_t) j;
        }
        for (int x = 32; x; x >>= 1)
        {
          const uint32_t on = (uint32_t) __shfl_xor((int) bn, x, 64), op = (uint32_t) __shfl_xor((int) bp, x, 64);
          if (on > bn || (on == bn && op < bp)) bn = on, bp = op;
        }
        if (bn > best_n[d]) best_n[d] = bn, best_p[d] = (uint32_t) (t0 + bp);
      }
      __syncthreads();
      t0 = t1;
    }
    // a voted breakpoint lies inside its window; where it does not (a table the caller changed), the +-2 bp around it that the
    // window does not cover get a lookup of their own
    if (voted && (e - 2 < lo || e + 2 > hi))
    {
      const uint64_t rlo = clip_lower(r, T, e - 3 - maxspan), rhi = clip_lower(r, T, e + 2);
      visited += (uint32_t) (rhi > rlo ? rhi - rlo : 0);
      for (uint64_t i = rlo + lane; i < rhi; i += 64)
      {
        if ((r.flag[i] & CLIP_FLAG_NEVER) || (int) r.mapq[i] < mapq_min || r.aux_off[i + 1] != r.aux_off[i]) continue;
        bool lead, trail;
        long long pt;
        const int32_t pos = r.pos[i];
        uint32_t ll, lt;
        clip_events(r, i, pos, min_clip, lead, trail, pt, words, ll, lt);
        const long long pl = (long long) pos + 1;
        if (lead && pl >= e - 2 && pl <= e + 2 && !(pl >= lo && pl <= hi)) ++n_at[1];
        if (trail && pt >= e - 2 && pt <= e + 2 && !(pt >= lo && pt <= hi)) ++n_at[0];
      }
    }
  }
#pragma unroll
  for (int d = 0; d < 2; ++d)
  {
    n_at[d] = wave_sum(n_at[d]);
    n_ev[d] = wave_sum(n_ev[d]);
  }
  if (stat) words = wave_sum(words);
  if (lane == 0)
  {
    // struct bk_clip_support { at, peak_pos, peak_n, events }, each [side][dir]: a wave stores the two directions of its side
    uint32_t *o = res + 16 * (uint64_t) c + 2 * side;
#pragma unroll
    for (int d = 0; d < 2; ++d)
    {
      o[d] = n_at[d];
      o[4 + d] = best_p[d];
      o[8 + d] = best_n[d];
      o[12 + d] = n_ev[d];
    }
    if (stat)
    {
      ClipStat s;
      s.visited = visited;
      s.words = words;
      s.tiles = tiles;
      s.pad = 0;
      stat[blockIdx.x] = s;
    }
  }
}
// ---- bk_clip_reads: the clip events at caller-given sites, counted and listed -------------------------------------
// Count, scan, emit, as bk_evidence does it: no atomic hands out a slot.  One wavefront per site, four to a workgroup (a site is a
// handful of positions: no LDS counters, nothing shared between the waves).  The records that can hold an event of the site are
// those a tile [pos - tol, pos + tol] of k_clip_support would look at; both passes walk them in the same order with the same
// predicate, so the listing fills exactly the range the scan of the counts gave it - and says so when it does not.
static_assert(sizeof(struct bk_clip_site) == 16, "bk_clip_site must be 16 bytes");
static_assert(sizeof(struct bk_clip_read) == 40 && offsetof(struct bk_clip_read, qcheck) == 16 && offsetof(struct bk_clip_read, tid) == 24 &&
                  offsetof(struct bk_clip_read, clip_len) == 32 && offsetof(struct bk_clip_read, flag) == 36 && offsetof(struct bk_clip_read, dir) == 39,
              "bk_clip_read must be 40 bytes");

__device__ __forceinline__ void store_clip_read(struct bk_clip_read *__restrict__ o, const struct bk_clip_read &v)
{
  uint2 t[5];
  __builtin_memcpy(t, &v, sizeof v);
  uint2 *o2 = reinterpret_cast<uint2 *>(o);  // (40-byte rows in a hipMalloc'ed array start 8-byte aligned)
#pragma unroll
  for (int j = 0; j < 5; ++j) o2[j] = t[j];
}

struct ClipSiteOut
{
  // count pass
  uint32_t *counts;
  uint64_t *counts64;  // the same numbers as the scan's input
  ClipStat *stat;      // may be null
  // emit pass
  const uint64_t *site_off;
  struct bk_clip_read *rows;
  uint64_t n_rows;
  uint32_t *bad;
};

template <bool EMIT>
__device__ __forceinline__ void clip_site_walk(const RecView &r, const ClipNames &nm, const struct bk_clip_site *__restrict__ sites, uint32_t n_sites, int mapq_min,
                                               int min_clip, int maxspan, const ClipSiteOut &out)
{
  const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= n_sites) return;  // (the whole wave)
  const struct bk_clip_site site = sites[k];
  const int32_t T = site.tid;
  const long long p_lo = (long long) site.pos - (long long) site.tol, p_hi = (long long) site.pos + (long long) site.tol;
  const bool want_lead = site.dir == 1u;  // RIGHT: leading events; LEFT: trailing ones
  uint64_t rlo = 0, rhi = 0;
  if (T >= 0 && r.n)
  {
    rlo = clip_lower(r, T, p_lo - 1 - maxspan);
    rhi = clip_lower(r, T, p_hi);
  }
  const uint64_t below = (1ull << lane) - 1ull;
  const uint64_t row0 = EMIT ? out.site_off[k] : 0, limit = EMIT ? out.site_off[k + 1] : 0;
  uint32_t n_mine = 0, words = 0;
  uint64_t n_out = 0;
  bool wrong = false;
  for (uint64_t base = rlo; base < rhi; base += CLIP_STEPS * 64)  // (rlo and rhi are the same on every lane: so is the trip count)
  {
    int32_t p[CLIP_STEPS];
    uint32_t a0[CLIP_STEPS], a1[CLIP_STEPS];
    uint16_t f[CLIP_STEPS];
    uint8_t q[CLIP_STEPS];
#pragma unroll
    for (int s = 0; s < CLIP_STEPS; ++s)
    {
      const uint64_t i = base + (uint64_t) s * 64 + lane;
      const bool in = i < rhi;
      p[s] = in ? r.pos[i] : 0;
      f[s] = in ? r.flag[i] : (uint16_t) 0x4;  // never eligible
      q[s] = in ? r.mapq[i] : (uint8_t) 0;
      a0[s] = in ? r.aux_off[i] : 0u;
      a1[s] = in ? r.aux_off[i + 1] : 0u;
    }
#pragma unroll
    for (int s = 0; s < CLIP_STEPS; ++s)
    {
      const uint64_t i = base + (uint64_t) s * 64 + lane;
      bool hit = false;
      long long pe = 0;
      uint32_t len = 0;
      if (!((f[s] & CLIP_FLAG_NEVER) || (int) q[s] < mapq_min || a1[s] != a0[s]))
      {
        bool lead, trail;
        long long pt;
        uint32_t ll, lt;
        clip_events(r, i, p[s], min_clip, lead, trail, pt, words, ll, lt);
        pe = want_lead ? (long long) p[s] + 1 : pt;
        len = want_lead ? ll : lt;
        hit = (want_lead ? lead : trail) && pe >= p_lo && pe <= p_hi;
      }
      if (!EMIT)
        n_mine += hit ? 1u : 0u;
      else
      {
        const uint64_t m = __ballot(hit);  // (every lane is here: the filter above has closed)
        if (hit)
        {
          const uint64_t dest = row0 + n_out + (uint64_t) __popcll(m & below);
          if (dest >= limit || dest >= out.n_rows)
            wrong = true;  // a row outside its range is never written
          else
          {
            struct bk_clip_read v;
            v.rec = i;
            if (nm.side)
            {
              v.qhash = nm.side[i].qhash;
              v.qcheck = nm.side[i].qcheck;
            }
            else
            {
              v.qhash = nm.qhash[i];
              v.qcheck = nm.qcheck ? nm.qcheck[i] : 0u;
            }
            v.site = k;
            v.tid = T;
            v.p = (uint32_t) pe;
            v.clip_len = len;
            v.flag = f[s];
            v.mapq = q[s];
            v.dir = (uint8_t) site.dir;
            store_clip_read(out.rows + dest, v);
          }
        }
        n_out += (uint64_t) __popcll(m);
      }
    }
  }
  if (!EMIT)
  {
    const uint32_t n = wave_sum(n_mine);
    if (out.stat) words = wave_sum(words);
    if (lane == 0)
    {
      out.counts[k] = n;
      out.counts64[k] = n;
      if (out.stat)
      {
        ClipStat st;
        st.visited = (uint32_t) (rhi - rlo);
        st.words = words;
        st.tiles = 1;
        st.pad = 0;
        out.stat[k] = st;
      }
    }
  }
  else
  {
    const bool any_wrong = __ballot(wrong) != 0ull;
    if (lane == 0 && (any_wrong || row0 + n_out != limit)) *out.bad = 1u;  // the listing and the counts disagree
  }
}

__global__ __launch_bounds__(256) void k_clip_site_count(RecView r, ClipNames nm, const struct bk_clip_site *__restrict__ sites, uint32_t n_sites, int mapq_min, int min_clip,
                                                         int maxspan, ClipSiteOut out)
{
  clip_site_walk<false>(r, nm, sites, n_sites, mapq_min, min_clip, maxspan, out);
}
__global__ __launch_bounds__(256) void k_clip_site_emit(RecView r, ClipNames nm, const struct bk_clip_site *__restrict__ sites, uint32_t n_sites, int mapq_min, int min_clip,
                                                        int maxspan, ClipSiteOut out)
{
  clip_site_walk<true>(r, nm, sites, n_sites, mapq_min, min_clip, maxspan, out);
}
}  // namespace

void clip_support(const RecView &rec, int maxspan, const bk_cluster *cl, uint64_t ncl, int mapq_min, int min_clip, double w, ClipBufs &b, hipStream_t st,
                  struct bk_clip_support **out, ClipStat **stat_out)
{
  static_assert(sizeof(struct bk_clip_support) == 64, "bk_clip_support must be 64 bytes");
  struct bk_clip_support *res = b.res.as<struct bk_clip_support>(ncl + 1);
  ClipStat *stat = stat_out ? b.stat.as<ClipStat>(2 * ncl + 2) : nullptr;
  *out = res;
  if (stat_out) *stat_out = stat;
  if (ncl == 0) return;
  if (ncl > 0x3FFFFFFFull) throw bk_error(BK_ERR_LIMIT, "too many clusters");
  const int W = (int) w;  // the integer the breakpoint stage passes as wi (bp.hip: bp_vote)
  const RecView r = rec_sampled(rec, b.samp, st);
  hipLaunchKernelGGL(k_clip_support, dim3((unsigned) (2 * ncl)), dim3(64), 0, st, r, cl, (uint32_t) ncl, mapq_min, min_clip, W, maxspan, (uint32_t *) res, stat);
}

void clip_reads(const RecView &rec, const ClipNames &nm, int maxspan, const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, bool listing,
                bool want_stat, ClipReadBufs &b, hipStream_t st, ClipReadsOut &o)
{
  o.counts = b.counts.as<uint32_t>(n_sites + 1);
  o.site_off = b.site_off.as<uint64_t>(n_sites + 1);
  o.rows = b.rows.as<struct bk_clip_read>(1);
  o.stat = want_stat ? b.stat.as<ClipStat>(n_sites + 1) : nullptr;
  o.n_rows = 0;
  o.bad = false;
  if (n_sites == 0)
  {
    HIP_CHECK(hipMemsetAsync(o.site_off, 0, sizeof(uint64_t), st));
    return;
  }
  struct bk_clip_site *d_sites = b.sites.as<struct bk_clip_site>(n_sites);
  HIP_CHECK(hipMemcpyAsync(d_sites, sites, n_sites * sizeof(struct bk_clip_site), hipMemcpyHostToDevice, st));
  const RecView r = rec_sampled(rec, b.samp, st);
  const uint32_t n32 = (uint32_t) n_sites;
  ClipSiteOut out{};
  out.counts = o.counts;
  out.counts64 = b.counts64.as<uint64_t>(n_sites + 1);
  out.stat = o.stat;
  hipLaunchKernelGGL(k_clip_site_count, dim3(cdiv(n_sites, 4)), dim3(256), 0, st, r, nm, d_sites, n32, mapq_min, min_clip, maxspan, out);
  if (!listing) return;
  prims::exclusive_scan<uint64_t>(out.counts64, o.site_off, n_sites, b.scan_tmp, st);
  uint64_t total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, o.site_off + n_sites, 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));  // the row count sizes the listing
  if (total > 0xFFFFFFFFull) throw bk_error(BK_ERR_LIMIT, "bk_clip_reads: more than 2^32 rows");
  o.n_rows = total;
  if (total == 0) return;
  o.rows = b.rows.as<struct bk_clip_read>(total + 1);
  uint32_t *bad = b.bad.as<uint32_t>(1);
  HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(uint32_t), st));
  out.site_off = o.site_off;
  out.rows = o.rows;
  out.n_rows = total;
  out.bad = bad;
  hipLaunchKernelGGL(k_clip_site_emit, dim3(cdiv(n_sites, 4)), dim3(256), 0, st, r, nm, d_sites, n32, mapq_min, min_clip, maxspan, out);
  uint32_t h_bad = 0;
  HIP_CHECK(hipMemcpyAsync(&h_bad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  o.bad = h_bad != 0;
}
