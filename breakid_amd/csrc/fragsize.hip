// The fragment lengths the member pairs imply across each call's junction (bk_fragment_sizes).
//   listing   evidence() in its pairs_only form lists the BK_EV_PAIR rows of every call, packed, into buffers of this stage's own
//   lengths   one lane per (row, side), the two sides of a row on neighbouring lanes.  A row whose strands do not fit the site is off
//             and looks nothing up.  Otherwise the lane finds the first record of the row's (tid, pos) by a binary search of its own
//             (the sampled keys of rec_lower's table, then the stride) and walks the records of that position for flag and name
//             hash: FRAG_LANE_WALK records on its own; what is still open then is finished by the whole wavefront, one open lane
//             after the other, 64 records a step (a pile-up of thousands of records at one position is 64 times fewer round trips,
//             and the other lanes of the wave do not idle behind one).  The walk starts at the front of the run, so the record
//             it finds is the one of smallest index.  The side-1 lane adds the two retained lengths and writes one FragLen.
//   reduction one wavefront per call, four to a workgroup, walks its FragLen entries 64 a step twice: counts, extremes and the
//             sum, then the deviations from the centre; lane 0 writes the row as three 16-byte stores
// Nothing hands out a slot and no result is accumulated by atomics (FragStat is a statistic), so two runs give the same bytes.
#include "fragsize.h"
#include <cstddef>

namespace
{
static_assert(sizeof(struct bk_frag_site) == 16 && offsetof(struct bk_frag_site, right1) == 8 && offsetof(struct bk_frag_site, skip) == 10, "bk_frag_site must be 16 bytes");
static_assert(sizeof(struct bk_frag_sizes) == 48 && offsetof(struct bk_frag_sizes, min) == 20 && offsetof(struct bk_frag_sizes, sum) == 32 &&
                  offsetof(struct bk_frag_sizes, abs_dev) == 40,
              "bk_frag_sizes must be 48 bytes");
static_assert(sizeof(FragLen) == 8, "FragLen must be 8 bytes");

constexpr uint64_t NONE = ~0ull;
constexpr unsigned LENGTH_BLOCKS = 4096;  // k_fg_lengths strides: its statistics cost three atomics per workgroup, not per wave

// first record index with (tid, pos) >= (T, P), by one lane: rec_lower (bp.h) without the wavefront
__device__ uint64_t lane_lower(const RecView &r, int32_t T, long long P)
{
  uint64_t lo = 0, hi = r.n;
  if (r.samp)
  {
    const unsigned long long want = rec_key(T, P);
    uint64_t a = 0, b = r.n_samp;
    while (a < b)
    {
      const uint64_t m = (a + b) >> 1;
      if (r.samp[m] < want) a = m + 1;
      else b = m;
    }
    lo = a ? ((a - 1) << REC_SAMPLE_SHIFT) + 1 : 0;
    hi = a < r.n_samp ? (a << REC_SAMPLE_SHIFT) : r.n;
  }
  const uint32_t Tu = (uint32_t) T;
  while (lo < hi)
  {
    const uint64_t m = (lo + hi) >> 1;
    const uint32_t t = (uint32_t) r.tid[m];
    if (t != Tu ? (t < Tu) : ((long long) r.pos[m] < P)) lo = m + 1;
    else hi = m;
  }
  return lo;
}

__device__ __forceinline__ uint64_t rec_hash(const EvidenceRecs &recs, uint64_t i) { return recs.side ? recs.side[i].qhash : recs.qhash[i]; }

__global__ __launch_bounds__(256) void k_fg_lengths(RecView r, EvidenceRecs recs, const struct bk_evidence *__restrict__ rows, uint64_t n_rows,
                                                    const struct bk_frag_site *__restrict__ sites, uint32_t ncl, FragLen *__restrict__ out, FragStat *__restrict__ stat)
{
  __shared__ unsigned long long sh[3];
  __shared__ unsigned int sh_longest;
  if (threadIdx.x < 3) sh[threadIdx.x] = 0ull;
  if (threadIdx.x == 3) sh_longest = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  unsigned long long lookups = 0, walked = 0, wave_walks = 0;
  uint32_t longest = 0;
  const uint64_t n_lanes = 2 * n_rows, stride = (uint64_t) gridDim.x * 256u;
  for (uint64_t base = (uint64_t) blockIdx.x * 256u; base < n_lanes; base += stride)  // (the same trip count on every lane of the workgroup)
  {
    const uint64_t t = base + threadIdx.x;
    const bool live = t < n_lanes;
    const int s = (int) (t & 1u);
    bool want = false, off = false, lost = false, skip = false, right = false;
    int32_t T = 0;
    long long P1 = 0, site_pos = 0;  // the row's own position and the site's, both 1-based
    uint16_t F = 0;
    uint64_t H = 0;
    if (live)
    {
      const struct bk_evidence *row = rows + (t >> 1);
      const uint32_t c = row->call;
      if (c >= ncl)
      {
        stat->bad = 1u;
        skip = true;
      }
      else
      {
        const struct bk_frag_site site = sites[c];
        const uint16_t f1 = row->flag1, f2 = row->flag2;
        skip = site.skip != 0;
        off = !skip && ((((f1 & 0x10) != 0) != (site.right1 != 0)) || (((f2 & 0x10) != 0) != (site.right2 != 0)));
        want = !skip && !off;
        right = (s ? site.right2 : site.right1) != 0;
        site_pos = (long long) (s ? site.pos2 : site.pos1);
        T = s ? row->tid2 : row->tid1;
        P1 = (long long) (s ? row->pos2 : row->pos1);
        F = s ? f2 : f1;
        H = row->qhash;
      }
    }
    // the record of this side: the first of its position, then the walk
    const long long P0 = P1 - 1;
    uint64_t j = 0, R = NONE;
    uint32_t steps = 0;
    bool pending = false;
    if (want)
    {
      ++lookups;
      if (P0 > 0x7FFFFFFFll)
        lost = true;  // (a pos column is int32)
      else
      {
        j = lane_lower(r, T, P0);
        for (int k = 0; k < FRAG_LANE_WALK; ++k)
        {
          if (j >= r.n || r.tid[j] != T || (long long) r.pos[j] != P0)
          {
            lost = true;
            break;
          }
          ++steps;
          if (r.flag[j] == F && rec_hash(recs, j) == H)
          {
            R = j;
            break;
          }
          ++j;
        }
        pending = R == NONE && !lost;
      }
    }
    // what is still open: the whole wavefront, one lane's walk after the other, 64 records a step
    for (uint64_t pend = __ballot(pending); pend; pend &= pend - 1)
    {
      const int src = __ffsll((unsigned long long) pend) - 1;
      uint64_t j0 = __shfl((unsigned long long) j, src, 64);
      const int32_t T0 = __shfl(T, src, 64);
      const long long P00 = __shfl(P0, src, 64);
      const uint32_t F0 = (uint32_t) __shfl((int) F, src, 64);
      const uint64_t H0 = __shfl((unsigned long long) H, src, 64);
      uint64_t res = NONE;
      uint32_t wsteps = 0;
      for (;;)  // (the records are coordinate sorted: those of (T0, P00) are a prefix of the lanes; idx >= r.n ends the walk at the latest)
      {
        const uint64_t idx = j0 + lane;
        const bool same = idx < r.n && r.tid[idx] == T0 && (long long) r.pos[idx] == P00;
        const bool match = same && r.flag[idx] == (uint16_t) F0 && rec_hash(recs, idx) == H0;
        const uint64_t mb = __ballot(match), sb = __ballot(same);
        if (mb)
        {
          const int first = __ffsll((unsigned long long) mb) - 1;
          res = j0 + first;
          wsteps += (uint32_t) first + 1u;
          break;
        }
        wsteps += (uint32_t) __popcll(sb);
        if (sb != ~0ull) break;
        j0 += 64;
      }
      if (lane == src)
      {
        R = res;
        lost = res == NONE;
        steps += wsteps;
        ++wave_walks;
      }
    }
    long long a = 0;
    if (want && R != NONE)
    {
      if (right)
      {
        const long long E = (long long) bam_endpos_hts(r.flag[R], r.pos[R], r.cigar, r.cigar_off[R], r.cigar_off[R + 1]);  // 1-based: the last aligned base
        a = E - site_pos + 1;
      }
      else
        a = site_pos - P1 + 1;
    }
    walked += steps;
    if (steps > longest) longest = steps;
    const long long a_other = __shfl_xor(a, 1, 64);
    const bool lost_other = __shfl_xor((int) lost, 1, 64) != 0;
    if (live && s == 0)
    {
      FragLen v;
      v.len = 0;
      v.mark = skip ? FRAG_SKIP : off ? FRAG_OFF : (lost || lost_other) ? FRAG_LOST : FRAG_USED;
      if (v.mark == FRAG_USED)
      {
        long long L = a + a_other;
        if (L > 0x7FFFFFFFll) L = 0x7FFFFFFFll;
        if (L < -0x7FFFFFFFll) L = -0x7FFFFFFFll;
        v.len = (int32_t) L;
      }
      out[t >> 1] = v;
    }
  }
  lookups = wave_sum(lookups);
  walked = wave_sum(walked);
  wave_walks = wave_sum(wave_walks);
  longest = wave_max(longest);
  if (lane == 0)
  {
    atomicAdd(&sh[0], lookups);
    atomicAdd(&sh[1], walked);
    atomicAdd(&sh[2], wave_walks);
    atomicMax(&sh_longest, longest);
  }
  __syncthreads();
  if (threadIdx.x == 0 && sh[0])  // (statistics, not slots)
  {
    atomicAdd(&stat->lookups, sh[0]);
    atomicAdd(&stat->walked, sh[1]);
    if (sh[2]) atomicAdd(&stat->wave_walks, sh[2]);
    atomicMax(&stat->longest, sh_longest);
  }
}

// One wave per call over the FragLen entries of its pair rows.
__global__ __launch_bounds__(256) void k_fg_reduce(const FragLen *__restrict__ len, uint64_t n_rows, const uint64_t *__restrict__ pair_off,
                                                   const struct bk_frag_site *__restrict__ sites, uint32_t ncl, int32_t lo, int32_t hi, struct bk_frag_sizes *__restrict__ res,
                                                   FragStat *__restrict__ stat)
{
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= ncl) return;
  uint64_t b0 = pair_off[c], b1 = pair_off[c + 1];
  if (b0 > b1 || b1 > n_rows)
  {
    if (lane == 0) stat->bad = 1u;
    b0 = b1 = 0;
  }
  if (sites[c].skip) b0 = b1 = 0;
  uint32_t n_used = 0, n_off = 0, n_lost = 0, n_short = 0, n_long = 0;
  int32_t mn = 0x7FFFFFFF, mx = -0x7FFFFFFF - 1;
  long long sum = 0;
  for (uint64_t i = b0 + lane; i < b1; i += 64)
  {
    const FragLen v = len[i];
    if (v.mark == FRAG_OFF) ++n_off;
    else if (v.mark == FRAG_LOST) ++n_lost;
    else if (v.mark == FRAG_USED)
    {
      ++n_used;
      n_short += v.len < lo;
      n_long += v.len > hi;
      if (v.len < mn) mn = v.len;
      if (v.len > mx) mx = v.len;
      sum += v.len;
    }
  }
  n_used = wave_sum(n_used);
  n_off = wave_sum(n_off);
  n_lost = wave_sum(n_lost);
  n_short = wave_sum(n_short);
  n_long = wave_sum(n_long);
  sum = wave_sum(sum);
  for (int d = 32; d; d >>= 1)
  {
    const int32_t a = __shfl_xor(mn, d, 64), b = __shfl_xor(mx, d, 64);
    if (a < mn) mn = a;
    if (b > mx) mx = b;
  }
  unsigned long long dev = 0;
  if (n_used)  // (the same on every lane)
  {
    const long long num = 2 * sum + (long long) n_used, den = 2 * (long long) n_used;
    long long centre = num / den;
    if (num % den != 0 && num < 0) --centre;  // the floor goes towards minus infinity
    for (uint64_t i = b0 + lane; i < b1; i += 64)
    {
      const FragLen v = len[i];
      if (v.mark != FRAG_USED) continue;
      const long long d = (long long) v.len - centre;
      dev += (unsigned long long) (d < 0 ? -d : d);
    }
    dev = wave_sum(dev);
  }
  if (lane == 0)
  {
    struct bk_frag_sizes v;
    v.n_used = n_used;
    v.n_off = n_off;
    v.n_lost = n_lost;
    v.n_short = n_short;
    v.n_long = n_long;
    v.min = n_used ? mn : 0;
    v.max = n_used ? mx : 0;
    v.reserved = 0;
    v.sum = sum;
    v.abs_dev = dev;
    uint4 t[3];
    __builtin_memcpy(t, &v, sizeof v);
    uint4 *o4 = reinterpret_cast<uint4 *>(res + c);  // (rows start 16-byte aligned: 48-byte rows in a hipMalloc'ed array)
    o4[0] = t[0];
    o4[1] = t[1];
    o4[2] = t[2];
  }
}
}  // namespace

void fragsize_upload(const struct bk_frag_site *sites, uint64_t n, FragBufs &b, hipStream_t st)
{
  struct bk_frag_site *d = b.sites.as<struct bk_frag_site>(n + 1);
  if (n) HIP_CHECK(hipMemcpyAsync(d, sites, n * sizeof(struct bk_frag_site), hipMemcpyHostToDevice, st));
}

void fragment_sizes(const JunctionPairs &p, const TupleTable &tt, const bk_cluster *cl, uint64_t ncl, const EvidenceRecs &recs, const RecView &rec, int32_t lo, int32_t hi,
                    FragBufs &b, hipStream_t st, struct bk_frag_sizes **res_out, FragLen **len_out, uint64_t **pair_off_out, uint64_t *n_rows_out, EvidenceStat **ev_stat_out,
                    FragStat **stat_out)
{
  FragStat *stat = b.stat.as<FragStat>(1);
  HIP_CHECK(hipMemsetAsync(stat, 0, sizeof(FragStat), st));
  *stat_out = stat;
  struct bk_evidence *rows;
  evidence(p, tt, cl, ncl, recs, b.ev, st, &rows, pair_off_out, ev_stat_out, nullptr, true);
  uint64_t n_rows = 0;
  if (ncl)
  {
    HIP_CHECK(hipMemcpyAsync(&n_rows, *pair_off_out + ncl, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }
  *n_rows_out = n_rows;
  struct bk_frag_sizes *res = b.res.as<struct bk_frag_sizes>(ncl + 1);
  FragLen *len = b.len.as<FragLen>(n_rows + 1);
  *res_out = res;
  *len_out = len;
  if (ncl == 0) return;
  const struct bk_frag_site *sites = b.sites.get<struct bk_frag_site>();
  if (n_rows)
  {
    const RecView r = rec_sampled(rec, b.samp, st);
    const unsigned grid = cdiv(2 * n_rows, 256);
    hipLaunchKernelGGL(k_fg_lengths, dim3(grid < LENGTH_BLOCKS ? grid : LENGTH_BLOCKS), dim3(256), 0, st, r, recs, rows, n_rows, sites, (uint32_t) ncl, len, stat);
  }
  hipLaunchKernelGGL(k_fg_reduce, dim3(cdiv(ncl, 4)), dim3(256), 0, st, len, n_rows, *pair_off_out, sites, (uint32_t) ncl, lo, hi, res, stat);
}
