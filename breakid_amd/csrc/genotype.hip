// Reference-allele evidence of every voted call (bk_ref_support): on each side of a call, how many reads align
// across the breakpoint base with `anchor` bases on either side, and how many properly paired fragments span it.  A window search
// over the resident, coordinate-sorted record table - one wavefront per (call, side), as k_bp_depth and k_normal_drp.
#include "genotype.h"

namespace
{
// With b = exact - 1 (0-based breakpoint base), A = anchor: a record counts only if pos <= b - A, and it reaches b + 1 + A only if
// pos >= b + 1 + A - max(maxspan, W) (its alignment is at most maxspan long, its fragment at most W).  Two record lookups bound the
// window [lo, hi); all its records lie on the side's chromosome.  Lanes stride over it, 64 records per step and the column loads
// of REF_STEPS steps in flight at once.  The CIGAR is walked only for eligible records that start within maxspan of the far
// bound: with 100-150 bp reads and a ~1.3 kb window about a tenth of them.  The loop has no bound of its own: a 5 000x panel
// locus puts ~10^5 records into one window, and every one of them is part of the count.
// (Both sides of a call in one wave, the two windows one after the other, measured 12 % slower at the bench shape: DESIGN.md §12.)
constexpr int REF_STEPS = 4;
constexpr uint16_t REF_FLAG_NEVER = 0x4 | 0x100 | 0x200 | 0x400 | 0x800;

__global__ __launch_bounds__(256) void k_ref_support(RecView r, const bk_cluster *__restrict__ cl, uint32_t ncl, int mapq_min, int A, int W, int maxspan,
                                                     uint32_t *__restrict__ res, RefStat *__restrict__ stat)
{
  const uint32_t wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t c = wv >> 1, side = wv & 1u;
  const int lane = threadIdx.x & 63;
  if (c >= ncl) return;
  const bk_cluster k = cl[c];
  const int32_t T = side ? k.p2_tid : k.p1_tid;
  const long long e = side ? (long long) k.p2_exact : (long long) k.p1_exact;
  const long long b = e - 1;
  const long long need = b + 1 + A;  // bam_endpos, or pos + isize, must reach this
  const long long pmax = b - A;      // ... from a pos no further right than this
  const long long plo = need - (maxspan > W ? maxspan : W);
  uint32_t n_reads = 0, n_pairs = 0, visited = 0, words = 0;
  if ((k.flags & 2u) && T >= 0 && r.n && plo <= 0x7FFFFFFFll && pmax >= -0x80000000ll)
  {
    const uint64_t lo = rec_lower(r, T, plo);
    // (a pos column is int32: beyond its range the window ends where the next chromosome begins)
    const uint64_t hi = pmax < 0x7FFFFFFFll ? rec_lower(r, T, pmax + 1) : rec_lower(r, T + 1, -0x80000000ll);
    visited = hi > lo ? (uint32_t) (hi - lo) : 0u;
    for (uint64_t base = lo; base < hi; base += REF_STEPS * 64)
    {
      int32_t p[REF_STEPS], is[REF_STEPS];
      uint32_t a0[REF_STEPS], a1[REF_STEPS];
      uint16_t f[REF_STEPS];
      uint8_t q[REF_STEPS];
#pragma unroll
      for (int s = 0; s < REF_STEPS; ++s)
      {
        const uint64_t i = base + (uint64_t) s * 64 + lane;
        const bool in = i < hi;
        p[s] = in ? r.pos[i] : 0;
        f[s] = in ? r.flag[i] : (uint16_t) 0;  // flag 0 lacks 0x1: never eligible
        q[s] = in ? r.mapq[i] : (uint8_t) 0;
        is[s] = in ? r.isize[i] : 0;
        a0[s] = in ? r.aux_off[i] : 0u;
        a1[s] = in ? r.aux_off[i + 1] : 0u;
      }
#pragma unroll
      for (int s = 0; s < REF_STEPS; ++s)
      {
        const bool elig = (f[s] & 1) && !(f[s] & REF_FLAG_NEVER) && (int) q[s] >= mapq_min && a1[s] == a0[s];
        const bool pair = elig && (f[s] & 2) && !(f[s] & 8) && is[s] > 0 && is[s] <= W && (long long) p[s] + is[s] >= need;
        bool read = false;
        if (elig && (long long) p[s] + maxspan >= need)
        {
          const uint64_t i = base + (uint64_t) s * 64 + lane;
          const uint32_t c0 = r.cigar_off[i], c1 = r.cigar_off[i + 1];
          read = (long long) bam_endpos_hts(f[s], p[s], r.cigar, c0, c1) >= need;
          words += c1 - c0;
        }
        n_reads += (uint32_t) __popcll(__ballot(read));
        n_pairs += (uint32_t) __popcll(__ballot(pair));
      }
    }
  }
  if (stat) words = wave_sum(words);
  if (lane == 0)
  {
    // struct bk_ref_support { ref_pairs1, ref_pairs2, ref_reads1, ref_reads2 }: each wave stores the two fields of its side
    res[4 * (uint64_t) c + side] = n_pairs;
    res[4 * (uint64_t) c + 2 + side] = n_reads;
    if (stat)
    {
      RefStat o;
      o.visited = visited;
      o.words = words;
      stat[wv] = o;
    }
  }
}
}  // namespace

void ref_support(const RecView &rec, int maxspan, const bk_cluster *cl, uint64_t ncl, int mapq_min, int anchor, double w, RefBufs &b, hipStream_t st,
                 struct bk_ref_support **out, RefStat **stat_out)
{
  static_assert(sizeof(struct bk_ref_support) == 16, "bk_ref_support must be 16 bytes");
  struct bk_ref_support *res = b.res.as<struct bk_ref_support>(ncl + 1);
  RefStat *stat = stat_out ? b.stat.as<RefStat>(2 * ncl + 2) : nullptr;
  *out = res;
  if (stat_out) *stat_out = stat;
  if (ncl == 0) return;
  if (ncl > 0x3FFFFFFFull) throw bk_error(BK_ERR_LIMIT, "too many clusters");
  const int W = (int) w;  // the integer the breakpoint stage passes as wi (bp.hip: bp_vote)
  const RecView r = rec_sampled(rec, b.samp, st);
  hipLaunchKernelGGL(k_ref_support, dim3(cdiv(2 * ncl, 4)), dim3(256), 0, st, r, cl, (uint32_t) ncl, mapq_min, anchor, W, maxspan, (uint32_t *) res, stat);
}
