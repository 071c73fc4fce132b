// Window coverage (bk_window_coverage): the aligned bases of the eligible records inside arbitrary windows, each window
// in time that does not depend on its length.  The table is coordinate-sorted, so the records that start in front of a position x of
// contig T are a prefix of it; one streaming pass sums the eligible reference lengths per tile of 256 records, a scan makes them
// prefixes, and a window is the difference of two prefix values, corrected by the few records that reach across an edge.
#include "coverage.h"

namespace
{
constexpr uint16_t COV_FLAG_NEVER = 0x4 | 0x100 | 0x200 | 0x400 | 0x800;
constexpr uint32_t COV_TILE = 1u << COV_TILE_SHIFT;
static_assert(COV_TILE == 4 * 64, "k_cov_tiles deals four records to each of 64 lanes");

// reference length of BAM CIGAR words (M, D, N, =, X: BAM_CIGAR_TYPE 0x3C1A7, as cigar_reflen_hts), summed in 64 bits
__device__ __forceinline__ long long cov_reflen(const uint32_t *__restrict__ w, uint32_t n)
{
  long long l = 0;
  for (uint32_t k = 0; k < n; ++k)
  {
    const uint32_t v = w[k], op = v & 15u;
    if ((0x3C1A7u >> (op << 1)) & 2u) l += (long long) (v >> 4);
  }
  return l;
}
__device__ __forceinline__ bool cov_passes(int32_t tid, uint16_t flag, uint8_t mapq, int mapq_min) { return tid >= 0 && !(flag & COV_FLAG_NEVER) && (int) mapq >= mapq_min; }
// the eligible reference length of record i < r.n: 0 when it is not eligible.  The tile pass and the window kernel share it, so a
// record counts the same in a tile sum and in the partial tile in front of an edge.
__device__ __forceinline__ long long cov_len(const RecView &r, uint64_t i, int mapq_min)
{
  if (!cov_passes(r.tid[i], r.flag[i], r.mapq[i], mapq_min)) return 0;
  const uint32_t c0 = r.cigar_off[i], c1 = r.cigar_off[i + 1];
  return c1 > c0 ? cov_reflen(r.cigar + c0, c1 - c0) : 0;
}

// Tile pass: one wavefront per tile.  Lane l takes the four consecutive records 4 l .. 4 l + 3 of the tile and reads each column with one
// vector load (16 bytes of tid, 8 of flag, 4 of mapq, five cigar_off words): the fixed columns of every table form are 16-byte aligned
// (bk_upload_records) and a tile starts at a multiple of 256 records.  The four CIGARs of a lane are one contiguous run of words, and the
// runs of neighbouring lanes adjoin.  A lane whose four records are not all below n (the last tile only) reads them one by one, guarded:
// records at or beyond n do not exist.  One pair of stores per tile, by lane 0.
__global__ __launch_bounds__(256) void k_cov_tiles(RecView r, int mapq_min, uint64_t n_tiles, unsigned long long *__restrict__ len, unsigned long long *__restrict__ cnt)
{
  const uint64_t t = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const int lane = threadIdx.x & 63;
  const uint64_t i0 = (t << COV_TILE_SHIFT) + 4u * (uint32_t) lane;
  int32_t td[4] = {-1, -1, -1, -1};  // tid -1: never eligible
  uint16_t f[4] = {0, 0, 0, 0};
  uint8_t q[4] = {0, 0, 0, 0};
  uint32_t c[5] = {0, 0, 0, 0, 0};
  if (i0 + 4 <= r.n)
  {
    const int4 tv = *reinterpret_cast<const int4 *>(r.tid + i0);
    const ushort4 fv = *reinterpret_cast<const ushort4 *>(r.flag + i0);
    const uchar4 qv = *reinterpret_cast<const uchar4 *>(r.mapq + i0);
    const uint4 cv = *reinterpret_cast<const uint4 *>(r.cigar_off + i0);
    td[0] = tv.x; td[1] = tv.y; td[2] = tv.z; td[3] = tv.w;
    f[0] = fv.x; f[1] = fv.y; f[2] = fv.z; f[3] = fv.w;
    q[0] = qv.x; q[1] = qv.y; q[2] = qv.z; q[3] = qv.w;
    c[0] = cv.x; c[1] = cv.y; c[2] = cv.z; c[3] = cv.w;
    c[4] = r.cigar_off[i0 + 4];
  }
  else
    for (int s = 0; s < 4 && i0 + s < r.n; ++s)
    {
      td[s] = r.tid[i0 + s];
      f[s] = r.flag[i0 + s];
      q[s] = r.mapq[i0 + s];
      c[s] = r.cigar_off[i0 + s];
      c[s + 1] = r.cigar_off[i0 + s + 1];  // (a record beyond n keeps c[s + 1] == c[s] or 0: tid -1 bars it)
    }
  long long l = 0, k = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s)
  {
    if (!cov_passes(td[s], f[s], q[s], mapq_min) || c[s + 1] <= c[s]) continue;
    const long long v = cov_reflen(r.cigar + c[s], c[s + 1] - c[s]);
    l += v;
    k += v > 0;
  }
  l = wave_sum(l);
  k = wave_sum(k);
  if (lane == 0)
  {
    len[t] = (unsigned long long) l;
    cnt[t] = (unsigned long long) k;
  }
}

// (a pos column is int32: beyond its range the records in front of x are all those of the contig, as clip.hip has it)
__device__ __forceinline__ uint64_t cov_lower(const RecView &r, int32_t T, long long P)
{
  return P <= 0x7FFFFFFFll ? rec_lower(r, T, P) : rec_lower(r, (int32_t) ((uint32_t) T + 1u), -0x80000000ll);
}

// One edge x of a window on contig T, by a whole wave.  h = the first record of T with pos >= x.  On every lane afterwards:
//   below    = the eligible length of the records in front of h that lies in front of x: S(h) - over(x)
//   n_below  = the eligible records in front of h: C(h)
//   straddle = the eligible records with pos < x < endpos
// S(h), C(h): the tile prefix at h / 256 and the records [h / 256 * 256, h) of the partial tile.  over(x): a record that reaches x
// starts no further than maxspan in front of it, so the walk begins at the first record of T with pos >= x - maxspan; all its
// records lie on T.  Both walks end at h, so they are one loop from the smaller start.  Every index is < h <= r.n.
struct CovEdge
{
  long long below, n_below, straddle;
};
__device__ CovEdge cov_edge(const RecView &r, const unsigned long long *__restrict__ len, const unsigned long long *__restrict__ cnt, int32_t T, long long x, int maxspan,
                            int mapq_min)
{
  const int lane = threadIdx.x & 63;
  const uint64_t h = cov_lower(r, T, x), lo = cov_lower(r, T, x - maxspan);
  const uint64_t tile = h >> COV_TILE_SHIFT, tile0 = tile << COV_TILE_SHIFT;
  long long s = 0, c = 0, st = 0;
  for (uint64_t i = (lo < tile0 ? lo : tile0) + lane; i < h; i += 64)
  {
    const long long l = cov_len(r, i, mapq_min);
    if (l <= 0) continue;
    if (i >= tile0)
    {
      s += l;
      ++c;
    }
    const long long e = (long long) r.pos[i] + l;
    if (i >= lo && e > x)
    {
      s -= e - x;
      ++st;
    }
  }
  CovEdge o;
  o.below = (long long) len[tile] + wave_sum(s);
  o.n_below = (long long) cnt[tile] + wave_sum(c);
  o.straddle = wave_sum(st);
  return o;
}

// One wavefront per window, four to a workgroup (as k_base_depth_at).  The overlap of a record with [a, b) is what it has in front of
// b less what it has in front of a; a record overlaps when it starts in front of b and does not end at or in front of a.
__global__ __launch_bounds__(256) void k_window_coverage(RecView r, const unsigned long long *__restrict__ len, const unsigned long long *__restrict__ cnt,
                                                         const struct bk_cov_window *__restrict__ win, uint32_t n, int32_t n_targets, int maxspan, int mapq_min,
                                                         struct bk_window_cov *__restrict__ res)
{
  const uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  const struct bk_cov_window w = win[j];
  struct bk_window_cov o = {0, 0, 0};
  if (w.tid >= 0 && w.tid < n_targets && w.end > w.beg)
  {
    const CovEdge ea = cov_edge(r, len, cnt, w.tid, (long long) w.beg, maxspan, mapq_min);
    const CovEdge eb = cov_edge(r, len, cnt, w.tid, (long long) w.end, maxspan, mapq_min);
    o.bases = (uint64_t) (eb.below - ea.below);
    o.reads = (uint32_t) (eb.n_below - ea.n_below + ea.straddle);
  }
  if ((threadIdx.x & 63) == 0) res[j] = o;
}
}  // namespace

void cov_tiles_build(const RecView &rec, int mapq_min, CovBufs &b, hipStream_t st)
{
  const uint64_t nt = cov_tiles(rec.n);
  unsigned long long *len = b.len.as<unsigned long long>(nt + 1), *cnt = b.cnt.as<unsigned long long>(nt + 1);
  if (nt) hipLaunchKernelGGL(k_cov_tiles, dim3(cdiv(nt, 4)), dim3(256), 0, st, rec, mapq_min, nt, len, cnt);
  prims::exclusive_scan<unsigned long long>(len, len, nt, b.scan_tmp, st);
  prims::exclusive_scan<unsigned long long>(cnt, cnt, nt, b.scan_tmp, st);
}

void window_coverage(const RecView &rec, int32_t n_targets, int maxspan, uint64_t n, int mapq_min, CovBufs &b, hipStream_t st, struct bk_window_cov **res)
{
  static_assert(sizeof(struct bk_cov_window) == 16 && sizeof(struct bk_window_cov) == 16, "bk_cov_window and bk_window_cov must be 16 bytes");
  struct bk_window_cov *out = b.res.as<struct bk_window_cov>(n + 1);
  *res = out;
  if (n == 0) return;
  const RecView r = rec_sampled(rec, b.samp, st);
  hipLaunchKernelGGL(k_window_coverage, dim3(cdiv(n, 4)), dim3(256), 0, st, r, b.len.get<unsigned long long>(), b.cnt.get<unsigned long long>(),
                     b.win.get<struct bk_cov_window>(), (uint32_t) n, n_targets, maxspan, mapq_min, out);
}
