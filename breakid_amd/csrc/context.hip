// Window context (bk_window_context): the record classes and the mapping quality of the records that START inside arbitrary
// windows, each window in time that does not depend on its length.  The table is coordinate-sorted, so the records of contig T with
// pos < x are a prefix of it; one streaming pass classifies every record and sums nine counters per tile of 256 records, scans make
// them prefixes, and a window is the difference of the prefix values at its two edges.  Membership is by start, so no record reaches
// across an edge and nothing is corrected afterwards (coverage.hip has to).
#include "context.h"

namespace
{
constexpr uint32_t CTX_TILE = 1u << CTX_TILE_SHIFT;
static_assert(CTX_TILE == 4 * 64, "k_ctx_tiles deals four records to each of 64 lanes");
constexpr uint32_t OP_S = 4, OP_H = 5;  // BAM CIGAR operations

// What a set of at most 256 records adds to the nine counters: eight counts of 10 bits each (256 < 1024), three to a word, and the
// sum of mapq (256 * 255 < 2^16).  Sets add word by word, and so does a wave.
struct CtxAcc
{
  uint32_t a, b, c, q;  // a: reads | mq0 << 10 | lowq << 20; b: clipped | improper << 10 | orphan << 20; c: dup | secsup << 10; q: mapq_sum
};
__device__ __forceinline__ void ctx_add(CtxAcc &x, const CtxAcc &y)
{
  x.a += y.a;
  x.b += y.b;
  x.c += y.c;
  x.q += y.q;
}
__device__ __forceinline__ CtxAcc ctx_wave_sum(CtxAcc v)
{
  v.a = wave_sum(v.a);
  v.b = wave_sum(v.b);
  v.c = wave_sum(v.c);
  v.q = wave_sum(v.q);
  return v;
}

// The nine counters as the CTX_ARRAYS 64-bit words the prefix arrays hold: word 0 is mapq_sum, word k = 1..4 holds counter 2k - 2 of
// the row's order (reads, mq0, lowq, clipped, improper, orphan, dup, secsup) in its low half and counter 2k - 1 in its high half.
// Two 32-bit counts share one 64-bit prefix: a low half that passes 2^32 carries into the high one, and the difference of two
// prefixes still has both halves right, because each half of a window's row is below 2^32 (the fields are uint32_t).
struct CtxWords
{
  unsigned long long w[CTX_ARRAYS];
};
__device__ __forceinline__ CtxWords ctx_words(const CtxAcc &v)
{
  auto pair = [](uint32_t lo, uint32_t hi) { return (unsigned long long) lo | ((unsigned long long) hi << 32); };
  CtxWords o;
  o.w[0] = v.q;
  o.w[1] = pair(v.a & 1023u, (v.a >> 10) & 1023u);
  o.w[2] = pair(v.a >> 20, v.b & 1023u);
  o.w[3] = pair((v.b >> 10) & 1023u, v.b >> 20);
  o.w[4] = pair(v.c & 1023u, v.c >> 10);
  return o;
}

// One record by the words of include/breakid_hip.h: its tid, flag, mapq and the CIGAR words [c0, c1).  The tile pass and the window
// kernel share it, so a record counts the same in a tile sum and in the partial tile in front of an edge.  It reads the first and the
// last CIGAR word, and the one beside either only where that end is a hard clip; every index lies in [c0, c1).
__device__ __forceinline__ CtxAcc ctx_record(const uint32_t *__restrict__ cigar, int32_t tid, uint16_t flag, uint8_t mapq, uint32_t c0, uint32_t c1, int mapq_min)
{
  CtxAcc o = {0, 0, 0, 0};
  if (tid < 0 || (flag & 0x4)) return o;  // not mapped: counts nowhere
  if (flag & (0x100 | 0x800))
  {
    o.c = 1u << 10;  // secsup, whatever 0x200 and 0x400 say
    return o;
  }
  if (flag & 0x200) return o;
  if (flag & 0x400)
  {
    o.c = 1u;  // dup
    return o;
  }
  // the base set
  bool clipped = false;
  if (c1 > c0)
  {
    uint32_t lo = c0, hi = c1;
    uint32_t first = cigar[lo] & 15u, last = cigar[hi - 1] & 15u;
    if (first == OP_H) ++lo;
    if (lo < hi && last == OP_H) --hi;
    if (lo < hi)
    {
      if (lo != c0) first = cigar[lo] & 15u;
      if (hi != c1) last = cigar[hi - 1] & 15u;
      clipped = first == OP_S || last == OP_S;
    }
  }
  const bool paired = flag & 0x1, mate_unmapped = flag & 0x8;
  o.a = 1u | ((uint32_t) (mapq == 0) << 10) | ((uint32_t) ((int) mapq < mapq_min) << 20);
  o.b = (uint32_t) clipped | ((uint32_t) (paired && !mate_unmapped && !(flag & 0x2)) << 10) | ((uint32_t) (paired && mate_unmapped) << 20);
  o.q = mapq;
  return o;
}

// Tile pass: one wavefront per tile, the layout of k_cov_tiles (coverage.hip).  Lane l takes the four consecutive records 4 l .. 4 l + 3
// of the tile and reads each column with one vector load (16 bytes of tid, 8 of flag, 4 of mapq, five cigar_off words): the fixed
// columns of every table form are 16-byte aligned (bk_upload_records) and a tile starts at a multiple of 256 records.  pos is not read.
// The CIGAR words a lane looks at lie in one contiguous run, and the runs of neighbouring lanes adjoin.  A lane whose four records are
// not all below n (the last tile only) reads them one by one, guarded: records at or beyond n do not exist (tid -1 counts nowhere).
// CTX_ARRAYS stores per tile, by lanes 0 .. CTX_ARRAYS - 1; array k begins at pre + k * stride.
__global__ __launch_bounds__(256) void k_ctx_tiles(RecView r, int mapq_min, uint64_t n_tiles, unsigned long long *__restrict__ pre, uint64_t stride)
{
  const uint64_t t = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const int lane = threadIdx.x & 63;
  const uint64_t i0 = (t << CTX_TILE_SHIFT) + 4u * (uint32_t) lane;
  int32_t td[4] = {-1, -1, -1, -1};
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
      c[s + 1] = r.cigar_off[i0 + s + 1];  // (cigar_off has n + 1 entries)
    }
  CtxAcc v = {0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < 4; ++s) ctx_add(v, ctx_record(r.cigar, td[s], f[s], q[s], c[s], c[s + 1], mapq_min));
  const CtxWords o = ctx_words(ctx_wave_sum(v));
  if (lane < (int) CTX_ARRAYS)
  {
    unsigned long long mine = o.w[0];
#pragma unroll
    for (uint32_t k = 1; k < CTX_ARRAYS; ++k) mine = lane == (int) k ? o.w[k] : mine;
    pre[(uint64_t) lane * stride + t] = mine;
  }
}

// (a pos column is int32: beyond its range the records in front of x are all those of the contig, as coverage.hip has it)
__device__ __forceinline__ uint64_t ctx_lower(const RecView &r, int32_t T, long long P)
{
  return P <= 0x7FFFFFFFll ? rec_lower(r, T, P) : rec_lower(r, (int32_t) ((uint32_t) T + 1u), -0x80000000ll);
}

// One edge x of a window on contig T, by a whole wave: the counters of the records in front of h = the first record of T with
// pos >= x, on every lane: the prefixes of tile h / 256 plus the records [h / 256 * 256, h) of that tile, at most 255.  Every index
// is < h <= r.n.
__device__ CtxWords ctx_edge(const RecView &r, const unsigned long long *__restrict__ pre, uint64_t stride, int32_t T, long long x, int mapq_min)
{
  const int lane = threadIdx.x & 63;
  const uint64_t h = ctx_lower(r, T, x);
  const uint64_t tile = h >> CTX_TILE_SHIFT;
  CtxAcc v = {0, 0, 0, 0};
  for (uint64_t i = (tile << CTX_TILE_SHIFT) + lane; i < h; i += 64) ctx_add(v, ctx_record(r.cigar, r.tid[i], r.flag[i], r.mapq[i], r.cigar_off[i], r.cigar_off[i + 1], mapq_min));
  CtxWords o = ctx_words(ctx_wave_sum(v));
#pragma unroll
  for (uint32_t k = 0; k < CTX_ARRAYS; ++k) o.w[k] += pre[k * stride + tile];
  return o;
}

// One wavefront per window, four to a workgroup (as k_window_coverage): its two edges one after the other, then one row by lane 0.
__global__ __launch_bounds__(256) void k_window_context(RecView r, const unsigned long long *__restrict__ pre, uint64_t stride, const struct bk_cov_window *__restrict__ win,
                                                        uint32_t n, int32_t n_targets, int mapq_min, struct bk_window_ctx *__restrict__ res)
{
  const uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  const struct bk_cov_window w = win[j];
  struct bk_window_ctx o = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (w.tid >= 0 && w.tid < n_targets && w.end > w.beg)
  {
    const CtxWords ea = ctx_edge(r, pre, stride, w.tid, (long long) w.beg, mapq_min);
    const CtxWords eb = ctx_edge(r, pre, stride, w.tid, (long long) w.end, mapq_min);
    unsigned long long d[CTX_ARRAYS];
#pragma unroll
    for (uint32_t k = 0; k < CTX_ARRAYS; ++k) d[k] = eb.w[k] - ea.w[k];
    o.mapq_sum = d[0];
    o.reads = (uint32_t) d[1], o.mq0 = (uint32_t) (d[1] >> 32);
    o.lowq = (uint32_t) d[2], o.clipped = (uint32_t) (d[2] >> 32);
    o.improper = (uint32_t) d[3], o.orphan = (uint32_t) (d[3] >> 32);
    o.dup = (uint32_t) d[4], o.secsup = (uint32_t) (d[4] >> 32);
  }
  if ((threadIdx.x & 63) == 0) res[j] = o;
}
}  // namespace

void ctx_tiles_build(const RecView &rec, int mapq_min, CtxBufs &b, hipStream_t st)
{
  const uint64_t nt = ctx_tiles(rec.n), stride = nt + 1;
  unsigned long long *pre = b.pre.as<unsigned long long>(CTX_ARRAYS * stride);
  if (nt) hipLaunchKernelGGL(k_ctx_tiles, dim3(cdiv(nt, 4)), dim3(256), 0, st, rec, mapq_min, nt, pre, stride);
  for (uint32_t k = 0; k < CTX_ARRAYS; ++k) prims::exclusive_scan<unsigned long long>(pre + k * stride, pre + k * stride, nt, b.scan_tmp, st);
}

void window_context(const RecView &rec, int32_t n_targets, uint64_t n, int mapq_min, CtxBufs &b, hipStream_t st, struct bk_window_ctx **res)
{
  static_assert(sizeof(struct bk_cov_window) == 16 && sizeof(struct bk_window_ctx) == 40, "bk_cov_window must be 16 bytes and bk_window_ctx 40");
  struct bk_window_ctx *out = b.res.as<struct bk_window_ctx>(n + 1);
  *res = out;
  if (n == 0) return;
  const RecView r = rec_sampled(rec, b.samp, st);
  hipLaunchKernelGGL(k_window_context, dim3(cdiv(n, 4)), dim3(256), 0, st, r, b.pre.get<unsigned long long>(), ctx_tiles(rec.n) + 1, b.win.get<struct bk_cov_window>(), (uint32_t) n,
                     n_targets, mapq_min, out);
}
