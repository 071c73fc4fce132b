// Soft-clip pile-ups over the whole record table (bk_clip_loci).  The record pass is the hot one: one wavefront per tile
// of 256 records, four consecutive records a lane, flag, mapq, cigar_off and aux_off (and, in the count pass, tid) read as vectors; a
// record whose flag, mapq and empty aux blob pass goes through clip_events (clip.h: the one statement of the event rule).  Pass one sums
// the events of a tile, a scan makes the sums offsets, pass two looks at the records of the tiles that hold an event again and writes
// 32-byte event rows in record order.  Behind it: stable LSD stages of the radix sort by qhash (whose run heads rank the reads) and by
// (dir, tid, p); the heads of the exact sites, of the reads inside them and of the loci; one stage by (locus, read rank); one wavefront
// per locus for its row; one wavefront per locus for its facing partner; the mutual bit; one lane per locus for the claiming call; a
// scan that compacts.  Integer arithmetic only, no atomic: every result word has one writer.
#include "cliploci.h"
#include "runs.h"
#include <cstddef>

using runs::bits_of;
using runs::NONE;

namespace
{
static_assert(sizeof(struct bk_clip_locus) == 96 && offsetof(struct bk_clip_locus, clip_sum) == 56 && offsetof(struct bk_clip_locus, mate) == 80,
              "bk_clip_locus must be 96 bytes");

struct ClipEvent
{
  uint64_t qhash;
  uint32_t p;
  uint32_t dt;     // dir << 31 | tid
  uint32_t clip;   // length of the S op
  uint32_t fm;     // improper << 10 | orphan << 9 | reverse strand << 8 | mapq
  uint32_t qrank;  // dense rank of qhash among the events
  uint32_t pad;
};
static_assert(sizeof(ClipEvent) == 32, "event rows of cliploci.hip");

// ---- the record pass ------------------------------------------------------------------------------------------------------------------
// what the lane's four records look like to both passes: flag, mapq and the empty aux blob pass (bit s of `pass`)
struct ClipLane
{
  uint32_t c[5];
  uint32_t pass;
  uint16_t f[4];
  uint8_t q[4];
};

// Lane `lane` of tile t takes the records i0 = 256 t + 4 lane .. i0 + 3 and reads each column with one vector load (a tile starts at a
// multiple of 256 records); a lane whose four records are not all below n (the last tile only) reads them one by one, guarded.
// cigar_off and aux_off have n + 1 entries.
__device__ __forceinline__ ClipLane clip_lane(const RecView &r, uint64_t i0, int mapq_min)
{
  ClipLane o = {{0, 0, 0, 0, 0}, 0, {CLIP_FLAG_NEVER, CLIP_FLAG_NEVER, CLIP_FLAG_NEVER, CLIP_FLAG_NEVER}, {0, 0, 0, 0}};
  uint32_t a[5] = {0, 1, 2, 3, 4};  // (unequal neighbours: a record that is not read has an aux blob)
  if (i0 + 4 <= r.n)
  {
    const ushort4 fv = *reinterpret_cast<const ushort4 *>(r.flag + i0);
    const uchar4 qv = *reinterpret_cast<const uchar4 *>(r.mapq + i0);
    const uint4 cv = *reinterpret_cast<const uint4 *>(r.cigar_off + i0);
    const uint4 av = *reinterpret_cast<const uint4 *>(r.aux_off + i0);
    o.f[0] = fv.x; o.f[1] = fv.y; o.f[2] = fv.z; o.f[3] = fv.w;
    o.q[0] = qv.x; o.q[1] = qv.y; o.q[2] = qv.z; o.q[3] = qv.w;
    o.c[0] = cv.x; o.c[1] = cv.y; o.c[2] = cv.z; o.c[3] = cv.w;
    o.c[4] = r.cigar_off[i0 + 4];
    a[0] = av.x; a[1] = av.y; a[2] = av.z; a[3] = av.w;
    a[4] = r.aux_off[i0 + 4];
  }
  else
    for (int s = 0; s < 4 && i0 + s < r.n; ++s)
    {
      o.f[s] = r.flag[i0 + s];
      o.q[s] = r.mapq[i0 + s];
      o.c[s] = r.cigar_off[i0 + s];
      o.c[s + 1] = r.cigar_off[i0 + s + 1];
      a[s] = r.aux_off[i0 + s];
      a[s + 1] = r.aux_off[i0 + s + 1];
    }
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (!(o.f[s] & CLIP_FLAG_NEVER) && (int) o.q[s] >= mapq_min && a[s + 1] == a[s]) o.pass |= 1u << s;
  return o;
}

// a record's CIGAR words must lie inside the CIGAR array; one without a word has no reference length
__device__ __forceinline__ bool clip_walkable(uint32_t c0, uint32_t c1, uint64_t n_words) { return c1 > c0 && c1 <= n_words; }
// the reference length is above 0: stops at the first word that says so (the first or second of nearly every record)
__device__ __forceinline__ bool cigar_has_ref(const uint32_t *__restrict__ cg, uint32_t c0, uint32_t c1)
{
  for (uint32_t c = c0; c < c1; ++c)
    if (cigar_op_ref(cg[c])) return true;
  return false;
}

// The first and the last CIGAR word of the lane's records that are looked at (bit s of `look`), all loads in flight at once: the lane's
// words are neighbours in the CIGAR array, so clip_events, which loads its words itself one record after the other, then finds them
// in the cache, and the count of eligible records seldom needs another word.
struct ClipWords
{
  uint32_t first[4], last[4];
};
__device__ __forceinline__ ClipWords clip_words(const uint32_t *__restrict__ cg, const ClipLane &l, uint32_t look)
{
  ClipWords w;
#pragma unroll
  for (int s = 0; s < 4; ++s)
  {
    const bool on = (look >> s) & 1u;
    w.first[s] = on ? cg[l.c[s]] : 0u;
    w.last[s] = on ? cg[l.c[s + 1] - 1u] : 0u;
  }
  return w;
}

// The events of record i, which has passed flag, mapq and aux, tid >= 0 and clip_walkable: bit 0 of `kept` = the leading event (RIGHT, at
// pos + 1), bit 1 = the trailing one (LEFT, at bam_endpos), each only when it lies on its contig.
struct ClipRec
{
  uint32_t kept, beyond, elig;
  uint32_t p[2], len[2];
};
__device__ __forceinline__ ClipRec clip_record(const ClipLociInput &in, uint64_t i, uint32_t c0, uint32_t c1, int32_t tid, int min_clip, uint32_t w_first, uint32_t w_last)
{
  ClipRec o = {0, 0, 0, {0, 0}, {0, 0}};
  bool lead, trail;
  long long pt;
  uint32_t words = 0;
  // clip_events takes a table and an index and loads the record's two offsets itself.  The lane has them already: it is handed a view
  // whose offsets are these two, as record 0, so that no offset is loaded twice.  From pos 0: pt is the reference length.
  const uint32_t span[2] = {c0, c1};
  RecView one = in.rec;
  one.cigar_off = span;
  clip_events(one, 0, 0, min_clip, lead, trail, pt, words, o.len[0], o.len[1]);
  o.elig = lead || trail || cigar_op_ref(w_first) || cigar_op_ref(w_last) || cigar_has_ref(in.rec.cigar, c0, c1);
  if (!lead && !trail) return o;
  const int32_t pos = in.rec.pos[i];  // only a record with an event has its pos read
  pt += pos;
  const long long tl = runs::tlen(in.tprefix, in.nt, tid), pl = (long long) pos + 1;
  if (lead)
  {
    if (pl < 1 || pl > tl)
      ++o.beyond;
    else
      o.kept |= 1u, o.p[0] = (uint32_t) pl;
  }
  if (trail)
  {
    if (pt < 1 || pt > tl)
      ++o.beyond;
    else
      o.kept |= 2u, o.p[1] = (uint32_t) pt;
  }
  return o;
}

// Pass one.  tile_ev[t] = the kept events of tile t, tile_eb[t] = its eligible records | its events beyond a contig's end << 32.  tid is
// read for every record here (the table need not be sorted); pos and the CIGAR words only for a record that passes.
__global__ __launch_bounds__(256) void k_cll_count(ClipLociInput in, ClipLociParams p, uint64_t n_tiles, uint32_t *__restrict__ tile_ev, unsigned long long *__restrict__ tile_eb)
{
  const uint64_t t = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const int lane = threadIdx.x & 63;
  const RecView &r = in.rec;
  const uint64_t i0 = (t << runs::TILE_SHIFT) + 4u * (uint32_t) lane;
  const ClipLane l = clip_lane(r, i0, p.mapq_min);
  int32_t td[4] = {-1, -1, -1, -1};
  if (i0 + 4 <= r.n)
  {
    const int4 tv = *reinterpret_cast<const int4 *>(r.tid + i0);
    td[0] = tv.x; td[1] = tv.y; td[2] = tv.z; td[3] = tv.w;
  }
  else
    for (int s = 0; s < 4 && i0 + s < r.n; ++s) td[s] = r.tid[i0 + s];
  uint32_t ev = 0, elig = 0, beyond = 0, look = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (((l.pass >> s) & 1u) && td[s] >= 0 && clip_walkable(l.c[s], l.c[s + 1], in.n_cigar_words)) look |= 1u << s;
  const ClipWords w = clip_words(r.cigar, l, look);
#pragma unroll
  for (int s = 0; s < 4; ++s)
  {
    if (!((look >> s) & 1u)) continue;
    const ClipRec o = clip_record(in, i0 + s, l.c[s], l.c[s + 1], td[s], p.min_clip, w.first[s], w.last[s]);
    elig += o.elig;
    beyond += o.beyond;
    ev += (o.kept & 1u) + (o.kept >> 1);
  }
  ev = wave_sum(ev);
  elig = wave_sum(elig);
  beyond = wave_sum(beyond);
  if (lane == 0)
  {
    tile_ev[t] = ev;
    tile_eb[t] = (unsigned long long) elig | ((unsigned long long) beyond << 32);
  }
}

// Pass two.  ex = the exclusive scan of tile_ev (n_tiles + 1 entries).  A tile without an event ends at once.  A lane finds the events
// of its records, a wave scan gives its offset inside the tile, and it writes the rows: slot ex[t] + (the events of the lanes in
// front) + (its own so far), which is below ex[t + 1] <= ex[n_tiles] = the rows of `out`, because both passes apply the same rule to
// the same words.
__global__ __launch_bounds__(256) void k_cll_emit(ClipLociInput in, ClipLociParams p, uint64_t n_tiles, const uint32_t *__restrict__ ex, ClipEvent *__restrict__ out)
{
  const uint64_t t = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const uint32_t base = ex[t], end = ex[t + 1];
  if (base == end) return;
  const int lane = threadIdx.x & 63;
  const RecView &r = in.rec;
  const uint64_t i0 = (t << runs::TILE_SHIFT) + 4u * (uint32_t) lane;
  const ClipLane l = clip_lane(r, i0, p.mapq_min);
  int32_t td[4] = {-1, -1, -1, -1};
  ClipRec rc[4];
  uint32_t mine = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s)
  {
    rc[s] = ClipRec{0, 0, 0, {0, 0}, {0, 0}};
    if (!((l.pass >> s) & 1u) || !clip_walkable(l.c[s], l.c[s + 1], in.n_cigar_words)) continue;
    td[s] = r.tid[i0 + s];  // (pass is 0 for a record at or beyond n)
    if (td[s] < 0) continue;
    rc[s] = clip_record(in, i0 + s, l.c[s], l.c[s + 1], td[s], p.min_clip, r.cigar[l.c[s]], r.cigar[l.c[s + 1] - 1u]);
    mine += (rc[s].kept & 1u) + (rc[s].kept >> 1);
  }
  uint32_t slot = base + prims::wave_inclusive_scan(mine) - mine;
  if (!mine) return;
#pragma unroll
  for (int s = 0; s < 4; ++s)
  {
    if (!rc[s].kept) continue;
    const uint64_t i = i0 + s;
    const uint32_t f = l.f[s];
    ClipEvent e;
    e.qhash = in.side ? in.side[i].qhash : in.qhash[i];
    const uint32_t paired = f & 1u, munmap = (f >> 3) & 1u, proper = (f >> 1) & 1u;
    e.fm = ((paired & ~munmap & ~proper & 1u) << 10) | ((paired & munmap) << 9) | (((f >> 4) & 1u) << 8) | l.q[s];
    e.qrank = 0;
    e.pad = 0;
#pragma unroll
    for (uint32_t d = 0; d < 2; ++d)  // the leading event (RIGHT = 1) first
      if ((rc[s].kept >> d) & 1u)
      {
        e.p = rc[s].p[d];
        e.dt = ((d ^ 1u) << 31) | (uint32_t) td[s];
        e.clip = rc[s].len[d];
        if (slot < end) out[slot] = e;
        ++slot;
      }
  }
}

// ---- the sort stages ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t group_of(uint32_t dt, int tid_bits) { return ((uint64_t) (dt >> 31) << tid_bits) | (dt & 0x7FFFFFFFu); }

// keys[i] = the stage's key of event perm[i] (perm == nullptr: the identity); vals[i] = that event.  perm may be vals itself.
__global__ __launch_bounds__(256) void k_cll_keys(const ClipEvent *__restrict__ ev, const uint32_t *perm, uint32_t e, int mode, int pos_bits, int tid_bits, uint64_t *__restrict__ keys,
                                                  uint32_t *vals)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  const uint32_t k = perm ? perm[i] : i;  // (k < e: perm is a permutation that the sort made of the identity)
  const ClipEvent t = ev[k];
  keys[i] = mode == 0 ? t.qhash : (group_of(t.dt, tid_bits) << pos_bits) | t.p;
  vals[i] = k;
}

// over the rows sorted by (dir, tid, p, read rank): the heads of the loci, of the exact sites and of the reads inside an exact site;
// all 1 at i == 0
__global__ __launch_bounds__(256) void k_cll_heads(const ClipEvent *__restrict__ sorted, uint32_t e, uint32_t tol, uint32_t *__restrict__ lhead, uint32_t *__restrict__ xhead,
                                                   uint32_t *__restrict__ qhead)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  uint32_t l = 1, x = 1, q = 1;
  if (i)
  {
    const ClipEvent a = sorted[i - 1], b = sorted[i];
    l = a.dt != b.dt || b.p - a.p > tol;  // (b.p >= a.p inside one dt)
    x = l | (a.p != b.p);
    q = x | (a.qrank != b.qrank);
  }
  lhead[i] = l;
  xhead[i] = x;
  qhead[i] = q;
}

// (locus of the row) << rank_bits | read rank: equal keys are one read of one locus
__global__ __launch_bounds__(256) void k_cll_read_keys(const ClipEvent *__restrict__ sorted, const uint32_t *__restrict__ exl, uint32_t e, int rank_bits, uint64_t *__restrict__ keys,
                                                       uint32_t *__restrict__ vals)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  keys[i] = ((uint64_t) (exl[i + 1] - 1u) << rank_bits) | sorted[i].qrank;
  vals[i] = i;
}

// ---- the loci -----------------------------------------------------------------------------------------------------------------------
// One wavefront per locus l, four to a workgroup.  Its rows are [lstart[l], lstart[l + 1]) of the table sorted by (dir, tid, p, read
// rank), and the same range of the list sorted by (locus, read rank).  exx / exq / exd = the exclusive scans of the heads of the exact
// sites, of the reads inside them, and of the reads inside the loci; xstart = the first row of every exact site.  lkey[l] = the sort
// key of the representative: it ascends with l, because loci are disjoint intervals in the order of the sort.
__global__ __launch_bounds__(256) void k_cll_loci(const ClipEvent *__restrict__ sorted, const uint32_t *__restrict__ lstart, const uint32_t *__restrict__ xstart,
                                                  const uint32_t *__restrict__ exx, const uint32_t *__restrict__ exq, const uint32_t *__restrict__ exd, uint32_t n_loci,
                                                  uint32_t min_reads, int pos_bits, int tid_bits, struct bk_clip_locus *__restrict__ rows, uint64_t *__restrict__ lkey,
                                                  uint32_t *__restrict__ keep)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t l = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= n_loci) return;
  const uint32_t a = lstart[l], b = lstart[l + 1];  // (a < b <= e)
  uint32_t n_rev = 0, n_orphan = 0, n_improper = 0, max_clip = 0;
  unsigned long long mq = 0, cs = 0, rep = 0;
  for (uint32_t i = a + lane; i < b; i += 64)
  {
    const ClipEvent t = sorted[i];
    n_rev += (t.fm >> 8) & 1u;
    n_orphan += (t.fm >> 9) & 1u;
    n_improper += (t.fm >> 10) & 1u;
    mq += t.fm & 255u;
    cs += t.clip;
    max_clip = t.clip > max_clip ? t.clip : max_clip;
    if (exx[i + 1] != exx[i])
    {
      // (exx[i] is the exact site that begins at row i; exx[i] + 1 <= x).  The most reads, then the smaller p.
      const unsigned long long k = ((unsigned long long) (exq[xstart[exx[i] + 1]] - exq[i]) << 32) | (0xFFFFFFFFu - t.p);
      rep = k > rep ? k : rep;
    }
  }
  n_rev = wave_sum(n_rev);
  n_orphan = wave_sum(n_orphan);
  n_improper = wave_sum(n_improper);
  mq = wave_sum(mq);
  cs = wave_sum(cs);
  max_clip = wave_max(max_clip);
  rep = wave_max(rep);
  if (lane) return;
  struct bk_clip_locus r;
  const uint32_t dt = sorted[a].dt;  // (one direction and one contig in a locus)
  r.tid = (int32_t) (dt & 0x7FFFFFFFu);
  r.pos = 0xFFFFFFFFu - (uint32_t) rep;
  r.dir = dt >> 31;
  r.flags = 0;
  r.n_reads = exd[b] - exd[a];
  r.n_rows = b - a;
  r.n_exact = exx[b] - exx[a];
  r.top_reads = (uint32_t) (rep >> 32);
  r.lo_pos = sorted[a].p;
  r.hi_pos = sorted[b - 1].p;
  r.n_fwd = b - a - n_rev;
  r.n_rev = n_rev;
  r.max_clip = max_clip;
  r.n_orphan = n_orphan;
  r.clip_sum = cs;
  r.mapq_sum = mq;
  r.n_improper = n_improper;
  r.claim = NONE;
  r.mate = NONE;
  r.mate_pos = 0;
  r.mate_reads = 0;
  r.mate_off = 0;
  rows[l] = r;
  lkey[l] = (group_of(dt, tid_bits) << pos_bits) | r.pos;
  keep[l] = r.n_reads >= min_reads;
}

// the first j in [0, n) with keys[j] >= want (n when there is none)
__device__ __forceinline__ uint32_t lower_key(const uint64_t *__restrict__ keys, uint32_t n, uint64_t want)
{
  uint32_t lo = 0, hi = n;
  while (lo < hi)
  {
    const uint32_t m = lo + ((hi - lo) >> 1);
    if (keys[m] < want)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}

// One wavefront per locus l.  A LEFT locus at p faces the RIGHT loci of its contig at q with |q - p - 1| <= pair_dist, a RIGHT locus at q
// the LEFT ones at p: either way the partner's representative lies within pair_dist of centre = own + 1 (LEFT) or own - 1 (RIGHT).
// A search finds the first locus of the other direction at or above centre - pair_dist, and the wave walks 64 loci a step up to
// centre + pair_dist.  The partner: the most reads, then the smaller distance, then the smaller position (= the smaller index).
__global__ __launch_bounds__(256) void k_cll_facing(const struct bk_clip_locus *__restrict__ rows, const uint64_t *__restrict__ lkey, uint32_t n_loci, uint32_t pair_dist,
                                                    int pos_bits, int tid_bits, uint32_t *__restrict__ partner)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t l = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= n_loci) return;
  const uint64_t own = lkey[l], pmask = (1ull << pos_bits) - 1ull;
  const uint64_t g = own >> pos_bits, dir = g >> tid_bits;
  const long long centre = dir ? (long long) (own & pmask) - 1 : (long long) (own & pmask) + 1;
  long long lo = centre - (long long) pair_dist, hi = centre + (long long) pair_dist;
  lo = lo < 0 ? 0 : lo;
  hi = hi > (long long) pmask ? (long long) pmask : hi;
  const uint64_t og = g ^ (1ull << tid_bits);
  uint32_t best_n = 0;
  unsigned long long best_k = ~0ull;  // distance << 32 | index
  if (lo <= hi)
  {
    const uint64_t klo = (og << pos_bits) | (uint64_t) lo, khi = (og << pos_bits) | (uint64_t) hi;
    const uint32_t first = lower_key(lkey, n_loci, klo);
    for (uint32_t base = first; base < n_loci; base += 64)  // (uniform: every lane leaves at the same step)
    {
      const uint32_t j = base + lane;
      const bool in = j < n_loci && lkey[j] <= khi;
      if (in)
      {
        const long long q = (long long) (lkey[j] & pmask);
        const unsigned long long k = ((unsigned long long) (q > centre ? q - centre : centre - q) << 32) | j;
        const uint32_t n = rows[j].n_reads;
        if (n > best_n || (n == best_n && k < best_k)) best_n = n, best_k = k;
      }
      if (__ballot(in) != ~0ull) break;
    }
  }
#pragma unroll
  for (int d = 32; d; d >>= 1)
  {
    const uint32_t on = __shfl_xor(best_n, d, 64);
    const unsigned long long ok = __shfl_xor(best_k, d, 64);
    if (on > best_n || (on == best_n && ok < best_k)) best_n = on, best_k = ok;
  }
  if (lane == 0) partner[l] = best_n ? (uint32_t) best_k : NONE;  // (a locus has at least one read)
}

__global__ __launch_bounds__(256) void k_cll_mutual(const uint32_t *__restrict__ partner, uint32_t n_loci, uint32_t *__restrict__ mutual)
{
  const uint32_t l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n_loci) return;
  const uint32_t m = partner[l];
  mutual[l] = m < n_loci && partner[m] == l;
}

// ---- the claim ----------------------------------------------------------------------------------------------------------------------
// item 2 r + s = side s of cluster row r: key = tid << 32 | ps_exact for a voted side, `invalid` (above every valid key) otherwise
__global__ __launch_bounds__(256) void k_cll_bp_keys(const bk_cluster *__restrict__ cl, uint32_t m, int nt, uint64_t invalid, uint64_t *__restrict__ keys,
                                                     uint32_t *__restrict__ vals)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const bk_cluster c = cl[i >> 1];
  const int32_t tid = (i & 1u) ? c.p2_tid : c.p1_tid;
  const bool ok = (c.flags & 2u) && tid >= 0 && tid < nt && ((i & 1u) == 0 || c.p2_exact >= 0);
  const uint32_t pos = (i & 1u) ? (uint32_t) c.p2_exact : c.p1_exact;
  keys[i] = ok ? ((uint64_t) (uint32_t) tid << 32) | pos : invalid;
  vals[i] = i >> 1;
}

// one lane per locus: the smallest row among the breakpoints inside [lo_pos - 2, hi_pos + 2] of its contig
__global__ __launch_bounds__(256) void k_cll_claim(const struct bk_clip_locus *__restrict__ rows, uint32_t n_loci, const uint64_t *__restrict__ keys,
                                                   const uint32_t *__restrict__ vals, uint32_t m, uint32_t *__restrict__ claim)
{
  const uint32_t l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n_loci) return;
  const struct bk_clip_locus r = rows[l];
  const uint64_t t = (uint64_t) (uint32_t) r.tid << 32;
  const uint64_t hi = (uint64_t) r.hi_pos + 2u > 0xFFFFFFFFull ? 0xFFFFFFFFull : (uint64_t) r.hi_pos + 2u;
  const uint64_t klo = t | (r.lo_pos > 2u ? r.lo_pos - 2u : 0u), khi = t | hi;
  uint32_t best = NONE;
  for (uint32_t j = lower_key(keys, m, klo); j < m && keys[j] <= khi; ++j) best = vals[j] < best ? vals[j] : best;
  claim[l] = best;
}

// ---- the output -----------------------------------------------------------------------------------------------------------------------
// exk = the exclusive scan of keep: a kept locus l is output row exk[l]
__global__ __launch_bounds__(256) void k_cll_out(const struct bk_clip_locus *__restrict__ rows, const uint32_t *__restrict__ exk, const uint32_t *__restrict__ partner,
                                                 const uint32_t *__restrict__ mutual, const uint32_t *claim, uint32_t n_loci, struct bk_clip_locus *__restrict__ out)
{
  const uint32_t l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n_loci) return;
  if (exk[l + 1] == exk[l]) return;
  struct bk_clip_locus r = rows[l];
  const uint32_t m = partner[l];
  if (m < n_loci)
  {
    const struct bk_clip_locus o = rows[m];
    r.flags = 1u | (mutual[l] << 1);
    r.mate = exk[m + 1] != exk[m] ? exk[m] : NONE;
    r.mate_pos = o.pos;
    r.mate_reads = o.n_reads;
    r.mate_off = r.dir ? (int32_t) (r.pos - o.pos) : (int32_t) (o.pos - r.pos);  // q - p: RIGHT minus LEFT
  }
  if (claim) r.claim = claim[l];
  out[exk[l]] = r;
}

}  // namespace

// include/breakid_hip.h states both models
uint64_t ClipLociStats::touched_records() const
{
  const uint64_t tiles = runs::tiles_of(n);
  return n * 15ull + tiles * 56ull + std::min(events, tiles) * (runs::TILE * 11ull) + events * 48ull;
}

uint64_t ClipLociStats::touched_calls() const
{
  const uint64_t p1 = 8, p2 = ((uint64_t) pos_bits + tid_bits + 1 + 7) / 8, p3 = ((uint64_t) bits_of(loci) + bits_of(events) + 7) / 8;
  const uint64_t pb = (33ull + tid_bits + 7) / 8;
  return events * (36ull * (p1 + p2 + p3) + 376ull) + loci * 176ull + written * 224ull + breakpoints * (36ull * pb + 40ull);
}

void cliploci_events(const ClipLociInput &in, const ClipLociParams &p, ClipLociBufs &b, hipStream_t st, ClipLociStats *stats)
{
  ClipLociStats s;
  s.n = in.rec.n;
  s.pos_bits = bits_of(in.max_len);
  s.tid_bits = in.nt > 1 ? bits_of((uint64_t) in.nt - 1) : 0;
  *stats = s;
  runs::record_pass(
      in.rec.n, b, st, "bk_clip_loci: more than 2^30 events", *stats,
      [&](uint64_t nt, uint32_t *tile_ev, unsigned long long *tile_eb) { hipLaunchKernelGGL(k_cll_count, dim3(cdiv(nt, 4)), dim3(256), 0, st, in, p, nt, tile_ev, tile_eb); },
      [&](uint64_t nt, const uint32_t *ex) { hipLaunchKernelGGL(k_cll_emit, dim3(cdiv(nt, 4)), dim3(256), 0, st, in, p, nt, ex, b.ev.as<ClipEvent>(stats->events)); });
}

void cliploci_calls(const ClipLociParams &p, const bk_cluster *cl, uint64_t ncl, ClipLociBufs &b, hipStream_t st, struct bk_clip_locus **rows_out, ClipLociStats *stats)
{
  ClipLociStats s = *stats;
  *rows_out = b.out.as<struct bk_clip_locus>(1);
  if (s.events == 0) return;
  const uint32_t e = (uint32_t) s.events;
  const unsigned ge = cdiv(e, 256);
  ClipEvent *ev = b.ev.get<ClipEvent>();

  // stable LSD stages, least significant first: qhash (and its dense rank), (dir, tid, p)
  uint64_t *keys = b.keys.as<uint64_t>(e), *sk;
  uint32_t *vals = b.vals.as<uint32_t>(e), *sv;
  uint32_t *lhead = b.lhead.as<uint32_t>((uint64_t) e + 1), *xhead = b.xhead.as<uint32_t>((uint64_t) e + 1), *qhead = b.qhead.as<uint32_t>((uint64_t) e + 1);
  hipLaunchKernelGGL(k_cll_keys, dim3(ge), dim3(256), 0, st, ev, (const uint32_t *) nullptr, e, 0, s.pos_bits, s.tid_bits, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, 64, b.radix, st, &sk, &sv);
  hipLaunchKernelGGL(runs::k_key_heads, dim3(ge), dim3(256), 0, st, sk, e, 0, 0u, lhead, (uint32_t *) nullptr);
  prims::exclusive_scan<uint32_t>(lhead, lhead, e, b.scan_tmp, st);
  hipLaunchKernelGGL(runs::k_dense_rank<ClipEvent>, dim3(ge), dim3(256), 0, st, sv, lhead, e, ev);
  hipLaunchKernelGGL(k_cll_keys, dim3(ge), dim3(256), 0, st, ev, sv, e, 1, s.pos_bits, s.tid_bits, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, s.pos_bits + s.tid_bits + 1, b.radix, st, &sk, &sv);
  ClipEvent *sorted = b.sorted.as<ClipEvent>(e);
  hipLaunchKernelGGL(runs::k_gather_rows<ClipEvent>, dim3(ge), dim3(256), 0, st, ev, sv, e, sorted);

  // the loci, the exact sites and their reads
  uint32_t *exl = b.exl.as<uint32_t>((uint64_t) e + 1), *exx = b.exx.as<uint32_t>((uint64_t) e + 1), *exq = b.exq.as<uint32_t>((uint64_t) e + 1);
  hipLaunchKernelGGL(k_cll_heads, dim3(ge), dim3(256), 0, st, sorted, e, p.tol, lhead, xhead, qhead);
  prims::exclusive_scan<uint32_t>(lhead, exl, e, b.scan_tmp, st);
  prims::exclusive_scan<uint32_t>(xhead, exx, e, b.scan_tmp, st);
  prims::exclusive_scan<uint32_t>(qhead, exq, e, b.scan_tmp, st);
  uint32_t *lstart = b.lstart.as<uint32_t>((uint64_t) e + 1), *xstart = b.xstart.as<uint32_t>((uint64_t) e + 1);
  hipLaunchKernelGGL(runs::k_run_starts, dim3(ge), dim3(256), 0, st, exl, e, lstart, (uint32_t *) nullptr);
  hipLaunchKernelGGL(runs::k_run_starts, dim3(ge), dim3(256), 0, st, exx, e, xstart, (uint32_t *) nullptr);
  uint32_t counts[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(&counts[0], exl + e, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&counts[1], exx + e, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  const uint32_t n_loci = counts[0];  // (1 <= n_loci <= x <= e)
  s.loci = n_loci;
  s.exact = counts[1];
  const unsigned gl = cdiv(n_loci, 256);

  // the rows by (locus, read rank): the heads are the distinct reads of a locus
  const int rank_bits = bits_of(e);
  hipLaunchKernelGGL(k_cll_read_keys, dim3(ge), dim3(256), 0, st, sorted, exl, e, rank_bits, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, rank_bits + bits_of(n_loci), b.radix, st, &sk, &sv);
  uint32_t *exd = b.exd.as<uint32_t>((uint64_t) e + 1);
  hipLaunchKernelGGL(runs::k_key_heads, dim3(ge), dim3(256), 0, st, sk, e, 0, 1u, lhead, (uint32_t *) nullptr);
  prims::exclusive_scan<uint32_t>(lhead, exd, e, b.scan_tmp, st);

  // the rows, the partners and the mutual bit
  struct bk_clip_locus *rows = b.rows.as<struct bk_clip_locus>(n_loci);
  uint64_t *lkey = b.lkey.as<uint64_t>(n_loci);
  uint32_t *keep = b.keep.as<uint32_t>((uint64_t) n_loci + 1);
  uint32_t *partner = b.partner.as<uint32_t>(n_loci), *mutual = b.mutual.as<uint32_t>((uint64_t) n_loci + 1);
  hipLaunchKernelGGL(k_cll_loci, dim3(cdiv(n_loci, 4)), dim3(256), 0, st, sorted, lstart, xstart, exx, exq, exd, n_loci, p.min_reads, s.pos_bits, s.tid_bits, rows, lkey, keep);
  hipLaunchKernelGGL(k_cll_facing, dim3(cdiv(n_loci, 4)), dim3(256), 0, st, rows, lkey, n_loci, p.pair_dist, s.pos_bits, s.tid_bits, partner);
  hipLaunchKernelGGL(k_cll_mutual, dim3(gl), dim3(256), 0, st, partner, n_loci, mutual);

  // the claim: the voted breakpoints sorted by (tid, pos); equal keys keep the order of their rows
  uint32_t *claim = nullptr;
  s.breakpoints = 0;
  if (cl)
  {
    claim = b.claim.as<uint32_t>(n_loci);
    const uint32_t m = (uint32_t) (2 * ncl);
    s.breakpoints = m;
    uint64_t *bk = b.bkeys.as<uint64_t>((uint64_t) m + 1), *sbk = bk;
    uint32_t *bv = b.bvals.as<uint32_t>((uint64_t) m + 1), *sbv = bv;
    if (m)
    {
      hipLaunchKernelGGL(k_cll_bp_keys, dim3(cdiv(m, 256)), dim3(256), 0, st, cl, m, 1 << s.tid_bits, 1ull << (32 + s.tid_bits), bk, bv);
      prims::radix_sort_pairs(bk, bv, m, 0, 33 + s.tid_bits, b.radix, st, &sbk, &sbv);
    }
    hipLaunchKernelGGL(k_cll_claim, dim3(gl), dim3(256), 0, st, rows, n_loci, sbk, sbv, m, claim);
  }

  // those with enough reads
  uint32_t *exm = lhead;  // (e + 1 >= n_loci + 1 entries)
  prims::exclusive_scan<uint32_t>(mutual, exm, n_loci, b.scan_tmp, st);
  prims::exclusive_scan<uint32_t>(keep, keep, n_loci, b.scan_tmp, st);
  struct bk_clip_locus *out = b.out.as<struct bk_clip_locus>((uint64_t) n_loci + 1);
  hipLaunchKernelGGL(k_cll_out, dim3(gl), dim3(256), 0, st, rows, keep, partner, mutual, claim, n_loci, out);
  HIP_CHECK(hipMemcpyAsync(&counts[0], exm + n_loci, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&counts[1], keep + n_loci, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  s.mutual = counts[0];
  s.written = counts[1];
  *rows_out = out;
  *stats = s;
}
