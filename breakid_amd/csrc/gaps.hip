// Deletions and insertions from CIGAR gaps (bk_cigar_gaps).  The record pass is the hot one: one wavefront per tile
// of 256 records, four consecutive records a lane, cigar_off, flag and mapq (and, in the count pass, tid) read as vectors; a record
// whose flag and mapq pass and that has three or more operations is walked by its lane.  Pass one sums the events of a tile, a scan
// makes the sums offsets, pass two walks the records of the tiles that hold an event again and writes 32-byte event rows in record
// order.  Behind it: stable LSD stages of the radix sort by qhash (whose run heads rank the reads), len and (kind, tid, start); the
// heads of the loci; one stage by (locus, len); the heads of the calls, of the exact events and of the reads inside them; one stage by
// (call, read rank); one wavefront per call.  Integer arithmetic only, no atomic: every result word has one writer.
#include "gaps.h"
#include "runs.h"

using runs::bits_of;
using runs::NONE;

namespace
{
constexpr uint32_t OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_EQ = 7, OP_X = 8;  // BAM CIGAR operations
constexpr uint16_t FLAG_DROP = 0x4 | 0x100 | 0x200 | 0x400 | 0x800;

struct GapEvent
{
  uint64_t qhash;
  uint32_t start, len;
  uint32_t kt;     // kind << 31 | tid
  uint32_t sm;     // reverse strand << 8 | mapq
  uint32_t qrank;  // dense rank of qhash among the events
  uint32_t pad;
};
static_assert(sizeof(GapEvent) == 32, "event rows of gaps.hip");

// ---- the walk -----------------------------------------------------------------------------------------------------------------------
// The definition of include/breakid_hip.h for one eligible record with the CIGAR words [c0, c1): f(kind, start, len) for every event
// that is kept; returns the events beyond the contig's end.  Two loops over the words: the first sums the matched bases, so that the
// second knows what lies behind an operation.
template <class F> __device__ __forceinline__ uint32_t gap_walk(const uint32_t *__restrict__ cigar, uint32_t c0, uint32_t c1, int32_t pos, uint32_t tlen, const GapParams &p, F &&f)
{
  unsigned long long total = 0;
  for (uint32_t c = c0; c < c1; ++c)
  {
    const uint32_t w = cigar[c], op = w & 15u;
    if (op == OP_M || op == OP_EQ || op == OP_X) total += w >> 4;
  }
  if (total < 2ull * p.anchor) return 0;
  uint32_t beyond = 0;
  long long at = pos;
  unsigned long long m = 0;
  for (uint32_t c = c0; c < c1; ++c)
  {
    const uint32_t w = cigar[c], op = w & 15u, len = w >> 4;
    if ((op == OP_D || op == OP_I) && len >= p.min_len && m >= p.anchor && total - m >= p.anchor)
    {
      const long long right = op == OP_D ? at + (long long) len + 1 : at + 1;
      if (at < 0 || right > (long long) tlen)
        ++beyond;
      else
        f(op == OP_I ? 1u : 0u, (uint32_t) at, len);
    }
    if (op == OP_M || op == OP_EQ || op == OP_X)
    {
      at += len;
      m += len;
    }
    else if (op == OP_D || op == OP_N)
      at += len;
  }
  return beyond;
}

// what the lane's four records look like to both passes: flag and mapq pass (bit s of `pass`), and the CIGAR offsets
struct GapLane
{
  uint32_t c[5];
  uint32_t pass;
};

// Lane `lane` of tile t takes the records i0 = 256 t + 4 lane .. i0 + 3 and reads each column with one vector load (the fixed columns
// of every table form are 16-byte aligned and a tile starts at a multiple of 256 records); a lane whose four records are not all
// below n (the last tile only) reads them one by one, guarded.  cigar_off has n + 1 entries.
__device__ __forceinline__ GapLane gap_lane(const RecView &r, uint64_t i0, int mapq_min)
{
  GapLane o = {{0, 0, 0, 0, 0}, 0};
  uint16_t f[4] = {FLAG_DROP, FLAG_DROP, FLAG_DROP, FLAG_DROP};
  uint8_t q[4] = {0, 0, 0, 0};
  if (i0 + 4 <= r.n)
  {
    const ushort4 fv = *reinterpret_cast<const ushort4 *>(r.flag + i0);
    const uchar4 qv = *reinterpret_cast<const uchar4 *>(r.mapq + i0);
    const uint4 cv = *reinterpret_cast<const uint4 *>(r.cigar_off + i0);
    f[0] = fv.x; f[1] = fv.y; f[2] = fv.z; f[3] = fv.w;
    q[0] = qv.x; q[1] = qv.y; q[2] = qv.z; q[3] = qv.w;
    o.c[0] = cv.x; o.c[1] = cv.y; o.c[2] = cv.z; o.c[3] = cv.w;
    o.c[4] = r.cigar_off[i0 + 4];
  }
  else
    for (int s = 0; s < 4 && i0 + s < r.n; ++s)
    {
      f[s] = r.flag[i0 + s];
      q[s] = r.mapq[i0 + s];
      o.c[s] = r.cigar_off[i0 + s];
      o.c[s + 1] = r.cigar_off[i0 + s + 1];
    }
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (!(f[s] & FLAG_DROP) && (int) q[s] >= mapq_min) o.pass |= 1u << s;
  return o;
}

// a record can hold an anchored gap only with three or more operations; its words must lie inside the CIGAR array
__device__ __forceinline__ bool gap_walkable(uint32_t c0, uint32_t c1, uint64_t n_words) { return c1 > c0 && c1 - c0 >= 3u && c1 <= n_words; }

// Pass one.  tile_ev[t] = the events of tile t, tile_eb[t] = its eligible records | its events beyond a contig's end << 32.  tid is
// read for every record here (eligibility needs it and the table need not be sorted yet); pos only for a record that is walked.
__global__ __launch_bounds__(256) void k_gap_count(GapInput in, GapParams p, uint64_t n_tiles, uint32_t *__restrict__ tile_ev, unsigned long long *__restrict__ tile_eb)
{
  const uint64_t t = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const int lane = threadIdx.x & 63;
  const RecView &r = in.rec;
  const uint64_t i0 = (t << runs::TILE_SHIFT) + 4u * (uint32_t) lane;
  const GapLane l = gap_lane(r, i0, p.mapq_min);
  int32_t td[4] = {-1, -1, -1, -1};
  if (i0 + 4 <= r.n)
  {
    const int4 tv = *reinterpret_cast<const int4 *>(r.tid + i0);
    td[0] = tv.x; td[1] = tv.y; td[2] = tv.z; td[3] = tv.w;
  }
  else
    for (int s = 0; s < 4 && i0 + s < r.n; ++s) td[s] = r.tid[i0 + s];
  uint32_t ev = 0, elig = 0, beyond = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s)
  {
    if (!((l.pass >> s) & 1u) || td[s] < 0) continue;
    ++elig;
    if (!gap_walkable(l.c[s], l.c[s + 1], in.n_cigar_words)) continue;
    beyond += gap_walk(r.cigar, l.c[s], l.c[s + 1], r.pos[i0 + s], runs::tlen(in.tprefix, in.nt, td[s]), p, [&](uint32_t, uint32_t, uint32_t) { ++ev; });
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

// Pass two.  ex = the exclusive scan of tile_ev (n_tiles + 1 entries).  A tile without an event ends at once.  A lane counts the events
// of its records, a wave scan gives its offset inside the tile, and a second walk writes the rows: slot ex[t] + (the events of the
// lanes in front) + (its own so far), which is below ex[t + 1] <= ex[n_tiles] = the rows of `out`, because both passes walk the same words.
__global__ __launch_bounds__(256) void k_gap_emit(GapInput in, GapParams p, uint64_t n_tiles, const uint32_t *__restrict__ ex, GapEvent *__restrict__ out)
{
  const uint64_t t = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const uint32_t base = ex[t], end = ex[t + 1];
  if (base == end) return;
  const int lane = threadIdx.x & 63;
  const RecView &r = in.rec;
  const uint64_t i0 = (t << runs::TILE_SHIFT) + 4u * (uint32_t) lane;
  const GapLane l = gap_lane(r, i0, p.mapq_min);
  int32_t td[4] = {-1, -1, -1, -1};
  uint32_t mine = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s)
  {
    if (!((l.pass >> s) & 1u) || !gap_walkable(l.c[s], l.c[s + 1], in.n_cigar_words)) continue;
    td[s] = r.tid[i0 + s];  // (pass is 0 for a record at or beyond n)
    if (td[s] < 0) continue;
    (void) gap_walk(r.cigar, l.c[s], l.c[s + 1], r.pos[i0 + s], runs::tlen(in.tprefix, in.nt, td[s]), p, [&](uint32_t, uint32_t, uint32_t) { ++mine; });
  }
  uint32_t slot = base + prims::wave_inclusive_scan(mine) - mine;
  if (!mine) return;
#pragma unroll
  for (int s = 0; s < 4; ++s)
  {
    if (td[s] < 0) continue;
    const uint64_t i = i0 + s;
    GapEvent e;
    e.qhash = in.side ? in.side[i].qhash : in.qhash[i];
    e.sm = (((uint32_t) r.flag[i] >> 4) & 1u) << 8 | r.mapq[i];
    e.qrank = 0;
    e.pad = 0;
    const uint32_t tid = (uint32_t) td[s];
    (void) gap_walk(r.cigar, l.c[s], l.c[s + 1], r.pos[i], runs::tlen(in.tprefix, in.nt, td[s]), p, [&](uint32_t kind, uint32_t start, uint32_t len) {
      e.start = start;
      e.len = len;
      e.kt = (kind << 31) | tid;
      if (slot < end) out[slot] = e;
      ++slot;
    });
  }
}

// ---- the sort stages ----------------------------------------------------------------------------------------------------------------
// keys[i] = the stage's key of event perm[i] (perm == nullptr: the identity); vals[i] = that event.  perm may be vals itself.
__global__ __launch_bounds__(256) void k_gap_keys(const GapEvent *__restrict__ ev, const uint32_t *perm, uint32_t e, int mode, int start_bits, int tid_bits, uint64_t *__restrict__ keys,
                                                  uint32_t *vals)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  const uint32_t k = perm ? perm[i] : i;  // (k < e: perm is a permutation that the sort made of the identity)
  const GapEvent t = ev[k];
  const uint64_t group = ((uint64_t) (t.kt >> 31) << tid_bits) | (t.kt & 0x7FFFFFFFu);
  keys[i] = mode == 0 ? t.qhash : mode == 1 ? (uint64_t) t.len : (group << start_bits) | t.start;
  vals[i] = k;
}

// over the rows sorted by (kind, tid, start, len): 1 where a locus begins (also at i == 0)
__global__ __launch_bounds__(256) void k_gap_locus_heads(const GapEvent *__restrict__ sorted, uint32_t e, uint32_t tol, uint32_t *__restrict__ head)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  uint32_t h = 1;
  if (i)
  {
    const GapEvent a = sorted[i - 1], b = sorted[i];
    h = a.kt != b.kt || b.start - a.start > tol;  // (b.start >= a.start inside one kt)
  }
  head[i] = h;
}

// exl = the exclusive scan of the locus heads: the locus of row i is exl[i + 1] - 1
__global__ __launch_bounds__(256) void k_gap_locus_keys(const GapEvent *__restrict__ sorted, const uint32_t *__restrict__ exl, uint32_t e, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  keys[i] = ((uint64_t) (exl[i + 1] - 1u) << GAP_LEN_BITS) | sorted[i].len;
  vals[i] = i;
}

// over the rows sorted by (locus, len, start, read rank), keys = locus << 28 | len: the heads of the calls, of the exact events and of
// the reads inside an exact event; all 1 at i == 0
__global__ __launch_bounds__(256) void k_gap_call_heads(const GapEvent *__restrict__ bylen, const uint64_t *__restrict__ keys, uint32_t e, uint32_t tol, uint32_t *__restrict__ chead,
                                                        uint32_t *__restrict__ xhead, uint32_t *__restrict__ qhead)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  uint32_t c = 1, x = 1, q = 1;
  if (i)
  {
    const uint64_t ka = keys[i - 1], kb = keys[i];
    const GapEvent a = bylen[i - 1], b = bylen[i];
    c = (ka >> GAP_LEN_BITS) != (kb >> GAP_LEN_BITS) || b.len - a.len > tol;  // (b.len >= a.len inside one locus)
    x = c | (ka != kb) | (a.start != b.start);
    q = x | (a.qrank != b.qrank);
  }
  chead[i] = c;
  xhead[i] = x;
  qhead[i] = q;
}

// (call of the row) << rank_bits | read rank: equal keys are one read of one call
__global__ __launch_bounds__(256) void k_gap_read_keys(const GapEvent *__restrict__ bylen, const uint32_t *__restrict__ exc, uint32_t e, int rank_bits, uint64_t *__restrict__ keys,
                                                       uint32_t *__restrict__ vals)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e) return;
  keys[i] = ((uint64_t) (exc[i + 1] - 1u) << rank_bits) | bylen[i].qrank;
  vals[i] = i;
}

// ---- the calls ----------------------------------------------------------------------------------------------------------------------
// One wavefront per call c, four to a workgroup.  Its rows are [cstart[c], cstart[c + 1]) of the table sorted by (locus, len, start,
// read rank), and the same range of the list sorted by (call, read rank).  exx / exq / exd = the exclusive scans of the heads of the
// exact events, of the reads inside them, and of the reads inside the calls; xstart = the first row of every exact event.
__global__ __launch_bounds__(256) void k_gap_calls(const GapEvent *__restrict__ bylen, const uint32_t *__restrict__ cstart, const uint32_t *__restrict__ xstart,
                                                   const uint32_t *__restrict__ exx, const uint32_t *__restrict__ exq, const uint32_t *__restrict__ exd, uint32_t n_calls,
                                                   uint32_t min_reads, struct bk_cigar_gap *__restrict__ rows, uint32_t *__restrict__ keep)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_calls) return;
  const uint32_t a = cstart[c], b = cstart[c + 1];  // (a < b <= e)
  uint32_t n_rev = 0, lo_s = NONE, hi_s = 0, lo_l = NONE, hi_l = 0, top = 0;
  unsigned long long mq = 0;
  for (uint32_t i = a + lane; i < b; i += 64)
  {
    const GapEvent t = bylen[i];
    n_rev += t.sm >> 8;
    mq += t.sm & 255u;
    lo_s = t.start < lo_s ? t.start : lo_s;
    hi_s = t.start > hi_s ? t.start : hi_s;
    lo_l = t.len < lo_l ? t.len : lo_l;
    hi_l = t.len > hi_l ? t.len : hi_l;
    if (exx[i + 1] != exx[i])
    {
      const uint32_t reads = exq[xstart[exx[i] + 1]] - exq[i];  // (exx[i] is the exact event that begins at row i; exx[i] + 1 <= x)
      top = reads > top ? reads : top;
    }
  }
  n_rev = wave_sum(n_rev);
  mq = wave_sum(mq);
  lo_s = wave_min(lo_s);
  hi_s = wave_max(hi_s);
  lo_l = wave_min(lo_l);
  hi_l = wave_max(hi_l);
  top = wave_max(top);
  // the representative: among the exact events with `top` reads the smallest (start, len)
  unsigned long long rep = ~0ull;
  for (uint32_t i = a + lane; i < b; i += 64)
    if (exx[i + 1] != exx[i] && exq[xstart[exx[i] + 1]] - exq[i] == top)
    {
      const unsigned long long k = ((unsigned long long) bylen[i].start << 32) | bylen[i].len;
      rep = k < rep ? k : rep;
    }
  rep = wave_min(rep);
  if (lane) return;
  struct bk_cigar_gap r;
  const uint32_t kt = bylen[a].kt;  // (one kind and one contig in a call)
  r.tid = (int32_t) (kt & 0x7FFFFFFFu);
  r.start = (uint32_t) (rep >> 32);
  r.len = (uint32_t) rep;
  r.kind = kt >> 31;
  r.n_reads = exd[b] - exd[a];
  r.n_rows = b - a;
  r.n_exact = exx[b] - exx[a];
  r.top_reads = top;
  r.lo_start = lo_s;
  r.hi_start = hi_s;
  r.lo_len = lo_l;
  r.hi_len = hi_l;
  r.n_fwd = b - a - n_rev;
  r.n_rev = n_rev;
  r.mapq_sum = mq;
  rows[c] = r;
  keep[c] = r.n_reads >= min_reads;
}

}  // namespace

// include/breakid_hip.h states both models
uint64_t GapStats::touched_records() const
{
  const uint64_t tiles = runs::tiles_of(n);
  return n * 11ull + tiles * 56ull + std::min(events, tiles) * (runs::TILE * 7ull) + events * 48ull;
}

uint64_t GapStats::touched_calls() const
{
  const uint64_t p1 = 8 + (GAP_LEN_BITS + 7) / 8 + ((uint64_t) start_bits + tid_bits + 1 + 7) / 8;
  const uint64_t p2 = ((uint64_t) bits_of(loci) + GAP_LEN_BITS + 7) / 8, p3 = ((uint64_t) bits_of(calls) + bits_of(events) + 7) / 8;
  return events * (36ull * (p1 + p2 + p3) + 400ull) + calls * 144ull + written * 128ull;
}

void gap_events(const GapInput &in, const GapParams &p, GapBufs &b, hipStream_t st, GapStats *stats)
{
  GapStats s;
  s.n = in.rec.n;
  s.start_bits = bits_of(in.max_len);
  s.tid_bits = in.nt > 1 ? bits_of((uint64_t) in.nt - 1) : 0;
  *stats = s;
  runs::record_pass(
      in.rec.n, b, st, "bk_cigar_gaps: more than 2^30 events", *stats,
      [&](uint64_t nt, uint32_t *tile_ev, unsigned long long *tile_eb) { hipLaunchKernelGGL(k_gap_count, dim3(cdiv(nt, 4)), dim3(256), 0, st, in, p, nt, tile_ev, tile_eb); },
      [&](uint64_t nt, const uint32_t *ex) { hipLaunchKernelGGL(k_gap_emit, dim3(cdiv(nt, 4)), dim3(256), 0, st, in, p, nt, ex, b.ev.as<GapEvent>(stats->events)); });
}

void gap_calls(const GapParams &p, GapBufs &b, hipStream_t st, struct bk_cigar_gap **rows_out, GapStats *stats)
{
  static_assert(sizeof(struct bk_cigar_gap) == 64, "bk_cigar_gap must be 64 bytes");
  GapStats s = *stats;
  *rows_out = b.out.as<struct bk_cigar_gap>(1);
  if (s.events == 0) return;
  const uint32_t e = (uint32_t) s.events;
  const unsigned ge = cdiv(e, 256);
  GapEvent *ev = b.ev.get<GapEvent>();

  // stable LSD stages, least significant first: qhash (and its dense rank), len, (kind, tid, start)
  uint64_t *keys = b.keys.as<uint64_t>(e), *sk;
  uint32_t *vals = b.vals.as<uint32_t>(e), *sv;
  uint32_t *head = b.head.as<uint32_t>((uint64_t) e + 1), *qhead = b.qhead.as<uint32_t>((uint64_t) e + 1);
  hipLaunchKernelGGL(k_gap_keys, dim3(ge), dim3(256), 0, st, ev, (const uint32_t *) nullptr, e, 0, s.start_bits, s.tid_bits, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, 64, b.radix, st, &sk, &sv);
  hipLaunchKernelGGL(runs::k_key_heads, dim3(ge), dim3(256), 0, st, sk, e, 0, 0u, head, (uint32_t *) nullptr);
  prims::exclusive_scan<uint32_t>(head, head, e, b.scan_tmp, st);
  hipLaunchKernelGGL(runs::k_dense_rank<GapEvent>, dim3(ge), dim3(256), 0, st, sv, head, e, ev);
  hipLaunchKernelGGL(k_gap_keys, dim3(ge), dim3(256), 0, st, ev, sv, e, 1, s.start_bits, s.tid_bits, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, GAP_LEN_BITS, b.radix, st, &sk, &sv);
  hipLaunchKernelGGL(k_gap_keys, dim3(ge), dim3(256), 0, st, ev, sv, e, 2, s.start_bits, s.tid_bits, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, s.start_bits + s.tid_bits + 1, b.radix, st, &sk, &sv);
  GapEvent *sorted = b.sorted.as<GapEvent>(e);
  hipLaunchKernelGGL(runs::k_gather_rows<GapEvent>, dim3(ge), dim3(256), 0, st, ev, sv, e, sorted);

  // the loci, and the stage by (locus, len)
  uint32_t *exl = b.ex.as<uint32_t>((uint64_t) e + 1);
  hipLaunchKernelGGL(k_gap_locus_heads, dim3(ge), dim3(256), 0, st, sorted, e, p.tol, head);
  prims::exclusive_scan<uint32_t>(head, exl, e, b.scan_tmp, st);
  const uint32_t n_loci = runs::read_u32(exl + e, st);  // (1 <= n_loci <= e)
  s.loci = n_loci;
  hipLaunchKernelGGL(k_gap_locus_keys, dim3(ge), dim3(256), 0, st, sorted, exl, e, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, GAP_LEN_BITS + bits_of(n_loci), b.radix, st, &sk, &sv);
  GapEvent *bylen = b.bylen.as<GapEvent>(e);
  hipLaunchKernelGGL(runs::k_gather_rows<GapEvent>, dim3(ge), dim3(256), 0, st, sorted, sv, e, bylen);

  // the calls, the exact events and their reads
  uint32_t *exc = exl, *exx = b.exx.as<uint32_t>((uint64_t) e + 1), *exq = b.exq.as<uint32_t>((uint64_t) e + 1);
  uint32_t *xhead = exx;
  hipLaunchKernelGGL(k_gap_call_heads, dim3(ge), dim3(256), 0, st, bylen, sk, e, p.tol, head, xhead, qhead);
  prims::exclusive_scan<uint32_t>(head, exc, e, b.scan_tmp, st);
  prims::exclusive_scan<uint32_t>(xhead, exx, e, b.scan_tmp, st);
  prims::exclusive_scan<uint32_t>(qhead, exq, e, b.scan_tmp, st);
  uint32_t *cstart = b.cstart.as<uint32_t>((uint64_t) e + 1), *xstart = b.xstart.as<uint32_t>((uint64_t) e + 1);
  hipLaunchKernelGGL(runs::k_run_starts, dim3(ge), dim3(256), 0, st, exc, e, cstart, (uint32_t *) nullptr);
  hipLaunchKernelGGL(runs::k_run_starts, dim3(ge), dim3(256), 0, st, exx, e, xstart, (uint32_t *) nullptr);
  uint32_t counts[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(&counts[0], exc + e, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&counts[1], exx + e, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  const uint32_t n_calls = counts[0];  // (1 <= n_calls <= x <= e)
  s.calls = n_calls;
  s.exact = counts[1];

  // the rows by (call, read rank): the heads are the distinct reads of a call
  const int rank_bits = bits_of(e);
  hipLaunchKernelGGL(k_gap_read_keys, dim3(ge), dim3(256), 0, st, bylen, exc, e, rank_bits, keys, vals);
  prims::radix_sort_pairs(keys, vals, e, 0, rank_bits + bits_of(n_calls), b.radix, st, &sk, &sv);
  uint32_t *exd = b.exd.as<uint32_t>((uint64_t) e + 1);
  hipLaunchKernelGGL(runs::k_key_heads, dim3(ge), dim3(256), 0, st, sk, e, 0, 1u, head, (uint32_t *) nullptr);
  prims::exclusive_scan<uint32_t>(head, exd, e, b.scan_tmp, st);

  // the rows, and those with enough reads
  struct bk_cigar_gap *rows = b.rows.as<struct bk_cigar_gap>(n_calls);
  uint32_t *keep = b.keep.as<uint32_t>((uint64_t) n_calls + 1);
  hipLaunchKernelGGL(k_gap_calls, dim3(cdiv(n_calls, 4)), dim3(256), 0, st, bylen, cstart, xstart, exx, exq, exd, n_calls, p.min_reads, rows, keep);
  prims::exclusive_scan<uint32_t>(keep, keep, n_calls, b.scan_tmp, st);
  struct bk_cigar_gap *out = b.out.as<struct bk_cigar_gap>((uint64_t) n_calls + 1);
  hipLaunchKernelGGL(runs::k_keep_out<struct bk_cigar_gap>, dim3(cdiv(n_calls, 256)), dim3(256), 0, st, rows, keep, n_calls, out);
  s.written = runs::read_u32(keep + n_calls, st);
  *rows_out = out;
  *stats = s;
}
