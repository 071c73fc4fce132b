// The reads behind every call (bk_evidence): what bk_junctions counts, listed.  Count, scan, emit: the counts are
// those of junctions() itself (junction.hip); an exclusive scan over the calls in BK_STAGE_CLUSTERS order gives every call its
// range of rows; the rows are then written at ranks that depend on the data alone, so two runs give the same bytes:
//   pair rows   the clustered list is sorted (stable, prims.h) by the call a list entry belongs to, so the entries of a call are
//               neighbours in ascending list position = ascending BK_STAGE_CLUSTERED row (members of an AHC cluster need not be
//               neighbours in the list itself); entry i of the sorted list is row i - pair_off[call] of its call
//   split rows  one wavefront per voted cluster walks the tuple ranges of tuple_match.h in ascending tuple index, 64 at a time; a
//               matching tuple's rank is the matches before it: a running count plus a ballot prefix
// No atomic hands out a slot.  A row is three 16-byte stores.
#include "evidence.h"
#include "tuple_match.h"
#include <cstddef>

namespace
{
static_assert(sizeof(struct bk_evidence) == 48 && offsetof(struct bk_evidence, qcheck) == 16 && offsetof(struct bk_evidence, tid1) == 24 &&
                  offsetof(struct bk_evidence, flag1) == 40 && offsetof(struct bk_evidence, kind) == 46 && offsetof(struct bk_evidence, sides) == 47,
              "bk_evidence must be 48 bytes");

__device__ __forceinline__ void store_row(struct bk_evidence *__restrict__ o, const struct bk_evidence &v)
{
  uint4 t[3];
  __builtin_memcpy(t, &v, sizeof v);
  uint4 *o4 = reinterpret_cast<uint4 *>(o);  // (rows start 16-byte aligned: 48-byte rows in a hipMalloc'ed array)
  o4[0] = t[0];
  o4[1] = t[1];
  o4[2] = t[2];
}

// Row c of the device cluster table is call c (BK_STAGE_CLUSTERS order: bp.hip, cluster_summary), so the counts of junctions() are
// the per-call counts as they stand: the rows of a call, and how many of them are pair rows.
__global__ __launch_bounds__(256) void k_ev_counts(const struct bk_junction *__restrict__ res, uint32_t ncl, uint64_t *__restrict__ cnt, uint64_t *__restrict__ npair)
{
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncl) return;
  const struct bk_junction j = res[c];
  const uint64_t np = (uint64_t) j.pairs[0] + j.pairs[1] + j.pairs[2] + j.pairs[3];
  const uint64_t ns = (uint64_t) j.splits[0] + j.splits[1] + j.splits[2] + j.splits[3];
  cnt[c] = np + ns;
  npair[c] = np;
}

// sort key of a list entry: the row of its cluster, ncl for an entry whose cluster has no row (k_junction_pairs)
__global__ __launch_bounds__(256) void k_ev_pair_keys(JunctionPairs in, uint32_t ncl, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
  const uint64_t p = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= in.n) return;
  const uint32_t s = in.slotbase[in.gof[p]] + in.cl[p];
  uint32_t key = ncl;
  if (s < in.slotbase[in.ng] && in.keep[s])
  {
    const uint32_t row = in.off[s];
    if (row < ncl) key = row;
  }
  keys[p] = key;
  vals[p] = (uint32_t) p;
}

__global__ __launch_bounds__(256) void k_ev_emit_pairs(JunctionPairs in, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t ncl,
                                                       const uint64_t *__restrict__ call_off, const uint64_t *__restrict__ pair_off, EvidenceRecs recs,
                                                       struct bk_evidence *__restrict__ rows, uint64_t n_rows, EvidenceStat *__restrict__ stat, uint64_t *__restrict__ kw)
{
  const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= in.n) return;
  const uint64_t c = keys[i];
  if (c >= ncl) return;
  const uint64_t p0 = pair_off[c], p1 = pair_off[c + 1];
  const uint64_t dest = call_off[c] + (i - p0);
  const uint32_t p = vals[i];
  if (i < p0 || i >= p1 || dest >= call_off[c + 1] || dest >= n_rows || p >= in.n)
  {
    stat->bad = 1u;
    return;
  }
  const bk_pair pr = in.pairs[in.idx[p]];
  if (kw)  // (the fragment key of the row: evidence.h)
  {
    kw[dest] = (uint64_t) pr.p1_pos << 32 | pr.p2_pos;
    kw[n_rows + dest] = 2u * (pr.p1_rev ? 1u : 0u) + (pr.p2_rev ? 1u : 0u);
    kw[2 * n_rows + dest] = 0;
    kw[3 * n_rows + dest] = c << 1;
  }
  if (!rows) return;
  struct bk_evidence v;
  v.rec = pr.rec;
  v.qhash = 0;
  v.qcheck = 0;
  if (pr.rec < recs.n)
  {
    if (recs.side)
    {
      v.qhash = recs.side[pr.rec].qhash;
      v.qcheck = recs.side[pr.rec].qcheck;
    }
    else
    {
      v.qhash = recs.qhash[pr.rec];
      v.qcheck = recs.qcheck ? recs.qcheck[pr.rec] : 0u;
    }
  }
  else
    stat->bad = 1u;
  v.call = (uint32_t) c;
  v.tid1 = pr.p1_tid;
  v.pos1 = pr.p1_pos;
  v.tid2 = pr.p2_tid;
  v.pos2 = pr.p2_pos;
  v.flag1 = pr.p1_flag;
  v.flag2 = pr.p2_flag;
  v.mapq1 = pr.p1_mapq;
  v.mapq2 = pr.p2_mapq;
  v.kind = BK_EV_PAIR;
  v.sides = (uint8_t) (2u * (pr.p1_rev ? 1u : 0u) + (pr.p2_rev ? 1u : 0u));
  store_row(rows + dest, v);
}

// One wave per cluster.  The up to four tuple ranges are put in ascending order and walked as their union, so the
// matches come in ascending BK_STAGE_SPLITS row; sides as in k_junction_sr.
__global__ __launch_bounds__(256) void k_ev_emit_splits(TupleTable tt, const bk_cluster *__restrict__ cl, uint32_t ncl, const uint64_t *__restrict__ call_off,
                                                        const uint64_t *__restrict__ pair_off, EvidenceRecs recs, struct bk_evidence *__restrict__ rows, uint64_t n_rows,
                                                        EvidenceStat *__restrict__ stat, uint64_t *__restrict__ kw)
{
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= ncl) return;
  const bk_cluster k = cl[c];
  if (!(k.flags & 2u)) return;
  const uint64_t base = call_off[c] + (pair_off[c + 1] - pair_off[c]), limit = call_off[c + 1];
  const TupleRanges r = tuple_ranges(tt, k);
  uint64_t lo[4], hi[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
  {
    const bool some = r.hi[q] > r.lo[q];
    lo[q] = some ? r.lo[q] : ~0ull;  // (empty ranges go last)
    hi[q] = some ? r.hi[q] : ~0ull;
  }
  auto order = [&](int a, int b) {
    if (lo[b] < lo[a])
    {
      const uint64_t tl = lo[a], th = hi[a];
      lo[a] = lo[b];
      hi[a] = hi[b];
      lo[b] = tl;
      hi[b] = th;
    }
  };
  order(0, 1);
  order(2, 3);
  order(0, 2);
  order(1, 3);
  order(1, 2);
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t done = 0, n_out = 0;
  uint32_t visited = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
  {
    if (lo[q] == ~0ull) continue;
    const uint64_t a = lo[q] > done ? lo[q] : done, e = hi[q];
    for (uint64_t t0 = a; t0 < e; t0 += 64)  // (the same trip count on every lane)
    {
      const uint64_t t = t0 + lane;
      int side = 0;
      bk_split s;
      if (t < e)
      {
        s = tt.sp[t];
        side = tuple_side(s, r, k);
      }
      const uint64_t m = __ballot(side != 0);
      if (side)
      {
        const uint64_t dest = base + n_out + (uint64_t) __popcll(m & below);
        if (dest >= limit || dest >= n_rows)
          stat->bad = 1u;
        else
        {
          const bool swapped = side == 2;
          if (kw)  // (the fragment key of the row: evidence.h)
          {
            int32_t mt = 0, mp = 0;
            if (s.rec < recs.n)
            {
              mt = recs.side ? recs.side[s.rec].mtid : recs.mtid[s.rec];
              mp = recs.side ? recs.side[s.rec].mpos : recs.mpos[s.rec];
            }
            else
              stat->bad = 1u;
            const uint64_t prim = (uint64_t) s.prim_start << 32 | s.prim_end, sec = (uint64_t) s.sec_start << 32 | s.sec_end;
            kw[dest] = swapped ? sec : prim;
            kw[n_rows + dest] = swapped ? prim : sec;
            kw[2 * n_rows + dest] = (uint64_t) (uint32_t) mt << 32 | (uint32_t) mp;
            kw[3 * n_rows + dest] = (uint64_t) c << 1 | 1u;
          }
          if (rows)
          {
            struct bk_evidence v;
            v.rec = s.rec;
            v.qhash = s.qhash;
            v.qcheck = s.qcheck;
            v.call = c;
            v.tid1 = k.p1_tid;
            v.pos1 = swapped ? s.sec_bp : s.prim_bp;
            v.tid2 = k.p2_tid;
            v.pos2 = swapped ? s.prim_bp : s.sec_bp;
            v.flag1 = (uint16_t) (s.flags & 0xFFFFu);
            v.flag2 = swapped ? 1 : 0;
            v.mapq1 = 0;
            if (s.rec < recs.n)
              v.mapq1 = recs.mapq[s.rec];
            else
              stat->bad = 1u;
            v.mapq2 = 0;
            v.kind = BK_EV_SPLIT;
            v.sides = (uint8_t) split_sides(s, swapped);
            store_row(rows + dest, v);
          }
        }
      }
      n_out += (uint64_t) __popcll(m);
    }
    if (e > a) visited += (uint32_t) (e - a);
    if (e > done) done = e;
  }
  if (lane == 0)
  {
    if (base + n_out != limit) stat->bad = 1u;  // the listing and the count of k_junction_sr disagree
    if (visited) atomicAdd(&stat->visited, (unsigned long long) visited);  // (a statistic for the byte model, not a slot)
  }
}
}  // namespace

void evidence(const JunctionPairs &p, const TupleTable &tt, const bk_cluster *cl, uint64_t ncl, const EvidenceRecs &recs, EvidenceBufs &b, hipStream_t st,
              struct bk_evidence **rows_out, uint64_t **call_off_out, EvidenceStat **stat_out, EvidenceKeys *keys, bool pairs_only)
{
  uint64_t *call_off = b.call_off.as<uint64_t>(ncl + 1);
  EvidenceStat *stat = b.stat.as<EvidenceStat>(1);
  *call_off_out = call_off;
  *stat_out = stat;
  *rows_out = b.rows.as<struct bk_evidence>(1);
  if (keys)
  {
    keys->d = nullptr;
    keys->n = 0;
  }
  HIP_CHECK(hipMemsetAsync(stat, 0, sizeof(EvidenceStat), st));
  if (ncl == 0)
  {
    HIP_CHECK(hipMemsetAsync(call_off, 0, sizeof(uint64_t), st));
    return;
  }
  if (ncl > 0x7FFFFFFFull) throw bk_error(BK_ERR_LIMIT, "too many clusters");
  if (p.n > 0xFFFFFFF0ull) throw bk_error(BK_ERR_LIMIT, "too many clustered pairs");
  const uint32_t n32 = (uint32_t) ncl;
  struct bk_junction *res;
  uint32_t *vis;
  junctions(p, tt, cl, ncl, b.jn, st, &res, &vis, pairs_only);
  // every call's counts and the two scans
  uint64_t *cnt = b.cnt.as<uint64_t>(ncl + 1), *npair = b.npair.as<uint64_t>(ncl + 1), *pair_off = b.pair_off.as<uint64_t>(ncl + 1);
  hipLaunchKernelGGL(k_ev_counts, dim3(cdiv(ncl, 256)), dim3(256), 0, st, res, n32, cnt, npair);
  prims::exclusive_scan<uint64_t>(cnt, call_off, ncl, b.scan_tmp, st);
  prims::exclusive_scan<uint64_t>(npair, pair_off, ncl, b.scan_tmp, st);
  if (pairs_only)  // the pair rows alone, packed: a call's range of rows is its range of sorted list entries
  {
    call_off = pair_off;
    *call_off_out = pair_off;
  }
  uint64_t total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, call_off + ncl, 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));  // the row count sizes the output
  const bool keys_only = keys && keys->keys_only;
  struct bk_evidence *rows = keys_only ? nullptr : b.rows.as<struct bk_evidence>(total + 1);
  if (!keys_only) *rows_out = rows;
  if (total == 0) return;
  uint64_t *kw = nullptr;
  if (keys)
  {
    kw = keys->d = keys->w.as<uint64_t>(4 * total);
    keys->n = total;
  }
  if (p.n)
  {
    uint64_t *keys = b.keys.as<uint64_t>(p.n);
    uint32_t *vals = b.vals.as<uint32_t>(p.n);
    hipLaunchKernelGGL(k_ev_pair_keys, dim3(cdiv(p.n, 256)), dim3(256), 0, st, p, n32, keys, vals);
    int bits = 1;
    while ((ncl >> bits) != 0) ++bits;  // keys are 0 .. ncl
    prims::radix_sort_pairs(keys, vals, p.n, 0, bits, b.radix, st, &keys, &vals);
    hipLaunchKernelGGL(k_ev_emit_pairs, dim3(cdiv(p.n, 256)), dim3(256), 0, st, p, keys, vals, n32, call_off, pair_off, recs, rows, total, stat, kw);
  }
  if (!pairs_only) hipLaunchKernelGGL(k_ev_emit_splits, dim3(cdiv(ncl, 4)), dim3(256), 0, st, tt, cl, n32, call_off, pair_off, recs, rows, total, stat, kw);
}
