// The unique fragments behind every call (bk_unique_support): bk_evidence's rows, grouped by fragment key.
// evidence() lists the rows and writes, beside each, its key as four 64-bit words (evidence.h); here the row indices are sorted by
// those words and read back per call:
//   differ   OR and AND of every key word over all rows; a digit in which OR == AND orders nothing and is not sorted
//   sort     stable LSD radix passes (the kernels of prims.h) over the three key words and then over call << 1 | kind, the row
//            index as the value.  That last word ascends with the row index, so the sorted positions of a call's pair rows are the
//            positions of its pair rows, likewise its split rows; inside such a range equal keys are neighbours, and because the
//            sort is stable and starts from row order the first of a run is the fragment's smallest row index
//   runs     one wavefront per call walks its two ranges UNIQUE_TILE sorted rows at a time: a row is a head when any key word
//            differs from the row before it (the full key: no hash stands in for it); a max-scan of the head lanes gives every row its
//            head, the head of a run that began in an earlier step is carried in a register; heads are counted, the longest run kept
// Nothing hands out a slot: every write goes to an index the data alone decides, so two runs give the same bytes.
#include "unique.h"
#include "wave.h"
#include <cstddef>

namespace
{
static_assert(sizeof(struct bk_unique_support) == 16 && offsetof(struct bk_unique_support, top_pairs) == 4 && offsetof(struct bk_unique_support, uniq_splits) == 8 &&
                  offsetof(struct bk_unique_support, top_splits) == 12,
              "bk_unique_support must be 16 bytes");
static_assert(UNIQUE_TILE == BK_WAVE, "k_uq_runs steps one wavefront at a time");

constexpr int KEY_WORDS = 4;

// d[j] |= word j of every row, d[KEY_WORDS + j] &= it (set to 0 and ~0 before); OR and AND commute: the result does not depend on who comes
// first.  A grid of at most DIFFER_BLOCKS workgroups strides over the rows and folds its waves in LDS, so the global atomics number
// 2 * KEY_WORDS per workgroup: one per wave of a grid over all rows took 19.8 of the stage's 27 ms at 14 M rows, all on one cache line.
constexpr unsigned DIFFER_BLOCKS = 1024;
__global__ __launch_bounds__(256) void k_uq_differ(const uint64_t *__restrict__ kw, uint64_t n, unsigned long long *__restrict__ d)
{
  __shared__ unsigned long long sh[2 * KEY_WORDS];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 2 * KEY_WORDS) sh[threadIdx.x] = threadIdx.x < KEY_WORDS ? 0ull : ~0ull;
  __syncthreads();
  uint64_t o[KEY_WORDS], a[KEY_WORDS];
#pragma unroll
  for (int j = 0; j < KEY_WORDS; ++j)
  {
    o[j] = 0ull;
    a[j] = ~0ull;
  }
  const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride)
#pragma unroll
    for (int j = 0; j < KEY_WORDS; ++j)
    {
      const uint64_t v = kw[(uint64_t) j * n + r];
      o[j] |= v;
      a[j] &= v;
    }
#pragma unroll
  for (int j = 0; j < KEY_WORDS; ++j)
  {
    const uint64_t wo = wave_or(o[j]), wa = ~wave_or(~a[j]);
    if (lane == 0)
    {
      atomicOr(&sh[j], (unsigned long long) wo);
      atomicAnd(&sh[KEY_WORDS + j], (unsigned long long) wa);
    }
  }
  __syncthreads();
  if (threadIdx.x < KEY_WORDS) atomicOr(&d[threadIdx.x], sh[threadIdx.x]);
  else if (threadIdx.x < 2 * KEY_WORDS) atomicAnd(&d[threadIdx.x], sh[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_uq_iota(uint32_t *__restrict__ vals, uint64_t n)
{
  const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) vals[i] = (uint32_t) i;
}

// the next key word of the rows in their current order
__global__ __launch_bounds__(256) void k_uq_gather(const uint64_t *__restrict__ col, const uint32_t *__restrict__ vals, uint64_t *__restrict__ keys, uint64_t n,
                                                   EvidenceStat *__restrict__ stat)
{
  const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = vals[i];
  if (r >= n)
  {
    stat->bad = 1u;
    return;
  }
  keys[i] = col[r];
}

// One wave per call; perm = the row indices in sorted order.
__global__ __launch_bounds__(256) void k_uq_runs(const uint32_t *__restrict__ perm, const uint64_t *__restrict__ kw, uint64_t n, const uint64_t *__restrict__ call_off,
                                                 const uint64_t *__restrict__ pair_off, uint32_t ncl, struct bk_unique_support *__restrict__ res, uint64_t *__restrict__ first,
                                                 EvidenceStat *__restrict__ stat)
{
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= ncl) return;
  uint64_t b0 = call_off[c], b2 = call_off[c + 1], b1 = b0 + (pair_off[c + 1] - pair_off[c]);
  if (b0 > b1 || b1 > b2 || b2 > n)
  {
    if (lane == 0) stat->bad = 1u;
    b0 = b1 = b2 = 0;
  }
  uint32_t out[4];
#pragma unroll
  for (int kind = 0; kind < 2; ++kind)
  {
    const uint64_t lo = kind ? b1 : b0, hi = kind ? b2 : b1;
    const uint64_t seg = (uint64_t) c << 1 | (uint64_t) kind;
    uint64_t carry_pos = lo;
    uint32_t carry_row = 0, uniq = 0, top = 0;
    for (uint64_t t0 = lo; t0 < hi; t0 += UNIQUE_TILE)  // (the same trip count on every lane)
    {
      const uint64_t i = t0 + lane;
      const bool active = i < hi;
      uint32_t row = 0;
      bool head = false;
      if (active)
      {
        row = perm[i];
        uint32_t prev = i > lo ? perm[i - 1] : row;
        if (row >= n || prev >= n)
        {
          stat->bad = 1u;
          row = prev = 0;
        }
        if (kw[3 * n + row] != seg) stat->bad = 1u;  // a row sorted outside the range of its call
        head = i == lo || kw[row] != kw[prev] || kw[n + row] != kw[n + prev] || kw[2 * n + row] != kw[2 * n + prev];
      }
      uint32_t hp = head ? (uint32_t) lane + 1u : 0u;  // lane + 1 of the last head at or before this lane, 0: none in this step
#pragma unroll
      for (int d = 1; d < 64; d <<= 1)
      {
        const uint32_t o = (uint32_t) __shfl_up((int) hp, d, 64);
        if (lane >= d && o > hp) hp = o;
      }
      uint32_t hrow = (uint32_t) __shfl((int) row, hp ? (int) hp - 1 : 0, 64);
      if (!hp) hrow = carry_row;
      const uint64_t hpos = hp ? t0 + hp - 1u : carry_pos;
      if (active)
      {
        if (first) first[row] = hrow;
        const uint32_t len = (uint32_t) (i - hpos) + 1u;
        if (len > top) top = len;
      }
      uniq += (uint32_t) __popcll(__ballot(head));
      const uint32_t hp_last = (uint32_t) __shfl((int) hp, 63, 64);
      if (hp_last)  // (the same on every lane)
      {
        carry_pos = t0 + hp_last - 1u;
        carry_row = (uint32_t) __shfl((int) row, (int) hp_last - 1, 64);
      }
    }
    for (int d = 32; d; d >>= 1)
    {
      const uint32_t o = (uint32_t) __shfl_xor((int) top, d, 64);
      if (o > top) top = o;
    }
    out[2 * kind] = uniq;
    out[2 * kind + 1] = top;
  }
  if (lane == 0)
  {
    struct bk_unique_support v;
    v.uniq_pairs = out[0];
    v.top_pairs = out[1];
    v.uniq_splits = out[2];
    v.top_splits = out[3];
    res[c] = v;
  }
}
}  // namespace

void unique_support(const JunctionPairs &p, const TupleTable &tt, const bk_cluster *cl, uint64_t ncl, const EvidenceRecs &recs, bool listing, UniqueBufs &b, hipStream_t st,
                    struct bk_unique_support **res_out, uint64_t **first_out, EvidenceStat **ev_stat_out, UniqueStat *stat)
{
  *stat = UniqueStat{};
  struct bk_evidence *rows;
  uint64_t *call_off;
  b.keys.keys_only = true;
  evidence(p, tt, cl, ncl, recs, b.ev, st, &rows, &call_off, ev_stat_out, &b.keys);
  struct bk_unique_support *res = b.res.as<struct bk_unique_support>(ncl + 1);
  const uint64_t n = b.keys.n;
  uint64_t *first = b.first.as<uint64_t>(n + 1);
  *res_out = res;
  *first_out = first;
  stat->n_rows = n;
  if (ncl == 0) return;
  if (n == 0)
  {
    HIP_CHECK(hipMemsetAsync(res, 0, ncl * sizeof(struct bk_unique_support), st));
    return;
  }
  if (n > 0xFFFFFFF0ull) throw bk_error(BK_ERR_LIMIT, "too many evidence rows");
  const uint64_t *kw = b.keys.d;
  const unsigned grid = cdiv(n, 256);
  // the digits in which two rows differ
  unsigned long long *d_differ = b.differ.as<unsigned long long>(2 * KEY_WORDS);
  HIP_CHECK(hipMemsetAsync(d_differ, 0, KEY_WORDS * 8, st));
  HIP_CHECK(hipMemsetAsync(d_differ + KEY_WORDS, 0xFF, KEY_WORDS * 8, st));
  hipLaunchKernelGGL(k_uq_differ, dim3(grid < DIFFER_BLOCKS ? grid : DIFFER_BLOCKS), dim3(256), 0, st, kw, n, d_differ);
  unsigned long long h[2 * KEY_WORDS];
  HIP_CHECK(hipMemcpyAsync(h, d_differ, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));  // which passes run is decided here
  // the sort: two sides that swap roles after every pass
  uint64_t *ka = b.key_a.as<uint64_t>(n), *kb = b.key_b.as<uint64_t>(n);
  uint32_t *va = b.val_a.as<uint32_t>(n), *vb = b.val_b.as<uint32_t>(n);
  const uint32_t nb = cdiv(n, prims::RS_TILE);
  uint32_t *hist = b.hist.as<uint32_t>((uint64_t) 256 * nb + 1);
  hipLaunchKernelGGL(k_uq_iota, dim3(grid), dim3(256), 0, st, va, n);
  for (int j = 0; j < KEY_WORDS; ++j)
  {
    const uint64_t differ = h[j] ^ h[KEY_WORDS + j];
    if (!differ) continue;
    hipLaunchKernelGGL(k_uq_gather, dim3(grid), dim3(256), 0, st, kw + (uint64_t) j * n, va, ka, n, *ev_stat_out);
    ++stat->gathers;
    for (int shift = 0; shift < 64; shift += 8)
    {
      if (!((differ >> shift) & 255u)) continue;  // (whole digits: the mask of a pass is 255)
      hipLaunchKernelGGL(prims::k_radix_hist, dim3(nb), dim3(prims::BLOCK), 0, st, ka, hist, n, shift, 255u, nb);
      prims::exclusive_scan<uint32_t>(hist, hist, (uint64_t) 256 * nb, b.scan_tmp, st);
      hipLaunchKernelGGL(prims::k_radix_scatter, dim3(nb), dim3(prims::BLOCK), 0, st, ka, va, kb, vb, hist, n, shift, 255u, nb);
      std::swap(ka, kb);
      std::swap(va, vb);
      ++stat->passes;
    }
  }
  hipLaunchKernelGGL(k_uq_runs, dim3(cdiv(ncl, 4)), dim3(256), 0, st, va, kw, n, call_off, b.ev.pair_off.get<uint64_t>(), (uint32_t) ncl, res, listing ? first : nullptr,
                     *ev_stat_out);
}
