// What the callers that list events and then sort them share (sjcall.hip, gaps.hip, cliploci.hip): the record pass that lists the events
// of a record table tile by tile, and the kernels between the stages of the radix sort that turn sorted keys into runs.  Everything here
// is identical in its callers up to the row type; what carries a definition of include/breakid_hip.h stays in the caller's file.
#pragma once
#include "bk_common.h"
#include "bp.h"
#include "prims.h"

namespace runs
{
constexpr uint32_t NONE = 0xFFFFFFFFu;

inline int bits_of(uint64_t v)
{
  int b = 0;
  for (; v; v >>= 1) ++b;
  return b;
}

// one word from the device; waits for the stream
inline uint32_t read_u32(const uint32_t *d, hipStream_t st)
{
  uint32_t v = 0;
  HIP_CHECK(hipMemcpyAsync(&v, d, sizeof v, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  return v;
}

// ---- the record pass ------------------------------------------------------------------------------------------------------------------
// One wavefront per tile of 256 records, four tiles to a workgroup; lane l of tile t takes the records i0 = 256 t + 4 l .. i0 + 3.
constexpr uint32_t TILE_SHIFT = 8;
constexpr uint32_t TILE = 1u << TILE_SHIFT;
static_assert(TILE == 4 * BK_WAVE, "the record pass deals four records to each of 64 lanes");
inline uint64_t tiles_of(uint64_t n) { return (n + TILE - 1) >> TILE_SHIFT; }

// the length of contig tid >= 0 from the nt + 1 prefix sums of the lengths, 0 for a contig that the reference list does not have
__device__ __forceinline__ uint32_t tlen(const uint32_t *__restrict__ tprefix, int nt, int32_t tid) { return tid < nt ? tprefix[tid + 1] - tprefix[tid] : 0u; }

struct Totals
{
  uint32_t events;
  uint32_t pad;
  unsigned long long elig_beyond;  // eligible records | beyond << 32
};

// the three totals in one place, for one copy to the host
static __global__ void k_totals(const uint32_t *__restrict__ ex, const unsigned long long *__restrict__ eb, uint64_t n_tiles, Totals *__restrict__ tot)
{
  if (threadIdx.x || blockIdx.x) return;
  Totals o;
  o.events = ex[n_tiles];
  o.pad = 0;
  o.elig_beyond = eb[n_tiles];
  *tot = o;
}

// The host's side of the pass over n records (none: nothing is launched).  count(n_tiles, tile_ev, tile_eb) launches pass one, which writes the events of every
// tile and its eligible records | its events beyond a contig's end << 32; both are scanned in place (n_tiles + 1 entries), the three
// totals go into s (events, eligible, beyond) with one copy and one wait, and emit(n_tiles, ex) launches pass two over the scanned
// events when there is one.  Throws BK_ERR_LIMIT with `too_many` beyond 2^30 events, s filled in.
template <class Bufs, class Stats, class Count, class Emit>
inline void record_pass(uint64_t n, Bufs &b, hipStream_t st, const char *too_many, Stats &s, Count count, Emit emit)
{
  if (n == 0) return;
  const uint64_t nt = tiles_of(n);
  uint32_t *tile_ev = b.tile_ev.template as<uint32_t>(nt + 1);
  unsigned long long *tile_eb = b.tile_eb.template as<unsigned long long>(nt + 1);
  count(nt, tile_ev, tile_eb);
  prims::exclusive_scan<uint32_t>(tile_ev, tile_ev, nt, b.scan_tmp, st);
  prims::exclusive_scan<unsigned long long>(tile_eb, tile_eb, nt, b.scan_tmp64, st);
  Totals *d_tot = b.totals.template as<Totals>(1), tot;
  hipLaunchKernelGGL(k_totals, dim3(1), dim3(64), 0, st, tile_ev, tile_eb, nt, d_tot);
  HIP_CHECK(hipMemcpyAsync(&tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  s.events = tot.events;
  s.eligible = tot.elig_beyond & 0xFFFFFFFFull;
  s.beyond = tot.elig_beyond >> 32;
  if (s.events == 0) return;
  if (s.events > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, too_many);
  emit(nt, (const uint32_t *) tile_ev);
}

// ---- between the sort stages ----------------------------------------------------------------------------------------------------------
// head[i] = 1 where sorted key i differs from its predecessor in the bits from `shift` up (`first` at i == 0); sub[i] (may be null) = 1
// where the whole key differs or head[i] is set
static __global__ __launch_bounds__(256) void k_key_heads(const uint64_t *__restrict__ keys, uint32_t n, int shift, uint32_t first, uint32_t *__restrict__ head, uint32_t *__restrict__ sub)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t h = first, s = first;
  if (i)
  {
    const uint64_t a = keys[i - 1], b = keys[i];
    h = (a >> shift) != (b >> shift);
    s = a != b;
  }
  head[i] = h;
  if (sub) sub[i] = s | h;
}

// ex = the exclusive scan of heads that are 0 or 1, and 1 at i == 0 (n + 1 entries), so item i is a head exactly where ex[i + 1] != ex[i]
// and the heads themselves need not be kept.  start[r] = the first item of run r, start[runs] = n (the array has n + 1 entries and
// runs <= n); id[i] (may be null) = the run of item i.
static __global__ __launch_bounds__(256) void k_run_starts(const uint32_t *__restrict__ ex, uint32_t n, uint32_t *__restrict__ start, uint32_t *__restrict__ id)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (ex[i + 1] != ex[i]) start[ex[i]] = i;
  if (i == 0) start[ex[n]] = n;
  if (id) id[i] = ex[i + 1] - 1u;
}

// ex = the exclusive scan of heads that are 0 at i == 0: ex[i + 1] is the dense rank of sorted key i, which goes to the row it came from
template <class Row> __global__ __launch_bounds__(256) void k_dense_rank(const uint32_t *__restrict__ vals, const uint32_t *__restrict__ ex, uint32_t n, Row *__restrict__ row)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  row[vals[i]].qrank = ex[i + 1];
}

template <class Row> __global__ __launch_bounds__(256) void k_gather_rows(const Row *__restrict__ row, const uint32_t *__restrict__ vals, uint32_t n, Row *__restrict__ sorted)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  sorted[i] = row[vals[i]];
}

// exk = the exclusive scan of keep (n + 1 entries): a kept row i is output row exk[i]
template <class Row> __global__ __launch_bounds__(256) void k_keep_out(const Row *__restrict__ rows, const uint32_t *__restrict__ exk, uint32_t n, Row *__restrict__ out)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (exk[i + 1] != exk[i]) out[exk[i]] = rows[i];
}
}  // namespace runs
