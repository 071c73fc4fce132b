// Fusion frame (bk_fusion_frame): for every call the transcripts that overlap either breakpoint, what each retains of
// its coding sequence on the side the call keeps, and the class of every pair of them.  The model is sorted by (tid, tx_start), so the
// transcripts that start in front of a position are a prefix of their contig's run; the running maximum of tx_end says where a walk
// backwards through that prefix may stop.  One wavefront per call: both sides staged in LDS a chunk at a time, the pairs dealt to the
// lanes, one key reduced by shuffles.  Integer arithmetic only, no atomics.
#include "frame.h"
#include "wave.h"
#include "prims.h"

namespace
{
// ---- what the device derives on upload ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_frame_part_len(const uint32_t *__restrict__ s, const uint32_t *__restrict__ e, uint32_t n, unsigned long long *__restrict__ len)
{
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g < n) len[g] = (unsigned long long) (e[g] - s[g]);
}

__global__ __launch_bounds__(256) void k_frame_keys(const int32_t *__restrict__ tid, const uint32_t *__restrict__ start, uint32_t n, unsigned long long *__restrict__ key)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) key[i] = ((unsigned long long) (uint32_t) tid[i] << 32) | start[i];
}

// The running maximum of tx_end inside every contig's run, as the running maximum of (tid << 32) | tx_end over the whole model: tid
// ascends, so the largest key up to row i carries tid[i] and the largest tx_end of its run so far.  One workgroup walks the rows 256
// at a time with the carry in a register (the shape of prims::k_scan_one, with max in place of +).
__global__ __launch_bounds__(256) void k_frame_run_max(const int32_t *__restrict__ tid, const uint32_t *__restrict__ end, uint32_t n, uint32_t *__restrict__ run_max)
{
  __shared__ unsigned long long wmax[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < n; base += 256)
  {
    const uint32_t i = base + threadIdx.x;
    unsigned long long v = i < n ? ((unsigned long long) (uint32_t) tid[i] << 32) | end[i] : 0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
      const unsigned long long o = __shfl_up(v, d, 64);
      if (lane >= d && o > v) v = o;
    }
    if (lane == 63) wmax[w] = v;
    __syncthreads();
    unsigned long long tot = carry;
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
      const unsigned long long s = wmax[k];
      if (k < w && s > v) v = s;
      tot = s > tot ? s : tot;
    }
    __syncthreads();
    if (carry > v) v = carry;
    if (i < n) run_max[i] = (uint32_t) v;
    carry = tot;
  }
}

// ---- one transcript on one side -------------------------------------------------------------------------------------------------------
struct TxInfo
{
  uint32_t L, cod, role, exon, loc;
};

// Transcript i < n_tx against the side (P, right), P >= 1.  Its parts are the entries o0 .. o1 - 1, o1 <= n_parts; cum has
// n_parts + 1 entries.  k = the parts that start in front of P (those with a retained base on a LEFT side are 0 .. k - 1), j = the
// parts that end in front of P (those with a retained base on a RIGHT side are j .. np - 1).
__device__ __forceinline__ TxInfo tx_info(const FrameModel &m, uint32_t i, long long P, bool right)
{
  const uint32_t o0 = m.ex_off[i], o1 = m.ex_off[i + 1], np = o1 - o0;
  const bool minus = m.strand[i] != 0;
  const unsigned long long base = m.cum[o0];
  TxInfo t;
  t.L = (uint32_t) (m.cum[o1] - base);
  uint32_t lo = o0, hi = o1;
  while (lo < hi)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((long long) m.ex_start[mid] < P)
      lo = mid + 1;
    else
      hi = mid;
  }
  const uint32_t k = lo - o0;
  lo = o0, hi = o1;
  while (lo < hi)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((long long) m.ex_end[mid] < P)
      lo = mid + 1;
    else
      hi = mid;
  }
  const uint32_t j = lo - o0;
  const long long b = P - 1;
  long long r;
  if (!right)
  {
    r = 0;
    if (k)
    {
      const long long s = m.ex_start[o0 + k - 1], e = m.ex_end[o0 + k - 1];
      r = (long long) (m.cum[o0 + k - 1] - base) + (P < e ? P : e) - s;
    }
  }
  else
  {
    long long below = (long long) (m.cum[o0 + j] - base);  // (j == np: the whole length)
    if (j < np)
    {
      const long long s = m.ex_start[o0 + j];
      if (b > s) below += b - s;
    }
    r = (long long) t.L - below;
  }
  const bool head = !minus == !right;
  t.role = head ? BK_FRAME_HEAD : BK_FRAME_TAIL;
  t.cod = (uint32_t) (head ? r : (long long) t.L - r);
  uint32_t exon;
  if (!right)
    exon = !k ? 0u : !minus ? k : np - (k - 1);
  else
    exon = j >= np ? 0u : minus ? np - j : j + 1;
  t.exon = exon > 65535u ? 65535u : exon;
  if (np == 0)
    t.loc = BK_LOC_NONCODING;
  else if (b < (long long) m.ex_start[o0])
    t.loc = minus ? BK_LOC_3UTR : BK_LOC_5UTR;
  else if (b >= (long long) m.ex_end[o1 - 1])
    t.loc = minus ? BK_LOC_5UTR : BK_LOC_3UTR;
  else  // (k >= 1: the first part starts at or in front of b)
    t.loc = b < (long long) m.ex_end[o0 + k - 1] ? BK_LOC_CDS : BK_LOC_INTRON;
  return t;
}

__device__ __forceinline__ uint32_t pair_class(uint32_t role_a, uint32_t cod_a, uint32_t L_a, uint32_t role_b, uint32_t cod_b, uint32_t L_b)
{
  if (role_a == role_b) return BK_FRAME_ANTISENSE;
  const bool a_head = role_a == BK_FRAME_HEAD;
  const uint32_t h = a_head ? cod_a : cod_b, Lh = a_head ? L_a : L_b, t = a_head ? cod_b : cod_a, Lt = a_head ? L_b : L_a;
  if (h > 0 && h < Lh && t > 0 && t < Lt) return h % 3u == t % 3u ? BK_FRAME_INFRAME : BK_FRAME_OUTFRAME;
  if (h == 0 && t == 0 && Lh > 0 && Lt > 0) return BK_FRAME_PROMOTER;
  return BK_FRAME_TRUNCATING;
}

// ---- the walk over the transcripts that overlap one side ------------------------------------------------------------------------------
struct SideTx
{
  uint32_t idx, L, cod, role;
};
struct WaveLds
{
  SideTx s[2][FRAME_CHUNK];
};
static_assert(FRAME_CHUNK >= 64 && FRAME_CHUNK % 64 == 0, "a chunk takes whole steps of 64 candidates");

// U = the rows whose key is below (tid, P): the rows in front of the contig's run and those of the run with tx_start < P
__device__ __forceinline__ uint32_t frame_upper(const FrameModel &m, int32_t tid, uint32_t P)
{
  const unsigned long long want = ((unsigned long long) (uint32_t) tid << 32) | P;
  uint32_t lo = 0, hi = m.n_tx;
  while (lo < hi)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (m.key[mid] < want)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// Fills s[0 .. count) with the next overlapping transcripts of the side, walking backwards from `top` (the next row to test, -1: the
// walk is over), whole steps of 64 rows while a step's worst case still fits.  A step ends the walk when its first row lies on another
// contig or the running maximum there is below P: nothing further back reaches P.  Every row read is 0 <= top - lane <= top < U <= n_tx.
// single: the side's best transcript alone, (L << 24) | (0xFFFFFF - idx), kept per lane.
__device__ __forceinline__ uint32_t frame_fill(const FrameModel &m, int32_t tid, uint32_t P, bool right, long long &top, SideTx *s, unsigned long long &single)
{
  const int lane = threadIdx.x & 63;
  uint32_t count = 0;
  while (top >= 0 && count + 64 <= FRAME_CHUNK)
  {
    if ((int32_t) (m.key[top] >> 32) != tid || m.run_max[top] < P)
    {
      top = -1;
      break;
    }
    const long long i = top - lane;
    const bool hit = i >= 0 && (int32_t) (m.key[i] >> 32) == tid && m.tx_end[i] >= P;
    const unsigned long long mask = __ballot(hit);
    if (hit)
    {
      const TxInfo t = tx_info(m, (uint32_t) i, (long long) P, right);
      SideTx e;
      e.idx = (uint32_t) i, e.L = t.L, e.cod = t.cod, e.role = t.role;
      s[count + __popcll(mask & ((1ull << lane) - 1ull))] = e;
      const unsigned long long key = ((unsigned long long) t.L << 24) | (0xFFFFFFull - (unsigned long long) i);
      single = key > single ? key : single;
    }
    count += (uint32_t) __popcll(mask);
    top -= 64;
  }
  if (top < 0) top = -1;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return count;
}

// One wavefront per site, four to a workgroup; a wavefront touches its own part of the LDS only, so no workgroup barrier.
// The pair key: hi = (class << 33) | (L_A + L_B), lo = ((0xFFFFFF - idx_A) << 24) | (0xFFFFFF - idx_B); a pair has a class >= 1, so
// hi == 0 is "no pair".  Side 2 is walked again for every chunk of side 1; a side of at most FRAME_CHUNK - 63 transcripts is one chunk.
__global__ __launch_bounds__(256) void k_fusion_frame(FrameModel m, const struct bk_frame_site *__restrict__ sites, uint32_t n, struct bk_frame_call *__restrict__ res)
{
  __shared__ WaveLds lds[4];
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t k = blockIdx.x * 4 + wv;
  if (k >= n) return;
  WaveLds &S = lds[wv];
  const struct bk_frame_site site = sites[k];
  const int32_t tid[2] = {site.tid1, site.tid2};
  const uint32_t P[2] = {site.pos1, site.pos2};
  const bool right[2] = {site.right1 != 0, site.right2 != 0};
  long long first[2];
  for (int s = 0; s < 2; ++s) first[s] = tid[s] >= 0 && m.n_tx ? (long long) frame_upper(m, tid[s], P[s]) - 1 : -1;

  unsigned long long best_hi = 0, best_lo = 0, n_in = 0, n_ok = 0, single[2] = {0, 0};
  uint32_t n_side[2] = {0, 0};
  long long top1 = first[0];
  bool first_pass = true;
  do
  {
    const uint32_t c1 = frame_fill(m, tid[0], P[0], right[0], top1, S.s[0], single[0]);
    n_side[0] += c1;
    long long top2 = first[1];
    do
    {
      const uint32_t c2 = frame_fill(m, tid[1], P[1], right[1], top2, S.s[1], single[1]);
      if (first_pass) n_side[1] += c2;
      for (uint32_t p = lane; p < c1 * c2; p += 64)
      {
        const SideTx a = S.s[0][p / c2], b = S.s[1][p % c2];
        const uint32_t cls = pair_class(a.role, a.cod, a.L, b.role, b.cod, b.L);
        n_in += cls == BK_FRAME_INFRAME;
        n_ok += cls >= BK_FRAME_TRUNCATING;
        const unsigned long long hi = ((unsigned long long) cls << 33) | ((unsigned long long) a.L + (unsigned long long) b.L);
        const unsigned long long lo = ((0xFFFFFFull - a.idx) << 24) | (0xFFFFFFull - b.idx);
        if (hi > best_hi || (hi == best_hi && lo > best_lo)) best_hi = hi, best_lo = lo;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the next fill overwrites what the lanes have just read)
      __builtin_amdgcn_wave_barrier();
    } while (top2 >= 0);
    first_pass = false;
  } while (top1 >= 0);

  // the largest (hi, lo): first hi, then lo among the lanes that hold it
  const unsigned long long top_hi = wave_max(best_hi);
  const unsigned long long top_lo = wave_max(best_hi == top_hi ? best_lo : 0ull);
  n_in = wave_sum(n_in);
  n_ok = wave_sum(n_ok);
  single[0] = wave_max(single[0]);
  single[1] = wave_max(single[1]);

  struct bk_frame_call o;
  o.cls = o.order = 0;
  o.reserved = 0, o.reserved2 = 0;
  o.n_inframe = n_in > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) n_in;
  o.n_compatible = n_ok > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) n_ok;
  for (int s = 0; s < 2; ++s)
  {
    o.n_tx[s] = n_side[s];
    o.tx[s] = -1;
    o.loc[s] = o.role[s] = 0;
    o.exon[s] = 0;
    o.cod[s] = 0;
    long long idx = -1;
    if (top_hi)
      idx = (long long) (0xFFFFFFull - ((top_lo >> (s ? 0 : 24)) & 0xFFFFFFull));
    else if (n_side[s])
      idx = (long long) (0xFFFFFFull - (single[s] & 0xFFFFFFull));
    if (idx < 0) continue;
    const TxInfo t = tx_info(m, (uint32_t) idx, (long long) P[s], right[s]);  // (the same on every lane)
    o.tx[s] = (int32_t) idx;
    o.loc[s] = (uint8_t) t.loc;
    o.role[s] = (uint8_t) t.role;
    o.exon[s] = (uint16_t) t.exon;
    o.cod[s] = t.cod;
  }
  if (top_hi)
  {
    o.cls = (uint8_t) (top_hi >> 33);
    o.order = o.cls == BK_FRAME_ANTISENSE ? 0 : o.role[0] == BK_FRAME_HEAD ? 1 : 2;
  }
  if (lane == 0) res[k] = o;
}
}  // namespace

void frame_upload(const bk_txmodel &t, const struct bk_frame_site *sites, uint64_t n, FrameBufs &b, hipStream_t st)
{
  FrameModel &v = b.view;
  v.n_tx = (uint32_t) t.n_tx;
  (void) upload(b.tid, t.tid, t.n_tx, st);
  (void) upload(b.tx_start, t.tx_start, t.n_tx, st);
  v.tx_end = upload(b.tx_end, t.tx_end, t.n_tx, st);
  v.strand = upload(b.strand, t.strand, t.n_tx, st);
  v.ex_off = upload(b.ex_off, t.ex_off, t.n_tx ? t.n_tx + 1 : 0, st);
  v.ex_start = upload(b.ex_start, t.ex_start, t.n_tx ? t.n_parts : 0, st);
  v.ex_end = upload(b.ex_end, t.ex_end, t.n_tx ? t.n_parts : 0, st);
  b.d_sites = upload(b.sites, sites, n, st);
}

void frame_derive(const bk_txmodel &t, FrameBufs &b, hipStream_t st)
{
  FrameModel &v = b.view;
  const uint32_t n_tx = (uint32_t) t.n_tx, n_parts = t.n_tx ? (uint32_t) t.n_parts : 0u;
  unsigned long long *key = b.key.as<unsigned long long>(t.n_tx + 1), *cum = b.cum.as<unsigned long long>((uint64_t) n_parts + 1);
  uint32_t *run_max = b.run_max.as<uint32_t>(t.n_tx + 1);
  v.key = key, v.cum = cum, v.run_max = run_max;
  if (n_parts) hipLaunchKernelGGL(k_frame_part_len, dim3(cdiv(n_parts, 256)), dim3(256), 0, st, v.ex_start, v.ex_end, n_parts, cum);
  prims::exclusive_scan<unsigned long long>(cum, cum, n_parts, b.scan_tmp, st);
  if (!n_tx) return;
  hipLaunchKernelGGL(k_frame_keys, dim3(cdiv(n_tx, 256)), dim3(256), 0, st, b.tid.get<int32_t>(), b.tx_start.get<uint32_t>(), n_tx, key);
  hipLaunchKernelGGL(k_frame_run_max, dim3(1), dim3(256), 0, st, b.tid.get<int32_t>(), v.tx_end, n_tx, run_max);
}

void fusion_frame(uint64_t n, FrameBufs &b, hipStream_t st, struct bk_frame_call **res_out)
{
  static_assert(sizeof(struct bk_frame_site) == 24 && sizeof(struct bk_frame_call) == 48, "bk_frame_site must be 24 bytes and bk_frame_call 48");
  struct bk_frame_call *res = b.res.as<struct bk_frame_call>(n + 1);
  *res_out = res;
  if (n == 0) return;
  hipLaunchKernelGGL(k_fusion_frame, dim3(cdiv(n, 4)), dim3(256), 0, st, b.view, b.d_sites, (uint32_t) n, res);
}
