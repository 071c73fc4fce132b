// Junction consensus (bk_clip_consensus): the clipped bases of a table of reads, piled up per breakpoint side and
// voted per column.  Count, scan, fill, pile up: one lane per alignment walks its CIGAR, finds its clip events and looks them up in
// the sorted site keys; integer atomics count, then hand out, the slots of a site's range (the order inside a range cannot show:
// every result is a sum or an argmax); one wavefront per site then reads the bases, lane j the column j.
#include "consensus.h"
#include "bp.h"
#include "prims.h"
#include <algorithm>

namespace
{
constexpr uint16_t CONS_FLAG_NEVER = 0x4 | 0x200 | 0x400;
constexpr uint32_t CIGAR_S = 4, CIGAR_H = 5;
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;

using ReadsView = ConsensusReads;

// (tid, p, dir) as one ascending key: tid >= 0 and p fits 32 bits, or no site can hold the event
__host__ __device__ __forceinline__ unsigned long long site_key(int32_t tid, uint32_t p, uint32_t dir)
{
  return ((unsigned long long) (uint32_t) tid << 33) | ((unsigned long long) p << 1) | (unsigned long long) dir;
}

struct ClipEvent
{
  bool on;
  unsigned long long key;
  uint32_t c;               // length of the S op
  unsigned long long q0;    // nibble index of column 0 in the seq bytes: column j is nibble q0 + j (LEFT) or q0 - j (RIGHT)
};

// The events of alignment i: ev[0] trailing (LEFT), ev[1] leading (RIGHT), as bk_clip_support places them, on an alignment that is
// eligible here (include/breakid_hip.h).  l_seq == the CIGAR's query length is part of that: with it c <= l_seq, so every nibble
// q0 +- j with j < c lies inside the (l_seq + 1) / 2 bytes of the read.
__device__ __forceinline__ void read_events(const ReadsView &r, uint64_t i, int mapq_min, int min_clip, ClipEvent ev[2], uint32_t &words)
{
  ev[0].on = ev[1].on = false;
  const int32_t tid = r.tid[i];
  const uint32_t l_seq = r.l_seq[i];
  if (tid < 0 || (r.flag[i] & CONS_FLAG_NEVER) || (int) r.mapq[i] < mapq_min || l_seq == 0) return;
  const uint32_t c0 = r.cigar_off[i], c1 = r.cigar_off[i + 1];
  if (c1 <= c0) return;
  const uint32_t *__restrict__ cg = r.cigar;
  uint32_t a = c0, z = c1 - 1;
  uint32_t wa = cg[a], wz = cg[z];
  while ((wa & 15u) == CIGAR_H && a < z) wa = cg[++a];
  while ((wz & 15u) == CIGAR_H && z > a) wz = cg[--z];
  const bool l = (wa & 15u) == CIGAR_S && (long long) (wa >> 4) >= min_clip;
  const bool t = (wz & 15u) == CIGAR_S && (long long) (wz >> 4) >= min_clip;
  words += 2;
  if (!l && !t) return;
  long long reflen = 0;
  unsigned long long qlen = 0;
  for (uint32_t k = c0; k < c1; ++k)
  {
    const uint32_t v = cg[k], op = v & 15u;
    if ((0x3C1A7u >> (op << 1)) & 2u) reflen += (long long) (v >> 4);  // M, D, N, =, X
    if ((0x3C1A7u >> (op << 1)) & 1u) qlen += (unsigned long long) (v >> 4);  // M, I, S, =, X
  }
  words += c1 - c0;
  if (reflen <= 0 || qlen != (unsigned long long) l_seq) return;
  const long long pos = r.pos[i];
  const unsigned long long nib0 = r.seq_off[i] * 2ull;
  const long long pt = pos + reflen, pl = pos + 1;
  if (t && pt >= 0 && pt <= 0xFFFFFFFFll)
  {
    ev[0].on = true;
    ev[0].key = site_key(tid, (uint32_t) pt, 0u);
    ev[0].c = wz >> 4;
    ev[0].q0 = nib0 + (unsigned long long) (l_seq - (wz >> 4));
  }
  if (l && pl >= 0 && pl <= 0xFFFFFFFFll)
  {
    ev[1].on = true;
    ev[1].key = site_key(tid, (uint32_t) pl, 1u);
    ev[1].c = wa >> 4;
    ev[1].q0 = nib0 + (unsigned long long) ((wa >> 4) - 1u);
  }
}

__device__ __forceinline__ uint32_t key_lower(const unsigned long long *__restrict__ keys, uint32_t n, unsigned long long key)
{
  uint32_t lo = 0, hi = n;
  while (lo < hi)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// FILL = false: counts[s] += 1 for every event of slot s.  FILL = true: the event takes the next free place of off[s] .. off[s + 1].
template <bool FILL>
__global__ __launch_bounds__(256) void k_cons_walk(ReadsView r, int mapq_min, int min_clip, const unsigned long long *__restrict__ keys, uint32_t n_keys,
                                                   unsigned long long *__restrict__ counts, const unsigned long long *__restrict__ off, unsigned long long n_contrib,
                                                   unsigned long long *__restrict__ q0, uint32_t *__restrict__ clen, ConsensusStat *__restrict__ stat)
{
  const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  uint32_t words = 0;
  if (i < r.n)
  {
    ClipEvent ev[2];
    read_events(r, i, mapq_min, min_clip, ev, words);
#pragma unroll
    for (int d = 0; d < 2; ++d)
    {
      if (!ev[d].on) continue;
      for (uint32_t s = key_lower(keys, n_keys, ev[d].key); s < n_keys && keys[s] == ev[d].key; ++s)
      {
        const unsigned long long at = atomicAdd(&counts[s], 1ull);
        if (FILL)
        {
          const unsigned long long dest = off[s] + at;
          if (dest < off[s + 1] && dest < n_contrib)  // (always: both walks see the same events)
          {
            q0[dest] = ev[d].q0;
            clen[dest] = ev[d].c;
          }
        }
      }
    }
  }
  words = wave_sum(words);
  if ((threadIdx.x & 63) == 0 && words) atomicAdd(&stat->words, (unsigned long long) words);
}

// One wavefront per site, four to a workgroup.  Lane j owns column j, in rounds of 64 columns: the 64 lanes read 32 consecutive
// bytes of one read, then the next read's.  Four counters and the depth stay in registers.
__global__ __launch_bounds__(256) void k_cons_pile(const uint32_t *__restrict__ slot_of, uint32_t n_sites, const unsigned long long *__restrict__ keys,
                                                   const unsigned long long *__restrict__ off, const unsigned long long *__restrict__ q0, const uint32_t *__restrict__ clen,
                                                   const uint8_t *__restrict__ seq, uint32_t max_len, uint32_t min_depth, struct bk_consensus *__restrict__ res,
                                                   uint8_t *__restrict__ bases, uint32_t *__restrict__ depth, ConsensusStat *__restrict__ stat)
{
  const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (k >= n_sites) return;  // (the whole wave)
  const uint32_t s = slot_of[k];
  unsigned long long b0 = 0, b1 = 0;
  bool right = false;
  if (s != NO_SLOT)
  {
    b0 = off[s];
    b1 = off[s + 1];
    right = (keys[s] & 1ull) != 0;
  }
  uint32_t len = 0, match = 0, total = 0, cmax = 0;
  unsigned long long seq_bytes = 0;
  for (uint32_t j0 = 0; j0 < max_len; j0 += 64)
  {
    const uint32_t j = j0 + lane;
    const bool in = j < max_len;
    uint32_t nA = 0, nC = 0, nG = 0, nT = 0, dep = 0;
    if (j0 == 0 || j0 < cmax)  // (the same on every lane)
      for (unsigned long long t = b0; t < b1; ++t)
      {
        const uint32_t c = clen[t];
        const unsigned long long q = q0[t];
        if (j0 == 0)
        {
          cmax = c > cmax ? c : cmax;
          seq_bytes += ((c < max_len ? c : max_len) + 1u) / 2u;
        }
        if (in && j < c)
        {
          const unsigned long long nib = right ? q - j : q + j;
          const uint32_t byte = seq[nib >> 1];
          const uint32_t code = (nib & 1ull) ? (byte & 15u) : (byte >> 4);
          ++dep;
          nA += code == 1u;
          nC += code == 2u;
          nG += code == 4u;
          nT += code == 8u;
        }
      }
    uint32_t w = nA;
    uint8_t ch = 'A';
    if (nC > w) w = nC, ch = 'C';
    if (nG > w) w = nG, ch = 'G';
    if (nT > w) w = nT, ch = 'T';
    if (w == 0) ch = 'N';
    const bool ok = in && dep >= min_depth;
    len += (uint32_t) __popcll(__ballot(ok));
    match += ok ? w : 0u;
    total += ok ? dep : 0u;
    if (in)
    {
      const uint64_t o = (uint64_t) k * max_len + j;
      bases[o] = ok ? ch : (uint8_t) 0;
      depth[o] = dep;
    }
  }
  match = wave_sum(match);
  total = wave_sum(total);
  if (lane == 0)
  {
    struct bk_consensus v;
    v.n_reads = (uint32_t) (b1 - b0);
    v.len = len;
    v.match = match;
    v.total = total;
    res[k] = v;
    if (b1 > b0)
    {
      atomicAdd(&stat->contributions, b1 - b0);
      atomicAdd(&stat->seq_bytes, seq_bytes);
    }
  }
}

template <class T> const T *upload(DevBuf &b, const T *host, uint64_t count, hipStream_t st)
{
  T *d = b.as<T>(count + 1);
  if (count) HIP_CHECK(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, st));
  return d;
}
}  // namespace

void consensus_upload(const bk_reads &reads, ConsensusBufs &b, hipStream_t st)
{
  ConsensusReads &r = b.view;
  r = ConsensusReads{};
  b.d_seq = nullptr;
  r.n = reads.n;
  if (!reads.n) return;
  r.tid = upload(b.tid, reads.tid, reads.n, st);
  r.pos = upload(b.pos, reads.pos, reads.n, st);
  r.flag = upload(b.flag, reads.flag, reads.n, st);
  r.mapq = upload(b.mapq, reads.mapq, reads.n, st);
  r.cigar_off = upload(b.cigar_off, reads.cigar_off, reads.n + 1, st);
  r.cigar = upload(b.cigar, reads.cigar, reads.cigar_off[reads.n], st);
  r.l_seq = upload(b.l_seq, reads.l_seq, reads.n, st);
  r.seq_off = upload(b.seq_off, reads.seq_off, reads.n + 1, st);
  b.d_seq = upload(b.seq, reads.seq, reads.seq_off[reads.n], st);
}

void clip_consensus(const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, uint32_t max_len, uint32_t min_depth, ConsensusBufs &b, hipStream_t st,
                    struct bk_consensus **res_out, uint8_t **bases_out, uint32_t **depth_out, ConsensusStat **stat_out)
{
  static_assert(sizeof(struct bk_consensus) == 16, "bk_consensus must be 16 bytes");
  struct bk_consensus *res = b.res.as<struct bk_consensus>(n_sites + 1);
  uint8_t *bases = b.bases.as<uint8_t>(n_sites * max_len + 1);
  uint32_t *depth = b.depth.as<uint32_t>(n_sites * max_len + 1);
  ConsensusStat *stat = b.stat.as<ConsensusStat>(1);
  HIP_CHECK(hipMemsetAsync(stat, 0, sizeof(ConsensusStat), st));
  *res_out = res;
  *bases_out = bases;
  *depth_out = depth;
  *stat_out = stat;
  if (n_sites == 0) return;
  // the sites in key order; equal sites keep a slot each, so an event counts under each of them
  std::vector<std::pair<unsigned long long, uint32_t>> order;
  order.reserve(n_sites);
  for (uint64_t k = 0; k < n_sites; ++k)
    if (sites[k].tid >= 0) order.emplace_back(site_key(sites[k].tid, sites[k].pos, sites[k].dir), (uint32_t) k);
  std::sort(order.begin(), order.end());
  const uint32_t n_keys = (uint32_t) order.size();
  std::vector<unsigned long long> &h_keys = b.h_keys;
  std::vector<uint32_t> &h_slot = b.h_slot;
  h_keys.assign(n_keys, 0ull);
  h_slot.assign(n_sites, NO_SLOT);
  for (uint32_t s = 0; s < n_keys; ++s)
  {
    h_keys[s] = order[s].first;
    h_slot[order[s].second] = s;
  }
  const unsigned long long *d_keys = upload(b.keys, h_keys.data(), n_keys, st);
  const uint32_t *d_slot = upload(b.slot_of, h_slot.data(), n_sites, st);
  unsigned long long *counts = b.counts.as<unsigned long long>((uint64_t) n_keys + 1);
  unsigned long long *off = b.off.as<unsigned long long>((uint64_t) n_keys + 1);
  HIP_CHECK(hipMemsetAsync(off, 0, ((uint64_t) n_keys + 1) * 8, st));
  const unsigned long long *d_q0 = nullptr;
  const uint32_t *d_clen = nullptr;
  const uint8_t *d_seq = b.d_seq;
  const ReadsView &r = b.view;
  if (r.n && n_keys)
  {
    const unsigned grid = cdiv(r.n, 256);
    HIP_CHECK(hipMemsetAsync(counts, 0, ((uint64_t) n_keys + 1) * 8, st));
    hipLaunchKernelGGL(k_cons_walk<false>, dim3(grid), dim3(256), 0, st, r, mapq_min, min_clip, d_keys, n_keys, counts, (const unsigned long long *) nullptr, 0ull,
                       (unsigned long long *) nullptr, (uint32_t *) nullptr, stat);
    prims::exclusive_scan<unsigned long long>(counts, off, n_keys, b.scan_tmp, st);
    unsigned long long n_contrib = 0;
    HIP_CHECK(hipMemcpyAsync(&n_contrib, off + n_keys, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));  // the number of contributions sizes their list
    if (n_contrib > 0xFFFFFFFFull) throw bk_error(BK_ERR_LIMIT, "bk_clip_consensus: more than 2^32 contributions");
    if (n_contrib)
    {
      unsigned long long *q0 = b.q0.as<unsigned long long>(n_contrib);
      uint32_t *clen = b.clen.as<uint32_t>(n_contrib);
      HIP_CHECK(hipMemsetAsync(counts, 0, ((uint64_t) n_keys + 1) * 8, st));  // (now the cursor of every range)
      HIP_CHECK(hipMemsetAsync(clen, 0, n_contrib * 4, st));                  // (a place nobody takes holds no column)
      hipLaunchKernelGGL(k_cons_walk<true>, dim3(grid), dim3(256), 0, st, r, mapq_min, min_clip, d_keys, n_keys, counts, off, n_contrib, q0, clen, stat);
      d_q0 = q0;
      d_clen = clen;
    }
  }
  hipLaunchKernelGGL(k_cons_pile, dim3(cdiv(n_sites, 4)), dim3(256), 0, st, d_slot, (uint32_t) n_sites, d_keys, off, d_q0, d_clen, d_seq, max_len, min_depth, res, bases,
                     depth, stat);
}
