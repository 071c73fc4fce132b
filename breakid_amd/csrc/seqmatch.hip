// Sequence match (bk_sequence_match): short queries searched in a library of sequences the caller supplies, by a k-mer
// index and seeded ungapped extension.  The index: every k-mer of the panel (k = seed) that holds no N and lies inside one sequence, as
// a 2k-bit key with its position in the panel as the value, sorted by prims::radix_sort_pairs.  The probes: one wavefront per probe
// stages both orientations of the query in LDS as codes, its lanes take the query's k-mers, look each up in the sorted keys by binary
// search and walk the equal run.  A hit whose preceding cell matches too lies inside a run and is skipped, so that every run of at
// least k cells is met exactly once, at its first cell: that is n_seeds.  Every run start scans its whole diagonal with the running sum
// of bk_locus_similarity.  No atomics, no float; nothing is capped (a k-mer that the panel holds R times costs R per query k-mer
// that equals it).
#include "seqmatch.h"
#include "runs.h"
#include "wave.h"

namespace
{
constexpr uint32_t SM_N = 4;            // the codes are A C G T = 0 1 2 3, so that the complement is ^ 3
constexpr uint32_t SM_SEQ = 0xFFFFFu;   // 2^20 sequences
constexpr uint32_t SM_POS = 0xFFFFFFFu; // 2^28 panel bases
// the key that orders the candidates (include/breakid_hip.h) in two words.  hi: the score, then the shorter, the smaller sequence,
// orientation 0; lo: the smaller start on the panel, the smaller start in the query.  A candidate has a score of 1 at least, so hi == 0
// is "none".
constexpr int HI_SCORE = 30, HI_LEN = 21, HI_SEQ = 1, LO_START = 9;
// a diagonal's best score with its sequence, for score2 / seq2: score << 20 | (SM_SEQ - seq); 0 is "none"
constexpr int E_SCORE = 20;

__device__ __forceinline__ uint32_t base_code(uint8_t b) { return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : SM_N; }

// the sequence that holds panel position p: the last s with off[s] <= p (an empty sequence never is: off[s + 1] > p)
__device__ __forceinline__ uint32_t seq_of(const uint64_t *__restrict__ off, uint32_t n_seqs, uint64_t p)
{
  uint32_t lo = 0, hi = n_seqs;  // the answer lies in [lo, hi)
  while (hi - lo > 1)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// codes[p] = the code of base p; flag[p] = 1 where the k-mer from p holds no N and ends inside p's sequence
__global__ __launch_bounds__(256) void k_panel_flags(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ off, uint32_t n_seqs, uint32_t total, uint32_t k,
                                                     uint8_t *__restrict__ codes, uint32_t *__restrict__ flag)
{
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  codes[p] = (uint8_t) base_code(bases[p]);
  const uint64_t end = off[seq_of(off, n_seqs, p) + 1];
  uint32_t ok = (uint64_t) p + k <= end;
  if (ok)
    for (uint32_t j = 0; j < k; ++j)
      if (base_code(bases[p + j]) == SM_N) ok = 0;
  flag[p] = ok;
}

// ex = the exclusive scan of the flags (total + 1 entries): a flagged position p is k-mer ex[p]
__global__ __launch_bounds__(256) void k_panel_kmers(const uint8_t *__restrict__ codes, const uint32_t *__restrict__ ex, uint32_t total, uint32_t k, uint64_t *__restrict__ keys,
                                                     uint32_t *__restrict__ vals)
{
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const uint32_t at = ex[p];
  if (ex[p + 1] == at) return;
  uint64_t key = 0;
  for (uint32_t j = 0; j < k; ++j) key = (key << 2) | codes[p + j];  // (the flag says that p + k <= total)
  keys[at] = key;
  vals[at] = p;
}

struct WaveQ
{
  uint8_t q[2][256];  // q_0 and q_1 as codes
};

struct LaneBest
{
  unsigned long long hi = 0, lo = 0;
  uint32_t run = 0, e1 = 0, e2 = 0;
};

// One diagonal: the cells max(0, -d) .. min(qlen, len_s - d) - 1 of q_o against P[i + d].  The sum restarts where it is <= 0; every
// matching cell offers (sum, length since the restart), and no other end can win.
__device__ __forceinline__ void scan_diagonal(const uint8_t *q, int qlen, const uint8_t *__restrict__ P, long long len_s, long long d, uint32_t s, uint32_t o, LaneBest &b)
{
  const int i_lo = d < 0 ? (int) -d : 0;
  const int i_hi = len_s - d < (long long) qlen ? (int) (len_s - d) : qlen;
  const unsigned long long rank = ((unsigned long long) (SM_SEQ - s) << HI_SEQ) | (unsigned long long) (1u - o);
  int sum = 0, len = 0, cur = 0, top = 0;
  for (int i = i_lo; i < i_hi; ++i)
  {
    const uint32_t c = q[i];
    if (c < SM_N && c == P[i + d])
    {
      if (sum <= 0) sum = 0, len = 0;
      ++sum, ++len, ++cur;
      b.run = (uint32_t) cur > b.run ? (uint32_t) cur : b.run;
      top = sum > top ? sum : top;
      if ((unsigned long long) sum >= (b.hi >> HI_SCORE))
      {
        const int i0 = i + 1 - len;
        const unsigned long long hi = ((unsigned long long) sum << HI_SCORE) | ((unsigned long long) (511 - len) << HI_LEN) | rank;
        const unsigned long long lo = ((unsigned long long) (SM_POS - (uint32_t) (i0 + d)) << LO_START) | (unsigned long long) (511 - i0);
        if (hi > b.hi || (hi == b.hi && lo > b.lo)) b.hi = hi, b.lo = lo;
      }
    }
    else
      sum -= 2, ++len, cur = 0;
  }
  // the two best sequences of this lane by (score, smaller index)
  const uint32_t e = ((uint32_t) top << E_SCORE) | (SM_SEQ - s);
  if (b.e1 && (b.e1 & SM_SEQ) == (e & SM_SEQ))
    b.e1 = e > b.e1 ? e : b.e1;
  else if (b.e2 && (b.e2 & SM_SEQ) == (e & SM_SEQ))
  {
    b.e2 = e > b.e2 ? e : b.e2;
    if (b.e2 > b.e1)
    {
      const uint32_t t = b.e1;
      b.e1 = b.e2;
      b.e2 = t;
    }
  }
  else if (e > b.e1)
    b.e2 = b.e1, b.e1 = e;
  else if (e > b.e2)
    b.e2 = e;
}

// One wavefront per probe, four to a workgroup.
__global__ __launch_bounds__(256) void k_seq_probes(const uint8_t *__restrict__ codes, const uint64_t *__restrict__ off, uint32_t n_seqs, const uint64_t *__restrict__ keys,
                                                    const uint32_t *__restrict__ vals, uint32_t m, const struct bk_seq_probe *__restrict__ probes,
                                                    const uint8_t *__restrict__ query, uint32_t n, uint32_t max_len, uint32_t k, struct bk_seq_hit *__restrict__ res)
{
  __shared__ WaveQ lds[4];
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t kq = blockIdx.x * 4 + wv;
  WaveQ &Q = lds[wv];
  struct bk_seq_probe pr = {0, 0};
  if (kq < n) pr = probes[kq];
  const int qlen = (int) pr.qlen;  // (qlen <= max_len <= 256 is checked on the host)
  for (int j = (int) lane; j < qlen; j += 64)
  {
    const uint32_t c = base_code(query[(uint64_t) kq * max_len + (uint32_t) (pr.reversed ? qlen - 1 - j : j)]);
    Q.q[0][j] = (uint8_t) c;
    Q.q[1][qlen - 1 - j] = (uint8_t) (c < SM_N ? c ^ 3u : SM_N);
  }
  __syncthreads();
  if (kq >= n) return;
  LaneBest best;
  unsigned long long seeds = 0;
  const int per = qlen - (int) k + 1;  // the k-mers of one orientation
  for (int u = (int) lane; u < 2 * per; u += 64)  // (never entered when qlen < k, and so when m == 0 is all there is: keys is then not read)
  {
    const uint32_t o = u >= per ? 1u : 0u;
    const int i = u - (int) o * per;
    const uint8_t *q = Q.q[o];
    uint64_t key = 0;
    bool valid = true;
    for (uint32_t j = 0; j < k; ++j)
    {
      const uint32_t c = q[i + j];
      valid = valid && c < SM_N;
      key = (key << 2) | (c & 3u);
    }
    if (!valid) continue;
    uint32_t lo = 0, hi = m;  // the first sorted key >= key
    while (lo < hi)
    {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (keys[mid] < key)
        lo = mid + 1;
      else
        hi = mid;
    }
    for (uint32_t at = lo; at < m && keys[at] == key; ++at)
    {
      const uint64_t p = vals[at];
      const uint32_t s = seq_of(off, n_seqs, p);
      const uint64_t first = off[s];
      if (i > 0 && p > first)
      {
        const uint32_t c = q[i - 1];
        if (c < SM_N && c == codes[p - 1]) continue;  // inside a run: its first cell is another lane's hit
      }
      ++seeds;
      scan_diagonal(q, qlen, codes + first, (long long) (off[s + 1] - first), (long long) (p - first) - i, s, o, best);
    }
  }
  seeds = wave_sum(seeds);
  const uint32_t run = wave_max(best.run);
  const unsigned long long H = wave_max(best.hi);
  const unsigned long long L = wave_max(best.hi == H ? best.lo : 0ull);
  const uint32_t winner = SM_SEQ - (uint32_t) ((H >> HI_SEQ) & SM_SEQ);
  // the best of the other sequences: a lane's best is its first entry unless that is the winner's
  const uint32_t other = wave_max(best.e1 && SM_SEQ - (best.e1 & SM_SEQ) == winner ? best.e2 : best.e1);
  if (lane != 0) return;
  struct bk_seq_hit v = {0, -1, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0};
  if (seeds)
  {
    const uint32_t i0 = 511u - (uint32_t) (L & 511u);
    v.found = 1;
    v.seq = (int32_t) winner;
    v.orient = 1u - (uint32_t) (H & 1u);
    v.score = (uint32_t) (H >> HI_SCORE);
    v.len = 511u - (uint32_t) ((H >> HI_LEN) & 511u);
    v.mism = (v.len - v.score) / 3u;
    v.run = run;
    v.q_start = v.orient ? (uint32_t) qlen - i0 - v.len : i0;
    v.s_start = SM_POS - (uint32_t) (L >> LO_START);
    v.n_seeds = seeds > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) seeds;
    if (other)
    {
      v.seq2 = (int32_t) (SM_SEQ - (other & SM_SEQ));
      v.score2 = other >> E_SCORE;
    }
  }
  res[kq] = v;
}
}  // namespace

void seqmatch_upload(const bk_seq_panel &panel, const struct bk_seq_probe *probes, uint64_t n, const uint8_t *query, uint32_t max_len, SeqmatchBufs &b, hipStream_t st)
{
  const uint64_t total = panel.n_seqs ? panel.off[panel.n_seqs] : 0;
  (void) upload(b.bases, panel.bases, total, st);
  b.d_off = upload(b.off, panel.off, panel.n_seqs ? panel.n_seqs + 1 : 0, st);
  b.d_probes = upload(b.probes, probes, n, st);
  b.d_query = upload(b.query, query, n * max_len, st);
}

uint64_t seqmatch_index(const bk_seq_panel &panel, uint32_t seed, SeqmatchBufs &b, hipStream_t st)
{
  const uint64_t total = panel.n_seqs ? panel.off[panel.n_seqs] : 0;  // (at most 2^28: the caller has checked)
  b.m = 0;
  b.ikeys = nullptr;
  b.ivals = nullptr;
  uint8_t *codes = b.codes.as<uint8_t>(total + 1);
  if (total == 0) return 0;
  uint32_t *flag = b.flag.as<uint32_t>(total + 1);
  hipLaunchKernelGGL(k_panel_flags, dim3(cdiv(total, 256)), dim3(256), 0, st, b.bases.get<uint8_t>(), b.d_off, (uint32_t) panel.n_seqs, (uint32_t) total, seed, codes, flag);
  prims::exclusive_scan<uint32_t>(flag, flag, total, b.scan_tmp, st);
  const uint64_t m = runs::read_u32(flag + total, st);
  if (m == 0) return 0;
  uint64_t *keys = b.keys.as<uint64_t>(m + 1);
  uint32_t *vals = b.vals.as<uint32_t>(m + 1);
  hipLaunchKernelGGL(k_panel_kmers, dim3(cdiv(total, 256)), dim3(256), 0, st, codes, flag, (uint32_t) total, seed, keys, vals);
  uint64_t *skeys;
  uint32_t *svals;
  prims::radix_sort_pairs(keys, vals, m, 0, 2 * (int) seed, b.rx, st, &skeys, &svals);
  b.ikeys = skeys;
  b.ivals = svals;
  b.m = m;
  return m;
}

void seqmatch_probes(const bk_seq_panel &panel, uint64_t n, uint32_t max_len, uint32_t seed, SeqmatchBufs &b, hipStream_t st, struct bk_seq_hit **res_out)
{
  static_assert(sizeof(struct bk_seq_probe) == 8 && sizeof(struct bk_seq_hit) == 48, "bk_seq_probe must be 8 bytes and bk_seq_hit 48");
  struct bk_seq_hit *res = b.res.as<struct bk_seq_hit>(n + 1);
  *res_out = res;
  if (n == 0) return;
  hipLaunchKernelGGL(k_seq_probes, dim3(cdiv(n, 4)), dim3(256), 0, st, b.codes.get<uint8_t>(), b.d_off, (uint32_t) panel.n_seqs, b.ikeys, b.ivals, (uint32_t) b.m, b.d_probes,
                     b.d_query, (uint32_t) n, max_len, seed, res);
}
