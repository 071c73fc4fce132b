// Junction fit (bk_junction_fit): the voted sequence of a breakpoint side searched in the reference at the other side,
// every start offset x every insertion length.  One wavefront per probe: it stages the query and the two reference walks into LDS as
// bit planes (a low bit, a high bit and a valid bit per base, 64 bases to a word; the 2-bit code is A C G T = 0 1 2 3, so that the
// complement is ^ 3), deals the placements to its lanes, and a lane compares a placement 64 columns at a time: the walk's planes
// shifted to the diagonal, three XOR / OR, a column mask and a population count.  No byte compares in the loop, no atomics, no float.
#include "jfit.h"

namespace
{
constexpr int JF_QW = 4;  // query words: 256 columns
constexpr int JF_MW = 9;  // mate walk: one empty word in front (a diagonal may start left of the walk on columns the mask drops), at
                          // most 64 + 64 + 256 + 64 = 448 bases, one word behind for the shifted read
constexpr int JF_OW = 6;  // own walk: at most 64 + 256 = 320 bases, one word behind

struct WaveLds
{
  unsigned long long q[3][JF_QW], m[3][JF_MW], o[3][JF_OW];  // [0] low bit, [1] high bit, [2] valid
};

// One wavefront per probe, four to a workgroup.
__global__ __launch_bounds__(256) void k_junction_fit(JfitRef ref, const struct bk_junction_probe *__restrict__ probes, uint32_t n, const uint8_t *__restrict__ query,
                                                      uint32_t max_len, int S, int I, int H, struct bk_junction_fit *__restrict__ res)
{
  __shared__ WaveLds lds[4];
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t k = blockIdx.x * 4 + wv;
  WaveLds &L = lds[wv];
  struct bk_junction_probe pr = {-1, 0, 0, -1, 0, 0, 0, 0};
  if (k < n) pr = probes[k];
  const int qlen = (int) (pr.qlen < max_len ? pr.qlen : max_len);  // (qlen <= max_len is checked on the host: the bound keeps every index in range)
  const bool placed = k < n && qlen >= 1 && pr.tid_own >= 0 && pr.tid_mate >= 0;  // (the same on every lane of the wave)
  if (placed)
  {
    // the query
    for (int w = 0; w < JF_QW; ++w)
    {
      const int j = w * 64 + (int) lane;
      uint32_t code = CODE_N;
      if (j < qlen)
      {
        const uint8_t c = query[(uint64_t) k * max_len + (uint32_t) j];
        code = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : CODE_N;
      }
      const unsigned long long lo = __ballot(code & 1u), hi = __ballot(code & 2u), ok = __ballot(code < CODE_N);
      if (lane == 0) L.q[0][w] = lo, L.q[1][w] = hi, L.q[2][w] = ok;
    }
    // the mate walk: bit 64 + S + H + i holds M[i], i = -(S + H) .. qlen + S - 1
    {
      const long long t = pr.tid_mate, pos = pr.pos_mate;
      const bool fwd = pr.dir_mate == 1u, comp = pr.dir_own == pr.dir_mate;
      const int first = -(S + H), last = qlen + S - 1;
      const long long g0 = seg_upper(ref, t, (fwd ? pos + first : pos - last) - 1) - 1;
      for (int w = 0; w < JF_MW; ++w)
      {
        const int i = w * 64 + (int) lane - 64 + first;
        uint32_t code = CODE_N;
        if (w >= 1 && (w - 1) * 64 + first <= last)  // (wave-uniform: a word without a base of the walk is zero)
        {
          if (i <= last) code = ref_code(ref, g0, t, fwd ? pos + i : pos - i);
          if (comp && code < CODE_N) code ^= 3u;
        }
        const unsigned long long lo = __ballot(code & 1u), hi = __ballot(code & 2u), ok = __ballot(code < CODE_N);
        if (lane == 0) L.m[0][w] = lo, L.m[1][w] = hi, L.m[2][w] = ok;
      }
    }
    // the own walk: bit H + j holds O[j], j = -H .. qlen - 1
    {
      const long long t = pr.tid_own, pos = pr.pos_own;
      const bool left = pr.dir_own == 0u;
      const int first = -H, last = qlen - 1;
      const long long g0 = seg_upper(ref, t, (left ? pos + 1 + first : pos - 1 - last) - 1) - 1;
      for (int w = 0; w < JF_OW; ++w)
      {
        const int j = w * 64 + (int) lane + first;
        uint32_t code = CODE_N;
        if (w * 64 + first <= last && j <= last) code = ref_code(ref, g0, t, left ? pos + 1 + j : pos - 1 - j);
        const unsigned long long lo = __ballot(code & 1u), hi = __ballot(code & 2u), ok = __ballot(code < CODE_N);
        if (lane == 0) L.o[0][w] = lo, L.o[1][w] = hi, L.o[2][w] = ok;
      }
    }
  }
  __syncthreads();
  if (!placed)
  {
    if (k < n && lane == 0)
    {
      struct bk_junction_fit none = {0, 0, 0, 0, 0, 0, 0, 0};
      res[k] = none;
    }
    return;
  }
  // the placements, dealt to the lanes; the key orders them: the score, then the smaller ins, the smaller |shift|, shift >= 0 first
  const int imax = I < qlen - 1 ? I : qlen - 1;
  const int W = 2 * S + 1, P = (imax + 1) * W, nq = (qlen + 63) >> 6;
  unsigned long long best = 0;
  for (int pi = (int) lane; pi < P; pi += 64)
  {
    const int ins = pi / W, shift = pi % W - S;
    const uint32_t base = (uint32_t) (64 + S + H + shift - ins);  // bit of the walk under column 0 (>= 0: ins <= 64)
    int mism = 0;
    for (int w = 0; w < nq; ++w)
    {
      const unsigned long long cols = low_bits(qlen - w * 64) & ~low_bits(ins - w * 64);
      const uint32_t at = base + (uint32_t) w * 64u;
      const unsigned long long x = (L.q[0][w] ^ window(L.m[0], at)) | (L.q[1][w] ^ window(L.m[1], at)) | ~(L.q[2][w] & window(L.m[2], at));
      mism += __popcll(x & cols);
    }
    const int score = qlen - ins - 2 * mism;
    const uint32_t rank = ((uint32_t) ins << 8) | ((uint32_t) (shift < 0 ? -shift : shift) << 1) | (shift < 0 ? 1u : 0u);
    const unsigned long long key = ((unsigned long long) (uint32_t) (score + 1024) << 32) | (unsigned long long) (0xFFFFFFFFu - rank);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
  {
    const unsigned long long o = __shfl_xor(best, d, 64);
    best = o > best ? o : best;
  }
  if (lane != 0) return;
  const int score = (int) (uint32_t) (best >> 32) - 1024;
  const uint32_t rank = 0xFFFFFFFFu - (uint32_t) best;
  const int ins = (int) (rank >> 8), shift = (rank & 1u) ? -(int) ((rank >> 1) & 127u) : (int) ((rank >> 1) & 127u);
  struct bk_junction_fit v;
  v.shift = shift;
  v.ins = (uint32_t) ins;
  v.aligned = (uint32_t) (qlen - ins);
  v.mism = (uint32_t) ((qlen - ins - score) / 2);
  v.hom_fwd = v.hom_back = 0;
  v.score = score;
  v.placed = 1;
  if (ins == 0)
  {
    // forward: the leading columns where query, own walk and mate walk agree
    const uint32_t mbase = (uint32_t) (64 + S + H + shift);
    for (int w = 0; w < nq; ++w)
    {
      const uint32_t ma = mbase + (uint32_t) w * 64u, oa = (uint32_t) (H + w * 64);
      const unsigned long long ql = L.q[0][w], qh = L.q[1][w];
      const unsigned long long agree = ~((ql ^ window(L.m[0], ma)) | (qh ^ window(L.m[1], ma)) | (ql ^ window(L.o[0], oa)) | (qh ^ window(L.o[1], oa))) & L.q[2][w] &
                                       window(L.m[2], ma) & window(L.o[2], oa) & low_bits(qlen - w * 64);
      const int run = ~agree ? __ffsll((long long) ~agree) - 1 : 64;
      v.hom_fwd += (uint32_t) run;
      if (run < 64) break;
    }
    // backward: bit b of both windows is index b - H, so O[-1 - i] and M[shift - 1 - i] meet at bit H - 1 - i
    if (H > 0)
    {
      const uint32_t ma = (uint32_t) (64 + S + shift);  // (= 64 + S + H + shift - H)
      const unsigned long long agree = ~((L.o[0][0] ^ window(L.m[0], ma)) | (L.o[1][0] ^ window(L.m[1], ma))) & L.o[2][0] & window(L.m[2], ma) & low_bits(H);
      const unsigned long long top = agree << (64 - H);  // bit H - 1 at the top; the bits below it are zero and end the run
      v.hom_back = (uint32_t) (~top ? __clzll((long long) ~top) : 64);
    }
  }
  res[k] = v;
}

}  // namespace

void refseq_upload(const bk_refseq &ref, RefseqBufs &b, hipStream_t st)
{
  JfitRef &r = b.view;
  r = JfitRef{};
  r.n = (uint32_t) ref.n_segs;
  if (!ref.n_segs) return;
  r.tid = upload(b.tid, ref.tid, ref.n_segs, st);
  r.start = upload(b.start, ref.start, ref.n_segs, st);
  r.len = upload(b.len, ref.len, ref.n_segs, st);
  r.off = upload(b.off, ref.off, ref.n_segs + 1, st);
  r.bases = upload(b.bases, ref.bases, ref.off[ref.n_segs], st);
}

void jfit_upload(const bk_refseq &ref, const struct bk_junction_probe *probes, uint64_t n, const uint8_t *query, uint32_t max_len, JfitBufs &b, hipStream_t st)
{
  refseq_upload(ref, b.ref, st);
  b.d_probes = upload(b.probes, probes, n, st);
  b.d_query = upload(b.query, query, n * max_len, st);
}

void junction_fit(uint64_t n, uint32_t max_len, uint32_t max_shift, uint32_t max_ins, uint32_t max_hom, JfitBufs &b, hipStream_t st, struct bk_junction_fit **res_out)
{
  static_assert(sizeof(struct bk_junction_probe) == 32 && sizeof(struct bk_junction_fit) == 32, "bk_junction_probe and bk_junction_fit must be 32 bytes");
  struct bk_junction_fit *res = b.res.as<struct bk_junction_fit>(n + 1);
  *res_out = res;
  if (n == 0) return;
  hipLaunchKernelGGL(k_junction_fit, dim3(cdiv(n, 4)), dim3(256), 0, st, b.ref.view, b.d_probes, (uint32_t) n, b.d_query, max_len, (int) max_shift, (int) max_ins, (int) max_hom,
                     res);
}
