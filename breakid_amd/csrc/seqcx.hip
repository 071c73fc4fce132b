// Site complexity (bk_site_complexity): the reference window around one position described by itself: how much of it is
// soft-masked, its trinucleotide counts (DUST) and its exact tandem tracts.  One wavefront per site: it stages the window into LDS as
// five bit planes (covered, valid, masked and the two bits of a base, 64 columns to a word, as locsim.hip has them) and then uses its
// 64 lanes three ways: every lane popcounts the planes, lane t counts trinucleotide t, lane p - 1 walks the tracts of period p.  No
// byte compares, no atomics, no float.
#include "seqcx.h"
#include "wave.h"

namespace
{
constexpr int CX_W = 9;  // at most 511 columns: eight words and the zero word behind them that window() reads
enum { P_COV = 0, P_VAL = 1, P_MSK = 2, P_B0 = 3, P_B1 = 4, N_PLANES = 5 };
// the key that orders the tracts (include/breakid_hip.h): the longer, then the shorter period, then the smaller start; 0 is "none",
// since a tract has two columns at least
constexpr int KEY_LEN = 15, KEY_PERIOD = 9;

struct WaveLds
{
  unsigned long long p[N_PLANES][CX_W];  // bit i of a plane is column i
};

// the columns whose base has the 2-bit code c, 64 of them from column `at` on
__device__ __forceinline__ unsigned long long has_code(const WaveLds &S, uint32_t at, uint32_t c)
{
  const unsigned long long b0 = window(S.p[P_B0], at), b1 = window(S.p[P_B1], at);
  return window(S.p[P_VAL], at) & ((c & 1u) ? b0 : ~b0) & ((c & 2u) ? b1 : ~b1);
}

// The maximal run of masked columns through column R: the ones from R upwards, then those below R downwards.  Columns from L on are
// zero in every plane and so is the word behind the last, so that both walks end by themselves.
__device__ __forceinline__ uint32_t mask_run_at(const WaveLds &S, int R)
{
  const unsigned long long *m = S.p[P_MSK];
  if (!((m[R >> 6] >> (R & 63)) & 1ull)) return 0;
  uint32_t run = 0;
  for (int pos = R;;)
  {
    const unsigned long long x = ~window(m, (uint32_t) pos);
    const int ones = x ? __builtin_ctzll(x) : 64;
    run += (uint32_t) ones, pos += ones;
    if (ones < 64) break;
  }
  for (int pos = R; pos > 0;)
  {
    // the 64 columns that end at pos - 1, the last of them in bit 63 (below column 0: zeros)
    const unsigned long long x = ~(pos >= 64 ? window(m, (uint32_t) (pos - 64)) : m[0] << (64 - pos));
    const int ones = x ? __builtin_clzll(x) : 64;
    run += (uint32_t) ones, pos -= ones;
    if (ones < 64) break;
  }
  return run;
}

// The columns at which triplet t = 16 w[i] + 4 w[i + 1] + w[i + 2] starts.  Columns from L on are not valid, so that no start beyond
// L - 3 passes.
__device__ __forceinline__ uint32_t count_triplet(const WaveLds &S, uint32_t t, int nw)
{
  uint32_t c_t = 0;
  for (int w = 0; w < nw; ++w)
  {
    const uint32_t at = (uint32_t) w * 64u;
    c_t += (uint32_t) __popcll(has_code(S, at, t >> 4) & has_code(S, at + 1, (t >> 2) & 3u) & has_code(S, at + 2, t & 3u));
  }
  return c_t;
}

// The tracts of period p: m_p, the columns that equal the column p further on, is walked run by run; a run is carried over the word
// boundaries and offered where it ends.  Column i + p >= L is not valid, so that m_p ends at L - p by itself.  best: the first tract of
// this period in the contract's order, best_bp: the first that holds one of the columns R - 1 .. R + 1.
__device__ __forceinline__ void walk_tracts(const WaveLds &S, int p, int R, int nw, uint32_t &best, uint32_t &best_bp)
{
  int run = 0, start = 0;
  auto flush = [&]() {
    if (run >= p)
    {
      const int len = run + p;
      const uint32_t key = ((uint32_t) len << KEY_LEN) | ((uint32_t) (64 - p) << KEY_PERIOD) | (uint32_t) (511 - start);
      best = key > best ? key : best;
      if (start <= R + 1 && start + len - 1 >= R - 1) best_bp = key > best_bp ? key : best_bp;
    }
    run = 0;
  };
  for (int w = 0; w < nw; ++w)
  {
    const uint32_t at = (uint32_t) (w * 64 + p);  // at most 7 * 64 + 64: word 8 and nothing behind it
    const unsigned long long m = S.p[P_VAL][w] & window(S.p[P_VAL], at) & ~((S.p[P_B0][w] ^ window(S.p[P_B0], at)) | (S.p[P_B1][w] ^ window(S.p[P_B1], at)));
    int done = 0;  // columns of the word behind us
    while (done < 64)
    {
      unsigned long long rest = m >> done;
      if (!rest)
      {
        flush();
        break;
      }
      const int zeros = __builtin_ctzll(rest);
      if (zeros) flush(), done += zeros, rest >>= zeros;
      const int ones = ~rest ? __builtin_ctzll(~rest) : 64;  // (the bits shifted in are zeros: at most 64 - done)
      if (run == 0) start = w * 64 + done;
      run += ones, done += ones;
    }
  }
  flush();
}

// One wavefront per site, four to a workgroup.
__global__ __launch_bounds__(256) void k_site_complexity(JfitRef ref, const struct bk_ref_site *__restrict__ sites, uint32_t n, int R, int max_period,
                                                         struct bk_site_cplx *__restrict__ res)
{
  __shared__ WaveLds lds[4];
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t k = blockIdx.x * 4 + wv;
  WaveLds &S = lds[wv];
  struct bk_ref_site site = {-1, 0};
  if (k < n) site = sites[k];
  const int L = 2 * R + 1, nw = (L + 63) >> 6;  // (1 <= R <= 255 is checked on the host: L <= 511, nw <= 8)
  const bool live = k < n && site.tid >= 0;    // (the same on every lane of the wave)
  if (live)
  {
    const long long t = site.tid, first = (long long) site.pos - R;
    const long long g0 = seg_upper(ref, t, first - 1) - 1;
    for (int w = 0; w < CX_W; ++w)
    {
      const int i = w * 64 + (int) lane;
      uint32_t nib = 0;
      if (w < nw && i < L) nib = ref_nibble(ref, g0, t, first + i);  // (w < nw is wave-uniform: a word without a column is zero)
      const bool valid = (nib & NIB_COVERED) && !(nib & 4u);
      const uint32_t code = valid ? (0x87u >> ((nib & 3u) << 1)) & 3u : 0u;  // T C A G -> 3 1 0 2
      const unsigned long long cov = __ballot(nib & NIB_COVERED), val = __ballot(valid), msk = __ballot((nib & NIB_COVERED) && (nib & 8u));
      const unsigned long long b0 = __ballot(code & 1u), b1 = __ballot(code & 2u);
      if (lane == 0) S.p[P_COV][w] = cov, S.p[P_VAL][w] = val, S.p[P_MSK][w] = msk, S.p[P_B0][w] = b0, S.p[P_B1][w] = b1;
    }
  }
  __syncthreads();
  if (!live)
  {
    if (k < n && lane == 0)
    {
      struct bk_site_cplx none = {};
      res[k] = none;
    }
    return;
  }
  // the counts: every lane adds up the same words
  uint32_t covered = 0, valid = 0, gc = 0, masked = 0;
  for (int w = 0; w < nw; ++w)
  {
    covered += (uint32_t) __popcll(S.p[P_COV][w]);
    valid += (uint32_t) __popcll(S.p[P_VAL][w]);
    masked += (uint32_t) __popcll(S.p[P_MSK][w]);
    gc += (uint32_t) __popcll(S.p[P_B0][w] ^ S.p[P_B1][w]);  // C = 1 and G = 2; a column without a base has both bits zero
  }
  const uint32_t mask_run = mask_run_at(S, R);

  // trinucleotides: lane t counts the columns at which triplet t starts
  const uint32_t c_t = count_triplet(S, lane, nw);
  const uint32_t tri_total = wave_sum(c_t), tri_pairs = wave_sum(c_t * (c_t - 1u) / 2u);
  const uint32_t tri_distinct = (uint32_t) __popcll(__ballot(c_t > 0));

  // tandem tracts: lane p - 1 walks the tracts of period p
  const int p = (int) lane + 1;
  uint32_t best = 0, best_bp = 0;
  if (p <= max_period && p < L) walk_tracts(S, p, R, nw, best, best_bp);
  best = wave_max(best);
  best_bp = wave_max(best_bp);
  if (lane != 0) return;
  struct bk_site_cplx v = {};
  v.covered = covered, v.valid = valid, v.gc = gc, v.masked = masked, v.mask_run = mask_run;
  v.tri_total = tri_total, v.tri_pairs = tri_pairs, v.tri_distinct = tri_distinct;
  if (best_bp) v.bp_period = 64u - ((best_bp >> KEY_PERIOD) & 63u), v.bp_len = best_bp >> KEY_LEN, v.bp_start = 511u - (best_bp & 511u);
  if (best) v.max_period = 64u - ((best >> KEY_PERIOD) & 63u), v.max_len = best >> KEY_LEN, v.max_start = 511u - (best & 511u);
  res[k] = v;
}
}  // namespace

void seqcx_upload(const bk_refseq &ref, const struct bk_ref_site *sites, uint64_t n, SeqcxBufs &b, hipStream_t st)
{
  refseq_upload(ref, b.ref, st);
  b.d_sites = upload(b.sites, sites, n, st);
}

void site_complexity(uint64_t n, uint32_t flank, uint32_t max_period, SeqcxBufs &b, hipStream_t st, struct bk_site_cplx **res_out)
{
  static_assert(sizeof(struct bk_ref_site) == 8 && sizeof(struct bk_site_cplx) == 64, "bk_ref_site must be 8 bytes and bk_site_cplx 64");
  struct bk_site_cplx *res = b.res.as<struct bk_site_cplx>(n + 1);
  *res_out = res;
  if (n == 0) return;
  hipLaunchKernelGGL(k_site_complexity, dim3(cdiv(n, 4)), dim3(256), 0, st, b.ref.view, b.d_sites, (uint32_t) n, (int) flank, (int) max_period, res);
}
