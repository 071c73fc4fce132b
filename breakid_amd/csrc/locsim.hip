// Locus similarity (bk_locus_similarity): the reference window around one breakpoint of a call searched in the window
// around the other, every diagonal in both orientations.  One wavefront per pair: it stages window A and both orientations of window B
// into LDS as bit planes (a low bit, a high bit and a valid bit per base, 64 bases to a word, as jfit.hip has them), deals the diagonals
// to its lanes, and a lane forms the match mask of a diagonal 64 columns at a time (window B's planes shifted to the diagonal, three
// XOR / OR and the valid planes) and walks it run by run for the best-scoring stretch and the longest run of matches.  No byte compares
// in the loop, no atomics, no float.
#include "locsim.h"

namespace
{
constexpr int LS_AW = 8;   // window A: at most 511 bases
constexpr int LS_BW = 10;  // window B: one empty word in front (a diagonal may start left of the window, on columns whose valid bit is
                           // zero), eight words of bases, one word behind for the shifted read
// the key that orders the candidates (include/breakid_hip.h): the score, then the shorter, orientation 0, the smaller |d|, d >= 0, the
// smaller start; 0 is "none", since a candidate has a score of 1 at least
constexpr int KEY_SCORE = 29, KEY_LEN = 20, KEY_ORIENT = 19, KEY_DIAG = 10, KEY_SIGN = 9;

struct WaveLds
{
  unsigned long long a[3][LS_AW], b[2][3][LS_BW];  // [0] low bit, [1] high bit, [2] valid; b[o]: bit 64 + j holds b_o[j]
};

// One diagonal: columns max(0, -d) .. min(L, L - d) - 1 of A against b_o[i + d].  Outside either window the valid planes are zero, so
// that the mask needs no column bounds: the zeros in front of the first column restart the sum, those behind the last one only lower it.
// The sum restarts where it is <= 0; the end of every run of ones offers (sum, length since the restart), and no other end can win.
__device__ __forceinline__ void scan_diagonal(const WaveLds &S, int o, int d, int L, unsigned long long &best, uint32_t &run)
{
  const int i_lo = d < 0 ? -d : 0, i_hi = d < 0 ? L - 1 : L - 1 - d;
  const unsigned long long rank = ((unsigned long long) (1 - o) << KEY_ORIENT) | ((unsigned long long) (511 - (d < 0 ? -d : d)) << KEY_DIAG) |
                                  ((unsigned long long) (d >= 0 ? 1 : 0) << KEY_SIGN);
  int sum = 0, len = 0, cur = 0;
  for (int w = i_lo >> 6; w <= (i_hi >> 6); ++w)
  {
    const uint32_t at = (uint32_t) (64 + w * 64 + d);  // bit of b_o under column 64 w: 1 .. 574
    unsigned long long m = ~((S.a[0][w] ^ window(S.b[o][0], at)) | (S.a[1][w] ^ window(S.b[o][1], at))) & S.a[2][w] & window(S.b[o][2], at);
    int done = 0;  // columns of the word behind us
    while (m)
    {
      const int zeros = __builtin_ctzll(m);
      if (zeros) sum -= 2 * zeros, len += zeros, cur = 0;
      m >>= zeros;
      const int ones = ~m ? __builtin_ctzll(~m) : 64;
      m = ones < 64 ? m >> ones : 0ull;
      done += zeros + ones;
      if (sum <= 0) sum = 0, len = 0;
      sum += ones, len += ones, cur += ones;
      run = (uint32_t) cur > run ? (uint32_t) cur : run;
      const int start = w * 64 + done - len;
      const unsigned long long key = ((unsigned long long) sum << KEY_SCORE) | ((unsigned long long) (511 - len) << KEY_LEN) | rank | (unsigned long long) (511 - start);
      best = key > best ? key : best;
    }
    if (done < 64) sum -= 2 * (64 - done), len += 64 - done, cur = 0;
  }
}

// One wavefront per pair, four to a workgroup.
__global__ __launch_bounds__(256) void k_locus_similarity(JfitRef ref, const struct bk_locus_pair *__restrict__ pairs, uint32_t n, int R, struct bk_locus_sim *__restrict__ res)
{
  __shared__ WaveLds lds[4];
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t k = blockIdx.x * 4 + wv;
  WaveLds &S = lds[wv];
  struct bk_locus_pair pr = {-1, 0, -1, 0};
  if (k < n) pr = pairs[k];
  const int L = 2 * R + 1, nw = (L + 63) >> 6;                 // (1 <= R <= 255 is checked on the host: L <= 511, nw <= 8)
  const bool live = k < n && pr.tid_a >= 0 && pr.tid_b >= 0;  // (the same on every lane of the wave)
  if (live)
  {
    // window A: bit i holds a[i]
    {
      const long long t = pr.tid_a, first = (long long) pr.pos_a - R;
      const long long g0 = seg_upper(ref, t, first - 1) - 1;
      for (int w = 0; w < LS_AW; ++w)
      {
        const int i = w * 64 + (int) lane;
        uint32_t code = CODE_N;
        if (w < nw && i < L) code = ref_code(ref, g0, t, first + i);  // (w < nw is wave-uniform: a word without a base is zero)
        const unsigned long long lo = __ballot(code & 1u), hi = __ballot(code & 2u), ok = __ballot(code < CODE_N);
        if (lane == 0) S.a[0][w] = lo, S.a[1][w] = hi, S.a[2][w] = ok;
      }
    }
    // window B as it lies and reverse-complemented
    {
      const long long t = pr.tid_b, first = (long long) pr.pos_b - R, last = (long long) pr.pos_b + R;
      const long long g0 = seg_upper(ref, t, first - 1) - 1;
      for (int w = 0; w < LS_BW; ++w)
      {
        const int j = (w - 1) * 64 + (int) lane;
        uint32_t fwd = CODE_N, rev = CODE_N;
        if (w >= 1 && w <= nw && j < L)
        {
          fwd = ref_code(ref, g0, t, first + j);
          rev = ref_code(ref, g0, t, last - j);
          if (rev < CODE_N) rev ^= 3u;
        }
        const unsigned long long lo = __ballot(fwd & 1u), hi = __ballot(fwd & 2u), ok = __ballot(fwd < CODE_N);
        const unsigned long long rlo = __ballot(rev & 1u), rhi = __ballot(rev & 2u), rok = __ballot(rev < CODE_N);
        if (lane == 0) S.b[0][0][w] = lo, S.b[0][1][w] = hi, S.b[0][2][w] = ok, S.b[1][0][w] = rlo, S.b[1][1][w] = rhi, S.b[1][2][w] = rok;
      }
    }
  }
  __syncthreads();
  if (!live)
  {
    if (k < n && lane == 0)
    {
      struct bk_locus_sim none = {0, 0, 0, 0, 0, 0, 0, 0};
      res[k] = none;
    }
    return;
  }
  // The 2 (2 L - 1) diagonals, dealt to the lanes in units of one length: unit x of an orientation is the diagonal x with the diagonal
  // x - L (L - x and x columns; unit 0 is the main diagonal alone), so that every unit walks L columns.
  const long long apart = (long long) pr.pos_a - (long long) pr.pos_b;
  const bool excluded = pr.tid_a == pr.tid_b && apart > -(long long) L && apart < (long long) L;  // orientation 0, d = apart: a base against itself
  unsigned long long best = 0;
  uint32_t run = 0;
  for (int u = (int) lane; u < 2 * L; u += 64)
  {
    const int o = u >= L ? 1 : 0, x = u - o * L;
    if (!(o == 0 && excluded && x == (int) apart)) scan_diagonal(S, o, x, L, best, run);
    if (x > 0 && !(o == 0 && excluded && x - L == (int) apart)) scan_diagonal(S, o, x - L, L, best, run);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
  {
    const unsigned long long ob = __shfl_xor(best, d, 64);
    const uint32_t orun = __shfl_xor(run, d, 64);
    best = ob > best ? ob : best;
    run = orun > run ? orun : run;
  }
  if (lane != 0) return;
  struct bk_locus_sim v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (best)
  {
    const int ad = 511 - (int) ((best >> KEY_DIAG) & 511u);
    v.score = (uint32_t) (best >> KEY_SCORE);
    v.len = 511u - (uint32_t) ((best >> KEY_LEN) & 511u);
    v.mism = (v.len - v.score) / 3u;
    v.run = run;
    v.diag = ((best >> KEY_SIGN) & 1u) ? ad : -ad;
    v.start = 511u - (uint32_t) (best & 511u);
    v.orient = 1u - (uint32_t) ((best >> KEY_ORIENT) & 1u);
    v.found = 1;
  }
  res[k] = v;
}
}  // namespace

void locsim_upload(const bk_refseq &ref, const struct bk_locus_pair *pairs, uint64_t n, LocsimBufs &b, hipStream_t st)
{
  refseq_upload(ref, b.ref, st);
  b.d_pairs = upload(b.pairs, pairs, n, st);
}

void locus_similarity(uint64_t n, uint32_t flank, LocsimBufs &b, hipStream_t st, struct bk_locus_sim **res_out)
{
  static_assert(sizeof(struct bk_locus_pair) == 16 && sizeof(struct bk_locus_sim) == 32, "bk_locus_pair must be 16 bytes and bk_locus_sim 32");
  struct bk_locus_sim *res = b.res.as<struct bk_locus_sim>(n + 1);
  *res_out = res;
  if (n == 0) return;
  hipLaunchKernelGGL(k_locus_similarity, dim3(cdiv(n, 4)), dim3(256), 0, st, b.ref.view, b.d_pairs, (uint32_t) n, (int) flank, res);
}
