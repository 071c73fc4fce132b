// A bk_refseq table on the device and how a kernel reads it: the upload of its columns, the lookup of ref(t, p) as a 2-bit code, and the
// shifted read of a bit plane.  Shared by jfit.hip (bk_junction_fit), locsim.hip (bk_locus_similarity) and seqcx.hip
// (bk_site_complexity, which also reads the raw nibble).
#pragma once
#include "bk_common.h"

// a bk_refseq table on the device (refseq_upload)
struct JfitRef
{
  uint32_t n = 0;
  const int32_t *tid = nullptr;
  const uint32_t *start = nullptr, *len = nullptr;
  const uint64_t *off = nullptr;
  const uint8_t *bases = nullptr;
};

// the columns of the table, uploaded per call
struct RefseqBufs
{
  DevBuf tid, start, len, off, bases;
  JfitRef view;
};

// `ref` is a host table that the caller has checked (include/breakid_hip.h: the segments ascend and do not overlap, every off span
// holds its bases); the copies are queued on `st` (defined in jfit.hip)
void refseq_upload(const bk_refseq &ref, RefseqBufs &b, hipStream_t st);

template <class T> const T *upload(DevBuf &b, const T *host, uint64_t count, hipStream_t st)
{
  T *d = b.as<T>(count + 1);
  if (count) HIP_CHECK(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, st));
  return d;
}

constexpr uint32_t CODE_N = 4;  // the 2-bit codes are A C G T = 0 1 2 3, so that the complement is ^ 3

// the segments in (tid, start) order: how many have a key <= (t, p0)
__device__ __forceinline__ long long seg_upper(const JfitRef &r, long long t, long long p0)
{
  uint32_t lo = 0, hi = r.n;
  while (lo < hi)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    const long long mt = r.tid[mid], ms = r.start[mid];
    if (mt < t || (mt == t && ms <= p0))
      lo = mid + 1;
    else
      hi = mid;
  }
  return (long long) lo;
}

// ref(t, p1) as a 2-bit code, CODE_N for N.  g0: the last segment whose key is <= the walk's lowest position (-1: none); the lane
// goes on from there over the segments that start at or before its own position.
__device__ __forceinline__ uint32_t ref_code(const JfitRef &r, long long g0, long long t, long long p1)
{
  const long long p0 = p1 - 1;
  if (p0 < 0) return CODE_N;
  long long g = g0;
  while (g + 1 < (long long) r.n)
  {
    const long long nt = r.tid[g + 1], ns = r.start[g + 1];
    if (nt < t || (nt == t && ns <= p0))
      ++g;
    else
      break;
  }
  if (g < 0 || (long long) r.tid[g] != t) return CODE_N;
  const long long i = p0 - (long long) r.start[g];
  if (i >= (long long) r.len[g]) return CODE_N;
  const uint32_t byte = r.bases[r.off[g] + (unsigned long long) (i >> 1)];
  const uint32_t nib = (i & 1) ? (byte & 15u) : (byte >> 4);
  if (nib & 4u) return CODE_N;                // 4..7 are N; bit 3 is the soft-mask
  return (0x87u >> ((nib & 3u) << 1)) & 3u;  // T C A G -> 3 1 0 2
}

constexpr uint32_t NIB_COVERED = 16;  // ref_nibble: a segment holds the position

// ref(t, p1) as it lies in the table: NIB_COVERED | the raw nibble (bit 3 the soft-mask, bit 2 N, the low bits T C A G) when a segment
// covers the position, 0 otherwise.  g0 and the walk as in ref_code.
__device__ __forceinline__ uint32_t ref_nibble(const JfitRef &r, long long g0, long long t, long long p1)
{
  const long long p0 = p1 - 1;
  if (p0 < 0) return 0;
  long long g = g0;
  while (g + 1 < (long long) r.n)
  {
    const long long nt = r.tid[g + 1], ns = r.start[g + 1];
    if (nt < t || (nt == t && ns <= p0))
      ++g;
    else
      break;
  }
  if (g < 0 || (long long) r.tid[g] != t) return 0;
  const long long i = p0 - (long long) r.start[g];
  if (i >= (long long) r.len[g]) return 0;
  const uint32_t byte = r.bases[r.off[g] + (unsigned long long) (i >> 1)];
  return NIB_COVERED | ((i & 1) ? (byte & 15u) : (byte >> 4));
}

// 64 bits of a plane from bit position `bit` on (the word behind the last one that holds data is there and is zero)
__device__ __forceinline__ unsigned long long window(const unsigned long long *plane, uint32_t bit)
{
  const uint32_t k = bit >> 6, r = bit & 63u;
  const unsigned long long a = plane[k] >> r;
  return r ? a | (plane[k + 1] << (64u - r)) : a;
}

__device__ __forceinline__ unsigned long long low_bits(int n)  // the n lowest bits, n clamped to 0..64
{
  return n <= 0 ? 0ull : n >= 64 ? ~0ull : (1ull << n) - 1ull;
}
