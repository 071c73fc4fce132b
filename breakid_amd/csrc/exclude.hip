// bk_exclude_regions on the device (include/breakid_hip.h): the record table without the records that overlap an excluded interval,
// stable and out of place.  gfx950 only; HBM-bound integer work.
//   k_exclude_classify  one lane per four consecutive records (tid, pos, flag, cigar_off as 16- / 8-byte loads): bam_endpos from the
//                       CIGAR words, a lower bound among the merged intervals of the record's contig, keep bits (one byte per lane)
//                       and the tile's kept records, CIGAR words and aux bytes
//   prims::exclusive_scan of the three per-tile counts: each tile's first output record, CIGAR word and aux byte
//   k_exclude_compact   the same tiles again: block scans place every kept record; the fixed columns are read as 16-byte vectors and
//                       written through an LDS stage as one contiguous run per column and tile; cigar_off / aux_off are rebuilt; the
//                       CIGAR words and aux bytes of the tile are copied by all 256 lanes over the tile's source span (coalesced on
//                       both sides, the words of excluded records are not read)
#include "exclude.h"
#include "prims.h"

namespace
{
constexpr int EX_V = 4;                   // consecutive records per lane
constexpr int EX_BLOCK = 256;
constexpr int EX_TILE = EX_BLOCK * EX_V;  // records per workgroup

// the first interval of the record's contig with end > pos decides: the record overlaps it iff it starts before bam_endpos
// (intervals before it end at or before pos, the ones behind it start behind its start)
__device__ __forceinline__ bool excluded(const ExclRegions &rg, int32_t tid, int32_t pos, uint16_t flag, const uint32_t *__restrict__ cigar, uint32_t c0, uint32_t c1)
{
  if (tid < 0 || tid >= rg.n_targets) return false;
  uint32_t lo = rg.off[tid], hi = rg.off[tid + 1];
  const uint32_t last = hi;
  while (lo < hi)
  {
    const uint32_t mid = (lo + hi) >> 1;
    if (rg.end[mid] > pos)
      hi = mid;
    else
      lo = mid + 1;
  }
  if (lo == last) return false;
  const int32_t b = rg.beg[lo];
  return b < pos || bam_endpos_hts(flag, pos, cigar, c0, c1) > b;  // (bam_endpos >= pos)
}

// four consecutive elements from i0 (m of them inside the table): one 16-byte access (two for 8-byte elements, one 8- or 4-byte access
// for the narrow columns) when the whole group is inside and the column is 16-byte aligned, else element by element
template <class T> struct alignas(sizeof(T) * EX_V > 16 ? 16 : sizeof(T) * EX_V) Vec4
{
  T e[EX_V];
};
template <class T> __device__ __forceinline__ void ld4(const T *__restrict__ p, uint64_t i0, uint32_t m, bool vec, T (&v)[EX_V])
{
  if (vec && m == EX_V)
  {
    const Vec4<T> x = *reinterpret_cast<const Vec4<T> *>(p + i0);
#pragma unroll
    for (int k = 0; k < EX_V; ++k) v[k] = x.e[k];
  }
  else
  {
#pragma unroll
    for (int k = 0; k < EX_V; ++k) v[k] = (uint32_t) k < m ? p[i0 + k] : (T) 0;
  }
}
// offset entries i0 .. i0 + 4 of a lane's group; entries behind the table's last record repeat off[n] (empty ranges)
__device__ __forceinline__ void ld_offs(const uint32_t *__restrict__ off, uint64_t i0, uint32_t m, uint32_t (&o)[EX_V + 1])
{
  if (m == EX_V)
  {
    const uint4 v = *reinterpret_cast<const uint4 *>(off + i0);
    o[0] = v.x;
    o[1] = v.y;
    o[2] = v.z;
    o[3] = v.w;
    o[4] = off[i0 + EX_V];
  }
  else
  {
#pragma unroll
    for (int k = 0; k <= EX_V; ++k) o[k] = off[i0 + ((uint32_t) k < m ? (uint32_t) k : m)];
  }
}

__global__ __launch_bounds__(EX_BLOCK) void k_exclude_classify(bk_soa s, ExclRegions rg, uint8_t *__restrict__ keep, uint32_t *__restrict__ counts, uint32_t stride)
{
  __shared__ uint32_t lds[prims::WAVES];
  const uint64_t q = (uint64_t) blockIdx.x * EX_BLOCK + threadIdx.x, i0 = q * EX_V;
  uint32_t nk = 0, nc = 0, na = 0;
  if (i0 < s.n)
  {
    const uint32_t m = (uint32_t) (s.n - i0 < EX_V ? s.n - i0 : EX_V);
    int32_t t[EX_V], p[EX_V];
    uint16_t f[EX_V];
    uint32_t c[EX_V + 1], a[EX_V + 1];
    ld4(s.tid, i0, m, true, t);
    ld4(s.pos, i0, m, true, p);
    ld4(s.flag, i0, m, true, f);
    ld_offs(s.cigar_off, i0, m, c);
    ld_offs(s.aux_off, i0, m, a);
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < EX_V; ++k)
      if ((uint32_t) k < m && !excluded(rg, t[k], p[k], f[k], s.cigar, c[k], c[k + 1]))
      {
        bits |= 1u << k;
        ++nk;
        nc += c[k + 1] - c[k];
        na += a[k + 1] - a[k];
      }
    keep[q] = (uint8_t) bits;
  }
  uint32_t tot;
  (void) prims::block_exclusive_scan(nk, lds, tot);
  if (threadIdx.x == 0) counts[blockIdx.x] = tot;
  (void) prims::block_exclusive_scan(nc, lds, tot);
  if (threadIdx.x == 0) counts[stride + blockIdx.x] = tot;
  (void) prims::block_exclusive_scan(na, lds, tot);
  if (threadIdx.x == 0) counts[2 * stride + blockIdx.x] = tot;
}

struct ExclDst
{
  int32_t *tid, *pos, *mtid, *mpos, *isize;
  uint16_t *flag;
  uint8_t *mapq;
  uint64_t *qhash;
  uint32_t *qcheck, *cigar_off, *cigar, *aux_off;
  uint8_t *aux;
};

// the kept values of one column of the tile, in record order, as one contiguous run: out[0 .. tk)
template <class T> __device__ __forceinline__ void put(uint64_t *stage, const T (&v)[EX_V], uint32_t bits, uint32_t xk, uint32_t tk, T *__restrict__ out)
{
  T *sg = reinterpret_cast<T *>(stage);
  __syncthreads();  // the stage's previous column is out
#pragma unroll
  for (int k = 0; k < EX_V; ++k)
    if (bits >> k & 1u) sg[xk++] = v[k];
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < tk; j += EX_BLOCK) out[j] = sg[j];
}

// the variable-length blob of the tile: source span [src[0], src[nloc]); element j belongs to the last record r with src[r] <= j and goes
// to dst[r] + (j - src[r]) when the record is kept (dst[r] != ~0)
template <class T>
__device__ __forceinline__ void copy_blob(const uint32_t *src, const uint32_t *dst, uint32_t nloc, const T *__restrict__ in, T *__restrict__ out)
{
  const uint64_t s1 = src[nloc];
  for (uint64_t j = (uint64_t) src[0] + threadIdx.x; j < s1; j += EX_BLOCK)
  {
    uint32_t lo = 0, hi = nloc;
    while (hi - lo > 1)
    {
      const uint32_t mid = (lo + hi) >> 1;
      if (src[mid] <= j)
        lo = mid;
      else
        hi = mid;
    }
    const uint32_t o = dst[lo];
    if (o != ~0u) out[o + (uint32_t) (j - src[lo])] = in[j];
  }
}

// VEC: mtid, mpos, qhash (and qcheck) are 16-byte aligned as well (bk_upload_records only demands it of the other columns)
template <bool VEC>
__global__ __launch_bounds__(EX_BLOCK) void k_exclude_compact(bk_soa s, ExclDst d, const uint8_t *__restrict__ keep, const uint32_t *__restrict__ first, uint32_t stride)
{
  __shared__ uint32_t lds[prims::WAVES];
  __shared__ uint32_t csrc[EX_TILE + 1], cdst[EX_TILE], asrc[EX_TILE + 1], adst[EX_TILE];
  __shared__ uint64_t stage[EX_TILE];
  const uint64_t base = (uint64_t) blockIdx.x * EX_TILE;
  const uint32_t nloc = (uint32_t) (s.n - base < EX_TILE ? s.n - base : EX_TILE);
  const uint64_t q = (uint64_t) blockIdx.x * EX_BLOCK + threadIdx.x, i0 = q * EX_V;
  const uint32_t m = i0 < s.n ? (uint32_t) (s.n - i0 < EX_V ? s.n - i0 : EX_V) : 0u;
  const uint32_t bits = m ? keep[q] : 0u;
  uint32_t c[EX_V + 1] = {}, a[EX_V + 1] = {};
  if (m)
  {
    ld_offs(s.cigar_off, i0, m, c);
    ld_offs(s.aux_off, i0, m, a);
  }
  uint32_t nk = 0, nc = 0, na = 0;
#pragma unroll
  for (int k = 0; k < EX_V; ++k)
    if (bits >> k & 1u)
    {
      ++nk;
      nc += c[k + 1] - c[k];
      na += a[k + 1] - a[k];
    }
  uint32_t tk, tc, ta;
  const uint32_t xk = prims::block_exclusive_scan(nk, lds, tk);
  const uint32_t xc = prims::block_exclusive_scan(nc, lds, tc);
  const uint32_t xa = prims::block_exclusive_scan(na, lds, ta);
  (void) tc;
  (void) ta;
  const uint64_t o_rec = first[blockIdx.x];
  // new cigar_off / aux_off of the kept records; the tile's source offsets and destinations for the blob copies
  uint32_t co[EX_V], ao[EX_V];
  uint32_t rc = first[stride + blockIdx.x] + xc, ra = first[2 * stride + blockIdx.x] + xa;
#pragma unroll
  for (int k = 0; k < EX_V; ++k)
  {
    const uint32_t r = threadIdx.x * EX_V + k;
    const bool kept = bits >> k & 1u;
    co[k] = rc;
    ao[k] = ra;
    if ((uint32_t) k < m)
    {
      csrc[r] = c[k];
      asrc[r] = a[k];
      cdst[r] = kept ? rc : ~0u;
      adst[r] = kept ? ra : ~0u;
    }
    if (kept)
    {
      rc += c[k + 1] - c[k];
      ra += a[k + 1] - a[k];
    }
  }
  if (m && threadIdx.x * EX_V + m == nloc)
  {
    csrc[nloc] = c[m];
    asrc[nloc] = a[m];
  }
  // fixed columns: only lanes with a kept record read theirs
  const uint32_t mm = bits ? m : 0u;
  int32_t tid[EX_V], pos[EX_V], mtid[EX_V], mpos[EX_V], isz[EX_V];
  uint16_t fl[EX_V];
  uint8_t mq[EX_V];
  uint64_t qh[EX_V];
  ld4(s.tid, i0, mm, true, tid);
  ld4(s.pos, i0, mm, true, pos);
  ld4(s.isize, i0, mm, true, isz);
  ld4(s.flag, i0, mm, true, fl);
  ld4(s.mapq, i0, mm, true, mq);
  ld4(s.mtid, i0, mm, VEC, mtid);
  ld4(s.mpos, i0, mm, VEC, mpos);
  ld4(s.qhash, i0, mm, VEC, qh);
  put(stage, tid, bits, xk, tk, d.tid + o_rec);
  put(stage, pos, bits, xk, tk, d.pos + o_rec);
  put(stage, mtid, bits, xk, tk, d.mtid + o_rec);
  put(stage, mpos, bits, xk, tk, d.mpos + o_rec);
  put(stage, isz, bits, xk, tk, d.isize + o_rec);
  put(stage, fl, bits, xk, tk, d.flag + o_rec);
  put(stage, mq, bits, xk, tk, d.mapq + o_rec);
  put(stage, qh, bits, xk, tk, d.qhash + o_rec);
  if (s.qcheck)
  {
    uint32_t qc[EX_V];
    ld4(s.qcheck, i0, mm, VEC, qc);
    put(stage, qc, bits, xk, tk, d.qcheck + o_rec);
  }
  put(stage, co, bits, xk, tk, d.cigar_off + o_rec);
  put(stage, ao, bits, xk, tk, d.aux_off + o_rec);
  __syncthreads();
  copy_blob(csrc, cdst, nloc, s.cigar, d.cigar);
  copy_blob(asrc, adst, nloc, s.aux, d.aux);
}

bool aligned16(const void *p) { return ((uintptr_t) p & 15u) == 0; }
}  // namespace

void exclude_compact(const bk_soa &s, const ExclRegions &rg, DevBuf dst[13], bk_soa &out, hipStream_t st,
                     const std::function<void(const char *, uint64_t, bool)> &tick)
{
  const uint64_t n = s.n;
  const uint32_t nb = cdiv(n, EX_TILE), stride = nb + 1;
  DevBuf keep, counts, tmp;
  uint8_t *kb = keep.as<uint8_t>(cdiv(n, EX_V) + 16);
  uint32_t *cnt = counts.as<uint32_t>(3ull * stride);
  // bytes: tid, pos, flag, cigar_off, aux_off of every record and the CIGAR words (those of a record whose answer needs bam_endpos:
  // credited in full), one keep byte per four records
  tick("k_exclude_classify", 18ull * n + 4ull * s.n_cigar_words + n / EX_V, true);
  if (nb) hipLaunchKernelGGL(k_exclude_classify, dim3(nb), dim3(EX_BLOCK), 0, st, s, rg, kb, cnt, stride);
  HIP_CHECK(hipGetLastError());
  tick(nullptr, 0, false);
  tick("exclude_scan", 3ull * 12ull * nb, true);
  for (int w = 0; w < 3; ++w) prims::exclusive_scan<uint32_t>(cnt + (uint64_t) w * stride, cnt + (uint64_t) w * stride, nb, tmp, st);
  tick(nullptr, 0, false);
  uint32_t tot[3];
  for (int w = 0; w < 3; ++w) HIP_CHECK(hipMemcpyAsync(&tot[w], cnt + (uint64_t) w * stride + nb, 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  const uint64_t m = tot[0], nc = tot[1], na = tot[2];
  const size_t bytes[13] = {m * 4, m * 4, m * 4, m * 4, m * 4, m * 2, m, m * 8, (m + 1) * 4, nc * 4, (m + 1) * 4, na, s.qcheck ? m * 4 : 0};
  void *p[13];
  for (int k = 0; k < 13; ++k) p[k] = dst[k].ensure(bytes[k] + 16);  // the layout of a device table: 16-byte aligned, 16-byte tail pad
  ExclDst d;
  d.tid = (int32_t *) p[0]; d.pos = (int32_t *) p[1]; d.mtid = (int32_t *) p[2]; d.mpos = (int32_t *) p[3]; d.isize = (int32_t *) p[4];
  d.flag = (uint16_t *) p[5]; d.mapq = (uint8_t *) p[6]; d.qhash = (uint64_t *) p[7]; d.cigar_off = (uint32_t *) p[8]; d.cigar = (uint32_t *) p[9];
  d.aux_off = (uint32_t *) p[10]; d.aux = (uint8_t *) p[11]; d.qcheck = s.qcheck ? (uint32_t *) p[12] : nullptr;
  const bool vec = aligned16(s.mtid) && aligned16(s.mpos) && aligned16(s.qhash) && (!s.qcheck || aligned16(s.qcheck));
  // bytes: keep bytes, both offset columns; the fixed columns of the kept records read and written (35 B, 39 with qcheck), their new offsets
  // written, their CIGAR words and aux bytes read and written
  const uint64_t fixed = s.qcheck ? 39 : 35;
  tick("k_exclude_compact", n / EX_V + 8ull * n + (2 * fixed + 8) * m + 8ull * nc + 2ull * na, true);
  if (nb)
  {
    if (vec)
      hipLaunchKernelGGL(k_exclude_compact<true>, dim3(nb), dim3(EX_BLOCK), 0, st, s, d, kb, cnt, stride);
    else
      hipLaunchKernelGGL(k_exclude_compact<false>, dim3(nb), dim3(EX_BLOCK), 0, st, s, d, kb, cnt, stride);
    HIP_CHECK(hipGetLastError());
  }
  // the end entries of the offset columns: the totals of the scans
  HIP_CHECK(hipMemcpyAsync(d.cigar_off + m, cnt + stride + nb, 4, hipMemcpyDeviceToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d.aux_off + m, cnt + 2ull * stride + nb, 4, hipMemcpyDeviceToDevice, st));
  tick(nullptr, 0, false);
  HIP_CHECK(hipStreamSynchronize(st));
  out = s;
  out.n = m;
  out.tid = d.tid; out.pos = d.pos; out.mtid = d.mtid; out.mpos = d.mpos; out.isize = d.isize; out.flag = d.flag; out.mapq = d.mapq; out.qhash = d.qhash;
  out.cigar_off = d.cigar_off; out.cigar = d.cigar; out.aux_off = d.aux_off; out.aux = d.aux; out.qcheck = d.qcheck;
  out.n_cigar_words = nc;
  out.n_aux_bytes = na;
  out.side = nullptr;
}
