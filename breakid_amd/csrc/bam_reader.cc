// Host feed: BGZF/BAM decoder -> pinned columnar record table (include/breakid_hip.h: bk_soa).
// Own implementation (zlib inflate only); replaces the htslib reader the reference uses for its two
// sequential passes (BreakID.cc:1414 samread, :1929 sam_read1).  Record layout: SAM spec §4.2 /
// htslib/sam.h:148-181; aux walk as sam.c:1267-1279 (bam_aux_get).
//
// BGZF blocks are independent deflate streams and BAM records are self-delimiting, so both stages run on all host
// cores: (1) block headers are hopped sequentially (18 bytes each), the blocks are inflated in parallel into one
// buffer; (2) record starts are hopped sequentially (4 bytes each) into checkpoints every CHUNK records, the
// chunks are decoded in parallel straight into the fixed-width columns, CIGAR words / aux blobs go through
// chunk-local buffers and are placed by a prefix sum.  Columns live in pinned host memory (hipHostMalloc) when a
// GPU is present, so bk_upload_records(BK_MEM_HOST) runs at PCIe speed.  BREAKID_THREADS overrides the thread count.
#include <hip/hip_runtime_api.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <ctime>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "bk_debug.h"
#include <thread>
#include <unistd.h>
#include <unordered_map>
#include <vector>

#include "../../include/breakid_hip.h"
#include "bk_hash.h"

namespace
{
struct HostBuf
{
  void *p = nullptr;
  bool pinned = false;
  size_t bytes = 0;
  HostBuf() = default;
  HostBuf(const HostBuf &) = delete;
  HostBuf &operator=(const HostBuf &) = delete;
  ~HostBuf() { release(); }
  void release()
  {
    if (!p) return;
    if (pinned)
      (void) hipHostFree(p);
    else
      free(p);
    p = nullptr;
    bytes = 0;
  }
  // pinned when the HIP runtime has a device; plain memory otherwise (the decoder itself is host code)
  bool alloc(size_t n, bool want_pinned)
  {
    release();
    if (n == 0) n = 16;
    if (want_pinned && hipHostMalloc(&p, n, hipHostMallocDefault) == hipSuccess && p)
    {
      pinned = true;
      bytes = n;
      return true;
    }
    (void) hipGetLastError();
    p = malloc(n);
    pinned = false;
    bytes = p ? n : 0;
    return p != nullptr;
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

unsigned n_threads()
{
  if (const char *e = getenv("BREAKID_THREADS"))
  {
    int v = atoi(e);
    if (v > 0) return (unsigned) v;
  }
  unsigned h = std::thread::hardware_concurrency();
  if (h == 0) h = 4;
  return h > 64 ? 64 : h;
}

// dynamic scheduling over [0, njobs): fn(job) on up to nt threads
template <class F> void parallel_for(size_t njobs, unsigned nt, F fn)
{
  if (njobs == 0) return;
  if (nt > njobs) nt = (unsigned) njobs;
  if (nt <= 1)
  {
    for (size_t j = 0; j < njobs; ++j) fn(j);
    return;
  }
  std::atomic<size_t> next{0};
  std::vector<std::thread> th;
  th.reserve(nt);
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([&]() {
      for (;;)
      {
        size_t j = next.fetch_add(1);
        if (j >= njobs) break;
        fn(j);
      }
    });
  for (auto &t : th) t.join();
}
}  // namespace

struct bk_bam
{
  std::string path;
  std::vector<uint8_t> data;  // inflated stream
  size_t rec_begin = 0;
  std::vector<std::string> names;
  std::vector<const char *> name_ptrs;
  std::vector<uint32_t> lens;
  // decoded columns
  HostBuf tid, pos, mtid, mpos, isize, flag, mapq, qhash, qcheck, cigar_off, cigar, aux_off, aux;
  double t_inflate_s = 0, t_decode_s = 0;
};

extern "C" uint64_t bk_qname_hash(const char *name, size_t len)
{
  uint64_t h = 0xCBF29CE484222325ull;
  for (size_t i = 0; i < len; ++i)
  {
    h ^= (unsigned char) name[i];
    h *= 0x100000001B3ull;
  }
  h ^= h >> 30;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 27;
  h *= 0x94D049BB133111EBull;
  h ^= h >> 31;
  return h;
}

extern "C" uint32_t bk_qname_check(const char *name, size_t len) { return qname_check32((const uint8_t *) name, (uint32_t) len); }

namespace
{
void set_err(char *err, size_t errlen, const std::string &m)
{
  if (err && errlen) snprintf(err, errlen, "%s", m.c_str());
}
inline uint32_t rd32(const uint8_t *p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24); }
inline uint16_t rd16(const uint8_t *p) { return (uint16_t) (p[0] | (p[1] << 8)); }

struct Block
{
  size_t in_off, clen, out_off;
  uint32_t isize;
};

bool inflate_all(const std::vector<uint8_t> &file, std::vector<uint8_t> &out, std::string &why)
{
  // pass 1: hop over the block headers
  std::vector<Block> blocks;
  size_t off = 0, total = 0;
  while (off < file.size())
  {
    if (off + 18 > file.size())
    {
      why = "truncated BGZF header";
      return false;
    }
    const uint8_t *h = file.data() + off;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4))
    {
      why = "not a BGZF block";
      return false;
    }
    uint16_t xlen = rd16(h + 10);
    if (off + 12 + (size_t) xlen > file.size())
    {
      why = "truncated BGZF header";
      return false;
    }
    const uint8_t *x = h + 12;
    int bsize = -1;
    for (size_t k = 0; k + 4 <= xlen;)
    {
      uint16_t slen = rd16(x + k + 2);
      if (x[k] == 66 && x[k + 1] == 67 && slen == 2 && k + 6 <= xlen) bsize = rd16(x + k + 4);
      k += 4 + (size_t) slen;
    }
    if (bsize < 0 || off + (size_t) bsize + 1 > file.size() || (size_t) bsize + 1 < 12 + (size_t) xlen + 8)
    {
      why = "bad BGZF block size";
      return false;
    }
    Block b;
    b.in_off = off + 12 + xlen;
    b.clen = (size_t) bsize + 1 - (12 + (size_t) xlen) - 8;
    b.isize = rd32(h + bsize + 1 - 4);
    if (b.isize > 65536u)  // BGZF: a block inflates to at most 64 KiB (bgzf.h BGZF_MAX_BLOCK_SIZE); same check as the GPU scanner
    {
      why = "BGZF block claims more than 64 KiB of data";
      return false;
    }
    b.out_off = total;
    total += b.isize;
    blocks.push_back(b);
    off += (size_t) bsize + 1;
  }
  out.assign(total, 0);
  // pass 2: independent deflate streams
  std::atomic<int> bad{0};
  parallel_for(blocks.size(), n_threads(), [&](size_t j) {
    const Block &b = blocks[j];
    if (!b.isize) return;
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK)
    {
      bad = 1;
      return;
    }
    zs.next_in = const_cast<Bytef *>(file.data() + b.in_off);
    zs.avail_in = (uInt) b.clen;
    zs.next_out = out.data() + b.out_off;
    zs.avail_out = b.isize;
    int rc = inflate(&zs, Z_FINISH);
    inflateEnd(&zs);
    if (rc != Z_STREAM_END) bad = 2;
  });
  if (bad)
  {
    why = bad == 1 ? "inflateInit2 failed" : "inflate failed";
    return false;
  }
  return true;
}

double now_s()
{
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + ts.tv_nsec * 1e-9;
}
}  // namespace

static int bam_open_impl(const char *path, bk_bam **out, char *err, size_t errlen)
{
  if (!path || !out) return BK_ERR_ARG;
  *out = nullptr;
  FILE *f = fopen(path, "rb");
  if (!f)
  {
    set_err(err, errlen, std::string("cannot open ") + path);
    return BK_ERR_IO;
  }
  std::vector<uint8_t> file;
  fseek(f, 0, SEEK_END);
  long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  file.resize(sz > 0 ? (size_t) sz : 0);
  if (sz > 0 && fread(file.data(), 1, (size_t) sz, f) != (size_t) sz)
  {
    fclose(f);
    set_err(err, errlen, "short read");
    return BK_ERR_IO;
  }
  fclose(f);
  std::unique_ptr<bk_bam> guard(new bk_bam());  // freed on every error return and on an exception
  bk_bam *b = guard.get();
  b->path = path;
  std::string why;
  const double t0 = now_s();
  if (!inflate_all(file, b->data, why))
  {
    set_err(err, errlen, why);
    return BK_ERR_IO;
  }
  b->t_inflate_s = now_s() - t0;
  std::vector<uint8_t>().swap(file);
  const std::vector<uint8_t> &d = b->data;
  if (d.size() < 12 || memcmp(d.data(), "BAM\1", 4) != 0)
  {
    set_err(err, errlen, "not a BAM file");
    return BK_ERR_IO;
  }
  size_t p = 4;
  uint32_t l_text = rd32(d.data() + p);
  p += 4 + (size_t) l_text;
  if (p + 4 > d.size())
  {
    set_err(err, errlen, "truncated BAM header");
    return BK_ERR_IO;
  }
  uint32_t n_ref = rd32(d.data() + p);
  p += 4;
  for (uint32_t i = 0; i < n_ref; ++i)
  {
    if (p + 4 > d.size()) { set_err(err, errlen, "truncated BAM header"); return BK_ERR_IO; }
    uint32_t l_name = rd32(d.data() + p);
    p += 4;
    if (p + l_name + 4 > d.size()) { set_err(err, errlen, "truncated BAM header"); return BK_ERR_IO; }
    b->names.emplace_back((const char *) d.data() + p, l_name ? l_name - 1 : 0);
    p += l_name;
    b->lens.push_back(rd32(d.data() + p));
    p += 4;
  }
  for (auto &s : b->names) b->name_ptrs.push_back(s.c_str());
  b->rec_begin = p;
  *out = guard.release();
  return BK_OK;
}

extern "C" int bk_bam_header(const bk_bam *b, int *n_targets, const char *const **names, const uint32_t **lens)
{
  if (!b) return BK_ERR_ARG;
  if (n_targets) *n_targets = (int) b->names.size();
  if (names) *names = b->name_ptrs.data();
  if (lens) *lens = b->lens.data();
  return BK_OK;
}

namespace
{
constexpr size_t CHUNK = 1 << 16;  // records per decode job

struct ChunkOut
{
  std::vector<uint32_t> cigar;
  std::vector<uint8_t> aux;
  uint64_t cigar_base = 0, aux_base = 0;
  int bad = 0;
};

struct Cols
{
  int32_t *tid, *pos, *mtid, *mpos, *isize;
  uint16_t *flag;
  uint8_t *mapq;
  uint64_t *qhash;
  uint32_t *qcheck;
  uint32_t *cigar_off, *aux_off;  // chunk-local offsets first, rebased in the placement pass
};

// decode records [r0, r1) starting at byte offset p of the inflated stream
void decode_chunk(const uint8_t *d, size_t dsize, size_t p, size_t r0, size_t r1, const Cols &c, ChunkOut &o)
{
  for (size_t i = r0; i < r1; ++i)
  {
    uint32_t bs = rd32(d + p);
    p += 4;
    const uint8_t *r = d + p;
    uint8_t l_name = r[8];
    uint16_t n_cig = rd16(r + 12);
    uint32_t l_seq = rd32(r + 16);
    size_t q = 32;
    size_t need = q + l_name + (size_t) n_cig * 4 + ((size_t) l_seq + 1) / 2 + l_seq;
    if (need > bs || p + bs > dsize)
    {
      o.bad = 1;
      return;
    }
    c.tid[i] = (int32_t) rd32(r);
    c.pos[i] = (int32_t) rd32(r + 4);
    c.mapq[i] = r[9];
    c.flag[i] = rd16(r + 14);
    c.mtid[i] = (int32_t) rd32(r + 20);
    c.mpos[i] = (int32_t) rd32(r + 24);
    c.isize[i] = (int32_t) rd32(r + 28);
    size_t qn = l_name ? strnlen((const char *) r + q, l_name) : 0;  // bam_get_qname is a C string
    c.qhash[i] = bk_qname_hash((const char *) r + q, qn);
    c.qcheck[i] = bk_qname_check((const char *) r + q, qn);
    q += l_name;
    c.cigar_off[i] = (uint32_t) o.cigar.size();
    for (uint16_t k = 0; k < n_cig; ++k) o.cigar.push_back(rd32(r + q + 4 * (size_t) k));
    q += (size_t) n_cig * 4 + ((size_t) l_seq + 1) / 2 + l_seq;
    // aux walk, the same rule as aux_scan in bam_gpu.hip (sam.c bam_aux_get / skip_aux, BamAlignment.cc saTag / originCigar):
    // the FIRST field named SA (OC) is the one that counts, whatever its type, and its text is the C string that starts behind
    // its type byte (cut at the end of the record); an empty one still hides every later field of that name.  Fields are
    // skipped by type: A c C 1, s S 2, i I f 4, d 8 bytes, Z H up to and with the NUL, B 5 + count elements of 1 (c C),
    // 2 (s S), 4 (i I f) or 8 (d) bytes.  The walk ends at a type or element type outside these (htslib aborts or goes astray).
    const uint8_t *sa = nullptr, *oc = nullptr;
    size_t sa_len = 0, oc_len = 0;
    while (q + 3 <= bs)
    {
      const uint8_t *tag = r + q;
      uint8_t type = r[q + 2];
      q += 3;
      const bool is_sa = !sa && tag[0] == 'S' && tag[1] == 'A', is_oc = !oc && tag[0] == 'O' && tag[1] == 'C';
      if (is_sa || is_oc)
      {
        size_t e = q;
        while (e < bs && r[e]) ++e;
        if (is_sa) { sa = r + q; sa_len = e - q; }
        else { oc = r + q; oc_len = e - q; }
      }
      size_t len = 0;
      switch (type)
      {
      case 'A': case 'c': case 'C': len = 1; break;
      case 's': case 'S': len = 2; break;
      case 'i': case 'I': case 'f': len = 4; break;
      case 'd': len = 8; break;
      case 'Z': case 'H':
      {
        size_t e = q;
        while (e < bs && r[e]) ++e;
        len = e - q + 1;
        break;
      }
      case 'B':
      {
        if (q + 5 > bs) { q = bs; continue; }
        uint8_t sub = r[q];
        uint32_t cnt = rd32(r + q + 1);
        size_t es = 0;
        switch (sub)
        {
        case 'c': case 'C': es = 1; break;
        case 's': case 'S': es = 2; break;
        case 'i': case 'I': case 'f': es = 4; break;
        case 'd': es = 8; break;
        }
        if (!es) { q = bs; continue; }
        len = 5 + (size_t) cnt * es;
        break;
      }
      default:
        q = bs;
        continue;
      }
      q += len;
    }
    c.aux_off[i] = (uint32_t) o.aux.size();
    if (sa && sa_len)
    {
      if (oc && oc_len)
      {
        o.aux.insert(o.aux.end(), oc, oc + oc_len);
        o.aux.push_back('\t');
      }
      o.aux.insert(o.aux.end(), sa, sa + sa_len);
    }
    p += bs;
  }
}
}  // namespace

static int bam_decode_impl(bk_bam *b, bk_soa *out, char *err, size_t errlen)
{
  if (!b || !out) return BK_ERR_ARG;
  const double t0 = now_s();
  const std::vector<uint8_t> &dv = b->data;
  const uint8_t *d = dv.data();
  const size_t dsize = dv.size();
  // pass 1: record starts, one checkpoint per CHUNK records
  std::vector<size_t> ckpt;
  size_t n = 0, p = b->rec_begin;
  while (p + 4 <= dsize)
  {
    uint32_t bs = rd32(d + p);
    if (bs < 32 || p + 4 + (size_t) bs > dsize)
    {
      set_err(err, errlen, "truncated BAM record");
      return BK_ERR_IO;
    }
    if (n % CHUNK == 0) ckpt.push_back(p);
    ++n;
    p += 4 + (size_t) bs;
  }
  if (n >= 0xFFFFFFF0ull)
  {
    set_err(err, errlen, "more than 2^32 records in one BAM");
    return BK_ERR_LIMIT;
  }
  int ndev = 0;
  const bool pin = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
  (void) hipGetLastError();
  bool ok = b->tid.alloc(n * 4, pin) && b->pos.alloc(n * 4, pin) && b->mtid.alloc(n * 4, pin) && b->mpos.alloc(n * 4, pin) && b->isize.alloc(n * 4, pin) &&
            b->flag.alloc(n * 2, pin) && b->mapq.alloc(n, pin) && b->qhash.alloc(n * 8, pin) && b->qcheck.alloc(n * 4, pin) && b->cigar_off.alloc((n + 1) * 4, pin) && b->aux_off.alloc((n + 1) * 4, pin);
  if (!ok)
  {
    set_err(err, errlen, "out of host memory for the record table");
    return BK_ERR_IO;
  }
  Cols c{b->tid.as<int32_t>(), b->pos.as<int32_t>(), b->mtid.as<int32_t>(), b->mpos.as<int32_t>(), b->isize.as<int32_t>(), b->flag.as<uint16_t>(),
         b->mapq.as<uint8_t>(), b->qhash.as<uint64_t>(), b->qcheck.as<uint32_t>(), b->cigar_off.as<uint32_t>(), b->aux_off.as<uint32_t>()};
  // pass 2: chunks in parallel
  const size_t nchunks = ckpt.size();
  std::vector<ChunkOut> co(nchunks);
  const unsigned nt = n_threads();
  parallel_for(nchunks, nt, [&](size_t j) {
    const size_t r0 = j * CHUNK, r1 = (r0 + CHUNK < n) ? r0 + CHUNK : n;
    decode_chunk(d, dsize, ckpt[j], r0, r1, c, co[j]);
  });
  uint64_t ncig = 0, naux = 0;
  for (size_t j = 0; j < nchunks; ++j)
  {
    if (co[j].bad)
    {
      set_err(err, errlen, "corrupt BAM record");
      return BK_ERR_IO;
    }
    co[j].cigar_base = ncig;
    co[j].aux_base = naux;
    ncig += co[j].cigar.size();
    naux += co[j].aux.size();
  }
  if (ncig >= 0xFFFFFFF0ull || naux >= 0xFFFFFFF0ull)
  {
    set_err(err, errlen, "CIGAR / SA columns exceed 32-bit offsets");
    return BK_ERR_LIMIT;
  }
  if (!b->cigar.alloc((ncig ? ncig : 1) * 4, pin) || !b->aux.alloc(naux ? naux : 1, pin))
  {
    set_err(err, errlen, "out of host memory for the record table");
    return BK_ERR_IO;
  }
  uint32_t *cig = b->cigar.as<uint32_t>();
  uint8_t *aux = b->aux.as<uint8_t>();
  if (!ncig) cig[0] = 0;
  if (!naux) aux[0] = 0;
  // pass 3: place the variable-length columns, rebase the offsets
  parallel_for(nchunks, nt, [&](size_t j) {
    const size_t r0 = j * CHUNK, r1 = (r0 + CHUNK < n) ? r0 + CHUNK : n;
    ChunkOut &o = co[j];
    if (!o.cigar.empty()) memcpy(cig + o.cigar_base, o.cigar.data(), o.cigar.size() * 4);
    if (!o.aux.empty()) memcpy(aux + o.aux_base, o.aux.data(), o.aux.size());
    const uint32_t cb = (uint32_t) o.cigar_base, ab = (uint32_t) o.aux_base;
    for (size_t i = r0; i < r1; ++i)
    {
      c.cigar_off[i] += cb;
      c.aux_off[i] += ab;
    }
    std::vector<uint32_t>().swap(o.cigar);
    std::vector<uint8_t>().swap(o.aux);
  });
  c.cigar_off[n] = (uint32_t) ncig;
  c.aux_off[n] = (uint32_t) naux;
  memset(out, 0, sizeof *out);
  out->n = n;
  out->tid = c.tid; out->pos = c.pos; out->mtid = c.mtid; out->mpos = c.mpos; out->isize = c.isize;
  out->flag = c.flag; out->mapq = c.mapq; out->qhash = c.qhash; out->qcheck = c.qcheck;
  out->cigar_off = c.cigar_off; out->cigar = cig; out->aux_off = c.aux_off; out->aux = aux;
  out->n_cigar_words = (uint32_t) ncig;
  out->n_aux_bytes = (uint32_t) naux;
  b->t_decode_s = now_s() - t0;
  if (bk_debug("feed"))
    fprintf(stderr, "[feed] %zu records, %.1f MB inflated: inflate %.3f s, decode %.3f s, %u threads, %s host columns\n", n, dsize / 1e6, b->t_inflate_s,
            b->t_decode_s, nt, b->tid.pinned ? "pinned" : "pageable");
  return BK_OK;
}

// no C++ exception crosses the C boundary: a corrupt file (attacker-chosen ISIZE sums, record counts) must come back as an
// error code, not std::terminate
template <class F> static int no_throw(char *err, size_t errlen, F &&f)
{
  try
  {
    return f();
  }
  catch (const std::bad_alloc &)
  {
    set_err(err, errlen, "out of host memory while decoding the BAM");
    return BK_ERR_LIMIT;
  }
  catch (const std::exception &e)
  {
    set_err(err, errlen, e.what());
    return BK_ERR_IO;
  }
}
extern "C" int bk_bam_open(const char *path, bk_bam **out, char *err, size_t errlen)
{
  return no_throw(err, errlen, [&] { return bam_open_impl(path, out, err, errlen); });
}
extern "C" int bk_bam_decode(bk_bam *b, bk_soa *out, char *err, size_t errlen)
{
  return no_throw(err, errlen, [&] { return bam_decode_impl(b, out, err, errlen); });
}
extern "C" void bk_bam_close(bk_bam *b) { delete b; }

// ---- bk_bam_extract: read names back from their hashes, and the reads themselves (include/breakid_hip.h) -----------------------
// One streaming pass with bounded memory: the file is read in chunks, every BGZF block is inflated on its own into a carry buffer
// that holds the bytes of the header or record still incomplete (records may cross blocks), and selected records go straight
// into the BGZF writer.  Nothing of bk_bam_open is used: it holds the whole inflated file.

namespace
{
struct ExtractError
{
  int code;
  std::string msg;
};

// BGZF writer with htslib's layout (bgzf.c: bgzf_write / bgzf_flush_try / deflate_block): a block takes at most 0xff00 payload bytes,
// it is flushed before a record that would not fit, a longer record spans blocks, the 28-byte EOF block ends the file.
struct BgzfWriter
{
  static constexpr size_t BLOCK = 0xff00;
  FILE *f = nullptr;
  std::vector<uint8_t> buf, zbuf;
  BgzfWriter() { buf.reserve(BLOCK); }
  void flush()
  {
    if (buf.empty()) return;
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw ExtractError{BK_ERR_IO, "deflateInit2 failed"};
    zbuf.resize(18 + deflateBound(&zs, (uLong) buf.size()) + 8);
    zs.next_in = buf.data();
    zs.avail_in = (uInt) buf.size();
    zs.next_out = zbuf.data() + 18;
    zs.avail_out = (uInt) (zbuf.size() - 18 - 8);
    const int rc = deflate(&zs, Z_FINISH);
    const size_t clen = zs.total_out;
    deflateEnd(&zs);
    size_t total = 18 + clen + 8;
    if (rc != Z_STREAM_END || total > 65536)
    {
      // (incompressible data: stored deflate blocks of 0xff00 bytes fit, as in htslib, which retries at level 0)
      memset(&zs, 0, sizeof zs);
      if (deflateInit2(&zs, 0, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw ExtractError{BK_ERR_IO, "deflateInit2 failed"};
      zs.next_in = buf.data();
      zs.avail_in = (uInt) buf.size();
      zs.next_out = zbuf.data() + 18;
      zs.avail_out = (uInt) (zbuf.size() - 18 - 8);
      const int rc0 = deflate(&zs, Z_FINISH);
      total = 18 + zs.total_out + 8;
      deflateEnd(&zs);
      if (rc0 != Z_STREAM_END || total > 65536) throw ExtractError{BK_ERR_IO, "cannot deflate a BGZF block"};
    }
    static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    memcpy(zbuf.data(), head, 16);
    zbuf[16] = (uint8_t) ((total - 1) & 0xff);
    zbuf[17] = (uint8_t) ((total - 1) >> 8);
    const uint32_t crc = (uint32_t) crc32(crc32(0L, nullptr, 0), buf.data(), (uInt) buf.size()), isize = (uint32_t) buf.size();
    uint8_t *t = zbuf.data() + total - 8;
    for (int i = 0; i < 4; ++i)
    {
      t[i] = (uint8_t) (crc >> (8 * i));
      t[4 + i] = (uint8_t) (isize >> (8 * i));
    }
    if (fwrite(zbuf.data(), 1, total, f) != total) throw ExtractError{BK_ERR_IO, "cannot write the output BAM"};
    buf.clear();
  }
  void write(const uint8_t *p, size_t n)
  {
    while (n)
    {
      const size_t take = std::min(n, BLOCK - buf.size());
      buf.insert(buf.end(), p, p + take);
      p += take;
      n -= take;
      if (buf.size() == BLOCK) flush();
    }
  }
  // a record of n bytes follows: it starts a new block unless it fits into this one
  void record_follows(size_t n)
  {
    if (buf.size() + n > BLOCK) flush();
  }
  void finish()
  {
    flush();
    static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (fwrite(eof, 1, 28, f) != 28 || fflush(f) != 0) throw ExtractError{BK_ERR_IO, "cannot write the output BAM"};
  }
};

// the inflated stream, one BGZF block at a time: `buf` holds the bytes not consumed yet
struct BgzfStream
{
  static constexpr size_t CHUNK_BYTES = 4u << 20;
  FILE *f = nullptr;
  std::vector<uint8_t> in;   // file bytes not parsed yet
  size_t in_pos = 0;
  bool file_end = false;
  std::vector<uint8_t> buf;  // inflated bytes not consumed yet
  size_t pos = 0;
  void refill()
  {
    in.erase(in.begin(), in.begin() + (ptrdiff_t) in_pos);
    in_pos = 0;
    const size_t old = in.size();
    in.resize(old + CHUNK_BYTES);
    const size_t got = fread(in.data() + old, 1, CHUNK_BYTES, f);
    if (got < CHUNK_BYTES)
    {
      if (ferror(f)) throw ExtractError{BK_ERR_IO, "read error on the input BAM"};
      file_end = true;
    }
    in.resize(old + got);
  }
  bool have(size_t n)  // n bytes of the file at in_pos; false at a clean end of file (no byte left)
  {
    while (in.size() - in_pos < n && !file_end) refill();
    if (in.size() - in_pos >= n) return true;
    if (in.size() == in_pos) return false;
    throw ExtractError{BK_ERR_IO, "truncated BGZF block"};
  }
  // appends the next block's data to buf; false at the end of the file
  bool next_block()
  {
    if (!have(18)) return false;
    const uint8_t *h = in.data() + in_pos;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) throw ExtractError{BK_ERR_IO, "not a BGZF block"};
    const uint16_t xlen = rd16(h + 10);
    if (!have(12 + (size_t) xlen)) throw ExtractError{BK_ERR_IO, "truncated BGZF block"};
    h = in.data() + in_pos;
    const uint8_t *x = h + 12;
    int bsize = -1;
    for (size_t k = 0; k + 4 <= xlen;)
    {
      const uint16_t slen = rd16(x + k + 2);
      if (x[k] == 66 && x[k + 1] == 67 && slen == 2 && k + 6 <= xlen) bsize = rd16(x + k + 4);
      k += 4 + (size_t) slen;
    }
    if (bsize < 0 || (size_t) bsize + 1 < 12 + (size_t) xlen + 8) throw ExtractError{BK_ERR_IO, "bad BGZF block size"};
    if (!have((size_t) bsize + 1)) throw ExtractError{BK_ERR_IO, "truncated BGZF block"};
    h = in.data() + in_pos;
    const size_t clen = (size_t) bsize + 1 - (12 + (size_t) xlen) - 8;
    const uint32_t crc = rd32(h + bsize + 1 - 8), isize = rd32(h + bsize + 1 - 4);
    if (isize > 65536u) throw ExtractError{BK_ERR_IO, "BGZF block claims more than 64 KiB of data"};
    if (pos > (1u << 20) && pos * 2 > buf.size())  // drop what was consumed, now and then
    {
      buf.erase(buf.begin(), buf.begin() + (ptrdiff_t) pos);
      pos = 0;
    }
    const size_t old = buf.size();
    buf.resize(old + isize);
    if (isize)
    {
      z_stream zs;
      memset(&zs, 0, sizeof zs);
      if (inflateInit2(&zs, -15) != Z_OK) throw ExtractError{BK_ERR_IO, "inflateInit2 failed"};
      zs.next_in = const_cast<Bytef *>(h + 12 + xlen);
      zs.avail_in = (uInt) clen;
      zs.next_out = buf.data() + old;
      zs.avail_out = isize;
      const int rc = inflate(&zs, Z_FINISH);
      const bool whole = zs.avail_out == 0;
      inflateEnd(&zs);
      if (rc != Z_STREAM_END || !whole) throw ExtractError{BK_ERR_IO, "inflate failed: bad BGZF block"};
      if ((uint32_t) crc32(crc32(0L, nullptr, 0), buf.data() + old, isize) != crc) throw ExtractError{BK_ERR_IO, "bad BGZF block: CRC mismatch"};
    }
    in_pos += (size_t) bsize + 1;
    return true;
  }
  // at least n unconsumed bytes in buf; false when the stream ends before that (avail() tells how many there are)
  bool need(size_t n)
  {
    while (buf.size() - pos < n)
      if (!next_block()) return false;
    return true;
  }
  size_t avail() const { return buf.size() - pos; }
  const uint8_t *ptr() const { return buf.data() + pos; }
};

struct KeyHash
{
  size_t operator()(uint64_t h) const { return (size_t) h; }
};

// qhash -> the keys that carry it, in key order; shared by bk_bam_extract and bk_bam_reads
struct KeyMap
{
  const bk_read_key *keys = nullptr;
  std::unordered_map<uint64_t, std::vector<uint64_t>, KeyHash> by_hash;
  // `check(k)` may refuse key k before it is entered; `who` names the caller in the duplicate's message
  template <class C> void build(const bk_read_key *ks, uint64_t n_keys, const char *who, C &&check)
  {
    keys = ks;
    by_hash.reserve((size_t) n_keys * 2 + 1);
    for (uint64_t k = 0; k < n_keys; ++k)
    {
      check(k);
      std::vector<uint64_t> &v = by_hash[keys[k].qhash];
      for (uint64_t o : v)
        if (keys[o].qcheck == keys[k].qcheck) throw ExtractError{BK_ERR_ARG, std::string(who) + ": duplicate key " + std::to_string(k)};
      v.push_back(k);
    }
  }
  // the first key that selects the read name (-1: none); every selecting key is passed to `each`
  template <class E> int64_t match(const char *qn, size_t qlen, E &&each) const
  {
    const auto it = by_hash.find(bk_qname_hash(qn, qlen));
    if (it == by_hash.end()) return -1;
    const uint32_t check = bk_qname_check(qn, qlen);
    int64_t first = -1;
    for (uint64_t k : it->second)
      if (keys[k].qcheck == 0 || keys[k].qcheck == check)
      {
        if (first < 0) first = (int64_t) k;
        each(k);
      }
    return first;
  }
};

// The record walk both share: header(ptr, len) sees the header's bytes once, record(r, bs, qn, qlen) every record (r = the bs bytes
// behind block_size, checked to hold name, CIGAR, SEQ and QUAL; qn / qlen = the read name as a C string).
template <class H, class R> void walk_records(BgzfStream &s, H &&header, R &&record)
{
  if (!s.need(12) || memcmp(s.ptr(), "BAM\1", 4) != 0) throw ExtractError{BK_ERR_IO, "not a BAM file"};
  const size_t l_text = rd32(s.ptr() + 4);
  if (!s.need(12 + l_text)) throw ExtractError{BK_ERR_IO, "truncated BAM header"};
  const uint32_t n_ref = rd32(s.ptr() + 8 + l_text);
  size_t hlen = 12 + l_text;
  for (uint32_t i = 0; i < n_ref; ++i)
  {
    if (!s.need(hlen + 4)) throw ExtractError{BK_ERR_IO, "truncated BAM header"};
    const size_t l_name = rd32(s.ptr() + hlen);
    hlen += 4 + l_name + 4;
    if (!s.need(hlen)) throw ExtractError{BK_ERR_IO, "truncated BAM header"};
  }
  header(s.ptr(), hlen);
  s.pos += hlen;
  for (;;)
  {
    if (!s.need(4))
    {
      if (s.avail() == 0) break;
      throw ExtractError{BK_ERR_IO, "truncated BAM record"};
    }
    const size_t bs = rd32(s.ptr());
    if (bs < 32) throw ExtractError{BK_ERR_IO, "corrupt BAM record"};
    if (!s.need(4 + bs)) throw ExtractError{BK_ERR_IO, "truncated BAM record: it is longer than its stream"};
    const uint8_t *r = s.ptr() + 4;
    const size_t l_name = r[8], n_cig = rd16(r + 12), l_seq = rd32(r + 16);
    if (32 + l_name + n_cig * 4 + (l_seq + 1) / 2 + l_seq > bs) throw ExtractError{BK_ERR_IO, "corrupt BAM record"};
    const char *qn = (const char *) r + 32;
    const size_t qlen = l_name ? strnlen(qn, l_name) : 0;  // bam_get_qname is a C string
    record(r, bs, qn, qlen);
    s.pos += 4 + bs;
  }
}

int bam_extract_impl(const char *in_bam, const char *out_bam, const bk_read_key *keys, uint64_t n_keys, const char *const *tags, uint64_t n_tags, char **names_out,
                     uint64_t *n_written, std::string &tmp_path, FILE *&fin, FILE *&fout)
{
  if (!in_bam) throw ExtractError{BK_ERR_ARG, "bk_bam_extract: null input path"};
  if ((n_keys && !keys) || (n_tags && !tags)) throw ExtractError{BK_ERR_ARG, "bk_bam_extract: null keys or tags"};
  KeyMap km;
  km.build(keys, n_keys, "bk_bam_extract", [&](uint64_t k) {
    if (keys[k].tag >= n_tags) throw ExtractError{BK_ERR_ARG, "bk_bam_extract: key " + std::to_string(k) + " has tag " + std::to_string(keys[k].tag) + " of " + std::to_string(n_tags)};
    if (!tags[keys[k].tag]) throw ExtractError{BK_ERR_ARG, "bk_bam_extract: null tag text"};
  });
  std::vector<std::string> names(n_keys);
  std::vector<uint8_t> seen(n_keys, 0);
  fin = fopen(in_bam, "rb");
  if (!fin) throw ExtractError{BK_ERR_IO, std::string("cannot open ") + in_bam};
  BgzfStream s;
  s.f = fin;
  BgzfWriter w;
  if (out_bam)
  {
    tmp_path = std::string(out_bam) + ".tmp." + std::to_string((long) getpid());
    fout = fopen(tmp_path.c_str(), "wb");
    if (!fout)
    {
      tmp_path.clear();
      throw ExtractError{BK_ERR_IO, std::string("cannot write ") + out_bam};
    }
    w.f = fout;
  }
  uint64_t written = 0;
  std::vector<uint8_t> rec;
  walk_records(
      s,
      [&](const uint8_t *h, size_t hlen) {  // header: copied byte for byte
        if (!out_bam) return;
        w.write(h, hlen);
        w.flush();  // (htslib ends the header's block before the first record)
      },
      [&](const uint8_t *r, size_t bs, const char *qn, size_t qlen) {
        const int64_t first = km.match(qn, qlen, [&](uint64_t k) {
          if (!seen[k])
          {
            seen[k] = 1;
            names[k].assign(qn, qlen);
          }
        });
        if (first < 0) return;
        ++written;
        if (!out_bam) return;
        const char *tag = tags[keys[first].tag];
        const size_t tl = strlen(tag), nbs = bs + 3 + tl + 1;
        if (nbs > 0x7FFFFFFFull) throw ExtractError{BK_ERR_IO, "record too long for a bk tag"};
        rec.resize(4 + nbs);
        for (int i = 0; i < 4; ++i) rec[i] = (uint8_t) (nbs >> (8 * i));
        memcpy(rec.data() + 4, r, bs);
        uint8_t *a = rec.data() + 4 + bs;
        a[0] = 'b';
        a[1] = 'k';
        a[2] = 'Z';
        memcpy(a + 3, tag, tl + 1);
        w.record_follows(rec.size());
        w.write(rec.data(), rec.size());
      });
  if (names_out)  // (before the rename: a failure here must leave no output file)
  {
    size_t total = 0;
    for (const std::string &n : names) total += n.size() + 1;
    char *p = (char *) malloc(total ? total : 1);
    if (!p) throw std::bad_alloc();
    *names_out = p;
    for (const std::string &n : names)
    {
      memcpy(p, n.c_str(), n.size() + 1);
      p += n.size() + 1;
    }
  }
  if (out_bam)
  {
    w.finish();
    FILE *f = fout;
    fout = nullptr;
    if (fclose(f) != 0) throw ExtractError{BK_ERR_IO, std::string("cannot write ") + out_bam};
    if (rename(tmp_path.c_str(), out_bam) != 0) throw ExtractError{BK_ERR_IO, std::string("cannot rename the output to ") + out_bam};
    tmp_path.clear();
  }
  if (n_written) *n_written = written;
  return BK_OK;
}

// ---- bk_bam_reads: the alignments of named reads with their bases (include/breakid_hip.h) ---------------------------------------
// The same pass as bk_bam_extract; a selected record goes into the columns of a ReadsTable instead of a file.
struct ReadsTable
{
  std::vector<int32_t> tid, pos;
  std::vector<uint16_t> flag;
  std::vector<uint8_t> mapq;
  std::vector<uint32_t> key, cigar_off{0}, cigar, l_seq;
  std::vector<uint64_t> seq_off{0};
  std::vector<uint8_t> seq;
};

void bam_reads_impl(const char *in_bam, const bk_read_key *keys, uint64_t n_keys, ReadsTable &t, FILE *&fin)
{
  if (!in_bam) throw ExtractError{BK_ERR_ARG, "bk_bam_reads: null input path"};
  if (n_keys && !keys) throw ExtractError{BK_ERR_ARG, "bk_bam_reads: null keys"};
  if (n_keys > 0xFFFFFFFFull) throw ExtractError{BK_ERR_ARG, "bk_bam_reads: more than 2^32 keys"};
  KeyMap km;
  km.build(keys, n_keys, "bk_bam_reads", [](uint64_t) {});
  fin = fopen(in_bam, "rb");
  if (!fin) throw ExtractError{BK_ERR_IO, std::string("cannot open ") + in_bam};
  BgzfStream s;
  s.f = fin;
  walk_records(
      s, [](const uint8_t *, size_t) {},
      [&](const uint8_t *r, size_t, const char *qn, size_t qlen) {
        const int64_t first = km.match(qn, qlen, [](uint64_t) {});
        if (first < 0) return;
        const size_t l_name = r[8], n_cig = rd16(r + 12), l_seq = rd32(r + 16);
        if (t.cigar.size() + n_cig > 0xFFFFFFFFull) throw ExtractError{BK_ERR_LIMIT, "bk_bam_reads: more than 2^32 CIGAR words"};
        t.tid.push_back((int32_t) rd32(r));
        t.pos.push_back((int32_t) rd32(r + 4));
        t.mapq.push_back(r[9]);
        t.flag.push_back(rd16(r + 14));
        t.key.push_back((uint32_t) first);
        const uint8_t *cg = r + 32 + l_name;
        for (size_t j = 0; j < n_cig; ++j) t.cigar.push_back(rd32(cg + 4 * j));
        t.cigar_off.push_back((uint32_t) t.cigar.size());
        t.l_seq.push_back((uint32_t) l_seq);
        const uint8_t *sq = cg + 4 * n_cig;
        t.seq.insert(t.seq.end(), sq, sq + (l_seq + 1) / 2);
        t.seq_off.push_back((uint64_t) t.seq.size());
      });
}
}  // namespace

extern "C" int bk_bam_extract(const char *in_bam, const char *out_bam, const bk_read_key *keys, uint64_t n_keys, const char *const *tags, uint64_t n_tags,
                              char **names_out, uint64_t *n_written, char *err, size_t errlen)
{
  if (names_out) *names_out = nullptr;
  if (n_written) *n_written = 0;
  std::string tmp_path;
  FILE *fin = nullptr, *fout = nullptr;
  int rc = no_throw(err, errlen, [&] {
    try
    {
      return bam_extract_impl(in_bam, out_bam, keys, n_keys, tags, n_tags, names_out, n_written, tmp_path, fin, fout);
    }
    catch (const ExtractError &e)
    {
      set_err(err, errlen, e.msg);
      return e.code;
    }
  });
  if (fin) fclose(fin);
  if (fout) fclose(fout);
  if (rc != BK_OK)
  {
    if (!tmp_path.empty()) (void) remove(tmp_path.c_str());  // no output file on any failure (the target itself is only ever renamed into)
    if (names_out && *names_out)
    {
      free(*names_out);
      *names_out = nullptr;
    }
    if (n_written) *n_written = 0;
  }
  return rc;
}

extern "C" void bk_bam_names_free(char *names) { free(names); }

extern "C" int bk_bam_reads(const char *in_bam, const bk_read_key *keys, uint64_t n_keys, bk_reads *out, char *err, size_t errlen)
{
  if (!out)
  {
    set_err(err, errlen, "bk_bam_reads: null output");
    return BK_ERR_ARG;
  }
  memset(out, 0, sizeof *out);
  ReadsTable *t = nullptr;
  FILE *fin = nullptr;
  const int rc = no_throw(err, errlen, [&] {
    try
    {
      t = new ReadsTable;
      bam_reads_impl(in_bam, keys, n_keys, *t, fin);
      return (int) BK_OK;
    }
    catch (const ExtractError &e)
    {
      set_err(err, errlen, e.msg);
      return e.code;
    }
  });
  if (fin) fclose(fin);
  if (rc != BK_OK)
  {
    delete t;
    return rc;
  }
  out->n = t->tid.size();
  out->tid = t->tid.data();
  out->pos = t->pos.data();
  out->flag = t->flag.data();
  out->mapq = t->mapq.data();
  out->key = t->key.data();
  out->cigar_off = t->cigar_off.data();
  out->cigar = t->cigar.data();
  out->l_seq = t->l_seq.data();
  out->seq_off = t->seq_off.data();
  out->seq = t->seq.data();
  out->owner = t;
  return BK_OK;
}

extern "C" void bk_reads_free(bk_reads *r)
{
  if (!r) return;
  delete static_cast<ReadsTable *>(r->owner);
  memset(r, 0, sizeof *r);
}
