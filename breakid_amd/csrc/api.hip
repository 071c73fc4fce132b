// C ABI of libbreakid_hip.so (include/breakid_hip.h): context, record upload, stage drivers, fetch.
#include <algorithm>
#include <cmath>
#include <limits>
#include <cstring>
#include <numeric>

#include "bk_common.h"
#include "prims.h"
#include "stream.h"
#include "join.h"
#include "cluster.h"
#include "bp.h"
#include "normal.h"
#include "genotype.h"
#include "clip.h"
#include "junction.h"
#include "evidence.h"
#include "unique.h"
#include "consensus.h"
#include "jfit.h"
#include "locsim.h"
#include "seqmatch.h"
#include "seqcx.h"
#include "coverage.h"
#include "context.h"
#include "frame.h"
#include "link.h"
#include "partners.h"
#include "fragsize.h"
#include "known.h"
#include "sjcall.h"
#include "gaps.h"
#include "cliploci.h"
#include "exclude.h"
#include "ahc.h"
#include "lanes.h"
#include "bgzf_gpu.h"

namespace
{
thread_local std::string g_init_error;

uint64_t fnv64(const std::string &s)
{
  uint64_t h = 0xCBF29CE484222325ull;
  for (unsigned char c : s)
  {
    h ^= c;
    h *= 0x100000001B3ull;
  }
  return h;
}
std::string chrom_id_to_name(int tid)  // util_bam.cc:128-142
{
  if (tid == 23) return "chrY";
  if (tid == 22) return "chrX";
  if (tid >= 0 && tid < 22) return "chr" + std::to_string(tid + 1);
  return "";
}

struct StageTimer
{
  std::string name;
  hipEvent_t a = nullptr, b = nullptr;
  uint64_t bytes = 0;    // SURVEY 8(d) algorithmic bytes credited to this stage (every column once for the whole path)
  uint64_t touched = 0;  // bytes this stage's kernels themselves load + store (0 = not modelled)
};
}  // namespace

struct bk_ctx
{
  int device = 0;
  hipStream_t st = nullptr;
  bool own_stream = true;
  std::string err;
  int nt = 0;
  std::vector<uint32_t> tlen;
  std::vector<std::string> tname;
  std::vector<int32_t> hdr_id_host;
  DevBuf d_tprefix, d_nhash, d_nid, d_own, d_hdr;
  NameTableDev names{};

  // records
  bk_soa rec{};
  DevBuf col[13];
  DevBuf d_side;  // bk_side rows of an uploaded host table
  DevBuf xcol[13];  // bk_exclude_regions: the kept records are written here, then the two sets swap
  bool have_records = false;
  bool streamed = false;  // a stream pass has started on this table (bk_exclude_regions is refused from then on)

  // stream pass
  DevBuf d_counters, d_sd, d_cand, d_split_raw, d_split, d_sa_list;
  StreamCounters hc{};
  SdState hsd{};
  bool stream_done = false, splits_sorted = false;
  int mapq_min = 20;
  int stream_mapq = -1;  // threshold the candidate list in d_cand was filtered with
  uint64_t cand_cap = 0, split_cap = 0, sa_cap = 0;
  // sharded sample: this table is records [rec_base, rec_base + n) of the sample; gathered tables replace the local ones
  uint64_t rec_base = 0;
  std::vector<uint64_t> route_counts;
  JoinBufs jb2;  // grouping of the pairs received from the other ranks (jb still backs the routed send buffer)
  const Cand *ext_cand = nullptr;
  const bk_split *ext_split = nullptr;
  bk_cluster *ext_clusters = nullptr;
  std::vector<uint8_t> own_groups;  // per group (numeric key order): 1 = this rank clusters it; empty = all
  const Cand *cand_ptr() const { return ext_cand ? ext_cand : d_cand.get<Cand>(); }
  const bk_split *split_raw_ptr() const { return ext_split ? ext_split : d_split_raw.get<bk_split>(); }
  bk_cluster *clusters_ptr() const { return ext_clusters ? ext_clusters : d_clusters.get<bk_cluster>(); }
  SdBufs sdb;
  double mean = 0, sd = 0;
  bool stats_done = false;

  // join
  JoinBufs jb;
  JoinResult jr;
  std::vector<uint32_t> gkey_host, glex_host, lex_to_num;
  std::vector<uint64_t> gstart_host;
  DevBuf d_glex, d_lex_to_num;  // device copies of glex_host and lex_to_num (cluster_summary numbers the slots in lexicographic group order)

  // mask + cluster (lanes.hip): the lists and cluster numbers it leaves, its lanes, its sort service
  ClusterStage stage;
  bool clustered = false;

  // summary + breakpoints
  BpBufs bb;
  DevBuf d_clusters;
  uint64_t n_clusters = 0;

  // call order / kind of this context, checked by bk_normal_support
  bool joined = false, bp_done = false, shard = false;
  double join_w = 0;
  // matched normal (bk_normal_support: this context is the tumour)
  NormalBufs nb;
  std::vector<struct bk_normal_support> f_normal;
  // reference-allele evidence (bk_ref_support: this context holds the calls)
  RefBufs rb;
  std::vector<struct bk_ref_support> f_ref;
  // soft-clip evidence (bk_clip_support: this context holds the calls) and depth at arbitrary positions (bk_base_depth)
  ClipBufs cb;
  std::vector<struct bk_clip_support> f_clip;
  DevBuf d_bd_tid, d_bd_pos, d_bd_out, d_bd_samp;
  std::vector<uint32_t> f_base_depth;
  // the clipped reads at given sites (bk_clip_reads: this context holds the records)
  ClipReadBufs crb;
  std::vector<uint32_t> f_cr_counts;
  std::vector<struct bk_clip_read> f_cr_rows;
  std::vector<uint64_t> f_cr_off;
  // junction evidence (bk_junctions); summary_map: bb still holds the slot -> cluster-row map of the last bk_cluster_summary
  JunctionBufs jnb;
  std::vector<struct bk_junction> f_junction;
  bool summary_map = false;
  // evidence export (bk_evidence)
  EvidenceBufs evb;
  std::vector<struct bk_evidence> f_evidence;
  std::vector<uint64_t> f_ev_off;
  // unique fragments (bk_unique_support)
  UniqueBufs uqb;
  std::vector<struct bk_unique_support> f_unique;
  std::vector<uint64_t> f_uq_first;
  // junction consensus (bk_clip_consensus)
  ConsensusBufs cnb;
  std::vector<struct bk_consensus> f_cons;
  std::vector<uint8_t> f_cons_bases;
  std::vector<uint32_t> f_cons_depth;
  // junction fit (bk_junction_fit)
  JfitBufs jfb;
  std::vector<struct bk_junction_fit> f_jfit;
  // locus similarity (bk_locus_similarity)
  LocsimBufs lsb;
  std::vector<struct bk_locus_sim> f_locsim;
  // sequence match (bk_sequence_match)
  SeqmatchBufs smb;
  std::vector<struct bk_seq_hit> f_seqhit;
  // site complexity (bk_site_complexity)
  SeqcxBufs scb;
  std::vector<struct bk_site_cplx> f_sitecx;
  // window coverage (bk_window_coverage: this context holds the records)
  CovBufs cvb;
  std::vector<struct bk_window_cov> f_wincov;
  // window context (bk_window_context: this context holds the records)
  CtxBufs cxb;
  std::vector<struct bk_window_ctx> f_winctx;
  // fusion frame (bk_fusion_frame)
  FrameBufs frb;
  std::vector<struct bk_frame_call> f_frame;
  // linked calls (bk_link_calls)
  LinkBufs lkb;
  std::vector<struct bk_call_link> f_link;
  // partner loci (bk_locus_partners)
  PartnerBufs ptb;
  std::vector<struct bk_locus_partners> f_partners;
  // fragment sizes (bk_fragment_sizes)
  FragBufs fgb;
  std::vector<struct bk_frag_sizes> f_fragsize;
  // known junctions (bk_known_calls)
  KnownBufs knb;
  std::vector<struct bk_known_call> f_known;
  // split junctions (bk_split_junctions)
  SjBufs sjb;
  SjStats sj_stats;
  std::vector<SjClaim> sj_claims;  // the voted rows' breakpoints, sorted; valid until the breakpoint stage runs again
  bool sj_claims_valid = false;
  std::vector<struct bk_split_junction> f_sj;
  // CIGAR gaps (bk_cigar_gaps: this context holds the records)
  GapBufs gpb;
  GapStats gap_stats;
  std::vector<struct bk_cigar_gap> f_gaps;
  // soft-clip loci (bk_clip_loci: this context holds the records)
  ClipLociBufs cllb;
  ClipLociStats cll_stats;
  std::vector<struct bk_clip_locus> f_cll;

  // test hooks of the primitives (bk_debug_scan, bk_debug_radix_sort): buffers that live as long as the context, as a stage's do
  prims::RadixBufs dbg_radix;
  DevBuf dbg_in, dbg_out, dbg_vals;

  // fetch staging
  std::vector<bk_pair> f_pairs[3];
  std::vector<uint64_t> f_off[3];
  std::vector<bk_split> f_splits;
  std::vector<bk_cluster> f_clusters;
  std::vector<int32_t> f_gkeys;
  std::vector<bk_group_stat> f_gstats;

  // timing
  bool timing = false;
  std::vector<StageTimer> timers;
  Timing tout;

  void tick(const char *name, uint64_t bytes, bool begin, uint64_t touched = 0)
  {
    if (!timing) return;
    if (begin)
    {
      StageTimer t;
      t.name = name;
      t.bytes = bytes;
      t.touched = touched;
      HIP_CHECK(hipEventCreate(&t.a));
      HIP_CHECK(hipEventCreate(&t.b));
      HIP_CHECK(hipEventRecord(t.a, st));
      timers.push_back(t);
    }
    else
      HIP_CHECK(hipEventRecord(timers.back().b, st));
  }
};

static RecView rec_view(const bk_ctx *ctx)
{
  RecView r;
  r.n = ctx->rec.n;
  r.tid = ctx->rec.tid; r.pos = ctx->rec.pos; r.flag = ctx->rec.flag; r.mapq = ctx->rec.mapq;
  r.cigar_off = ctx->rec.cigar_off; r.cigar = ctx->rec.cigar;
  r.isize = ctx->rec.isize; r.aux_off = ctx->rec.aux_off;
  return r;
}

namespace
{
struct Scope
{
  bk_ctx *c;
  Scope(bk_ctx *c, const char *name, uint64_t bytes = 0, uint64_t touched = 0) : c(c) { c->tick(name, bytes, true, touched); }
  ~Scope()
  {
    try
    {
      c->tick("", 0, false);
    }
    catch (...)
    {
    }
  }
};

template <class F> int guarded(bk_ctx *ctx, F &&f)
{
  if (!ctx) return BK_ERR_ARG;
  try
  {
    HIP_CHECK(hipSetDevice(ctx->device));
    f();
    return BK_OK;
  }
  catch (const bk_error &e)
  {
    ctx->err = e.msg;
    return e.code;
  }
  catch (const std::exception &e)
  {
    ctx->err = e.what();
    return BK_ERR_HIP;
  }
}

// n device rows into `out`; returns when they (and every copy queued before them) have arrived
template <class T> void rows_to_host(bk_ctx *ctx, const T *d_rows, uint64_t n, std::vector<T> &out)
{
  out.resize(n);
  if (n) HIP_CHECK(hipMemcpyAsync(out.data(), d_rows, n * sizeof(T), hipMemcpyDeviceToHost, ctx->st));
  HIP_CHECK(hipStreamSynchronize(ctx->st));
}

void build_name_tables(bk_ctx *c)
{
  const int nt = c->nt;
  std::map<std::string, int> ids;
  for (int i = 0; i < nt; ++i)
    if (!ids.count(c->tname[i])) ids[c->tname[i]] = i;
  if (!ids.count("")) ids[""] = nt;
  if (!ids.count("*")) ids["*"] = nt + 1;
  for (int t = 0; t < 24; ++t)
  {
    std::string s = chrom_id_to_name(t);
    if (!ids.count(s)) ids[s] = nt + 2 + t;
  }
  uint32_t cap = 64;
  while (cap < ids.size() * 4) cap <<= 1;
  std::vector<uint64_t> hash(cap, 0);
  std::vector<int32_t> idv(cap, -1);
  for (auto &kv : ids)
  {
    uint64_t h = fnv64(kv.first);
    if (h == 0) h = 1;
    uint32_t slot = (uint32_t) h & (cap - 1);
    while (hash[slot] != 0 && hash[slot] != h) slot = (slot + 1) & (cap - 1);
    if (hash[slot] == 0)
    {
      hash[slot] = h;
      idv[slot] = kv.second;
    }
  }
  std::vector<int32_t> own(std::max(nt, 1));
  for (int t = 0; t < nt; ++t) own[t] = ids[chrom_id_to_name(t)];
  c->hdr_id_host.assign(nt + 1, 0);
  c->hdr_id_host[0] = ids["*"];
  for (int t = 0; t < nt; ++t) c->hdr_id_host[t + 1] = ids[c->tname[t]];
  std::vector<uint32_t> prefix(nt + 1, 0);
  for (int t = 0; t < nt; ++t) prefix[t + 1] = prefix[t] + c->tlen[t];
  HIP_CHECK(hipMemcpy(c->d_nhash.as<uint64_t>(cap), hash.data(), cap * 8, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(c->d_nid.as<int32_t>(cap), idv.data(), cap * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(c->d_own.as<int32_t>(own.size()), own.data(), own.size() * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(c->d_hdr.as<int32_t>(nt + 1), c->hdr_id_host.data(), (nt + 1) * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(c->d_tprefix.as<uint32_t>(nt + 1), prefix.data(), (nt + 1) * 4, hipMemcpyHostToDevice));
  c->names.hash = c->d_nhash.get<uint64_t>();
  c->names.id = c->d_nid.get<int32_t>();
  c->names.mask = cap - 1;
  c->names.own_id = c->d_own.get<int32_t>();
  c->names.n_targets = nt;
  c->names.empty_id = ids[""];
}

std::string rname(const bk_ctx *c, int tid) { return tid < 0 ? "*" : c->tname[tid]; }

// ---- stream pass (A1 sums, A2 filter, A12 gate) ------------------------------------------------------------------
// Three steps so that the table may arrive in pieces (bk_bam_decode_device_ctx: the pass runs on the records of a feed chunk
// while the next chunks are still being copied and inflated): prepare (outputs sized, counters cleared), any number of
// launches over consecutive record ranges (the counters accumulate, candidates / SA-bearing record indices append), finish
// (counters read back, rare-path kernel over the SA-bearing records).
StreamArgs stream_args(bk_ctx *c, uint64_t n)
{
  StreamArgs a{};
  a.n = n;
  a.q_begin = 0;
  a.rec_base = c->rec_base;
  a.tid = c->rec.tid; a.pos = c->rec.pos; a.mtid = c->rec.mtid; a.mpos = c->rec.mpos; a.isize = c->rec.isize;
  a.flag = c->rec.flag; a.mapq = c->rec.mapq; a.qhash = c->rec.qhash; a.qcheck = c->rec.qcheck;
  static const bool no_side = getenv("BREAKID_NO_SIDE") != nullptr;  // (comparison: the four columns even when the table has the rows)
  a.side = no_side && c->rec.qhash ? nullptr : c->rec.side;
  a.cigar_off = c->rec.cigar_off; a.cigar = c->rec.cigar; a.aux_off = c->rec.aux_off; a.aux = c->rec.aux;
  a.mapq_min = c->mapq_min;
  a.names = c->names;
  a.counters = c->d_counters.get<StreamCounters>();
  a.sd = c->d_sd.get<SdState>();
  a.cand = c->d_cand.get<Cand>();
  a.cand_cap = c->cand_cap;
  a.split = c->d_split_raw.get<bk_split>();
  a.split_cap = c->split_cap;
  a.sa_list = c->d_sa_list.get<uint32_t>();
  a.sa_cap = c->sa_cap;
  return a;
}
void stream_prepare(bk_ctx *c, uint64_t n_expected)
{
  c->streamed = true;
  c->cand_cap = std::max<uint64_t>(c->cand_cap, std::max<uint64_t>(1u << 16, n_expected / 8 + 1024));
  c->split_cap = std::max<uint64_t>(c->split_cap, std::max<uint64_t>(1u << 14, n_expected / 32 + 1024));
  c->sa_cap = std::max<uint64_t>(c->sa_cap, std::max<uint64_t>(1u << 14, n_expected / 16 + 1024));
  StreamCounters *dc = c->d_counters.as<StreamCounters>(1);
  SdState *dsd = c->d_sd.as<SdState>(1);
  HIP_CHECK(hipMemsetAsync(dc, 0, sizeof(StreamCounters), c->st));
  HIP_CHECK(hipMemsetAsync(dsd, 0, sizeof(SdState), c->st));
  (void) c->d_cand.as<Cand>(c->cand_cap);
  (void) c->d_split_raw.as<bk_split>(c->split_cap);
  (void) c->d_sa_list.as<uint32_t>(c->sa_cap);
}
// returns false when an output capacity was exceeded (the caller enlarges and repeats the pass)
bool stream_finish(bk_ctx *c)
{
  HIP_CHECK(hipMemcpyAsync(&c->hc, c->d_counters.get<StreamCounters>(), sizeof(StreamCounters), hipMemcpyDeviceToHost, c->st));
  HIP_CHECK(hipMemcpyAsync(&c->hsd, c->d_sd.get<SdState>(), sizeof(SdState), hipMemcpyDeviceToHost, c->st));
  HIP_CHECK(hipStreamSynchronize(c->st));
  if (c->hc.n_cand > c->cand_cap || c->hc.n_sa > c->sa_cap)
  {
    c->cand_cap = std::max<uint64_t>(c->cand_cap, c->hc.n_cand + 1024);
    c->sa_cap = std::max<uint64_t>(c->sa_cap, c->hc.n_sa + 1024);
    return false;
  }
  return true;
}
void stream_rare_path(bk_ctx *c)
{
  const uint64_t n = c->rec.n;
  if (c->timing && !c->timers.empty())
  {
    c->timers.back().bytes += 32ull * c->hc.n_cand + 4ull * c->hc.n_sa;
    // what k_stream itself moves: tid, pos, isize, flag, mapq, cigar_off, aux_off of every record (23 B), the CIGAR words (span bound),
    // qhash + mtid + mpos (+ qcheck) only of the candidates (16-20 B read; with the bk_side rows the kernel asks for the whole 32-byte row -
    // the model keeps the 16-20 bytes it needs, i.e. it does not credit the row's padding) + the 40-byte candidate written, 4 B per SA-bearing record index
    c->timers.back().touched = 23ull * n + 4ull * c->rec.n_cigar_words + (c->rec.qcheck ? 60ull : 56ull) * c->hc.n_cand + 4ull * c->hc.n_sa;
  }
  if (c->hc.unsorted) throw bk_error(BK_ERR_UNSORTED, "records are not coordinate sorted (the reference requires an indexed, sorted BAM)");
  // rare path: evidence tuples of the SA-bearing records (capacity = one tuple per listed record)
  if (c->hc.n_sa > c->split_cap)
  {
    c->split_cap = c->hc.n_sa + 1024;
    (void) c->d_split_raw.as<bk_split>(c->split_cap);
  }
  StreamArgs a = stream_args(c, n);
  {
    Scope s(c, "k_split_records", c->rec.n_aux_bytes + 4ull * c->hc.n_sa);
    launch_split_records(a, c->hc.n_sa, c->st);
  }
  HIP_CHECK(hipMemcpyAsync(&c->hc, c->d_counters.get<StreamCounters>(), sizeof(StreamCounters), hipMemcpyDeviceToHost, c->st));
  HIP_CHECK(hipStreamSynchronize(c->st));
  if (c->timing && !c->timers.empty())
  {
    c->timers.back().bytes += 48ull * c->hc.n_split;
    c->timers.back().touched = c->timers.back().bytes + 40ull * c->hc.n_sa + 32ull * c->hc.n_split;  // + the fixed columns of the listed records, 80-byte tuples
  }
  c->stream_done = true;
  c->stream_mapq = c->mapq_min;
  c->splits_sorted = false;
  c->stats_done = false;
}

void run_stream(bk_ctx *c)
{
  if (!c->have_records) throw bk_error(BK_ERR_ARG, "no records uploaded");
  const uint64_t n = c->rec.n;
  for (int attempt = 0; attempt < 3; ++attempt)
  {
    stream_prepare(c, n);
    {
      // algorithmic bytes of this pass: 39 B/record + 4 B per CIGAR op (+ 32 B per candidate, added below)
      Scope s(c, "k_stream", 39ull * n + 4ull * c->rec.n_cigar_words);
      launch_stream(stream_args(c, n), c->st);
    }
    if (stream_finish(c)) break;
    if (c->timing && !c->timers.empty()) c->timers.pop_back();  // overflowed attempt is not a measured pass
    if (attempt == 2) throw bk_error(BK_ERR_LIMIT, "stream pass: output capacity");
  }
  stream_rare_path(c);
}

void ensure_splits_sorted(bk_ctx *c)
{
  if (c->splits_sorted) return;
  Scope s(c, "split_sort");
  bk_split *sorted = c->d_split.as<bk_split>(c->hc.n_split + 1);
  // tuples of this table carry its own record indices; a sharded sample's carry rec_base + i of every rank: the passes of the sort
  // follow the largest index among the tuples then (bits = 0: sort_splits looks)
  int bits = 0;
  if (!c->ext_split && c->rec_base == 0)
  {
    bits = 1;
    while (bits < 32 && (1ull << bits) < c->rec.n) ++bits;
  }
  sort_splits(const_cast<bk_split *>(c->split_raw_ptr()), c->hc.n_split, sorted, c->bb, c->st, bits);
  c->splits_sorted = true;
}
}  // namespace

extern "C" {

// once per process, before its first HIP call if the caller allows: bk_multi_run* calls this before it starts its rank threads
// (setenv must not run beside threads that read the environment)
void bk_prepare_process()
{
  static std::once_flag once;
  std::call_once(once, [] {
    const char *q = getenv("GPU_MAX_HW_QUEUES");
    stage_set_hw_queues(q ? atoi(q) : 4);  // (ROCm's default is 4 when it is unset)
  });
}

int bk_init(int device, const uint32_t *target_len, const char *const *target_name, int n_targets, bk_ctx **out)
{
  {
    // the hardware-queue count the runtime started with (the lanes of bk_mask_and_cluster and the chunk streams of the GPU feed
    // share queues when there are fewer than they have streams: the stage tells it once on stderr)
    bk_prepare_process();
  }
  if (!out || n_targets < 0 || (n_targets && (!target_len || !target_name)))
  {
    g_init_error = "bk_init: bad arguments";
    return BK_ERR_ARG;
  }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
  {
    g_init_error = "bk_init: no HIP device " + std::to_string(device) + " (this library has no CPU path)";
    return BK_ERR_NO_DEVICE;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
  {
    g_init_error = std::string("bk_init: device is not gfx950 (") + prop.gcnArchName + "); kernels are built for MI355X only";
    return BK_ERR_NO_DEVICE;
  }
  bk_ctx *c = new bk_ctx();
  c->device = device;
  c->nt = n_targets;
  for (int i = 0; i < n_targets; ++i)
  {
    c->tlen.push_back(target_len[i]);
    c->tname.push_back(target_name[i]);
  }
  int rc = guarded(c, [&] {
    HIP_CHECK(hipStreamCreate(&c->st));
    build_name_tables(c);
  });
  if (rc != BK_OK)
  {
    g_init_error = c->err;
    delete c;
    return rc;
  }
  *out = c;
  return BK_OK;
}

void bk_free(bk_ctx *ctx)
{
  if (!ctx) return;
  (void) hipSetDevice(ctx->device);
  (void) hipStreamSynchronize(ctx->st);
  for (auto &t : ctx->timers)
  {
    if (t.a) (void) hipEventDestroy(t.a);
    if (t.b) (void) hipEventDestroy(t.b);
  }
  if (ctx->own_stream && ctx->st) (void) hipStreamDestroy(ctx->st);
  delete ctx;
}

const char *bk_last_error(const bk_ctx *ctx) { return ctx ? ctx->err.c_str() : g_init_error.c_str(); }

int bk_set_stream(bk_ctx *ctx, void *hip_stream)
{
  return guarded(ctx, [&] {
    if (ctx->own_stream && ctx->st) HIP_CHECK(hipStreamDestroy(ctx->st));
    ctx->st = (hipStream_t) hip_stream;
    ctx->own_stream = false;
  });
}
int bk_get_stream(bk_ctx *ctx, void **hip_stream)
{
  return guarded(ctx, [&] {
    if (!hip_stream) throw bk_error(BK_ERR_ARG, "bk_get_stream: null output");
    *hip_stream = (void *) ctx->st;
  });
}
int bk_sync(bk_ctx *ctx)
{
  return guarded(ctx, [&] { HIP_CHECK(hipStreamSynchronize(ctx->st)); });
}

int bk_records(bk_ctx *ctx, bk_soa *cols)
{
  return guarded(ctx, [&] {
    if (!cols) throw bk_error(BK_ERR_ARG, "bk_records: null output");
    if (!ctx->have_records) throw bk_error(BK_ERR_ARG, "bk_records: the context holds no record table");
    HIP_CHECK(hipStreamSynchronize(ctx->st));
    *cols = ctx->rec;
  });
}

int bk_upload_records(bk_ctx *ctx, const bk_soa *s, int mem_space)
{
  return guarded(ctx, [&] {
    if (!s) throw bk_error(BK_ERR_ARG, "bk_upload_records: null table");
    if (s->n > 0xFFFFFFF0ull) throw bk_error(BK_ERR_LIMIT, "more than 2^32 records in one context (shard across GPUs)");
    ctx->stream_done = ctx->stats_done = ctx->clustered = false;
    ctx->joined = ctx->bp_done = ctx->shard = false;
    ctx->sj_claims_valid = false;
    ctx->ext_cand = nullptr;
    ctx->ext_split = nullptr;
    ctx->ext_clusters = nullptr;
    ctx->own_groups.clear();
    ctx->rec_base = 0;
    ctx->streamed = false;
    if (mem_space == BK_MEM_DEVICE)
    {
      // the columns are used in place: they must live on this context's GPU (a table decoded on another device would be
      // read across xGMI, or fault without peer access)
      hipPointerAttribute_t at;
      if (s->n && s->tid && hipPointerGetAttributes(&at, s->tid) == hipSuccess && at.type == hipMemoryTypeDevice && at.device != ctx->device)
        throw bk_error(BK_ERR_ARG, "bk_upload_records: BK_MEM_DEVICE table lives on device " + std::to_string(at.device) + ", context on device " +
                                       std::to_string(ctx->device));
      (void) hipGetLastError();
      // the streaming kernels read the fixed columns as 16-byte vectors (four or eight records per lane)
      for (const void *p : {(const void *) s->tid, (const void *) s->pos, (const void *) s->isize, (const void *) s->flag, (const void *) s->mapq, (const void *) s->cigar_off,
                            (const void *) s->aux_off})
        if (s->n && ((uintptr_t) p & 15u)) throw bk_error(BK_ERR_ARG, "bk_upload_records: BK_MEM_DEVICE columns must be 16-byte aligned");
      if (s->n && s->side && ((uintptr_t) s->side & 15u)) throw bk_error(BK_ERR_ARG, "bk_upload_records: BK_MEM_DEVICE side rows must be 16-byte aligned");
      ctx->rec = *s;
    }
    else
    {
      const uint64_t n = s->n;
      const void *src[13] = {s->tid, s->pos, s->mtid, s->mpos, s->isize, s->flag, s->mapq, s->qhash, s->cigar_off, s->cigar, s->aux_off, s->aux, s->qcheck};
      const size_t bytes[13] = {n * 4, n * 4, n * 4, n * 4, n * 4, n * 2, n, n * 8, (n + 1) * 4, s->n_cigar_words * 4, (n + 1) * 4, s->n_aux_bytes,
                                s->qcheck ? n * 4 : 0};
      void *dst[13];
      for (int k = 0; k < 13; ++k)
      {
        dst[k] = ctx->col[k].ensure(bytes[k] + 16);
        if (bytes[k]) HIP_CHECK(hipMemcpyAsync(dst[k], src[k], bytes[k], hipMemcpyHostToDevice, ctx->st));
      }
      HIP_CHECK(hipStreamSynchronize(ctx->st));
      bk_soa d = *s;
      d.tid = (const int32_t *) dst[0]; d.pos = (const int32_t *) dst[1]; d.mtid = (const int32_t *) dst[2]; d.mpos = (const int32_t *) dst[3];
      d.isize = (const int32_t *) dst[4]; d.flag = (const uint16_t *) dst[5]; d.mapq = (const uint8_t *) dst[6]; d.qhash = (const uint64_t *) dst[7];
      d.cigar_off = (const uint32_t *) dst[8]; d.cigar = (const uint32_t *) dst[9]; d.aux_off = (const uint32_t *) dst[10]; d.aux = (const uint8_t *) dst[11];
      d.qcheck = s->qcheck ? (const uint32_t *) dst[12] : nullptr;
      // the side layout for the streaming pass (one 32-byte row per record, include/breakid_hip.h: bk_side), made on the device
      bk_side *side = ctx->d_side.as<bk_side>(n + 1);
      launch_make_side(d.qhash, d.mtid, d.mpos, d.qcheck, n, side, ctx->st);
      d.side = side;
      ctx->rec = d;
    }
    ctx->have_records = true;
  });
}

int bk_exclude_regions(bk_ctx *ctx, const bk_regions *r, uint64_t *n_removed)
{
  return guarded(ctx, [&] {
    if (!ctx->have_records || ctx->streamed || ctx->shard)
      throw bk_error(BK_ERR_ARG, "bk_exclude_regions: call it after bk_upload_records and before the stream pass (bk_isize_stats, bk_shard_begin, "
                                 "or a context of bk_bam_decode_device_ctx)");
    if (!r || (r->n && (!r->tid || !r->beg || !r->end))) throw bk_error(BK_ERR_ARG, "bk_exclude_regions: null interval list");
    const bk_soa &s = ctx->rec;
    if (s.n && (!s.tid || !s.pos || !s.mtid || !s.mpos || !s.isize || !s.flag || !s.mapq || !s.qhash || !s.cigar_off || !s.aux_off))
      throw bk_error(BK_ERR_ARG, "bk_exclude_regions: the table lacks a column");
    // merged per contig on the host: sorted by start, overlapping and touching intervals joined (their ends are sorted then too)
    std::vector<std::vector<std::pair<int32_t, int32_t>>> by(ctx->nt);
    for (uint64_t k = 0; k < r->n; ++k)
    {
      const int32_t t = r->tid[k], b = r->beg[k], e = r->end[k];
      if (t < 0 || t >= ctx->nt || b < 0 || e <= b)
        throw bk_error(BK_ERR_ARG, "bk_exclude_regions: interval " + std::to_string(k) + " (tid " + std::to_string(t) + ", [" + std::to_string(b) + ", " +
                                       std::to_string(e) + ")): needs 0 <= tid < n_targets, 0 <= beg < end");
      by[t].emplace_back(b, e);
    }
    std::vector<uint32_t> off(ctx->nt + 1, 0);
    std::vector<int32_t> beg, end;
    for (int t = 0; t < ctx->nt; ++t)
    {
      auto &v = by[t];
      std::sort(v.begin(), v.end());
      for (auto &iv : v)
        if (beg.size() > off[t] && iv.first <= end.back())
          end.back() = std::max(end.back(), iv.second);
        else
        {
          beg.push_back(iv.first);
          end.push_back(iv.second);
        }
      off[t + 1] = (uint32_t) beg.size();
    }
    const bool owned = s.tid && s.tid == ctx->col[0].get<int32_t>();  // (a host upload, or a table this call made before)
    if (beg.empty() && owned)
    {
      // nothing to take out, and the context already owns its columns
      if (n_removed) *n_removed = 0;
      return;
    }
    DevBuf d_off, d_beg, d_end;
    ExclRegions rg;
    rg.n_targets = ctx->nt;
    rg.off = d_off.as<uint32_t>(off.size());
    rg.beg = d_beg.as<int32_t>(beg.size() + 1);
    rg.end = d_end.as<int32_t>(end.size() + 1);
    HIP_CHECK(hipMemcpyAsync((void *) rg.off, off.data(), off.size() * 4, hipMemcpyHostToDevice, ctx->st));
    if (!beg.empty())
    {
      HIP_CHECK(hipMemcpyAsync((void *) rg.beg, beg.data(), beg.size() * 4, hipMemcpyHostToDevice, ctx->st));
      HIP_CHECK(hipMemcpyAsync((void *) rg.end, end.data(), end.size() * 4, hipMemcpyHostToDevice, ctx->st));
    }
    bk_soa out;
    const uint64_t n_before = s.n;
    exclude_compact(s, rg, ctx->xcol, out, ctx->st, [&](const char *name, uint64_t bytes, bool begin) { ctx->tick(name ? name : "", bytes, begin, bytes); });
    // the kept table becomes the context's own: the caller's device table is never read again, the columns of a host upload are released
    for (int k = 0; k < 13; ++k)
    {
      std::swap(ctx->col[k], ctx->xcol[k]);
      ctx->xcol[k].release();
    }
    {
      Scope sc(ctx, "make_side", (out.qcheck ? 56ull : 52ull) * out.n, (out.qcheck ? 56ull : 52ull) * out.n);  // qhash, mtid, mpos (qcheck) in, 32-byte rows out
      bk_side *side = ctx->d_side.as<bk_side>(out.n + 1);
      launch_make_side(out.qhash, out.mtid, out.mpos, out.qcheck, out.n, side, ctx->st);
      out.side = side;
    }
    HIP_CHECK(hipStreamSynchronize(ctx->st));
    ctx->rec = out;
    if (n_removed) *n_removed = n_before - out.n;
  });
}

int bk_isize_stats(bk_ctx *ctx, double *mean, double *sd)
{
  return guarded(ctx, [&] {
    if (!ctx->stream_done) run_stream(ctx);
    if (!ctx->stats_done)
    {
      const double n = (double) ctx->hc.isize_n;
      const double m = (double) (long long) ctx->hc.isize_sum / n;  // (double) long / (double) size_t, BreakID.cc:1941
      ctx->mean = m;
      if (ctx->hc.isize_n == 0)
        ctx->sd = std::nan("");
      else
      {
        double sum_d = ctx->hsd.sumsq - 2.0 * m * (double) ctx->hc.isize_sum + n * m * m;
        if (!(sum_d > 0)) sum_d = 0;
        double da = (double) ctx->hsd.vmax - m, dmax = da * da + m * m;
        double bound = 2.0 * sum_d + 2.0 * n + 2.0 * dmax + 4.0;
        int k = std::ilogb(bound) + 1;
        double thr = k >= 51 ? 1.0e300 : std::ldexp(1.0, k - 53);
        {
          Scope s(ctx, "isize_sd", 0, 6ull * ctx->rec.n);  // flag + isize re-read: already credited to the path once (k_stream)
          launch_sd(ctx->rec.flag, ctx->rec.isize, ctx->rec.n, m, thr, ctx->d_sd.get<SdState>(), ctx->sdb, ctx->st);
        }
        HIP_CHECK(hipMemcpyAsync(&ctx->hsd, ctx->d_sd.get<SdState>(), sizeof(SdState), hipMemcpyDeviceToHost, ctx->st));
        HIP_CHECK(hipStreamSynchronize(ctx->st));
        ctx->sd = std::sqrt((double) ctx->hsd.t_final / n);  // sqrt(long / (double) size), :1946
      }
      ctx->stats_done = true;
    }
    if (mean) *mean = ctx->mean;
    if (sd) *sd = ctx->sd;
  });
}

// host-side group tables of ctx->jr and the reference's group order; `all_keys` (sharded sample: the chr-pair keys of
// every rank) makes the cluster/pair `group` ordinals global
static void finish_groups(bk_ctx *ctx, const std::vector<uint32_t> *all_keys)
{
  const uint32_t ng = ctx->jr.n_groups;
  ctx->gkey_host.assign(ng, 0);
  ctx->gstart_host.assign(ng + 1, 0);
  if (ng)
  {
    HIP_CHECK(hipMemcpyAsync(ctx->gkey_host.data(), ctx->jr.gkey, ng * 4, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipMemcpyAsync(ctx->gstart_host.data(), ctx->jr.gstart, (ng + 1) * 8, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipStreamSynchronize(ctx->st));
  }
  // the reference iterates groups in std::map<string> order of "chrA_chrB" (BreakID.cc:93,119)
  auto key_name = [&](uint32_t k) {
    int t1 = (int) (k / (uint32_t) (ctx->nt + 1)) - 1, t2 = (int) (k % (uint32_t) (ctx->nt + 1)) - 1;
    return rname(ctx, t1) + "_" + rname(ctx, t2);
  };
  std::vector<std::string> keys(ng);
  for (uint32_t g = 0; g < ng; ++g) keys[g] = key_name(ctx->gkey_host[g]);
  ctx->lex_to_num.resize(ng);
  std::iota(ctx->lex_to_num.begin(), ctx->lex_to_num.end(), 0u);
  std::sort(ctx->lex_to_num.begin(), ctx->lex_to_num.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  ctx->glex_host.assign(ng, 0);
  if (!all_keys)
    for (uint32_t l = 0; l < ng; ++l) ctx->glex_host[ctx->lex_to_num[l]] = l;
  else
  {
    std::vector<std::string> names;
    names.reserve(all_keys->size());
    for (uint32_t k : *all_keys) names.push_back(key_name(k));
    std::sort(names.begin(), names.end());
    names.erase(std::unique(names.begin(), names.end()), names.end());
    for (uint32_t g = 0; g < ng; ++g)
    {
      auto it = std::lower_bound(names.begin(), names.end(), keys[g]);
      if (it == names.end() || *it != keys[g]) throw bk_error(BK_ERR_ARG, "bk_shard_group_pairs: a local group is missing from the global key list");
      ctx->glex_host[g] = (uint32_t) (it - names.begin());
    }
  }
  uint32_t *dg = ctx->d_glex.as<uint32_t>((uint64_t) ng + 1), *dl = ctx->d_lex_to_num.as<uint32_t>((uint64_t) ng + 1);
  if (ng) HIP_CHECK(hipMemcpyAsync(dg, ctx->glex_host.data(), ng * 4, hipMemcpyHostToDevice, ctx->st));
  if (ng) HIP_CHECK(hipMemcpyAsync(dl, ctx->lex_to_num.data(), ng * 4, hipMemcpyHostToDevice, ctx->st));
  join_assign_ids(ctx->jr, dg, ctx->st);
}

int bk_discordant_pairs(bk_ctx *ctx, int mapq_min, double w, uint64_t *n_pairs, uint32_t *n_groups)
{
  return guarded(ctx, [&] {
    if (!ctx->stream_done || mapq_min != ctx->stream_mapq)
    {
      ctx->mapq_min = mapq_min;
      run_stream(ctx);
    }
    {
      Scope s(ctx, "mate_join");
      // discovery indices are record indices: of this table when the candidates are its own, of the whole sample (up to 64 bits:
      // rec_base + i) when they came from other shards
      ctx->jb.rec_bits = -1;
      if (!ctx->ext_cand && ctx->rec_base == 0)
      {
        int bits = 1;
        while (bits < 32 && (1ull << bits) < ctx->rec.n) ++bits;
        ctx->jb.rec_bits = bits;
      }
      join_candidates(ctx->cand_ptr(), ctx->hc.n_cand, w, ctx->d_tprefix.get<uint32_t>(), ctx->nt, ctx->jb, ctx->st, ctx->jr);
    }
    finish_groups(ctx, nullptr);
    ctx->clustered = false;
    ctx->joined = true;
    ctx->bp_done = false;
    ctx->sj_claims_valid = false;
    ctx->join_w = w;
    if (n_pairs) *n_pairs = ctx->jr.n_pairs;
    if (n_groups) *n_groups = ctx->jr.n_groups;
  });
}

int bk_mask_and_cluster(bk_ctx *ctx, double w, int fast, uint64_t *n_clustered)
{
  return guarded(ctx, [&] {
    // the stage itself, its lanes and its sort service: lanes.hip
    const StageInput in{ctx->device, ctx->st, ctx->jr, ctx->gstart_host, ctx->own_groups,
                        [&](const char *name, const std::function<void()> &body) { Scope s(ctx, name); body(); }};
    ctx->summary_map = false;
    ctx->stage.run(in, w, fast);
    ctx->clustered = true;
    if (n_clustered) *n_clustered = ctx->stage.list.n;
  });
}

int bk_split_evidence(bk_ctx *ctx, uint64_t *n_tuples)
{
  return guarded(ctx, [&] {
    if (!ctx->stream_done) run_stream(ctx);
    ensure_splits_sorted(ctx);
    if (n_tuples) *n_tuples = ctx->hc.n_split;
  });
}

int bk_cluster_summary(bk_ctx *ctx, double w, uint64_t *n_clusters)
{
  return guarded(ctx, [&] {
    if (!ctx->clustered) throw bk_error(BK_ERR_ARG, "bk_cluster_summary: call bk_mask_and_cluster first");
    ctx->bp_done = false;
    ctx->sj_claims_valid = false;
    // (lex_to_num, glex and gkey are tables over the groups of the join; the list's groups are the same ones: lanes.hip)
    if (ctx->stage.list.ng != ctx->jr.n_groups) throw bk_error(BK_ERR_HIP, "bk_cluster_summary: the clustered list and the join disagree on the groups (internal error)");
    Scope s(ctx, "cluster_summary");
    ctx->n_clusters = cluster_summary(ctx->jr.pairs, ctx->stage.list.idx.get<uint32_t>(), ctx->stage.list.gof.get<uint32_t>(), ctx->stage.d_cluster.get<uint32_t>(), ctx->stage.list.n,
                                      ctx->stage.list.ng, ctx->jr.gkey, ctx->d_glex.get<uint32_t>(), ctx->d_lex_to_num.get<uint32_t>(), ctx->nt, w, ctx->d_clusters, ctx->bb, ctx->st);
    ctx->summary_map = true;
    if (n_clusters) *n_clusters = ctx->n_clusters;
  });
}

int bk_split_breakpoints(bk_ctx *ctx, double w, uint64_t *n_valid)
{
  return guarded(ctx, [&] {
    ensure_splits_sorted(ctx);
    RecView r;
    r.n = ctx->rec.n;
    r.tid = ctx->rec.tid; r.pos = ctx->rec.pos; r.flag = ctx->rec.flag; r.mapq = ctx->rec.mapq;
    r.cigar_off = ctx->rec.cigar_off; r.cigar = ctx->rec.cigar;
    {
      Scope s(ctx, "split_breakpoints");
      split_breakpoints(r, ctx->d_split.get<bk_split>(), ctx->hc.n_split, ctx->clusters_ptr(), ctx->n_clusters, w, (int) ctx->hc.max_span,
                        ctx->d_hdr.get<int32_t>(), ctx->bb, ctx->st);
    }
    ctx->bp_done = true;
    ctx->sj_claims_valid = false;
    if (n_valid) *n_valid = count_valid_clusters(ctx->clusters_ptr(), ctx->n_clusters, ctx->bb, ctx->st);
  });
}

// ---- the frame of the per-call outputs (bk_normal_support, bk_ref_support, bk_junctions, bk_evidence) -----------------------------
// Each runs one wave per row of the device cluster table and returns one row per call.  The table is in BK_STAGE_CLUSTERS order
// (bp.hip, cluster_summary), so the rows go to the caller as the kernels wrote them.
static TupleTable tuple_table(const bk_ctx *ctx)
{
  return TupleTable{ctx->d_split.get<bk_split>(), ctx->hc.n_split, (int) ctx->hc.max_span, ctx->d_hdr.get<int32_t>(), ctx->names.own_id, ctx->nt, ctx->names.empty_id};
}
// the clustered list and the slot -> row map of the last bk_cluster_summary
static JunctionPairs junction_pairs(const bk_ctx *ctx)
{
  JunctionPairs jp{};
  if (ctx->n_clusters)  // (no cluster: bk_cluster_summary may have returned before it built the map)
  {
    jp.pairs = ctx->jr.pairs;
    jp.idx = ctx->stage.list.idx.get<uint32_t>();
    jp.gof = ctx->stage.list.gof.get<uint32_t>();
    jp.cl = ctx->stage.d_cluster.get<uint32_t>();
    jp.n = ctx->stage.list.n;
    jp.ng = ctx->stage.list.ng;
    jp.slotbase = ctx->bb.slotbase.get<uint32_t>();
    jp.keep = ctx->bb.keep.get<uint32_t>();
    jp.off = ctx->bb.off.get<uint32_t>();
  }
  return jp;
}
// two contexts of one call: the same device and the same reference list
static void require_same_reference(const std::string &who, const char *role_a, const bk_ctx *a, const char *role_b, const bk_ctx *b)
{
  if (b->device != a->device)
    throw bk_error(BK_ERR_ARG, who + ": " + role_a + " (device " + std::to_string(a->device) + ") and " + role_b + " (device " + std::to_string(b->device) +
                                   ") contexts are on different devices");
  if (b != a && (b->nt != a->nt || b->tname != a->tname || b->tlen != a->tlen))
    throw bk_error(BK_ERR_ARG, who + ": " + role_a + " and " + role_b + " reference lists differ (names or lengths)");
}

int bk_normal_support(bk_ctx *tumor, bk_ctx *normal, double w, const struct bk_normal_support **out, uint64_t *count)
{
  if (!normal) return guarded(tumor, [&] { throw bk_error(BK_ERR_ARG, "bk_normal_support: null normal context"); });
  return guarded(tumor, [&] {
    if (!out || !count) throw bk_error(BK_ERR_ARG, "bk_normal_support: null output");
    if (tumor->shard || normal->shard) throw bk_error(BK_ERR_ARG, "bk_normal_support: sharded contexts (bk_shard_*) are not supported");
    if (!tumor->bp_done) throw bk_error(BK_ERR_ARG, "bk_normal_support: call bk_split_breakpoints on the tumour context first");
    if (!normal->stats_done || !normal->joined || !normal->splits_sorted)
      throw bk_error(BK_ERR_ARG, "bk_normal_support: call bk_isize_stats, bk_discordant_pairs and bk_split_evidence on the normal context first");
    if (tumor->join_w != w) throw bk_error(BK_ERR_ARG, "bk_normal_support: w is not the tumour's distance (its bk_discordant_pairs w)");
    if (normal->stream_mapq != tumor->stream_mapq || normal->join_w != w)
      throw bk_error(BK_ERR_ARG, "bk_normal_support: the normal's bk_discordant_pairs must use the tumour's mapq_min and w");
    require_same_reference("bk_normal_support", "tumour", tumor, "normal", normal);
    Scope s(tumor, "normal_support");
    HIP_CHECK(hipStreamSynchronize(normal->st));  // the normal's stages ran on its own stream
    const NormalSide ns{normal->jr.pairs, normal->jr.n_pairs, tuple_table(normal), rec_view(normal)};
    const uint64_t ncl = tumor->n_clusters;
    struct bk_normal_support *d_res;
    normal_support(ns, tumor->clusters_ptr(), ncl, w, tumor->nb, tumor->st, &d_res);
    rows_to_host(tumor, d_res, ncl, tumor->f_normal);
    *out = tumor->f_normal.data();
    *count = ncl;
  });
}

int bk_ref_support(bk_ctx *calls, bk_ctx *records, int mapq_min, int anchor, double w, const struct bk_ref_support **out, uint64_t *count)
{
  if (!records) return guarded(calls, [&] { throw bk_error(BK_ERR_ARG, "bk_ref_support: null records context"); });
  return guarded(calls, [&] {
    if (!out || !count) throw bk_error(BK_ERR_ARG, "bk_ref_support: null output");
    if (calls->shard || records->shard) throw bk_error(BK_ERR_ARG, "bk_ref_support: sharded contexts (bk_shard_*) are not supported");
    if (!calls->bp_done) throw bk_error(BK_ERR_ARG, "bk_ref_support: call bk_split_breakpoints on the calls context first");
    if (!records->have_records || !records->stats_done) throw bk_error(BK_ERR_ARG, "bk_ref_support: call bk_isize_stats on the records context first");
    if (anchor < 0) throw bk_error(BK_ERR_ARG, "bk_ref_support: anchor must not be negative");
    if (mapq_min < 0) throw bk_error(BK_ERR_ARG, "bk_ref_support: mapq_min must not be negative");
    if (!(w >= 0.0 && w < 2147483648.0)) throw bk_error(BK_ERR_ARG, "bk_ref_support: w is out of range");
    require_same_reference("bk_ref_support", "calls", calls, "records", records);
    const bk_soa &t = records->rec;
    if (t.n && (!t.tid || !t.pos || !t.isize || !t.flag || !t.mapq || !t.cigar_off || !t.aux_off))
      throw bk_error(BK_ERR_ARG, "bk_ref_support: the record table lacks a column");
    const uint64_t ncl = calls->n_clusters;
    if (records != calls) HIP_CHECK(hipStreamSynchronize(records->st));  // its stages ran on its own stream
    struct bk_ref_support *d_res;
    RefStat *d_stat = nullptr;
    {
      Scope s(calls, "ref_support");  // the device work alone: the copies below would hide it
      ref_support(rec_view(records), (int) records->hc.max_span, calls->clusters_ptr(), ncl, mapq_min, anchor, w, calls->rb, calls->st, &d_res,
                  calls->timing ? &d_stat : nullptr);
    }
    std::vector<RefStat> stat(d_stat ? 2 * ncl : 0);
    if (!stat.empty()) HIP_CHECK(hipMemcpyAsync(stat.data(), d_stat, 2 * ncl * sizeof(RefStat), hipMemcpyDeviceToHost, calls->st));
    rows_to_host(calls, d_res, ncl, calls->f_ref);
    if (calls->timing && !calls->timers.empty())
    {
      // bytes: pos, flag, mapq, isize and two aux_off words of every record of a window (19 B each; bytes / 19 = records visited).
      // touched: those, the CIGAR words that were walked, and per call two bk_cluster reads (one per side) and the row.
      uint64_t visited = 0, words = 0;
      for (const RefStat &x : stat)
      {
        visited += x.visited;
        words += x.words;
      }
      calls->timers.back().bytes = 19ull * visited;
      calls->timers.back().touched = 19ull * visited + 4ull * words + ncl * (2ull * sizeof(bk_cluster) + sizeof(struct bk_ref_support));
    }
    *out = calls->f_ref.data();
    *count = ncl;
  });
}

int bk_clip_support(bk_ctx *calls, bk_ctx *records, int mapq_min, int min_clip, double w, const struct bk_clip_support **out, uint64_t *count)
{
  if (!records) return guarded(calls, [&] { throw bk_error(BK_ERR_ARG, "bk_clip_support: null records context"); });
  return guarded(calls, [&] {
    if (!out || !count) throw bk_error(BK_ERR_ARG, "bk_clip_support: null output");
    if (calls->shard || records->shard) throw bk_error(BK_ERR_ARG, "bk_clip_support: sharded contexts (bk_shard_*) are not supported");
    if (!calls->bp_done) throw bk_error(BK_ERR_ARG, "bk_clip_support: call bk_split_breakpoints on the calls context first");
    if (!records->have_records || !records->stats_done) throw bk_error(BK_ERR_ARG, "bk_clip_support: call bk_isize_stats on the records context first");
    if (min_clip < 1) throw bk_error(BK_ERR_ARG, "bk_clip_support: min_clip must be at least 1");
    if (mapq_min < 0) throw bk_error(BK_ERR_ARG, "bk_clip_support: mapq_min must not be negative");
    if (!(w >= 0.0 && w < 2147483648.0)) throw bk_error(BK_ERR_ARG, "bk_clip_support: w is out of range");
    require_same_reference("bk_clip_support", "calls", calls, "records", records);
    const bk_soa &t = records->rec;
    if (t.n && (!t.tid || !t.pos || !t.flag || !t.mapq || !t.cigar_off || !t.aux_off)) throw bk_error(BK_ERR_ARG, "bk_clip_support: the record table lacks a column");
    const uint64_t ncl = calls->n_clusters;
    if (records != calls) HIP_CHECK(hipStreamSynchronize(records->st));  // its stages ran on its own stream
    struct bk_clip_support *d_res;
    ClipStat *d_stat = nullptr;
    {
      Scope s(calls, "clip_support");  // the device work alone: the copies below would hide it
      clip_support(rec_view(records), (int) records->hc.max_span, calls->clusters_ptr(), ncl, mapq_min, min_clip, w, calls->cb, calls->st, &d_res,
                   calls->timing ? &d_stat : nullptr);
    }
    std::vector<ClipStat> stat(d_stat ? 2 * ncl : 0);
    if (!stat.empty()) HIP_CHECK(hipMemcpyAsync(stat.data(), d_stat, 2 * ncl * sizeof(ClipStat), hipMemcpyDeviceToHost, calls->st));
    rows_to_host(calls, d_res, ncl, calls->f_clip);
    if (calls->timing && !calls->timers.empty())
    {
      // bytes: pos, flag, mapq and two aux_off words of every record a tile looks at (15 B each; bytes / 15 = records visited).
      // touched: those, the CIGAR offsets and words read, and per call two bk_cluster reads (one per side) and the row.
      uint64_t visited = 0, words = 0;
      for (const ClipStat &x : stat)
      {
        visited += x.visited;
        words += x.words;
      }
      calls->timers.back().bytes = 15ull * visited;
      calls->timers.back().touched = 15ull * visited + 4ull * words + ncl * (2ull * sizeof(bk_cluster) + sizeof(struct bk_clip_support));
    }
    *out = calls->f_clip.data();
    *count = ncl;
  });
}

int bk_clip_reads(bk_ctx *records, const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, const uint32_t **counts,
                  const struct bk_clip_read **rows, const uint64_t **site_off)
{
  return guarded(records, [&] {
    if (!counts) throw bk_error(BK_ERR_ARG, "bk_clip_reads: null counts");
    if ((rows == nullptr) != (site_off == nullptr)) throw bk_error(BK_ERR_ARG, "bk_clip_reads: rows and site_off go together (both, or neither for the counts only)");
    if (n_sites && !sites) throw bk_error(BK_ERR_ARG, "bk_clip_reads: null sites");
    if (records->shard) throw bk_error(BK_ERR_ARG, "bk_clip_reads: sharded contexts (bk_shard_*) are not supported");
    if (!records->have_records || !records->stats_done) throw bk_error(BK_ERR_ARG, "bk_clip_reads: call bk_isize_stats first");
    if (min_clip < 1) throw bk_error(BK_ERR_ARG, "bk_clip_reads: min_clip must be at least 1");
    if (mapq_min < 0) throw bk_error(BK_ERR_ARG, "bk_clip_reads: mapq_min must not be negative");
    if (n_sites > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_clip_reads: more than 2^30 sites");
    for (uint64_t k = 0; k < n_sites; ++k)
      if (sites[k].dir > 1u) throw bk_error(BK_ERR_ARG, "bk_clip_reads: site " + std::to_string(k) + " has a dir above 1 (0 = LEFT, 1 = RIGHT)");
    const bool listing = rows != nullptr;
    const bk_soa &t = records->rec;
    if (t.n && (!t.tid || !t.pos || !t.flag || !t.mapq || !t.cigar_off || !t.aux_off)) throw bk_error(BK_ERR_ARG, "bk_clip_reads: the record table lacks a column");
    if (listing && t.n && !t.side && !t.qhash) throw bk_error(BK_ERR_ARG, "bk_clip_reads: a listing needs the read-name hashes: the record table has neither qhash nor side");
    const ClipNames nm{listing ? t.side : nullptr, listing ? t.qhash : nullptr, listing ? t.qcheck : nullptr};
    ClipReadsOut o{};
    {
      Scope s(records, "clip_reads");
      clip_reads(rec_view(records), nm, (int) records->hc.max_span, sites, n_sites, mapq_min, min_clip, listing, records->timing, records->crb, records->st, o);
    }
    if (o.bad) throw bk_error(BK_ERR_HIP, "bk_clip_reads: the listing and the counts disagree (internal error)");
    std::vector<ClipStat> stat(o.stat ? n_sites : 0);
    if (!stat.empty()) HIP_CHECK(hipMemcpyAsync(stat.data(), o.stat, n_sites * sizeof(ClipStat), hipMemcpyDeviceToHost, records->st));
    records->f_cr_off.assign(listing ? n_sites + 1 : 0, 0);
    if (listing) HIP_CHECK(hipMemcpyAsync(records->f_cr_off.data(), o.site_off, (n_sites + 1) * 8, hipMemcpyDeviceToHost, records->st));
    records->f_cr_rows.resize(o.n_rows);
    if (o.n_rows) HIP_CHECK(hipMemcpyAsync(records->f_cr_rows.data(), o.rows, o.n_rows * sizeof(struct bk_clip_read), hipMemcpyDeviceToHost, records->st));
    rows_to_host(records, o.counts, n_sites, records->f_cr_counts);
    if (records->timing && !records->timers.empty())
    {
      // bytes: pos, flag, mapq and two aux_off words of every record a site looks at (15 B each, as clip_support models it), per pass.
      // touched: those, the CIGAR offsets and words read, per site its 16 bytes read and its count (4 + 8 B) written; a listing
      // walks the records a second time, reads the offsets (16 B per site), gathers a 32-byte sector of hashes per row and writes the row.
      uint64_t visited = 0, words = 0;
      for (const ClipStat &x : stat)
      {
        visited += x.visited;
        words += x.words;
      }
      const uint64_t passes = listing && o.n_rows ? 2 : 1;
      records->timers.back().bytes = passes * 15ull * visited;
      records->timers.back().touched = passes * (15ull * visited + 4ull * words + n_sites * sizeof(struct bk_clip_site)) + n_sites * 12ull +
                                       (listing ? n_sites * 16ull + o.n_rows * (32ull + sizeof(struct bk_clip_read)) : 0ull);
    }
    *counts = records->f_cr_counts.data();
    if (listing)
    {
      *rows = records->f_cr_rows.data();
      *site_off = records->f_cr_off.data();
    }
  });
}

int bk_base_depth(bk_ctx *records, const int32_t *tid, const uint32_t *pos, uint64_t n, const uint32_t **out)
{
  return guarded(records, [&] {
    if (!out || (n && (!tid || !pos))) throw bk_error(BK_ERR_ARG, "bk_base_depth: null argument");
    if (records->shard) throw bk_error(BK_ERR_ARG, "bk_base_depth: sharded contexts (bk_shard_*) are not supported");
    if (!records->have_records || !records->stats_done) throw bk_error(BK_ERR_ARG, "bk_base_depth: call bk_isize_stats first");
    const bk_soa &t = records->rec;
    if (t.n && (!t.tid || !t.pos || !t.flag || !t.mapq || !t.cigar_off)) throw bk_error(BK_ERR_ARG, "bk_base_depth: the record table lacks a column");
    records->f_base_depth.assign(n, 0u);
    if (n)
    {
      int32_t *d_tid = records->d_bd_tid.as<int32_t>(n);
      uint32_t *d_pos = records->d_bd_pos.as<uint32_t>(n), *d_out = records->d_bd_out.as<uint32_t>(n);
      HIP_CHECK(hipMemcpyAsync(d_tid, tid, n * 4, hipMemcpyHostToDevice, records->st));
      HIP_CHECK(hipMemcpyAsync(d_pos, pos, n * 4, hipMemcpyHostToDevice, records->st));
      {
        Scope s(records, "base_depth");
        base_depth_at(rec_view(records), d_tid, d_pos, n, (int) records->hc.max_span, records->d_bd_samp, records->st, d_out);
      }
      HIP_CHECK(hipMemcpyAsync(records->f_base_depth.data(), d_out, n * 4, hipMemcpyDeviceToHost, records->st));
      HIP_CHECK(hipStreamSynchronize(records->st));
    }
    *out = records->f_base_depth.data();
  });
}

// The genotype model of one call (include/breakid_hip.h): pure host code, every product rounded on its own (the library is built
// with -ffp-contract=off).
int bk_genotype_call(uint32_t alt, uint32_t ref, uint8_t *gt, uint8_t *gq, float *vaf)
{
  if (!gt || !gq || !vaf) return BK_ERR_ARG;
  if ((uint64_t) alt + ref == 0)
  {
    *gt = 255;
    *gq = 0;
    *vaf = std::numeric_limits<float>::quiet_NaN();
    return BK_OK;
  }
  static const double c[3] = {-0x1.4d104d427de80p+0, -0x1.34413509f79ffp-2, -0x1.6cf9f8b075bd8p-6};  // log10 of 0.05, 0.5, 0.95
  const double k = (double) alt, r = (double) ref;
  double L[3];
  for (int g = 0; g < 3; ++g)
  {
    const double a = k * c[g], b = r * c[2 - g];
    L[g] = a + b;
  }
  int best = 0;
  for (int g = 1; g < 3; ++g)
    if (L[g] > L[best]) best = g;
  int second = -1;
  for (int g = 0; g < 3; ++g)
    if (g != best && (second < 0 || L[g] > L[second])) second = g;
  const double q = std::floor(10.0 * (L[best] - L[second]) + 0.5);
  *gt = (uint8_t) best;
  *gq = (uint8_t) (q < 99.0 ? q : 99.0);
  *vaf = (float) alt / (float) ((uint64_t) alt + ref);
  return BK_OK;
}

int bk_junctions(bk_ctx *ctx, const struct bk_junction **out, uint64_t *count)
{
  return guarded(ctx, [&] {
    if (!out || !count) throw bk_error(BK_ERR_ARG, "bk_junctions: null output");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_junctions: sharded contexts (bk_shard_*) are not supported");
    if (!ctx->bp_done || !ctx->clustered || !ctx->summary_map) throw bk_error(BK_ERR_ARG, "bk_junctions: call bk_split_breakpoints first");
    const uint64_t ncl = ctx->n_clusters;
    const JunctionPairs jp = junction_pairs(ctx);
    struct bk_junction *d_res;
    uint32_t *d_vis;
    {
      // bytes: per list entry its three list words and the four mapq / strand bytes of its pair row (a 32-byte sector of the 56-byte
      // row is what the load fetches); touched adds the tuples searched and, per cluster, its row read and the result written
      Scope s(ctx, "junctions", jp.n * (12ull + 4ull));
      junctions(jp, tuple_table(ctx), ctx->clusters_ptr(), ncl, ctx->jnb, ctx->st, &d_res, &d_vis);
    }
    std::vector<uint32_t> vis(ctx->timing ? ncl : 0);
    if (!vis.empty()) HIP_CHECK(hipMemcpyAsync(vis.data(), d_vis, ncl * 4, hipMemcpyDeviceToHost, ctx->st));
    rows_to_host(ctx, d_res, ncl, ctx->f_junction);
    if (ctx->timing && !ctx->timers.empty())
    {
      uint64_t visited = 0;
      for (uint32_t v : vis) visited += v;
      ctx->timers.back().touched = jp.n * (12ull + 32ull) + visited * sizeof(bk_split) + ncl * (sizeof(bk_cluster) + 2ull * sizeof(struct bk_junction) + 4ull);
    }
    *out = ctx->f_junction.data();
    *count = ncl;
  });
}

int bk_evidence(bk_ctx *ctx, const struct bk_evidence **out, uint64_t *count, const uint64_t **call_off)
{
  return guarded(ctx, [&] {
    if (!out || !count || !call_off) throw bk_error(BK_ERR_ARG, "bk_evidence: null output");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_evidence: sharded contexts (bk_shard_*) are not supported");
    if (!ctx->bp_done || !ctx->clustered || !ctx->summary_map) throw bk_error(BK_ERR_ARG, "bk_evidence: call bk_split_breakpoints first");
    const uint64_t ncl = ctx->n_clusters;
    const bk_soa &t = ctx->rec;
    if (ncl && (!ctx->have_records || !t.mapq || (!t.side && !t.qhash))) throw bk_error(BK_ERR_ARG, "bk_evidence: the record table lacks a column");
    const JunctionPairs jp = junction_pairs(ctx);
    EvidenceRecs er{t.n, t.side, t.qhash, t.qcheck, t.mapq};
    struct bk_evidence *d_rows;
    uint64_t *d_off;
    EvidenceStat *d_stat;
    {
      // bytes: what bk_junctions reads (the counts are its own) and, per list entry, its sort key and value written and read once
      Scope s(ctx, "evidence", jp.n * (12ull + 4ull + 2ull * 12ull));
      evidence(jp, tuple_table(ctx), ctx->clusters_ptr(), ncl, er, ctx->evb, ctx->st, &d_rows, &d_off, &d_stat);
    }
    ctx->f_ev_off.assign(ncl + 1, 0);
    EvidenceStat stat{};
    HIP_CHECK(hipMemcpyAsync(ctx->f_ev_off.data(), d_off, (ncl + 1) * 8, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipMemcpyAsync(&stat, d_stat, sizeof stat, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipStreamSynchronize(ctx->st));
    if (stat.bad) throw bk_error(BK_ERR_HIP, "bk_evidence: the listing and the counts of bk_junctions disagree (internal error)");
    const uint64_t n = ctx->f_ev_off[ncl];
    rows_to_host(ctx, d_rows, n, ctx->f_evidence);
    if (ctx->timing && !ctx->timers.empty())
    {
      // touched: the counting pass as in bk_junctions (the tuples are searched twice: counted, then listed; the cluster row is read
      // by both, and per cluster come its tuple count and its two 8-byte counts written: 20 B), the radix passes over the list
      // (8-byte key + 4-byte value, read twice and written once per 8-bit digit), the pair rows gathered (a 56-byte row and a
      // 32-byte sector of the hashes each), and every row written
      uint64_t n_pair_rows = 0;
      for (uint64_t i = 0; i < n; ++i) n_pair_rows += ctx->f_evidence[i].kind == BK_EV_PAIR;
      int bits = 1;
      while ((ncl >> bits) != 0) ++bits;
      const uint64_t passes = (uint64_t) (bits + 7) / 8;
      ctx->timers.back().touched = jp.n * (12ull + 32ull) + 2ull * stat.visited * sizeof(bk_split) + ncl * (2ull * sizeof(bk_cluster) + 2ull * sizeof(struct bk_junction) + 20ull) +
                                   jp.n * (12ull + 12ull + passes * 32ull + 12ull) + n_pair_rows * (64ull + 32ull) + (n - n_pair_rows) * 32ull +
                                   n * sizeof(struct bk_evidence);
    }
    *out = ctx->f_evidence.data();
    *count = n;
    *call_off = ctx->f_ev_off.data();
  });
}

int bk_unique_support(bk_ctx *ctx, const struct bk_unique_support **out, uint64_t *count, const uint64_t **first, uint64_t *n_rows)
{
  return guarded(ctx, [&] {
    if (!out || !count) throw bk_error(BK_ERR_ARG, "bk_unique_support: null output");
    if (!first != !n_rows) throw bk_error(BK_ERR_ARG, "bk_unique_support: first and n_rows go together (both, or both null for the counts alone)");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_unique_support: sharded contexts (bk_shard_*) are not supported");
    if (!ctx->bp_done || !ctx->clustered || !ctx->summary_map) throw bk_error(BK_ERR_ARG, "bk_unique_support: call bk_split_breakpoints first");
    const uint64_t ncl = ctx->n_clusters;
    const bk_soa &t = ctx->rec;
    if (ncl && (!ctx->have_records || !t.mapq || (!t.side && (!t.qhash || !t.mtid || !t.mpos))))
      throw bk_error(BK_ERR_ARG, "bk_unique_support: the record table lacks a column (mtid and mpos, or bk_side rows)");
    const JunctionPairs jp = junction_pairs(ctx);
    EvidenceRecs er{t.n, t.side, t.qhash, t.qcheck, t.mapq, t.mtid, t.mpos};
    const bool listing = first != nullptr;
    struct bk_unique_support *d_res;
    uint64_t *d_first;
    EvidenceStat *d_stat;
    UniqueStat us;
    {
      // bytes: what bk_evidence reads to list the rows, and the four key words of every row written once and read once
      Scope s(ctx, "unique", jp.n * (12ull + 4ull + 2ull * 12ull));
      unique_support(jp, tuple_table(ctx), ctx->clusters_ptr(), ncl, er, listing, ctx->uqb, ctx->st, &d_res, &d_first, &d_stat, &us);
    }
    EvidenceStat stat{};
    HIP_CHECK(hipMemcpyAsync(&stat, d_stat, sizeof stat, hipMemcpyDeviceToHost, ctx->st));
    if (listing)
    {
      ctx->f_uq_first.resize(us.n_rows);
      if (us.n_rows) HIP_CHECK(hipMemcpyAsync(ctx->f_uq_first.data(), d_first, us.n_rows * 8, hipMemcpyDeviceToHost, ctx->st));
    }
    rows_to_host(ctx, d_res, ncl, ctx->f_unique);
    if (stat.bad) throw bk_error(BK_ERR_HIP, "bk_unique_support: the listing and the counts of bk_junctions disagree (internal error)");
    if (ctx->timing && !ctx->timers.empty())
    {
      // touched: the listing as in bk_evidence without the rows written (a row's source is read all the same: a 56-byte pair row or
      // an 88-byte tuple, and a 32-byte sector of the mate columns per split row), the radix passes over the list, then per row:
      // four key words written (32 B) and read for the OR / AND (32 B), per key word that is sorted a gather (8 B read, 8 B
      // written, 4 B index), per radix pass 8-byte key + 4-byte index read twice and written once (36 B), the last pass (index, two
      // rows' key words: 4 + 64 B) and `first`; per call its two offsets read and its row written
      int bits = 1;
      while ((ncl >> bits) != 0) ++bits;
      const uint64_t ev_passes = (uint64_t) (bits + 7) / 8, n = us.n_rows;
      ctx->timers.back().bytes += n * 64ull;
      ctx->timers.back().touched = jp.n * (12ull + 32ull) + 2ull * stat.visited * sizeof(bk_split) + ncl * (2ull * sizeof(bk_cluster) + 2ull * sizeof(struct bk_junction) + 20ull) +
                                   jp.n * (12ull + 12ull + ev_passes * 32ull + 12ull) + n * (64ull + 32ull) +
                                   n * (64ull + us.gathers * 20ull + us.passes * 36ull + 68ull + (listing ? 8ull : 0ull)) + ncl * (32ull + sizeof(struct bk_unique_support));
    }
    *out = ctx->f_unique.data();
    *count = ncl;
    if (listing)
    {
      *first = ctx->f_uq_first.data();
      *n_rows = us.n_rows;
    }
  });
}

int bk_clip_consensus(bk_ctx *ctx, const bk_reads *reads, const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, uint32_t max_len,
                      uint32_t min_depth, const struct bk_consensus **out, const uint8_t **bases, const uint32_t **col_depth)
{
  return guarded(ctx, [&] {
    if (!reads || !out || !bases) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: null reads, out or bases");
    if (n_sites && !sites) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: null sites");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: sharded contexts (bk_shard_*) are not supported");
    if (max_len < 1 || max_len > 256) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: max_len must be 1..256");
    if (min_depth == 0) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: min_depth must be at least 1");
    if (min_clip < 1) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: min_clip must be at least 1");
    if (mapq_min < 0) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: mapq_min must not be negative");
    if (reads->n > 0x100000000ull) throw bk_error(BK_ERR_LIMIT, "bk_clip_consensus: more than 2^32 reads");
    if (n_sites > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_clip_consensus: more than 2^30 sites");
    for (uint64_t k = 0; k < n_sites; ++k)
    {
      if (sites[k].dir > 1u) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: site " + std::to_string(k) + " has a dir above 1 (0 = LEFT, 1 = RIGHT)");
      if (sites[k].tol != 0u) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: site " + std::to_string(k) + " has a tol other than 0");
    }
    const bk_reads &t = *reads;
    if (t.n && (!t.tid || !t.pos || !t.flag || !t.mapq || !t.cigar_off || !t.l_seq || !t.seq_off)) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: the reads table lacks a column");
    for (uint64_t i = 0; i < t.n; ++i)
    {
      if (t.cigar_off[i + 1] < t.cigar_off[i]) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: cigar_off does not ascend at read " + std::to_string(i));
      if (t.seq_off[i + 1] < t.seq_off[i]) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: seq_off does not ascend at read " + std::to_string(i));
      if (t.seq_off[i + 1] - t.seq_off[i] < ((uint64_t) t.l_seq[i] + 1) / 2)
        throw bk_error(BK_ERR_ARG, "bk_clip_consensus: read " + std::to_string(i) + " has fewer seq bytes than (l_seq + 1) / 2");
    }
    if (t.n && ((t.cigar_off[t.n] && !t.cigar) || (t.seq_off[t.n] && !t.seq))) throw bk_error(BK_ERR_ARG, "bk_clip_consensus: the reads table lacks a column");
    struct bk_consensus *d_res;
    uint8_t *d_bases;
    uint32_t *d_depth;
    ConsensusStat *d_stat;
    consensus_upload(t, ctx->cnb, ctx->st);  // (outside the scope: it times the work on the device copy)
    {
      // bytes: the columns of the reads and the sites once, the result once
      const uint64_t words = t.n ? t.cigar_off[t.n] : 0, sbytes = t.n ? t.seq_off[t.n] : 0;
      Scope s(ctx, "consensus", t.n * 27ull + 12ull + words * 4ull + sbytes + n_sites * (16ull + sizeof(struct bk_consensus) + 5ull * max_len));
      clip_consensus(sites, n_sites, mapq_min, min_clip, max_len, min_depth, ctx->cnb, ctx->st, &d_res, &d_bases, &d_depth, &d_stat);
    }
    ConsensusStat stat{};
    HIP_CHECK(hipMemcpyAsync(&stat, d_stat, sizeof stat, hipMemcpyDeviceToHost, ctx->st));
    const uint64_t cols = n_sites * max_len;
    ctx->f_cons_bases.resize(cols);
    if (cols) HIP_CHECK(hipMemcpyAsync(ctx->f_cons_bases.data(), d_bases, cols, hipMemcpyDeviceToHost, ctx->st));
    if (col_depth)
    {
      ctx->f_cons_depth.resize(cols);
      if (cols) HIP_CHECK(hipMemcpyAsync(ctx->f_cons_depth.data(), d_depth, cols * 4, hipMemcpyDeviceToHost, ctx->st));
    }
    rows_to_host(ctx, d_res, n_sites, ctx->f_cons);
    if (ctx->timing && !ctx->timers.empty())
    {
      // touched: both walks read the fixed columns of every read (tid, flag, mapq, l_seq, two cigar offsets: 19 B) and
      // the CIGAR words they count themselves; a contribution is written once and read once (12 B each way) and gives
      // ceil(min(c, max_len) / 2) bytes of SEQ; per site its slot, key and two offsets, its row and its columns
      ctx->timers.back().touched = 2ull * t.n * 19ull + stat.words * 4ull + stat.contributions * 24ull + stat.seq_bytes +
                                   n_sites * (4ull + 8ull + 16ull + sizeof(struct bk_consensus) + 5ull * max_len);
    }
    *out = ctx->f_cons.data();
    *bases = ctx->f_cons_bases.data();
    if (col_depth) *col_depth = ctx->f_cons_depth.data();
  });
}

// What both calls that take a bk_refseq table refuse it for (include/breakid_hip.h); `who` names the call in the message.  The limit
// is looked at before any array.
static void check_refseq(const bk_refseq &t, const std::string &who)
{
  if (t.n_segs > 0x100000ull) throw bk_error(BK_ERR_LIMIT, who +": more than 2^20 segments");
  if (t.n_segs && (!t.tid || !t.start || !t.len || !t.off)) throw bk_error(BK_ERR_ARG, who + ": the reference table lacks a column");
  for (uint64_t g = 0; g < t.n_segs; ++g)
  {
    if (t.off[g + 1] < t.off[g]) throw bk_error(BK_ERR_ARG, who + ": off does not ascend at segment " + std::to_string(g));
    if (t.off[g + 1] - t.off[g] < ((uint64_t) t.len[g] + 1) / 2)
      throw bk_error(BK_ERR_ARG, who + ": segment " + std::to_string(g) + " has fewer bytes than (len + 1) / 2");
    if (g + 1 < t.n_segs)
    {
      if (t.tid[g + 1] < t.tid[g] || (t.tid[g + 1] == t.tid[g] && t.start[g + 1] < t.start[g]))
        throw bk_error(BK_ERR_ARG, who + ": segment " + std::to_string(g + 1) + " is out of order (the segments ascend by tid, then start)");
      if (t.tid[g + 1] == t.tid[g] && (long long) t.start[g] + (long long) t.len[g] > (long long) t.start[g + 1])
        throw bk_error(BK_ERR_ARG, who + ": segment " + std::to_string(g + 1) + " overlaps the one before it");
    }
  }
  if (t.n_segs && t.off[t.n_segs] && !t.bases) throw bk_error(BK_ERR_ARG, who + ": the reference table lacks a column");
}

int bk_junction_fit(bk_ctx *ctx, const bk_refseq *ref, const struct bk_junction_probe *probes, uint64_t n, const uint8_t *query, uint32_t max_len, uint32_t max_shift,
                    uint32_t max_ins, uint32_t max_hom, const struct bk_junction_fit **out)
{
  return guarded(ctx, [&] {
    if (!ref || !out) throw bk_error(BK_ERR_ARG, "bk_junction_fit: null ref or out");
    if (n && (!probes || !query)) throw bk_error(BK_ERR_ARG, "bk_junction_fit: null probes or query");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_junction_fit: sharded contexts (bk_shard_*) are not supported");
    if (max_len < 1 || max_len > 256) throw bk_error(BK_ERR_ARG, "bk_junction_fit: max_len must be 1..256");
    if (max_shift > 64) throw bk_error(BK_ERR_ARG, "bk_junction_fit: max_shift must be 0..64");
    if (max_ins > 64) throw bk_error(BK_ERR_ARG, "bk_junction_fit: max_ins must be 0..64");
    if (max_hom > 64) throw bk_error(BK_ERR_ARG, "bk_junction_fit: max_hom must be 0..64");
    if (n > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_junction_fit: more than 2^30 probes");
    const bk_refseq &t = *ref;
    check_refseq(t, "bk_junction_fit");
    uint64_t qbytes = 0, walk_bases = 0;
    for (uint64_t k = 0; k < n; ++k)
    {
      const struct bk_junction_probe &p = probes[k];
      if (p.dir_own > 1u || p.dir_mate > 1u) throw bk_error(BK_ERR_ARG, "bk_junction_fit: probe " + std::to_string(k) + " has a dir above 1 (0 = LEFT, 1 = RIGHT)");
      if (p.qlen > max_len) throw bk_error(BK_ERR_ARG, "bk_junction_fit: probe " + std::to_string(k) + " has a qlen above max_len");
      const uint8_t *q = query + k * max_len;
      for (uint32_t j = 0; j < p.qlen; ++j)
        if (q[j] != 'A' && q[j] != 'C' && q[j] != 'G' && q[j] != 'T' && q[j] != 'N')
          throw bk_error(BK_ERR_ARG, "bk_junction_fit: probe " + std::to_string(k) + " has a query byte outside ACGTN in column " + std::to_string(j));
      if (p.qlen >= 1 && p.tid_own >= 0 && p.tid_mate >= 0)
      {
        qbytes += p.qlen;
        walk_bases += 2ull * p.qlen + 2ull * max_shift + 2ull * max_hom;  // the mate walk -(S + H) .. qlen + S - 1, the own walk -H .. qlen - 1
      }
    }
    struct bk_junction_fit *d_res;
    jfit_upload(t, probes, n, query, max_len, ctx->jfb, ctx->st);  // (outside the scope: it times the work on the device copy)
    {
      // bytes: the probes, their queries and the result once; the reference segments once
      Scope s(ctx, "junction_fit", n * (sizeof(struct bk_junction_probe) + sizeof(struct bk_junction_fit) + (uint64_t) max_len) + t.n_segs * 24ull +
                                       (t.n_segs ? t.off[t.n_segs] : 0));
      junction_fit(n, max_len, max_shift, max_ins, max_hom, ctx->jfb, ctx->st, &d_res);
    }
    rows_to_host(ctx, d_res, n, ctx->f_jfit);
    // touched: the probe row, qlen query bytes, the nibbles of both walks and the result row
    if (ctx->timing && !ctx->timers.empty()) ctx->timers.back().touched = n * (sizeof(struct bk_junction_probe) + sizeof(struct bk_junction_fit)) + qbytes + (walk_bases + 1) / 2;
    *out = ctx->f_jfit.data();
  });
}

int bk_locus_similarity(bk_ctx *ctx, const bk_refseq *ref, const struct bk_locus_pair *pairs, uint64_t n, uint32_t flank, const struct bk_locus_sim **out)
{
  return guarded(ctx, [&] {
    if (!ref || !out) throw bk_error(BK_ERR_ARG, "bk_locus_similarity: null ref or out");
    if (n && !pairs) throw bk_error(BK_ERR_ARG, "bk_locus_similarity: null pairs");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_locus_similarity: sharded contexts (bk_shard_*) are not supported");
    if (flank < 1 || flank > 255) throw bk_error(BK_ERR_ARG, "bk_locus_similarity: flank must be 1..255");
    if (n > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_locus_similarity: more than 2^30 pairs");
    const bk_refseq &t = *ref;
    check_refseq(t, "bk_locus_similarity");
    const uint64_t L = 2ull * flank + 1;
    struct bk_locus_sim *d_res;
    locsim_upload(t, pairs, n, ctx->lsb, ctx->st);  // (outside the scope: it times the work on the device copy)
    {
      // bytes: the pairs and the result once; the reference segments once
      Scope s(ctx, "locus_similarity", n * (sizeof(struct bk_locus_pair) + sizeof(struct bk_locus_sim)) + t.n_segs * 24ull + (t.n_segs ? t.off[t.n_segs] : 0));
      locus_similarity(n, flank, ctx->lsb, ctx->st, &d_res);
    }
    rows_to_host(ctx, d_res, n, ctx->f_locsim);
    // touched: the pair row, the result row and L nibbles of each of the two windows
    if (ctx->timing && !ctx->timers.empty()) ctx->timers.back().touched = n * (sizeof(struct bk_locus_pair) + sizeof(struct bk_locus_sim) + L);
    *out = ctx->f_locsim.data();
  });
}

// Short queries searched in a library of sequences (include/breakid_hip.h, seqmatch.hip)
int bk_sequence_match(bk_ctx *ctx, const bk_seq_panel *panel, const struct bk_seq_probe *probes, uint64_t n, const uint8_t *query, uint32_t max_len, uint32_t seed,
                      const struct bk_seq_hit **out)
{
  return guarded(ctx, [&] {
    if (!panel || !out) throw bk_error(BK_ERR_ARG, "bk_sequence_match: null panel or out");
    if (n && (!probes || !query)) throw bk_error(BK_ERR_ARG, "bk_sequence_match: null probes or query");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_sequence_match: sharded contexts (bk_shard_*) are not supported");
    if (max_len < 1 || max_len > 256) throw bk_error(BK_ERR_ARG, "bk_sequence_match: max_len must be 1..256");
    if (seed < 8 || seed > 16) throw bk_error(BK_ERR_ARG, "bk_sequence_match: seed must be 8..16");
    if (n > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_sequence_match: more than 2^30 probes");
    const bk_seq_panel &t = *panel;
    if (t.n_seqs > 0x100000ull) throw bk_error(BK_ERR_LIMIT, "bk_sequence_match: more than 2^20 sequences");
    if (t.n_seqs && !t.off) throw bk_error(BK_ERR_ARG, "bk_sequence_match: null off");
    const uint64_t total = t.n_seqs ? t.off[t.n_seqs] : 0;
    if (total > 0x10000000ull) throw bk_error(BK_ERR_LIMIT, "bk_sequence_match: more than 2^28 panel bases");
    if (t.n_seqs && t.off[0] != 0) throw bk_error(BK_ERR_ARG, "bk_sequence_match: off does not start at 0");
    for (uint64_t s = 0; s < t.n_seqs; ++s)
      if (t.off[s] > t.off[s + 1]) throw bk_error(BK_ERR_ARG, "bk_sequence_match: off does not ascend at sequence " + std::to_string(s));
    if (total && !t.bases) throw bk_error(BK_ERR_ARG, "bk_sequence_match: null bases");
    auto acgtn = [](uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; };
    for (uint64_t i = 0; i < total; ++i)
      if (!acgtn(t.bases[i])) throw bk_error(BK_ERR_ARG, "bk_sequence_match: panel byte " + std::to_string(i) + " is outside ACGTN (lower case is the caller's to fold)");
    for (uint64_t k = 0; k < n; ++k)
    {
      const struct bk_seq_probe &p = probes[k];
      if (p.reversed > 1u) throw bk_error(BK_ERR_ARG, "bk_sequence_match: probe " + std::to_string(k) + " has reversed above 1");
      if (p.qlen > max_len) throw bk_error(BK_ERR_ARG, "bk_sequence_match: probe " + std::to_string(k) + " has a qlen above max_len");
      const uint8_t *q = query + k * max_len;
      for (uint32_t j = 0; j < p.qlen; ++j)
        if (!acgtn(q[j])) throw bk_error(BK_ERR_ARG, "bk_sequence_match: probe " + std::to_string(k) + " has a query byte outside ACGTN in column " + std::to_string(j));
    }
    SeqmatchBufs &b = ctx->smb;
    struct bk_seq_hit *d_res = nullptr;
    seqmatch_upload(t, probes, n, query, max_len, b, ctx->st);  // (outside the scope: it times the work on the device copies)
    {
      // (the two scopes inside push timers of their own, so the whole one ends by its index, not at timers.back(); the model needs
      // the number of k-mers, which is known once the index has run)
      struct Whole
      {
        bk_ctx *c;
        size_t at;
        ~Whole()
        {
          if (c->timing && at < c->timers.size()) (void) hipEventRecord(c->timers[at].b, c->st);
        }
      } whole{ctx, ctx->timers.size()};
      ctx->tick("sequence_match", 0, true, 0);
      uint64_t kmers = 0;
      {
        Scope s(ctx, "sequence_match_index");
        kmers = seqmatch_index(t, seed, b, ctx->st);
      }
      const uint64_t by_index = seqmatch_touched_index(total, kmers, seed), by_probes = seqmatch_touched_probes(n, max_len);
      if (ctx->timing && !ctx->timers.empty()) ctx->timers.back().bytes = ctx->timers.back().touched = by_index;
      {
        Scope s(ctx, "sequence_match_probes", by_probes, by_probes);
        seqmatch_probes(t, n, max_len, seed, b, ctx->st, &d_res);
      }
      if (ctx->timing && whole.at < ctx->timers.size()) ctx->timers[whole.at].bytes = ctx->timers[whole.at].touched = by_index + by_probes;
      if (bk_debug("seqmatch"))
        fprintf(stderr, "bk_sequence_match: %llu probes, %llu sequences, %llu bases, %llu k-mers of %u, %u sort passes\n", (unsigned long long) n, (unsigned long long) t.n_seqs,
                (unsigned long long) total, (unsigned long long) kmers, seed, seqmatch_passes(seed));
    }
    rows_to_host(ctx, d_res, n, ctx->f_seqhit);
    *out = ctx->f_seqhit.data();
  });
}

int bk_site_complexity(bk_ctx *ctx, const bk_refseq *ref, const struct bk_ref_site *sites, uint64_t n, uint32_t flank, uint32_t max_period, const struct bk_site_cplx **out)
{
  return guarded(ctx, [&] {
    if (!ref || !out) throw bk_error(BK_ERR_ARG, "bk_site_complexity: null ref or out");
    if (n && !sites) throw bk_error(BK_ERR_ARG, "bk_site_complexity: null sites");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_site_complexity: sharded contexts (bk_shard_*) are not supported");
    if (flank < 1 || flank > 255) throw bk_error(BK_ERR_ARG, "bk_site_complexity: flank must be 1..255");
    if (max_period < 1 || max_period > 64) throw bk_error(BK_ERR_ARG, "bk_site_complexity: max_period must be 1..64");
    if (n > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_site_complexity: more than 2^30 sites");
    const bk_refseq &t = *ref;
    check_refseq(t, "bk_site_complexity");
    const uint64_t L = 2ull * flank + 1;
    struct bk_site_cplx *d_res;
    seqcx_upload(t, sites, n, ctx->scb, ctx->st);  // (outside the scope: it times the work on the device copy)
    {
      // bytes: the sites and the result once; the reference segments once
      Scope s(ctx, "site_complexity", n * (sizeof(struct bk_ref_site) + sizeof(struct bk_site_cplx)) + t.n_segs * 24ull + (t.n_segs ? t.off[t.n_segs] : 0));
      site_complexity(n, flank, max_period, ctx->scb, ctx->st, &d_res);
    }
    rows_to_host(ctx, d_res, n, ctx->f_sitecx);
    // touched: the site row, the result row and the L nibbles of the window
    if (ctx->timing && !ctx->timers.empty()) ctx->timers.back().touched = n * (sizeof(struct bk_ref_site) + sizeof(struct bk_site_cplx) + L);
    *out = ctx->f_sitecx.data();
  });
}

int bk_window_coverage(bk_ctx *records, const struct bk_cov_window *windows, uint64_t n, int mapq_min, const struct bk_window_cov **out)
{
  return guarded(records, [&] {
    if (!out || (n && !windows)) throw bk_error(BK_ERR_ARG, "bk_window_coverage: null argument");
    if (records->shard) throw bk_error(BK_ERR_ARG, "bk_window_coverage: sharded contexts (bk_shard_*) are not supported");
    if (!records->have_records || !records->stats_done) throw bk_error(BK_ERR_ARG, "bk_window_coverage: call bk_isize_stats first");
    if (mapq_min < 0) throw bk_error(BK_ERR_ARG, "bk_window_coverage: mapq_min must be >= 0");
    if (n > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_window_coverage: more than 2^30 windows");
    for (uint64_t k = 0; k < n; ++k)
      if (windows[k].reserved) throw bk_error(BK_ERR_ARG, "bk_window_coverage: window " + std::to_string(k) + " has a non-zero reserved field");
    const bk_soa &t = records->rec;
    if (t.n && (!t.tid || !t.pos || !t.flag || !t.mapq || !t.cigar_off)) throw bk_error(BK_ERR_ARG, "bk_window_coverage: the record table lacks a column");
    if (t.n_cigar_words && !t.cigar) throw bk_error(BK_ERR_ARG, "bk_window_coverage: the record table lacks a column");
    CovBufs &b = records->cvb;
    struct bk_window_cov *d_res = nullptr;
    if (n) HIP_CHECK(hipMemcpyAsync(b.win.as<struct bk_cov_window>(n), windows, n * sizeof(struct bk_cov_window), hipMemcpyHostToDevice, records->st));
    {
      // the tile sums depend on mapq_min: rebuilt by every call.  touched: flag, mapq, tid and cigar_off of every record and its CIGAR
      // words, the tile arrays, the window and its row (include/breakid_hip.h)
      const uint64_t bytes = t.n * 11ull + t.n_cigar_words * 4ull + cov_tiles(t.n) * 16ull + n * 32ull;
      // (the two scopes inside push timers of their own, so the whole one ends by its index, not at timers.back())
      struct Whole
      {
        bk_ctx *c;
        size_t at;
        ~Whole()
        {
          if (c->timing && at < c->timers.size()) (void) hipEventRecord(c->timers[at].b, c->st);
        }
      } whole{records, records->timers.size()};
      records->tick("window_coverage", bytes, true, bytes);
      {
        Scope s(records, "window_coverage_tiles", 0, t.n * 11ull + t.n_cigar_words * 4ull + cov_tiles(t.n) * 16ull);
        cov_tiles_build(rec_view(records), mapq_min, b, records->st);
      }
      {
        Scope s(records, "window_coverage_windows", 0, n * 32ull);
        window_coverage(rec_view(records), records->nt, (int) records->hc.max_span, n, mapq_min, b, records->st, &d_res);
      }
    }
    rows_to_host(records, d_res, n, records->f_wincov);
    *out = records->f_wincov.data();
  });
}

int bk_window_context(bk_ctx *records, const struct bk_cov_window *windows, uint64_t n, int mapq_min, const struct bk_window_ctx **out)
{
  return guarded(records, [&] {
    if (!out || (n && !windows)) throw bk_error(BK_ERR_ARG, "bk_window_context: null argument");
    if (records->shard) throw bk_error(BK_ERR_ARG, "bk_window_context: sharded contexts (bk_shard_*) are not supported");
    if (!records->have_records) throw bk_error(BK_ERR_ARG, "bk_window_context: the context holds no record table");
    if (mapq_min < 0) throw bk_error(BK_ERR_ARG, "bk_window_context: mapq_min must be >= 0");
    if (n > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_window_context: more than 2^30 windows");
    for (uint64_t k = 0; k < n; ++k)
      if (windows[k].reserved) throw bk_error(BK_ERR_ARG, "bk_window_context: window " + std::to_string(k) + " has a non-zero reserved field");
    const bk_soa &t = records->rec;
    if (t.n && (!t.tid || !t.pos || !t.flag || !t.mapq || !t.cigar_off)) throw bk_error(BK_ERR_ARG, "bk_window_context: the record table lacks a column");
    if (t.n_cigar_words && !t.cigar) throw bk_error(BK_ERR_ARG, "bk_window_context: the record table lacks a column");
    CtxBufs &b = records->cxb;
    struct bk_window_ctx *d_res = nullptr;
    if (n) HIP_CHECK(hipMemcpyAsync(b.win.as<struct bk_cov_window>(n), windows, n * sizeof(struct bk_cov_window), hipMemcpyHostToDevice, records->st));
    {
      // lowq depends on mapq_min: the tile sums are rebuilt by every call.  touched: flag, mapq, tid and cigar_off of every record and two
      // of its CIGAR words, the tile words, the window and its row (include/breakid_hip.h)
      const uint64_t tiles_bytes = t.n * 19ull + ctx_tiles(t.n) * CTX_TILE_BYTES, windows_bytes = n * (sizeof(struct bk_cov_window) + sizeof(struct bk_window_ctx));
      // (the two scopes inside push timers of their own, so the whole one ends by its index, not at timers.back())
      struct Whole
      {
        bk_ctx *c;
        size_t at;
        ~Whole()
        {
          if (c->timing && at < c->timers.size()) (void) hipEventRecord(c->timers[at].b, c->st);
        }
      } whole{records, records->timers.size()};
      records->tick("window_context", tiles_bytes + windows_bytes, true, tiles_bytes + windows_bytes);
      {
        Scope s(records, "window_context_tiles", 0, tiles_bytes);
        ctx_tiles_build(rec_view(records), mapq_min, b, records->st);
      }
      {
        Scope s(records, "window_context_windows", 0, windows_bytes);
        window_context(rec_view(records), records->nt, n, mapq_min, b, records->st, &d_res);
      }
    }
    rows_to_host(records, d_res, n, records->f_winctx);
    *out = records->f_winctx.data();
  });
}

// What bk_fusion_frame refuses a model for (include/breakid_hip.h).  The limits are looked at before any array.
static void check_txmodel(const bk_txmodel &t)
{
  const std::string who = "bk_fusion_frame: ";
  if (t.n_tx > 0x1000000ull) throw bk_error(BK_ERR_LIMIT, who + "more than 2^24 transcripts");
  if (t.n_parts > 0x10000000ull) throw bk_error(BK_ERR_LIMIT, who + "more than 2^28 coding parts");
  if (!t.n_tx) return;
  if (!t.tid || !t.tx_start || !t.tx_end || !t.strand || !t.ex_off || (t.n_parts && (!t.ex_start || !t.ex_end))) throw bk_error(BK_ERR_ARG, who + "the model lacks a column");
  if (t.ex_off[0] != 0 || t.ex_off[t.n_tx] != t.n_parts) throw bk_error(BK_ERR_ARG, who + "ex_off does not run from 0 to n_parts");
  for (uint64_t i = 0; i < t.n_tx; ++i)
  {
    const std::string at = "transcript " + std::to_string(i);
    if (t.tid[i] < 0) throw bk_error(BK_ERR_ARG, who + at + " has a negative tid");
    if (t.strand[i] > 1) throw bk_error(BK_ERR_ARG, who + at + " has a strand above 1 (0 = '+', 1 = '-')");
    if (t.tx_end[i] < t.tx_start[i]) throw bk_error(BK_ERR_ARG, who + at + " ends in front of its start");
    if (i + 1 < t.n_tx && (t.tid[i + 1] < t.tid[i] || (t.tid[i + 1] == t.tid[i] && t.tx_start[i + 1] < t.tx_start[i])))
      throw bk_error(BK_ERR_ARG, who + "transcript " + std::to_string(i + 1) + " is out of order (the rows ascend by tid, then tx_start)");
    if (t.ex_off[i + 1] < t.ex_off[i] || t.ex_off[i + 1] > t.n_parts) throw bk_error(BK_ERR_ARG, who + "ex_off does not ascend at " + at);
    for (uint64_t g = t.ex_off[i]; g < t.ex_off[i + 1]; ++g)
    {
      if (t.ex_end[g] <= t.ex_start[g]) throw bk_error(BK_ERR_ARG, who + at + " has an empty or descending coding part");
      if (g > t.ex_off[i] && t.ex_start[g] < t.ex_end[g - 1]) throw bk_error(BK_ERR_ARG, who + at + " has coding parts that descend or overlap");
      if (t.ex_start[g] < t.tx_start[i] || t.ex_end[g] > t.tx_end[i]) throw bk_error(BK_ERR_ARG, who + at + " has a coding part outside [tx_start, tx_end)");
    }
  }
}

int bk_fusion_frame(bk_ctx *ctx, const bk_txmodel *model, const struct bk_frame_site *sites, uint64_t n, const struct bk_frame_call **out)
{
  return guarded(ctx, [&] {
    if (!model || !out) throw bk_error(BK_ERR_ARG, "bk_fusion_frame: null model or out");
    if (n && !sites) throw bk_error(BK_ERR_ARG, "bk_fusion_frame: null sites");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_fusion_frame: sharded contexts (bk_shard_*) are not supported");
    if (n > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_fusion_frame: more than 2^30 sites");
    const bk_txmodel &t = *model;
    check_txmodel(t);
    for (uint64_t k = 0; k < n; ++k)
      if (sites[k].right1 > 1u || sites[k].right2 > 1u) throw bk_error(BK_ERR_ARG, "bk_fusion_frame: site " + std::to_string(k) + " has a right above 1 (0 = LEFT, 1 = RIGHT)");
    struct bk_frame_call *d_res;
    frame_upload(t, sites, n, ctx->frb, ctx->st);  // (outside the scope: it times the work on the device copy)
    {
      // touched (include/breakid_hip.h): the model's columns and what is derived from them once, the site and its row
      const uint64_t bytes = t.n_tx * 21ull + (t.n_tx ? t.n_parts : 0) * 16ull + n * (sizeof(struct bk_frame_site) + sizeof(struct bk_frame_call));
      Scope s(ctx, "fusion_frame", bytes, bytes);
      frame_derive(t, ctx->frb, ctx->st);
      fusion_frame(n, ctx->frb, ctx->st, &d_res);
    }
    rows_to_host(ctx, d_res, n, ctx->f_frame);
    *out = ctx->f_frame.data();
  });
}

int bk_link_calls(bk_ctx *ctx, const struct bk_link_site *sites, uint64_t n, uint32_t max_dist, const struct bk_call_link **out)
{
  return guarded(ctx, [&] {
    if (!out) throw bk_error(BK_ERR_ARG, "bk_link_calls: null out");
    if (n && !sites) throw bk_error(BK_ERR_ARG, "bk_link_calls: null sites");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_link_calls: sharded contexts (bk_shard_*) are not supported");
    if (max_dist > BK_LINK_MAX_DIST) throw bk_error(BK_ERR_ARG, "bk_link_calls: max_dist above " + std::to_string(BK_LINK_MAX_DIST));
    if (n > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_link_calls: more than 2^30 sites");
    LinkShape shape;
    shape.n = n;
    for (uint64_t k = 0; k < n; ++k)
    {
      if (sites[k].right1 > 1u || sites[k].right2 > 1u) throw bk_error(BK_ERR_ARG, "bk_link_calls: site " + std::to_string(k) + " has a right above 1 (0 = LEFT, 1 = RIGHT)");
      for (const int32_t tid : {sites[k].tid1, sites[k].tid2})
        if (tid >= 0)
        {
          ++shape.m;
          if (tid > shape.max_tid) shape.max_tid = tid;
        }
    }
    struct bk_call_link *d_res;
    uint32_t rounds;
    link_upload(sites, n, ctx->lkb, ctx->st);  // (outside the scope: it times the work on the device copy)
    {
      // touched (include/breakid_hip.h): the site and its row, and per breakend the sort passes and what the runs and events keep
      const uint64_t bytes = shape.touched();
      Scope s(ctx, "link_calls", bytes, bytes);
      link_calls(shape, max_dist, ctx->lkb, ctx->st, &d_res, &rounds);
    }
    if (bk_debug("link")) fprintf(stderr, "bk_link_calls: %llu sites, %llu breakends with a contig, %d key bits, %u rounds of label propagation\n", (unsigned long long) n, (unsigned long long) shape.m, shape.key_bits(), rounds);
    rows_to_host(ctx, d_res, n, ctx->f_link);
    *out = ctx->f_link.data();
  });
}

int bk_locus_partners(bk_ctx *ctx, const struct bk_partner_site *sites, uint64_t n, uint32_t max_gap, const struct bk_locus_partners **out)
{
  return guarded(ctx, [&] {
    if (!out) throw bk_error(BK_ERR_ARG, "bk_locus_partners: null out");
    if (n && !sites) throw bk_error(BK_ERR_ARG, "bk_locus_partners: null sites");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_locus_partners: sharded contexts (bk_shard_*) are not supported");
    if (!ctx->joined) throw bk_error(BK_ERR_ARG, "bk_locus_partners: call bk_discordant_pairs first");
    if (n > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_locus_partners: more than 2^30 sites");
    for (uint64_t k = 0; k < n; ++k)
      if (sites[k].reserved[0] || sites[k].reserved[1]) throw bk_error(BK_ERR_ARG, "bk_locus_partners: site " + std::to_string(k) + " has a non-zero reserved field");
    PartnerBufs &b = ctx->ptb;
    const uint64_t np = ctx->jr.n_pairs;
    struct bk_locus_partners *d_res = nullptr;
    partners_upload(sites, n, b, ctx->st);  // (outside the scope: it times the work on the device copy)
    {
      // (the two scopes inside push timers of their own, so the whole one ends by its index, not at timers.back(); the model needs
      // the elsewhere rows, which are known once the count has run)
      struct Whole
      {
        bk_ctx *c;
        size_t at;
        ~Whole()
        {
          if (c->timing && at < c->timers.size()) (void) hipEventRecord(c->timers[at].b, c->st);
        }
      } whole{ctx, ctx->timers.size()};
      ctx->tick("locus_partners", 0, true, 0);
      {
        Scope s(ctx, "locus_partners_index", 0, partners_touched_index(np));
        partners_index(ctx->jr.pairs, np, ctx->nt, b, ctx->st);
      }
      {
        const size_t at = ctx->timers.size();
        Scope s(ctx, "locus_partners_sites");
        const uint64_t rows = partners_count(ctx->nt, n, b, ctx->st);
        if (rows > 0xFFFFFFF0ull) throw bk_error(BK_ERR_LIMIT, "bk_locus_partners: " + std::to_string(rows) + " ends go elsewhere, more than the 2^32 - 16 rows a sort takes");
        partners_rows(ctx->nt, n, rows, max_gap, b, ctx->st, &d_res);
        if (ctx->timing && at < ctx->timers.size())
        {
          ctx->timers[at].touched = partners_touched_sites(ctx->nt, n, rows);
          ctx->timers[whole.at].bytes = ctx->timers[whole.at].touched = partners_touched_index(np) + ctx->timers[at].touched;
        }
        if (bk_debug("partners")) fprintf(stderr, "bk_locus_partners: %llu sites, %llu ends in the index, %llu rows elsewhere, %u sort passes over them\n", (unsigned long long) n, (unsigned long long) (2 * np), (unsigned long long) rows, partners_row_passes(ctx->nt, n));
      }
    }
    rows_to_host(ctx, d_res, n, ctx->f_partners);
    *out = ctx->f_partners.data();
  });
}

// The two sites of one call (include/breakid_hip.h): pure host code.
int bk_call_partner_sites(const bk_cluster *c, double w, struct bk_partner_site out[2])
{
  if (!c || !out) return BK_ERR_ARG;
  const long long W = (int) w;
  const int32_t tid[2] = {c->p1_tid, c->p2_tid};
  const uint32_t lo[2] = {c->p1_min, c->p2_min}, hi[2] = {c->p1_max, c->p2_max};
  uint32_t beg[2], end[2];
  for (int s = 0; s < 2; ++s)
  {
    long long a = (long long) lo[s] - W, b = (long long) hi[s] + W;
    if (a < 1) a = 1;
    if (a > 0xFFFFFFFFll) a = 0xFFFFFFFFll;
    if (b > 0xFFFFFFFFll) b = 0xFFFFFFFFll;
    if (b < a) a = 1, b = 0;
    beg[s] = (uint32_t) a, end[s] = (uint32_t) b;
  }
  for (int s = 0; s < 2; ++s) out[s] = bk_partner_site{tid[s], beg[s], end[s], tid[1 - s], beg[1 - s], end[1 - s], {0u, 0u}};
  return BK_OK;
}

int bk_fragment_sizes(bk_ctx *ctx, const struct bk_frag_site *sites, uint64_t n, int32_t lo, int32_t hi, const struct bk_frag_sizes **out)
{
  return guarded(ctx, [&] {
    if (!out) throw bk_error(BK_ERR_ARG, "bk_fragment_sizes: null out");
    if (n && !sites) throw bk_error(BK_ERR_ARG, "bk_fragment_sizes: null sites");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_fragment_sizes: sharded contexts (bk_shard_*) are not supported");
    if (!ctx->bp_done || !ctx->clustered || !ctx->summary_map) throw bk_error(BK_ERR_ARG, "bk_fragment_sizes: call bk_split_breakpoints first");
    const uint64_t ncl = ctx->n_clusters;
    if (n != ncl) throw bk_error(BK_ERR_ARG, "bk_fragment_sizes: " + std::to_string(n) + " sites for " + std::to_string(ncl) + " clusters (one site per BK_STAGE_CLUSTERS row)");
    if (lo > hi) throw bk_error(BK_ERR_ARG, "bk_fragment_sizes: lo above hi");
    for (uint64_t k = 0; k < n; ++k)
    {
      const struct bk_frag_site &s = sites[k];
      if (s.right1 > 1u || s.right2 > 1u || s.skip > 1u) throw bk_error(BK_ERR_ARG, "bk_fragment_sizes: site " + std::to_string(k) + " has a right or a skip above 1");
      for (const uint8_t r : s.reserved)
        if (r) throw bk_error(BK_ERR_ARG, "bk_fragment_sizes: site " + std::to_string(k) + " has a non-zero reserved field");
    }
    const bk_soa &t = ctx->rec;
    if (ncl && (!ctx->have_records || !t.tid || !t.pos || !t.flag || !t.mapq || !t.cigar_off || (t.n_cigar_words && !t.cigar) || (!t.side && !t.qhash)))
      throw bk_error(BK_ERR_ARG, "bk_fragment_sizes: the record table lacks a column");
    const JunctionPairs jp = junction_pairs(ctx);
    EvidenceRecs er{t.n, t.side, t.qhash, t.qcheck, t.mapq};
    FragBufs &b = ctx->fgb;
    struct bk_frag_sizes *d_res;
    FragLen *d_len;
    uint64_t *d_off;
    uint64_t n_rows = 0;
    EvidenceStat *d_ev_stat;
    FragStat *d_stat;
    fragsize_upload(sites, n, b, ctx->st);  // (outside the scope: it times the work on the device copy)
    {
      // bytes: what bk_evidence reads to list the rows
      Scope s(ctx, "fragment_sizes", jp.n * (12ull + 4ull + 2ull * 12ull));
      fragment_sizes(jp, tuple_table(ctx), ctx->clusters_ptr(), ncl, er, rec_view(ctx), lo, hi, b, ctx->st, &d_res, &d_len, &d_off, &n_rows, &d_ev_stat, &d_stat);
    }
    EvidenceStat ev_stat{};
    FragStat stat{};
    HIP_CHECK(hipMemcpyAsync(&ev_stat, d_ev_stat, sizeof ev_stat, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipMemcpyAsync(&stat, d_stat, sizeof stat, hipMemcpyDeviceToHost, ctx->st));
    rows_to_host(ctx, d_res, ncl, ctx->f_fragsize);
    if (ev_stat.bad || stat.bad) throw bk_error(BK_ERR_HIP, "bk_fragment_sizes: the listing and the counts of bk_junctions disagree (internal error)");
    uint64_t used = 0;
    for (const struct bk_frag_sizes &r : ctx->f_fragsize) used += r.n_used;
    if (ctx->timing && !ctx->timers.empty())
    {
      // touched (include/breakid_hip.h): the listing as in bk_evidence without the split rows, then per pair row, per looked-up
      // record, per walked record, per used side and per site
      int bits = 1;
      while ((ncl >> bits) != 0) ++bits;
      const uint64_t ev_passes = (uint64_t) (bits + 7) / 8;
      ctx->timers.back().bytes += n_rows * 120ull;
      ctx->timers.back().touched = jp.n * (12ull + 32ull) + ncl * (sizeof(bk_cluster) + 2ull * sizeof(struct bk_junction) + 20ull) + jp.n * (12ull + 12ull + ev_passes * 32ull + 12ull) +
                                   n_rows * (64ull + 32ull) + n_rows * 120ull + stat.lookups * 80ull + stat.walked * 18ull + 2ull * used * 8ull + ncl * 80ull;
    }
    if (bk_debug("fragsize"))
    {
      fprintf(stderr, "bk_fragment_sizes: %llu sites, %llu pair rows, %llu used, library %d-%d; %llu records looked up, their walks read %llu records, the longest %u, %llu finished by a wavefront\n",
              (unsigned long long) n, (unsigned long long) n_rows, (unsigned long long) used, lo, hi, (unsigned long long) stat.lookups, (unsigned long long) stat.walked, stat.longest,
              (unsigned long long) stat.wave_walks);
      std::vector<FragLen> len(n_rows);
      std::vector<uint64_t> off(ncl + 1, 0);
      if (n_rows) HIP_CHECK(hipMemcpyAsync(len.data(), d_len, n_rows * sizeof(FragLen), hipMemcpyDeviceToHost, ctx->st));
      if (ncl) HIP_CHECK(hipMemcpyAsync(off.data(), d_off, (ncl + 1) * 8, hipMemcpyDeviceToHost, ctx->st));
      HIP_CHECK(hipStreamSynchronize(ctx->st));
      int shown = 0;
      for (uint64_t c = 0; c < ncl && shown < 32; ++c)
      {
        if (sites[c].skip) continue;
        ++shown;
        fprintf(stderr, "  call %llu (%u-%u, %c%c):", (unsigned long long) c, sites[c].pos1, sites[c].pos2, sites[c].right1 ? 'R' : 'L', sites[c].right2 ? 'R' : 'L');
        for (uint64_t i = off[c]; i < off[c + 1] && i < off[c] + 64; ++i)
          if (len[i].mark == FRAG_USED) fprintf(stderr, " %d", len[i].len);
          else fprintf(stderr, " %s", len[i].mark == FRAG_OFF ? "off" : len[i].mark == FRAG_LOST ? "lost" : "?");
        fprintf(stderr, "%s\n", off[c + 1] - off[c] > 64 ? " ..." : "");
      }
    }
    *out = ctx->f_fragsize.data();
  });
}

// The library's bounds (include/breakid_hip.h): pure host code.
int bk_fragment_bounds(double mean, double sd, int32_t *lo, int32_t *hi)
{
  if (!lo || !hi || !std::isfinite(mean) || !std::isfinite(sd) || sd < 0) return BK_ERR_ARG;
  auto clamp = [](double v) { return v >= 2147483647.0 ? (int32_t) 2147483647 : v <= -2147483648.0 ? (int32_t) (-2147483647 - 1) : (int32_t) v; };
  const double three = 3.0 * sd;
  const double a = std::floor(mean - three), b = std::ceil(mean + three);
  *lo = clamp(a < 0 ? 0.0 : a);
  *hi = clamp(b);
  return BK_OK;
}

// Every call against a panel of pairs of intervals (include/breakid_hip.h).
int bk_known_calls(bk_ctx *ctx, const struct bk_known_entry *entries, uint64_t n_entries, const struct bk_known_site *sites, uint64_t n, uint32_t slop, const struct bk_known_call **out)
{
  return guarded(ctx, [&] {
    if (!out) throw bk_error(BK_ERR_ARG, "bk_known_calls: null out");
    if (n && !sites) throw bk_error(BK_ERR_ARG, "bk_known_calls: null sites");
    if (n_entries && !entries) throw bk_error(BK_ERR_ARG, "bk_known_calls: null entries");
    if (ctx->shard) throw bk_error(BK_ERR_ARG, "bk_known_calls: sharded contexts (bk_shard_*) are not supported");
    if (slop > BK_KNOWN_MAX_SLOP) throw bk_error(BK_ERR_ARG, "bk_known_calls: slop above " + std::to_string(BK_KNOWN_MAX_SLOP));
    if (n > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_known_calls: more than 2^30 sites");
    if (n_entries > 0x40000000ull) throw bk_error(BK_ERR_LIMIT, "bk_known_calls: more than 2^30 entries");
    KnownShape shape;
    shape.n = n;
    shape.n_entries = n_entries;
    for (uint64_t k = 0; k < n; ++k)
    {
      if (sites[k].right1 > 1u || sites[k].right2 > 1u) throw bk_error(BK_ERR_ARG, "bk_known_calls: site " + std::to_string(k) + " has a right above 1 (0 = LEFT, 1 = RIGHT)");
      for (const uint8_t r : sites[k].reserved)
        if (r) throw bk_error(BK_ERR_ARG, "bk_known_calls: site " + std::to_string(k) + " has a non-zero reserved field");
    }
    for (uint64_t k = 0; k < n_entries; ++k)
    {
      const struct bk_known_entry &e = entries[k];
      if (e.strand1 > 2u || e.strand2 > 2u) throw bk_error(BK_ERR_ARG, "bk_known_calls: entry " + std::to_string(k) + " has a strand above 2 (0 = unstated, 1 = LEFT, 2 = RIGHT)");
      for (const uint8_t r : e.reserved)
        if (r) throw bk_error(BK_ERR_ARG, "bk_known_calls: entry " + std::to_string(k) + " has a non-zero reserved field");
      const int32_t tid[2] = {e.tid1, e.tid2};
      const uint32_t beg[2] = {e.beg1, e.beg2}, end[2] = {e.end1, e.end2};
      for (int i = 0; i < 2; ++i)
        if (tid[i] >= 0)
        {
          if (end[i] <= beg[i]) throw bk_error(BK_ERR_ARG, "bk_known_calls: entry " + std::to_string(k) + " has an interval with end <= beg");
          ++shape.m;
          if (tid[i] > shape.max_tid) shape.max_tid = tid[i];
        }
      if (e.name > shape.max_name) shape.max_name = e.name;
    }
    KnownBufs &b = ctx->knb;
    struct bk_known_call *d_res = nullptr;
    known_upload(entries, n_entries, sites, n, b, ctx->st);  // (outside the scope: it times the work on the device copies)
    {
      // (the two scopes inside push timers of their own, so the whole one ends by its index, not at timers.back(); the model needs
      // the listed hits, which are known once the count has run)
      struct Whole
      {
        bk_ctx *c;
        size_t at;
        ~Whole()
        {
          if (c->timing && at < c->timers.size()) (void) hipEventRecord(c->timers[at].b, c->st);
        }
      } whole{ctx, ctx->timers.size()};
      ctx->tick("known_calls", 0, true, 0);
      {
        Scope s(ctx, "known_calls_index", shape.touched_index(), shape.touched_index());
        known_index(shape, b, ctx->st);
      }
      {
        const size_t at = ctx->timers.size();
        Scope s(ctx, "known_calls_sites");
        const uint64_t hits = known_count(shape, slop, b, ctx->st, &d_res);
        if (hits > 0xFFFFFFF0ull) throw bk_error(BK_ERR_LIMIT, "bk_known_calls: " + std::to_string(hits) + " listed hits, more than the 2^32 - 16 rows a sort takes");
        known_names(shape, slop, hits, b, ctx->st);
        if (ctx->timing && at < ctx->timers.size())
        {
          ctx->timers[at].bytes = ctx->timers[at].touched = shape.touched_sites(hits);
          ctx->timers[whole.at].bytes = ctx->timers[whole.at].touched = shape.touched_index() + shape.touched_sites(hits);
        }
        if (bk_debug("known"))
          fprintf(stderr, "bk_known_calls: %llu sites, %llu entries, %llu intervals with a contig, %u index passes, %llu listed hits, %u name passes\n", (unsigned long long) n,
                  (unsigned long long) n_entries, (unsigned long long) shape.m, shape.index_passes(), (unsigned long long) hits, shape.name_passes());
      }
    }
    rows_to_host(ctx, d_res, n, ctx->f_known);
    *out = ctx->f_known.data();
  });
}

// Junction calls from the split-evidence tuples alone (include/breakid_hip.h, sjcall.hip).  `rows` (null: the context's own voted rows,
// once bk_split_breakpoints has run) is the cluster table in which the claimed row is looked up.
static void sj_claim_table(const bk_cluster *cl, uint64_t n, std::vector<SjClaim> &claims)
{
  // the voted rows' exact breakpoints, both orientations, sorted: they are few
  claims.clear();
  for (uint64_t r = 0; r < n && r < 0x40000000ull; ++r)
  {
    const bk_cluster &c = cl[r];
    if (!(c.flags & 2u) || c.p1_tid < 0 || c.p2_tid < 0 || c.p2_exact < 0) continue;
    claims.push_back(SjClaim{((uint64_t) (c.p1_tid + 1) << 32) | c.p1_exact, c.p2_tid, (uint32_t) c.p2_exact, (uint32_t) (2 * r), 0});
    claims.push_back(SjClaim{((uint64_t) (c.p2_tid + 1) << 32) | (uint32_t) c.p2_exact, c.p1_tid, c.p1_exact, (uint32_t) (2 * r + 1), 0});
  }
  std::sort(claims.begin(), claims.end(), [](const SjClaim &a, const SjClaim &b) { return a.key != b.key ? a.key < b.key : a.code < b.code; });
}

static void sj_run(bk_ctx *ctx, const std::string &who, int mapq_min, uint32_t tol, uint32_t min_reads, const bk_cluster *rows, uint64_t n_rows, bool own_rows,
                   const struct bk_split_junction **out, uint64_t *count)
{
  if (!out || !count) throw bk_error(BK_ERR_ARG, who + ": null output");
  if (ctx->shard) throw bk_error(BK_ERR_ARG, who + ": sharded contexts (bk_shard_*) are not supported");
  if (!ctx->stream_done || !ctx->splits_sorted) throw bk_error(BK_ERR_ARG, who + ": call bk_split_evidence first");
  if (mapq_min < 0) throw bk_error(BK_ERR_ARG, who + ": mapq_min below 0");
  if (tol > BK_SJ_MAX_TOL) throw bk_error(BK_ERR_ARG, who + ": tol above " + std::to_string(BK_SJ_MAX_TOL));
  if (min_reads == 0) throw bk_error(BK_ERR_ARG, who + ": min_reads must be at least 1");
  if (!own_rows && n_rows && !rows) throw bk_error(BK_ERR_ARG, who + ": null rows");
  if (ctx->nt > 0x40000000) throw bk_error(BK_ERR_LIMIT, who + ": more than 2^30 reference sequences (the group key takes two contig numbers and two sides in 64 bits)");
  SjInput in;
  in.split = ctx->d_split.get<bk_split>();
  in.n = ctx->hc.n_split;
  in.flag = ctx->rec.flag;
  in.mapq = ctx->rec.mapq;
  in.n_rec = ctx->rec.n;
  in.tprefix = ctx->d_tprefix.get<uint32_t>();
  in.nt = ctx->nt;
  for (const uint32_t l : ctx->tlen) in.max_len = std::max(in.max_len, l);
  if (in.n && (!ctx->have_records || !in.flag || !in.mapq)) throw bk_error(BK_ERR_ARG, who + ": the record table lacks a column");
  std::vector<SjClaim> given;
  const std::vector<SjClaim> *claims = &given;
  if (!own_rows)
    sj_claim_table(rows, n_rows, given);
  else if (ctx->bp_done)
  {
    // the context's own table: fetched and sorted once, kept until the breakpoint stage runs again
    if (!ctx->sj_claims_valid)
    {
      std::vector<bk_cluster> cl;
      rows_to_host(ctx, ctx->clusters_ptr(), ctx->n_clusters, cl);
      sj_claim_table(cl.data(), cl.size(), ctx->sj_claims);
      ctx->sj_claims_valid = true;
    }
    claims = &ctx->sj_claims;
  }
  struct bk_split_junction *d_rows;
  ctx->sj_stats = SjStats{};
  {
    Scope s(ctx, "split_junctions");
    split_junctions(in, mapq_min, tol, min_reads, claims->data(), claims->size(), ctx->sjb, ctx->st, &d_rows, &ctx->sj_stats);
  }
  if (ctx->timing && !ctx->timers.empty()) ctx->timers.back().bytes = ctx->timers.back().touched = ctx->sj_stats.touched();  // (include/breakid_hip.h)
  const SjStats &t = ctx->sj_stats;
  if (bk_debug("sj"))
    fprintf(stderr, "%s: %llu tuples, %llu eligible, %llu exact, %llu calls, %llu rounds of label propagation, %llu returned\n", who.c_str(), (unsigned long long) t.n,
            (unsigned long long) t.eligible, (unsigned long long) t.exact, (unsigned long long) t.calls, (unsigned long long) t.rounds, (unsigned long long) t.written);
  rows_to_host(ctx, d_rows, t.written, ctx->f_sj);
  *out = ctx->f_sj.data();
  *count = t.written;
}

int bk_split_junctions(bk_ctx *ctx, int mapq_min, uint32_t tol, uint32_t min_reads, const struct bk_split_junction **out, uint64_t *count)
{
  return guarded(ctx, [&] { sj_run(ctx, "bk_split_junctions", mapq_min, tol, min_reads, nullptr, 0, true, out, count); });
}

// test hook: the same call with the claimed row looked up in a cluster table of the caller's (a context's own rows put the lower end first)
int bk_debug_split_junctions(bk_ctx *ctx, int mapq_min, uint32_t tol, uint32_t min_reads, const bk_cluster *rows, uint64_t n_rows, const struct bk_split_junction **out,
                             uint64_t *count)
{
  return guarded(ctx, [&] { sj_run(ctx, "bk_debug_split_junctions", mapq_min, tol, min_reads, rows, n_rows, false, out, count); });
}

int bk_split_junction_counts(bk_ctx *ctx, uint64_t out[6])
{
  return guarded(ctx, [&] {
    if (!out) throw bk_error(BK_ERR_ARG, "bk_split_junction_counts: null out");
    const SjStats &t = ctx->sj_stats;
    out[0] = t.n; out[1] = t.eligible; out[2] = t.exact; out[3] = t.calls; out[4] = t.claimed; out[5] = t.rounds;
  });
}

// Deletions and insertions from the CIGAR gaps of the context's record table (include/breakid_hip.h, gaps.hip)
int bk_cigar_gaps(bk_ctx *records, int mapq_min, uint32_t min_len, uint32_t anchor, uint32_t tol, uint32_t min_reads, const struct bk_cigar_gap **out, uint64_t *count)
{
  return guarded(records, [&] {
    if (!out || !count) throw bk_error(BK_ERR_ARG, "bk_cigar_gaps: null output");
    if (records->shard) throw bk_error(BK_ERR_ARG, "bk_cigar_gaps: sharded contexts (bk_shard_*) are not supported");
    if (!records->have_records) throw bk_error(BK_ERR_ARG, "bk_cigar_gaps: the context holds no record table");
    if (mapq_min < 0) throw bk_error(BK_ERR_ARG, "bk_cigar_gaps: mapq_min below 0");
    if (min_len == 0) throw bk_error(BK_ERR_ARG, "bk_cigar_gaps: min_len must be at least 1");
    if (min_len > BK_GAP_MAX_LEN) throw bk_error(BK_ERR_ARG, "bk_cigar_gaps: min_len above " + std::to_string(BK_GAP_MAX_LEN));
    if (anchor == 0) throw bk_error(BK_ERR_ARG, "bk_cigar_gaps: anchor must be at least 1");
    if (tol > BK_GAP_MAX_TOL) throw bk_error(BK_ERR_ARG, "bk_cigar_gaps: tol above " + std::to_string(BK_GAP_MAX_TOL));
    if (min_reads == 0) throw bk_error(BK_ERR_ARG, "bk_cigar_gaps: min_reads must be at least 1");
    const bk_soa &t = records->rec;
    if (t.n && (!t.tid || !t.pos || !t.flag || !t.mapq || !t.cigar_off || (!t.side && !t.qhash))) throw bk_error(BK_ERR_ARG, "bk_cigar_gaps: the record table lacks a column");
    if (t.n_cigar_words && !t.cigar) throw bk_error(BK_ERR_ARG, "bk_cigar_gaps: the record table lacks a column");
    GapInput in;
    in.rec = rec_view(records);
    in.n_cigar_words = t.n_cigar_words;
    in.side = t.side;
    in.qhash = t.qhash;
    in.tprefix = records->d_tprefix.get<uint32_t>();
    in.nt = records->nt;
    for (const uint32_t l : records->tlen) in.max_len = std::max(in.max_len, l);
    const GapParams p{mapq_min, min_len, anchor, tol, min_reads};
    struct bk_cigar_gap *d_rows = nullptr;
    records->gap_stats = GapStats{};
    GapStats &s = records->gap_stats;
    {
      // (the two scopes inside push timers of their own, so the whole one ends by its index, not at timers.back())
      struct Whole
      {
        bk_ctx *c;
        size_t at;
        ~Whole()
        {
          if (c->timing && at < c->timers.size()) (void) hipEventRecord(c->timers[at].b, c->st);
        }
      } whole{records, records->timers.size()};
      records->tick("cigar_gaps", 0, true, 0);
      {
        Scope sc(records, "cigar_gaps_records");
        gap_events(in, p, records->gpb, records->st, &s);
      }
      if (records->timing && !records->timers.empty()) records->timers.back().bytes = records->timers.back().touched = s.touched_records();
      {
        Scope sc(records, "cigar_gaps_calls");
        gap_calls(p, records->gpb, records->st, &d_rows, &s);
      }
      if (records->timing && !records->timers.empty()) records->timers.back().bytes = records->timers.back().touched = s.touched_calls();
      if (records->timing && whole.at < records->timers.size()) records->timers[whole.at].bytes = records->timers[whole.at].touched = s.touched_records() + s.touched_calls();
    }
    if (bk_debug("gaps"))
      fprintf(stderr, "bk_cigar_gaps: %llu records, %llu eligible, %llu events, %llu beyond, %llu exact, %llu loci, %llu calls, %llu returned\n", (unsigned long long) s.n,
              (unsigned long long) s.eligible, (unsigned long long) s.events, (unsigned long long) s.beyond, (unsigned long long) s.exact, (unsigned long long) s.loci,
              (unsigned long long) s.calls, (unsigned long long) s.written);
    rows_to_host(records, d_rows, s.written, records->f_gaps);
    *out = records->f_gaps.data();
    *count = s.written;
  });
}

int bk_cigar_gap_counts(bk_ctx *records, uint64_t out[8])
{
  return guarded(records, [&] {
    if (!out) throw bk_error(BK_ERR_ARG, "bk_cigar_gap_counts: null out");
    const GapStats &t = records->gap_stats;
    out[0] = t.n; out[1] = t.eligible; out[2] = t.events; out[3] = t.beyond; out[4] = t.exact; out[5] = t.loci; out[6] = t.calls; out[7] = t.written;
  });
}

// Soft-clip pile-ups of the context's record table (include/breakid_hip.h, cliploci.hip)
int bk_clip_loci(bk_ctx *records, bk_ctx *calls, int mapq_min, int min_clip, uint32_t tol, uint32_t pair_dist, uint32_t min_reads, const struct bk_clip_locus **out,
                 uint64_t *count)
{
  return guarded(records, [&] {
    if (!out || !count) throw bk_error(BK_ERR_ARG, "bk_clip_loci: null output");
    if (records->shard || (calls && calls->shard)) throw bk_error(BK_ERR_ARG, "bk_clip_loci: sharded contexts (bk_shard_*) are not supported");
    if (!records->have_records) throw bk_error(BK_ERR_ARG, "bk_clip_loci: the context holds no record table");
    if (mapq_min < 0) throw bk_error(BK_ERR_ARG, "bk_clip_loci: mapq_min below 0");
    if (min_clip < 1) throw bk_error(BK_ERR_ARG, "bk_clip_loci: min_clip must be at least 1");
    if (tol > BK_CLIPLOCI_MAX_TOL) throw bk_error(BK_ERR_ARG, "bk_clip_loci: tol above " + std::to_string(BK_CLIPLOCI_MAX_TOL));
    if (pair_dist > BK_CLIPLOCI_MAX_PAIR) throw bk_error(BK_ERR_ARG, "bk_clip_loci: pair_dist above " + std::to_string(BK_CLIPLOCI_MAX_PAIR));
    if (min_reads == 0) throw bk_error(BK_ERR_ARG, "bk_clip_loci: min_reads must be at least 1");
    if (calls)
    {
      if (!calls->bp_done) throw bk_error(BK_ERR_ARG, "bk_clip_loci: call bk_split_breakpoints on the calls context first");
      if (calls != records) require_same_reference("bk_clip_loci", "calls", calls, "records", records);
      if (calls->n_clusters > 0x3FFFFFFFull) throw bk_error(BK_ERR_LIMIT, "bk_clip_loci: too many clusters");
    }
    const bk_soa &t = records->rec;
    if (t.n && (!t.tid || !t.pos || !t.flag || !t.mapq || !t.cigar_off || !t.aux_off || (!t.side && !t.qhash)))
      throw bk_error(BK_ERR_ARG, "bk_clip_loci: the record table lacks a column");
    if (t.n_cigar_words && !t.cigar) throw bk_error(BK_ERR_ARG, "bk_clip_loci: the record table lacks a column");
    ClipLociInput in;
    in.rec = rec_view(records);
    in.n_cigar_words = t.n_cigar_words;
    in.side = t.side;
    in.qhash = t.qhash;
    in.tprefix = records->d_tprefix.get<uint32_t>();
    in.nt = records->nt;
    for (const uint32_t l : records->tlen) in.max_len = std::max(in.max_len, l);
    const ClipLociParams p{mapq_min, min_clip, tol, pair_dist, min_reads};
    if (calls && calls != records) HIP_CHECK(hipStreamSynchronize(calls->st));  // its stages ran on its own stream
    struct bk_clip_locus *d_rows = nullptr;
    records->cll_stats = ClipLociStats{};
    ClipLociStats &s = records->cll_stats;
    {
      // (the two scopes inside push timers of their own, so the whole one ends by its index, not at timers.back())
      struct Whole
      {
        bk_ctx *c;
        size_t at;
        ~Whole()
        {
          if (c->timing && at < c->timers.size()) (void) hipEventRecord(c->timers[at].b, c->st);
        }
      } whole{records, records->timers.size()};
      records->tick("clip_loci", 0, true, 0);
      {
        Scope sc(records, "clip_loci_records");
        cliploci_events(in, p, records->cllb, records->st, &s);
      }
      if (records->timing && !records->timers.empty()) records->timers.back().bytes = records->timers.back().touched = s.touched_records();
      {
        Scope sc(records, "clip_loci_calls");
        cliploci_calls(p, calls ? calls->clusters_ptr() : nullptr, calls ? calls->n_clusters : 0, records->cllb, records->st, &d_rows, &s);
      }
      if (records->timing && !records->timers.empty()) records->timers.back().bytes = records->timers.back().touched = s.touched_calls();
      if (records->timing && whole.at < records->timers.size()) records->timers[whole.at].bytes = records->timers[whole.at].touched = s.touched_records() + s.touched_calls();
    }
    if (bk_debug("cliploci"))
      fprintf(stderr, "bk_clip_loci: %llu records, %llu eligible, %llu events, %llu beyond, %llu exact, %llu loci, %llu mutual, %llu returned\n", (unsigned long long) s.n,
              (unsigned long long) s.eligible, (unsigned long long) (s.events + s.beyond), (unsigned long long) s.beyond, (unsigned long long) s.exact,
              (unsigned long long) s.loci, (unsigned long long) s.mutual, (unsigned long long) s.written);
    rows_to_host(records, d_rows, s.written, records->f_cll);
    *out = records->f_cll.data();
    *count = s.written;
  });
}

int bk_clip_locus_counts(bk_ctx *records, uint64_t out[8])
{
  return guarded(records, [&] {
    if (!out) throw bk_error(BK_ERR_ARG, "bk_clip_locus_counts: null out");
    const ClipLociStats &t = records->cll_stats;
    out[0] = t.n; out[1] = t.eligible; out[2] = t.events + t.beyond; out[3] = t.beyond; out[4] = t.exact; out[5] = t.loci; out[6] = t.mutual; out[7] = t.written;
  });
}

// The side rule of one call and the ALT text of one breakend (include/breakid_hip.h): pure host code.
int bk_junction_sides(const struct bk_junction *j, uint8_t *right1, uint8_t *right2, uint8_t *source)
{
  if (!j || !right1 || !right2 || !source) return BK_ERR_ARG;
  auto largest = [](const uint32_t *v) {
    int best = 0;
    for (int i = 1; i < 4; ++i)
      if (v[i] > v[best]) best = i;
    return v[best] ? best : -1;
  };
  int idx = largest(j->splits);
  *source = 2;
  if (idx < 0)
  {
    idx = largest(j->pairs);
    *source = 1;
  }
  if (idx < 0)
  {
    idx = 1;
    *source = 0;
  }
  *right1 = (uint8_t) (idx >> 1);
  *right2 = (uint8_t) (idx & 1);
  return BK_OK;
}

// The windows of one call (include/breakid_hip.h): pure host code.
int bk_call_windows(const bk_cluster *c, int right1, int right2, uint32_t flank, const uint32_t *target_len, struct bk_cov_window out[5])
{
  if (!c || !target_len || !out || flank == 0) return BK_ERR_ARG;
  const int32_t tid[2] = {c->p1_tid, c->p2_tid};
  const long long cut[2] = {(long long) c->p1_exact - (right1 ? 1 : 0), (long long) c->p2_exact - (right2 ? 1 : 0)};
  auto window = [&](int32_t t, long long a, long long b) {
    struct bk_cov_window w = {t, 0u, 0u, 0u};
    if (t < 0) return w;
    const long long len = (long long) target_len[t];
    a = a < 0 ? 0 : a;
    b = b > len ? len : b;
    if (b > a)
    {
      w.beg = (uint32_t) a;
      w.end = (uint32_t) b;
    }
    return w;
  };
  for (int s = 0; s < 2; ++s)
  {
    out[2 * s] = window(tid[s], cut[s] - (long long) flank, cut[s]);
    out[2 * s + 1] = window(tid[s], cut[s], cut[s] + (long long) flank);
  }
  out[4] = tid[0] == tid[1] && tid[0] >= 0 ? window(tid[0], std::min(cut[0], cut[1]), std::max(cut[0], cut[1])) : window(-1, 0, 0);
  return BK_OK;
}

// The rescue rule of one unvoted cluster (include/breakid_hip.h): pure host code.
int bk_clip_rescue(const bk_cluster *c, const struct bk_junction *j, const struct bk_clip_support *s, uint32_t min_support, uint32_t *pos1, uint32_t *pos2, uint32_t *n1,
                   uint32_t *n2)
{
  if (!c || !j || !s || !pos1 || !pos2 || !n1 || !n2 || min_support == 0) return BK_ERR_ARG;
  if ((c->flags & 2u) || c->p1_tid < 0 || c->p2_tid < 0) return 0;
  uint8_t d1 = 0, d2 = 1, source = 0;
  bk_junction_sides(j, &d1, &d2, &source);
  if (s->peak_n[0][d1] < min_support || s->peak_n[1][d2] < min_support) return 0;
  *pos1 = s->peak_pos[0][d1];
  *pos2 = s->peak_pos[1][d2];
  *n1 = s->peak_n[0][d1];
  *n2 = s->peak_n[1][d2];
  return 1;
}

int bk_vcf_breakend_alt(char ref_base, int own_right, const char *mate_chr, uint32_t mate_pos, int mate_right, char *buf, size_t cap)
{
  if (!mate_chr || !buf) return BK_ERR_ARG;
  const char br = mate_right ? '[' : ']';
  const std::string mate = br + std::string(mate_chr) + ":" + std::to_string(mate_pos) + br;
  const std::string alt = own_right ? mate + ref_base : ref_base + mate;
  if (alt.size() + 1 > cap) return BK_ERR_ARG;
  std::memcpy(buf, alt.c_str(), alt.size() + 1);
  return BK_OK;
}

int bk_run(bk_ctx *ctx, int mapq_min, int fast, double *w_out, uint64_t *n_valid)
{
  if (!ctx) return BK_ERR_ARG;
  if (ctx->stream_done && mapq_min != ctx->stream_mapq) ctx->stream_done = false;  // candidates were filtered with another threshold
  ctx->mapq_min = mapq_min;
  double mean, sd;
  int rc = bk_isize_stats(ctx, &mean, &sd);
  if (rc) return rc;
  const int times = 2;
  const double w = times * std::sqrt(times) * (mean + 3 * sd);  // BreakID.cc:103
  if (w_out) *w_out = w;
  if ((rc = bk_discordant_pairs(ctx, mapq_min, w, nullptr, nullptr))) return rc;
  if ((rc = bk_mask_and_cluster(ctx, w, fast, nullptr))) return rc;
  if ((rc = bk_split_evidence(ctx, nullptr))) return rc;
  if ((rc = bk_cluster_summary(ctx, w, nullptr))) return rc;
  if ((rc = bk_split_breakpoints(ctx, w, n_valid))) return rc;
  return BK_OK;
}

int bk_fetch(bk_ctx *ctx, int stage, const void **data, uint64_t *count, const uint64_t **group_off, uint32_t *n_groups)
{
  return guarded(ctx, [&] {
    if (!data || !count) throw bk_error(BK_ERR_ARG, "bk_fetch: null output");
    const uint32_t ng = ctx->jr.n_groups;
    if (group_off) *group_off = nullptr;
    if (n_groups) *n_groups = 0;
    auto fetch_list = [&](int slot, const uint32_t *d_idx, const uint64_t *d_goff, const uint32_t *d_cl, uint64_t n) {
      std::vector<bk_pair> all(ctx->jr.n_pairs);
      if (!all.empty()) HIP_CHECK(hipMemcpyAsync(all.data(), ctx->jr.pairs, all.size() * sizeof(bk_pair), hipMemcpyDeviceToHost, ctx->st));
      std::vector<uint32_t> idx(n), cl(d_cl ? n : 0);
      std::vector<uint64_t> goff(ng + 1, 0);
      if (n && d_idx) HIP_CHECK(hipMemcpyAsync(idx.data(), d_idx, n * 4, hipMemcpyDeviceToHost, ctx->st));
      if (n && d_cl) HIP_CHECK(hipMemcpyAsync(cl.data(), d_cl, n * 4, hipMemcpyDeviceToHost, ctx->st));
      if (ng && d_goff) HIP_CHECK(hipMemcpyAsync(goff.data(), d_goff, (ng + 1) * 8, hipMemcpyDeviceToHost, ctx->st));
      HIP_CHECK(hipStreamSynchronize(ctx->st));
      auto &out = ctx->f_pairs[slot];
      auto &off = ctx->f_off[slot];
      out.clear();
      off.assign(1, 0);
      for (uint32_t l = 0; l < ng; ++l)
      {
        uint32_t g = ctx->lex_to_num[l];
        for (uint64_t p = goff[g]; p < goff[g + 1]; ++p)
        {
          bk_pair pr = all[d_idx ? idx[p] : p];
          if (d_cl) pr.cluster = (int32_t) cl[p];
          out.push_back(pr);
        }
        off.push_back(out.size());
      }
      *data = out.data();
      *count = out.size();
      if (group_off) *group_off = off.data();
      if (n_groups) *n_groups = ng;
    };
    switch (stage)
    {
    case BK_STAGE_SCAN:
      fetch_list(0, nullptr, ctx->jr.gstart, nullptr, ctx->jr.n_pairs);
      break;
    case BK_STAGE_ISO:
      fetch_list(1, ctx->stage.iso_idx.get<uint32_t>(), ctx->stage.iso_goff.get<uint64_t>(), nullptr, ctx->stage.iso_n);
      break;
    case BK_STAGE_CLUSTERED:
      if (!ctx->clustered) throw bk_error(BK_ERR_ARG, "bk_fetch: not clustered yet");
      fetch_list(2, ctx->stage.list.idx.get<uint32_t>(), ctx->stage.list.goff.get<uint64_t>(), ctx->stage.d_cluster.get<uint32_t>(), ctx->stage.list.n);
      break;
    case BK_STAGE_SPLITS:
      ensure_splits_sorted(ctx);
      ctx->f_splits.resize(ctx->hc.n_split);
      if (ctx->hc.n_split)
        HIP_CHECK(hipMemcpyAsync(ctx->f_splits.data(), ctx->d_split.get<bk_split>(), ctx->hc.n_split * sizeof(bk_split), hipMemcpyDeviceToHost, ctx->st));
      HIP_CHECK(hipStreamSynchronize(ctx->st));
      *data = ctx->f_splits.data();
      *count = ctx->f_splits.size();
      break;
    case BK_STAGE_CLUSTERS:
      rows_to_host(ctx, ctx->clusters_ptr(), ctx->n_clusters, ctx->f_clusters);
      // The reference appends groups in std::map<string> order.  A context's own table is built in that order (bp.hip,
      // cluster_summary); a sharded one holds the ranks' tables one after the other.
      {
        auto by_group = [](const bk_cluster &a, const bk_cluster &b) { return a.group < b.group; };
        if (ctx->ext_clusters)
          std::stable_sort(ctx->f_clusters.begin(), ctx->f_clusters.end(), by_group);
        else if (!std::is_sorted(ctx->f_clusters.begin(), ctx->f_clusters.end(), by_group))
          throw bk_error(BK_ERR_HIP, "bk_fetch: the cluster table is not in group order (internal error)");
      }
      *data = ctx->f_clusters.data();
      *count = ctx->f_clusters.size();
      break;
    case BK_STAGE_GROUP_KEYS:
      ctx->f_gkeys.clear();
      for (uint32_t l = 0; l < ng; ++l)
      {
        uint32_t k = ctx->gkey_host[ctx->lex_to_num[l]];
        ctx->f_gkeys.push_back((int32_t) (k / (uint32_t) (ctx->nt + 1)) - 1);
        ctx->f_gkeys.push_back((int32_t) (k % (uint32_t) (ctx->nt + 1)) - 1);
      }
      *data = ctx->f_gkeys.data();
      *count = ng;
      break;
    default:
      throw bk_error(BK_ERR_ARG, "bk_fetch: unknown stage");
    }
  });
}

// ---- single-sample sharding: one context per GPU holds a contiguous range of the sample's records ----------
int bk_shard_begin(bk_ctx *ctx, uint64_t rec_base, int mapq_min)
{
  return guarded(ctx, [&] {
    ctx->rec_base = rec_base;
    ctx->shard = true;
    ctx->streamed = true;
    ctx->mapq_min = mapq_min;
    ctx->ext_cand = nullptr;
    ctx->ext_split = nullptr;
    ctx->ext_clusters = nullptr;
    run_stream(ctx);
  });
}

int bk_shard_get_stats(bk_ctx *ctx, bk_shard_stats *out)
{
  return guarded(ctx, [&] {
    if (!ctx->stream_done || !out) throw bk_error(BK_ERR_ARG, "bk_shard_get_stats: call bk_shard_begin first");
    out->isize_sum = ctx->hc.isize_sum;
    out->isize_n = ctx->hc.isize_n;
    out->sumsq = ctx->hsd.sumsq;
    out->vmax = ctx->hsd.vmax;
    out->max_span = ctx->hc.max_span;
    out->n_cand = ctx->hc.n_cand;
    out->n_split = ctx->hc.n_split;
  });
}

int bk_shard_set_stats(bk_ctx *ctx, const bk_shard_stats *total)
{
  return guarded(ctx, [&] {
    if (!ctx->stream_done || !total) throw bk_error(BK_ERR_ARG, "bk_shard_set_stats: call bk_shard_begin first");
    ctx->hc.isize_sum = total->isize_sum;
    ctx->hc.isize_n = total->isize_n;
    ctx->hsd.sumsq = total->sumsq;
    ctx->hsd.vmax = total->vmax;
    ctx->hc.max_span = total->max_span;
    ctx->stats_done = false;
  });
}

static void sd_mean_thr(bk_ctx *ctx, double &m, double &thr)
{
  const double n = (double) ctx->hc.isize_n;
  m = (double) (long long) ctx->hc.isize_sum / n;  // (double) long / (double) size_t, BreakID.cc:1941
  if (ctx->hc.isize_n == 0)
  {
    // no eligible record in the whole sample: the mean is NaN (0 / 0), there is nothing to replay, and ilogb(NaN) is no exponent
    thr = 0;
    return;
  }
  double sum_d = ctx->hsd.sumsq - 2.0 * m * (double) ctx->hc.isize_sum + n * m * m;
  if (!(sum_d > 0)) sum_d = 0;
  double da = (double) ctx->hsd.vmax - m, dmax = da * da + m * m;
  double bound = 2.0 * sum_d + 2.0 * n + 2.0 * dmax + 4.0;
  int k = std::ilogb(bound) + 1;
  thr = k >= 51 ? 1.0e300 : std::ldexp(1.0, k - 53);
}

int bk_shard_sd_local(bk_ctx *ctx, uint64_t *l_total, void **ex_dev, uint64_t *n_ex)
{
  return guarded(ctx, [&] {
    if (!ctx->stream_done) throw bk_error(BK_ERR_ARG, "bk_shard_sd_local: call bk_shard_begin / bk_shard_set_stats first");
    double m, thr;
    sd_mean_thr(ctx, m, thr);
    unsigned long long lt = 0, ne = 0;
    launch_sd_local(ctx->rec.flag, ctx->rec.isize, ctx->rec.n, m, thr, ctx->sdb, ctx->st, &lt, &ne);
    HIP_CHECK(hipStreamSynchronize(ctx->st));
    if (l_total) *l_total = lt;
    if (n_ex) *n_ex = ne;
    if (ex_dev) *ex_dev = ctx->sdb.exceptions.p;
  });
}

int bk_shard_sd_finish(bk_ctx *ctx, const void *all_ex_dev, uint64_t n_all, uint64_t l_grand, double *mean, double *sd)
{
  return guarded(ctx, [&] {
    double m, thr;
    sd_mean_thr(ctx, m, thr);
    launch_sd_walk((const SdException *) all_ex_dev, n_all, l_grand, ctx->d_sd.get<SdState>(), ctx->st);
    HIP_CHECK(hipMemcpyAsync(&ctx->hsd.t_final, &ctx->d_sd.get<SdState>()->t_final, 8, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipStreamSynchronize(ctx->st));
    ctx->mean = m;
    ctx->sd = std::sqrt((double) ctx->hsd.t_final / (double) ctx->hc.isize_n);
    ctx->stats_done = true;
    if (mean) *mean = ctx->mean;
    if (sd) *sd = ctx->sd;
  });
}

int bk_shard_buffer(bk_ctx *ctx, int which, void **dev, uint64_t *count, uint32_t *elem_bytes)
{
  return guarded(ctx, [&] {
    if (!dev || !count || !elem_bytes) throw bk_error(BK_ERR_ARG, "bk_shard_buffer: null output");
    switch (which)
    {
    case BK_BUF_CANDIDATES: *dev = ctx->d_cand.p; *count = ctx->ext_cand ? 0 : ctx->hc.n_cand; *elem_bytes = sizeof(Cand); break;
    case BK_BUF_TUPLES: *dev = ctx->d_split_raw.p; *count = ctx->ext_split ? 0 : ctx->hc.n_split; *elem_bytes = sizeof(bk_split); break;
    case BK_BUF_CLUSTERS: *dev = ctx->d_clusters.p; *count = ctx->ext_clusters ? 0 : ctx->n_clusters; *elem_bytes = sizeof(bk_cluster); break;
    default: throw bk_error(BK_ERR_ARG, "bk_shard_buffer: unknown buffer");
    }
  });
}

int bk_shard_set_buffer(bk_ctx *ctx, int which, const void *dev, uint64_t count)
{
  return guarded(ctx, [&] {
    switch (which)
    {
    case BK_BUF_CANDIDATES: ctx->ext_cand = (const Cand *) dev; ctx->hc.n_cand = count; break;
    case BK_BUF_TUPLES: ctx->ext_split = (const bk_split *) dev; ctx->hc.n_split = count; ctx->splits_sorted = false; break;
    case BK_BUF_CLUSTERS: ctx->ext_clusters = (bk_cluster *) dev; ctx->n_clusters = count; break;
    default: throw bk_error(BK_ERR_ARG, "bk_shard_set_buffer: unknown buffer");
    }
  });
}

int bk_shard_group_sizes(bk_ctx *ctx, const uint64_t **starts, uint32_t *n_groups)
{
  return guarded(ctx, [&] {
    if (starts) *starts = ctx->gstart_host.data();
    if (n_groups) *n_groups = ctx->jr.n_groups;
  });
}

int bk_shard_own_groups(bk_ctx *ctx, const uint8_t *own, uint32_t n_groups)
{
  return guarded(ctx, [&] {
    if (n_groups != ctx->jr.n_groups) throw bk_error(BK_ERR_ARG, "bk_shard_own_groups: wrong group count");
    ctx->own_groups.assign(own, own + n_groups);
  });
}

int bk_shard_route_candidates(bk_ctx *ctx, uint32_t world, void **dev, const uint64_t **counts)
{
  return guarded(ctx, [&] {
    if (!ctx->stream_done || ctx->ext_cand) throw bk_error(BK_ERR_ARG, "bk_shard_route_candidates: needs this shard's own candidates (after bk_shard_begin)");
    if (!world || world > 4096 || !dev || !counts) throw bk_error(BK_ERR_ARG, "bk_shard_route_candidates: bad arguments");
    *dev = route_candidates(ctx->d_cand.get<Cand>(), ctx->hc.n_cand, world, ctx->jb, ctx->st, ctx->route_counts);
    *counts = ctx->route_counts.data();
  });
}

int bk_shard_group_keys(bk_ctx *ctx, const uint32_t **keys, uint32_t *n_groups)
{
  return guarded(ctx, [&] {
    if (keys) *keys = ctx->gkey_host.data();
    if (n_groups) *n_groups = ctx->jr.n_groups;
  });
}

int bk_shard_route_pairs(bk_ctx *ctx, const uint32_t *dest_of_group, uint32_t n_groups, uint32_t world, void **dev, const uint64_t **counts)
{
  return guarded(ctx, [&] {
    if (n_groups != ctx->jr.n_groups || !world || !dev || !counts || (n_groups && !dest_of_group)) throw bk_error(BK_ERR_ARG, "bk_shard_route_pairs: bad arguments");
    ctx->route_counts.assign(world, 0);
    for (uint32_t g = 0; g < n_groups; ++g)
    {
      if (dest_of_group[g] >= world) throw bk_error(BK_ERR_ARG, "bk_shard_route_pairs: destination out of range");
      ctx->route_counts[dest_of_group[g]] += ctx->gstart_host[g + 1] - ctx->gstart_host[g];
    }
    std::vector<uint64_t> base(world, 0), off(n_groups, 0);
    for (uint32_t d = 1; d < world; ++d) base[d] = base[d - 1] + ctx->route_counts[d - 1];
    for (uint32_t g = 0; g < n_groups; ++g)
    {
      off[g] = base[dest_of_group[g]];
      base[dest_of_group[g]] += ctx->gstart_host[g + 1] - ctx->gstart_host[g];
    }
    *dev = route_pairs(ctx->jr, off, ctx->jb, ctx->st);
    *counts = ctx->route_counts.data();
  });
}

int bk_shard_group_pairs(bk_ctx *ctx, const void *pairs_dev, uint64_t n, const uint32_t *all_keys, uint32_t n_all_keys)
{
  return guarded(ctx, [&] {
    if ((n && !pairs_dev) || (n_all_keys && !all_keys)) throw bk_error(BK_ERR_ARG, "bk_shard_group_pairs: null input");
    {
      Scope s(ctx, "group_pairs");
      ctx->jb2.rec_bits = -1;  // the pairs carry the discovery indices of the whole sample
      group_pairs((const bk_pair *) pairs_dev, n, ctx->nt, ctx->jb2, ctx->st, ctx->jr);
    }
    std::vector<uint32_t> keys(all_keys, all_keys + n_all_keys);
    finish_groups(ctx, &keys);
    ctx->own_groups.clear();  // the table holds exactly the groups this rank owns
    ctx->clustered = false;
  });
}

int bk_shard_bp_cov(bk_ctx *ctx, double w, void **cov_dev, uint64_t *n)
{
  return guarded(ctx, [&] {
    uint32_t *cov = bp_cov_partial(rec_view(ctx), ctx->clusters_ptr(), ctx->n_clusters, w, (int) ctx->hc.max_span, ctx->bb, ctx->st);
    HIP_CHECK(hipStreamSynchronize(ctx->st));
    if (cov_dev) *cov_dev = cov;
    if (n) *n = 2 * ctx->n_clusters;
  });
}

int bk_shard_bp_vote(bk_ctx *ctx, double w, const void *cov_total_dev)
{
  return guarded(ctx, [&] {
    ensure_splits_sorted(ctx);
    bp_vote(ctx->d_split.get<bk_split>(), ctx->hc.n_split, ctx->clusters_ptr(), ctx->n_clusters, w, (int) ctx->hc.max_span, (const uint32_t *) cov_total_dev,
            ctx->d_hdr.get<int32_t>(), ctx->bb, ctx->st);
    HIP_CHECK(hipStreamSynchronize(ctx->st));
  });
}

int bk_shard_bp_vote_slice(bk_ctx *ctx, double w, const void *cov_total_dev, uint64_t lo, uint64_t hi, void **clusters_dev, void **voted_dev)
{
  return guarded(ctx, [&] {
    if (lo > hi || hi > ctx->n_clusters || !clusters_dev || !voted_dev) throw bk_error(BK_ERR_ARG, "bk_shard_bp_vote_slice: bad range");
    ensure_splits_sorted(ctx);
    bp_vote(ctx->d_split.get<bk_split>(), ctx->hc.n_split, ctx->clusters_ptr() + lo, hi - lo, w, (int) ctx->hc.max_span,
            cov_total_dev ? (const uint32_t *) cov_total_dev + 2 * lo : nullptr, ctx->d_hdr.get<int32_t>(), ctx->bb, ctx->st);
    HIP_CHECK(hipStreamSynchronize(ctx->st));
    *clusters_dev = ctx->clusters_ptr() + lo;
    *voted_dev = ctx->bb.voted.p;
  });
}

int bk_shard_bp_set_voted(bk_ctx *ctx, const void *voted_all_dev)
{
  return guarded(ctx, [&] {
    uint32_t *v = ctx->bb.voted.as<uint32_t>(ctx->n_clusters + 1);
    if (ctx->n_clusters && voted_all_dev != v)
      HIP_CHECK(hipMemcpyAsync(v, voted_all_dev, ctx->n_clusters * 4, hipMemcpyDeviceToDevice, ctx->st));
    HIP_CHECK(hipStreamSynchronize(ctx->st));
  });
}

int bk_shard_bp_depth(bk_ctx *ctx, void **depth_dev, uint64_t *n)
{
  return guarded(ctx, [&] {
    uint32_t *d = bp_depth_partial(rec_view(ctx), ctx->clusters_ptr(), ctx->n_clusters, (int) ctx->hc.max_span, ctx->bb, ctx->st);
    HIP_CHECK(hipStreamSynchronize(ctx->st));
    if (depth_dev) *depth_dev = d;
    if (n) *n = 2 * ctx->n_clusters;
  });
}

int bk_shard_bp_finish(bk_ctx *ctx, const void *depth_total_dev)
{
  return guarded(ctx, [&] {
    bp_finish(ctx->clusters_ptr(), ctx->n_clusters, (const uint32_t *) depth_total_dev, ctx->bb, ctx->st);
    HIP_CHECK(hipStreamSynchronize(ctx->st));
  });
}

int bk_debug_std_sort(bk_ctx *ctx, const uint32_t *key, const uint64_t *group_off, uint32_t n_groups, uint32_t *perm_out)
{
  return guarded(ctx, [&] {
    if (!key || !group_off || !perm_out) throw bk_error(BK_ERR_ARG, "bk_debug_std_sort: null argument");
    const uint64_t n = group_off[n_groups];
    DevBuf dk, dp, dgof, dgoff;
    std::vector<uint32_t> gof(n), iota(n);
    for (uint32_t g = 0; g < n_groups; ++g)
      for (uint64_t p = group_off[g]; p < group_off[g + 1]; ++p) gof[p] = g;
    std::iota(iota.begin(), iota.end(), 0u);
    HIP_CHECK(hipMemcpy(dk.as<uint32_t>(n + 1), key, n * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dp.as<uint32_t>(n + 1), iota.data(), n * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dgof.as<uint32_t>(n + 1), gof.data(), n * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dgoff.as<uint64_t>((uint64_t) n_groups + 1), group_off, ((uint64_t) n_groups + 1) * 8, hipMemcpyHostToDevice));
    uint64_t max_group = 0;
    for (uint32_t g = 0; g < n_groups; ++g) max_group = std::max<uint64_t>(max_group, group_off[g + 1] - group_off[g]);
    ctx->stage.debug_sort(ctx->device, ctx->st, dk.get<uint32_t>(), dp.get<uint32_t>(), dgof.get<uint32_t>(), dgoff.get<uint64_t>(), n_groups, n, max_group);
    HIP_CHECK(hipMemcpyAsync(perm_out, dp.get<uint32_t>(), n * 4, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipStreamSynchronize(ctx->st));
  });
}

int bk_debug_scan(bk_ctx *ctx, int elem_bytes, const void *in, uint64_t n, int in_place, void *out)
{
  return guarded(ctx, [&] {
    if (elem_bytes != 4 && elem_bytes != 8) throw bk_error(BK_ERR_ARG, "bk_debug_scan: elem_bytes must be 4 or 8");
    if (!out || (n && !in)) throw bk_error(BK_ERR_ARG, "bk_debug_scan: null argument");
    auto run = [&](auto zero) {
      using T = decltype(zero);
      T *d_in = ctx->dbg_in.as<T>(n + 1);
      T *d_out = in_place ? d_in : ctx->dbg_out.as<T>(n + 1);
      // the output holds a pattern first: an entry the scan does not write shows as that, not as what an earlier call left
      HIP_CHECK(hipMemsetAsync(d_out, 0xA5, (n + 1) * sizeof(T), ctx->st));
      if (n) HIP_CHECK(hipMemcpyAsync(d_in, in, n * sizeof(T), hipMemcpyHostToDevice, ctx->st));
      prims::exclusive_scan<T>(d_in, d_out, n, ctx->dbg_radix.scan_tmp, ctx->st);
      HIP_CHECK(hipMemcpyAsync(out, d_out, (n + 1) * sizeof(T), hipMemcpyDeviceToHost, ctx->st));
      HIP_CHECK(hipStreamSynchronize(ctx->st));
    };
    if (elem_bytes == 4)
      run(uint32_t(0));
    else
      run(uint64_t(0));
  });
}

int bk_debug_radix_sort(bk_ctx *ctx, const uint64_t *keys, const uint32_t *vals, uint64_t n, int begin_bit, int end_bit, uint64_t *keys_out, uint32_t *vals_out)
{
  return guarded(ctx, [&] {
    if (n && (!keys || !vals || !keys_out || !vals_out)) throw bk_error(BK_ERR_ARG, "bk_debug_radix_sort: null argument");
    if (begin_bit < 0 || end_bit > 64) throw bk_error(BK_ERR_ARG, "bk_debug_radix_sort: bits outside [0, 64]");
    prims::radix_check_count(n);
    if (!n) return;
    prims::RadixBufs &rb = ctx->dbg_radix;
    uint64_t *dk = ctx->dbg_in.as<uint64_t>(n);
    uint32_t *dv = ctx->dbg_vals.as<uint32_t>(n);
    // (the alternate buffers hold a pattern, not an earlier call's result, wherever this call does not write them)
    HIP_CHECK(hipMemsetAsync(rb.keys_alt.as<uint64_t>(n), 0xA5, n * 8, ctx->st));
    HIP_CHECK(hipMemsetAsync(rb.vals_alt.as<uint32_t>(n), 0xA5, n * 4, ctx->st));
    HIP_CHECK(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, ctx->st));
    HIP_CHECK(hipMemcpyAsync(dv, vals, n * 4, hipMemcpyHostToDevice, ctx->st));
    uint64_t *ko = nullptr;
    uint32_t *vo = nullptr;
    prims::radix_sort_pairs(dk, dv, n, begin_bit, end_bit, rb, ctx->st, &ko, &vo);
    HIP_CHECK(hipMemcpyAsync(keys_out, ko, n * 8, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipMemcpyAsync(vals_out, vo, n * 4, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipStreamSynchronize(ctx->st));
  });
}

int bk_debug_prims_info(uint64_t out[4])
{
  if (!out) return BK_ERR_ARG;
  out[0] = prims::BLOCK;
  out[1] = prims::SCAN_TILE;
  out[2] = prims::SCAN_ONE_MAX;
  out[3] = prims::RS_TILE;
  return BK_OK;
}

int bk_sort_forms(bk_ctx *ctx, uint64_t out[3])
{
  return guarded(ctx, [&] {
    if (!out) throw bk_error(BK_ERR_ARG, "bk_sort_forms: null output");
    ctx->stage.sort_forms(out);
  });
}

int bk_debug_sort_info(bk_ctx *ctx, uint64_t out[13])
{
  return guarded(ctx, [&] {
    if (!out) throw bk_error(BK_ERR_ARG, "bk_debug_sort_info: null output");
    static_assert(SORT_INFO_WORDS == 11, "bk_debug_sort_info: eleven words of the build, two of the last sort");
    std_sort_info(out);
    const SortEmuBufs &se = ctx->stage.cb().se;
    out[11] = se.last_heap[0];
    out[12] = se.last_heap[1];
  });
}

int bk_debug_ahc(bk_ctx *ctx, const uint32_t *x, const uint32_t *y, uint32_t n, double w, uint32_t *idx_out, int32_t *cluster_out, uint32_t *n_out)
{
  return guarded(ctx, [&] {
    if (!x || !y || !idx_out || !cluster_out || !n_out) throw bk_error(BK_ERR_ARG, "bk_debug_ahc: null argument");
    std::vector<bk_pair> hp(n);
    for (uint32_t i = 0; i < n; ++i)
    {
      memset(&hp[i], 0, sizeof(bk_pair));
      hp[i].x = x[i];
      hp[i].y = y[i];
    }
    DevBuf dp, dcl;
    PairList L;
    L.n = n;
    L.ng = 1;
    std::vector<uint32_t> iota(n), gof(n, 0);
    std::iota(iota.begin(), iota.end(), 0u);
    uint64_t goff[2] = {0, n};
    HIP_CHECK(hipMemcpy(dp.as<bk_pair>(n + 1), hp.data(), n * sizeof(bk_pair), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(L.idx.as<uint32_t>(n + 1), iota.data(), n * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(L.gof.as<uint32_t>(n + 1), gof.data(), n * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(L.goff.as<uint64_t>(2), goff, 16, hipMemcpyHostToDevice));
    ahc_cluster_all(dp.get<bk_pair>(), L, w, dcl, ctx->stage.ab, ctx->stage.cb(), ctx->st);
    *n_out = (uint32_t) L.n;
    if (L.n)
    {
      HIP_CHECK(hipMemcpyAsync(idx_out, L.idx.get<uint32_t>(), L.n * 4, hipMemcpyDeviceToHost, ctx->st));
      HIP_CHECK(hipMemcpyAsync(cluster_out, dcl.get<uint32_t>(), L.n * 4, hipMemcpyDeviceToHost, ctx->st));
    }
    HIP_CHECK(hipStreamSynchronize(ctx->st));
  });
}

}  // extern "C"

// ---- feed and stream pass overlapped: the reference's two sequential BAM passes (BreakID.cc:1929, :1414)
// become one read of the file, and the record-level kernel of the hot path runs while the file is still arriving -------------
namespace
{
struct FeedLink
{
  int device = 0, mapq_min = 20;
  bk_ctx *ctx = nullptr;
  int rc = BK_OK;
  std::string err;
  uint64_t done = 0;      // records [0, done) have been through k_stream (a multiple of 4)
  bool prepared = false, overflow = false;
  hipEvent_t t0 = nullptr, t1 = nullptr;  // timing: first and last k_stream piece
  template <class F> void guard(F &&f)
  {
    if (rc != BK_OK) return;
    try
    {
      f();
    }
    catch (const bk_error &e)
    {
      rc = e.code;
      err = e.msg;
    }
  }
};
void link_header(void *u, int nt, const char *const *names, const uint32_t *lens)
{
  FeedLink *L = (FeedLink *) u;
  if (L->ctx || L->rc != BK_OK) return;
  L->rc = bk_init(L->device, lens, names, nt, &L->ctx);
  if (L->rc != BK_OK) L->err = bk_last_error(nullptr);
}
void link_reset(void *u)
{
  FeedLink *L = (FeedLink *) u;
  L->guard([&] {
    if (L->ctx) HIP_CHECK(hipStreamSynchronize(L->ctx->st));
    L->done = 0;
    L->prepared = false;
    L->overflow = false;
  });
}
void link_before_move(void *u)
{
  FeedLink *L = (FeedLink *) u;
  L->guard([&] {
    if (L->ctx) HIP_CHECK(hipStreamSynchronize(L->ctx->st));
  });
}
void link_chunk(void *u, const bk_soa *cols, uint64_t n_ready, uint64_t n_est, hipEvent_t ready)
{
  FeedLink *L = (FeedLink *) u;
  L->guard([&] {
    bk_ctx *c = L->ctx;
    if (!c || n_ready < (uint64_t) STREAM_V + 1) return;
    c->rec = *cols;  // device pointers of the columns as they stand now
    c->have_records = true;
    c->mapq_min = L->mapq_min;
    if (!L->prepared)
    {
      stream_prepare(c, n_est + n_est / 4);
      L->prepared = true;
    }
    // the last ready record stays for the next piece: its quad reads the offset entry that follows it
    const uint64_t lim = (n_ready - 1) / STREAM_V * STREAM_V;
    if (lim <= L->done) return;
    HIP_CHECK(hipStreamWaitEvent(c->st, ready, 0));
    StreamArgs a = stream_args(c, lim);
    a.q_begin = L->done / STREAM_V;
    launch_stream(a, c->st);
    L->done = lim;
  });
}
}  // namespace


extern "C" {

int bk_bam_decode_device_ctx(const char *path, int device, int mapq_min, bk_bam_dev **bam_out, bk_ctx **ctx_out, int *n_targets, const char *const **names,
                             const uint32_t **lens, char *err, size_t errlen)
{
  auto fail = [&](int code, const std::string &m) {
    if (err && errlen) snprintf(err, errlen, "%s", m.c_str());
    return code;
  };
  if (!path || !bam_out || !ctx_out) return fail(BK_ERR_ARG, "bk_bam_decode_device_ctx: null argument");
  *bam_out = nullptr;
  *ctx_out = nullptr;
  FeedLink L;
  L.device = device;
  L.mapq_min = mapq_min;
  FeedConsumer fc;
  fc.user = &L;
  fc.on_header = link_header;
  fc.on_chunk = link_chunk;
  fc.before_move = link_before_move;
  fc.on_reset = link_reset;
  bk_soa cols;
  bk_bam_dev *bam = nullptr;
  int rc = bam_decode_device_impl(path, device, &bam, &cols, n_targets, names, lens, err, errlen, &fc);
  if (rc == BK_OK && L.rc != BK_OK) rc = fail(L.rc, L.err);
  if (rc == BK_OK && !L.ctx) rc = fail(BK_ERR_IO, "bk_bam_decode_device_ctx: no header");
  if (rc != BK_OK)
  {
    if (L.ctx) bk_free(L.ctx);
    if (bam) bk_bam_dev_free(bam);
    return rc;
  }
  bk_ctx *c = L.ctx;
  rc = guarded(c, [&] {
    // the complete table (final pointers, end entries of the offset columns written), then the records the pieces left
    const uint64_t done = L.prepared ? L.done : 0;
    c->stream_done = c->stats_done = c->clustered = false;
    c->rec = cols;
    c->have_records = true;
    c->mapq_min = mapq_min;
    c->rec_base = 0;
    bool ok = false;
    if (L.prepared)
    {
      Scope s(c, "k_stream", 39ull * cols.n + 4ull * cols.n_cigar_words);
      StreamArgs a = stream_args(c, cols.n);
      a.q_begin = done / STREAM_V;
      launch_stream(a, c->st);
      ok = stream_finish(c);
    }
    if (ok)
      stream_rare_path(c);
    else
      run_stream(c);  // file without chunked feed (records across BGZF blocks), or an output capacity estimated too small
    if (bk_debug("feed"))
      fprintf(stderr, "[feed/stream] stream pass %s: %llu of %llu records went through k_stream while the file was still arriving\n", ok ? "overlapped" : "after the feed",
              (unsigned long long) (ok ? done : 0), (unsigned long long) cols.n);
  });
  if (rc != BK_OK)
  {
    fail(rc, c->err);
    bk_free(c);
    bk_bam_dev_free(bam);
    return rc;
  }
  *bam_out = bam;
  *ctx_out = c;
  return BK_OK;
}

int bk_group_stats(bk_ctx *ctx, const bk_group_stat **out, uint32_t *n_groups)
{
  return guarded(ctx, [&] {
    if (!out || !n_groups) throw bk_error(BK_ERR_ARG, "bk_group_stats: null output");
    if (!ctx->clustered) throw bk_error(BK_ERR_ARG, "bk_group_stats: call bk_mask_and_cluster (and bk_cluster_summary) first");
    const uint32_t ng = ctx->jr.n_groups;
    std::vector<uint64_t> iso(ng + 1, 0), clu(ng + 1, 0);
    std::vector<uint32_t> kmax(ng + 1, 0);
    if (ng)
    {
      HIP_CHECK(hipMemcpyAsync(iso.data(), ctx->stage.iso_goff.get<uint64_t>(), ((uint64_t) ng + 1) * 8, hipMemcpyDeviceToHost, ctx->st));
      HIP_CHECK(hipMemcpyAsync(clu.data(), ctx->stage.list.goff.get<uint64_t>(), ((uint64_t) ng + 1) * 8, hipMemcpyDeviceToHost, ctx->st));
      if (ctx->stage.list.n && ctx->bb.kmax.p) HIP_CHECK(hipMemcpyAsync(kmax.data(), ctx->bb.kmax.get<uint32_t>(), (uint64_t) ng * 4, hipMemcpyDeviceToHost, ctx->st));
      HIP_CHECK(hipStreamSynchronize(ctx->st));
    }
    ctx->f_gstats.assign(ng, bk_group_stat{});
    for (uint32_t l = 0; l < ng; ++l)
    {
      const uint32_t g = ctx->lex_to_num[l];
      bk_group_stat &o = ctx->f_gstats[l];
      const uint32_t k = ctx->gkey_host[g];
      o.p1_tid = (int32_t) (k / (uint32_t) (ctx->nt + 1)) - 1;
      o.p2_tid = (int32_t) (k % (uint32_t) (ctx->nt + 1)) - 1;
      o.n_scan = ctx->gstart_host[g + 1] - ctx->gstart_host[g];
      o.n_isolated_removed = iso[g + 1] - iso[g];
      o.n_clustered = clu[g + 1] - clu[g];
      o.cluster_id_end = o.n_clustered ? kmax[g] : 0;
      o.ordinal = ctx->glex_host[g];
    }
    *out = ctx->f_gstats.data();
    *n_groups = ng;
  });
}

int bk_debug_points_groups(bk_ctx *ctx, int mode, const uint32_t *x, const uint32_t *y, const uint64_t *group_off, uint32_t n_groups, double w, uint32_t *idx_out,
                           int32_t *cluster_out, uint64_t *goff_out, uint32_t *n_out)
{
  return guarded(ctx, [&] {
    if (!group_off || !idx_out || !n_out || mode < 0 || mode > 2) throw bk_error(BK_ERR_ARG, "bk_debug_points_groups: bad argument");
    if (group_off[0] != 0) throw bk_error(BK_ERR_ARG, "bk_debug_points_groups: group_off[0] must be 0");
    for (uint32_t g = 0; g < n_groups; ++g)
      if (group_off[g + 1] < group_off[g]) throw bk_error(BK_ERR_ARG, "bk_debug_points_groups: group_off must ascend");
    const uint64_t n = group_off[n_groups];
    if (n >= (1ull << 31) || (n && (!x || !y))) throw bk_error(BK_ERR_ARG, "bk_debug_points_groups: bad argument");
    std::vector<bk_pair> hp(n);
    std::vector<uint32_t> gof(n);
    for (uint32_t g = 0; g < n_groups; ++g)
      for (uint64_t i = group_off[g]; i < group_off[g + 1]; ++i)
      {
        memset(&hp[i], 0, sizeof(bk_pair));
        hp[i].x = x[i];
        hp[i].y = y[i];
        gof[i] = g;
      }
    DevBuf dp, dcl, dgof, dgoff;
    PairList L;
    const size_t goff_bytes = ((size_t) n_groups + 1) * 8;
    if (n) HIP_CHECK(hipMemcpy(dp.as<bk_pair>(n + 1), hp.data(), n * sizeof(bk_pair), hipMemcpyHostToDevice));
    if (n) HIP_CHECK(hipMemcpy(dgof.as<uint32_t>(n + 1), gof.data(), n * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dgoff.as<uint64_t>((uint64_t) n_groups + 1), group_off, goff_bytes, hipMemcpyHostToDevice));
    const bk_pair *pairs = dp.as<bk_pair>(n + 1);
    // one list over all groups, as the lanes hand it to these functions (lanes.hip)
    if (mode == 1)
      remove_isolated_all(pairs, dgof.get<uint32_t>(), dgoff.get<uint64_t>(), n_groups, n, w, L, ctx->stage.cb(), ctx->st);
    else
    {
      // the list as given: identity order
      L.n = n;
      L.ng = n_groups;
      std::vector<uint32_t> iota(n);
      std::iota(iota.begin(), iota.end(), 0u);
      uint32_t *lidx = L.idx.as<uint32_t>(n + 1), *lgof = L.gof.as<uint32_t>(n + 1);
      if (n) HIP_CHECK(hipMemcpy(lidx, iota.data(), n * 4, hipMemcpyHostToDevice));
      if (n) HIP_CHECK(hipMemcpy(lgof, gof.data(), n * 4, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(L.goff.as<uint64_t>((uint64_t) n_groups + 1), group_off, goff_bytes, hipMemcpyHostToDevice));
      if (mode == 0)
        debug_mask_list(pairs, L, (long) w, ctx->stage.cb(), ctx->st);
      else
        fast_cluster_all(pairs, L, w, dcl, ctx->stage.cb(), ctx->st);
    }
    if (L.n > 2 * n) throw bk_error(BK_ERR_LIMIT, "bk_debug_points_groups: the list grew beyond 2 n entries");
    *n_out = (uint32_t) L.n;
    if (L.n)
    {
      HIP_CHECK(hipMemcpyAsync(idx_out, L.idx.get<uint32_t>(), L.n * 4, hipMemcpyDeviceToHost, ctx->st));
      if (mode == 2 && cluster_out) HIP_CHECK(hipMemcpyAsync(cluster_out, dcl.get<uint32_t>(), L.n * 4, hipMemcpyDeviceToHost, ctx->st));
    }
    if (goff_out)
    {
      // (without a point nothing ran and the list's offsets were never written: they are all 0)
      if (n)
        HIP_CHECK(hipMemcpyAsync(goff_out, L.goff.get<uint64_t>(), goff_bytes, hipMemcpyDeviceToHost, ctx->st));
      else
        memset(goff_out, 0, goff_bytes);
    }
    HIP_CHECK(hipStreamSynchronize(ctx->st));
  });
}

int bk_debug_points(bk_ctx *ctx, int mode, const uint32_t *x, const uint32_t *y, uint32_t n, double w, uint32_t *idx_out, int32_t *cluster_out, uint32_t *n_out)
{
  // one group holding the points in the given order
  const uint64_t goff[2] = {0, n};
  return bk_debug_points_groups(ctx, mode, x, y, goff, 1, w, idx_out, cluster_out, nullptr, n_out);
}

int bk_debug_cluster_info(uint64_t out[2])
{
  if (!out) return BK_ERR_ARG;
  out[0] = FW_TILE;
  out[1] = FW_LEVELS;
  return BK_OK;
}

int bk_debug_stream_info(uint64_t out[4])
{
  if (!out) return BK_ERR_ARG;
  try
  {
    stream_debug_info(out);
  }
  catch (const bk_error &e)
  {
    return e.code;
  }
  return BK_OK;
}

int bk_debug_stream_blocks(unsigned blocks)
{
  stream_debug_blocks(blocks);
  return BK_OK;
}

int bk_debug_cigar(bk_ctx *ctx, uint32_t n, const uint8_t *kind, const uint32_t *c1_off, const uint8_t *c1, const uint32_t *c2_off, const uint8_t *c2, const int32_t *e,
                   int32_t *out6)
{
  return guarded(ctx, [&] {
    if (!n) return;
    if (!kind || !c1_off || !c1 || !c2_off || !c2 || !e || !out6) throw bk_error(BK_ERR_ARG, "bk_debug_cigar: null argument");
    DevBuf dk, d1o, d1, d2o, d2, de, dout;
    HIP_CHECK(hipMemcpy(dk.as<uint8_t>(n), kind, n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d1o.as<uint32_t>(n + 1), c1_off, (n + 1) * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d1.as<uint8_t>(c1_off[n] + 16), c1, c1_off[n], hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d2o.as<uint32_t>(n + 1), c2_off, (n + 1) * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d2.as<uint8_t>(c2_off[n] + 16), c2, c2_off[n], hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(de.as<int32_t>(n), e, n * 4, hipMemcpyHostToDevice));
    int32_t *o = dout.as<int32_t>(6ull * n);
    debug_cigar(dk.get<uint8_t>(), d1o.get<uint32_t>(), d1.get<uint8_t>(), d2o.get<uint32_t>(), d2.get<uint8_t>(), de.get<int32_t>(), n, o, ctx->st);
    HIP_CHECK(hipMemcpyAsync(out6, o, 24ull * n, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipStreamSynchronize(ctx->st));
  });
}

int bk_debug_vote(bk_ctx *ctx, const bk_split *side1, uint32_t n1, const bk_split *side2, uint32_t n2, int32_t p1_tid, int32_t p2_tid, int32_t *out3)
{
  return guarded(ctx, [&] {
    if ((n1 && !side1) || (n2 && !side2) || !out3) throw bk_error(BK_ERR_ARG, "bk_debug_vote: null argument");
    // one cluster; side-1 tuples lie in its first region, side-2 tuples in its second one; two extra tuples per side that
    // match nothing keep find_sa_reads' "at least 2 evidence alignments" verdict out of the way (the vectors were taken
    // from find_bp_pair directly, BreakID.cc:577-857)
    const uint32_t pos1 = 100000, pos2 = 300000;
    std::vector<bk_split> t;
    auto put = [&](const bk_split *src, uint32_t n, int32_t tid, uint32_t pos, uint64_t salt) {
      for (uint32_t i = 0; i < n + 2; ++i)
      {
        bk_split s;
        if (i < n)
          s = src[i];
        else
        {
          memset(&s, 0, sizeof s);
          s.qhash = 0xD00D000000000000ull + salt + i;
          s.prim_chr = s.sec_chr = -7;
        }
        s.tid = tid;
        s.pos = (int32_t) pos;
        s.endpos = (int32_t) pos + 50;
        t.push_back(s);
      }
    };
    put(side1, n1, p1_tid, pos1, 0);
    put(side2, n2, p2_tid, pos2, 1000);
    // tuples must be in coordinate order
    std::stable_sort(t.begin(), t.end(), [](const bk_split &a, const bk_split &b) { return (uint32_t) a.tid != (uint32_t) b.tid ? (uint32_t) a.tid < (uint32_t) b.tid : a.pos < b.pos; });
    for (size_t i = 0; i < t.size(); ++i) t[i].rec = i;
    bk_cluster c;
    memset(&c, 0, sizeof c);
    c.p1_tid = p1_tid;
    c.p2_tid = p2_tid;
    c.p1_mean = pos1 + 10;
    c.p2_mean = pos2 + 10;
    c.p1_exact = 0xFFFFFFFFu;
    c.p2_exact = -1;
    DevBuf dt, dc, dcov;
    HIP_CHECK(hipMemcpy(dt.as<bk_split>(t.size() + 1), t.data(), t.size() * sizeof(bk_split), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dc.as<bk_cluster>(2), &c, sizeof c, hipMemcpyHostToDevice));
    const uint32_t cov[2] = {5, 5};
    HIP_CHECK(hipMemcpy(dcov.as<uint32_t>(4), cov, 8, hipMemcpyHostToDevice));
    bp_vote(dt.get<bk_split>(), t.size(), dc.get<bk_cluster>(), 1, 1000.0, 200, dcov.get<uint32_t>(), ctx->d_hdr.get<int32_t>(), ctx->bb, ctx->st);
    uint32_t voted = 0;
    HIP_CHECK(hipMemcpyAsync(&voted, ctx->bb.voted.get<uint32_t>(), 4, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipMemcpyAsync(&c, dc.get<bk_cluster>(), sizeof c, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipStreamSynchronize(ctx->st));
    out3[0] = voted ? (int32_t) c.p1_exact : -1;
    out3[1] = voted ? c.p2_exact : -1;
    out3[2] = voted ? (int32_t) c.n_sr : 0;
  });
}

int bk_debug_region(bk_ctx *ctx, int32_t tid, uint32_t start, uint32_t end, uint64_t depth_pos, bk_split *out, uint32_t cap, uint32_t *n_out, uint32_t *cov_out,
                    uint32_t *depth_out)
{
  return guarded(ctx, [&] {
    if (!ctx->stream_done) run_stream(ctx);
    ensure_splits_sorted(ctx);
    DevBuf dout, dres;
    bk_split *o = dout.as<bk_split>((uint64_t) cap + 1);
    uint32_t *res = dres.as<uint32_t>(4);
    debug_region(rec_view(ctx), ctx->d_split.get<bk_split>(), ctx->hc.n_split, tid, start, end, (int) ctx->hc.max_span, depth_pos, o, cap, res, ctx->st);
    uint32_t h[4] = {0, 0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(h, res, 16, hipMemcpyDeviceToHost, ctx->st));
    HIP_CHECK(hipStreamSynchronize(ctx->st));
    const uint32_t n = h[0] < cap ? h[0] : cap;
    if (n && out) HIP_CHECK(hipMemcpy(out, o, n * sizeof(bk_split), hipMemcpyDeviceToHost));
    if (n_out) *n_out = h[0];
    if (cov_out) *cov_out = h[1];
    if (depth_out) *depth_out = h[2];
  });
}

int bk_timing_enable(bk_ctx *ctx, int on)
{
  return guarded(ctx, [&] {
    ctx->timing = on != 0;
    for (auto &t : ctx->timers)
    {
      if (t.a) (void) hipEventDestroy(t.a);
      if (t.b) (void) hipEventDestroy(t.b);
    }
    ctx->timers.clear();
  });
}

int bk_timing(bk_ctx *ctx, const char *const **names, const float **ms, const uint64_t **bytes, int *n)
{
  return guarded(ctx, [&] {
    HIP_CHECK(hipStreamSynchronize(ctx->st));
    Timing &t = ctx->tout;
    t.names.clear(); t.ms.clear(); t.bytes.clear(); t.touched.clear(); t.cnames.clear();
    for (auto &s : ctx->timers)
    {
      float v = 0;
      HIP_CHECK(hipEventElapsedTime(&v, s.a, s.b));
      t.names.push_back(s.name);
      t.ms.push_back(v);
      t.bytes.push_back(s.bytes);
      t.touched.push_back(s.touched);
    }
    for (auto &s : t.names) t.cnames.push_back(s.c_str());
    if (names) *names = t.cnames.data();
    if (ms) *ms = t.ms.data();
    if (bytes) *bytes = t.bytes.data();
    if (n) *n = (int) t.names.size();
  });
}

int bk_timing_touched(bk_ctx *ctx, const uint64_t **touched, int *n)
{
  return guarded(ctx, [&] {
    if (touched) *touched = ctx->tout.touched.data();
    if (n) *n = (int) ctx->tout.touched.size();
  });
}

}  // extern "C"
