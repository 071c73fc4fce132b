// The mask-and-cluster stage (bk_mask_and_cluster): hardware-queue budget, resident sort service, lanes of chromosome-pair groups.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <thread>
#include <dirent.h>

#include "lanes.h"

// The hardware queues of the stage.  The runtime gives a process GPU_MAX_HW_QUEUES of them (ROCm's default: 4) and maps its
// streams onto them; two streams on one queue wait for each other's kernels, and a persistent kernel holds its queue for the whole
// stage.  So the budget is decided from the count the runtime started with, before any stream or persistent kernel of the stage
// exists:
//   service   LANE_STREAMS_MAX streams of the lanes + the two persistent kernels' streams + the copy stream of the quit word
//             (SortService::start) = 7 queues; below that nothing of the service is started (every sort of the stage is one task
//             dispatch on its lane's stream: the launch path)
//   launches  one queue stays with the process's first stream (the null stream of torch and of the runtime's copies: the kernel
//             trace at 4 queues shows it on a queue of its own, and the stage's fourth stream sharing a queue with another lane);
//             a lane has one stream and sorts on it; no more lanes than streams that get a queue each.  At ROCm's four queues
//             that is three lanes
static int g_hw_queues_at_init = 0;
void stage_set_hw_queues(int n) { g_hw_queues_at_init = n; }

static bool sort_service_on()
{
  // BREAKID_SORT_SERVICE=0: every std::sort replay as its own chain of launches (the earlier form)
  static const bool on = !(getenv("BREAKID_SORT_SERVICE") && atoi(getenv("BREAKID_SORT_SERVICE")) == 0);
  return on;
}
constexpr int LANE_STREAMS_MAX = 4;
constexpr int SVC_STAGE_QUEUES = LANE_STREAMS_MAX + 3;
static bool lane_service(int fast) { return sort_service_on() && fast && g_hw_queues_at_init >= SVC_STAGE_QUEUES; }
static int stage_queues() { return std::max(1, g_hw_queues_at_init - 1); }
static int lanes_wanted(bool svc)
{
  // with the resident sort service a lane's sort is a submit and a wait of its thread, so there can be a lane for every one or two
  // of the groups that carry long heap segments: twelve by default (each with a stream of its own; measured 12 / 16 / 18 / 24 lanes
  // on 12 streams: 30.6 / 33.4 / 34.3 / 35.7 ms for the stage - every lane costs its ~160 other launches)
  const char *env = getenv("BREAKID_GROUP_LANES");
  static const int want_svc = env ? atoi(env) : 12;
  if (svc) return want_svc < 1 ? 1 : (want_svc > 26 ? 26 : want_svc);
  // four lanes unless the caller says otherwise (BREAKID_GROUP_LANES=1: one pass); lanes_apply decides from the data whether they
  // pay.  Measured on the 30x WGS shape when a sort was still a chain of launches: 2 lanes 42.0 ms, 3 lanes 42.6, 4 lanes 39.6,
  // 5 lanes 48.5 (more lanes shorten a lane's "longest heap of any of its groups" per sort, and each costs the stage's other
  // launches once more).  Without an explicit count no more lanes than hardware queues (min(4, stage_queues())): a lane whose next
  // small kernel sits behind another lane's sort on a shared queue waits for that sort.
  static const int want = env ? atoi(env) : std::min(4, stage_queues());
  return want < 1 ? 1 : (want > 26 ? 26 : want);
}
static bool lanes_apply(const StageInput &in, int fast)
{
  static const uint64_t min_pairs = getenv("BREAKID_LANES_MIN_PAIRS") ? strtoull(getenv("BREAKID_LANES_MIN_PAIRS"), nullptr, 10) : (1ull << 20);  // below: launch-bound anyway
  // picked from the data: lanes pay when at least two groups are large enough to run into long sorts side by side
  uint32_t large = 0;
  const uint64_t big = std::max<uint64_t>(2, min_pairs >> 6);  // 16 K pairs with the default threshold
  for (uint32_t g = 0; g < in.jr.n_groups && g + 1 < in.gstart_host.size(); ++g) large += in.gstart_host[g + 1] - in.gstart_host[g] >= big ? 1u : 0u;
  const bool yes = lanes_wanted(lane_service(fast)) >= 2 && fast && in.jr.n_groups >= 4 && in.jr.n_pairs >= min_pairs && large >= 2;
  if (yes)
  {
    static bool told = false;
    const int K = lanes_wanted(lane_service(fast));
    if (!told && !lane_service(fast) && K > stage_queues() && bk_debug("lanes"))
    {
      told = true;
      fprintf(stderr, "[breakid] GPU_MAX_HW_QUEUES=%d: the lanes of chromosome-pair groups (bk_mask_and_cluster) and their heap kernels will share hardware queues "
                        "(BREAKID_GROUP_LANES=1: one pass)\n", g_hw_queues_at_init);
    }
  }
  return yes;
}

// The resident sort service runs while a SvcStage lives: every sort through the stage's (and its lanes') buffers is a job.
// Its two persistent kernels occupy a hardware queue each until the stage ends, so a stream of this stage that shares one of those
// queues (more streams in the process than the runtime has hardware queues: GPU_MAX_HW_QUEUES) would never get its turn.  That is
// why the stage (a) is the only one on its device (contexts of one process on one GPU - `-comm local` - take turns: the others sort
// by launches), and (b) probes every stream it is going to use after the kernels have started: an empty kernel that has not run
// after 50 ms sends the whole stage back to the launch path (the service stops, the stream drains).
__global__ void k_svc_probe() {}
// Compute queues that exist on the device right now, over ALL processes (the kernel driver's sysfs: /sys/class/kfd/kfd/proc/<pid>/
// queues/<n>/{gpuid,type}); -1 when that cannot be told.  Measured on MI355X: beyond 24 compute queues on a device - this process's
// 16-17 plus a second process holding 8 or more - the driver maps the queues in turns, and persistent kernels whose submitters wait
// for their turn leave jobs unfinished for seconds (4 streams held by a second process were fine, 8 were not: DESIGN.md, "Hardware queues").  The service runs only while the census stays at or below that.
static int kfd_compute_queues(int device)
{
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, (int) sizeof bus, device) != hipSuccess) return -1;
  unsigned dom = 0, b = 0, d = 0, f = 0;
  if (sscanf(bus, "%x:%x:%x.%x", &dom, &b, &d, &f) != 4) return -1;
  const unsigned long want_loc = (b << 8) | (d << 3) | f;
  auto read_file = [](const std::string &path, std::string &out) {
    FILE *fp = fopen(path.c_str(), "r");
    if (!fp) return false;
    char buf[4096];
    const size_t n = fread(buf, 1, sizeof buf - 1, fp);
    fclose(fp);
    buf[n] = 0;
    out = buf;
    return true;
  };
  auto list_dir = [](const std::string &path, std::vector<std::string> &names) {
    DIR *dp = opendir(path.c_str());
    if (!dp) return false;
    while (dirent *e = readdir(dp))
      if (e->d_name[0] != '.') names.push_back(e->d_name);
    closedir(dp);
    return true;
  };
  // the device's gpu_id: the topology node with its PCI location
  unsigned long gpu_id = 0;
  {
    std::vector<std::string> nodes;
    if (!list_dir("/sys/class/kfd/kfd/topology/nodes", nodes)) return -1;
    for (const std::string &n : nodes)
    {
      std::string props, id;
      const std::string base = "/sys/class/kfd/kfd/topology/nodes/" + n;
      if (!read_file(base + "/properties", props) || !read_file(base + "/gpu_id", id)) continue;
      unsigned long loc = ~0ul, domain = ~0ul;
      size_t p = props.find("location_id ");
      if (p != std::string::npos) loc = strtoul(props.c_str() + p + 12, nullptr, 10);
      p = props.find("domain ");
      if (p != std::string::npos) domain = strtoul(props.c_str() + p + 7, nullptr, 10);
      if (loc == want_loc && (domain == ~0ul || domain == dom) && strtoul(id.c_str(), nullptr, 10) != 0) gpu_id = strtoul(id.c_str(), nullptr, 10);
    }
  }
  if (!gpu_id) return -1;
  std::vector<std::string> procs;
  if (!list_dir("/sys/class/kfd/kfd/proc", procs)) return -1;
  int total = 0;
  for (const std::string &pid : procs)
  {
    std::vector<std::string> qs;
    const std::string qdir = "/sys/class/kfd/kfd/proc/" + pid + "/queues";
    if (!list_dir(qdir, qs)) continue;  // (another user's process: not readable - and not on a GPU this process may use either)
    for (const std::string &q : qs)
    {
      std::string g, t;
      if (!read_file(qdir + "/" + q + "/gpuid", g) || !read_file(qdir + "/" + q + "/type", t)) continue;
      if (strtoul(g.c_str(), nullptr, 10) == gpu_id && strtoul(t.c_str(), nullptr, 10) == 0) ++total;
    }
  }
  return total;
}
constexpr int SVC_MAX_DEVICE_QUEUES = 24;
static std::mutex g_svc_device_m[64];
// once per process on stderr: the stage sorts by launches although the service was wanted
static void tell_no_service()
{
  static std::atomic<bool> told{false};
  if (!getenv("BREAKID_QUIET") && !told.exchange(true))
    fprintf(stderr, "[breakid] the resident sort service shares a hardware queue with a stream of its own stage (GPU_MAX_HW_QUEUES too low for the streams of this process), or other processes hold hardware queues on this device: sorting by launches instead\n");
}
struct SvcStage
{
  ClusterStage &cs;
  hipStream_t st;  // the context's stream (lane 0's)
  bool on;
  std::unique_lock<std::mutex> device_turn;
  SvcStage(ClusterStage &s, int device, hipStream_t st, bool want, uint64_t n_bound, uint64_t max_group, const std::vector<hipStream_t> &streams)
      : cs(s), st(st), on(want && sort_service_on() && !s.svc_refused)
  {
    if (on && device >= 0 && device < 64)
    {
      device_turn = std::unique_lock<std::mutex>(g_svc_device_m[device], std::try_to_lock);
      on = device_turn.owns_lock();
    }
    if (!on) return;
    const auto ts0 = std::chrono::steady_clock::now();
    cs.svc.start(n_bound, max_group + 2, st);  // (+2: a mask may emit one element twice)
    const auto ts1 = std::chrono::steady_clock::now();
    // (the count is kept for a quarter of a second per device: reading it is ~0.5 ms of sysfs, and a sample's stages - or a bench's
    // steps - follow each other faster than processes come and go)
    int census;
    {
      static std::mutex cm;
      static std::chrono::steady_clock::time_point when[64];
      static int last[64];
      static bool have[64] = {};
      std::lock_guard<std::mutex> l(cm);
      const int d = device & 63;
      if (!have[d] || std::chrono::duration<double>(ts1 - when[d]).count() > 0.25)
      {
        last[d] = kfd_compute_queues(device);
        when[d] = std::chrono::steady_clock::now();
        have[d] = true;
      }
      census = last[d];
    }
    if (bk_debug("lanes"))
      fprintf(stderr, "[lanes] sort service started in %.3f ms; compute queues on the device (all processes): %d (counted in %.3f ms)\n", std::chrono::duration<double, std::milli>(ts1 - ts0).count(), census,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts1).count());
    const bool crowded = census > SVC_MAX_DEVICE_QUEUES;
    const bool behind = !crowded && !reachable(streams);
    const bool late = !crowded && !behind && !cs.svc.narrow_running(0.03);
    if (crowded || behind || late)
    {
      cs.svc.stop();
      on = false;
      // a stream behind a persistent kernel's queue or a crowded device stay that way: this context does not try again; a narrow
      // kernel that was merely late (a busy device) gets a second chance
      if (crowded || behind || ++cs.svc_late >= 2) cs.svc_refused = true;
      device_turn.unlock();
      tell_no_service();
      return;
    }
    cs.svc_late = 0;
    set(&cs.svc);
  }
  bool reachable(const std::vector<hipStream_t> &streams)
  {
    while (cs.svc_probe.size() < streams.size())
    {
      hipEvent_t e;
      HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      cs.svc_probe.push_back(e);
    }
    for (size_t k = 0; k < streams.size(); ++k)
    {
      hipLaunchKernelGGL(k_svc_probe, dim3(1), dim3(64), 0, streams[k]);
      HIP_CHECK(hipEventRecord(cs.svc_probe[k], streams[k]));
    }
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    bool ok = true;
    for (size_t k = 0; k < streams.size() && ok; ++k)
      for (;;)
      {
        const hipError_t e = hipEventQuery(cs.svc_probe[k]);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) throw bk_error(BK_ERR_HIP, std::string("sort service probe: ") + hipGetErrorString(e));
        if (since() > 0.05)
        {
          ok = false;
          break;
        }
      }
    // An empty kernel per stream comes back within ~0.1-0.3 ms.  Milliseconds mean that the device's hardware queues are
    // oversubscribed (other processes hold queues too: the scheduler then maps the queues in turns, and persistent kernels whose
    // submitters wait for their turn crawl - measured with a second process holding 16 queues: the stage 3-6 times slower or a job
    // that never finished) - no service then either.
    const double took = since();
    if (bk_debug("lanes")) fprintf(stderr, "[lanes] sort service probe: %zu streams in %.3f ms%s\n", streams.size(), took * 1e3, ok ? "" : " (gave up)");
    return ok && took < 0.003;
  }
  void set(SortService *s)
  {
    for (auto &l : cs.lanes)
    {
      l->cb.se.svc = s;
      l->cb.se.svc_slot = 0xFFFFFFFFu;
    }
  }
  void finish()
  {
    if (!on) return;
    on = false;
    set(nullptr);
    // every job has been waited for by its caller: the streams must be through before the workgroups are told to leave
    hipError_t e = hipStreamSynchronize(st);
    for (auto &l : cs.lanes)
      if (l->st && e == hipSuccess) e = hipStreamSynchronize(l->st);
    cs.svc.stop();
    device_turn.unlock();
    if (e != hipSuccess) throw bk_error(BK_ERR_HIP, std::string("sort service: ") + hipGetErrorString(e));
  }
  ~SvcStage()
  {
    try
    {
      finish();
    }
    catch (const bk_error &)
    {
    }
  }
};

// the list as it stands after masking, kept (for bk_fetch and bk_group_stats, and for the merge of the lanes) before clustering
// thins L; gof only where a merge is going to need it
static void snapshot_list(const PairList &L, DevBuf &idx, DevBuf *gof, DevBuf &goff, hipStream_t st)
{
  uint32_t *ii = idx.as<uint32_t>(L.n + 1), *ig = gof ? gof->as<uint32_t>(L.n + 1) : nullptr;
  uint64_t *io = goff.as<uint64_t>((uint64_t) L.ng + 1);
  if (L.n) HIP_CHECK(hipMemcpyAsync(ii, L.idx.get<uint32_t>(), L.n * 4, hipMemcpyDeviceToDevice, st));
  if (L.n && ig) HIP_CHECK(hipMemcpyAsync(ig, L.gof.get<uint32_t>(), L.n * 4, hipMemcpyDeviceToDevice, st));
  if (L.ng) HIP_CHECK(hipMemcpyAsync(io, L.goff.get<uint64_t>(), ((uint64_t) L.ng + 1) * 8, hipMemcpyDeviceToDevice, st));
}
// clusters the masked list, fast or exact: L becomes the clustered list, cl its cluster numbers
static void cluster_list(const bk_pair *pairs, PairList &L, double w, int fast, DevBuf &cl, ClusterBufs &cb, AhcBufs &ab, hipStream_t st)
{
  if (fast)
    fast_cluster_all(pairs, L, w, cl, cb, st);
  else
    ahc_cluster_all(pairs, L, w, cl, ab, cb, st);
}

// K lanes of groups.  The reference clusters its chromosome-pair groups one after the other and independently of each other
// (BreakID.cc:119-167).  All groups in one pass pay, in each of the five sorts, the longest heapsort segment of ANY group; disjoint
// sets of groups on streams of their own, each driven by its own host thread, overlap the lone-wave heaps of one set with the
// bandwidth- and launch-bound partition levels of the others.  A lane's time is (a) per sort the LONGEST heapsort segment of any of
// its groups - a serial chain of one wave - plus (b) partition levels and masks in proportion to its pairs plus (c) a fixed number
// of launch-bound late levels.  Which groups own long heap segments cannot be told from their sizes (all same-chromosome groups of
// a WGS sample are about equally large; two or three of them carry segments of 30-46 K elements, most carry a few thousand), but
// on the launch path it can be OBSERVED: a group whose sort by x (by y) ran into the depth limit does so again in the next sort by
// the same coordinate.  So there the stage runs in two parts:
//   part 1  sorts 1-3 (x, mask, y, mask, x: remove_isolated_pairs) in K lanes split blindly (longest-processing-time on size^e);
//           every lane records the longest heap segment of each of its groups in the sort by y and in the LAST sort by x;
//   part 2  sorts 4-5 (x-windows, y, y-windows, x) in K lanes split on what was observed: the groups are placed, heaviest
//           chain first, where the lane's longest segment by y + longest segment by x (+ a term for its pair count) grows least.
// On the 30x WGS shape part 2 comes out balanced (18.9 / 21.4 ms with two lanes) where the blind split leaves one lane 9 ms behind
// the other (46.6 / 37 ms); part 1 stays as the blind split leaves it (24.1 / 21.3 ms); the barrier and the re-split cost ~1 ms.
// Under the resident sort service (which does not report heap segments back to the host) the blind split holds for all five sorts,
// over more lanes than streams (lanes_wanted, group_lanes).
// Results are identical whatever the split: the groups never interact, a lane's list keeps every group's order, and the lists are
// merged back into group order.
using LanePlan = std::vector<int>;  // the lane of every group; -1: none of this rank's (sharded sample: bk_shard_own_groups)
// every group this rank masks and clusters in lane 0, the others in none
static LanePlan plan_owned(const StageInput &in)
{
  const uint32_t ng = in.jr.n_groups;
  const bool owned_only = !in.own_groups.empty();
  if (owned_only && in.own_groups.size() != ng) throw bk_error(BK_ERR_ARG, "bk_shard_own_groups: group count changed");
  LanePlan p(ng, 0);
  for (uint32_t g = 0; owned_only && g < ng; ++g)
    if (!in.own_groups[g]) p[g] = -1;
  return p;
}
static LanePlan plan_blind(const StageInput &in, int K)
{
  const uint32_t ng = in.jr.n_groups;
  std::vector<uint32_t> order(ng);
  std::iota(order.begin(), order.end(), 0u);
  auto size_of = [&](uint32_t g) { return in.gstart_host[g + 1] - in.gstart_host[g]; };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return size_of(a) > size_of(b); });
  constexpr double wexp = 2.0;  // longest-processing-time on size^2
  LanePlan p = plan_owned(in);
  std::vector<double> load(K, 0.0);
  for (uint32_t i = 0; i < ng; ++i)
  {
    const uint32_t g = order[i];
    if (p[g] < 0) continue;
    int l = 0;
    for (int k = 1; k < K; ++k)
      if (load[k] < load[l]) l = k;
    load[l] += std::pow((double) size_of(g), wexp);
    p[g] = l;
  }
  return p;
}
// sizes = pairs per group now; hx / hy = longest heap segment per group seen in a sort by x / by y (0: none)
static LanePlan plan_observed(const std::vector<uint64_t> &sizes, const std::vector<uint32_t> &hx, const std::vector<uint32_t> &hy, int K)
{
  const uint32_t ng = (uint32_t) sizes.size();
  // in units of one pop of a lone wave in LDS (~0.15 us): a pair costs a lane ~0.15 ns in the two sorts that are left (most of a
  // lane's time outside the heaps is a fixed number of launches), an element of a heap segment beyond what fits the LDS of a
  // CU costs twice as much (the hybrid loop: 0.30 us per pop while the heap's tail is in global memory)
  constexpr double per_pair = 0.001;
  auto heap_cost = [](uint32_t m) { return (double) m + (m > 40947u ? 1.0 * (double) (m - 40947u) : 0.0); };
  std::vector<uint32_t> order(ng);
  std::iota(order.begin(), order.end(), 0u);
  auto chain = [&](uint32_t g) { return heap_cost(hx[g]) + heap_cost(hy[g]); };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const double ca = chain(a), cb = chain(b);
    return ca != cb ? ca > cb : sizes[a] > sizes[b];
  });
  LanePlan p(ng, 0);
  std::vector<double> mx(K, 0.0), my(K, 0.0), pairs(K, 0.0);
  auto cost = [&](int l) { return mx[l] + my[l] + per_pair * pairs[l]; };  // one sort by x and one by y are left
  for (uint32_t g : order)
  {
    int best = 0;
    double best_cost = 0;
    for (int l = 0; l < K; ++l)
    {
      const double c = std::max(mx[l], heap_cost(hx[g])) + std::max(my[l], heap_cost(hy[g])) + per_pair * (pairs[l] + (double) sizes[g]);
      // the lane whose own cost ends lowest takes the group (ties: the emptier lane)
      if (l == 0 || c < best_cost || (c == best_cost && cost(l) < cost(best)))
      {
        best = l;
        best_cost = c;
      }
    }
    mx[best] = std::max(mx[best], heap_cost(hx[g]));
    my[best] = std::max(my[best], heap_cost(hy[g]));
    pairs[best] += (double) sizes[g];
    p[g] = best;
  }
  if (bk_debug("lanes"))
    for (int l = 0; l < K; ++l)
    {
      fprintf(stderr, "[lanes] lane %d: max heap x %.0f y %.0f, %.0f pairs, cost %.0f; heavy groups:", l, mx[l], my[l], pairs[l], cost(l));
      for (uint32_t g = 0; g < ng; ++g)
        if (p[g] == l && (hx[g] || hy[g])) fprintf(stderr, " %u(%u,%u)", g, hx[g], hy[g]);
      fprintf(stderr, "\n");
    }
  return p;
}
// the plan on the device, one row of ng + 1 words per lane in one copy: row l holds 1 for the groups lane l leaves alone (what
// another lane, or another rank, owns); the stream is through when this returns
static uint32_t *upload_drop(const LanePlan &p, int K, DevBuf &buf, hipStream_t st)
{
  const size_t row = p.size() + 1;
  std::vector<uint32_t> drop((size_t) K * row, 0u);
  for (int l = 0; l < K; ++l)
    for (size_t g = 0; g + 1 < row; ++g) drop[(size_t) l * row + g] = p[g] == l ? 0u : 1u;
  uint32_t *d = buf.as<uint32_t>(drop.size() + 1);
  HIP_CHECK(hipMemcpyAsync(d, drop.data(), drop.size() * 4, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipStreamSynchronize(st));
  return d;
}

static void group_lanes(ClusterStage &cs, const StageInput &in, double w, int fast)
{
  const uint32_t ng = in.jr.n_groups;
  static const bool dbg = bk_debug("lanes");  // (the timing lines below; the others ask at every call)
  // With the resident sort service a lane's stream is idle most of the time (its thread waits for the sort's job), so the twelve
  // lanes share FOUR streams (LANE_STREAMS_MAX): measured 12 lanes on 12 / 8 / 4 streams 44.5-44.8 / 44.4-44.7 / 44.5-45.2 ms per
  // step (6 streams, two heavy lanes per stream: 46.7-47.4; round-4 start, with waiting kernels on the streams: 12 / 4 / 3 / 2
  // streams 31.6 / 31.2 / 35.0 / 40.2 ms for the stage).  Fewer streams = fewer hardware queues: the stage then needs 4 + 3 of
  // them (SVC_STAGE_QUEUES), and a second process on the device (a test runner's parent, another sample) leaves the device's
  // queues uncrowded (SVC_MAX_DEVICE_QUEUES).
  auto make_lanes = [&](int K, int S) {
    while ((int) cs.lanes.size() < K)
    {
      cs.lanes.emplace_back(new ClusterStage::Lane());
      cs.lanes.back()->cb.max_group_bound = cs.cb().max_group_bound;
    }
    for (int k = 1; k < S; ++k)
      if (!cs.lanes[k]->st) HIP_CHECK(hipStreamCreateWithFlags(&cs.lanes[k]->st, hipStreamNonBlocking));
  };
  bool use_svc = sort_service_on() && fast;
  if (use_svc && !lane_service(fast))
  {
    // too few hardware queues for the service and the lanes' streams: nothing of the service is started
    use_svc = false;
    tell_no_service();
    if (bk_debug("lanes")) fprintf(stderr, "[lanes] %d hardware queues, the sort service needs %d: not started\n", g_hw_queues_at_init, SVC_STAGE_QUEUES);
  }
  int K = lanes_wanted(use_svc);
  int S = use_svc ? std::max(1, std::min(LANE_STREAMS_MAX, K)) : K;
  make_lanes(K, S);
  std::vector<hipStream_t> stage_streams{in.st};
  for (int k = 1; k < S; ++k) stage_streams.push_back(cs.lanes[k]->st);
  SvcStage svc_stage(cs, in.device, in.st, use_svc, in.jr.n_pairs + 2ull * ng + 4096, cs.cb().max_group_bound, stage_streams);  // the service runs from here to the end of the lanes (also when one of them throws)
  if (use_svc && !svc_stage.on)
  {
    // the service is not to be had (another context of this process has it on this device, or a hardware queue is shared): the lanes of the launch path
    use_svc = false;
    K = lanes_wanted(false);
    S = K;
    make_lanes(K, S);
  }
  if (!use_svc && bk_debug("lanes"))
  {
    fprintf(stderr, "[lanes] launch path: %d lanes, 1 stream each, %d hardware queues\n", K, g_hw_queues_at_init);
    fprintf(stderr, "[lanes] sorts as task dispatches on the lane streams\n");
  }
  auto lane = [&](int l) -> ClusterStage::Lane & { return *cs.lanes[l]; };
  auto lane_st = [&](int l) { const int k = l % S; return k == 0 ? in.st : cs.lanes[k]->st; };
  uint32_t *drop_base = nullptr;  // the lanes' plans on the device (upload_drop)
  auto lane_drop = [&](int l) { return drop_base + (size_t) l * ((size_t) ng + 1); };
  std::vector<std::vector<uint8_t>> keep(K, std::vector<uint8_t>(ng, 0));  // keep[l][g]: lane l owns group g (host copy of the plan)
  auto upload_plan = [&](const LanePlan &p) {
    for (int l = 0; l < K; ++l)
      for (uint32_t g = 0; g < ng; ++g) keep[l][g] = p[g] == l ? 1 : 0;
    drop_base = upload_drop(p, K, cs.d_drop, in.st);  // (the pair table and the masks are ready for all lanes when the stream is through)
  };
  // runs body(l) for every lane, lane 0 on this thread; the lanes' streams are synchronised when this returns
  auto in_lanes = [&](auto body) {
    std::vector<std::string> err(K);
    std::vector<int> code(K, BK_OK);
    const auto t_start = std::chrono::steady_clock::now();
    auto guarded_body = [&](int l) {
      try
      {
        body(l);
        HIP_CHECK(hipStreamSynchronize(lane_st(l)));
        if (dbg)
          fprintf(stderr, "[lanes] lane %d done after %.2f ms\n", l, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
      }
      catch (const bk_error &e)
      {
        code[l] = e.code;
        err[l] = e.msg;
      }
    };
    std::vector<std::thread> th;
    for (int l = 1; l < K; ++l)
      th.emplace_back([&, l] {
        (void) hipSetDevice(in.device);
        guarded_body(l);
      });
    guarded_body(0);
    for (std::thread &t : th) t.join();
    for (int l = 0; l < K; ++l)
      if (code[l] != BK_OK) throw bk_error(code[l], err[l]);
  };
  // folds the lanes' lists (disjoint groups) into one list in group order; cl_out: the cluster numbers travel along
  auto merge_all = [&](PairList ClusterStage::Lane::*which, PairList &out, DevBuf *cl_out) {
    std::vector<const PairList *> ls(K);
    std::vector<const uint32_t *> cls(K);
    for (int l = 0; l < K; ++l)
    {
      ls[l] = &(lane(l).*which);
      cls[l] = lane(l).d_cluster.get<uint32_t>();
    }
    merge_lists_many(ls.data(), cl_out ? cls.data() : nullptr, K, out, cl_out, in.st);
  };
  const bk_pair *pairs = in.jr.pairs;
  // sorts 1-3 of lane l: its groups' pairs masked; observe: the longest heap segment of every group is recorded in cb.heavy_y
  // (the sort by y) and cb.heavy_x (the third sort, by x on the masked list: the one that tells about the fifth)
  auto mask_lane = [&](int l, bool observe) {
    ClusterBufs &cb = lane(l).cb;
    if (observe)
    {
      cb.heavy_x.assign(ng, 0u);
      cb.heavy_y.assign(ng, 0u);
      cb.observe = true;
      cb.se.heavy_all = false;
    }
    remove_isolated_begin(pairs, in.jr.gof, in.jr.gstart, ng, in.jr.n_pairs, w, lane(l).list, cb, lane_st(l), lane_drop(l), in.gstart_host.data(), keep[l].data());
    if (observe) cb.heavy_x.assign(ng, 0u);
    remove_isolated_end(pairs, lane(l).list, cb, lane_st(l));
    if (observe) cb.observe = false;
  };
  // sorts 4-5 of lane l: its masked list kept, then clustered
  auto cluster_lane = [&](int l) {
    PairList &L = lane(l).list, &iso = lane(l).iso;
    iso.n = L.n;
    iso.ng = L.ng;
    snapshot_list(L, iso.idx, &iso.gof, iso.goff, lane_st(l));
    cluster_list(pairs, L, w, fast, lane(l).d_cluster, lane(l).cb, cs.ab, lane_st(l));
  };
  const auto tp0 = std::chrono::steady_clock::now();
  auto phase = [&](const char *what) {
    if (dbg) fprintf(stderr, "[lanes] %s at %.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count());
  };
  upload_plan(plan_blind(in, K));
  phase("plan uploaded");
  if (use_svc)  // (the service does not report the groups' longest heap segments back to the host: the blind deal stays)
    in_lanes([&](int l) {
      mask_lane(l, false);
      cluster_lane(l);
    });
  else
  {
    // part 1: sorts 1-3, observed.  (Dealing again after the second sort already - x from the first sort, y from the second, three
    // sorts left - was measured worse, 42.0 ms against 38.1: the heaps of the FIRST sort by x, short, on the unmasked list, say
    // little about the later ones.)
    in_lanes([&](int l) { mask_lane(l, true); });
    PairList &mid = cs.lane_mid;
    merge_all(&ClusterStage::Lane::list, mid, nullptr);
    std::vector<uint64_t> goff_h((size_t) ng + 1);
    HIP_CHECK(hipMemcpyAsync(goff_h.data(), mid.goff.get<uint64_t>(), ((size_t) ng + 1) * 8, hipMemcpyDeviceToHost, in.st));
    HIP_CHECK(hipStreamSynchronize(in.st));
    std::vector<uint64_t> sizes(ng);
    std::vector<uint32_t> hx(ng, 0u), hy(ng, 0u);
    for (uint32_t g = 0; g < ng; ++g) sizes[g] = goff_h[g + 1] - goff_h[g];
    for (int l = 0; l < K; ++l)
      for (uint32_t g = 0; g < ng; ++g)
      {
        hx[g] = std::max(hx[g], lane(l).cb.heavy_x[g]);
        hy[g] = std::max(hy[g], lane(l).cb.heavy_y[g]);
      }
    upload_plan(plan_observed(sizes, hx, hy, K));
    // part 2: sorts 4, 5 on the new deal
    in_lanes([&](int l) {
      list_subset_ranges(mid, goff_h.data(), keep[l].data(), lane(l).list, lane_st(l));
      cluster_lane(l);
    });
  }
  phase("lanes done");
  svc_stage.finish();  // (throws what a task reported)
  phase("service stopped");
  if (use_svc && bk_debug("lanes")) fprintf(stderr, "[svc] tasks: %u wide, %u narrow\n", cs.svc.stats[0], cs.svc.stats[1]);
  // one list in group order again
  PairList &iso_m = cs.lane_iso_m;
  merge_all(&ClusterStage::Lane::iso, iso_m, nullptr);
  merge_all(&ClusterStage::Lane::list, cs.list, &cs.d_cluster);
  HIP_CHECK(hipStreamSynchronize(in.st));
  phase("lists merged");
  cs.iso_n = iso_m.n;
  std::swap(cs.iso_idx, iso_m.idx);
  std::swap(cs.iso_goff, iso_m.goff);
}

void ClusterStage::run(const StageInput &in, double w, int fast)
{
  uint64_t mg = 0;
  for (uint32_t g = 0; g < in.jr.n_groups && g + 1 < in.gstart_host.size(); ++g) mg = std::max<uint64_t>(mg, in.gstart_host[g + 1] - in.gstart_host[g]);
  for (auto &l : lanes) l->cb.max_group_bound = mg;
  if (lanes_apply(in, fast))
  {
    in.timed("mask_and_cluster_lanes", [&] { group_lanes(*this, in, w, fast); });
    return;
  }
  // one pass over all groups on the context's stream.  (Unlike the lanes it asks for the service without looking at the queue budget.)
  SvcStage svc_stage(*this, in.device, in.st, true, in.jr.n_pairs + 2ull * in.jr.n_groups + 4096, cb().max_group_bound, {in.st});
  in.timed("remove_isolated", [&] {
    // sharded sample: this rank masks and clusters only the chromosome-pair groups it owns
    const uint32_t *drop = in.own_groups.empty() ? nullptr : upload_drop(plan_owned(in), 1, d_drop, in.st);
    remove_isolated_all(in.jr.pairs, in.jr.gof, in.jr.gstart, in.jr.n_groups, in.jr.n_pairs, w, list, cb(), in.st, drop);
  });
  iso_n = list.n;
  snapshot_list(list, iso_idx, nullptr, iso_goff, in.st);
  if (!fast) svc_stage.finish();  // (the exact UPGMA replay sorts nothing and may take long: the service's workgroups would hold their CUs, then leave on their own)
  in.timed(fast ? "fast_cluster" : "ahc_cluster", [&] { cluster_list(in.jr.pairs, list, w, fast, d_cluster, cb(), ab, in.st); });
  svc_stage.finish();
}

void ClusterStage::sort_forms(uint64_t out[3]) const
{
  out[0] = out[1] = out[2] = 0;  // (out[2] counted a form that no longer exists)
  for (const auto &l : lanes)
    for (int k = 0; k < 2; ++k) out[k] += l->cb.se.sorts[k];
}

void ClusterStage::debug_sort(int device, hipStream_t st, uint32_t *key, uint32_t *idx, const uint32_t *gof, const uint64_t *goff, uint32_t ng, uint64_t n, uint64_t max_group)
{
  SvcStage svc_stage(*this, device, st, true, n + 2ull * ng + 4096, max_group, {st});
  std_sort_groups(key, idx, gof, goff, ng, n, cb().se, st);
  svc_stage.finish();
}
