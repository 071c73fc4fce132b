// std::sort (libstdc++ introsort) emulation over all groups at once — see sortemu.hip.
#pragma once
#include "bk_common.h"
#include <vector>
#include <atomic>

// Resident sort service (sortsvc.inc): two persistent kernels that play the introsort replay of every std_sort_groups call made
// through a SortEmuBufs that points at a running service, as tasks.  One per device context; start() .. stop() bracket a stage.
struct SortService
{
  DevBuf ctl, slots[2], seq[2], jobs, dbg, pos[2];
  uint32_t pos_cap[2] = {0, 0};
  uint32_t cap[2] = {0, 0};
  hipStream_t st[2] = {nullptr, nullptr}, quit_stream = nullptr, st_copy = nullptr;
  uint32_t *quit_host = nullptr;  // mapped host memory the workgroups poll
  uint32_t *quit_dev = nullptr;
  uint32_t cap32 = 0;
  uint32_t quit_word = 0, starts = 0;
  size_t wide_lds = 0;
  bool running = false;
  std::atomic<uint32_t> next_slot{0};  // (the lanes' threads draw their slots at the same time)
  uint32_t stats[8] = {};
  // n_bound = elements of all lists that will be sorted while the service runs (sizes the task rings), max_group = the largest
  // group among them
  void start(uint64_t n_bound, uint64_t max_group, hipStream_t after);
  // has a narrow workgroup started within `seconds`?  (No: the narrow kernel's stream shares its hardware queue with the wide
  // kernel's and will wait behind it for ever.)
  bool narrow_running(double seconds) const;
  // ends the kernels; throws when a task reported an error
  void stop();
  uint32_t new_slot() { return next_slot.fetch_add(1u); }
  ~SortService();
  SortService() = default;
  SortService(const SortService &) = delete;
  SortService &operator=(const SortService &) = delete;
};

struct SortEmuBufs
{
  SortService *svc = nullptr;  // set (and running): std_sort_groups submits to it instead of dispatching the tasks itself
  uint32_t svc_slot = 0xFFFFFFFFu, svc_epoch = 0;
  DevBuf heap_scratch, scratch32, scratch32b, rk_a, rk_b, chk_key0, chk_cnt, chk_bad;
  // optional observer (host): heavy[g] = largest heapsort segment (elements) any task dispatch through these buffers met in group g
  // - what the lanes of lanes.hip balance on.  Set by the caller around the sorts it wants recorded.
  std::vector<uint32_t> *heavy = nullptr;
  bool heavy_all = false;  // record every segment that went to a heapsort task (a group that has one went through all ~2 lg n levels), not only the long ones
  // the sort as ONE task dispatch on the caller's stream (sortsvc.inc, k_sort_job) when no service runs: this caller's own queues,
  // job and position lists
  DevBuf tj_ctl, tj_jobs, tj_slots[2], tj_seq[2], tj_pos[2], tj_heavy, tj_trace;
  uint32_t tj_cap[2] = {0, 0}, tj_epoch = 0;
  bool tj_ready = false;  // the rings are initialised and consistent (a failed sort clears it)
  // sorts through these buffers by form: [0] jobs of the resident service, [1] task dispatches
  uint64_t sorts[2] = {0, 0};
  // the job statistics of the last sort through these buffers (bk_debug_sort_info): [0] its longest heap segment, [1] the elements in
  // its heap segments, as the task dispatch's look at its job read them; 0xFFFFFFFF = not read (a job of the resident service)
  uint32_t last_heap[2] = {0, 0};
  SortEmuBufs() = default;
  SortEmuBufs(const SortEmuBufs &) = delete;
  SortEmuBufs &operator=(const SortEmuBufs &) = delete;
};

// key/idx: n elements, groups are the contiguous ranges goff[g]..goff[g+1]; gof[p] = group of position p.
// On return every group is ordered exactly as std::sort(begin, end, [](a,b){return a.key < b.key;}) leaves it.
void std_sort_groups(uint32_t *key, uint32_t *idx, const uint32_t *gof, const uint64_t *goff, uint32_t ng, uint64_t n, SortEmuBufs &b, hipStream_t st);

// Test hook (bk_debug_sort_info): the constants of this build at which the replay changes its code path - FIN_MAX, HEAP_BIG_MIN,
// HEAP_RANKED_MAX, HEAP_LARGE, SVC_WIDE_MIN, F2_HB, F2_EXT, HEAP_PAD, SJ_MAX_WIDE, SJ_MAX_NARROW - and out[10] = cap32 of the task
// dispatch (the ranked heap entries that fit a wide workgroup's LDS, from the kernel's attributes on the current device).
constexpr int SORT_INFO_WORDS = 11;
void std_sort_info(uint64_t out[SORT_INFO_WORDS]);
