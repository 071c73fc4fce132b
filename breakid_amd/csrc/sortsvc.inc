// Resident sort service: the introsort replay of sortemu.hip as TASKS of two persistent kernels instead of launches.
// (included by sortemu.hip inside its anonymous namespace: the partition, finisher and heap bodies are the ones above)
//
// Why.  A std::sort of the reference (BreakID.cc:1091,1127,1274,1278,1282) replayed with kernels is a chain of ~100 dependent
// launches and host looks - partition levels, rounds of the tail, heaps, finisher, the finisher's heaps - whatever the data,
// i.e. 1.5-2.8 ms per sort in front of and behind the one thing that is inherently serial (the pops of the longest heap
// segment).  Here a sort is a set of tasks: a partition node pushes its children, a finished segment counts its elements off the
// job's `remaining`, the job is done when that reaches zero.  Nothing waits for a launch boundary: the critical path of a sort
// becomes root partition -> spine -> heap of ITS longest segment, and a lane of groups (lanes.hip) costs a submit kernel and a wait of
// its THREAD per sort instead of a hundred launches (the thread polls a word in host memory that the task which counts the job's
// last elements off writes: a kernel spinning on the lane's stream instead made every other queue's dependent launches 7x slower).
//
// Workgroups.  `wide` ones (1024 threads, all of a CU's LDS): heaps above HEAP_BIG_MIN elements (ranked 4-byte entries, sixteen
// waves rank and build, one wave pops) and partition nodes above SVC_WIDE_MIN elements.  `narrow` ones (256 threads, 44 KB): the
// smaller partition nodes, the finisher (segments of at most FIN_MAX elements, entirely in LDS) and the heaps of at most
// HEAP_BIG_MIN elements.  Each kind pulls from its own queue; a task never waits for another task, so any resident workgroup
// makes progress and the kernels' grids need not be co-resident.
//
// Visibility (per-XCD L2s, per-CU L1s; MI355X_MICROARCH.md, inter-workgroup visibility).  Everything a task leaves for another
// workgroup - the keys and payloads it has swapped or written back - is stored WRITE-THROUGH (sc1, st_through), every wave waits
// for its stores (s_waitcnt vmcnt(0)), the workgroup meets, and lane 0 touches the queue / the job's counter; a task starts with
// lane 0's polls -> ONE agent-scope acquire -> s_waitcnt vmcnt(0) -> __syncthreads -> plain loads (the guide's R1 form).
// In front of every push lane 0 also runs an agent-scope release (buffer_wbl2 + wait; +0.5 ms per stage): without it one task
// in ~10^7 started on keys that were not all there yet (a partition whose two passes saw different keys: 1 failure in ~80 bench
// steps, none in 170 with the release; SvcQueue::release bit 0 switches it, bit 1 adds it in front of every retire as well: +1.3 ms).  The
// write-through stores keep that release cheap (next to nothing is dirty).  What a workgroup writes with plain stores
// is private to it: its own slice of position lists (per workgroup, never shared) and the heaps' scratch arrays, whose addresses
// only one task of a sort touches; between two sorts lie kernel boundaries (the window sorts, the lane's other kernels), which
// write back every L2.  Queue words, task slots, job descriptors, the error and the quit word are only touched by atomic
// read-modify-writes, on both sides (svc_read / svc_write below, with what was seen without them).
// Hardware queues.  The two kernels hold a queue each until the stage ends; what that asks of the process and of the device is
// handled where the stage starts (lanes.hip: SvcStage - one stage per device, probes of the stage's streams, the census of the
// device's compute queues) and where it stops (SortService::stop: the quit word by two routes).

constexpr uint32_t SVC_T_PART = 1, SVC_T_FIN = 2, SVC_T_HEAP = 3;
constexpr uint32_t SVC_WIDE_MIN = 16384;    // partition nodes above this size go to the wide workgroups
constexpr uint32_t SVC_BIAS = 0x80000000u;  // held in `remaining` while the groups of a job are being submitted
constexpr uint32_t SVC_MAX_JOBS = 64;
constexpr uint32_t SVC_H_QUIT = 0, SVC_H_ERROR = 1, SVC_H_NARROW = 8, SVC_H_STARTED = 16, SVC_H_DONE = SVC_H_STARTED + 1024, SVC_H_WORDS = SVC_H_DONE + SVC_MAX_JOBS;
constexpr uint32_t SVC_NARROW_LDS = 45056;  // Fin2Lds and (HEAP_BIG_MIN + HEAP_PAD) * 8 fit (static_asserts below)
constexpr unsigned long long SVC_TIMEOUT_TICKS = 800000000ull;  // 8 s of wall_clock64 (100 MHz): a workgroup that saw no task for that long leaves

struct SvcTask
{
  uint32_t type_job;  // type | job slot << 4 | epoch << 12
  uint32_t first, last;
  int32_t depth;
};
static_assert(sizeof(SvcTask) == 16, "two 8-byte halves");

// one std::sort call over the groups of a list.  Written by k_svc_submit, read by the workgroups with agent-scope loads.
struct SvcJob
{
  uint32_t *key, *idx, *posL, *posR;  // (posL, posR: null, read by nobody; the descriptor keeps its nine leading 8-byte words)
  hent *hscratch;
  uint32_t *scratch32, *scratch32b;
  unsigned long long *rka, *rkb;
  uint32_t remaining;  // elements that are not final yet (+ SVC_BIAS while the job is being submitted)
  uint32_t done;       // 1 = every segment is final
  uint32_t max_heap;   // longest heap segment (statistics)
  uint32_t n_heap;     // elements in heap segments
  uint32_t epoch;
  uint32_t pad[3];
  // (BK_DEBUG=svc) 10 ns ticks: when the job was submitted, when its last partition / finisher task ended, when it was done; the heap
  // task that ended last: ticks it took << 32 | elements
  unsigned long long t_submit, t_parts, t_done, last_heap;
};
static_assert(sizeof(SvcJob) % 8 == 0, "copied in 8-byte words");

struct SvcQueue
{
  uint32_t *head, *tail;  // on cache lines of their own
  SvcTask *slots;
  uint32_t *seq;
  uint32_t mask;
  uint32_t release;  // (q[0]) bit 0: an agent-scope release in front of every push, bit 1: in front of every retire too (visibility note)
};
struct SvcParams
{
  SvcQueue q[2];           // 0 = wide, 1 = narrow
  SvcJob *jobs;            // SVC_MAX_JOBS
  uint32_t *error;         // != 0: a task failed, everybody leaves
  uint32_t *quit_d;        // the host's "no more jobs" (device memory: k_svc_quit, launched on the stage's own stream, writes it)
  uint32_t *host;          // host memory (mapped): [SVC_H_NARROW] set by the
                           // first narrow workgroup that runs, [SVC_H_ERROR] a task's error as the workgroups saw it, [SVC_H_STARTED ..] one word per wide
                           // workgroup, set when it runs, [SVC_H_DONE + slot] the epoch of the slot's last finished job
  uint32_t *stats;         // [0] tasks, [1] idle polls, ...
  uint32_t cap32;          // ranked entries that fit a wide workgroup's LDS (odd)
  uint32_t quit_word;      // what *quit reads when the host wants the workgroups to leave (0 = carry on)
  unsigned long long timeout_ticks;
  uint32_t *pos[2];        // position lists of the partition nodes: 2 * pos_cap[k] words per workgroup of kind k
  uint32_t pos_cap[2];
  uint32_t *dbg;           // (BK_DEBUG=svc) four words per workgroup, wide ones first: state, polls, last head, last seq read
};

// a task failed: the code for the host (svc.stop() throws it), the first failing task's description for BK_DEBUG=svc
#define SVC_FAIL(P, code, a, b, c)                                  \
  do                                                                \
  {                                                                 \
    if (atomicOr((P).error, (code)) == 0u)                          \
    {                                                               \
      (P).error[8] = (code);                                        \
      (P).error[9] = (a);                                           \
      (P).error[10] = (b);                                          \
      (P).error[11] = (c);                                          \
    }                                                               \
  } while (0)
#define SVC_LD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
// Control words that another workgroup changes while this one waits for them (sequence words, task slots, job descriptors, the
// error and quit words) are read with an atomic read-modify-write: it is performed where the device's atomics meet, whatever an
// XCD's L2 still holds of the line.  A relaxed agent-scope LOAD is served by the XCD's L2, and a poll loop of such loads was seen
// to return the old value for ever once nothing else on that XCD invalidated the line (a second process holding hardware queues
// on the GPU, every workgroup idle: 50 of 4 018 pushed tasks never seen by the workgroups whose tickets they carried).
__device__ __forceinline__ uint32_t svc_read(uint32_t *p) { return atomicAdd(p, 0u); }
__device__ __forceinline__ unsigned long long svc_read(unsigned long long *p) { return atomicAdd(p, 0ull); }
// ... and written by an atomic exchange: a read-modify-write poll and a plain (write-through) store of the same word are not
// performed at the same place, and a poll that wrote its old value back over a store that had just landed would lose a task for
// good (one bench run in ten ended with "a job did not finish" while the polls were atomics and the publications stores).
__device__ __forceinline__ void svc_write(uint32_t *p, uint32_t v) { (void) atomicExch(p, v); }
__device__ __forceinline__ void svc_write(unsigned long long *p, unsigned long long v) { (void) atomicExch(p, v); }
#define SVC_ST(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
__device__ __forceinline__ void svc_release()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the compiler may drop the wait behind buffer_wbl2: MI355X_MICROARCH.md, compiler hazard)
}
__device__ __forceinline__ void svc_acquire()
{
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// every wave of the workgroup: its global stores have left the wave, then the workgroup meets (what lane 0 releases afterwards is
// everything the workgroup has written)
template <class T = WgTeam> __device__ __forceinline__ void svc_drain_barrier(const T &team = T())
{
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  team.sync();
}

// one lane.  The caller has released the data the task stands for.
__device__ __forceinline__ void svc_push(const SvcQueue &q, const SvcTask t, uint32_t *error)
{
  const uint32_t pos = atomicAdd(q.tail, 1u);
  const uint32_t slot = pos & q.mask;
  // the slot is free once the pop of the lap before has read it (never spins unless the ring is full)
  for (uint32_t spins = 0; svc_read(q.seq + slot) != pos; ++spins)
  {
    __builtin_amdgcn_s_sleep(16);
    if (spins > (1u << 22) || svc_read(error) != 0)
    {
      atomicOr(error, 2u);  // ring overflow
      return;
    }
  }
  unsigned long long *d = reinterpret_cast<unsigned long long *>(q.slots + slot);
  svc_write(d, (unsigned long long) t.type_job | ((unsigned long long) t.first << 32));
  svc_write(d + 1, (unsigned long long) t.last | ((unsigned long long) (uint32_t) t.depth << 32));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  svc_write(q.seq + slot, pos + 1u);
}
// Taking a task, one lane.  A workgroup that wants work draws a TICKET (one fetch-add on the head: the position in the ring it
// will be served from) and then polls the sequence word of that slot only - its own address, no other poller's.  (The first form
// read the head and raced for it with a compare-and-swap: with some hundred idle workgroups one of them wins per round trip of
// the atomic, ~3.6 us, and 10^5 tasks per stage were 400 ms of pops.)  The head therefore runs ahead of the tail by the number of
// idle workgroups; a workgroup leaves for good when it leaves (quit, error, timeout), its ticket is never served.
__device__ __forceinline__ uint32_t svc_ticket(const SvcQueue &q) { return atomicAdd(q.head, 1u); }
// false = the ticket's slot has not been filled (yet)
__device__ __forceinline__ bool svc_take(const SvcQueue &q, const uint32_t pos, SvcTask &t)
{
  const uint32_t slot = pos & q.mask;
  if (svc_read(q.seq + slot) != pos + 1u) return false;
  unsigned long long *s = reinterpret_cast<unsigned long long *>(q.slots + slot);
  const unsigned long long a = svc_read(s), b = svc_read(s + 1);
  t.type_job = (uint32_t) a;
  t.first = (uint32_t) (a >> 32);
  t.last = (uint32_t) b;
  t.depth = (int32_t) (uint32_t) (b >> 32);
  svc_write(q.seq + slot, pos + q.mask + 1u);  // free for the push of the next lap
  return true;
}

__device__ __forceinline__ uint32_t svc_tag(uint32_t type, uint32_t job_tag) { return type | (job_tag << 4); }
// where a segment that still has to be partitioned / heapsorted goes
__device__ __forceinline__ void svc_push_part(const SvcParams &P, uint32_t job_tag, uint32_t first, uint32_t last, int32_t depth)
{
  svc_push(P.q[(last - first) > SVC_WIDE_MIN ? 0 : 1], SvcTask{svc_tag(SVC_T_PART, job_tag), first, last, depth}, P.error);
}
__device__ __forceinline__ void svc_push_heap(const SvcParams &P, SvcJob *job, uint32_t job_tag, uint32_t first, uint32_t last)
{
  atomicMax(&job->max_heap, last - first);
  atomicAdd(&job->n_heap, last - first);
  svc_push(P.q[(last - first) > HEAP_BIG_MIN ? 0 : 1], SvcTask{svc_tag(SVC_T_HEAP, job_tag), first, last, 0}, P.error);
}
// the job is done: the caller's host thread waits for the slot's word in host memory (every store of the job's result was
// write-through and had left its wave before the retire that counted it off)
__device__ __forceinline__ void svc_done(const SvcParams &P, SvcJob *job, const uint32_t epoch)
{
  if (P.dbg) job->t_done = wall_clock64();
  svc_write(&job->done, 1u);
  __hip_atomic_store(P.host + SVC_H_DONE + (uint32_t) (job - P.jobs), epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// `dec` elements of the job have become final (the caller's stores have left its waves)
// (job_tag = slot | epoch << 8 as the task carries it: the epoch the host waits for is not read from memory)
__device__ __forceinline__ void svc_retire(const SvcParams &P, SvcJob *job, const uint32_t job_tag, uint32_t dec)
{
  if (dec == 0) return;
  if (P.q[0].release & 2u) svc_release();  // (what counts a job's elements off is read by the host, and what the job leaves by kernels the host launches afterwards)
  if (atomicSub(&job->remaining, dec) == dec) svc_done(P, job, job_tag >> 8);
}

// the job descriptor as a workgroup keeps it in LDS
struct SvcJobLds
{
  uint32_t *key, *idx, *posL, *posR;
  hent *hscratch;
  uint32_t *scratch32, *scratch32b;
  unsigned long long *rka, *rkb;
  SvcJob *job;
  uint32_t tag;  // job slot | epoch << 8 of the descriptor held (0xFFFFFFFF: none)
};

// __move_median_to_first(first, first+1, mid, last-1); one lane
__device__ __forceinline__ uint32_t svc_pick_pivot(uint32_t first, uint32_t last, uint32_t *key, uint32_t *idx)
{
  const uint32_t a = first + 1, b = first + (last - first) / 2, c = last - 1;
  const uint32_t ka = key[a], kb = key[b], kc = key[c];
  uint32_t pick;
  if (ka < kb)
  {
    if (kb < kc) pick = b;
    else if (ka < kc) pick = c;
    else pick = a;
  }
  else if (ka < kc) pick = a;
  else if (kb < kc) pick = c;
  else pick = b;
  const uint32_t kf = key[first], kp = key[pick];
  const uint32_t xf = idx[first], xp = idx[pick];
  st_through(key + first, kp);
  st_through(key + pick, kf);
  st_through(idx + first, xp);
  st_through(idx + pick, xf);
  return kp;
}

// ---- a partition node and the spine below it (the larger side stays with the workgroup, children as tasks) -------------------------------------
constexpr uint32_t TL_UNROLL = 24;  // rows of 64 keys a wave has in flight in the count and the place pass of a node
template <uint32_t NT> struct SvcPartLds
{
  uint32_t first, last, pivot;
  int32_t depth;
  uint32_t cnt[2][NT / 64];
  uint32_t cut;
  int go_on;
};
template <uint32_t NT, bool WIDE, class T = WgTeam>
__device__ __forceinline__ void svc_part(const SvcParams &P, const SvcJobLds &J, SvcPartLds<NT> &S, const SvcTask t, uint32_t *pos, const uint32_t pos_cap, const T &team = T())
{
  constexpr uint32_t NW = NT / 64;
  const uint32_t tid = team.tid(), lane = tid & 63, w = tid >> 6;
  uint32_t *key = J.key, *idx = J.idx;
  const uint32_t job_tag = t.type_job >> 4;
  uint32_t retired = 0;  // (lane 0 of wave 0 only)
  if (tid == 0)
  {
    S.first = t.first;
    S.last = t.last;
    S.go_on = 1;
    if (t.depth == 0)
    {
      // std::sort switches to heapsort here (__partial_sort(first, last, last))
      svc_push_heap(P, J.job, job_tag, t.first, t.last);  // (nothing of this task has been written)
      S.go_on = 0;
    }
    else if (t.last - t.first > pos_cap + 1u)
    {
      atomicOr(P.error, 32u);  // a node beyond the position lists of this kind of workgroup
      S.go_on = 0;
    }
    else
    {
      S.pivot = svc_pick_pivot(t.first, t.last, key, idx);
      S.depth = t.depth - 1;
      S.cut = 0xFFFFFFFFu;
    }
  }
  team.sync();
  if (!S.go_on) return;
  unsigned long long tph = 0;  // (BK_DEBUG=svc, wide nodes: ticks per phase of a level)
  uint32_t *phase = (P.dbg && WIDE) ? P.dbg + 12 * 8192 + 32 : nullptr;
  auto mark = [&](int k) {
    if (phase && tid == 0)
    {
      const unsigned long long now = wall_clock64();
      if (k >= 0) atomicAdd(phase + k, (uint32_t) (now - tph));
      tph = now;
    }
  };
  for (;;)
  {
    const uint32_t first = S.first, last = S.last, pivot = S.pivot;
    const int32_t depth = S.depth;
    mark(-1);
    if (phase && tid == 0) atomicAdd(phase + 7, 1u);
    // stoppers among (first, last): key >= pivot stops the scan from the left, key <= pivot the scan from the right; wave w owns
    // a contiguous chunk (rows of 64 consecutive positions)
    const uint32_t lo = first + 1, total = last - lo;
    const uint32_t chunk = (((total + NW - 1) / NW) + 63u) & ~63u;
    const uint32_t wbeg = lo + min(total, w * chunk), wend = lo + min(total, (w + 1) * chunk);
    uint32_t cL = 0, cR = 0;
    {
      uint32_t p = wbeg + lane;
      for (; p + (TL_UNROLL - 1) * 64 < wend; p += TL_UNROLL * 64)
      {
        uint32_t k[TL_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) k[u] = key[p + u * 64];
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u)
        {
          cL += k[u] >= pivot ? 1u : 0u;
          cR += k[u] <= pivot ? 1u : 0u;
        }
      }
      for (; p < wend; p += 64)
      {
        const uint32_t k = key[p];
        cL += k >= pivot ? 1u : 0u;
        cR += k <= pivot ? 1u : 0u;
      }
    }
    for (int d = 32; d >= 1; d >>= 1)
    {
      cL += __shfl_xor(cL, d, 64);
      cR += __shfl_xor(cR, d, 64);
    }
    if (lane == 0)
    {
      S.cnt[0][w] = cL;
      S.cnt[1][w] = cR;
    }
    team.sync();
    mark(0);
    uint32_t runL = 0, runR = 0, nL = 0, nR = 0;
    for (uint32_t i = 0; i < NW; ++i)
    {
      const uint32_t a = S.cnt[0][i], b = S.cnt[1][i];
      if (i < w)
      {
        runL += a;
        runR += b;
      }
      nL += a;
      nR += b;
    }
    // the workgroup's own position lists (never another workgroup's addresses): at most last - first - 1 entries each
    uint32_t *pL = pos, *pR = pos + pos_cap;
    {
      auto place = [&](uint32_t p, bool valid, uint32_t k) {
        const bool fL = valid && k >= pivot, fR = valid && k <= pivot;
        const unsigned long long mL = __ballot(fL), mR = __ballot(fR);
        const uint32_t bL = __builtin_amdgcn_mbcnt_hi((uint32_t) (mL >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mL, 0u));
        const uint32_t bR = __builtin_amdgcn_mbcnt_hi((uint32_t) (mR >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mR, 0u));
        if (fL) pL[runL + bL] = p;
        if (fR) pR[runR + bR] = p;
        runL += (uint32_t) __popcll(mL);
        runR += (uint32_t) __popcll(mR);
      };
      uint32_t p0 = wbeg;
      for (; p0 + TL_UNROLL * 64 <= wend; p0 += TL_UNROLL * 64)
      {
        uint32_t k[TL_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) k[u] = key[p0 + u * 64 + lane];
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) place(p0 + u * 64 + lane, true, k[u]);
      }
      for (; p0 < wend; p0 += 64)
      {
        const uint32_t p = p0 + lane;
        const bool valid = p < wend;
        place(p, valid, valid ? key[p] : 0u);
      }
    }
    team.sync();
    mark(1);
    // pair j = (l_j, r_j): swapped while l_j < r_j; the first pair that is not gives the cut
    const uint32_t mm = nL < nR ? nL : nR;
    constexpr uint32_t SW = 4;
    for (uint32_t j0 = tid; j0 <= mm; j0 += SW * NT)
    {
      uint32_t lj[SW], rj[SW];
      bool sw[SW];
#pragma unroll
      for (uint32_t u = 0; u < SW; ++u)
      {
        const uint32_t j = j0 + u * NT;
        lj[u] = j < nL ? pL[j] : 0xFFFFFFFFu;
        rj[u] = j < nR ? pR[nR - 1 - j] : first;
      }
      uint32_t k1[SW], k2[SW], x1[SW], x2[SW];
#pragma unroll
      for (uint32_t u = 0; u < SW; ++u)
      {
        const uint32_t j = j0 + u * NT;
        sw[u] = j <= mm && (j < nL) && (j < nR) && (lj[u] < rj[u]);
        if (sw[u])
        {
          k1[u] = key[lj[u]];
          k2[u] = key[rj[u]];
          x1[u] = idx[lj[u]];
          x2[u] = idx[rj[u]];
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < SW; ++u)
        if (sw[u])
        {
          st_through(key + lj[u], k2[u]);
          st_through(key + rj[u], k1[u]);
          st_through(idx + lj[u], x2[u]);
          st_through(idx + rj[u], x1[u]);
        }
#pragma unroll
      for (uint32_t u = 0; u < SW; ++u)
      {
        const uint32_t j = j0 + u * NT;
        if (j > mm || sw[u]) continue;
        const uint32_t ljj = lj[u];
        bool prev_cont = false;
        uint32_t rprev = 0;
        if (j > 0)
        {
          const uint32_t lp = pL[j - 1];
          rprev = pR[nR - j];
          prev_cont = lp < rprev;
        }
        if (j == 0)
          S.cut = ljj;
        else if (prev_cont)
          S.cut = ljj < rprev ? ljj : rprev;
      }
      // l_j rises and r_j falls with j: behind the first pair that is not swapped nothing is (a degenerate node - a few per cent
      // peeled off - has few swapped pairs and tens of thousands of stoppers: this thread's later pairs need not be looked at)
      if (!sw[SW - 1]) break;
    }
    svc_drain_barrier(team);  // (every wave's swaps have left the wave)
    mark(2);
    const uint32_t cut = S.cut;
    team.sync();  // (everybody has the cut: lane 0 resets it below)
    if (cut == 0xFFFFFFFFu || cut <= first || cut > last)
    {
      if (tid == 0) SVC_FAIL(P, 8u, first, last, cut);  // (a partition always yields a cut inside the segment: reported, never silent)
      return;
    }
    if (tid == 0)
    {
      // the two sides [first, cut) and [cut, last): at most 16 elements = final (the insertion sort's business), at most FIN_MAX =
      // the finisher's, else another node.  The workgroup carries on with the larger node (a wide workgroup only while it is a wide
      // node), the rest is pushed - behind ONE release of everything this workgroup has swapped so far.
      const uint32_t a0 = first, a1 = cut, b0 = cut, b1 = last;
      const uint32_t sa = a1 - a0, sb = b1 - b0;
      const bool big_is_a = sa >= sb;
      const uint32_t g0 = big_is_a ? a0 : b0, g1 = big_is_a ? a1 : b1, h0 = big_is_a ? b0 : a0, h1 = big_is_a ? b1 : a1;  // g = larger, h = smaller side
      const uint32_t sg = g1 - g0, sh = h1 - h0;
      const bool carry = sg > FIN_MAX && (!WIDE || sg > SVC_WIDE_MIN);
      const bool push_g = sg > 16 && !carry, push_h = sh > 16;
      retired += (sg <= 16 ? sg : 0u) + (sh <= 16 ? sh : 0u);
      // a carried-on node whose depth budget is used up becomes a heap task as well
      const bool carry_heap = carry && depth == 0;
      if (push_g || push_h || carry_heap)
      {
        team.count_pushes((push_h ? 1u : 0u) + (push_g ? 1u : 0u));
        if (P.q[0].release & 1u) svc_release();  // (one release of everything this workgroup has swapped so far, in front of the pushes)
        if (push_h)
        {
          if (sh <= FIN_MAX)
            svc_push(P.q[1], SvcTask{svc_tag(SVC_T_FIN, job_tag), h0, h1, depth}, P.error);
          else
            svc_push_part(P, job_tag, h0, h1, depth);
        }
        if (push_g)
        {
          if (sg <= FIN_MAX)
            svc_push(P.q[1], SvcTask{svc_tag(SVC_T_FIN, job_tag), g0, g1, depth}, P.error);
          else
            svc_push_part(P, job_tag, g0, g1, depth);
        }
        if (carry_heap) svc_push_heap(P, J.job, job_tag, g0, g1);
      }
      if (carry && !carry_heap)
      {
        S.first = g0;
        S.last = g1;
        S.pivot = svc_pick_pivot(g0, g1, key, idx);
        S.depth = depth - 1;
        S.cut = 0xFFFFFFFFu;
        S.go_on = 1;
      }
      else
        S.go_on = 0;
    }
    svc_drain_barrier(team);
    mark(3);
    if (!S.go_on) break;
  }
  if (tid == 0 && retired) svc_retire(P, J.job, job_tag, retired);
}

// ---- the finisher of the service: a segment of at most FIN_MAX elements in LDS, its sub-segments dealt to the waves --------------
// An earlier form played the levels of ALL sub-segments in lock step: six workgroup barriers and eight passes over the whole
// segment per level, ~20 levels whatever is left alive, and every sub-segment that ran out of depth left as a heap segment of
// its own (117 us per task and 41 000 heap tasks of mostly 16-63 elements per stage, i.e. three quarters of what the narrow
// workgroups did).  Here a sub-segment belongs to ONE wave: the wave partitions it (stoppers listed by ballots, pairs
// swapped while l_j < r_j, cut = min(l_J, r_{J-1}): the partition of svc_part bit for bit), queues the smaller side
// for whichever wave is free and carries on with the larger one; a sub-segment that has used up its depth is heapsorted by the
// wave that holds it, in that wave's own buffer, when it has at most F2_HB elements (95 % of them), else it leaves as a heap task.
// Sub-segments are disjoint, so the order in which the waves take them does not matter.
constexpr uint32_t F2_HB = 256;    // a wave's heap buffer (entries)
constexpr uint32_t F2_QCAP = 256;  // queued sub-segments over the life of a task (each holds more than 16 elements: at most FIN_MAX / 17 pushes) + the waves' last tickets
constexpr uint32_t F2_EXT = 16;    // sub-segments of more than F2_HB elements that ran out of depth (disjoint: at most FIN_MAX / F2_HB)
struct Fin2Lds
{
  hent ent[FIN_MAX];
  uint16_t posL[FIN_MAX + 2], posR[FIN_MAX + 2];
  unsigned long long q[F2_QCAP];  // first | last << 16 | (depth + 1) << 32; 0 = not written yet
  hent hbuf[4][F2_HB + 4];
  uint2 ext[F2_EXT];
  uint32_t q_head, q_tail, pending, n_ext, ext_elems, bad;
};
static_assert(sizeof(Fin2Lds) <= SVC_NARROW_LDS, "narrow workgroup LDS");
static_assert(FIN_MAX / F2_HB + 1 <= F2_EXT && FIN_MAX / 17 + 8 <= F2_QCAP, "fin2 lists");

// LDS traffic of one wave is served in order; this keeps the compiler from moving accesses across
__device__ __forceinline__ void f2_wsync()
{
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void f2_push(Fin2Lds &L, uint32_t first, uint32_t last, int32_t depth)  // one lane
{
  const uint32_t slot = atomicAdd(&L.q_tail, 1u);
  if (slot >= F2_QCAP)
  {
    L.bad = 1u;
    return;
  }
  __hip_atomic_store(&L.q[slot], (unsigned long long) first | ((unsigned long long) last << 16) | ((unsigned long long) (uint32_t) (depth + 1) << 32), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the wave's sub-segment [first, last) (more than 16 elements, depth > 0): one partition step; returns the cut (all lanes)
__device__ __forceinline__ uint32_t f2_partition(Fin2Lds &L, const uint32_t first, const uint32_t last, const uint32_t lane)
{
  hent *ent = L.ent;
  // __move_median_to_first(first, first + 1, mid, last - 1)
  const uint32_t a = first + 1, b = first + (last - first) / 2, c = last - 1;
  const hent ea = ent[a], eb = ent[b], ec = ent[c];
  const uint32_t ka = hkey(ea), kb = hkey(eb), kc = hkey(ec);
  uint32_t pick;
  if (ka < kb)
  {
    if (kb < kc) pick = b;
    else if (ka < kc) pick = c;
    else pick = a;
  }
  else if (ka < kc) pick = a;
  else if (kb < kc) pick = c;
  else pick = b;
  const hent ep = pick == a ? ea : (pick == b ? eb : ec), ef = ent[first];
  const uint32_t pivot = hkey(ep);
  f2_wsync();
  if (lane == 0)
  {
    ent[first] = ep;
    ent[pick] = ef;
  }
  f2_wsync();
  // stoppers of (first, last) in ascending order of position: key >= pivot stops the scan from the left, key <= pivot the one from the right
  uint16_t *pL = L.posL + first + 1, *pR = L.posR + first + 1;
  uint32_t nL = 0, nR = 0;
  for (uint32_t p0 = first + 1; p0 < last; p0 += 64)
  {
    const uint32_t p = p0 + lane;
    const bool valid = p < last;
    const uint32_t k = valid ? hkey(ent[p]) : 0u;
    const bool fL = valid && k >= pivot, fR = valid && k <= pivot;
    const unsigned long long mL = __ballot(fL), mR = __ballot(fR);
    if (fL) pL[nL + __builtin_amdgcn_mbcnt_hi((uint32_t) (mL >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mL, 0u))] = (uint16_t) p;
    if (fR) pR[nR + __builtin_amdgcn_mbcnt_hi((uint32_t) (mR >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mR, 0u))] = (uint16_t) p;
    nL += (uint32_t) __popcll(mL);
    nR += (uint32_t) __popcll(mR);
  }
  f2_wsync();
  // pair j = (l_j, r_j) with r_j = pR[nR - 1 - j]: swapped while l_j < r_j; the first pair that is not gives the cut
  const uint32_t mm = nL < nR ? nL : nR;
  uint32_t cut = 0xFFFFFFFFu;
  for (uint32_t j0 = 0; j0 <= mm; j0 += 64)
  {
    const uint32_t j = j0 + lane;
    const bool act = j <= mm;
    const uint32_t lj = act && j < nL ? pL[j] : 0xFFFFFFFFu;
    const uint32_t rj = act && j < nR ? pR[nR - 1 - j] : first;
    const bool sw = act && j < nL && j < nR && lj < rj;
    uint32_t mycut = 0xFFFFFFFFu;
    if (sw)
    {
      const hent e1 = ent[lj], e2 = ent[rj];
      ent[lj] = e2;
      ent[rj] = e1;
    }
    else if (act)
    {
      if (j == 0)
        mycut = lj;
      else
      {
        const uint32_t lp = pL[j - 1], rprev = pR[nR - j];
        if (lp < rprev) mycut = lj < rprev ? lj : rprev;
      }
    }
    const unsigned long long mc = __ballot(mycut != 0xFFFFFFFFu);
    if (mc != 0ull)
    {
      cut = __shfl(mycut, (int) __builtin_ctzll(mc), 64);
      break;
    }
  }
  f2_wsync();
  return cut;
}
// every thread of the 256-thread team calls this; returns (thread 0) the elements handed on as heap tasks via L.ext / L.n_ext
template <class T = WgTeam> __device__ __forceinline__ void fin2_body(Fin2Lds &L, const uint32_t g0, const uint32_t g1, const int32_t depth0, uint32_t *key, uint32_t *idx, const T &team = T())
{
  const uint32_t tid = team.tid(), lane = tid & 63, w = tid >> 6, m = g1 - g0;
  for (uint32_t e = tid; e < m; e += 256) L.ent[e] = ((hent) key[g0 + e] << 32) | idx[g0 + e];
  for (uint32_t e = tid; e < F2_QCAP; e += 256) L.q[e] = 0ull;
  if (tid == 0)
  {
    L.q[0] = (unsigned long long) 0u | ((unsigned long long) m << 16) | ((unsigned long long) (uint32_t) (depth0 + 1) << 32);
    L.q_tail = 1;
    L.q_head = 0;
    L.pending = m;
    L.n_ext = 0;
    L.ext_elems = 0;
    L.bad = 0;
  }
  team.sync();
  for (;;)
  {
    // a ticket, then the entry it stands for - or the end of the task
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(&L.q_head, 1u);
    t = __shfl(t, 0, 64);
    unsigned long long e = 0ull;
    bool done = false;
    for (;;)
    {
      if (t < F2_QCAP) e = __hip_atomic_load(&L.q[t], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (e != 0ull) break;
      if (__hip_atomic_load(&L.pending, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u || __hip_atomic_load(&L.bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u)
      {
        done = true;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    if (done) break;
    uint32_t first = (uint32_t) e & 0xFFFFu, last = (uint32_t) (e >> 16) & 0xFFFFu;
    int32_t depth = (int32_t) (uint32_t) (e >> 32) - 1;
    f2_wsync();
    for (;;)
    {
      const uint32_t sz = last - first;
      uint32_t retired = 0;
      bool go_on = false;
      if (depth == 0)
      {
        // std::sort switches to heapsort here (__partial_sort(first, last, last))
        if (sz <= F2_HB)
        {
          hent *hb = L.hbuf[w];
          for (uint32_t i = lane; i < sz; i += 64) hb[i] = L.ent[first + i];
          f2_wsync();
          LdsMem mem{hb};
          make_heap_wave(mem, sz);
          sort_heap_asm<false>(hb, sz, 1);
          f2_wsync();
          for (uint32_t i = lane; i < sz; i += 64) L.ent[first + i] = hb[i];
          f2_wsync();
        }
        else if (lane == 0)
        {
          const uint32_t k = atomicAdd(&L.n_ext, 1u);
          if (k < F2_EXT) L.ext[k] = make_uint2(g0 + first, g0 + last); else L.bad = 1u;
          atomicAdd(&L.ext_elems, sz);
        }
        retired = sz;
      }
      else
      {
        const uint32_t cut = f2_partition(L, first, last, lane);
        if (cut <= first || cut > last)
        {
          if (lane == 0) L.bad = 2u;  // (a partition always yields a cut inside the segment: reported, never silent)
          retired = sz;
        }
        else
        {
          const uint32_t sa = cut - first, sb = last - cut;
          const bool big_a = sa >= sb;
          const uint32_t h0 = big_a ? first : cut, h1 = big_a ? cut : last, l0 = big_a ? cut : first, l1 = big_a ? last : cut;  // h = larger, l = smaller side
          const uint32_t sh = h1 - h0, sl = l1 - l0;
          --depth;
          if (sl > 16)
          {
            if (lane == 0) f2_push(L, l0, l1, depth);
          }
          else
            retired += sl;
          if (sh > 16)
          {
            first = h0;
            last = h1;
            go_on = true;
          }
          else
            retired += sh;
        }
      }
      if (retired && lane == 0) atomicSub(&L.pending, retired);
      if (!go_on) break;
    }
  }
  team.sync();
  for (uint32_t e = tid; e < m; e += 256)
  {
    const hent v = L.ent[e];
    st_through(key + g0 + e, hkey(v));
    st_through(idx + g0 + e, (uint32_t) v);
  }
}

// ---- the two kinds of resident workgroups -------------------------------------------------------------------------------------------
static_assert((HEAP_BIG_MIN + HEAP_PAD) * 8 <= SVC_NARROW_LDS, "narrow workgroup LDS");

template <bool WIDE> __global__ __launch_bounds__(WIDE ? 1024 : 256) void k_sort_service(const SvcParams P)
{
  constexpr uint32_t NT = WIDE ? 1024u : 256u;
  extern __shared__ __attribute__((aligned(16))) unsigned char pool[];
  __shared__ SvcTask s_task;
  __shared__ int s_state;
  __shared__ SvcJobLds s_job;
  __shared__ SvcPartLds<NT> s_part;
  const uint32_t tid = threadIdx.x;
  const SvcQueue q = P.q[WIDE ? 0 : 1];
  if (tid == 0)
  {
    s_job.tag = 0xFFFFFFFFu;
    atomicAdd(P.stats + (WIDE ? 2 : 3), 1u);
    if (!WIDE && blockIdx.x == 0) __hip_atomic_store(P.host + SVC_H_NARROW, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (WIDE) __hip_atomic_store(P.host + SVC_H_STARTED + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // (host memory: the narrow kernel is launched when every wide workgroup has its CU)
  }
  unsigned long long t_last = wall_clock64();
  const unsigned long long t_start = t_last;
  // (BK_DEBUG=svc) lane 0's account of the workgroup's time in 10 ns ticks: [0] waiting for a task, [1..3] inside tasks by type, [4..6] tasks by type, [7] longest task
  uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_poll = t_last, t_task = t_last;
  for (;;)
  {
    if (tid == 0)
    {
      int st = 0;
      t_poll = wall_clock64();
      SvcTask t;
      uint32_t nap = 1, polls = 0;
      const uint32_t ticket = svc_ticket(q);
      uint32_t *dbg = P.dbg ? P.dbg + 4 * (blockIdx.x + (WIDE ? 0u : 4096u)) : nullptr;
      for (;;)
      {
        if (dbg)
        {
          SVC_ST(dbg, 1u);
          SVC_ST(dbg + 1, polls);
          SVC_ST(dbg + 2, (uint32_t) (wall_clock64() - t_start));
        }
        if (svc_take(q, ticket, t))
        {
          st = 1;
          break;
        }
        if (const uint32_t err = ((polls & 7u) == 0 ? svc_read(P.error) : 0u))
        {
          for (uint32_t k = 0; k < 4; ++k) __hip_atomic_store(P.host + SVC_H_ERROR + 1 + k, SVC_LD(P.error + 8 + k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(P.host + SVC_H_ERROR, err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // (the waiting host threads give up)
          st = 2;
          if (dbg) SVC_ST(dbg + 3, 6u);
          break;
        }
        if ((++polls & 15u) == 0)
        {
          const uint32_t qv = svc_read(P.quit_d);
          if (qv == P.quit_word)
          {
            st = 2;
            if (dbg) SVC_ST(dbg + 3, 7u);
            break;
          }
          if (qv != 0u) atomicAdd(P.stats + 6, 1u);  // (neither "carry on" nor this run's "leave": counted, ignored)
        }
        if ((polls & 15u) == 0 && wall_clock64() - t_last > P.timeout_ticks)
        {
          atomicAdd(P.stats + (WIDE ? 4 : 5), 1u);  // left without having been told to
          st = 2;
          if (dbg) SVC_ST(dbg + 3, 8u);
          break;
        }
        // (its own slot's word: nobody else polls it, so a short nap costs nothing but this wave's issue slots)
        for (uint32_t k = 0; k < nap; ++k) __builtin_amdgcn_s_sleep(32);
        if (nap < 4) ++nap;
      }
      if (st == 1)
      {
        svc_acquire();
        const uint32_t tag = t.type_job >> 4;
        if (s_job.tag != tag)
        {
          SvcJob *job = P.jobs + (tag & 0xFFu);
          unsigned long long *src = reinterpret_cast<unsigned long long *>(job);
          unsigned long long v[9];
#pragma unroll
          for (int k = 0; k < 9; ++k) v[k] = svc_read(src + k);
          s_job.key = (uint32_t *) v[0];
          s_job.idx = (uint32_t *) v[1];
          s_job.posL = (uint32_t *) v[2];
          s_job.posR = (uint32_t *) v[3];
          s_job.hscratch = (hent *) v[4];
          s_job.scratch32 = (uint32_t *) v[5];
          s_job.scratch32b = (uint32_t *) v[6];
          s_job.rka = (unsigned long long *) v[7];
          s_job.rkb = (unsigned long long *) v[8];
          s_job.job = job;
          s_job.tag = tag;
        }
        s_task = t;
      }
      s_state = st;
      if (dbg) SVC_ST(dbg, st == 1 ? 5u : 9u);
      t_task = wall_clock64();
      acc[0] += (uint32_t) (t_task - t_poll);
      if (dbg && st != 1)
      {
        uint32_t *a = P.dbg + 4 * 8192 + 8 * (blockIdx.x + (WIDE ? 0u : 4096u));
        for (int k = 0; k < 8; ++k) SVC_ST(a + k, acc[k]);
      }
    }
    __syncthreads();
    if (s_state != 1) return;
    const SvcTask t = s_task;
    const uint32_t type = t.type_job & 15u;
    if (P.dbg && tid == 0 && !WIDE && type != SVC_T_PART)  // (BK_DEBUG=svc) sizes of the finisher's and the narrow heaps' tasks by power of two
      atomicAdd(P.dbg + 12 * 8192 + (type == SVC_T_HEAP ? 16 : 0) + (31 - __clz((int) (t.last - t.first))), 1u);
    if (type == SVC_T_PART)
      svc_part<NT, WIDE>(P, s_job, s_part, t, P.pos[WIDE ? 0 : 1] + 2ull * P.pos_cap[WIDE ? 0 : 1] * blockIdx.x, P.pos_cap[WIDE ? 0 : 1]);
    else if (type == SVC_T_HEAP)
    {
      if (WIDE)
        heap_big_body(t.first, t.last, s_job.key, s_job.idx, s_job.hscratch, s_job.scratch32, s_job.scratch32b, s_job.rka, s_job.rkb, reinterpret_cast<hent *>(pool), P.cap32, NT);
      else
        heap_small_body(t.first, t.last, s_job.key, s_job.idx, reinterpret_cast<hent *>(pool), NT);
      svc_drain_barrier();
      if (tid == 0) svc_retire(P, s_job.job, t.type_job >> 4, t.last - t.first);
    }
    else if (type == SVC_T_FIN && !WIDE)
    {
      Fin2Lds &L = *reinterpret_cast<Fin2Lds *>(pool);
      fin2_body(L, t.first, t.last, t.depth, s_job.key, s_job.idx);
      svc_drain_barrier();
      if (tid == 0)
      {
        if (L.bad) SVC_FAIL(P, 64u, t.first, t.last, L.bad | (L.q_tail << 8) | (L.n_ext << 20));
        const uint32_t nh = L.n_ext < F2_EXT ? L.n_ext : F2_EXT;
        if (nh && (P.q[0].release & 1u)) svc_release();
        for (uint32_t k = 0; k < nh; ++k) svc_push_heap(P, s_job.job, t.type_job >> 4, L.ext[k].x, L.ext[k].y);
        svc_retire(P, s_job.job, t.type_job >> 4, (t.last - t.first) - L.ext_elems);
      }
    }
    else if (tid == 0)
      atomicOr(P.error, 16u);  // a task in the wrong queue
    if (tid == 0)
    {
      t_last = wall_clock64();
      atomicAdd(P.stats + (WIDE ? 0 : 1), 1u);
      if (P.dbg)
      {
        if (type == SVC_T_HEAP)
          s_job.job->last_heap = ((unsigned long long) (t_last - t_task) << 32) | (t.last - t.first);
        else
          atomicMax(&s_job.job->t_parts, t_last);
      }
      const uint32_t dt = (uint32_t) (t_last - t_task), ty = type <= 3u ? type : 3u;
      acc[ty] += dt;
      acc[3 + ty] += 1u;
      acc[7] = dt > acc[7] ? dt : acc[7];
    }
    __syncthreads();
  }
}

// queue words: seq[i] = i, heads and tails 0
__global__ __launch_bounds__(256) void k_svc_reset(const SvcParams P)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  for (int k = 0; k < 2; ++k)
    if (i <= P.q[k].mask) P.q[k].seq[i] = i;
  if (i == 0)
  {
    for (int k = 0; k < 2; ++k) *P.q[k].head = *P.q[k].tail = 0u;
    *P.error = 0u;
    *P.quit_d = 0u;
    for (int k = 0; k < 8; ++k) P.stats[k] = 0u;
  }
  if (i < SVC_MAX_JOBS)
  {
    P.jobs[i].done = 0u;
    P.jobs[i].remaining = 0u;
  }
}

__global__ void k_svc_quit(uint32_t *quit_d, uint32_t word) { atomicExch(quit_d, word); }

// One block: the descriptor, then a task per group of more than 16 elements.
__global__ __launch_bounds__(256) void k_svc_submit(const SvcParams P, const SvcJob desc, uint32_t slot, const uint64_t *__restrict__ goff, uint32_t ng)
{
  __shared__ uint32_t s_total;
  SvcJob *job = P.jobs + slot;
  const uint32_t job_tag = slot | (desc.epoch << 8);
  if (threadIdx.x == 0)
  {
    s_total = 0;
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(&desc);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(job);
    for (uint32_t k = 0; k < sizeof(SvcJob) / 8; ++k)
      if (k != 9) svc_write(dst + k, src[k]);  // (word 9 = remaining / done, below)
    svc_write(&job->done, 0u);
    svc_write(&job->remaining, SVC_BIAS);
    job->t_submit = wall_clock64();
    job->t_parts = 0ull;
    job->last_heap = 0ull;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    svc_release();  // (the keys of the launch before this one are in memory: kernel boundary; this orders the descriptor)
  }
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t g = threadIdx.x; g < ng; g += blockDim.x)
  {
    const uint32_t first = (uint32_t) goff[g], last = (uint32_t) goff[g + 1], sz = last - first;
    if (sz <= 16) continue;
    mine += sz;
    const int32_t depth = 2 * (31 - __clz((int) sz));
    if (sz <= FIN_MAX)
      svc_push(P.q[1], SvcTask{svc_tag(SVC_T_FIN, job_tag), first, last, depth}, P.error);
    else
      svc_push_part(P, job_tag, first, last, depth);
  }
  atomicAdd(&s_total, mine);
  __syncthreads();
  if (threadIdx.x == 0)
  {
    // remaining += total - BIAS; whoever brings it to zero reports the job done (this lane when nothing was pushed or everything is final already)
    const uint32_t add = s_total - SVC_BIAS;
    if (atomicAdd(&job->remaining, add) + add == 0u) svc_done(P, job, desc.epoch);
  }
}

// ---- one sort as ONE ordinary dispatch on the caller's stream (the launch path: no service running) ---------------------------------
// The task bodies above on queues and a job of the caller's own (SortEmuBufs, never shared), seeded by k_sort_job_submit in front of
// the dispatch.  Every workgroup is 1024 threads with all of a CU's LDS: workgroups [0, n_wide) serve the wide queue as the service's
// wide kernel does, every other one is SJ_TEAMS teams of 256 threads that serve the narrow queue on their own (LdsTeam: their own
// barrier, thread index, slice of the LDS and of the position lists).  A task still never waits for another task.  A workgroup
// (team) leaves when the job is done, when a task failed, or when nothing can arrive any more: no partition or finisher task is
// queued or running (`live`, counted up before every push of one and down behind the last push of the task that pushed it; heaps
// push nothing) and its own ticket's slot is empty - so the idle CUs go back to the caller's other kernels while the long heaps run,
// and a workgroup that starts late finds the job done and leaves.  No progress for SJ_TIMEOUT_TICKS: error 4, never a hang.
constexpr uint32_t SJ_TEAMS = 4;
constexpr size_t SJ_TEAM_LDS = ((sizeof(Fin2Lds) > (HEAP_BIG_MIN + HEAP_PAD) * 8 ? sizeof(Fin2Lds) : (HEAP_BIG_MIN + HEAP_PAD) * 8) + 15) & ~(size_t) 15;
static_assert(SJ_TEAMS * SJ_TEAM_LDS + 4096 <= 160 * 1024, "four narrow teams in a CU's LDS");
constexpr uint32_t SJ_MAX_WIDE = 32, SJ_MAX_NARROW = 32;        // workgroups per dispatch of each kind (three lanes: 192 of 256 CUs)
constexpr unsigned long long SJ_TIMEOUT_TICKS = 100000000ull;  // 1 s of wall_clock64 without a task while tasks can still arrive
// ctl words of a caller's queues (SortEmuBufs::tj_ctl)
constexpr uint32_t SJ_C_ERROR = 128, SJ_C_STATS = 160, SJ_C_QUIT = 192, SJ_C_LIVE = 224, SJ_C_HOST = 256, SJ_C_WORDS = SJ_C_HOST + SVC_H_WORDS;

struct SjParams
{
  SvcParams P;          // the caller's queues; P.jobs = its job (slot 0); P.host = device words that stand in for the service's host words
  uint32_t n_wide;
  uint32_t *live;       // partition and finisher tasks pushed and not finished
  uint32_t *heavy;      // (or null) per group: the longest heap segment of more than heavy_min elements a partition node left
  const uint32_t *gof;  // group of every position
  uint32_t heavy_min;
  unsigned long long *trace;  // (BK_DEBUG=svc, or null) [0] first workgroup start, [1] longest heap: elements << 40 | start, [2] the
                              // same with its ticks, [3] end of the last partition / finisher task, [4] end of the last task
};

template <bool WIDE, class T>
__device__ __forceinline__ void sj_serve(const SjParams &S, const SvcJobLds &J, SvcTask &s_task, int &s_state, SvcPartLds<WIDE ? 1024u : 256u> &s_part, unsigned char *pool, uint32_t *pos, const T &team)
{
  constexpr uint32_t NT = WIDE ? 1024u : 256u;
  const SvcParams &P = S.P;
  const SvcQueue &q = P.q[WIDE ? 0 : 1];
  const uint32_t tid = team.tid();
  SvcJob *job = J.job;
  unsigned long long t_last = wall_clock64(), t_task = t_last;
  if (S.trace && tid == 0) atomicMin(S.trace, t_last);
  for (;;)
  {
    if (tid == 0)
    {
      int st = 0;
      SvcTask t;
      const uint32_t ticket = svc_ticket(q);
      for (uint32_t polls = 0, nap = 1;; ++polls)
      {
        if (svc_take(q, ticket, t))
        {
          st = 1;
          break;
        }
        if ((polls & 7u) == 0)
        {
          if (svc_read(P.error) != 0u || svc_read(&job->remaining) == 0u)
          {
            st = 2;
            break;
          }
          if (svc_read(S.live) == 0u)
          {
            // every push there will be has landed (the count goes down behind the pusher's waited stores): one more look at the slot
            st = svc_take(q, ticket, t) ? 1 : 2;
            break;
          }
          if (wall_clock64() - t_last > P.timeout_ticks)
          {
            SVC_FAIL(P, 4u, WIDE ? 1u : 0u, svc_read(&job->remaining), svc_read(S.live));
            st = 2;
            break;
          }
        }
        for (uint32_t k = 0; k < nap; ++k) __builtin_amdgcn_s_sleep(32);
        if (nap < 4) ++nap;
      }
      if (st == 1) svc_acquire();  // (also what a team of this CU wrote before it pushed: never optimised away)
      s_task = t;
      s_state = st;
      t_task = wall_clock64();
    }
    team.sync();
    if (s_state != 1) return;
    const SvcTask t = s_task;
    const uint32_t type = t.type_job & 15u, job_tag = t.type_job >> 4;
    if (type == SVC_T_PART)
    {
      svc_part<NT, WIDE, T>(P, J, s_part, t, pos, P.pos_cap[WIDE ? 0 : 1], team);
      if (tid == 0)
      {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the pushes have landed)
        atomicSub(S.live, 1u);
      }
    }
    else if (type == SVC_T_HEAP)
    {
      const uint32_t m = t.last - t.first;
      if (WIDE)
        heap_big_body(t.first, t.last, J.key, J.idx, J.hscratch, J.scratch32, J.scratch32b, J.rka, J.rkb, reinterpret_cast<hent *>(pool), P.cap32, NT);
      else
        heap_small_body<T>(t.first, t.last, J.key, J.idx, reinterpret_cast<hent *>(pool), NT, team);
      svc_drain_barrier(team);
      if (tid == 0)
      {
        // (what the lanes of lanes.hip balance on: heaps above FIN_MAX elements are the partition nodes', never the finisher's)
        if (S.heavy && m > S.heavy_min) atomicMax(S.heavy + S.gof[t.first], m);
        if (S.trace)
        {
          const unsigned long long now = wall_clock64();
          atomicMax(S.trace + 1, ((unsigned long long) m << 40) | (t_task & 0xFFFFFFFFFFull));
          atomicMax(S.trace + 2, ((unsigned long long) m << 40) | ((now - t_task) & 0xFFFFFFFFFFull));
        }
        svc_retire(P, job, job_tag, m);
      }
    }
    else if (type == SVC_T_FIN && !WIDE)
    {
      Fin2Lds &L = *reinterpret_cast<Fin2Lds *>(pool);
      fin2_body<T>(L, t.first, t.last, t.depth, J.key, J.idx, team);
      svc_drain_barrier(team);
      if (tid == 0)
      {
        if (L.bad) SVC_FAIL(P, 64u, t.first, t.last, L.bad | (L.q_tail << 8) | (L.n_ext << 20));
        const uint32_t nh = L.n_ext < F2_EXT ? L.n_ext : F2_EXT;
        if (nh && (P.q[0].release & 1u)) svc_release();
        for (uint32_t k = 0; k < nh; ++k) svc_push_heap(P, job, job_tag, L.ext[k].x, L.ext[k].y);
        svc_retire(P, job, job_tag, (t.last - t.first) - L.ext_elems);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        atomicSub(S.live, 1u);
      }
    }
    else if (tid == 0)
      SVC_FAIL(P, 16u, type, t.first, t.last);  // a task in the wrong queue
    if (tid == 0)
    {
      t_last = wall_clock64();
      if (S.trace)
      {
        if (type != SVC_T_HEAP) atomicMax(S.trace + 3, t_last);
        atomicMax(S.trace + 4, t_last);
      }
    }
    team.sync();
  }
}

__global__ __launch_bounds__(1024) void k_sort_job(const SjParams S, const SvcJobLds J)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char pool[];
  __shared__ SvcTask s_task[SJ_TEAMS];
  __shared__ int s_state[SJ_TEAMS];
  __shared__ uint32_t s_bar[SJ_TEAMS][2];
  __shared__ union
  {
    SvcPartLds<1024> wide;
    SvcPartLds<256> narrow[SJ_TEAMS];
  } s_part;
  if (blockIdx.x < S.n_wide)
  {
    sj_serve<true>(S, J, s_task[0], s_state[0], s_part.wide, pool, S.P.pos[0] + 2ull * S.P.pos_cap[0] * blockIdx.x, WgLive{{}, S.live});
    return;
  }
  const uint32_t team = threadIdx.x >> 8;
  if ((threadIdx.x & 255u) == 0)
  {
    s_bar[team][0] = 0u;
    s_bar[team][1] = 0u;
  }
  __syncthreads();  // (the only barrier of the whole workgroup: from here on the teams meet on their own)
  sj_serve<false>(S, J, s_task[team], s_state[team], s_part.narrow[team], pool + team * SJ_TEAM_LDS,
                  S.P.pos[1] + 2ull * S.P.pos_cap[1] * ((blockIdx.x - S.n_wide) * SJ_TEAMS + team), LdsTeam{s_bar[team], team * 256u, S.live});
}

// One block, in front of k_sort_job on the same stream: the queues start where the last sort left them (head = tail: tickets of
// workgroups that left unserved are given up), the descriptor, then a task per group of more than 16 elements (as k_svc_submit).
__global__ __launch_bounds__(256) void k_sort_job_submit(const SjParams S, const SvcJob desc, const uint64_t *__restrict__ goff, uint32_t ng)
{
  __shared__ uint32_t s_total, s_tasks;
  const SvcParams &P = S.P;
  SvcJob *job = P.jobs;
  const uint32_t job_tag = desc.epoch << 8;
  if (threadIdx.x == 0)
  {
    s_total = 0;
    s_tasks = 0;
    for (int k = 0; k < 2; ++k) svc_write(P.q[k].head, svc_read(P.q[k].tail));
    for (int k = 0; k < 12; ++k) svc_write(P.error + k, 0u);
    svc_write(S.live, 0u);
    if (S.trace)
    {
      svc_write(S.trace, ~0ull);
      for (int k = 1; k < 5; ++k) svc_write(S.trace + k, 0ull);
    }
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(&desc);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(job);
    for (uint32_t k = 0; k < sizeof(SvcJob) / 8; ++k)
      if (k != 9) svc_write(dst + k, src[k]);  // (word 9 = remaining / done, below)
    svc_write(&job->done, 0u);
    svc_write(&job->remaining, SVC_BIAS);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    svc_release();
  }
  __syncthreads();
  uint32_t mine = 0, tasks = 0;
  for (uint32_t g = threadIdx.x; g < ng; g += blockDim.x)
  {
    const uint32_t first = (uint32_t) goff[g], last = (uint32_t) goff[g + 1], sz = last - first;
    if (sz <= 16) continue;
    mine += sz;
    ++tasks;
    const int32_t depth = 2 * (31 - __clz((int) sz));
    if (sz <= FIN_MAX)
      svc_push(P.q[1], SvcTask{svc_tag(SVC_T_FIN, job_tag), first, last, depth}, P.error);
    else
      svc_push_part(P, job_tag, first, last, depth);
  }
  atomicAdd(&s_total, mine);
  atomicAdd(&s_tasks, tasks);
  __syncthreads();
  if (threadIdx.x == 0)
  {
    svc_write(S.live, s_tasks);
    const uint32_t add = s_total - SVC_BIAS;
    if (atomicAdd(&job->remaining, add) + add == 0u) svc_done(P, job, desc.epoch);
  }
}
