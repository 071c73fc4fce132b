// Exact, data-parallel emulation of libstdc++'s std::sort (introsort) on every group at once.
//
// The reference sorts its pair vectors with *unstable* std::sort (BreakID.cc:1091,1127,1274,1278,1282)
// and then reads neighbours of the sorted vector (mask_pairs_chr_pos :1847-1858, fast clustering
// :1064,:1100), so the order std::sort leaves equal keys in is observable.  std::sort is
// deterministic given the comparison outcomes:
//   __introsort_loop: while (size > 16) { median-of-3 of (first+1, mid, last-1) swapped to first;
//                     Hoare partition of [first+1,last) around *first; recurse right, loop left }
//   __final_insertion_sort: stable for equal keys.
// so the result = a stable sort by key of the array as the introsort loop leaves it.  One partition
// level is a data-parallel step: with l_j the j-th position (from the left) whose key >= pivot and r_j
// the j-th position (from the right) whose key <= pivot, the loop swaps (l_j, r_j) for every j < J,
// J = #{j : l_j < r_j}, and returns cut = min(l_J, r_{J-1}) (l_0 when J = 0).  All segments of all groups
// advance one level per pass (prefix sums give the ranks).
//
// The level loop itself lives in sortsvc.inc: partition nodes, the finisher and the heaps are tasks that workgroups pull from
// queues, either as jobs of the resident service (k_sort_service) or as one dispatch on the caller's stream (k_sort_job).
//
// Layout of this file:
//   sift_step / make_heap_* / sort_heap_asm / sort_heap_lds_q / sort_heap_hybrid   heapsort of a segment that hit the depth limit
//   wg_ranked_entries                                                             16-bit ranks of a heap's keys (4-byte heap entries)
//   WgTeam / WgLive / LdsTeam, heap_small_body, heap_big_body                     who runs a task body; the two heap task bodies
//   sortsvc.inc                                                                   queues, partition and finisher tasks, the kernels
//   k_se_window_sort                                                              __final_insertion_sort as two tilings of stable window sorts
//   sort_check                                                                    BK_DEBUG=sortcheck
//   SortService, std_sort_groups_svc, std_sort_groups_tasks, std_sort_groups      host side
#include "bk_common.h"
#include "sortemu.h"
#include <vector>
#include <mutex>
#include <algorithm>
#include <cstdio>
#include <chrono>
#include <thread>
#include <cstdlib>

namespace
{
// A store that goes through to memory (sc1): what another workgroup of a running kernel reads after its acquire without the
// storing workgroup having to write back its whole L2 (resident sort service, sortsvc.inc).  p is a global address.
typedef __attribute__((address_space(1))) uint32_t gu32_t;
__device__ __forceinline__ void st_through(uint32_t *p, uint32_t v) { __hip_atomic_store((gu32_t *) p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// Segments of more than 16 elements are partitioned until they hold at most FIN_MAX: the finisher then plays the rest of their
// introsort loop in LDS.  A segment whose depth budget (2 * floor(log2(n)), std::__lg(n) * 2) is used up is heapsorted: up to
// HEAP_BIG_MIN elements by a narrow workgroup or team (heap_small_body), above by a wide workgroup (heap_big_body).
constexpr uint32_t FIN_MAX = 2048;
constexpr uint32_t HEAP_BIG_MIN = 4096;  // = HEAP_RANKED_MIN

// ---- heapsort branch of std::sort (__partial_sort(first,last,last) = make_heap + sort_heap) ----------------
// libstdc++'s __adjust_heap moves the hole to the bottom along the larger-child path and pushes the value back
// up with a strict compare; the net effect equals a top-down sift that stops at the first node whose larger
// child is < value (ties between children go to the right child, equal child keeps descending).  In that form
// every write is final when it is made, so
//   * make_heap runs level by level (nodes of one depth own disjoint subtrees), and
//   * the pops of sort_heap are pipelined inside one wavefront: pop t+1 starts two steps behind pop t and
//     stalls while an in-flight pop could still reach the leaf it is about to detach (ancestor test).
// Verified on the host against std::partial_sort on tie-heavy inputs.
//
// heap entries are packed (key << 32 | idx): one 8-byte access moves an element, the two children of a node are
// adjacent.  Only the key half takes part in comparisons.
typedef unsigned long long hent;
__device__ __forceinline__ uint32_t hkey(hent e) { return (uint32_t) (e >> 32); }

// A second entry format serves heaps of HEAP_RANKED_MIN + 1 .. HEAP_RANKED_MAX elements: (rank of the key inside the segment) << 16
// | local index, 4 bytes, so that twice as much of the heap fits LDS (the heap's own workgroup ranks the keys: wg_ranked_entries).
struct E64
{
  typedef hent T;
  static __device__ __forceinline__ uint32_t key(T e) { return (uint32_t) (e >> 32); }
};
struct E32
{
  typedef uint32_t T;
  static __device__ __forceinline__ uint32_t key(T e) { return e >> 16; }
};

template <class E> struct LdsMemT
{
  typedef typename E::T T;
  T *e;
  static __device__ __forceinline__ uint32_t key(T v) { return E::key(v); }
  __device__ __forceinline__ T ld(uint32_t i) const { return e[i]; }
  __device__ __forceinline__ void st(uint32_t i, T v) const { e[i] = v; }
  __device__ __forceinline__ void step_sync() const { __builtin_amdgcn_wave_barrier(); }
  __device__ __forceinline__ void launch_sync() const { __builtin_amdgcn_wave_barrier(); }
};
// global-memory variant for segments that do not fit LDS.  All lanes belong to one wavefront on one CU, so
// plain accesses are coherent through that CU's write-through L1 (the same guarantee __syncthreads() gives a
// block); every step drains its stores before the next step's loads.
template <class E> struct GlbMemT
{
  typedef typename E::T T;
  T *e;  // plain accesses; the "memory" clobber of step_sync makes the compiler reload after every step
  static __device__ __forceinline__ uint32_t key(T v) { return E::key(v); }
  __device__ __forceinline__ T ld(uint32_t i) const { return e[i]; }
  __device__ __forceinline__ void st(uint32_t i, T v) const { e[i] = v; }
  __device__ __forceinline__ void step_sync() const { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
  // the detached leaf L is out of reach of every in-flight pop (ancestor stall), so its store needs no drain of its own
  __device__ __forceinline__ void launch_sync() const {}
};
typedef LdsMemT<E64> LdsMem;
typedef GlbMemT<E64> GlbMem;

// one top-down sift step of the value v sitting in `hole`; returns true while the hole keeps descending
template <class M> __device__ __forceinline__ bool sift_step(const M &mem, uint32_t &hole, uint32_t len, typename M::T v)
{
  typedef typename M::T T;
  const uint32_t right = 2 * (hole + 1), left = right - 1;
  T ec = 0;
  uint32_t c = 0;
  bool has = true;
  if (right < len)
  {
    const T el = mem.ld(left), er = mem.ld(right);
    if (M::key(er) < M::key(el))
    {
      c = left;
      ec = el;
    }
    else
    {
      c = right;
      ec = er;
    }
  }
  else if (left < len)
  {
    c = left;
    ec = mem.ld(left);
  }
  else
    has = false;
  if (has && !(M::key(ec) < M::key(v)))
  {
    mem.st(hole, ec);
    hole = c;
    return true;
  }
  mem.st(hole, v);
  return false;
}

constexpr uint32_t HEAP_PAD = 32;
// debug: 10 ns ticks of the phases of the last ranked heap of more than 36 000 elements (ranking, make_heap, pops beyond the LDS, pops
// in LDS), written by heap_big_body.  Nothing in the tree reads it (hipMemcpyFromSymbol does); why the stamps stayed when their
// reader went: DESIGN.md section 4, "Round 7"
__device__ unsigned long long g_heap_phase[8];

// the routines below are executed by one full wavefront (64 lanes, all active)
// make_heap, bottom level first (nodes of one depth own disjoint subtrees)
template <class M> __device__ void make_heap_wave(const M &mem, const uint32_t m)
{
  if (m < 2) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t lastp = (m - 2) / 2;
  for (int d = 31 - __clz(lastp + 1); d >= 0; --d)
  {
    const uint32_t lo = (1u << d) - 1;
    uint32_t hi = (1u << (d + 1)) - 2;
    if (hi > lastp) hi = lastp;
    for (uint32_t base = lo; base <= hi; base += 64)
    {
      const uint32_t p = base + lane;
      if (p <= hi)
      {
        uint32_t hole = p;
        const typename M::T v = mem.ld(p);
        while (sift_step(mem, hole, m, v))
        {
        }
      }
      mem.step_sync();
    }
  }
}

// the same with every wave of the workgroup (NT threads, all of them call this): the nodes of one depth are spread over the
// waves, a barrier separates the depths
template <class M> __device__ void make_heap_block(const M &mem, const uint32_t m, const uint32_t NT)
{
  if (m < 2) return;
  const uint32_t lastp = (m - 2) / 2;
  for (int d = 31 - __clz(lastp + 1); d >= 0; --d)
  {
    const uint32_t lo = (1u << d) - 1;
    uint32_t hi = (1u << (d + 1)) - 2;
    if (hi > lastp) hi = lastp;
    for (uint32_t p = lo + threadIdx.x; p <= hi; p += NT)
    {
      uint32_t hole = p;
      const typename M::T v = mem.ld(p);
      while (sift_step(mem, hole, m, v))
      {
      }
    }
    mem.step_sync();
    __syncthreads();
  }
}

// sort_heap: pops follow each other two steps apart (lag-2 pipeline) until the heap has shrunk to `stop` elements;
// every pop has finished when this returns.  One loop iteration = one sift step of every pop in flight (one lane
// each) + at most one launch; the values a launch needs (the root and the leaf about to be detached) are fetched
// together with the children of the holes.  Written in GCN assembly: a lone wavefront issues at most one instruction
// every 4 cycles, so the segment's critical path is the instruction count of one loop iteration; compiled C++ spends
// ~80 instructions per iteration on mask bookkeeping, this ~25 (+~25 in an iteration that launches).  Per-lane state: h1 = hole + 1 (v40), len (v41; 0 = idle lane), value (idx v42, key v43).
// Uniform state: next_t (s41), L+1 (s43), clz(L+1) (s44), budget (s45), t_end (s46).
// GLB = false: heap in LDS at byte offset `base`; GLB = true: heap in global memory at `gptr` (base = 0).
// Global variant: the loads of a step follow the stores of the step before in program order through the same L1,
// which keeps them ordered per address for one wavefront; the loop therefore only waits for its loads
// (`s_waitcnt vmcnt(0)` before their use also covers the older stores) and does not drain the store acknowledgements
// at the top of every step (0.34 -> 0.26 us per step).  The caller drains before it reads the result.
// Two ways to keep idle lanes (no pop in flight) harmless.  Global memory: their store is masked by EXEC and len = 0
// marks them.  LDS: an idle lane points at a spare slot behind the heap (h1 = m + 2, v55), so it runs the same
// unmasked instructions as everybody else - its "children" are out of range, its store hits the spare slot, and it
// can never be an ancestor of the leaf to detach; that takes 7 instructions out of an iteration.
#define BK_MASKED_STORE(ST) "v_cmp_ne_u32_e64 s[58:59], 0, v41\n s_and_saveexec_b64 s[56:57], s[58:59]\n" ST "s_mov_b64 exec, s[56:57]\n"
#define BK_PLAIN_STORE(ST) ST
#define BK_IDLE_BY_LEN "v_cndmask_b32_e64 v40, v40, v53, s[54:55]\n v_cndmask_b32_e64 v41, 0, v41, s[54:55]\n"
#define BK_IDLE_BY_SLOT "v_cndmask_b32_e64 v40, v55, v53, s[54:55]\n"
#define BK_CHECK_ACTIVE_LEN "v_cmp_ne_u32_e64 s[60:61], 0, v41\n s_and_b64 vcc, vcc, s[60:61]\n v_cmp_eq_u32_e64 s[60:61], s43, v54\n s_and_b64 s[60:61], s[60:61], s[58:59]\n"
#define BK_CHECK_ACTIVE_SLOT "v_cmp_eq_u32_e64 s[60:61], s43, v54\n"
#define BK_ANY_ACTIVE_LEN "v_cmp_ne_u32_e32 vcc, 0, v41\n"
#define BK_ANY_ACTIVE_SLOT "v_cmp_ne_u32_e32 vcc, v40, v55\n"

// one sift step of every pop in flight
#define BK_HEAP_SIFT(LD2_KIDS, STORE_HOLE, WAIT_LOADS, IDLE_UPD)                                                                         \
  "v_lshlrev_b32 v44, 1, v40\n"                                                                                            \
  "v_cmp_le_u32_e64 s[48:49], v44, v41\n"                                                                                  \
  "v_cmp_lt_u32_e64 s[50:51], v44, v41\n"                                                                                  \
  "v_lshl_add_u32 v45, v44, 3, s40\n"                                                                                      \
  "v_cndmask_b32_e64 v45, v60, v45, s[48:49]\n"                                                                            \
  LD2_KIDS                                                                                                                \
  "v_lshl_add_u32 v52, v40, 3, s40\n"                                                                                      \
  "v_mov_b32 v54, v40\n"                                                                                                   \
  WAIT_LOADS                                                                                                              \
  "v_cmp_ge_u32_e32 vcc, v49, v47\n"                                                                                       \
  "s_and_b64 s[52:53], vcc, s[50:51]\n"                                                                                    \
  "v_cndmask_b32_e64 v51, v47, v49, s[52:53]\n"                                                                            \
  "v_cndmask_b32_e64 v50, v46, v48, s[52:53]\n"                                                                            \
  "v_cmp_ge_u32_e32 vcc, v51, v43\n"                                                                                       \
  "s_and_b64 s[54:55], vcc, s[48:49]\n"                                                                                    \
  "v_cndmask_b32_e64 v51, v43, v51, s[54:55]\n"                                                                            \
  "v_cndmask_b32_e64 v50, v42, v50, s[54:55]\n"                                                                            \
  STORE_HOLE                                                                                                              \
  "v_addc_co_u32_e64 v53, vcc, v44, 0, s[52:53]\n"                                                                         \
  IDLE_UPD

// Loop A = the iteration right after a launch (the next pop may not start yet: lag 2), loop B = iterations that may
// launch: they prefetch the root and the leaf to detach together with the children of the holes.
#define BK_HEAP_ASM(LD1_ROOT, LD1_LEAF, LD2_KIDS, STORE_HOLE, ST_LEAF, WAIT_LOADS, WAIT_ALL, IDLE_UPD, CHECK_ACTIVE, ANY_ACTIVE)                                      \
  "v_mov_b32 v62, %[lane]\n"                                                                                               \
  "s_mov_b32 s62, %[plo]\n s_mov_b32 s63, %[phi]\n"                                                                          \
  "s_sub_u32 s40, %[base], 8\n"                                                                                            \
  "v_mov_b32 v60, %[base]\n"                                                                                               \
  "s_mov_b32 s46, %[tend]\n s_mov_b32 s41, 1\n s_mov_b32 s43, %[m]\n"                                                       \
  "s_flbit_i32_b32 s44, s43\n"                                                                                             \
  "s_lshl_b32 s47, s43, 3\n s_add_u32 s47, s47, s40\n v_mov_b32 v61, s47\n"                                                  \
  "s_mov_b32 s45, %[budget]\n"                                                                                             \
  "s_add_u32 s47, %[m], 2\n v_mov_b32 v55, s47\n v_mov_b32 v40, v55\n v_mov_b32 v41, 0\n v_mov_b32 v42, 0\n v_mov_b32 v43, 0\n"                                               \
  "s_branch BK_B_%=\n"                                                                                                     \
  "BK_A_%=:\n"                                                                                                            \
  WAIT_ALL                                                                                                                \
  BK_HEAP_SIFT(LD2_KIDS, STORE_HOLE, WAIT_LOADS, IDLE_UPD)                                                                             \
  "s_sub_u32 s45, s45, 1\n"                                                                                                \
  "s_cbranch_scc1 BK_DONE_%=\n"                                                                                            \
  "BK_B_%=:\n"                                                                                                            \
  WAIT_ALL LD1_ROOT LD1_LEAF                                                                                              \
  BK_HEAP_SIFT(LD2_KIDS, STORE_HOLE, WAIT_LOADS, IDLE_UPD)                                                                             \
  "s_cmp_ge_u32 s41, s46\n"                                                                                                \
  "s_cbranch_scc1 BK_NOMORE_%=\n"                                                                                          \
  "v_ffbh_u32_e32 v63, v40\n"                                                                                              \
  "v_subrev_u32_e32 v63, s44, v63\n"                                                                                       \
  "v_lshrrev_b32_e64 v64, v63, s43\n"                                                                                      \
  "v_cmp_eq_u32_e32 vcc, v64, v40\n"                                                                                       \
  "v_cmp_gt_u32_e64 s[60:61], 32, v63\n"                                                                                   \
  "s_and_b64 vcc, vcc, s[60:61]\n"                                                                                         \
  CHECK_ACTIVE                                                                                                            \
  "s_or_b64 vcc, vcc, s[60:61]\n"                                                                                          \
  "s_cbranch_vccnz BK_BNEXT_%=\n"                                                                                          \
  "s_and_b32 s47, s41, 63\n"                                                                                               \
  "v_cmp_eq_u32_e32 vcc, s47, v62\n"                                                                                       \
  "s_sub_u32 s47, s43, 1\n"                                                                                                \
  "s_and_saveexec_b64 s[56:57], vcc\n"                                                                                     \
  ST_LEAF                                                                                                                 \
  "v_mov_b32 v42, v58\n v_mov_b32 v43, v59\n v_mov_b32 v40, 1\n v_mov_b32 v41, s47\n"                                         \
  "s_mov_b64 exec, s[56:57]\n"                                                                                             \
  "s_add_u32 s41, s41, 1\n"                                                                                                \
  "s_mov_b32 s43, s47\n"                                                                                                   \
  "s_flbit_i32_b32 s44, s43\n"                                                                                             \
  "v_add_u32_e32 v61, -8, v61\n"                                                                                           \
  "s_sub_u32 s45, s45, 1\n"                                                                                                \
  "s_cbranch_scc0 BK_A_%=\n"                                                                                               \
  "s_branch BK_DONE_%=\n"                                                                                                  \
  "BK_NOMORE_%=:\n"                                                                                                       \
  ANY_ACTIVE                                                                                                              \
  "s_cbranch_vccz BK_DONE_%=\n"                                                                                            \
  "BK_BNEXT_%=:\n"                                                                                                        \
  "s_sub_u32 s45, s45, 1\n"                                                                                                \
  "s_cbranch_scc0 BK_B_%=\n"                                                                                               \
  "BK_DONE_%=:\n"                                                                                                         \
  WAIT_ALL

#define BK_HEAP_CLOBBERS                                                                                                     \
  "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v56", "v57", "v58", \
      "v55", "v59", "v60", "v61", "v62", "v63", "v64", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50",    \
      "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "vcc", "scc", "memory"

template <bool GLB> __device__ __forceinline__ void sort_heap_asm(hent *buf, const uint32_t m, const uint32_t stop)
{
  if (m < 2 || m <= stop) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t t_end = __builtin_amdgcn_readfirstlane(m - (stop < 1 ? 1 : stop) + 1);
  const uint32_t budget = __builtin_amdgcn_readfirstlane(m > 0x03000000u ? 0xFFFFFFFFu : 64u * m + 4096u);
  const uint32_t mm = __builtin_amdgcn_readfirstlane(m);
  const unsigned long long p = (unsigned long long) buf;
  const uint32_t plo = __builtin_amdgcn_readfirstlane((uint32_t) p), phi = __builtin_amdgcn_readfirstlane((uint32_t) (p >> 32));
  const uint32_t base = GLB ? 0u : plo;  // low half of a flat LDS address = byte offset inside LDS
  if (GLB)
    asm volatile(BK_HEAP_ASM("global_load_dwordx2 v[56:57], v60, s[62:63]\n", "global_load_dwordx2 v[58:59], v61, s[62:63]\n",
                             "global_load_dwordx4 v[46:49], v45, s[62:63]\n", BK_MASKED_STORE("global_store_dwordx2 v52, v[50:51], s[62:63]\n"),
                             "global_store_dwordx2 v61, v[56:57], s[62:63]\n", "s_waitcnt vmcnt(0)\n", "", BK_IDLE_BY_LEN, BK_CHECK_ACTIVE_LEN, BK_ANY_ACTIVE_LEN)
                 :
                 : [lane] "v"(lane), [plo] "s"(plo), [phi] "s"(phi), [base] "s"(base), [tend] "s"(t_end), [m] "s"(mm), [budget] "s"(budget)
                 : BK_HEAP_CLOBBERS);
  else
    asm volatile(BK_HEAP_ASM("ds_read_b64 v[56:57], v60\n", "ds_read_b64 v[58:59], v61\n", "ds_read2_b64 v[46:49], v45 offset1:1\n",
                             BK_PLAIN_STORE("ds_write_b64 v52, v[50:51]\n"), "ds_write_b64 v61, v[56:57]\n", "s_waitcnt lgkmcnt(0)\n", "", BK_IDLE_BY_SLOT,
                             BK_CHECK_ACTIVE_SLOT, BK_ANY_ACTIVE_SLOT)
                 :
                 : [lane] "v"(lane), [plo] "s"(plo), [phi] "s"(phi), [base] "s"(base), [tend] "s"(t_end), [m] "s"(mm), [budget] "s"(budget)
                 : BK_HEAP_CLOBBERS);
  if (!GLB) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ---- the pop pipeline for ranked entries in LDS: no existence masks, scheduled for a lone wave ------------------------------
// Entries are ((rank + 1) << 16 | local index), never 0.  The heap lives in LDS slots 1..m (slot s at base - 4 + 4 s, so the
// children of hole h are the adjacent slots 2h, 2h + 1); slot 0 is scratch, slots m + 1, m + 2 hold zeros and child
// addresses beyond them are clamped onto them.  A detached leaf slot is ZEROED and the popped root goes straight to the
// output array in global memory (a store nobody waits for) instead of into the freed slot.  A zero reads as "rank below
// every value": the sift stops in front of a child that does not exist (any more) without a per-lane heap length, so the
// two existence masks of the loop above, their SALU round trips and the key extraction are gone.  An idle lane sits on hole 0
// with value 0xffffffff: it reads slots 0 / 1, never descends, stores into slot 0, and can never look like an ancestor of the
// leaf to detach.  Same lag-2 launch rule and ancestor stall as above (a slot is only zeroed when no pop in flight can still
// reach it).
// A wave that is alone on its SIMD issues one instruction every 4 cycles whatever it is, so a pop costs its instruction
// count plus whatever LDS latency is left exposed:
//   * rank compares on the high halves directly (SDWA WORD_1 selects);
//   * the children of the NEXT step's hole are requested as soon as this step's hole is known (behind this step's store in
//     program order, so they see it); the launch decision, the launch and the bookkeeping of a launch (which moves into the
//     following iteration) run while that read is in flight;
//   * the ancestor test is prepared from the holes BEFORE the step while the children are still on their way: a lane that
//     descends ends one level deeper, so the only ancestor of L it can reach is L >> (clz(hole) - 1 - clz(L)) (a hole that
//     ends below L's level is compared with L itself, which it cannot equal; a lane that sits ON L stops there, so it is
//     compared with 0, the hole of a lane that stopped); after the step ONE vector compare against the new holes and a
//     branch are left - a scalar instruction that combines masks a vector compare has just written waits ~20 clocks for
//     them (tools/ubench/issue.hip);
//   * the launching lane is a rotating one-hot mask in SGPRs; the launches left are counted in the launch path (s46: its
//     borrow ends the launches), so an iteration that may launch does not test for the end; after the last launch a plain
//     loop of steps drains the pops in flight.
// 20 instructions in the iteration after a launch, 36 in a launching one.
// Per-lane: hole v40 (0 = idle), value v42 (-1 = idle).  Uniform: L s43, clz(L) + 1 s47, budget s45, clamp address s42,
// launch mask s[58:59].
#define BK_HEAP32Q_STEP                                                                                                   \
  "v_cmp_ge_u32_sdwa vcc, v47, v46 src0_sel:WORD_1 src1_sel:WORD_1\n"                                                      \
  "v_cndmask_b32 v50, v46, v47, vcc\n"                                                                                     \
  "v_addc_co_u32_e32 v53, vcc, v40, v40, vcc\n"                                                                            \
  "v_cmp_ge_u32_sdwa vcc, v50, v42 src0_sel:WORD_1 src1_sel:WORD_1\n"                                                      \
  "v_cndmask_b32 v51, v42, v50, vcc\n"                                                                                     \
  "ds_write_b32 v52, v51\n"                                                                                                \
  "v_cndmask_b32 v40, v55, v53, vcc\n"                                                                                     \
  "v_cndmask_b32 v42, v59, v42, vcc\n"
#define BK_HEAP32Q_NEXT                                                                                                   \
  "v_lshl_add_u32 v45, v40, 3, s40\n"                                                                                      \
  "v_min_u32 v45, s42, v45\n"                                                                                              \
  "ds_read2_b32 v[46:47], v45 offset1:1\n"
#define BK_HEAP32Q_ASM                                                                                                    \
  "s_setprio 3\n"                                                                                                          \
  "s_mov_b64 s[56:57], exec\n"                                                                                             \
  "s_mov_b32 s62, %[olo]\n s_mov_b32 s63, %[ohi]\n"                                                                        \
  "s_sub_u32 s40, %[base], 4\n"                                                                                            \
  "v_mov_b32 v60, %[base]\n"                                                                                               \
  "s_mov_b32 s43, %[m]\n"                                                                                                  \
  "s_sub_u32 s46, s43, 2\n"                                                                                               \
  "s_flbit_i32_b32 s47, s43\n s_add_u32 s47, s47, 1\n"                                                                     \
  "s_lshl_b32 s48, s43, 2\n s_add_u32 s42, s48, %[base]\n"                                                                 \
  "s_add_u32 s48, s48, s40\n v_mov_b32 v61, s48\n"                                                                         \
  "s_lshl_b32 s48, s43, 2\n s_sub_u32 s48, s48, 4\n v_mov_b32 v57, s48\n"                                                  \
  "s_mov_b32 s45, %[budget]\n"                                                                                             \
  "v_mov_b32 v55, 0\n v_mov_b32 v59, -1\n v_mov_b32 v40, 0\n v_mov_b32 v42, -1\n"                                          \
  "s_mov_b64 s[58:59], 1\n"                                                                                                \
  "v_mov_b32 v45, s40\n"                                                                                                   \
  "ds_read2_b32 v[46:47], v45 offset1:1\n"                                                                                 \
  "s_branch BK_QB_%=\n"                                                                                                    \
  "BK_QA_%=:\n"                                                                                                           \
  "v_lshl_add_u32 v52, v40, 2, s40\n"                                                                                      \
  "s_sub_u32 s43, s43, 1\n"                                                                                                \
  "s_flbit_i32_b32 s47, s43\n"                                                                                             \
  "s_add_u32 s47, s47, 1\n"                                                                                                \
  "v_add_u32 v61, -4, v61\n"                                                                                               \
  "v_add_u32 v57, -4, v57\n"                                                                                               \
  "s_lshl_b64 s[58:59], s[58:59], 1\n"                                                                                     \
  "s_cselect_b64 s[58:59], s[58:59], 1\n"                                                                                  \
  "s_waitcnt lgkmcnt(0)\n"                                                                                                 \
  BK_HEAP32Q_STEP                                                                                                         \
  BK_HEAP32Q_NEXT                                                                                                         \
  "BK_QB_%=:\n"                                                                                                           \
  "ds_read_b32 v56, v60\n"                                                                                                 \
  "ds_read_b32 v58, v61\n"                                                                                                 \
  "v_lshl_add_u32 v52, v40, 2, s40\n"                                                                                      \
  "v_ffbh_u32 v63, v40\n"                                                                                                  \
  "v_subrev_u32 v63, s47, v63\n"                                                                                           \
  "v_max_i32 v63, 0, v63\n"                                                                                                \
  "v_lshrrev_b32_e64 v64, v63, s43\n"                                                                                      \
  "v_cmp_eq_u32 vcc, s43, v40\n"                                                                                           \
  "v_cndmask_b32 v64, v64, v55, vcc\n"                                                                                     \
  "s_waitcnt lgkmcnt(2)\n"                                                                                                 \
  BK_HEAP32Q_STEP                                                                                                         \
  "v_cmp_eq_u32 vcc, v64, v40\n"                                                                                           \
  BK_HEAP32Q_NEXT                                                                                                         \
  "s_cbranch_vccnz BK_QBNEXT_%=\n"                                                                                         \
  "s_waitcnt lgkmcnt(2)\n"                                                                                                 \
  "s_mov_b64 exec, s[58:59]\n"                                                                                             \
  "ds_write_b32 v61, v55\n"                                                                                                \
  "global_store_dword v57, v56, s[62:63]\n"                                                                                \
  "v_mov_b32 v42, v58\n"                                                                                                   \
  "v_mov_b32 v40, 1\n"                                                                                                     \
  "ds_read2_b32 v[46:47], v60 offset0:1 offset1:2\n"                                                                       \
  "s_mov_b64 exec, s[56:57]\n"                                                                                                   \
  "s_sub_u32 s46, s46, 1\n"                                                                                               \
  "s_cbranch_scc0 BK_QA_%=\n"                                                                                              \
  "s_branch BK_QDRAIN_%=\n"                                                                                                 \
  "BK_QBNEXT_%=:\n"                                                                                                       \
  "s_sub_u32 s45, s45, 1\n"                                                                                               \
  "s_cbranch_scc0 BK_QB_%=\n"                                                                                             \
  "s_branch BK_QDONE_%=\n"                                                                                                \
  "BK_QDRAIN_%=:\n"                                                                                                       \
  "v_lshl_add_u32 v52, v40, 2, s40\n"                                                                                     \
  "s_waitcnt lgkmcnt(0)\n"                                                                                                \
  BK_HEAP32Q_STEP                                                                                                         \
  BK_HEAP32Q_NEXT                                                                                                         \
  "v_cmp_ne_u32 vcc, 0, v40\n"                                                                                            \
  "s_cbranch_vccz BK_QDONE_%=\n"                                                                                          \
  "s_sub_u32 s45, s45, 1\n"                                                                                               \
  "s_cbranch_scc0 BK_QDRAIN_%=\n"                                                                                         \
  "BK_QDONE_%=:\n"                                                                                                        \
  "s_waitcnt lgkmcnt(0)\n"                                                                                                 \
  "s_setprio 0\n"

// slot1 = LDS address of slot 1 (slot 0 in front of it and the two zero slots behind slot m belong to the caller); pops
// t = 1 .. m - 1 store the popped roots to out[m - 1] .. out[1]; the last element stays in slot 1
__device__ __forceinline__ void sort_heap_lds_q(uint32_t *slot1, const uint32_t m, uint32_t *out)
{
  if (m < 2) return;
  const uint32_t budget = __builtin_amdgcn_readfirstlane(64u * m + 4096u);
  const uint32_t mm = __builtin_amdgcn_readfirstlane(m);
  const unsigned long long o = (unsigned long long) out;
  const uint32_t olo = __builtin_amdgcn_readfirstlane((uint32_t) o), ohi = __builtin_amdgcn_readfirstlane((uint32_t) (o >> 32));
  const uint32_t base = __builtin_amdgcn_readfirstlane((uint32_t) (unsigned long long) slot1);
  asm volatile(BK_HEAP32Q_ASM
               :
               : [olo] "s"(olo), [ohi] "s"(ohi), [base] "s"(base), [m] "s"(mm), [budget] "s"(budget)
               : BK_HEAP_CLOBBERS);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

// ---- a heap that is larger than the LDS: the same loop with its tail in global memory ------------------------------------
// Slots 1 .. CAP (the CU's LDS) hold the upper levels, slots CAP+1 .. m live in a global array O (O[slot]); m < 2 (CAP + 1), so
// every slot in O is a leaf.  The loop is sort_heap_lds_q with three additions (model: the same schedule was checked against
// libstdc++ on the host before it was written):
//   * after every step one more vector compare asks whether a new hole lies beyond CAP / 2, i.e. has its children in O (or
//     lies in O itself); if none does - most iterations - nothing else changes;
//   * otherwise: a lane whose new hole lies IN O is done - a leaf: it stores its value there one step early and goes idle
//     (if that leaf is L, the value is also the leaf of the next launch); a lane whose children are in O loads them from
//     there (slots beyond m read the zeros behind the heap) over the zeros its clamped LDS read returned;
//   * the leaf to detach is in O: it is requested right after the launch before (two to three iterations ahead of its use)
//     and zeroed there by the launch.  When a lane finishes ON that leaf meanwhile, its value replaces the requested one in
//     v58 - behind a wait for the request, which would otherwise land in v58 afterwards with the slot's old content (the
//     hardware does not order a load's register write against a later VALU write: one payload lost, another doubled, in a few
//     per cent of the runs over a 53 K-element heap before this wait was there).
// Runs the m - CAP pops that bring the heap down to CAP slots, waits for the pops in flight and returns; the caller carries
// on with sort_heap_lds_q on the LDS part.  0.6 us per pop (everything in global memory) -> ~0.25.
#define BK_HEAP32H_SLOW(TAG)                                                                                                  \
  "v_cmp_lt_u32_e64 s[52:53], s67, v40\n"                                                                                  \
  "s_mov_b64 exec, s[52:53]\n"                                                                                             \
  "v_mov_b32 v71, v42\n"                                                                                                   \
  "v_lshlrev_b32 v70, 2, v40\n"                                                                                            \
  "global_store_dword v70, v42, s[64:65]\n"                                                                                \
  "v_cmp_eq_u32_e64 s[54:55], s43, v40\n"                                                                                  \
  "v_mov_b32 v40, 0\n"                                                                                                     \
  "v_mov_b32 v42, -1\n"                                                                                                    \
  "s_mov_b64 exec, s[56:57]\n"                                                                                             \
  "s_cmp_lg_u64 s[54:55], 0\n"                                                                                             \
  "s_cbranch_scc0 BK_HS1_" TAG "_%=\n"                                                                                             \
  "s_ff1_i32_b64 s70, s[54:55]\n"                                                                                          \
  "s_nop 3\n"                                                                                                              \
  "v_readlane_b32 s69, v71, s70\n"                                                                                         \
  "s_waitcnt vmcnt(0)\n"                                                                                                   \
  "v_mov_b32 v58, s69\n"                                                                                                   \
  "BK_HS1_" TAG "_%=:\n"                                                                                                          \
  "v_cmp_lt_u32_e64 s[50:51], s66, v40\n"                                                                                  \
  "s_mov_b64 exec, s[50:51]\n"                                                                                             \
  "v_lshlrev_b32 v70, 1, v40\n"                                                                                            \
  "v_min_u32 v70, s68, v70\n"                                                                                              \
  "v_lshlrev_b32 v70, 2, v70\n"                                                                                            \
  "global_load_dwordx2 v[68:69], v70, s[64:65]\n"                                                                          \
  "s_mov_b64 exec, s[56:57]\n"                                                                                             \
  "s_waitcnt vmcnt(0) lgkmcnt(0)\n"                                                                                        \
  "v_cndmask_b32_e64 v46, v46, v68, s[50:51]\n"                                                                            \
  "v_cndmask_b32_e64 v47, v47, v69, s[50:51]\n"
#define BK_HEAP32H_ASM                                                                                                    \
  "s_setprio 3\n"                                                                                                          \
  "s_mov_b64 s[56:57], exec\n"                                                                                             \
  "s_mov_b32 s62, %[olo]\n s_mov_b32 s63, %[ohi]\n"                                                                        \
  "s_mov_b32 s64, %[plo]\n s_mov_b32 s65, %[phi]\n"                                                                        \
  "s_sub_u32 s40, %[base], 4\n"                                                                                            \
  "v_mov_b32 v60, %[base]\n"                                                                                               \
  "s_mov_b32 s43, %[m]\n"                                                                                                  \
  "s_mov_b32 s67, %[cap]\n"                                                                                                \
  "s_lshr_b32 s66, s67, 1\n"                                                                                               \
  "s_add_u32 s68, s43, 1\n"                                                                                                \
  "s_sub_u32 s46, s43, s67\n s_sub_u32 s46, s46, 1\n"                                                                      \
  "s_flbit_i32_b32 s47, s43\n s_add_u32 s47, s47, 1\n"                                                                     \
  "s_add_u32 s48, s67, 1\n s_lshl_b32 s48, s48, 2\n s_add_u32 s42, s48, s40\n"                                             \
  "s_lshl_b32 s48, s43, 2\n v_mov_b32 v61, s48\n"                                                                          \
  "s_sub_u32 s48, s48, 4\n v_mov_b32 v57, s48\n"                                                                           \
  "s_mov_b32 s45, %[budget]\n"                                                                                             \
  "v_mov_b32 v55, 0\n v_mov_b32 v59, -1\n v_mov_b32 v40, 0\n v_mov_b32 v42, -1\n"                                          \
  "s_mov_b64 s[58:59], 1\n"                                                                                                \
  "global_load_dword v58, v61, s[64:65]\n"                                                                                 \
  "v_mov_b32 v45, s40\n"                                                                                                   \
  "ds_read2_b32 v[46:47], v45 offset1:1\n"                                                                                 \
  "s_branch BK_HB_%=\n"                                                                                                    \
  "BK_HA_%=:\n"                                                                                                           \
  "v_lshl_add_u32 v52, v40, 2, s40\n"                                                                                      \
  "s_sub_u32 s43, s43, 1\n"                                                                                                \
  "s_flbit_i32_b32 s47, s43\n"                                                                                             \
  "s_add_u32 s47, s47, 1\n"                                                                                                \
  "v_add_u32 v61, -4, v61\n"                                                                                               \
  "v_add_u32 v57, -4, v57\n"                                                                                               \
  "s_lshl_b64 s[58:59], s[58:59], 1\n"                                                                                     \
  "s_cselect_b64 s[58:59], s[58:59], 1\n"                                                                                  \
  "global_load_dword v58, v61, s[64:65]\n"                                                                                 \
  "s_waitcnt lgkmcnt(0)\n"                                                                                                 \
  BK_HEAP32Q_STEP                                                                                                         \
  "v_cmp_lt_u32_e64 s[50:51], s66, v40\n"                                                                                  \
  BK_HEAP32Q_NEXT                                                                                                         \
  "s_cmp_lg_u64 s[50:51], 0\n"                                                                                             \
  "s_cbranch_scc0 BK_HB_%=\n"                                                                                              \
  BK_HEAP32H_SLOW("a")                                                                                                    \
  "BK_HB_%=:\n"                                                                                                           \
  "ds_read_b32 v56, v60\n"                                                                                                 \
  "v_lshl_add_u32 v52, v40, 2, s40\n"                                                                                      \
  "v_ffbh_u32 v63, v40\n"                                                                                                  \
  "v_subrev_u32 v63, s47, v63\n"                                                                                           \
  "v_max_i32 v63, 0, v63\n"                                                                                                \
  "v_lshrrev_b32_e64 v64, v63, s43\n"                                                                                      \
  "s_waitcnt lgkmcnt(1)\n"                                                                                                 \
  BK_HEAP32Q_STEP                                                                                                         \
  "v_cmp_eq_u32 vcc, v64, v40\n"                                                                                           \
  "v_cmp_lt_u32_e64 s[50:51], s66, v40\n"                                                                                  \
  BK_HEAP32Q_NEXT                                                                                                         \
  "s_cmp_lg_u64 s[50:51], 0\n"                                                                                             \
  "s_cbranch_scc0 BK_HB2_%=\n"                                                                                             \
  BK_HEAP32H_SLOW("b")                                                                                                    \
  "v_cmp_eq_u32 vcc, v64, v40\n"                                                                                           \
  "BK_HB2_%=:\n"                                                                                                          \
  "s_cbranch_vccnz BK_HBNEXT_%=\n"                                                                                         \
  "s_waitcnt vmcnt(0) lgkmcnt(2)\n"                                                                                        \
  "s_mov_b64 exec, s[58:59]\n"                                                                                             \
  "global_store_dword v61, v55, s[64:65]\n"                                                                                \
  "global_store_dword v57, v56, s[62:63]\n"                                                                                \
  "v_mov_b32 v42, v58\n"                                                                                                   \
  "v_mov_b32 v40, 1\n"                                                                                                     \
  "ds_read2_b32 v[46:47], v60 offset0:1 offset1:2\n"                                                                       \
  "s_mov_b64 exec, s[56:57]\n"                                                                                             \
  "s_sub_u32 s46, s46, 1\n"                                                                                                \
  "s_cbranch_scc0 BK_HA_%=\n"                                                                                              \
  "s_branch BK_HDRAIN_%=\n"                                                                                                \
  "BK_HBNEXT_%=:\n"                                                                                                       \
  "s_sub_u32 s45, s45, 1\n"                                                                                                \
  "s_cbranch_scc0 BK_HB_%=\n"                                                                                              \
  "s_branch BK_HDONE_%=\n"                                                                                                 \
  "BK_HDRAIN_%=:\n"                                                                                                       \
  "v_lshl_add_u32 v52, v40, 2, s40\n"                                                                                      \
  "s_waitcnt lgkmcnt(0)\n"                                                                                                 \
  BK_HEAP32Q_STEP                                                                                                         \
  "v_cmp_lt_u32_e64 s[50:51], s66, v40\n"                                                                                  \
  BK_HEAP32Q_NEXT                                                                                                         \
  "s_cmp_lg_u64 s[50:51], 0\n"                                                                                             \
  "s_cbranch_scc0 BK_HD2_%=\n"                                                                                             \
  BK_HEAP32H_SLOW("d")                                                                                                    \
  "BK_HD2_%=:\n"                                                                                                          \
  "v_cmp_ne_u32 vcc, 0, v40\n"                                                                                             \
  "s_cbranch_vccz BK_HDONE_%=\n"                                                                                           \
  "s_sub_u32 s45, s45, 1\n"                                                                                                \
  "s_cbranch_scc0 BK_HDRAIN_%=\n"                                                                                          \
  "BK_HDONE_%=:\n"                                                                                                        \
  "s_waitcnt vmcnt(0) lgkmcnt(0)\n"                                                                                        \
  "s_setprio 0\n"

// slot1 = LDS address of slot 1 (slots 0, cap+1, cap+2 zero), ovf = O (ovf[slot] for cap < slot <= m + 2, the last two zero),
// m > cap odd, m < 2 (cap + 1); pops leaves m .. cap+1 to out[m-1 .. cap]; the heap is left in LDS slots 1 .. cap
__device__ __forceinline__ void sort_heap_hybrid(uint32_t *slot1, const uint32_t m, const uint32_t cap, uint32_t *ovf, uint32_t *out)
{
  const uint32_t budget = __builtin_amdgcn_readfirstlane(64u * (m - cap) + 4096u);
  const uint32_t mm = __builtin_amdgcn_readfirstlane(m), cc = __builtin_amdgcn_readfirstlane(cap);
  const unsigned long long o = (unsigned long long) out, pp = (unsigned long long) ovf;
  const uint32_t olo = __builtin_amdgcn_readfirstlane((uint32_t) o), ohi = __builtin_amdgcn_readfirstlane((uint32_t) (o >> 32));
  const uint32_t plo = __builtin_amdgcn_readfirstlane((uint32_t) pp), phi = __builtin_amdgcn_readfirstlane((uint32_t) (pp >> 32));
  const uint32_t base = __builtin_amdgcn_readfirstlane((uint32_t) (unsigned long long) slot1);
  asm volatile(BK_HEAP32H_ASM
               :
               : [olo] "s"(olo), [ohi] "s"(ohi), [plo] "s"(plo), [phi] "s"(phi), [base] "s"(base), [m] "s"(mm), [cap] "s"(cc), [budget] "s"(budget)
               : BK_HEAP_CLOBBERS, "v68", "v69", "v70", "v71", "s64", "s65", "s66", "s67", "s68", "s69", "s70");
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

constexpr uint32_t HEAP_LARGE = 20000;       // packed 8-byte entries that fit a CU's LDS (156 KiB): heaps beyond HEAP_RANKED_MAX finish there
constexpr uint32_t HEAP_RANKED_MIN = 4096;   // heaps above this size run on ranked entries (sort_heap_lds_q)
constexpr uint32_t HEAP_RANKED_MAX = 65534;  // rank + 1 must fit 16 bits and stay below the idle marker's 0xffff
constexpr uint32_t RK_UNROLL = 4;
// Dense ranks of the m <= 65534 keys of ONE heap segment by the workgroup that is about to heapsort it: entries (key << 16 | position)
// go through four stable 8-bit counting passes between two scratch arrays in global memory (wave w owns a contiguous run of rows
// of 64 entries; a row's lanes find the lanes of the same digit with eight ballots, the first of them moves the wave's running
// base of that digit), then out[position] = (number of smaller DISTINCT keys + 1) << 16 | position: the ranked entries of
// sort_heap_lds_q.  lds: (NW + 1) * 256 words of scratch, wcnt: NW + 1 words behind them (all inside the dynamic LDS the heap is
// loaded into afterwards: `out` may be that LDS - the scratch is dead when the entries are written).
// Replaces the device-wide ranking (count / gather / five radix passes / flags / scan / scatter: ~30 launches and two host looks in
// front of every sort's longest heap) by ~60 us inside the heap's own workgroup.
__device__ void wg_ranked_entries(const uint32_t *gk, const uint32_t m, unsigned long long *A, unsigned long long *B, uint32_t *out, uint32_t *lds, uint32_t *wcnt, const uint32_t NT)
{
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6, NW = NT >> 6;
  for (uint32_t i = tid; i < m; i += NT) A[i] = ((unsigned long long) gk[i] << 16) | i;
  const uint32_t rows = (m + 63) / 64, rpw = (rows + NW - 1) / NW;
  const uint32_t r0 = min(rows, w * rpw), r1 = min(rows, r0 + rpw);
  unsigned long long *src = A, *dst = B;
  __syncthreads();
  for (int pass = 0; pass < 4; ++pass)
  {
    const int sh = 16 + 8 * pass;
    uint32_t *hist = lds + w * 256;
    for (uint32_t d = lane; d < 256; d += 64) hist[d] = 0;
    for (uint32_t r = r0; r < r1; r += RK_UNROLL)
    {
      unsigned long long e[RK_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < RK_UNROLL; ++u)
      {
        const uint32_t i = (r + u) * 64 + lane;
        e[u] = (r + u < r1 && i < m) ? src[i] : ~0ull;
      }
#pragma unroll
      for (uint32_t u = 0; u < RK_UNROLL; ++u)
        if (e[u] != ~0ull) atomicAdd(&hist[(uint32_t) (e[u] >> sh) & 255u], 1u);
    }
    __syncthreads();
    // bases: digit-major, wave-minor
    if (tid < 256)
    {
      uint32_t tot = 0;
      for (uint32_t k = 0; k < NW; ++k) tot += lds[k * 256 + tid];
      uint32_t inc = tot;
      for (int d = 1; d < 64; d <<= 1)
      {
        const uint32_t o = __shfl_up(inc, d, 64);
        if ((int) lane >= d) inc += o;
      }
      if (lane == 63) wcnt[w] = inc;
      // (tid < 256 = the first four waves: they meet at the barrier below with everybody)
      lds[NW * 256 + tid] = inc - tot;  // exclusive inside the wave
    }
    __syncthreads();
    if (tid < 256)
    {
      uint32_t base = lds[NW * 256 + tid];
      for (uint32_t k = 0; k < w; ++k) base += wcnt[k];
      for (uint32_t k = 0; k < NW; ++k)
      {
        const uint32_t c = lds[k * 256 + tid];
        lds[k * 256 + tid] = base;
        base += c;
      }
    }
    __syncthreads();
    for (uint32_t r = r0; r < r1; r += RK_UNROLL)
    {
      unsigned long long e[RK_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < RK_UNROLL; ++u)
      {
        const uint32_t i = (r + u) * 64 + lane;
        e[u] = (r + u < r1 && i < m) ? src[i] : ~0ull;
      }
#pragma unroll
      for (uint32_t u = 0; u < RK_UNROLL; ++u)
      {
        const bool valid = e[u] != ~0ull;
        const uint32_t d = (uint32_t) (e[u] >> sh) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit)
        {
          const bool mine = (d >> bit) & 1u;
          const unsigned long long bal = __ballot(mine);
          peers &= mine ? bal : ~bal;
        }
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t) (peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) peers, 0u));
        const uint32_t base = valid ? hist[d] : 0u;
        if (valid) dst[base + before] = e[u];
        if (valid && before == 0) hist[d] = base + (uint32_t) __popcll(peers);  // (one lane per digit of the row; the wave's LDS operations stay in order)
      }
    }
    __syncthreads();
    unsigned long long *t = src;
    src = dst;
    dst = t;
  }
  // src: sorted by key, equal keys in position order.  rank = number of key changes in front of the entry
  uint32_t changes = 0;
  for (uint32_t r = r0; r < r1; ++r)
  {
    const uint32_t i = r * 64 + lane;
    const bool ch = i < m && i > 0 && (src[i] >> 16) != (src[i - 1] >> 16);
    changes += (uint32_t) __popcll(__ballot(ch));
  }
  if (lane == 0) wcnt[w] = changes;
  __syncthreads();
  uint32_t run = 0;
  for (uint32_t k = 0; k < w; ++k) run += wcnt[k];
  __syncthreads();  // (wcnt is read; the caller's LDS may be overwritten from here on)
  for (uint32_t r = r0; r < r1; r += RK_UNROLL)
  {
    unsigned long long e[RK_UNROLL], ep[RK_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < RK_UNROLL; ++u)
    {
      const uint32_t i = (r + u) * 64 + lane;
      const bool in = r + u < r1 && i < m;
      e[u] = in ? src[i] : ~0ull;
      ep[u] = in && i > 0 ? src[i - 1] : ~0ull;
    }
#pragma unroll
    for (uint32_t u = 0; u < RK_UNROLL; ++u)
    {
      const bool valid = e[u] != ~0ull;
      const bool ch = valid && ep[u] != ~0ull && (e[u] >> 16) != (ep[u] >> 16);
      const unsigned long long mk = __ballot(ch);
      const uint32_t upto = __builtin_amdgcn_mbcnt_hi((uint32_t) (mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mk, 0u)) + (ch ? 1u : 0u);
      if (valid)
      {
        const uint32_t pos = (uint32_t) e[u] & 0xFFFFu;
        out[pos] = ((run + upto + 1u) << 16) | pos;
      }
      run += (uint32_t) __popcll(mk);
    }
  }
}
// Who runs a task body: its thread index, its barrier, and what it counts of the tasks it pushes (sortsvc.inc).  WgTeam = the
// whole workgroup (every kernel but k_sort_job; compiles to threadIdx.x and __syncthreads, nothing counted).
struct WgTeam
{
  __device__ __forceinline__ uint32_t tid() const { return threadIdx.x; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ void count_pushes(uint32_t) const {}
};
// WgLive = the whole workgroup, partition and finisher tasks pushed added to *live (the wide workgroups of k_sort_job)
struct WgLive : WgTeam
{
  uint32_t *live;
  __device__ __forceinline__ void count_pushes(uint32_t k) const
  {
    if (k) atomicAdd(live, k);
  }
};
// LdsTeam = four waves (threads base .. base + 255) of a larger workgroup whose other waves do something else: the barrier is an
// arrival counter and a generation word in LDS (the waves of a workgroup are co-resident, so the spin always ends); partition and
// finisher tasks pushed are added to *live (k_sort_job: nothing can arrive any more once that is zero)
struct LdsTeam
{
  uint32_t *bar;  // LDS: [0] arrivals, [1] generation
  uint32_t base;
  uint32_t *live;
  __device__ __forceinline__ uint32_t tid() const { return threadIdx.x - base; }
  __device__ __forceinline__ void sync() const
  {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if ((threadIdx.x & 63u) == 0)
    {
      const uint32_t g = __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (__hip_atomic_fetch_add(bar, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) == 3u)
      {
        __hip_atomic_store(bar, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(bar + 1, g + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      else
        while (__hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == g) __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  __device__ __forceinline__ void count_pushes(uint32_t k) const
  {
    if (k) atomicAdd(live, k);
  }
};

// One heap segment of at most 4096 elements as packed 8-byte entries in LDS (buf): every thread of the team calls this (NT of
// them), the heap itself belongs to its first wave.
template <class T = WgTeam> __device__ __forceinline__ void heap_small_body(const uint32_t first, const uint32_t last, uint32_t *key, uint32_t *idx, hent *buf, const uint32_t NT, const T &team = T())
{
  const uint32_t m = last - first, tid = team.tid();
  uint32_t *gk = key + first, *gx = idx + first;
  for (uint32_t i = tid; i < m; i += NT) buf[i] = ((hent) gk[i] << 32) | gx[i];
  team.sync();
  if (tid < 64)
  {
    LdsMem mem{buf};
    make_heap_wave(mem, m);
    sort_heap_asm<false>(buf, m, 1);
  }
  team.sync();
  for (uint32_t i = tid; i < m; i += NT)
  {
    const hent e = buf[i];
    st_through(gk + i, hkey(e));
    st_through(gx + i, (uint32_t) e);
  }
}
// One heap segment of more than HEAP_BIG_MIN elements by a workgroup of NT threads that owns `dyn`: 4 * (cap32 + 3) bytes of LDS
// (cap32 as wide_lds_split() on the host makes it: odd, and 2 * (cap32 + 1) > HEAP_RANKED_MAX, so that a ranked heap that does not
// fit LDS has nothing but leaves outside it; at least 8 * HEAP_LARGE bytes when segments beyond HEAP_RANKED_MAX elements may come).
// The loads, the ranking and the final gather of a 40 000-element segment are 700 dependent round trips for a lone wave (0.9 ms)
// and a fraction of that for sixteen; the heap itself belongs to wave 0, the other waves sleep at the barriers meanwhile.
__device__ __forceinline__ void heap_big_body(const uint32_t first, const uint32_t last, uint32_t *key, uint32_t *idx, hent *scratch, uint32_t *scratch32, uint32_t *scratch32b,
                                              unsigned long long *rka, unsigned long long *rkb, hent *dyn, const uint32_t cap32, const uint32_t NT)
{
  const uint32_t m = last - first;
  uint32_t *gk = key + first, *gx = idx + first;
  hent *buf = scratch + first;
  const bool w0 = threadIdx.x < 64;  // the wave that owns the heap
  for (uint32_t i = threadIdx.x; i < m; i += NT) buf[i] = ((hent) gk[i] << 32) | gx[i];
  __syncthreads();
  if (m <= HEAP_RANKED_MAX)
  {
    // ranked 4-byte entries ((rank + 1) << 16 | local index, never 0): up to cap32 of them fit LDS (slots 1..m of l32,
    // slot 0 scratch, two zero slots behind).  buf keeps the packed originals; the sorted entries end up in g32.
    const unsigned long long tp0 = wall_clock64();
    uint32_t *l32 = reinterpret_cast<uint32_t *>(dyn);
    uint32_t *g32 = scratch32 + first;
    unsigned long long tp1, tp2, tp3;
    if (m <= cap32)
    {
      wg_ranked_entries(gk, m, rka + first, rkb + first, l32 + 1, l32, l32 + (NT / 64 + 1) * 256, NT);
      __syncthreads();
      if (threadIdx.x < 3) l32[threadIdx.x == 0 ? 0 : m + threadIdx.x] = 0;
      __syncthreads();
      tp1 = wall_clock64();
      {
        LdsMemT<E32> mem{l32 + 1};
        make_heap_block(mem, m, NT);
      }
      tp2 = tp3 = wall_clock64();
      if (w0) sort_heap_lds_q(l32 + 1, m, g32);
    }
    else
    {
      wg_ranked_entries(gk, m, rka + first, rkb + first, g32, l32, l32 + (NT / 64 + 1) * 256, NT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      tp1 = wall_clock64();
      {
        GlbMemT<E32> gmem{g32};
        make_heap_block(gmem, m, NT);
      }
      tp2 = wall_clock64();
      // m <= HEAP_RANKED_MAX < 2 * (cap32 + 1): the upper levels to LDS, the rest (all leaves) to the overflow array; the pops that
      // bring the heap down to the LDS part
      uint32_t *ovf = scratch32b + first;  // ovf[slot], slots cap32 + 1 .. m + 2
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < m; i += NT)
      {
        const uint32_t e = g32[i];
        if (i < cap32) l32[1 + i] = e; else ovf[1 + i] = e;
      }
      if (threadIdx.x < 3) l32[threadIdx.x == 0 ? 0 : cap32 + threadIdx.x] = 0;
      if (threadIdx.x < 2) ovf[m + 1 + threadIdx.x] = 0;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (w0) sort_heap_hybrid(l32 + 1, m, cap32, ovf, g32);
      tp3 = wall_clock64();
      __syncthreads();
      if (w0) sort_heap_lds_q(l32 + 1, cap32, g32);
    }
    __syncthreads();
    if (threadIdx.x == 0) g32[0] = l32[1];  // the last element never leaves the root
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    const unsigned long long tp4 = wall_clock64();
    if (threadIdx.x == 0 && m > 36000)
    {
      g_heap_phase[0] = m;
      g_heap_phase[1] = tp1 - tp0;
      g_heap_phase[2] = tp2 - tp1;
      g_heap_phase[3] = tp3 - tp2;
      g_heap_phase[4] = tp4 - tp3;
    }
    for (uint32_t i = threadIdx.x; i < m; i += NT)
    {
      const hent e = buf[g32[i] & 0xFFFFu];
      st_through(gk + i, hkey(e));
      st_through(gx + i, (uint32_t) e);
    }
    return;
  }
  // beyond the ranked form: heapify and pop in global memory until the heap fits LDS as packed entries, then finish there
  if (w0)
  {
    GlbMem gmem{buf};
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    make_heap_wave(gmem, m);
    sort_heap_asm<true>(buf, m, HEAP_LARGE);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < HEAP_LARGE; i += NT) dyn[i] = buf[i];
  __syncthreads();
  if (w0) sort_heap_asm<false>(dyn, HEAP_LARGE, 1);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < HEAP_LARGE; i += NT) buf[i] = dyn[i];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < m; i += NT)
  {
    const hent e = buf[i];
    st_through(gk + i, hkey(e));
    st_through(gx + i, (uint32_t) e);
  }
}

#include "sortsvc.inc"
}  // namespace

// __final_insertion_sort.  What the introsort loop (and the heapsorts) leave is ordered between segments and arbitrary
// only inside the left-over segments of at most 16 elements, so the stable sort by key is local: every such segment
// lies entirely inside a 32-element window of one of two tilings (offset 0 and offset 16), and a stable sort of every
// window of both tilings sorts the array (a window sort never disturbs what is already in order).  One half-wave per
// window: rank by counting over the 32 elements, (group, key) compared so that windows may straddle groups.
namespace
{
__global__ __launch_bounds__(256) void k_se_window_sort(uint32_t *__restrict__ key, uint32_t *__restrict__ idx, const uint32_t *__restrict__ gof, uint32_t n, uint32_t offset)
{
  const uint32_t lane = threadIdx.x & 63, half = lane & 32u, wl = lane & 31u;
  const uint64_t p = (uint64_t) offset + ((uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + lane;
  unsigned long long k64 = ~0ull;
  uint32_t kk = 0, xx = 0;
  if (p < n)
  {
    kk = key[p];
    xx = idx[p];
    k64 = ((unsigned long long) gof[p] << 32) | kk;
  }
  // already in order (heapsorted stretches, sorted input): nothing to do for this wave
  const unsigned long long prev = __shfl_up(k64, 1, 64);
  if (__ballot(wl != 0 && prev > k64) == 0ull) return;
  uint32_t rank = 0;
#pragma unroll 8
  for (uint32_t j = 0; j < 32; ++j)
  {
    const unsigned long long o = __shfl(k64, (int) (half + j), 64);
    rank += (o < k64 || (o == k64 && j < wl)) ? 1u : 0u;
  }
  if (p < n)
  {
    const uint64_t d = p - wl + rank;  // elements beyond n carry the largest key and rank last
    key[d] = kk;
    idx[d] = xx;
  }
}
}  // namespace

// BK_DEBUG=sortcheck (debugging): is idx still a permutation of 0 .. n-1 and does every element still carry its own key?
// (callers whose idx is not such a permutation must not set it)
__global__ __launch_bounds__(256) void k_chk_count(const uint32_t *__restrict__ idx, uint32_t n, uint32_t *__restrict__ cnt, uint32_t *__restrict__ bad)
{
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint32_t x = idx[p];
  if (x >= n)
  {
    atomicAdd(&bad[0], 1u);
    atomicMin(&bad[2], p);
    return;
  }
  if (atomicAdd(&cnt[x], 1u) != 0u)
  {
    atomicAdd(&bad[1], 1u);
    atomicMin(&bad[3], p);
  }
}
__global__ __launch_bounds__(256) void k_chk_keys(const uint32_t *__restrict__ key, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ key0, uint32_t n, uint32_t *__restrict__ bad)
{
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint32_t x = idx[p];
  if (x < n && key0[x] != key[p])
  {
    atomicAdd(&bad[4], 1u);
    atomicMin(&bad[5], p);
  }
}
static void sort_check(const char *phase, const uint32_t *key, const uint32_t *idx, const uint32_t *key0, uint32_t n, const uint64_t *goff, uint32_t ng, hipStream_t st, SortEmuBufs &b)
{
  uint32_t *c = b.chk_cnt.as<uint32_t>(n), *bd = b.chk_bad.as<uint32_t>(8);
  const uint32_t init[8] = {0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 0, 0};
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemset(c, 0, (size_t) n * 4));
  HIP_CHECK(hipMemcpy(bd, init, 32, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_chk_count, dim3(cdiv(n, 256)), dim3(256), 0, st, idx, n, c, bd);
  hipLaunchKernelGGL(k_chk_keys, dim3(cdiv(n, 256)), dim3(256), 0, st, key, idx, key0, n, bd);
  uint32_t h[8];
  HIP_CHECK(hipMemcpyAsync(h, bd, 32, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  if (h[0] || h[1] || h[4])
  {
    std::vector<uint64_t> go((size_t) ng + 1);
    HIP_CHECK(hipMemcpy(go.data(), goff, ((size_t) ng + 1) * 8, hipMemcpyDeviceToHost));
    auto grp = [&](uint32_t p) { return p == 0xFFFFFFFFu ? -1 : (int) (std::upper_bound(go.begin(), go.end(), (uint64_t) p) - go.begin()) - 1; };
    fprintf(stderr, "[sortemu] CHECK FAILED %s: %u payloads out of range (first at %u), %u duplicated payloads (first at position %u, group %d), %u elements whose key is not their own (first at %u, group %d); n=%u\n",
            phase, h[0], h[2], h[1], h[3], grp(h[3]), h[4], h[5], grp(h[5]), n);
  }
}

// The dynamic LDS of a wide workgroup: all of a CU's 160 KB but the kernel's static LDS, and cap32 = the ranked 4-byte heap entries
// that fit it (+ slot 0 and two zero slots), an odd count.  heap_big_body relies on 2 * (cap32 + 1) > HEAP_RANKED_MAX: every slot of
// a ranked heap that lies outside LDS is then a leaf (sort_heap_hybrid).
struct WideLds
{
  size_t dyn_lds;
  uint32_t cap32;
};
static WideLds wide_lds_split(const void *kernel)
{
  hipFuncAttributes fa;
  HIP_CHECK(hipFuncGetAttributes(&fa, kernel));
  WideLds w;
  w.dyn_lds = (size_t) ((160u * 1024u - (uint32_t) fa.sharedSizeBytes) & ~15u);
  w.cap32 = (uint32_t) (w.dyn_lds / 4 - 3);
  if ((w.cap32 & 1u) == 0) --w.cap32;
  if ((w.cap32 & 1u) == 0 || 2ull * (w.cap32 + 1ull) <= HEAP_RANKED_MAX)
    throw bk_error(BK_ERR_HIP, "sort: " + std::to_string(fa.sharedSizeBytes) + " bytes of static LDS leave too little for the ranked heaps");
  return w;
}

// ---- the resident sort service (sortsvc.inc), host side -----------------------------------------------------------------------
static SvcParams svc_params(SortService &S)
{
  SvcParams P;
  uint32_t *ctl = S.ctl.get<uint32_t>();
  for (int k = 0; k < 2; ++k)
  {
    P.q[k].head = ctl + 64 * k;
    P.q[k].tail = ctl + 64 * k + 32;
    P.q[k].slots = S.slots[k].get<SvcTask>();
    P.q[k].seq = S.seq[k].get<uint32_t>();
    P.q[k].mask = S.cap[k] - 1;
    P.q[k].release = 1u;  // an agent-scope release in front of every push (sortsvc.inc, visibility)
  }
  P.error = ctl + 128;
  P.stats = ctl + 160;
  P.jobs = S.jobs.get<SvcJob>();
  P.quit_d = ctl + 192;
  P.host = S.quit_dev;
  P.cap32 = S.cap32;
  P.quit_word = S.quit_word;
  P.dbg = S.dbg.get<uint32_t>();
  for (int k = 0; k < 2; ++k)
  {
    P.pos[k] = S.pos[k].get<uint32_t>();
    P.pos_cap[k] = S.pos_cap[k];
  }
  P.timeout_ticks = SVC_TIMEOUT_TICKS;
  return P;
}
void SortService::start(uint64_t n_bound, uint64_t max_group, hipStream_t after)
{
  if (running) return;
  quit_stream = after;  // (a stream of the stage that the stage probes: the word that ends the service is written by a kernel on it)
  int dev = 0, cus = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  // a quarter of the CUs to the wide workgroups (each takes a whole CU's LDS), two narrow ones on each of the others
  const int n_wide = std::min(1024, std::max(4, cus / 4));
  const int n_narrow = std::max(8, 2 * (cus - n_wide));
  if (!quit_host)
  {
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&quit_host), SVC_H_WORDS * 4, hipHostMallocMapped));  // SvcParams::host
    HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void **>(&quit_dev), quit_host, 0));
    for (int k = 0; k < 2; ++k) HIP_CHECK(hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&st_copy, hipStreamNonBlocking));
    const WideLds w = wide_lds_split(reinterpret_cast<const void *>(k_sort_service<true>));
    wide_lds = w.dyn_lds;
    cap32 = w.cap32;
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sort_service<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) wide_lds));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sort_service<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) SVC_NARROW_LDS));
  }
  // rings: every live segment holds more than 16 elements; the wide ring only sees segments above HEAP_BIG_MIN elements
  auto pow2 = [](uint64_t v) {
    uint32_t c = 1024;
    while (c < v && c < (1u << 30)) c <<= 1;
    return c;
  };
  cap[0] = pow2(n_bound / HEAP_BIG_MIN + 4096);
  cap[1] = pow2(n_bound / 16 + 4096);
  (void) ctl.as<uint32_t>(256);
  for (int k = 0; k < 2; ++k)
  {
    (void) slots[k].as<SvcTask>(cap[k]);
    (void) seq[k].as<uint32_t>(cap[k]);
  }
  (void) jobs.as<SvcJob>(SVC_MAX_JOBS);
  // every workgroup's own position lists (two per partition node): a wide one may be handed a whole group, a narrow one a node
  // of at most SVC_WIDE_MIN elements
  pos_cap[0] = (uint32_t) std::max<uint64_t>(max_group, SVC_WIDE_MIN) + 64;
  pos_cap[1] = SVC_WIDE_MIN + 64;
  (void) pos[0].as<uint32_t>(2ull * pos_cap[0] * (uint64_t) n_wide);
  (void) pos[1].as<uint32_t>(2ull * pos_cap[1] * (uint64_t) n_narrow);
  if (bk_debug("svc"))
  {
    (void) dbg.as<uint32_t>(12 * 8192 + 48);
    HIP_CHECK(hipMemsetAsync(dbg.p, 0, (12 * 8192 + 48) * 4, after));
  }
  __atomic_store_n(quit_host, 0u, __ATOMIC_SEQ_CST);
  quit_word = 0xC0DE0000u | (++starts & 0xFFFFu);
  for (uint32_t k = 1; k < SVC_H_WORDS; ++k) quit_host[k] = 0u;
  next_slot = 0;
  const SvcParams P = svc_params(*this);
  hipLaunchKernelGGL(k_svc_reset, dim3(cdiv(std::max(cap[0], cap[1]), 256)), dim3(256), 0, after, P);
  HIP_CHECK(hipStreamSynchronize(after));
  DeferredFrees::begin();
  running = true;
  hipLaunchKernelGGL(k_sort_service<true>, dim3(n_wide), dim3(1024), wide_lds, st[0], P);
  HIP_CHECK(hipGetLastError());
  // a wide workgroup needs a CU to itself: the narrow ones, which fit anywhere, are only launched when every wide one has its CU
  // (the other way round they could sit on every CU and keep the wide ones out for good)
  {
    const auto t0 = std::chrono::steady_clock::now();
    volatile uint32_t *started = quit_host + SVC_H_STARTED;
    for (;;)
    {
      int have = 0;
      for (int k = 0; k < n_wide; ++k) have += started[k] != 0u;
      if (have == n_wide) break;
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.25) break;  // (a busy device: the rest start when CUs free up)
    }
  }
  hipLaunchKernelGGL(k_sort_service<false>, dim3(n_narrow), dim3(256), SVC_NARROW_LDS, st[1], P);
  HIP_CHECK(hipGetLastError());
}
bool SortService::narrow_running(double seconds) const
{
  const auto t0 = std::chrono::steady_clock::now();
  volatile const uint32_t *flag = quit_host + SVC_H_NARROW;
  while (*flag == 0u)
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) return false;
  return true;
}
void SortService::stop()
{
  if (!running) return;
  running = false;
  // the word that ends the service, two ways: a kernel on a stream of the stage (the stage has probed it) and a copy from page-locked
  // memory on a stream of its own (a DMA engine's business, not a compute queue's) - whichever arrives first; a stage that gives
  // the service up BECAUSE one of its streams sits behind a persistent kernel's queue must not wait for that very stream
  __atomic_store_n(quit_host, quit_word, __ATOMIC_SEQ_CST);
  (void) hipMemcpyAsync(ctl.get<uint32_t>() + 192, quit_host, 4, hipMemcpyHostToDevice, st_copy);
  hipLaunchKernelGGL(k_svc_quit, dim3(1), dim3(1), 0, quit_stream, ctl.get<uint32_t>() + 192, quit_word);
  HIP_CHECK(hipStreamSynchronize(st[0]));
  HIP_CHECK(hipStreamSynchronize(st[1]));
  uint32_t h[40] = {};
  HIP_CHECK(hipMemcpy(h, ctl.get<uint32_t>() + 128, sizeof h, hipMemcpyDeviceToHost));
  for (int k = 0; k < 8; ++k) stats[k] = h[32 + k];
  DeferredFrees::end();
  if (bk_debug("svc"))
  {
    uint32_t c[128] = {};
    SvcJob j0 = {};
    HIP_CHECK(hipMemcpy(c, ctl.get<uint32_t>(), sizeof c, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(&j0, jobs.get<SvcJob>(), sizeof j0, hipMemcpyDeviceToHost));
    if (dbg.p)
    {
      std::vector<uint32_t> d(12 * 8192 + 48);
      HIP_CHECK(hipMemcpy(d.data(), dbg.p, d.size() * 4, hipMemcpyDeviceToHost));
      {
        const uint32_t *ph = d.data() + 12 * 8192 + 32;
        const double lv = ph[7] ? (double) ph[7] : 1.0;
        fprintf(stderr, "[svc]   wide partition nodes: %u levels; per level: count pass %.2f us, place pass %.2f us, swaps + drain %.2f us, cut, release, pushes and the next pivot %.2f us\n", ph[7], ph[0] * 1e-2 / lv,
                ph[1] * 1e-2 / lv, ph[2] * 1e-2 / lv, ph[3] * 1e-2 / lv);
      }
      for (int kind = 0; kind < 2; ++kind)
      {
        fprintf(stderr, "[svc]   %s tasks by size (2^k ..):", kind ? "narrow heap" : "finisher");
        for (int k = 4; k < 13; ++k) fprintf(stderr, " %d:%u", k, d[12 * 8192 + 16 * kind + k]);
        fprintf(stderr, "\n");
      }
      for (int kind = 0; kind < 2; ++kind)
      {
        // the workgroups' own accounts: time waiting and inside tasks by type (sums over the workgroups, ms), the longest task
        const uint32_t nw = kind == 0 ? stats[2] : stats[3];
        double sum[8] = {};
        uint32_t longest = 0;
        for (uint32_t w = 0; w < nw && w < 4096; ++w)
        {
          const uint32_t *a = d.data() + 4 * 8192 + 8 * (w + 4096 * kind);
          for (int k = 0; k < 7; ++k) sum[k] += a[k];
          longest = std::max(longest, a[7]);
        }
        fprintf(stderr, "[svc]   %s workgroups (%u): waiting %.2f ms; partition nodes %.0f in %.2f ms, finisher %.0f in %.2f ms, heaps %.0f in %.2f ms (sums over the workgroups); longest task %.3f ms\n", kind ? "narrow" : "wide", nw,
                sum[0] * 1e-5, sum[4], sum[1] * 1e-5, sum[5], sum[2] * 1e-5, sum[6], sum[3] * 1e-5, longest * 1e-5);
        std::map<uint32_t, int> hist;
        const uint32_t n = kind == 0 ? stats[2] : stats[3];
        for (uint32_t w = 0; w < n && w < 4096; ++w) hist[d[4 * (w + 4096 * kind)]]++;
        fprintf(stderr, "[svc]   %s workgroups by last state (1 polling, 5 took a task, 9 left):", kind ? "narrow" : "wide");
        for (auto &kv : hist) fprintf(stderr, " %u:%d", kv.first, kv.second);
        fprintf(stderr, "; first ones (state, polls, time of the last poll in 10 ns, how it left 6 error 7 quit 8 timeout):");
        for (uint32_t w = 0; w < 6 && w < n; ++w) fprintf(stderr, " [%u %u %u %u]", d[4 * (w + 4096 * kind)], d[4 * (w + 4096 * kind) + 1], d[4 * (w + 4096 * kind) + 2], d[4 * (w + 4096 * kind) + 3]);
        fprintf(stderr, "\n");
      }
    }
    uint32_t sq[4] = {};
    HIP_CHECK(hipMemcpy(sq, seq[1].get<uint32_t>(), sizeof sq, hipMemcpyDeviceToHost));
    fprintf(stderr, "[svc] tasks %u wide / %u narrow; workgroups started %u / %u, left on their own %u / %u, odd quit words read %u; error %u; wide queue head %u tail %u, narrow queue head %u tail %u (seq %u %u %u %u); job 0: remaining %u done %u heaps %u (longest %u)\n",
            stats[0], stats[1], stats[2], stats[3], stats[4], stats[5], stats[6], h[0], c[0], c[32], c[64], c[96], sq[0], sq[1], sq[2], sq[3], j0.remaining, j0.done, j0.n_heap, j0.max_heap);
  }
  if (h[0]) throw bk_error(h[0] & 2u ? BK_ERR_LIMIT : BK_ERR_HIP, "sort service: task error " + std::to_string(h[0]) + " (2 = ring overflow, 4 = a job timed out, 8 = a cut outside its segment, 16 = a task in the wrong queue, 32 = a node beyond the position lists, 64 = the finisher); first failing task: code " + std::to_string(h[8]) + ", " + std::to_string(h[9]) + " " + std::to_string(h[10]) + " " + std::to_string(h[11]));
}
SortService::~SortService()
{
  if (running)
  {
    running = false;
    if (quit_host && st_copy)
    {
      __atomic_store_n(quit_host, quit_word, __ATOMIC_SEQ_CST);
      (void) hipMemcpyAsync(ctl.get<uint32_t>() + 192, quit_host, 4, hipMemcpyHostToDevice, st_copy);
    }
    if (quit_stream) hipLaunchKernelGGL(k_svc_quit, dim3(1), dim3(1), 0, quit_stream, ctl.get<uint32_t>() + 192, quit_word);
    for (int k = 0; k < 2; ++k)
      if (st[k]) (void) hipStreamSynchronize(st[k]);
    DeferredFrees::end();
  }
  for (int k = 0; k < 2; ++k)
    if (st[k]) (void) hipStreamDestroy(st[k]);
  if (st_copy) (void) hipStreamDestroy(st_copy);
  if (quit_host) (void) hipHostFree(quit_host);
}

static void window_sorts(uint32_t *key, uint32_t *idx, const uint32_t *gof, uint32_t n, hipStream_t st);

// the sort as ONE job of the resident service: submit, wait (both on the caller's stream), then the insertion sort's windows
static void std_sort_groups_svc(uint32_t *key, uint32_t *idx, const uint32_t *gof, const uint64_t *goff, uint32_t ng, uint32_t n, SortEmuBufs &b, hipStream_t st)
{
  SortService &S = *b.svc;
  if (b.svc_slot == 0xFFFFFFFFu)
  {
    b.svc_slot = S.new_slot();
    if (b.svc_slot >= SVC_MAX_JOBS) throw bk_error(BK_ERR_LIMIT, "sort service: more than 64 callers");
  }
  SvcJob d = {};
  d.key = key;
  d.idx = idx;
  d.hscratch = b.heap_scratch.as<hent>((uint64_t) n + HEAP_PAD);
  d.scratch32 = b.scratch32.as<uint32_t>((uint64_t) n + HEAP_PAD);
  d.scratch32b = b.scratch32b.as<uint32_t>((uint64_t) n + HEAP_PAD);
  d.rka = b.rk_a.as<unsigned long long>((uint64_t) n + HEAP_PAD);
  d.rkb = b.rk_b.as<unsigned long long>((uint64_t) n + HEAP_PAD);
  d.epoch = (b.svc_epoch++ % 0xFFFFFu) + 1u;  // (never 0)
  const SvcParams P = svc_params(S);
  hipLaunchKernelGGL(k_svc_submit, dim3(1), dim3(256), 0, st, P, d, b.svc_slot, goff, ng);
  HIP_CHECK(hipGetLastError());
  // The caller's thread waits, not its stream: a kernel that spins on the stream until the job is done keeps the stream's hardware
  // queue busy, and the command processor serves the other queues' dependent launches the slower the more queues hold a running
  // kernel (twelve lanes' wait kernels: 21 us per dependent launch against 3, tools/ubench/beside.hip - the lanes' ~160 other
  // kernels then cost more than their sorts).
  {
    volatile const uint32_t *done = S.quit_host + SVC_H_DONE + b.svc_slot, *err = S.quit_host + SVC_H_ERROR;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; *done != d.epoch; ++spins)
    {
      if (*err != 0u)
        throw bk_error(BK_ERR_HIP, "sort service: a task failed (error " + std::to_string(*err) + "; first failing task: code " + std::to_string(err[1]) + ", " + std::to_string(err[2]) + " " + std::to_string(err[3]) + " " + std::to_string(err[4]) + ")");
      if ((spins & 1023u) == 1023u)
      {
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 20.0) throw bk_error(BK_ERR_HIP, "sort service: a job did not finish");
        std::this_thread::yield();
      }
      else
        __builtin_ia32_pause();
    }
  }
  if (bk_debug("svc"))
  {
    SvcJob j;
    HIP_CHECK(hipMemcpy(&j, S.jobs.get<SvcJob>() + b.svc_slot, sizeof j, hipMemcpyDeviceToHost));
    fprintf(stderr, "[svc] slot %u sort %u: %u elements in %u groups; partitions and finisher done after %.3f ms, job after %.3f ms; %u elements in heaps, the longest %u, the heap that ended last %u elements in %.3f ms\n", b.svc_slot,
            b.svc_epoch, n, ng, (double) (j.t_parts - j.t_submit) * 1e-5, (double) (j.t_done - j.t_submit) * 1e-5, j.n_heap, j.max_heap, (uint32_t) j.last_heap, (double) (j.last_heap >> 32) * 1e-5);
  }
  window_sorts(key, idx, gof, n, st);
}

// the sort as ONE task dispatch on the caller's stream (sortsvc.inc, k_sort_job): the caller's own queues and job, seeded with the
// root partition nodes of every group; then the insertion sort's windows and ONE look of the host at the job's error word (and at
// the groups' longest heaps when the caller observes them)
static void std_sort_groups_tasks(uint32_t *key, uint32_t *idx, const uint32_t *gof, const uint64_t *goff, uint32_t ng, uint32_t n, SortEmuBufs &b, hipStream_t st, const uint32_t *key0)
{
  static size_t dyn_lds = 0;
  static uint32_t cap32 = 0;
  static std::once_flag once;
  std::call_once(once, [] {
    const WideLds w = wide_lds_split(reinterpret_cast<const void *>(k_sort_job));
    dyn_lds = w.dyn_lds;
    cap32 = w.cap32;
    if (dyn_lds < SJ_TEAMS * SJ_TEAM_LDS) throw bk_error(BK_ERR_HIP, "k_sort_job: the narrow teams do not fit the LDS");
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sort_job), hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn_lds));
  });
  // the largest group sizes the wide workgroups' position lists (a wide one may be handed a whole group)
  std::vector<uint64_t> go((size_t) ng + 1);
  HIP_CHECK(hipMemcpyAsync(go.data(), goff, go.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  uint64_t max_group = 0;
  for (uint32_t g = 0; g < ng; ++g) max_group = std::max<uint64_t>(max_group, go[g + 1] - go[g]);
  // the grid: bounded, so that three lanes' dispatches and their other kernels share the device (a workgroup holds a CU's LDS)
  const uint32_t n_wide = std::min<uint32_t>(SJ_MAX_WIDE, std::max<uint32_t>(1, cdiv(n, 1u << 16)));
  const uint32_t n_narrow = std::min<uint32_t>(SJ_MAX_NARROW, std::max<uint32_t>(1, cdiv(n, 1u << 16)));
  SjParams S = {};
  SvcParams &P = S.P;
  {
    auto pow2 = [](uint64_t v) {
      uint32_t c = 1024;
      while (c < v && c < (1u << 30)) c <<= 1;
      return c;
    };
    // rings as the service sizes them: every live segment holds more than 16 elements, the wide ring only sees those above HEAP_BIG_MIN
    const uint32_t want[2] = {pow2((uint64_t) n / HEAP_BIG_MIN + 4096), pow2((uint64_t) n / 16 + 4096)};
    for (int k = 0; k < 2; ++k)
      if (want[k] > b.tj_cap[k])
      {
        b.tj_cap[k] = want[k];
        b.tj_ready = false;
      }
    uint32_t *ctl = b.tj_ctl.as<uint32_t>(SJ_C_WORDS);
    for (int k = 0; k < 2; ++k)
    {
      P.q[k].head = ctl + 64 * k;
      P.q[k].tail = ctl + 64 * k + 32;
      P.q[k].slots = b.tj_slots[k].as<SvcTask>(b.tj_cap[k]);
      P.q[k].seq = b.tj_seq[k].as<uint32_t>(b.tj_cap[k]);
      P.q[k].mask = b.tj_cap[k] - 1;
      P.q[k].release = 1u;  // an agent-scope release in front of every push (sortsvc.inc, visibility)
    }
    P.error = ctl + SJ_C_ERROR;
    P.stats = ctl + SJ_C_STATS;
    P.quit_d = ctl + SJ_C_QUIT;
    P.host = ctl + SJ_C_HOST;
    P.jobs = b.tj_jobs.as<SvcJob>(SVC_MAX_JOBS);  // (k_svc_reset clears SVC_MAX_JOBS of them; this caller's job is slot 0)
    P.cap32 = cap32;
    P.quit_word = 0u;
    P.timeout_ticks = SJ_TIMEOUT_TICKS;
    P.pos_cap[0] = (uint32_t) std::max<uint64_t>(max_group, SVC_WIDE_MIN) + 64;
    P.pos_cap[1] = SVC_WIDE_MIN + 64;
    P.pos[0] = b.tj_pos[0].as<uint32_t>(2ull * P.pos_cap[0] * n_wide);
    P.pos[1] = b.tj_pos[1].as<uint32_t>(2ull * P.pos_cap[1] * n_narrow * SJ_TEAMS);
    P.dbg = nullptr;
    S.n_wide = n_wide;
    S.live = ctl + SJ_C_LIVE;
    S.gof = gof;
    S.heavy_min = b.heavy_all ? FIN_MAX : HEAP_RANKED_MIN;
    if (b.heavy)
    {
      S.heavy = b.tj_heavy.as<uint32_t>(ng);
      HIP_CHECK(hipMemsetAsync(S.heavy, 0, (size_t) ng * 4, st));
    }
  }
  static const bool dbg = bk_debug("svc");
  if (dbg) S.trace = b.tj_trace.as<unsigned long long>(8);
  if (!b.tj_ready)
  {
    HIP_CHECK(hipMemsetAsync(b.tj_ctl.p, 0, SJ_C_WORDS * 4, st));
    hipLaunchKernelGGL(k_svc_reset, dim3(cdiv(std::max(b.tj_cap[0], b.tj_cap[1]), 256)), dim3(256), 0, st, P);
    b.tj_ready = true;
  }
  SvcJob d = {};
  d.key = key;
  d.idx = idx;
  d.hscratch = b.heap_scratch.as<hent>((uint64_t) n + HEAP_PAD);
  d.scratch32 = b.scratch32.as<uint32_t>((uint64_t) n + HEAP_PAD);
  d.scratch32b = b.scratch32b.as<uint32_t>((uint64_t) n + HEAP_PAD);
  d.rka = b.rk_a.as<unsigned long long>((uint64_t) n + HEAP_PAD);
  d.rkb = b.rk_b.as<unsigned long long>((uint64_t) n + HEAP_PAD);
  d.epoch = (b.tj_epoch++ % 0xFFFFFu) + 1u;  // (never 0)
  const SvcJobLds J = {d.key, d.idx, nullptr, nullptr, d.hscratch, d.scratch32, d.scratch32b, d.rka, d.rkb, P.jobs, d.epoch << 8};
  hipLaunchKernelGGL(k_sort_job_submit, dim3(1), dim3(256), 0, st, S, d, goff, ng);
  hipLaunchKernelGGL(k_sort_job, dim3(n_wide + n_narrow), dim3(1024), dyn_lds, st, S, J);
  HIP_CHECK(hipGetLastError());
  ++b.sorts[1];
  // the job's state: error words, and what the caller observes (the window sorts behind do not change it)
  if (key0) sort_check("after the task dispatch", key, idx, key0, n, goff, ng, st, b);
  window_sorts(key, idx, gof, n, st);
  uint32_t h[16] = {};
  HIP_CHECK(hipMemcpyAsync(h, P.error, 12 * 4, hipMemcpyDeviceToHost, st));
  std::vector<uint32_t> hv;
  if (S.heavy)
  {
    hv.resize(ng);
    HIP_CHECK(hipMemcpyAsync(hv.data(), S.heavy, (size_t) ng * 4, hipMemcpyDeviceToHost, st));
  }
  unsigned long long tr[8] = {};
  if (S.trace) HIP_CHECK(hipMemcpyAsync(tr, S.trace, 5 * 8, hipMemcpyDeviceToHost, st));
  SvcJob j = {};
  HIP_CHECK(hipMemcpyAsync(&j, P.jobs, sizeof j, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  b.last_heap[0] = j.max_heap;
  b.last_heap[1] = j.n_heap;
  if (h[0] || j.remaining != 0u)
  {
    b.tj_ready = false;  // (tasks may be left in the rings: initialised again before the next sort)
    throw bk_error(h[0] & 2u ? BK_ERR_LIMIT : BK_ERR_HIP, "sort task dispatch: task error " + std::to_string(h[0]) + " (2 = ring overflow, 4 = no progress for 1 s, 8 = a cut outside its segment, 16 = a task in the wrong queue, 32 = a node beyond the position lists, 64 = the finisher), " + std::to_string(j.remaining) + " elements not final; first failing task: code " + std::to_string(h[8]) + ", " + std::to_string(h[9]) + " " + std::to_string(h[10]) + " " + std::to_string(h[11]));
  }
  if (S.heavy)
  {
    if (b.heavy->size() < ng) b.heavy->resize(ng, 0u);
    for (uint32_t g = 0; g < ng; ++g) (*b.heavy)[g] = std::max((*b.heavy)[g], hv[g]);
  }
  if (S.trace)
  {
    // (tools/task_dispatch_heap_waits.py reads these lines)
    const double t0 = (double) tr[0];
    const uint32_t hm = (uint32_t) (tr[1] >> 40);
    const unsigned long long hs = tr[1] & 0xFFFFFFFFFFull, base = tr[0] & ~0xFFFFFFFFFFull;
    unsigned long long hstart = base | hs;
    if (hstart < tr[0]) hstart += 1ull << 40;
    fprintf(stderr, "[svc] task dispatch %u: %u elements in %u groups on %u wide + %u narrow workgroups; longest heap %u elements started %.3f ms after the dispatch and took %.3f ms; partitions and finisher done after %.3f ms, job after %.3f ms; %u elements in heaps, the longest %u\n",
            d.epoch, n, ng, n_wide, n_narrow, hm, hm ? ((double) hstart - t0) * 1e-5 : 0.0, hm ? (double) (tr[2] & 0xFFFFFFFFFFull) * 1e-5 : 0.0, tr[3] ? ((double) tr[3] - t0) * 1e-5 : 0.0, ((double) tr[4] - t0) * 1e-5, j.n_heap, j.max_heap);
  }
}

void std_sort_groups(uint32_t *key, uint32_t *idx, const uint32_t *gof, const uint64_t *goff, uint32_t ng, uint64_t n64, SortEmuBufs &b, hipStream_t st)
{
  if (n64 == 0 || ng == 0) return;
  if (n64 > 0x7FFFFFF0ull) throw bk_error(BK_ERR_LIMIT, "std_sort_groups: more than 2^31 pairs");
  const uint32_t n = (uint32_t) n64;
  if (b.svc && b.svc->running)
  {
    ++b.sorts[0];
    b.last_heap[0] = b.last_heap[1] = 0xFFFFFFFFu;  // (the service's job is not read back)
    std_sort_groups_svc(key, idx, gof, goff, ng, n, b, st);
    return;
  }
  static const bool chk = bk_debug("sortcheck");
  DevBuf &chk_key0 = b.chk_key0;  // (BK_DEBUG=sortcheck: per buffer set, i.e. per lane and device)
  uint32_t *key0 = nullptr;
  if (chk)
  {
    // key0[idx] = the key that belongs to payload idx (as the sort receives them)
    key0 = chk_key0.as<uint32_t>(n);
    std::vector<uint32_t> hk(n), hx(n), k0(n);
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipMemcpy(hk.data(), key, (size_t) n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hx.data(), idx, (size_t) n * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i)
      if (hx[i] < n) k0[hx[i]] = hk[i];
    HIP_CHECK(hipMemcpy(key0, k0.data(), (size_t) n * 4, hipMemcpyHostToDevice));
    sort_check("at entry", key, idx, key0, n, goff, ng, st, b);
  }
  if (const char *dump = getenv("BK_DEBUG_SORT_DUMP"))
  {
    // keys and group offsets as they arrive at this sort (debugging aid): <dump>.<call>.keys.u32 / .goff.u64, first 5 calls
    static int call = 0;
    if (call < 5)
    {
      std::vector<uint64_t> go((size_t) ng + 1);
      std::vector<uint32_t> kk(n);
      HIP_CHECK(hipStreamSynchronize(st));
      HIP_CHECK(hipMemcpy(go.data(), goff, ((size_t) ng + 1) * 8, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(kk.data(), key, (size_t) n * 4, hipMemcpyDeviceToHost));
      char name[512];
      snprintf(name, sizeof name, "%s.%d.keys.u32", dump, call);
      if (FILE *f = fopen(name, "wb"))
      {
        fwrite(kk.data(), 4, kk.size(), f);
        fclose(f);
      }
      snprintf(name, sizeof name, "%s.%d.goff.u64", dump, call);
      if (FILE *f = fopen(name, "wb"))
      {
        fwrite(go.data(), 8, go.size(), f);
        fclose(f);
      }
    }
    ++call;
  }
  std_sort_groups_tasks(key, idx, gof, goff, ng, n, b, st, chk ? key0 : nullptr);
}
void std_sort_info(uint64_t out[SORT_INFO_WORDS])
{
  const uint64_t c[SORT_INFO_WORDS] = {FIN_MAX, HEAP_BIG_MIN, HEAP_RANKED_MAX, HEAP_LARGE, SVC_WIDE_MIN, F2_HB, F2_EXT, HEAP_PAD, SJ_MAX_WIDE, SJ_MAX_NARROW,
                                       wide_lds_split(reinterpret_cast<const void *>(k_sort_job)).cap32};
  std::copy(c, c + SORT_INFO_WORDS, out);
}
static void window_sorts(uint32_t *key, uint32_t *idx, const uint32_t *gof, uint32_t n, hipStream_t st)
{
  hipLaunchKernelGGL(k_se_window_sort, dim3(cdiv(n, 256)), dim3(256), 0, st, key, idx, gof, n, 0u);
  if (n > 16) hipLaunchKernelGGL(k_se_window_sort, dim3(cdiv(n - 16, 256)), dim3(256), 0, st, key, idx, gof, n, 16u);
}
