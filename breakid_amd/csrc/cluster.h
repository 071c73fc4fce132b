// Interface of cluster.hip (isolated-pair masking + fast clustering) and ahc.hip.
#pragma once
#include "bk_common.h"
#include "prims.h"
#include "sortemu.h"

// The chain-following kernels of the fast clustering (cluster.hip: k_fw_exit, k_fw_chain, k_fw_mark) work on tiles of FW_TILE
// positions with FW_LEVELS rounds of pointer doubling in LDS.  2^FW_LEVELS >= FW_TILE must hold, and at 1024 / 10 it holds with
// nothing to spare:
//   k_fw_exit  starts one hop along the chain and doubles FW_LEVELS times: 2^FW_LEVELS hops.  A tile whose every nxt[p] = p + 1
//              (one-element windows throughout) needs FW_TILE hops to leave from its first position.
//   k_fw_mark  spreads a seed over 2^(FW_LEVELS-1) + ... + 2 + 1 = 2^FW_LEVELS - 1 hops: from local position 0 to FW_TILE - 1.
// With the bound k_fw_chain makes at most one hop per tile and k_fw_mark reaches the whole tile from any seed, whatever k_fw_exit
// returns.  Below it the marks would only be complete while every exit is EXACTLY 2^FW_LEVELS hops along (seeds 2^FW_LEVELS anchors
// apart, each spread over 2^FW_LEVELS - 1), and k_fw_exit does not promise that: its rounds read entries that their owners may
// already have moved on, so an exit can lie further along the chain.
// (FW_TILE is also the workgroup size of both kernels, and local positions are uint16 with 0xFFFF = "leaves the tile".)
constexpr uint32_t FW_TILE = 1024, FW_LEVELS = 10;
static_assert((1ull << FW_LEVELS) >= FW_TILE, "k_fw_exit / k_fw_mark: FW_LEVELS rounds of doubling must cover a tile of one-element windows");
static_assert(FW_LEVELS < 32 && FW_TILE <= 1024 && FW_TILE < 0xFFFFu, "FW_TILE is a workgroup size and its positions are uint16");

// an ordered list of pair-table indices partitioned into groups
struct PairList
{
  uint64_t n = 0;
  uint32_t ng = 0;
  DevBuf idx;   // u32[n]   index into the pair table
  DevBuf gof;   // u32[n]   group (numeric key order) of each element
  DevBuf goff;  // u64[ng+1]
  uint64_t total(hipStream_t st) const;
};

struct ClusterBufs
{
  // observers for the lanes of lanes.hip (host, may stay empty): the longest heapsort segment of every group in the sorts by x / by y
  std::vector<uint32_t> heavy_x, heavy_y;
  bool observe = false;
  // upper bound on the pairs of any one group (host; 0 = unknown): the anchored-window passes need log2 of it pointer-jumping levels
  uint64_t max_group_bound = 0;
  DevBuf key, perm, tmp, cnt, off, off2, idx2, gof2, goff2, jump, mark, apos, kid, kprev2, k1, k2, pk, knum, clfull, small, scan_tmp;
  SortEmuBufs se;
  prims::RadixBufs radix;
};

// remove_isolated_pairs for every group; L receives the surviving list (x-sorted, duplicates included)
void remove_isolated_all(const bk_pair *pairs, const uint32_t *gof0, const uint64_t *gstart, uint32_t ng, uint64_t n, double w, PairList &L, ClusterBufs &b, hipStream_t st,
                         const uint32_t *drop_group = nullptr);  // drop_group[g] != 0: group g is left to another rank
// the same in two parts, so that a caller may redistribute the groups between them: through the second mask / the third sort
// (gstart_host + keep_host given: the list is built straight from the ranges of the kept groups instead of filtering all n pairs)
void remove_isolated_begin(const bk_pair *pairs, const uint32_t *gof0, const uint64_t *gstart, uint32_t ng, uint64_t n, double w, PairList &L, ClusterBufs &b, hipStream_t st,
                           const uint32_t *drop_group = nullptr, const uint64_t *gstart_host = nullptr, const uint8_t *keep_host = nullptr);
void remove_isolated_end(const bk_pair *pairs, PairList &L, ClusterBufs &b, hipStream_t st);
// dst = the groups of src with keep_host[g] != 0 (offsets for all groups are kept); src_goff_host = src's offsets; one launch
void list_subset_ranges(const PairList &src, const uint64_t *src_goff_host, const uint8_t *keep_host, PairList &dst, hipStream_t st);
// removes the groups that keep fewer than 2 pairs (they are not clustered, BreakID.cc:125)
void drop_small_groups(PairList &L, ClusterBufs &b, hipStream_t st);
// find_cluster_pairs_enspan_fast for every group with >= 2 pairs; L becomes the clustered list, cluster_out[p] its cluster number
void fast_cluster_all(const bk_pair *pairs, PairList &L, double w, DevBuf &cluster_out, ClusterBufs &b, hipStream_t st);
// K lists over disjoint sets of groups (each with offsets for all ng groups) -> one list in group order; cls[l] = the cluster
// numbers that travel with the elements of list l (cls and cl_out may be null)
void merge_lists_many(const PairList *const *lists, const uint32_t *const *cls, int K, PairList &out, DevBuf *cl_out, hipStream_t st);
// test hook: mask_pairs_chr_pos on the list in its current order
void debug_mask_list(const bk_pair *pairs, PairList &L, long dist, ClusterBufs &b, hipStream_t st);
