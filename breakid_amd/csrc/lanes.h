// Interface of lanes.hip: the mask-and-cluster stage (bk_mask_and_cluster) and the state it keeps between calls.
#pragma once
#include <functional>
#include <memory>

#include "join.h"
#include "cluster.h"
#include "ahc.h"

// GPU_MAX_HW_QUEUES as the environment had it when the process made its first context (bk_prepare_process): the runtime's
// hardware-queue count as far as this library can know it, what the stage's queue budget is decided from
void stage_set_hw_queues(int n);

// what the stage reads of its context
struct StageInput
{
  int device;
  hipStream_t st;
  const JoinResult &jr;
  const std::vector<uint64_t> &gstart_host;  // jr.gstart on the host
  const std::vector<uint8_t> &own_groups;    // sharded sample (bk_shard_own_groups): 1 = this rank clusters the group; empty = all
  // runs body under the context's stage timer `name`: mask_and_cluster_lanes, or remove_isolated and then fast_cluster / ahc_cluster
  std::function<void(const char *name, const std::function<void()> &body)> timed;
};

struct ClusterStage
{
  SortService svc;  // resident sort service of the stage (sortsvc.inc)
  std::vector<hipEvent_t> svc_probe;
  int svc_late = 0;
  bool svc_refused = false;  // a stage of this context found the service out of reach once (shared hardware queue, crowded device): not tried again
  // a lane of chromosome-pair groups: its own buffers and host thread, the first few a stream.  Lane 0 always exists: it runs on the
  // context's stream and thread, and its buffers serve the one pass and the bk_debug_* entry points as well
  struct Lane
  {
    ClusterBufs cb;
    PairList list, iso;
    DevBuf d_cluster;
    hipStream_t st = nullptr;
    ~Lane()
    {
      if (st) (void) hipStreamDestroy(st);
    }
  };
  std::vector<std::unique_ptr<Lane>> lanes;
  ClusterBufs &cb() { return lanes[0]->cb; }
  AhcBufs ab;
  // what a call leaves: the clustered list in group order with its cluster numbers, and the list as it was after masking
  PairList list;
  DevBuf d_cluster, iso_idx, iso_goff;
  uint64_t iso_n = 0;
  // kept between calls: a list that is a local is allocated and freed (a device-wide wait) in every call
  PairList lane_mid, lane_iso_m;
  DevBuf d_drop;

  ClusterStage() { lanes.emplace_back(new Lane()); }
  // masks and clusters the groups of in.jr (of in.own_groups), in lanes when the data and the queues make them pay
  void run(const StageInput &in, double w, int fast);
  // sorts through the buffers of every lane by form (SortEmuBufs::sorts)
  void sort_forms(uint64_t out[3]) const;
  // test hook: one std_sort_groups through lane 0's buffers, as a job of the service when it is to be had
  void debug_sort(int device, hipStream_t st, uint32_t *key, uint32_t *idx, const uint32_t *gof, const uint64_t *goff, uint32_t ng, uint64_t n, uint64_t max_group);
};
