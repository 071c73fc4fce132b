// Interface of frame.hip: the 5' / 3' partners and the reading frame of every call (bk_fusion_frame).
#pragma once
#include "refseq_dev.h"

constexpr uint32_t FRAME_CHUNK = 128;  // overlapping transcripts of one side that a wavefront stages in LDS at a time

// a bk_txmodel on the device (frame_upload): the columns as they came, and what the device derives from them
struct FrameModel
{
  uint32_t n_tx = 0;
  const unsigned long long *key = nullptr;  // (tid << 32) | tx_start: ascending
  const uint32_t *tx_end = nullptr, *run_max = nullptr;  // run_max[i] = the largest tx_end of the rows of tid[i] up to i
  const uint8_t *strand = nullptr;
  const uint32_t *ex_off = nullptr, *ex_start = nullptr, *ex_end = nullptr;
  const unsigned long long *cum = nullptr;  // n_parts + 1: the coding bases in front of every part, over the whole model
};

struct FrameBufs
{
  DevBuf tid, tx_start, tx_end, strand, ex_off, ex_start, ex_end, key, run_max, cum, scan_tmp, sites, res;
  FrameModel view;
  const struct bk_frame_site *d_sites = nullptr;
};

// `model` and `sites` are host arrays that the caller has checked (include/breakid_hip.h: the rows ascend, the parts ascend inside
// their transcript, ex_off runs from 0 to n_parts, every right is 0 or 1).  frame_upload queues the copies into `b`; frame_derive
// queues the kernels that make key, run_max and cum; fusion_frame queues the site kernel.  Device array owned by `b`: res[n].
void frame_upload(const bk_txmodel &model, const struct bk_frame_site *sites, uint64_t n, FrameBufs &b, hipStream_t st);
void frame_derive(const bk_txmodel &model, FrameBufs &b, hipStream_t st);
void fusion_frame(uint64_t n, FrameBufs &b, hipStream_t st, struct bk_frame_call **res);
