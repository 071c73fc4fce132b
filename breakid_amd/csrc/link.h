// Interface of link.hip: reciprocal partners, duplicates and events of a list of calls (bk_link_calls).
#pragma once
#include "refseq_dev.h"
#include "prims.h"

struct LinkBufs
{
  DevBuf sites, res, keys, vals, flags, run_of, label, ev_min, ev_cnt, changed, scan_tmp;
  prims::RadixBufs radix;
  const struct bk_link_site *d_sites = nullptr;
};

// what the host's check of the sites found: the breakends with tid >= 0 and the largest tid among them (-1: none)
struct LinkShape
{
  uint64_t n = 0, m = 0;
  int32_t max_tid = -1;
  int key_bits() const;      // the bits of ((tid + 1) << 32) | pos that the sort looks at; 0 when m == 0
  uint64_t touched() const;  // the byte model of include/breakid_hip.h
};

// `sites` is a host array that the caller has checked (every right is 0 or 1, n <= 2^30, max_dist <= BK_LINK_MAX_DIST).  link_upload
// queues the copy into `b`; link_calls queues the kernels and, between the rounds of the components, waits for the stream to read a
// flag.  Throws BK_ERR_LIMIT when the components need more than n + 1 rounds.  Device array owned by `b`: res[n].
void link_upload(const struct bk_link_site *sites, uint64_t n, LinkBufs &b, hipStream_t st);
void link_calls(const LinkShape &shape, uint32_t max_dist, LinkBufs &b, hipStream_t st, struct bk_call_link **res, uint32_t *rounds);
