// Interface of partners.hip: where the discordant pairs inside arbitrary windows point to (bk_locus_partners).
#pragma once
#include "bp.h"

struct PartnerBufs
{
  DevBuf sites, res, key, val, mkey, info, cnt, off, rkey, rsite, skey, spos, fkey, scan_tmp;
  prims::RadixBufs rx_index, rx_rows, rx_site;  // three sorts whose results are alive at the same time
  const struct bk_partner_site *d_sites = nullptr;
  // the index of the last partners_index: the own keys of the 2 P ends in ascending order and the mates' keys in that order
  const uint64_t *ikeys = nullptr, *imates = nullptr;
  uint64_t n_ends = 0;
};

// the bits of ((tid + 1) << 32) | pos that vary over a reference list of n_targets contigs
int partners_key_bits(int32_t n_targets);
// the passes of the two sorts of the elsewhere rows: by the mate key's bits, then by the bits of the largest site number
uint32_t partners_row_passes(int32_t n_targets, uint64_t n_sites);
// the byte model of include/breakid_hip.h, in its two parts
uint64_t partners_touched_index(uint64_t n_pairs);
uint64_t partners_touched_sites(int32_t n_targets, uint64_t n_sites, uint64_t n_rows);

// `sites` is a host array that the caller has checked (reserved == 0, n <= 2^30).  partners_upload queues the copy into `b`.
// partners_index queues the index of the 2 * n_pairs ends of `pairs` (rebuilt by every call).  partners_count queues the count kernel
// and the scan of the elsewhere counts and waits for the stream once, to read their total, which it returns.  partners_rows queues the
// rest for that total, which the caller has checked against the sort's limit.  Device array owned by `b`: res[n].
void partners_upload(const struct bk_partner_site *sites, uint64_t n, PartnerBufs &b, hipStream_t st);
void partners_index(const bk_pair *pairs, uint64_t n_pairs, int32_t n_targets, PartnerBufs &b, hipStream_t st);
uint64_t partners_count(int32_t n_targets, uint64_t n, PartnerBufs &b, hipStream_t st);
void partners_rows(int32_t n_targets, uint64_t n, uint64_t n_rows, uint32_t max_gap, PartnerBufs &b, hipStream_t st, struct bk_locus_partners **res);
