// Interface of known.hip: every call of a list against a panel of pairs of intervals (bk_known_calls).
#pragma once
#include "refseq_dev.h"
#include "prims.h"

struct KnownBufs
{
  DevBuf entries, sites, res, keys, vals, iend, run_max, cnt, off, nkey, nval, scan_tmp;
  prims::RadixBufs rx_index, rx_name, rx_site;
  const struct bk_known_entry *d_entries = nullptr;
  const struct bk_known_site *d_sites = nullptr;
  // the index that known_index left: m sorted interval ends (key, 2 * entry + k, the running maximum of `end` inside the contig's run)
  const unsigned long long *ikeys = nullptr;
  const uint32_t *ivals = nullptr;
};

// what the host's check of the panel and the sites found
struct KnownShape
{
  uint64_t n = 0, n_entries = 0, m = 0;  // sites, entries, intervals with tid >= 0
  int32_t max_tid = -1;                  // the largest tid among those intervals (-1: none)
  uint32_t max_name = 0;                 // the largest name id of the panel
  int key_bits() const;                  // the bits of ((tid + 1) << 32) | beg that the index sort looks at; 0 when m == 0
  int name_bits() const;                 // the bits of a name id in use
  int site_bits() const;                 // the bits of a site index in use
  uint32_t index_passes() const;
  uint32_t name_passes() const;
  uint64_t touched_index() const;               // the byte model of include/breakid_hip.h
  uint64_t touched_sites(uint64_t hits) const;  // ... `hits` = the listed hits of all sites
};

// `entries` and `sites` are host arrays that the caller has checked (include/breakid_hip.h: every error of bk_known_calls but the
// limit on the listed hits).  known_upload queues the copies into `b`; known_index sorts the interval ends and keeps the running
// maximum; known_count answers every field of a row but n_names, and returns the listed hits of all sites after waiting for the
// stream once; known_names lists, sorts and counts the names.  Device array owned by `b`: res[n].
void known_upload(const struct bk_known_entry *entries, uint64_t n_entries, const struct bk_known_site *sites, uint64_t n, KnownBufs &b, hipStream_t st);
void known_index(const KnownShape &shape, KnownBufs &b, hipStream_t st);
uint64_t known_count(const KnownShape &shape, uint32_t slop, KnownBufs &b, hipStream_t st, struct bk_known_call **res);
void known_names(const KnownShape &shape, uint32_t slop, uint64_t hits, KnownBufs &b, hipStream_t st);
