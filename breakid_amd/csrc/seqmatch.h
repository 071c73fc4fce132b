// Interface of seqmatch.hip: short queries searched in a library of sequences (bk_sequence_match).
#pragma once
#include "refseq_dev.h"
#include "prims.h"

struct SeqmatchBufs
{
  // the panel, the probes and the queries, uploaded per call
  DevBuf bases, off, probes, query;
  // the panel as codes, the k-mer flags and their scan, the k-mers as (key, position) pairs
  DevBuf codes, flag, keys, vals, scan_tmp, res;
  prims::RadixBufs rx;
  const uint64_t *d_off = nullptr;
  const struct bk_seq_probe *d_probes = nullptr;
  const uint8_t *d_query = nullptr;
  // the index that seqmatch_index left: m sorted k-mers
  const uint64_t *ikeys = nullptr;
  const uint32_t *ivals = nullptr;
  uint64_t m = 0;
};

// the passes of the index sort over the 2 * seed bits of a key
inline uint32_t seqmatch_passes(uint32_t seed) { return (2 * seed + 7) / 8; }
// the byte model of include/breakid_hip.h: the index over `bases` panel bases of which `kmers` start a key, and the n probes
inline uint64_t seqmatch_touched_index(uint64_t bases, uint64_t kmers, uint32_t seed) { return bases + 36ull * kmers * seqmatch_passes(seed); }
inline uint64_t seqmatch_touched_probes(uint64_t n, uint32_t max_len) { return n * (sizeof(struct bk_seq_probe) + sizeof(struct bk_seq_hit) + (uint64_t) max_len); }

// `panel`, `probes` and `query` are host arrays that the caller has checked (include/breakid_hip.h: off ascends from 0, every byte is one
// of A C G T N, 8 <= seed <= 16, 1 <= max_len <= 256).  seqmatch_upload queues the copies into `b`; seqmatch_index lists the k-mers of
// the panel, sorts them and returns how many there are after waiting for the stream once; seqmatch_probes queues one kernel on `st`.
// Device array owned by `b`: res[n].
void seqmatch_upload(const bk_seq_panel &panel, const struct bk_seq_probe *probes, uint64_t n, const uint8_t *query, uint32_t max_len, SeqmatchBufs &b, hipStream_t st);
uint64_t seqmatch_index(const bk_seq_panel &panel, uint32_t seed, SeqmatchBufs &b, hipStream_t st);
void seqmatch_probes(const bk_seq_panel &panel, uint64_t n, uint32_t max_len, uint32_t seed, SeqmatchBufs &b, hipStream_t st, struct bk_seq_hit **res);
