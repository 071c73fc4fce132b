// Interface of consensus.hip: the clipped bases of a table of reads piled up per breakpoint side (bk_clip_consensus).
#pragma once
#include "bk_common.h"

// a bk_reads table on the device (consensus_upload); seq travels apart: only the pile-up reads it
struct ConsensusReads
{
  uint64_t n = 0;
  const int32_t *tid = nullptr, *pos = nullptr;
  const uint16_t *flag = nullptr;
  const uint8_t *mapq = nullptr;
  const uint32_t *cigar_off = nullptr, *cigar = nullptr, *l_seq = nullptr;
  const uint64_t *seq_off = nullptr;
};

struct ConsensusBufs
{
  // the reads, uploaded per call
  DevBuf tid, pos, flag, mapq, cigar_off, cigar, l_seq, seq_off, seq;
  // the sites: keys in ascending order, the slot of every site in that order
  DevBuf keys, slot_of, counts, off, q0, clen, scan_tmp, stat;
  DevBuf res, bases, depth;
  // host side of keys and slot_of: they outlive the copies queued from them
  std::vector<unsigned long long> h_keys;
  std::vector<uint32_t> h_slot;
  ConsensusReads view;
  const uint8_t *d_seq = nullptr;
};

// what the kernels themselves moved (one atomic per wavefront adds to it): CIGAR words read by the two walks, contributions listed,
// bytes of SEQ read by the pile-up (ceil(min(c, max_len) / 2) per contribution)
struct ConsensusStat
{
  unsigned long long words, contributions, seq_bytes;
};

// `reads` and `sites` are host arrays that the caller has checked (offsets ascend, spans hold the bases, dir <= 1, tol == 0).
// consensus_upload queues the copies of the table's columns into `b` (the call's time on the device is the kernels' own: the caller
// times clip_consensus alone); clip_consensus then works on that copy.
// Device arrays owned by `b`: res[n_sites], bases[n_sites * max_len], depth[n_sites * max_len], *stat_out.  The call only queues
// work on `st`, except for one synchronisation that sizes the contribution list.
void consensus_upload(const bk_reads &reads, ConsensusBufs &b, hipStream_t st);
void clip_consensus(const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, uint32_t max_len, uint32_t min_depth, ConsensusBufs &b, hipStream_t st,
                    struct bk_consensus **res, uint8_t **bases, uint32_t **depth, ConsensusStat **stat_out);
