// BreakID command line on top of libbreakid_hip.so: same options, same output files as the reference
// (src/BreakID.cc:6-192, help text src/BreakID.h:27-36).  The hot path (BreakID.cc:98-167 minus annotation)
// runs on the MI355X through the C ABI; this file is the host side the reference keeps in main():
// argument parsing, BAM decode into the columnar table, refGene/nib annotation (BreakID.cc:492-567,
// :1528-1793, RefSeqTranscript.cc, nibtools.cc, util_bam.cc:78-122, util_bed.cc:224-261) and the writers
// (:1170-1263).  There is no CPU implementation of the hot path in here.
#include <getopt.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include <zlib.h>

#include "../../include/breakid_hip.h"
#include "../../include/breakid_multi.h"

// -normal: looked up at run time, so that this file also links against a library without the call (the CPU build of the host
// code, oracle/Makefile); -normal then ends with an error
extern "C" int bk_normal_support(bk_ctx *tumor, bk_ctx *normal, double w, const struct bk_normal_support **out, uint64_t *count) __attribute__((weak));
// -genotype: the same for the reference-allele counts and the genotype model (the CPU build refuses -genotype)
extern "C" int bk_ref_support(bk_ctx *calls, bk_ctx *records, int mapq_min, int anchor, double w, const struct bk_ref_support **out, uint64_t *count)
    __attribute__((weak));
extern "C" int bk_genotype_call(uint32_t alt, uint32_t ref, uint8_t *gt, uint8_t *gq, float *vaf) __attribute__((weak));
// -vcf: the same for the junction evidence and the two breakend rules (the CPU build refuses -vcf)
extern "C" int bk_junctions(bk_ctx *ctx, const struct bk_junction **out, uint64_t *count) __attribute__((weak));
extern "C" int bk_junction_sides(const struct bk_junction *j, uint8_t *right1, uint8_t *right2, uint8_t *source) __attribute__((weak));
extern "C" int bk_vcf_breakend_alt(char ref_base, int own_right, const char *mate_chr, uint32_t mate_pos, int mate_right, char *buf, size_t cap) __attribute__((weak));
// -evidence: the same for the evidence rows (the CPU build refuses -evidence; bk_bam_extract is host code and always there)
extern "C" int bk_evidence(bk_ctx *ctx, const struct bk_evidence **out, uint64_t *count, const uint64_t **call_off) __attribute__((weak));
// -consensus: the same for the junction consensus (the CPU build refuses -consensus)
extern "C" int bk_clip_consensus(bk_ctx *ctx, const bk_reads *reads, const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, uint32_t max_len,
                                 uint32_t min_depth, const struct bk_consensus **out, const uint8_t **bases, const uint32_t **col_depth) __attribute__((weak));
// -homology: the same for the junction fit (the CPU build refuses -homology)
extern "C" int bk_junction_fit(bk_ctx *ctx, const bk_refseq *ref, const struct bk_junction_probe *probes, uint64_t n, const uint8_t *query, uint32_t max_len, uint32_t max_shift,
                               uint32_t max_ins, uint32_t max_hom, const struct bk_junction_fit **out) __attribute__((weak));
// -dedup: the same for the unique fragments behind every call (the CPU build refuses -dedup)
extern "C" int bk_unique_support(bk_ctx *ctx, const struct bk_unique_support **out, uint64_t *count, const uint64_t **first, uint64_t *n_rows) __attribute__((weak));
// -clip: the same for the soft-clip evidence, the depth at the rescued positions and the rescue rule (the CPU build refuses -clip)
extern "C" int bk_clip_support(bk_ctx *calls, bk_ctx *records, int mapq_min, int min_clip, double w, const struct bk_clip_support **out, uint64_t *count)
    __attribute__((weak));
extern "C" int bk_clip_reads(bk_ctx *records, const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, const uint32_t **counts,
                             const struct bk_clip_read **rows, const uint64_t **site_off) __attribute__((weak));
extern "C" int bk_base_depth(bk_ctx *records, const int32_t *tid, const uint32_t *pos, uint64_t n, const uint32_t **out) __attribute__((weak));
extern "C" int bk_clip_rescue(const bk_cluster *c, const struct bk_junction *j, const struct bk_clip_support *s, uint32_t min_support, uint32_t *pos1, uint32_t *pos2,
                              uint32_t *n1, uint32_t *n2) __attribute__((weak));
// -x: the same for the exclude list (the CPU build refuses -x)
extern "C" int bk_exclude_regions(bk_ctx *ctx, const bk_regions *r, uint64_t *n_removed) __attribute__((weak));
extern "C" int bk_multi_run_ex(const bk_soa *host_table, const uint32_t *target_len, const char *const *target_name, int n_targets, const bk_regions *exclude, int n_gpus,
                               int transport, int mapq_min, int fast, double *w_out, uint64_t *n_clustered_total, bk_ctx **ctx0_out, char *err, size_t errlen)
    __attribute__((weak));
extern "C" int bk_multi_run_bam_ex(const char *path, const bk_regions *exclude, int n_gpus, int transport, int mapq_min, int fast, double *w_out, uint64_t *n_clustered_total,
                                   bk_ctx **ctx0_out, int *n_targets, const char *const **names, const uint32_t **lens, char *err, size_t errlen) __attribute__((weak));
extern "C" int bk_multi_excluded(bk_ctx *ctx, uint64_t *n_removed) __attribute__((weak));

// bam_index_load (htslib-1.3.1 sam.h:302 -> hts.c:2042 hts_idx_load, :1580 hts_idx_load_local, :1528 hts_idx_load_core): the index is
// <bam>.csi, <bam with its extension replaced>.csi, <bam>.bai, <...>.bai - the first that can be opened - and it must parse to the
// end: magic, counts, every bin's chunk list and every linear index (a truncated or foreign file gives NULL, i.e. the reference's
// "please index bam-file first" exit, BreakID.cc:411-416).  The hot path streams the whole file and does not use the offsets; what is
// reproduced here is which files the reference accepts.  gzread() reads plain and (B)GZF-compressed files alike, as bgzf_read does.
static bool index_loads(const std::string &bam)
{
  auto candidate = [&](const char *ext) -> std::string {
    std::string a = bam + ext;
    if (FILE *f = fopen(a.c_str(), "rb"))
    {
      fclose(f);
      return a;
    }
    size_t i = bam.size();
    while (i > 1 && bam[i - 1] != '.') --i;  // hts_idx_getfn: the last '.' at an index > 0
    if (i > 1)
    {
      a = bam.substr(0, i - 1) + ext;
      if (FILE *f = fopen(a.c_str(), "rb"))
      {
        fclose(f);
        return a;
      }
    }
    return std::string();
  };
  std::string fn = candidate(".csi");
  if (fn.empty()) fn = candidate(".bai");
  if (fn.empty()) return false;
  gzFile fp = gzopen(fn.c_str(), "rb");
  if (!fp) return false;
  auto rd = [&](void *dst, size_t n) { return n == 0 || gzread(fp, dst, (unsigned) n) == (int) n; };
  auto skip = [&](uint64_t n) {
    char buf[65536];
    while (n)
    {
      const size_t k = n < sizeof buf ? (size_t) n : sizeof buf;
      if (!rd(buf, k)) return false;
      n -= k;
    }
    return true;
  };
  bool ok = false;
  do
  {
    uint8_t magic[4];
    if (!rd(magic, 4)) break;
    int fmt;  // 0 CSI, 1 BAI, 2 TBI
    int32_t n_ref = 0;
    if (!memcmp(magic, "CSI\1", 4))
    {
      uint32_t x[3];
      if (!rd(x, 12) || !skip(x[2]) || !rd(&n_ref, 4)) break;
      fmt = 0;
    }
    else if (!memcmp(magic, "TBI\1", 4))
    {
      uint32_t x[8];
      if (!rd(x, 32) || !skip(x[7])) break;
      n_ref = (int32_t) x[0];
      fmt = 2;
    }
    else if (!memcmp(magic, "BAI\1", 4))
    {
      if (!rd(&n_ref, 4)) break;
      fmt = 1;
    }
    else
      break;
    bool good = true;
    for (int32_t i = 0; i < n_ref && good; ++i)
    {
      int32_t n_bin;
      if (!rd(&n_bin, 4))
      {
        good = false;
        break;
      }
      std::set<uint32_t> seen;
      for (int32_t j = 0; j < n_bin && good; ++j)
      {
        uint32_t key;
        int32_t n_chunk;
        uint64_t loff;
        good = rd(&key, 4) && seen.insert(key).second && (fmt != 0 || rd(&loff, 8)) && rd(&n_chunk, 4) && n_chunk >= 0 && skip((uint64_t) n_chunk << 4);
      }
      if (good && fmt != 0)
      {
        int32_t n_intv;
        good = rd(&n_intv, 4) && n_intv >= 0 && skip((uint64_t) n_intv << 3);
      }
    }
    ok = good;  // (the trailing n_no_coor is optional: hts.c:1575)
  } while (false);
  gzclose(fp);
  return ok;
}

// the reference list of a BAM file (magic, header text, n_ref, name / length pairs); gzread reads the BGZF members in turn, so only
// the first blocks of the file are inflated
static bool bam_header_list(const std::string &path, std::vector<std::string> &names, std::vector<uint32_t> &lens)
{
  gzFile fp = gzopen(path.c_str(), "rb");
  if (!fp) return false;
  auto rd = [&](void *dst, size_t n) { return n == 0 || gzread(fp, dst, (unsigned) n) == (int) n; };
  bool ok = false;
  do
  {
    char magic[4];
    int32_t l_text = 0, n_ref = 0;
    if (!rd(magic, 4) || memcmp(magic, "BAM\1", 4) || !rd(&l_text, 4) || l_text < 0) break;
    std::vector<char> text((size_t) l_text);
    if (!rd(text.data(), text.size()) || !rd(&n_ref, 4) || n_ref < 0) break;
    bool good = true;
    for (int32_t i = 0; i < n_ref && good; ++i)
    {
      int32_t l_name = 0;
      uint32_t l_ref = 0;
      good = rd(&l_name, 4) && l_name > 0;
      std::vector<char> nm(good ? (size_t) l_name : 0);
      good = good && rd(nm.data(), nm.size()) && rd(&l_ref, 4);
      if (good)
      {
        names.emplace_back(nm.data(), strnlen(nm.data(), nm.size()));
        lens.push_back(l_ref);
      }
    }
    ok = good;
  } while (false);
  gzclose(fp);
  return ok;
}

// -x regions.bed: whitespace-separated fields, 0-based half-open coordinates.  Blank lines and lines that start with '#', "track" or
// "browser" are skipped; one field excludes the whole contig, three or more give an interval, clamped to the contig's length.  Names
// match the header's exactly.  Lines on contigs the header does not have are counted; two fields, a field that is not a number, a
// negative coordinate or end <= beg end the run.
struct ExcludeList
{
  std::vector<int32_t> tid, beg, end;
  uint64_t unknown = 0, lines = 0;
};
static ExcludeList read_exclude_bed(const std::string &path, const std::vector<std::string> &names, const std::vector<uint32_t> &lens)
{
  std::ifstream in(path.c_str());
  if (!in.is_open())
  {
    std::cerr << "Error: can not open exclude file: " << path << std::endl;
    exit(1);
  }
  std::map<std::string, int> id;
  for (size_t i = 0; i < names.size(); ++i) id.emplace(names[i], (int) i);
  ExcludeList x;
  std::string line;
  uint64_t no = 0;
  auto fail = [&](const std::string &why) {
    std::cerr << "Error: exclude file " << path << ", line " << no << ": " << why << std::endl;
    exit(1);
  };
  auto number = [&](const std::string &f) {
    char *e = nullptr;
    errno = 0;
    const long long v = strtoll(f.c_str(), &e, 10);
    if (f.empty() || *e || errno) fail("not a number: " + f);
    if (v < 0) fail("negative coordinate: " + f);
    return v;
  };
  while (std::getline(in, line))
  {
    ++no;
    std::istringstream ss(line);
    std::vector<std::string> f;
    for (std::string w; ss >> w;) f.push_back(w);
    if (f.empty() || f[0][0] == '#' || f[0] == "track" || f[0] == "browser") continue;
    if (f.size() == 2) fail("two fields (a line needs a contig name alone, or contig, start and end)");
    long long b = 0, e = 0;
    if (f.size() >= 3)
    {
      b = number(f[1]);
      e = number(f[2]);
      if (e <= b) fail("end <= start");
    }
    ++x.lines;
    auto it = id.find(f[0]);
    if (it == id.end())
    {
      ++x.unknown;
      continue;
    }
    const long long len = lens[it->second];
    if (f.size() == 1) e = len;
    b = std::min(b, len);
    e = std::min(e, len);
    if (e <= b) continue;  // (behind the contig's end)
    x.tid.push_back(it->second);
    x.beg.push_back((int32_t) b);
    x.end.push_back((int32_t) e);
  }
  if (x.unknown && x.unknown == x.lines)
    std::cerr << "Warning: no line of the exclude file " << path << " names a contig of the BAM header (" << x.unknown
              << " lines; names must match exactly): nothing is excluded" << std::endl;
  else if (x.unknown)
    std::cerr << "Warning: " << x.unknown << " lines of the exclude file " << path << " name contigs that are not in the BAM header" << std::endl;
  return x;
}

#ifndef BREAKID_INSTALLDIR
#define BREAKID_INSTALLDIR "."
#endif

using std::string;
using std::vector;

static const char *HELP =
    " Usage: \n \t BreakID -i input.bam -o prefix -n nib_folder <options> \n\n \
     DESCRIPTION\n \
     \t -h -? -help \t help\n \
     \t -i*        \t input bam-file\n \
     \t -o*        \t output file (prefix only)\n \
     \t -n*        \t folder name to nib files\n \
     \t -q         \t encompassing reads quality thresholds  [20]\n\
     \t -t         \t distance relative to (sqrt(2)*(insert size mean +3* insert size sd))  [2]\n \
     \t -fast      \t use the fast cluster strategy [default no] \n \
     \t -all       \t no filter enspan out [default is filter]  \n \
     \t -x         \t exclude list (BED: contig [start end]); records that overlap it are ignored  \n \
     \t -genotype  \t count reference-allele evidence and genotype every call (twin files *_genotype.txt)  \n \
     \t -anchor    \t bases a reference read must cover on either side of a breakpoint (with -genotype)  [10]\n \
     \t -vcf       \t also write the calls as VCF breakends (*_fusion.vcf)  \n \
     \t -evidence  \t also list the reads behind every call (*_evidence.txt) and write them as a BAM (*_evidence.bam)  \n \
     \t -dedup     \t count the different fragments behind every call (twin files *_dedup.txt; UPE / USR with -vcf, a Dup column with -evidence)  \n \
     \t -clip      \t count soft-clipped reads without an SA tag at every call (twin files *_clip.txt) and rescue clusters the vote left out (*_fusion_rescued.txt)  \n \
     \t -minclip   \t shortest soft clip that counts (with -clip)  [10]\n \
     \t -clipsupport \t clipped reads at one position that each side of a rescued cluster needs (with -clip)  [3]\n \
     \t -consensus \t vote the clipped bases at both breakpoints of every call into a junction sequence (twin files *_consensus.txt; CSEQ / CSN with -vcf)  \n \
     \t -conslen   \t longest junction sequence per side, 1 to 256 (with -consensus)  [64]\n \
     \t -homology  \t fit each junction sequence to the reference at the other breakpoint: offset, inserted bases, microhomology (with -consensus; twin files *_homology.txt; HOMLEN / HOMSEQ / JINS with -vcf)  \n \
     \t -homshift  \t largest offset of the continuation from the called position, 0 to 64 (with -homology)  [32]\n \
     \t -homins    \t longest inserted sequence, 0 to 64 (with -homology)  [32]\n ";

// ---- RefSeqTranscript.{h,cc} -------------------------------------------------------------------------------
struct Txpt
{
  string transcriptID, chrom, strand, geneName;
  uint32_t txStart = 0, txEnd = 0, cdsStart = 0, cdsEnd = 0, exonCount = 0, cDNALength = 0;
  vector<uint32_t> exonStarts, exonEnds, codingStarts, codingEnds, codingParts;
  int codingExonCount = 0;
};

static vector<uint32_t> split_to_int(const string &s)  // splitStringToInt(s, ","), empty tokens dropped
{
  vector<uint32_t> out;
  size_t st = 0;
  while (true)
  {
    size_t e = s.find(',', st);
    string tok = s.substr(st, e == string::npos ? string::npos : e - st);
    if (!tok.empty()) out.push_back((uint32_t) atol(tok.c_str()));
    if (e == string::npos) break;
    st = e + 1;
  }
  return out;
}

static Txpt parse_refgene_line(const string &line)  // RefSeqTranscript.cc:19-81 + removeUTR :94-142
{
  Txpt t;
  std::stringstream ss(line);
  string f[16];
  for (int i = 0; i < 16; ++i)
    if (!getline(ss, f[i], '\t')) f[i] = i ? f[i - 1] : "";  // getline leaves `tmp` unchanged at EOF
  t.transcriptID = f[1];
  t.chrom = f[2];
  t.strand = f[3];
  t.txStart = (uint32_t) atol(f[4].c_str());
  t.txEnd = (uint32_t) atol(f[5].c_str());
  t.cdsStart = (uint32_t) atol(f[6].c_str());
  t.cdsEnd = (uint32_t) atol(f[7].c_str());
  t.exonCount = (uint32_t) atol(f[8].c_str());
  t.exonStarts = split_to_int(f[9]);
  t.exonEnds = split_to_int(f[10]);
  t.geneName = f[12];
  if (t.cdsStart != t.cdsEnd)
  {
    for (uint32_t i = 0; i < t.exonCount && i < t.exonStarts.size() && i < t.exonEnds.size(); ++i)
    {
      uint32_t s = t.exonStarts[i], e = t.exonEnds[i];
      if (s < t.cdsEnd && e > t.cdsStart)
      {
        if (s < t.cdsStart && e > t.cdsStart && e <= t.cdsEnd) { t.codingStarts.push_back(t.cdsStart); t.codingEnds.push_back(e); }
        else if (s < t.cdsEnd && e > t.cdsEnd && s >= t.cdsStart) { t.codingStarts.push_back(s); t.codingEnds.push_back(t.cdsEnd); }
        else if (e > t.cdsEnd && s < t.cdsStart) { t.codingStarts.push_back(t.cdsStart); t.codingEnds.push_back(t.cdsEnd); }
        else { t.codingStarts.push_back(s); t.codingEnds.push_back(e); }
      }
    }
    t.codingExonCount = (int) t.codingStarts.size();
    for (size_t i = 0; i < t.codingStarts.size(); ++i) t.cDNALength += t.codingEnds[i] - t.codingStarts[i];
  }
  for (size_t i = 0; i < t.codingStarts.size(); ++i)  // add_cds_parts
  {
    t.codingParts.push_back(t.codingStarts[i]);
    t.codingParts.push_back(t.codingEnds[i]);
  }
  return t;
}

static bool read_refgene(const string &fn, vector<Txpt> &out)  // readRefSeqTranscript: NR_ transcripts skipped
{
  std::ifstream in(fn);
  if (!in.is_open()) return false;
  string line;
  while (getline(in, line, '\n'))
  {
    std::stringstream l2(line);
    string a, b;
    getline(l2, a, '\t');
    if (!getline(l2, b, '\t')) b = a;
    if (b.find("NR_") != string::npos) continue;
    out.push_back(parse_refgene_line(line));
  }
  return true;
}

// add_exon_num_anno, BreakID.cc:1753-1793
static void exon_numbers(const Txpt &t, long pos, int &s_no, int &e_no)
{
  s_no = e_no = 0;
  for (size_t i = 0; i + 1 < t.codingParts.size(); ++i)
  {
    if (pos >= (long) t.codingParts[i] && pos <= (long) t.codingParts[i + 1])
    {
      int idx = (int) i / 2 + 1;
      if (t.strand == "+")
      {
        s_no = idx;
        e_no = (i % 2 == 1) ? idx + 1 : idx;
      }
      if (t.strand == "-")
      {
        s_no = t.codingExonCount + 1 - (idx + 1);
        e_no = (i % 2 == 1) ? t.codingExonCount + 1 - idx : t.codingExonCount + 1 - (idx + 1);
      }
      break;
    }
  }
}

// one side of add_exon_anno, BreakID.cc:1549-1585 (find_the_longest_cds_txpt never updates its maximum, so the
// LAST overlapping transcript with cDNA > 0 wins, RefSeqTranscript.cc:311-320)
static void annotate_side(const vector<Txpt> &txpts, const string &chr, long pos, string &gene, string &exon_info, string &strand)
{
  if (pos == -1)
  {
    exon_info = gene = strand = ".";
    return;
  }
  vector<const Txpt *> hit;
  for (auto &t : txpts)
    if (chr == t.chrom && pos >= (long) t.txStart && pos <= (long) t.txEnd) hit.push_back(&t);
  if (hit.empty())
  {
    exon_info = ".";
    gene = "intergenic";
    strand = ".";
    return;
  }
  Txpt chosen;
  for (auto *t : hit)
    if ((int) t->cDNALength > 0) chosen = *t;
  gene = chosen.geneName;
  strand = chosen.strand;
  int a, b;
  exon_numbers(chosen, pos, a, b);
  exon_info = chosen.transcriptID + ":" + std::to_string(a) + "-" + std::to_string(b);
}

// ---- nib access: nibtools.cc:7-58, util_bam.cc:78-122 -------------------------------------------------------------------
struct Nib
{
  std::ifstream in;
  unsigned long nBases = 0;
  bool ok = false;
  void open(const string &fn)
  {
    in.open(fn, std::ios::binary);
    if (!in.is_open()) return;
    unsigned char raw[8];
    in.read((char *) raw, 8);
    unsigned long sig = raw[0] | (raw[1] << 8) | (raw[2] << 16) | ((unsigned long) raw[3] << 24);
    nBases = raw[4] | (raw[5] << 8) | (raw[6] << 16) | ((unsigned long) raw[7] << 24);
    ok = sig == 0x6be93d3aUL;
  }
  void base(char *out, unsigned long pos)  // leaves *out untouched on any failure, like the reference
  {
    if (!ok || pos >= nBases) return;
    in.seekg(8 + pos / 2);
    char r;
    in.read(&r, 1);
    int v = (pos % 2 == 0) ? ((r & 0xff) >> 4) : (r & 0x0f);
    static const char tab[16] = {'T', 'C', 'A', 'G', 'N', 'N', 'N', 'N', 'T', 'C', 'A', 'G', 'N', 'N', 'N', 'N'};
    *out = tab[v & 15];
  }
};

static string neighbour_seq(const string &nib_dir, const string &chr, int32_t bp)
{
  // left 20 (1-based bp-20 .. bp-1) + right 21 (bp .. bp+20), BreakID.cc:554-559
  Nib n;
  n.open(nib_dir + "/hg19_" + chr + ".nib");
  string s;
  char b = 'N';
  for (int32_t i = bp - 20; i < bp; ++i)
  {
    n.base(&b, (unsigned long) (long) (i - 1));
    s += b;
  }
  for (int32_t i = bp - 1; i < bp - 1 + 21; ++i)
  {
    n.base(&b, (unsigned long) (long) i);
    s += b;
  }
  return s;
}

static int longest_run(const string &s)  // find_longest_repeat_substring, util_bed.cc:224-261
{
  int best = 0;
  size_t i = 0;
  while (i < s.size())
  {
    size_t j = i + 1;
    while (j < s.size() && s[j] == s[i]) ++j;
    best = std::max(best, (int) (j - i));
    i = j;
  }
  return best;
}

static const char *fusion_type(uint32_t mask)  // determine_fusion_type_from_drp, BreakID.cc:1888-1907
{
  if (mask & BK_TYPE_DEFAULT_ORIENT) return "Deletion";
  if (mask & BK_TYPE_ABS_REVERSE) return "Duplication";
  if (mask & BK_TYPE_SAME_ORIENT) return "Inversion";
  if (mask & BK_TYPE_DIFF_CHR) return "Translocation";
  return "Unknown";
}

struct OutRow
{
  bk_cluster c;
  uint64_t idx;  // row of BK_STAGE_CLUSTERS (the matched normal's counts, bk_normal_support)
  string p1_chr, p2_chr, g1, g2, e1, e2, s1, s2, rpt1, rpt2;
  bool is_rpt;
  float af1, af2;
};
static bool cmp_cluster(OutRow a, OutRow b) { return a.c.n_drp > b.c.n_drp; }  // BreakID.h:185-188 (by value, like the reference)

// the eight genotype columns of one sample: a call is genotyped on its junction reads (alt = n_sr against the mean of the two sides'
// reference reads, rounded up); the pair counts stand beside it (include/breakid_hip.h: bk_genotype_call)
static void write_genotype(std::ostream &o, const struct bk_ref_support &rs, uint32_t n_drp, uint32_t n_sr)
{
  uint8_t gt = 255, gq = 0, gtp = 255, gqp = 0;
  float vaf = 0, vaf_pairs = 0;
  bk_genotype_call(n_sr, (uint32_t) (((uint64_t) rs.ref_reads1 + rs.ref_reads2 + 1) / 2), &gt, &gq, &vaf);
  bk_genotype_call(n_drp, (uint32_t) (((uint64_t) rs.ref_pairs1 + rs.ref_pairs2 + 1) / 2), &gtp, &gqp, &vaf_pairs);
  auto put_vaf = [&](float v) {
    if (v != v)
      o << "\t.";
    else
      o << "\t" << v;
  };
  o << "\t" << rs.ref_pairs1 << "\t" << rs.ref_pairs2 << "\t" << rs.ref_reads1 << "\t" << rs.ref_reads2;
  put_vaf(vaf_pairs);
  put_vaf(vaf);
  o << "\t" << (gt == 0 ? "0/0" : gt == 1 ? "0/1" : gt == 2 ? "1/1" : "./.") << "\t" << (int) gq;
}

// -clip: the eight clip columns of one call (the directions d_s are those of its bk_junction row), and with -normal the two of the normal
struct ClipCols
{
  uint32_t at[2], peak_pos[2], peak_n[2], events[2];
  bool with_normal = false;
  uint32_t normal_at[2] = {0, 0};
};
static ClipCols clip_cols(const struct bk_junction &j, const struct bk_clip_support &s, const struct bk_clip_support *normal)
{
  uint8_t d[2] = {0, 1}, source = 0;
  bk_junction_sides(&j, &d[0], &d[1], &source);
  ClipCols c;
  for (int side = 0; side < 2; ++side)
  {
    c.at[side] = s.at[side][d[side]];
    c.peak_pos[side] = s.peak_pos[side][d[side]];
    c.peak_n[side] = s.peak_n[side][d[side]];
    c.events[side] = s.events[side][d[side]];
    if (normal) c.normal_at[side] = normal->at[side][d[side]];
  }
  c.with_normal = normal != nullptr;
  return c;
}

static void write_row(std::ostream &o, const OutRow &r, const struct bk_normal_support *ns = nullptr, const struct bk_ref_support *gt = nullptr,
                      const struct bk_ref_support *gt_normal = nullptr, const ClipCols *clip = nullptr, const string *tail = nullptr)
{
  o << fusion_type(r.c.type_mask) << "\t";
  o << r.p1_chr << ":" << r.c.p1_exact << "\t";
  o << r.p2_chr << ":" << r.c.p2_exact << "\t";
  o << r.g1 << "\t" << r.s1 << ":" << r.e1 << "\t";
  o << r.g2 << "\t" << r.s2 << ":" << r.e2 << "\t";
  o << (long) r.c.n_drp << "\t" << (long) r.c.n_sr << "\t";
  o << (double) r.c.depth1 << "\t" << (double) r.c.depth2 << "\t";
  o << r.af1 << "\t" << r.af2 << "\t";
  o << r.rpt1 << "\t" << r.rpt2;
  if (gt) write_genotype(o, *gt, r.c.n_drp, r.c.n_sr);
  if (ns) o << "\t" << ns->n_drp << "\t" << ns->n_sr << "\t" << ns->depth1 << "\t" << ns->depth2;
  if (ns && gt_normal) write_genotype(o, *gt_normal, ns->n_drp, ns->n_sr);
  if (clip)
  {
    o << "\t" << clip->at[0] << "\t" << clip->at[1] << "\t" << clip->peak_pos[0] << "\t" << clip->peak_n[0] << "\t" << clip->peak_pos[1] << "\t" << clip->peak_n[1] << "\t"
      << clip->events[0] << "\t" << clip->events[1];
    if (clip->with_normal) o << "\t" << clip->normal_at[0] << "\t" << clip->normal_at[1];
  }
  if (tail) o << *tail;
  o << "\n";
}

static const char *HEADER =
    "Fusion_Type\tBreakPoint1\tBreakPoint2\tGene1\tBreakPoint_Info_Pair1\tGene2\tBreakPoint_Info_Pair2\tN_DRP\tN_SR\t"
    "BreakPoint1_Depth\tBreakPoint2_Depth\tBreakPoint1_AF\tBreakPoint2_AF\tBP1_Neighbour_Seq\tBP2_Neighbour_Seq\n";
static const char *NORMAL_COLUMNS = "\tNormal_DRP\tNormal_SR\tNormal_Depth1\tNormal_Depth2\n";
// -genotype: the twin files' columns for the sample itself, and behind the four Normal_* columns the same eight for the normal
static const char *GENOTYPE_COLUMNS = "\tRef_Pairs1\tRef_Pairs2\tRef_Reads1\tRef_Reads2\tVAF_Pairs\tVAF_Reads\tGT\tGQ";
static const char *GENOTYPE_COLUMNS_NORMAL =
    "\tNormal_Ref_Pairs1\tNormal_Ref_Pairs2\tNormal_Ref_Reads1\tNormal_Ref_Reads2\tNormal_VAF_Pairs\tNormal_VAF_Reads\tNormal_GT\tNormal_GQ";

// -clip: the twin files' columns, and behind them those of the normal
static const char *CLIP_COLUMNS = "\tClip1\tClip2\tClipPeak1\tClipPeakN1\tClipPeak2\tClipPeakN2\tClipBg1\tClipBg2";
static const char *CLIP_COLUMNS_NORMAL = "\tNormal_Clip1\tNormal_Clip2";
// -dedup: the twin files' columns (bk_unique_support: fragments among the N_DRP rows and the N_SR tuples, and the rows of the largest one)
static const char *DEDUP_COLUMNS = "\tUniq_DRP\tUniq_SR\tTop_DRP\tTop_SR";
// -consensus: the twin files' columns (bk_clip_consensus at the two breakpoints of the call: reads, voted columns, match / total, the
// voted bases in the orientation of the BAM)
static const char *CONSENSUS_COLUMNS = "\tCons_N1\tCons_Len1\tCons_Agree1\tCons_Seq1\tCons_N2\tCons_Len2\tCons_Agree2\tCons_Seq2";
// the vote's own threshold (BreakID.cc:446): a column counts from two reads on
static const uint32_t CONSENSUS_MIN_DEPTH = 2;

// One side of a written call: its bk_consensus row and its bases as the BAM reads them (reference-forward at the anchor): a LEFT side
// is columns 0 .. len - 1, a RIGHT side the same reversed, so that the text ends at the base just left of the breakpoint.
struct ConsensusSide
{
  struct bk_consensus c = {0, 0, 0, 0};
  string seq;
  string agree() const
  {
    if (!c.total) return ".";
    char buf[32];
    snprintf(buf, sizeof buf, "%.3f", (double) c.match / (double) c.total);
    return buf;
  }
};
// -homology: the twin files' columns (bk_junction_fit of each side's consensus against the reference at the other side)
static const char *HOMOLOGY_COLUMNS = "\tJ_Shift1\tJ_Ins1\tJ_Aligned1\tJ_Mism1\tJ_HomLen1\tJ_HomSeq1\tJ_InsSeq1\tJ_Shift2\tJ_Ins2\tJ_Aligned2\tJ_Mism2\tJ_HomLen2\tJ_HomSeq2\tJ_InsSeq2";
// the homology behind the breakpoint is looked for over this many retained bases
static const uint32_t HOMOLOGY_MAX_HOM = 32;

// One side of a written call: its bk_junction_fit row (on: the side was submitted and placed), the own contig's bases over the
// homologous stretch, reference-forward, and the inserted columns as the BAM reads them (reversed for a RIGHT side, as Cons_Seq is)
struct HomologySide
{
  bool on = false;
  struct bk_junction_fit f = {0, 0, 0, 0, 0, 0, 0, 0};
  string hom_seq, ins_seq;
  uint32_t hom_len() const { return f.hom_fwd + f.hom_back; }
  string fields() const
  {
    if (!on) return "\t.\t.\t.\t.\t.\t.\t.";
    std::ostringstream o;
    o << "\t" << f.shift << "\t" << f.ins << "\t" << f.aligned << "\t" << f.mism << "\t" << hom_len() << "\t" << (hom_seq.empty() ? "." : hom_seq) << "\t"
      << (ins_seq.empty() ? "." : ins_seq);
    return o.str();
  }
};
// -clip -normal: what _fusion_rescued_normal.txt adds to a row of _fusion_rescued.txt
static const char *RESCUED_COLUMNS_NORMAL = "\tNormal_DRP\tNormal_ClipAt1\tNormal_ClipAt2\tNormal_Depth1\tNormal_Depth2";

// A rescued call: a row that _fusion_rescued.txt writes.  Its breakends are its two clip peaks, in the directions of
// bk_junction_sides; the normal's counts are filled with -normal (bk_clip_reads within 2 bp of the peaks, bk_base_depth at them).
struct RescuedCall
{
  uint8_t right[2] = {0, 1};
  uint32_t peak_n[2] = {0, 0};
  uint32_t normal_drp = 0, normal_at[2] = {0, 0}, normal_depth[2] = {0, 0};
};

// Which rows the fusion files hold, and with them -vcf and -evidence: `all_ok` rows go to _fusion_all.txt (-all), those that also pass
// the gene-pair and repeat filters to _fusion.txt.
static bool call_all_ok(const OutRow &r) { return r.c.n_sr > 0 && r.c.p1_exact != 0xFFFFFFFFu && r.c.p2_exact != -1; }
static bool call_no_gene_pair(const OutRow &r) { return (r.g1 == "intergenic" && r.g2 == "intergenic") || r.g1 == r.g2; }
static bool call_filt_ok(const OutRow &r) { return call_all_ok(r) && !call_no_gene_pair(r) && !r.is_rpt; }
static bool call_written(const OutRow &r, bool all) { return all ? call_all_ok(r) : call_filt_ok(r); }
// a rescued cluster has no split read (N_SR is 0): the gene-pair and repeat filters apply to it as to a call, lifted by -all
static bool rescued_written(const OutRow &r, bool all) { return all || (!call_no_gene_pair(r) && !r.is_rpt); }

// ---- -vcf: the calls of the fusion files as VCF 4.2 breakends (section 5.4), two records per call ------------------------------
struct VcfInput
{
  int nt = 0;
  const char *const *names = nullptr;
  const uint32_t *lens = nullptr;
  string nib_dir;
  bool all = false;                                   // -all: the rows of _fusion_all.txt, the filtered ones with a FILTER
  const vector<struct bk_junction> *jsup = nullptr;   // per BK_STAGE_CLUSTERS row
  bool with_normal = false;                           // -normal: a NORMAL sample column from nsup
  const struct bk_normal_support *nsup = nullptr;
  uint64_t n_nsup = 0;
  const vector<struct bk_ref_support> *gsup = nullptr, *gsup_normal = nullptr;  // -genotype (else null): GT:GQ:DR:DV:RR:RV
  // _fusion_rescued.vcf (else null): `rows` are the rescued clusters, rescued[k] belongs to rows[k]; the records get INFO/SC and a
  // third sample field CV, the clipped reads of the side, and are never genotyped
  const vector<RescuedCall> *rescued = nullptr;
  const vector<struct bk_unique_support> *usup = nullptr;  // -dedup (else null; never for the rescued clusters): INFO/UPE and INFO/USR, last
  // -consensus (else null; never for the rescued clusters): the two sides of every written call by its BK_STAGE_CLUSTERS row; INFO/CSEQ
  // and INFO/CSN behind everything else
  const std::map<uint64_t, std::pair<ConsensusSide, ConsensusSide>> *cons = nullptr;
  // -homology (else null; needs cons): the same for the junction fit; HOMLEN / HOMSEQ / JINS / JAL / JMM / JSH behind CSN
  const std::map<uint64_t, std::pair<HomologySide, HomologySide>> *hom = nullptr;
};

static char nib_base(const string &nib_dir, const string &chr, long pos1)  // the base at a 1-based position; N without a file or beyond it
{
  char b = 'N';
  if (pos1 < 1) return b;
  Nib n;
  n.open(nib_dir + "/hg19_" + chr + ".nib");
  n.base(&b, (unsigned long) (pos1 - 1));
  return b;
}

static string vcf_info_text(string s)  // an INFO value holds no blank, ';', '=' or ','
{
  for (char &c : s)
    if (c == ' ' || c == '\t' || c == ';' || c == '=' || c == ',') c = '_';
  return s.empty() ? "." : s;
}

// one sample column: DV:RV, or with the reference-allele counts GT:GQ:DR:DV:RR:RV (GT / GQ as in the *_genotype.txt twins: the call
// is genotyped on its junction reads; DR / RR are the counts of the record's own side)
static string vcf_sample(uint32_t n_drp, uint32_t n_sr, const struct bk_ref_support *rs, int side)
{
  std::ostringstream o;
  if (rs)
  {
    uint8_t gt = 255, gq = 0;
    float vaf = 0;
    bk_genotype_call(n_sr, (uint32_t) (((uint64_t) rs->ref_reads1 + rs->ref_reads2 + 1) / 2), &gt, &gq, &vaf);
    o << (gt == 0 ? "0/0" : gt == 1 ? "0/1" : gt == 2 ? "1/1" : "./.") << ":" << (int) gq << ":" << (side ? rs->ref_pairs2 : rs->ref_pairs1) << ":" << n_drp << ":"
      << (side ? rs->ref_reads2 : rs->ref_reads1) << ":" << n_sr;
  }
  else
    o << n_drp << ":" << n_sr;
  return o.str();
}

struct VcfRecord
{
  int tid;
  uint32_t pos;
  string id, line;
};

// false when an evidence table lacks a row of a call (nothing is written then)
static bool write_vcf(const string &path, const vector<OutRow> &rows, const VcfInput &in)
{
  vector<VcfRecord> recs;
  if (in.rescued && (in.rescued->size() != rows.size() || in.gsup || in.gsup_normal)) return false;
  for (size_t k = 0; k < rows.size(); ++k)
  {
    const OutRow &r = rows[k];
    const RescuedCall *rc = in.rescued ? &(*in.rescued)[k] : nullptr;
    if (rc ? !rescued_written(r, in.all) : !call_written(r, in.all)) continue;
    const bool no_gene_pair = call_no_gene_pair(r), filt_ok = rc ? !no_gene_pair && !r.is_rpt : call_filt_ok(r);
    if (r.idx >= in.jsup->size() || (in.with_normal && !rc && r.idx >= in.n_nsup) || (in.gsup && r.idx >= in.gsup->size()) ||
        (in.gsup_normal && r.idx >= in.gsup_normal->size()) || (in.usup && !rc && r.idx >= in.usup->size()) || (in.cons && !rc && !in.cons->count(r.idx)))
      return false;
    const struct bk_junction &j = (*in.jsup)[r.idx];
    uint8_t right[2] = {0, 1}, source = 0;
    bk_junction_sides(&j, &right[0], &right[1], &source);
    const uint64_t n_members = (uint64_t) j.pairs[0] + j.pairs[1] + j.pairs[2] + j.pairs[3];
    string filter = "PASS";
    if (!filt_ok) filter = no_gene_pair ? (r.is_rpt ? "NoGenePair;Repeat" : "NoGenePair") : "Repeat";
    const string id = "bk" + std::to_string(r.idx);
    for (int s = 0; s < 2; ++s)
    {
      const string &chr = s ? r.p2_chr : r.p1_chr, &mate_chr = s ? r.p1_chr : r.p2_chr;
      const uint32_t pos = s ? (uint32_t) r.c.p2_exact : r.c.p1_exact, mate_pos = s ? r.c.p1_exact : (uint32_t) r.c.p2_exact;
      const char ref = nib_base(in.nib_dir, chr, (long) pos);
      vector<char> alt(mate_chr.size() + 32);
      if (bk_vcf_breakend_alt(ref, right[s], mate_chr.c_str(), mate_pos, right[1 - s], alt.data(), alt.size()) != BK_OK) return false;
      std::ostringstream o;
      o << chr << "\t" << pos << "\t" << id << "_" << s + 1 << "\t" << ref << "\t" << alt.data() << "\t.\t" << filter << "\t";
      o << "SVTYPE=BND;MATEID=" << id << "_" << 2 - s << ";EVENTTYPE=" << fusion_type(r.c.type_mask) << ";PE=" << r.c.n_drp << ";SR=" << r.c.n_sr
        << ";MAPQ=" << (n_members ? (s ? j.mapq_sum2 : j.mapq_sum1) / n_members : 0) << ";DP=" << (s ? r.c.depth2 : r.c.depth1) << ";GENE=" << vcf_info_text(s ? r.g2 : r.g1)
        << ";SIDES=" << (source == 2 ? "SR" : source == 1 ? "PE" : "NONE");
      if (in.usup && !rc) o << ";UPE=" << (*in.usup)[r.idx].uniq_pairs << ";USR=" << (*in.usup)[r.idx].uniq_splits;
      if (rc)
      {
        o << ";SC=" << rc->peak_n[s] << "\tDV:RV:CV\t" << vcf_sample(r.c.n_drp, 0, nullptr, s) << ":" << rc->peak_n[s];
        if (in.with_normal) o << "\t" << vcf_sample(rc->normal_drp, 0, nullptr, s) << ":" << rc->normal_at[s];
      }
      else
      {
        if (in.cons)
        {
          const ConsensusSide &cs = s ? in.cons->at(r.idx).second : in.cons->at(r.idx).first;
          if (!cs.seq.empty()) o << ";CSEQ=" << cs.seq;
          o << ";CSN=" << cs.c.n_reads;
        }
        if (in.cons && in.hom && in.hom->count(r.idx))
        {
          const HomologySide &h = s ? in.hom->at(r.idx).second : in.hom->at(r.idx).first;
          if (h.on)
          {
            if (h.hom_len()) o << ";HOMLEN=" << h.hom_len() << ";HOMSEQ=" << h.hom_seq;
            if (!h.ins_seq.empty()) o << ";JINS=" << h.ins_seq;
            o << ";JAL=" << h.f.aligned << ";JMM=" << h.f.mism << ";JSH=" << h.f.shift;
          }
        }
        o << "\t" << (in.gsup ? "GT:GQ:DR:DV:RR:RV" : "DV:RV") << "\t" << vcf_sample(r.c.n_drp, r.c.n_sr, in.gsup ? &(*in.gsup)[r.idx] : nullptr, s);
        if (in.with_normal) o << "\t" << vcf_sample(in.nsup[r.idx].n_drp, in.nsup[r.idx].n_sr, in.gsup_normal ? &(*in.gsup_normal)[r.idx] : nullptr, s);
      }
      o << "\n";
      VcfRecord rec;
      rec.tid = s ? r.c.p2_tid : r.c.p1_tid;
      rec.pos = pos;
      rec.id = id + "_" + std::to_string(s + 1);
      rec.line = o.str();
      recs.push_back(rec);
    }
  }
  std::sort(recs.begin(), recs.end(), [](const VcfRecord &a, const VcfRecord &b) {
    if (a.tid != b.tid) return a.tid < b.tid;
    if (a.pos != b.pos) return a.pos < b.pos;
    return a.id < b.id;
  });
  std::ofstream v(path.c_str());
  // no date and no command line: two runs write the same bytes
  v << "##fileformat=VCFv4.2\n##source=BreakID\n";
  for (int t = 0; t < in.nt; ++t) v << "##contig=<ID=" << in.names[t] << ",length=" << in.lens[t] << ">\n";
  v << "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n"
       "##INFO=<ID=MATEID,Number=1,Type=String,Description=\"ID of the mate breakend\">\n"
       "##INFO=<ID=EVENTTYPE,Number=1,Type=String,Description=\"Fusion_Type of the call in the fusion tables\">\n"
       "##INFO=<ID=PE,Number=1,Type=Integer,Description=\"Discordant read pairs of the call (N_DRP)\">\n"
       "##INFO=<ID=SR,Number=1,Type=Integer,Description=\"Split reads of the call (N_SR)\">\n"
       "##INFO=<ID=MAPQ,Number=1,Type=Integer,Description=\"Mean mapping quality of the member pairs' reads on this side\">\n"
       "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Read depth at this breakpoint\">\n"
       "##INFO=<ID=GENE,Number=1,Type=String,Description=\"Gene at this breakpoint, or intergenic\">\n"
       "##INFO=<ID=SIDES,Number=1,Type=String,Description=\"Evidence the breakend orientation comes from: SR split reads, PE read pairs, NONE\">\n";
  if (in.usup && !in.rescued)
    v << "##INFO=<ID=UPE,Number=1,Type=Integer,Description=\"Different fragments among the discordant read pairs of the call\">\n"
         "##INFO=<ID=USR,Number=1,Type=Integer,Description=\"Different fragments among the split-read alignments of the call\">\n";
  if (in.cons && !in.rescued)
    v << "##INFO=<ID=CSEQ,Number=1,Type=String,Description=\"Consensus of the bases soft-clipped at this breakpoint, in the orientation of the alignments\">\n"
         "##INFO=<ID=CSN,Number=1,Type=Integer,Description=\"Reads soft-clipped exactly at this breakpoint that the consensus was voted from\">\n";
  if (in.cons && in.hom && !in.rescued)
    v << "##INFO=<ID=HOMLEN,Number=1,Type=Integer,Description=\"Length of base pair identical micro-homology at event breakpoints\">\n"
         "##INFO=<ID=HOMSEQ,Number=1,Type=String,Description=\"Sequence of base pair identical micro-homology at event breakpoints\">\n"
         "##INFO=<ID=JINS,Number=1,Type=String,Description=\"Bases between the two sides that neither templates, in the orientation of the alignments at this breakpoint\">\n"
         "##INFO=<ID=JAL,Number=1,Type=Integer,Description=\"Bases of CSEQ placed in the reference at the mate breakpoint\">\n"
         "##INFO=<ID=JMM,Number=1,Type=Integer,Description=\"Mismatches among the JAL placed bases\">\n"
         "##INFO=<ID=JSH,Number=1,Type=Integer,Description=\"Offset of the placed sequence from the mate breakpoint, in bases into the mate's retained sequence\">\n";
  if (in.rescued) v << "##INFO=<ID=SC,Number=1,Type=Integer,Description=\"Soft-clipped reads without an SA tag that end at this position (the clip peak)\">\n";
  if (in.gsup)
    v << "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
         "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality\">\n"
         "##FORMAT=<ID=DR,Number=1,Type=Integer,Description=\"Reference read pairs that span this breakpoint\">\n";
  v << "##FORMAT=<ID=DV,Number=1,Type=Integer,Description=\"Discordant read pairs that support the call\">\n";
  if (in.gsup) v << "##FORMAT=<ID=RR,Number=1,Type=Integer,Description=\"Reference reads across this breakpoint\">\n";
  v << "##FORMAT=<ID=RV,Number=1,Type=Integer,Description=\"Split reads that support the call\">\n";
  if (in.rescued) v << "##FORMAT=<ID=CV,Number=1,Type=Integer,Description=\"Soft-clipped reads without an SA tag at this breakpoint\">\n";
  v << "##FILTER=<ID=PASS,Description=\"All filters passed\">\n";
  if (in.all)
    v << "##FILTER=<ID=NoGenePair,Description=\"Both sides intergenic, or both in the same gene\">\n"
         "##FILTER=<ID=Repeat,Description=\"A homopolymer run above 10 in the sequence next to a breakpoint\">\n";
  v << "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tTUMOR" << (in.with_normal ? "\tNORMAL" : "") << "\n";
  for (const VcfRecord &rec : recs) v << rec.line;
  return v.good();
}

// ---- -evidence: the reads behind the written calls: <prefix>_evidence.txt and <prefix>_evidence.bam ------------------------------
struct EvidenceInput
{
  int nt = 0;
  const char *const *names = nullptr;
  bool all = false;  // -all: the calls of _fusion_all.txt
  const vector<struct bk_evidence> *rows = nullptr;
  const vector<uint64_t> *call_off = nullptr;  // per BK_STAGE_CLUSTERS row, one more entry than rows
  const vector<uint64_t> *first = nullptr;     // -dedup (else null): bk_unique_support's first[], a last column Dup in _evidence.txt
};

// One listed read of a call: the hashes of its name, and the call (bk<call>) it stands behind
struct ReadRef
{
  uint64_t qhash;
  uint32_t qcheck;
  uint64_t call;
};
// the names bk_bam_extract gave back, by (qhash, qcheck)
struct ReadNames
{
  std::map<std::pair<uint64_t, uint32_t>, size_t> key_of;
  vector<const char *> name_of;
  char *names = nullptr;
  ~ReadNames() { bk_bam_names_free(names); }
  const char *operator()(uint64_t qhash, uint32_t qcheck) const
  {
    const char *name = name_of[key_of.at(std::make_pair(qhash, qcheck))];
    return *name ? name : ".";
  }
};

// One pass over the input BAM (bk_bam_extract) gives the names of the listed reads and writes every alignment of theirs to out_bam,
// tagged bk:Z:<the read's call ids, ascending, joined with commas>.  `refs` comes with its calls ascending.
static bool extract_reads(const string &inp_bam, const string &out_bam, const vector<ReadRef> &refs, ReadNames &rn, string &why)
{
  // the unique reads and, per read, its calls (ascending, each once)
  vector<bk_read_key> keys;
  vector<vector<uint64_t>> key_calls;
  for (const ReadRef &e : refs)
  {
    auto it = rn.key_of.emplace(std::make_pair(e.qhash, e.qcheck), keys.size());
    if (it.second)
    {
      keys.push_back(bk_read_key{e.qhash, e.qcheck, 0});
      key_calls.emplace_back();
    }
    vector<uint64_t> &kc = key_calls[it.first->second];
    if (kc.empty() || kc.back() != e.call) kc.push_back(e.call);
  }
  std::map<string, uint32_t> tag_of;
  vector<string> tag_text;
  for (size_t k = 0; k < keys.size(); ++k)
  {
    string t;
    for (uint64_t c : key_calls[k]) t += (t.empty() ? "bk" : ",bk") + std::to_string(c);
    auto it = tag_of.emplace(t, (uint32_t) tag_text.size());
    if (it.second) tag_text.push_back(t);
    keys[k].tag = it.first->second;
  }
  vector<const char *> tag_ptrs;
  for (const string &t : tag_text) tag_ptrs.push_back(t.c_str());
  char err[512] = "";
  if (bk_bam_extract(inp_bam.c_str(), out_bam.c_str(), keys.data(), keys.size(), tag_ptrs.data(), tag_ptrs.size(), &rn.names, nullptr, err, sizeof err) != BK_OK)
  {
    why = err;
    return false;
  }
  rn.name_of.assign(keys.size(), "");
  const char *p = rn.names;
  for (size_t k = 0; k < keys.size(); ++k)
  {
    rn.name_of[k] = p;
    p += strlen(p) + 1;
  }
  return true;
}

static const char *EVIDENCE_HEADER = "Call\tKind\tRead\tChr1\tPos1\tChr2\tPos2\tSides\tFlag1\tFlag2\tMapq1\tMapq2\tRecord";

static void write_evidence_line(std::ostream &o, uint64_t c, const struct bk_evidence &e, const ReadNames &rn, const EvidenceInput &in)
{
  auto chr = [&](int32_t tid) { return tid < 0 || tid >= in.nt ? "*" : in.names[tid]; };
  o << "bk" << c << "\t" << (e.kind == BK_EV_PAIR ? "PE" : "SR") << "\t" << rn(e.qhash, e.qcheck) << "\t" << chr(e.tid1) << "\t" << e.pos1 << "\t" << chr(e.tid2) << "\t"
    << e.pos2 << "\t" << ((e.sides >> 1) & 1 ? 'R' : 'L') << ((e.sides & 1) ? 'R' : 'L') << "\t" << e.flag1 << "\t" << e.flag2 << "\t" << (unsigned) e.mapq1 << "\t"
    << (unsigned) e.mapq2 << "\t" << e.rec;
}

// both files or neither
static bool close_evidence(std::ofstream &o, const string &txt, const string &bam, string &why)
{
  o.close();
  if (o) return true;
  (void) remove(txt.c_str());
  (void) remove(bam.c_str());
  why = "cannot write " + txt;
  return false;
}

// The calls covered are those of -vcf, with its ids (bk<row>).
static bool write_evidence(const string &prefix, const string &inp_bam, const vector<OutRow> &rows, const EvidenceInput &in, string &why)
{
  vector<uint64_t> calls;
  for (const OutRow &r : rows)
  {
    if (!call_written(r, in.all)) continue;
    if (r.idx + 1 >= in.call_off->size() || (*in.call_off)[r.idx + 1] > in.rows->size())
    {
      why = "the evidence table does not cover every call";
      return false;
    }
    calls.push_back(r.idx);
  }
  std::sort(calls.begin(), calls.end());  // ABI order: by row
  vector<ReadRef> refs;
  for (uint64_t c : calls)
    for (uint64_t i = (*in.call_off)[c]; i < (*in.call_off)[c + 1]; ++i) refs.push_back(ReadRef{(*in.rows)[i].qhash, (*in.rows)[i].qcheck, c});
  if (in.first && in.first->size() != in.rows->size())
  {
    why = "the unique-support listing does not cover every evidence row";
    return false;
  }
  ReadNames rn;
  if (!extract_reads(inp_bam, prefix + "_evidence.bam", refs, rn, why)) return false;
  std::ofstream o((prefix + "_evidence.txt").c_str());
  o << EVIDENCE_HEADER << (in.first ? "\tDup" : "") << "\n";
  for (uint64_t c : calls)
    for (uint64_t i = (*in.call_off)[c]; i < (*in.call_off)[c + 1]; ++i)
    {
      write_evidence_line(o, c, (*in.rows)[i], rn, in);
      if (in.first) o << "\t" << ((*in.first)[i] == i ? 0 : 1);  // 0 on a fragment's first line
      o << "\n";
    }
  return close_evidence(o, prefix + "_evidence.txt", prefix + "_evidence.bam", why);
}

// -clip -evidence: the reads behind the rescued calls: <prefix>_evidence_rescued.txt and <prefix>_evidence_rescued.bam.  Per call, ids
// ascending: its member pairs (the BK_EV_PAIR rows of bk_evidence: an unvoted row has no others), then the reads clipped exactly at
// its two peaks (bk_clip_reads, tol 0), side 1 before side 2.  `rescued` / `calls`: the rescued clusters and their RescuedCall;
// clip rows of sites 2 * j and 2 * j + 1 belong to the j-th written one of them.
static bool write_evidence_rescued(const string &prefix, const string &inp_bam, const vector<OutRow> &rescued, const vector<RescuedCall> &calls, const EvidenceInput &in,
                                   const vector<struct bk_clip_read> &clip_rows, const vector<uint64_t> &site_off, string &why)
{
  struct Item
  {
    uint64_t call;
    size_t k, j;  // index into rescued, ordinal among the written
  };
  vector<Item> items;
  for (size_t k = 0; k < rescued.size(); ++k)
  {
    const OutRow &r = rescued[k];
    if (!rescued_written(r, in.all)) continue;
    const size_t j = items.size();
    if (r.idx + 1 >= in.call_off->size() || (*in.call_off)[r.idx + 1] > in.rows->size() || 2 * j + 2 >= site_off.size() || site_off[2 * j + 2] > clip_rows.size())
    {
      why = "the evidence tables do not cover every rescued call";
      return false;
    }
    items.push_back(Item{r.idx, k, j});
  }
  std::sort(items.begin(), items.end(), [](const Item &a, const Item &b) { return a.call < b.call; });
  vector<ReadRef> refs;
  for (const Item &it : items)
  {
    for (uint64_t i = (*in.call_off)[it.call]; i < (*in.call_off)[it.call + 1]; ++i) refs.push_back(ReadRef{(*in.rows)[i].qhash, (*in.rows)[i].qcheck, it.call});
    for (uint64_t i = site_off[2 * it.j]; i < site_off[2 * it.j + 2]; ++i) refs.push_back(ReadRef{clip_rows[i].qhash, clip_rows[i].qcheck, it.call});
  }
  const string txt = prefix + "_evidence_rescued.txt", bam = prefix + "_evidence_rescued.bam";
  ReadNames rn;
  if (!extract_reads(inp_bam, bam, refs, rn, why)) return false;
  std::ofstream o(txt.c_str());
  o << EVIDENCE_HEADER << "\tClip\n";
  auto chr = [&](int32_t tid) { return tid < 0 || tid >= in.nt ? "*" : in.names[tid]; };
  for (const Item &it : items)
  {
    const OutRow &r = rescued[it.k];
    for (uint64_t i = (*in.call_off)[it.call]; i < (*in.call_off)[it.call + 1]; ++i)
    {
      write_evidence_line(o, it.call, (*in.rows)[i], rn, in);
      o << "\t.\n";
    }
    for (int s = 0; s < 2; ++s)
      for (uint64_t i = site_off[2 * it.j + s]; i < site_off[2 * it.j + s + 1]; ++i)
      {
        const struct bk_clip_read &e = clip_rows[i];
        o << "bk" << it.call << "\tSC\t" << rn(e.qhash, e.qcheck) << "\t" << chr(e.tid) << "\t" << e.p << "\t" << (s ? r.p1_chr : r.p2_chr) << "\t"
          << (s ? r.c.p1_exact : (uint32_t) r.c.p2_exact) << "\t" << s + 1 << (calls[it.k].right[s] ? 'R' : 'L') << "\t" << e.flag << "\t0\t" << (unsigned) e.mapq << "\t0\t"
          << e.rec << "\t" << e.clip_len << "\n";
      }
  }
  return close_evidence(o, txt, bam, why);
}

// one input BAM: its decoded table (host or device) and, once created, its context
struct Sample
{
  string path;
  bk_bam *bam = nullptr;
  bk_bam_dev *dbam = nullptr;
  int nt = 0;
  const char *const *names = nullptr;
  const uint32_t *lens = nullptr;
  bk_soa soa{};
  int soa_where = BK_MEM_HOST;
  bk_ctx *ctx = nullptr;
  // a copy of the reference list, so that the decoded table can be released once the context holds its kept records (-x)
  vector<string> name_copy;
  vector<const char *> name_ptrs;
  vector<uint32_t> len_copy;
  void own_header()
  {
    name_copy.assign(names, names + nt);
    len_copy.assign(lens, lens + nt);
    name_ptrs.clear();
    for (auto &n : name_copy) name_ptrs.push_back(n.c_str());
    names = name_ptrs.data();
    lens = len_copy.data();
  }
};

int main(int argc, char *argv[])
{
  clock_t start = clock();
  static struct option longopts[] = {{"help", 0, 0, 'h'}, {"i", 1, 0, 1}, {"o", 1, 0, 2}, {"q", 1, 0, 3}, {"n", 1, 0, 4},
                                     {"fast", 0, 0, 5},   {"t", 0, 0, 6}, {"all", 0, 0, 7}, {"gpu", 1, 0, 8}, {"gpus", 1, 0, 9},
                                     {"comm", 1, 0, 10},  {"normal", 1, 0, 11}, {"x", 1, 0, 12}, {"genotype", 0, 0, 13},
                                     {"anchor", 1, 0, 14}, {"vcf", 0, 0, 15}, {"evidence", 0, 0, 16}, {"clip", 0, 0, 17},
                                     {"minclip", 1, 0, 18}, {"clipsupport", 1, 0, 19}, {"dedup", 0, 0, 20}, {"consensus", 0, 0, 21},
                                     {"conslen", 1, 0, 22}, {"homology", 0, 0, 23}, {"homshift", 1, 0, 24}, {"homins", 1, 0, 25}, {0, 0, 0, 0}};
  string inp_file, out_file, nib_dir, normal_file, exclude_file, build = "hg19";
  int qual = 20, device = 0, n_gpus = 0, transport = BK_TRANSPORT_AUTO;  // -gpus N: one sample over N GPUs (include/breakid_multi.h)
  bool fast = false, filter = true, genotype = false, anchor_given = false, vcf = false, evidence = false;
  bool clip = false, minclip_given = false, clipsupport_given = false, dedup = false;
  bool consensus = false, conslen_given = false;
  long conslen = 64;  // -conslen: longest junction sequence per side
  bool homology = false, homshift_given = false, homins_given = false;
  long homshift = 32, homins = 32;  // -homshift, -homins: the largest offset and the longest insertion bk_junction_fit looks for
  long min_clip = 10, clip_support = 3;  // -minclip: shortest clip that counts; -clipsupport: reads at one position a rescued side needs
  long anchor = 10;  // -anchor: bases a reference read must cover on either side of the breakpoint base
  int opt, li;
  optind = 0;
  while ((opt = getopt_long_only(argc, argv, "h?", longopts, &li)) != -1)
  {
    switch (opt)
    {
    case 'h': case '?': std::cerr << HELP; exit(1);
    case 1: inp_file = optarg; break;
    case 2: out_file = optarg; break;
    case 3: qual = (int) std::labs(atol(optarg)); break;
    case 4: nib_dir = optarg; break;
    case 5: fast = true; break;
    case 6: break;  // the reference dereferences a NULL optarg here (has_arg = 0); `times` is effectively always 2
    case 7: filter = false; break;
    case 8: device = atoi(optarg); break;
    case 9: n_gpus = atoi(optarg); break;
    case 10: transport = !strcmp(optarg, "rccl") ? BK_TRANSPORT_RCCL : !strcmp(optarg, "local") ? BK_TRANSPORT_LOCAL : BK_TRANSPORT_AUTO; break;
    case 11: normal_file = optarg; break;
    case 12: exclude_file = optarg; break;
    case 13: genotype = true; break;
    case 14:
      anchor = atol(optarg);
      anchor_given = true;
      break;
    case 15: vcf = true; break;
    case 16: evidence = true; break;
    case 17: clip = true; break;
    case 18:
      min_clip = atol(optarg);
      minclip_given = true;
      break;
    case 19:
      clip_support = atol(optarg);
      clipsupport_given = true;
      break;
    case 20: dedup = true; break;
    case 21: consensus = true; break;
    case 22:
      conslen = atol(optarg);
      conslen_given = true;
      break;
    case 23: homology = true; break;
    case 24:
      homshift = atol(optarg);
      homshift_given = true;
      break;
    case 25:
      homins = atol(optarg);
      homins_given = true;
      break;
    default: std::cerr << "Error: cannot parse arguments.\n"; exit(1);
    }
  }
  if (inp_file.empty() || out_file.empty())
  {
    std::cerr << HELP << "Error: input- and output file is required.\n";
    exit(1);
  }
  if (nib_dir.empty())
  {
    std::cerr << HELP << "Error: nib file's root dir is required.\n";
    exit(1);
  }
  if (!normal_file.empty())
  {
    if (n_gpus >= 1)
    {
      std::cerr << HELP << "Error: -normal cannot be combined with -gpus.\n";
      exit(1);
    }
    if (!bk_normal_support)
    {
      std::cerr << "Error: -normal needs the GPU library" << std::endl;
      exit(1);
    }
    FILE *probe = fopen(normal_file.c_str(), "rb");
    if (!probe)
    {
      std::cerr << "Error: can not open normal bam-file: " << normal_file << std::endl;
      exit(1);
    }
    fclose(probe);
  }
  if (anchor_given && !genotype)
  {
    std::cerr << HELP << "Error: -anchor needs -genotype.\n";
    exit(1);
  }
  if (genotype)
  {
    if (n_gpus >= 1)
    {
      std::cerr << HELP << "Error: -genotype cannot be combined with -gpus.\n";
      exit(1);
    }
    if (anchor < 0 || anchor > 0x7FFFFFFFl)
    {
      std::cerr << HELP << "Error: -anchor must be a number from 0 to 2147483647.\n";
      exit(1);
    }
    if (!bk_ref_support || !bk_genotype_call)
    {
      std::cerr << "Error: -genotype needs the GPU library" << std::endl;
      exit(1);
    }
  }
  if (vcf)
  {
    if (n_gpus >= 1)
    {
      std::cerr << HELP << "Error: -vcf cannot be combined with -gpus.\n";
      exit(1);
    }
    if (!bk_junctions || !bk_junction_sides || !bk_vcf_breakend_alt)
    {
      std::cerr << "Error: -vcf needs the GPU library" << std::endl;
      exit(1);
    }
  }
  if (evidence)
  {
    if (n_gpus >= 1)
    {
      std::cerr << HELP << "Error: -evidence cannot be combined with -gpus.\n";
      exit(1);
    }
    if (!bk_evidence)
    {
      std::cerr << "Error: -evidence needs the GPU library" << std::endl;
      exit(1);
    }
  }
  if (dedup)
  {
    if (n_gpus >= 1)
    {
      std::cerr << HELP << "Error: -dedup cannot be combined with -gpus.\n";
      exit(1);
    }
    if (!bk_unique_support)
    {
      std::cerr << "Error: -dedup needs the GPU library" << std::endl;
      exit(1);
    }
  }
  if ((homshift_given || homins_given) && !homology)
  {
    std::cerr << HELP << "Error: -homshift and -homins need -homology.\n";
    exit(1);
  }
  if (homology)
  {
    if (!consensus)
    {
      std::cerr << HELP << "Error: -homology needs -consensus.\n";
      exit(1);
    }
    if (n_gpus >= 1)
    {
      std::cerr << HELP << "Error: -homology cannot be combined with -gpus.\n";
      exit(1);
    }
    if (!bk_junction_fit)
    {
      std::cerr << "Error: -homology needs the GPU library" << std::endl;
      exit(1);
    }
    if (homshift < 0 || homshift > 64 || homins < 0 || homins > 64)
    {
      std::cerr << HELP << "Error: -homshift and -homins must be numbers from 0 to 64.\n";
      exit(1);
    }
  }
  if (conslen_given && !consensus)
  {
    std::cerr << HELP << "Error: -conslen needs -consensus.\n";
    exit(1);
  }
  if (consensus)
  {
    if (n_gpus >= 1)
    {
      std::cerr << HELP << "Error: -consensus cannot be combined with -gpus.\n";
      exit(1);
    }
    if (!bk_clip_consensus || !bk_clip_reads || !bk_evidence || !bk_junctions || !bk_junction_sides)
    {
      std::cerr << "Error: -consensus needs the GPU library" << std::endl;
      exit(1);
    }
    if (conslen < 1 || conslen > 256)
    {
      std::cerr << HELP << "Error: -conslen must be a number from 1 to 256.\n";
      exit(1);
    }
    if (min_clip < 1 || min_clip > 0x7FFFFFFFl)
    {
      std::cerr << HELP << "Error: -minclip must be a number from 1 to 2147483647.\n";
      exit(1);
    }
  }
  if ((minclip_given && !clip && !consensus) || (clipsupport_given && !clip))
  {
    std::cerr << HELP << "Error: -minclip and -clipsupport need -clip.\n";
    exit(1);
  }
  if (clip)
  {
    if (!bk_clip_support || !bk_clip_reads || !bk_base_depth || !bk_clip_rescue || !bk_junctions || !bk_junction_sides)
    {
      std::cerr << "Error: -clip needs the GPU library" << std::endl;
      exit(1);
    }
    if (n_gpus >= 1)
    {
      std::cerr << HELP << "Error: -clip cannot be combined with -gpus.\n";
      exit(1);
    }
    if (min_clip < 1 || min_clip > 0x7FFFFFFFl || clip_support < 1 || clip_support > 0x7FFFFFFFl)
    {
      std::cerr << HELP << "Error: -minclip and -clipsupport must be numbers from 1 to 2147483647.\n";
      exit(1);
    }
  }
  const bool exclude = !exclude_file.empty();
  if (exclude)
  {
    if (!bk_exclude_regions || !bk_multi_run_ex || !bk_multi_run_bam_ex || !bk_multi_excluded)
    {
      std::cerr << "Error: -x needs the GPU library" << std::endl;
      exit(1);
    }
    std::ifstream probe(exclude_file.c_str());
    if (!probe.is_open())
    {
      std::cerr << "Error: can not open exclude file: " << exclude_file << std::endl;
      exit(1);
    }
  }
  std::cout << "start to stats the insert size...\n";
  // feed: the GPU decoder first (BGZF inflate + record decode on the device; every htslib-written BAM qualifies), the
  // host decoder (all cores, pinned columns) for files whose records straddle BGZF blocks or that exceed one batch.
  // BREAKID_HOST_DECODE=1 forces the host path.
  char err[512];
  Sample tumor, normal;
  tumor.path = inp_file;
  normal.path = normal_file;
  int &nt = tumor.nt;
  const char *const *&names = tumor.names;
  const uint32_t *&lens = tumor.lens;
  bk_soa &soa = tumor.soa;
  int &soa_where = tumor.soa_where;
  {
    FILE *probe = fopen(inp_file.c_str(), "rb");
    if (!probe)
    {
      std::cerr << "Error: can not open bam-file: " << inp_file << std::endl;
      exit(1);
    }
    fclose(probe);
  }
  // -x: the list is read against the file's reference list before anything is decoded
  ExcludeList xl;
  bk_regions regions{};
  if (exclude)
  {
    vector<string> hn;
    vector<uint32_t> hl;
    if (!bam_header_list(inp_file, hn, hl))
    {
      std::cerr << "Error: can not read the header of bam-file: " << inp_file << std::endl;
      exit(1);
    }
    xl = read_exclude_bed(exclude_file, hn, hl);
    regions.tid = xl.tid.data();
    regions.beg = xl.beg.data();
    regions.end = xl.end.data();
    regions.n = xl.tid.size();
  }
  uint64_t n_excluded = 0, n_excluded_normal = 0;
  const bool multi = n_gpus >= 1;  // the sharded run: every rank decodes its part of the file on its own GPU (below), or takes its range of the host table
  bk_ctx *&ctx = tumor.ctx;
  auto host_decode_sample = [&](Sample &s) {
    s.dbam = nullptr;
    if (bk_bam_open(s.path.c_str(), &s.bam, err, sizeof err) != BK_OK)
    {
      std::cerr << "Error: can not open bam-file: " << s.path << std::endl;
      exit(1);
    }
    bk_bam_header(s.bam, &s.nt, &s.names, &s.lens);
    if (bk_bam_decode(s.bam, &s.soa, err, sizeof err) != BK_OK)
    {
      std::cerr << "Error: " << err << std::endl;
      exit(1);
    }
  };
  auto host_decode = [&] { host_decode_sample(tumor); };
  // one read of the file: BGZF inflate + record decode on the device, the stream pass of the hot path running on the chunks
  // already decoded while the rest of the file is still arriving (the reference reads the BAM twice, BreakID.cc:1929, :1414);
  // false when the GPU feed refuses the file (or BREAKID_HOST_DECODE=1): the host decoder takes it then
  auto gpu_decode = [&](Sample &s) {
    if (exclude)
    {
      // -x: the table first (bk_init, bk_upload_records and bk_exclude_regions follow), the stream pass after the exclusion
      if (getenv("BREAKID_HOST_DECODE") || bk_bam_decode_device(s.path.c_str(), device, &s.dbam, &s.soa, &s.nt, &s.names, &s.lens, err, sizeof err) != BK_OK)
      {
        s.dbam = nullptr;
        return false;
      }
    }
    else if (getenv("BREAKID_HOST_DECODE") ||
             bk_bam_decode_device_ctx(s.path.c_str(), device, qual, &s.dbam, &s.ctx, &s.nt, &s.names, &s.lens, err, sizeof err) != BK_OK)
      return false;
    s.soa_where = BK_MEM_DEVICE;
    return true;
  };
  // -x: context, upload, exclusion; then the decoded table goes (the context holds the kept records), the reference list stays as a copy
  auto exclude_sample = [&](Sample &s) {
    uint64_t removed = 0;
    s.own_header();
    if (!s.ctx)
    {
      if (bk_init(device, s.lens, s.names, s.nt, &s.ctx) != BK_OK)
      {
        std::cerr << "Error: " << bk_last_error(nullptr) << std::endl;
        exit(1);
      }
      if (bk_upload_records(s.ctx, &s.soa, s.soa_where) != BK_OK || bk_exclude_regions(s.ctx, &regions, &removed) != BK_OK)
      {
        std::cerr << "Error: " << s.path << ": " << bk_last_error(s.ctx) << std::endl;
        exit(1);
      }
    }
    if (s.dbam) bk_bam_dev_free(s.dbam);
    if (s.bam) bk_bam_close(s.bam);
    s.dbam = nullptr;
    s.bam = nullptr;
    s.soa = bk_soa{};
    return removed;
  };
  const bool multi_from_file = multi && !getenv("BREAKID_HOST_DECODE");
  if (!multi && gpu_decode(tumor))
  {
    // the feed's staging buffers and slots (1-2.5 GB of device memory) go back once the last file of the process is decoded
    if (normal_file.empty()) bk_feed_release_caches();
  }
  else if (!multi_from_file)
    host_decode();
  if (exclude && !multi) n_excluded = exclude_sample(tumor);
  {
    std::ifstream rn((nib_dir + "/ref_names.txt").c_str());
    if (!rn.is_open())
    {
      std::cerr << "Error: cannot open reference names file.\n";
      exit(1);
    }
  }
  auto die = [&](int rc) {
    std::cerr << (rc == BK_ERR_CIGAR ? "error cigar: " : bk_last_error(ctx)) << std::endl;
    exit(rc == BK_ERR_CIGAR ? -1 : 1);
  };
  int rc;
  double w = 0;
  clock_t scan_start = clock(), scan_end = scan_start, cluster_start = scan_start, cluster_end = scan_start, bp_start = scan_start, bp_end = scan_start;
  uint64_t n_pairs = 0, n_clustered = 0, n_valid = 0, n_clusters = 0;
  uint32_t n_groups = 0;
  auto need_index = [&] {  // findEncompassingReadsAndBreakPointInfo loads the index for every group that reaches it (:405-416)
    if (!index_loads(inp_file))
    {
      std::cerr << "Error: please index bam-file first:\t" << inp_file << std::endl;
      exit(1);
    }
  };
  if (multi)
  {
    // one sample over n_gpus GPUs: record ranges per rank, RCCL (or in-process) exchange of the small tables
    // the GPU feed per rank first (bk_bam_decode_device_part); files it cannot cut into parts (records across BGZF blocks) and
    // anything else it refuses go through the host decoder and the record ranges of its table
    rc = BK_ERR_IO;
    // (-x: the _ex entry points, every rank excludes on its own table before the record bases are counted)
    if (multi_from_file)
      rc = exclude ? bk_multi_run_bam_ex(inp_file.c_str(), &regions, n_gpus, transport, qual, fast ? 1 : 0, &w, &n_clustered, &ctx, &nt, &names, &lens, err, sizeof err)
                   : bk_multi_run_bam(inp_file.c_str(), n_gpus, transport, qual, fast ? 1 : 0, &w, &n_clustered, &ctx, &nt, &names, &lens, err, sizeof err);
    if (rc != BK_OK && (!multi_from_file || rc == BK_ERR_IO || rc == BK_ERR_LIMIT))
    {
      host_decode();
      rc = exclude ? bk_multi_run_ex(&soa, lens, names, nt, &regions, n_gpus, transport, qual, fast ? 1 : 0, &w, &n_clustered, &ctx, err, sizeof err)
                   : bk_multi_run(&soa, lens, names, nt, n_gpus, transport, qual, fast ? 1 : 0, &w, &n_clustered, &ctx, err, sizeof err);
    }
    if (rc != BK_OK)
    {
      std::cerr << (rc == BK_ERR_CIGAR ? "error cigar: " : err) << std::endl;
      exit(rc == BK_ERR_CIGAR ? -1 : 1);
    }
    if (exclude)
    {
      (void) bk_multi_excluded(ctx, &n_excluded);
      std::cout << "excluded " << n_excluded << " records overlapping " << xl.tid.size() << " intervals of " << exclude_file << "\n";
    }
    double mean = 0, sd = 0;
    (void) bk_multi_stats(ctx, &mean, &sd, nullptr, nullptr);
    std::cout << "the insert size mean: " << mean << ", the insert size sd:" << sd << " .\n";
    std::cout << "cluster_dist = span_dist = mask_dist = scan_dist = " << w << " .\n";
    std::cout << "Scanning discordant read pairs ...\n";
    std::cout << "Scanning discordant read pairs done.\n";
    if (n_clustered) need_index();
  }
  else
  {
    if (!ctx)  // host decoder: the table is uploaded now (the GPU feed has attached it and run the stream pass already)
    {
      if (bk_init(device, lens, names, nt, &ctx) != BK_OK)
      {
        std::cerr << "Error: " << bk_last_error(nullptr) << std::endl;
        exit(1);
      }
      if ((rc = bk_upload_records(ctx, &soa, soa_where)) != BK_OK) die(rc);
    }
    if (exclude) std::cout << "excluded " << n_excluded << " records overlapping " << xl.tid.size() << " intervals of " << exclude_file << "\n";
    double mean = 0, sd = 0;
    if ((rc = bk_isize_stats(ctx, &mean, &sd)) != BK_OK) die(rc);
    std::cout << "the insert size mean: " << mean << ", the insert size sd:" << sd << " .\n";
    const int times = 2;
    w = times * std::sqrt(times) * (mean + 3 * sd);
    std::cout << "cluster_dist = span_dist = mask_dist = scan_dist = " << w << " .\n";
    scan_start = clock();
    std::cout << "Scanning discordant read pairs ...\n";
    if ((rc = bk_discordant_pairs(ctx, qual, w, &n_pairs, &n_groups)) != BK_OK) die(rc);
    std::cout << "Scanning discordant read pairs done.\n";
    scan_end = clock();
    cluster_start = clock();
    if ((rc = bk_mask_and_cluster(ctx, w, fast ? 1 : 0, &n_clustered)) != BK_OK) die(rc);
    cluster_end = clock();
    bp_start = clock();
    if ((rc = bk_split_evidence(ctx, nullptr)) != BK_OK) die(rc);
    if ((rc = bk_cluster_summary(ctx, w, &n_clusters)) != BK_OK) die(rc);
    if (n_clustered) need_index();
    if ((rc = bk_split_breakpoints(ctx, w, &n_valid)) != BK_OK) die(rc);
    bp_end = clock();
  }
  // matched normal: decoded now (both record tables stay resident), then only its record-level stages and the per-call search
  const struct bk_normal_support *nsup = nullptr;
  uint64_t n_nsup = 0;
  if (!normal_file.empty())
  {
    if (!gpu_decode(normal)) host_decode_sample(normal);
    bk_feed_release_caches();
    bool same = normal.nt == nt;
    for (int i = 0; same && i < nt; ++i) same = !strcmp(normal.names[i], names[i]) && normal.lens[i] == lens[i];
    if (!same)
    {
      std::cerr << "Error: tumor and normal BAM headers differ" << std::endl;
      exit(1);
    }
    if (exclude)
    {
      n_excluded_normal = exclude_sample(normal);
      std::cout << "excluded " << n_excluded_normal << " records of the normal overlapping " << xl.tid.size() << " intervals of " << exclude_file << "\n";
    }
    auto die_normal = [&] {
      std::cerr << "Error: normal " << normal.path << ": " << bk_last_error(normal.ctx) << std::endl;
      exit(1);
    };
    if (!normal.ctx)
    {
      if (bk_init(device, normal.lens, normal.names, normal.nt, &normal.ctx) != BK_OK)
      {
        std::cerr << "Error: " << bk_last_error(nullptr) << std::endl;
        exit(1);
      }
      if (bk_upload_records(normal.ctx, &normal.soa, normal.soa_where) != BK_OK) die_normal();
    }
    if (bk_isize_stats(normal.ctx, nullptr, nullptr) != BK_OK || bk_discordant_pairs(normal.ctx, qual, w, nullptr, nullptr) != BK_OK ||
        bk_split_evidence(normal.ctx, nullptr) != BK_OK)
      die_normal();
    if ((rc = bk_normal_support(ctx, normal.ctx, w, &nsup, &n_nsup)) != BK_OK) die(rc);
  }
  // -genotype: reference-allele counts of every call on the sample's own records, then on the normal's (both record tables are
  // still resident: the contexts and the decoded tables are released at the end)
  vector<struct bk_ref_support> gsup, gsup_normal;
  if (genotype)
  {
    const struct bk_ref_support *rs = nullptr;
    uint64_t n_rs = 0;
    if ((rc = bk_ref_support(ctx, ctx, qual, (int) anchor, w, &rs, &n_rs)) != BK_OK) die(rc);
    gsup.assign(rs, rs + n_rs);  // (the rows are the library's until the next call)
    if (normal.ctx)
    {
      if ((rc = bk_ref_support(ctx, normal.ctx, qual, (int) anchor, w, &rs, &n_rs)) != BK_OK) die(rc);
      gsup_normal.assign(rs, rs + n_rs);
    }
  }
  // -vcf: the junction evidence of every call (member pairs by strands, split tuples by clip side)
  vector<struct bk_junction> jsup;
  if (vcf || clip || consensus)
  {
    const struct bk_junction *js = nullptr;
    uint64_t n_js = 0;
    if ((rc = bk_junctions(ctx, &js, &n_js)) != BK_OK) die(rc);
    jsup.assign(js, js + n_js);
  }
  // -clip: the clipped reads without an SA tag at every cluster, voted or not, on the sample's records and on the normal's
  vector<struct bk_clip_support> csup, csup_normal;
  if (clip)
  {
    const struct bk_clip_support *cs = nullptr;
    uint64_t n_cs = 0;
    if ((rc = bk_clip_support(ctx, ctx, qual, (int) min_clip, w, &cs, &n_cs)) != BK_OK) die(rc);
    csup.assign(cs, cs + n_cs);
    if (normal.ctx)
    {
      if ((rc = bk_clip_support(ctx, normal.ctx, qual, (int) min_clip, w, &cs, &n_cs)) != BK_OK) die(rc);
      csup_normal.assign(cs, cs + n_cs);
    }
  }
  const void *data = nullptr;
  uint64_t cnt = 0;
  if ((rc = bk_fetch(ctx, BK_STAGE_CLUSTERS, &data, &cnt, nullptr, nullptr)) != BK_OK) die(rc);
  const bk_cluster *cl = (const bk_cluster *) data;
  // -evidence: the reads behind every call (one row per member pair and per matching split tuple), listed on the device
  vector<struct bk_evidence> ev_rows;
  vector<uint64_t> ev_off;
  if (evidence || consensus)
  {
    const struct bk_evidence *ev = nullptr;
    const uint64_t *off = nullptr;
    uint64_t n_ev = 0;
    if ((rc = bk_evidence(ctx, &ev, &n_ev, &off)) != BK_OK) die(rc);
    ev_rows.assign(ev, ev + n_ev);
    ev_off.assign(off, off + cnt + 1);
  }
  // -dedup: the different fragments among those rows, per call, and for every row the first row of its fragment
  vector<struct bk_unique_support> usup;
  vector<uint64_t> ufirst;
  if (dedup)
  {
    const struct bk_unique_support *us = nullptr;
    const uint64_t *first = nullptr;
    uint64_t n_us = 0, n_first = 0;
    if ((rc = bk_unique_support(ctx, &us, &n_us, &first, &n_first)) != BK_OK) die(rc);
    usup.assign(us, us + n_us);
    ufirst.assign(first, first + n_first);
    if (n_us != cnt)
    {
      std::cerr << "Error: the unique-support table does not cover every cluster" << std::endl;
      exit(1);
    }
  }
  if (multi)
  {
    n_valid = 0;
    for (uint64_t i = 0; i < cnt; ++i) n_valid += (cl[i].flags & 2u) != 0;
  }
  std::cout << "valid cluster count: " << n_valid << std::endl;
  // annotate_cluster_for_sa_tag (BreakID.cc:492-567)
  vector<OutRow> rows;
  vector<Txpt> txpts;
  bool have_valid = false;
  for (uint64_t i = 0; i < cnt; ++i) have_valid |= (cl[i].flags & 2u) != 0;
  if (n_clustered >= 1 || have_valid)
  {
    // the reference reads refGene.txt for every group that reaches findClusterBreakPointInfoSaTag and exits if it is missing
    const char *inst = getenv("BREAKID_INSTALLDIR");
    string ref_gene = string(inst ? inst : BREAKID_INSTALLDIR) + "/ref_files/refGene.txt";
    if (!read_refgene(ref_gene, txpts))
    {
      std::cerr << "Error: cannot open \t" << ref_gene << std::endl;
      exit(1);
    }
  }
  for (uint64_t i = 0; i < cnt; ++i)
  {
    if (!(cl[i].flags & 2u)) continue;
    OutRow r;
    r.c = cl[i];
    r.idx = i;
    r.p1_chr = cl[i].p1_tid < 0 ? "*" : names[cl[i].p1_tid];
    r.p2_chr = cl[i].p2_tid < 0 ? "*" : names[cl[i].p2_tid];
    long p1 = (long) cl[i].p1_exact, p2 = (long) cl[i].p2_exact;  // exact positions are never -1 for valid clusters
    annotate_side(txpts, r.p1_chr, p1, r.g1, r.e1, r.s1);
    annotate_side(txpts, r.p2_chr, p2, r.g2, r.e2, r.s2);
    r.rpt1 = neighbour_seq(nib_dir, r.p1_chr, (int32_t) cl[i].p1_exact);
    r.rpt2 = neighbour_seq(nib_dir, r.p2_chr, cl[i].p2_exact);
    r.is_rpt = longest_run(r.rpt1) > 10 || longest_run(r.rpt2) > 10;
    r.af1 = (float) (long) cl[i].n_sr / (float) (double) cl[i].depth1;  // :475-478
    r.af2 = (float) (long) cl[i].n_sr / (float) (double) cl[i].depth2;
    rows.push_back(r);
  }
  // write_enspan_out (BreakID.cc:1184-1263): std::sort with the reference's comparator
  std::sort(rows.begin(), rows.end(), cmp_cluster);
  // -clip: the unvoted clusters whose clipped reads pile up on both sides (bk_clip_rescue), as rows of their own: the peaks are
  // their breakpoints, N_SR is 0, the depth is counted at the peaks
  vector<OutRow> rescued;
  if (clip)
  {
    if (csup.size() != cnt || jsup.size() != cnt || (normal.ctx && csup_normal.size() != cnt))
    {
      std::cerr << "Error: the clip evidence does not cover every cluster" << std::endl;
      exit(1);
    }
    vector<int32_t> q_tid;
    vector<uint32_t> q_pos;
    for (uint64_t i = 0; i < cnt; ++i)
    {
      uint32_t pos1 = 0, pos2 = 0, n1 = 0, n2 = 0;
      rc = bk_clip_rescue(&cl[i], &jsup[i], &csup[i], (uint32_t) clip_support, &pos1, &pos2, &n1, &n2);
      if (rc < 0)
      {
        std::cerr << "Error: bk_clip_rescue refused its arguments" << std::endl;
        exit(1);
      }
      if (rc != 1) continue;
      OutRow r;
      r.c = cl[i];
      r.idx = i;
      r.c.p1_exact = pos1;
      r.c.p2_exact = (int32_t) pos2;
      r.c.n_sr = 0;
      rescued.push_back(r);
      q_tid.push_back(cl[i].p1_tid);
      q_tid.push_back(cl[i].p2_tid);
      q_pos.push_back(pos1);
      q_pos.push_back(pos2);
    }
    const uint32_t *depth = nullptr;
    if ((rc = bk_base_depth(ctx, q_tid.data(), q_pos.data(), q_tid.size(), &depth)) != BK_OK) die(rc);
    for (size_t k = 0; k < rescued.size(); ++k)
    {
      OutRow &r = rescued[k];
      r.c.depth1 = depth[2 * k];
      r.c.depth2 = depth[2 * k + 1];
      r.p1_chr = names[r.c.p1_tid];
      r.p2_chr = names[r.c.p2_tid];
      annotate_side(txpts, r.p1_chr, (long) r.c.p1_exact, r.g1, r.e1, r.s1);
      annotate_side(txpts, r.p2_chr, (long) r.c.p2_exact, r.g2, r.e2, r.s2);
      r.rpt1 = neighbour_seq(nib_dir, r.p1_chr, (int32_t) r.c.p1_exact);
      r.rpt2 = neighbour_seq(nib_dir, r.p2_chr, r.c.p2_exact);
      r.is_rpt = longest_run(r.rpt1) > 10 || longest_run(r.rpt2) > 10;
      r.af1 = r.af2 = 0.0f;  // no split read: 0 of any depth, and 0 where the depth is 0
    }
    std::cout << "rescued cluster count: " << rescued.size() << std::endl;
    std::sort(rescued.begin(), rescued.end(), cmp_cluster);
  }
  // the rescued calls (the rows _fusion_rescued.txt writes, in its order): their two sites (ps_tid, peak, d_s), for the normal's
  // counts (-normal), the VCF records (-vcf) and the clipped reads themselves (-evidence)
  vector<RescuedCall> rescued_calls(rescued.size());
  vector<struct bk_clip_read> rescued_reads;
  vector<uint64_t> rescued_read_off;
  if (clip && (normal.ctx || vcf || evidence))
  {
    vector<struct bk_clip_site> sites;
    vector<size_t> written;
    for (size_t k = 0; k < rescued.size(); ++k)
    {
      const OutRow &r = rescued[k];
      RescuedCall &rcall = rescued_calls[k];
      uint8_t source = 0;
      bk_junction_sides(&jsup[r.idx], &rcall.right[0], &rcall.right[1], &source);
      for (int s = 0; s < 2; ++s) rcall.peak_n[s] = csup[r.idx].peak_n[s][rcall.right[s]];
      if (!rescued_written(r, !filter)) continue;
      written.push_back(k);
      sites.push_back(bk_clip_site{r.c.p1_tid, r.c.p1_exact, 0u, rcall.right[0]});
      sites.push_back(bk_clip_site{r.c.p2_tid, (uint32_t) r.c.p2_exact, 0u, rcall.right[1]});
    }
    if (evidence)
    {
      const uint32_t *counts = nullptr;
      const struct bk_clip_read *cr = nullptr;
      const uint64_t *off = nullptr;
      if ((rc = bk_clip_reads(ctx, sites.data(), sites.size(), qual, (int) min_clip, &counts, &cr, &off)) != BK_OK) die(rc);
      rescued_read_off.assign(off, off + sites.size() + 1);
      rescued_reads.assign(cr, cr + off[sites.size()]);
    }
    if (normal.ctx)
    {
      // the +-2 bp of every other count of the normal
      for (struct bk_clip_site &x : sites) x.tol = 2;
      vector<int32_t> q_tid;
      vector<uint32_t> q_pos;
      for (const struct bk_clip_site &x : sites)
      {
        q_tid.push_back(x.tid);
        q_pos.push_back(x.pos);
      }
      const uint32_t *counts = nullptr, *depth = nullptr;
      auto die_normal = [&] {
        std::cerr << "Error: normal " << normal.path << ": " << bk_last_error(normal.ctx) << std::endl;
        exit(1);
      };
      if (bk_clip_reads(normal.ctx, sites.data(), sites.size(), qual, (int) min_clip, &counts, nullptr, nullptr) != BK_OK) die_normal();
      if (bk_base_depth(normal.ctx, q_tid.data(), q_pos.data(), q_tid.size(), &depth) != BK_OK) die_normal();
      for (size_t j = 0; j < written.size(); ++j)
      {
        RescuedCall &rcall = rescued_calls[written[j]];
        const uint64_t idx = rescued[written[j]].idx;
        rcall.normal_drp = idx < n_nsup ? nsup[idx].n_drp : 0;
        for (int s = 0; s < 2; ++s)
        {
          rcall.normal_at[s] = counts[2 * j + s];
          rcall.normal_depth[s] = depth[2 * j + s];
        }
      }
    }
  }
  // -consensus: the clipped bases at the two breakpoints of every written call.  Sites: side s of a call is (ps_tid, ps_exact, 0, d_s),
  // d_s from bk_junction_sides.  Reads: those of the call's BK_EV_SPLIT rows, and those bk_clip_reads lists at the sites (the reads
  // without an SA tag), each name once.  One pass over the file brings their alignments back with the bases, one call piles them up.
  std::map<uint64_t, std::pair<ConsensusSide, ConsensusSide>> cons;
  std::map<uint64_t, std::pair<HomologySide, HomologySide>> hom;  // -homology: the junction fit of the same sides
  if (consensus)
  {
    vector<struct bk_clip_site> sites;
    vector<uint64_t> site_call;
    std::set<std::pair<uint64_t, uint32_t>> seen;
    vector<bk_read_key> keys;
    auto add_key = [&](uint64_t qhash, uint32_t qcheck) {
      if (seen.emplace(qhash, qcheck).second) keys.push_back(bk_read_key{qhash, qcheck, 0});
    };
    for (const OutRow &r : rows)
    {
      if (!call_written(r, !filter)) continue;
      if (r.idx >= jsup.size() || r.idx + 1 >= ev_off.size() || ev_off[r.idx + 1] > ev_rows.size())
      {
        std::cerr << "Error: the evidence tables do not cover every call" << std::endl;
        exit(1);
      }
      uint8_t right[2] = {0, 1}, source = 0;
      bk_junction_sides(&jsup[r.idx], &right[0], &right[1], &source);
      site_call.push_back(r.idx);
      sites.push_back(bk_clip_site{r.c.p1_tid, r.c.p1_exact, 0u, right[0]});
      sites.push_back(bk_clip_site{r.c.p2_tid, (uint32_t) r.c.p2_exact, 0u, right[1]});
      for (uint64_t i = ev_off[r.idx]; i < ev_off[r.idx + 1]; ++i)
        if (ev_rows[i].kind == BK_EV_SPLIT) add_key(ev_rows[i].qhash, ev_rows[i].qcheck);
    }
    {
      const uint32_t *counts = nullptr;
      const struct bk_clip_read *cr = nullptr;
      const uint64_t *off = nullptr;
      if ((rc = bk_clip_reads(ctx, sites.data(), sites.size(), qual, (int) min_clip, &counts, &cr, &off)) != BK_OK) die(rc);
      for (uint64_t i = 0; i < off[sites.size()]; ++i) add_key(cr[i].qhash, cr[i].qcheck);
    }
    bk_reads reads;
    char rerr[512] = "";
    if (bk_bam_reads(inp_file.c_str(), keys.data(), keys.size(), &reads, rerr, sizeof rerr) != BK_OK)
    {
      std::cerr << "Error: cannot read the clipped reads back from " << inp_file << ": " << rerr << std::endl;
      exit(1);
    }
    const struct bk_consensus *cs = nullptr;
    const uint8_t *bases = nullptr;
    rc = bk_clip_consensus(ctx, &reads, sites.data(), sites.size(), qual, (int) min_clip, (uint32_t) conslen, CONSENSUS_MIN_DEPTH, &cs, &bases, nullptr);
    bk_reads_free(&reads);
    if (rc != BK_OK) die(rc);
    for (size_t j = 0; j < site_call.size(); ++j)
    {
      std::pair<ConsensusSide, ConsensusSide> &both = cons[site_call[j]];
      for (int s = 0; s < 2; ++s)
      {
        ConsensusSide &side = s ? both.second : both.first;
        side.c = cs[2 * j + s];
        const uint8_t *b = bases + (2 * j + s) * (size_t) conslen;
        side.seq.assign((const char *) b, side.c.len);
        if (sites[2 * j + s].dir == 1u) std::reverse(side.seq.begin(), side.seq.end());
      }
    }
    // -homology: one probe per side with a consensus, own = the side's site, mate = the other side's; the query is the side's row of
    // `bases` as it lies.  The reference: per contig the nib file is opened once and the windows around every probe position are
    // read, merged where they touch: one segment per window.  One call fits every probe of the run.
    if (homology)
    {
      std::map<int32_t, std::unique_ptr<Nib>> nibs;
      auto nib_of = [&](int32_t tid) -> Nib * {
        if (tid < 0 || tid >= nt) return nullptr;
        auto it = nibs.find(tid);
        if (it == nibs.end())
        {
          it = nibs.emplace(tid, std::unique_ptr<Nib>(new Nib)).first;
          it->second->open(nib_dir + "/hg19_" + string(names[tid]) + ".nib");
        }
        return it->second->ok ? it->second.get() : nullptr;
      };
      const long radius = conslen + homshift + (long) HOMOLOGY_MAX_HOM + 1;
      vector<struct bk_junction_probe> probes;
      vector<size_t> probe_site;
      vector<uint8_t> query;
      std::map<int32_t, vector<std::pair<long, long>>> spans;  // per contig the 1-based windows [a, b]
      for (size_t x = 0; x < sites.size(); ++x)
      {
        const struct bk_clip_site &own = sites[x], &mate = sites[x ^ 1];
        if (cs[x].len == 0 || !nib_of(own.tid) || !nib_of(mate.tid)) continue;
        probes.push_back(bk_junction_probe{own.tid, own.pos, own.dir, mate.tid, mate.pos, mate.dir, cs[x].len, 0u});
        probe_site.push_back(x);
        query.insert(query.end(), bases + x * (size_t) conslen, bases + (x + 1) * (size_t) conslen);
        for (const struct bk_clip_site *e : {&own, &mate})
        {
          const long a = std::max(1l, (long) e->pos - radius), b = std::min((long) nib_of(e->tid)->nBases, (long) e->pos + radius);
          if (a <= b) spans[e->tid].emplace_back(a, b);
        }
      }
      vector<int32_t> seg_tid;
      vector<uint32_t> seg_start, seg_len;
      vector<uint64_t> seg_off(1, 0);
      vector<uint8_t> seg_bases;
      for (auto &kv : spans)
      {
        std::sort(kv.second.begin(), kv.second.end());
        vector<std::pair<long, long>> merged;
        for (const auto &w : kv.second)
        {
          if (!merged.empty() && w.first <= merged.back().second + 1)
            merged.back().second = std::max(merged.back().second, w.second);
          else
            merged.push_back(w);
        }
        Nib *nb = nib_of(kv.first);
        for (const auto &w : merged)
        {
          const long start0 = (w.first - 1) & ~1l;  // a segment starts on a byte of the file
          const long len = w.second - start0;
          const size_t at = seg_bases.size(), nbytes = (size_t) ((len + 1) / 2);
          seg_bases.resize(at + nbytes);
          nb->in.clear();
          nb->in.seekg(8 + start0 / 2);
          nb->in.read((char *) seg_bases.data() + at, (std::streamsize) nbytes);
          if ((size_t) nb->in.gcount() != nbytes)
          {
            std::cerr << "Error: " << nib_dir << "/hg19_" << names[kv.first] << ".nib is shorter than its header says" << std::endl;
            exit(1);
          }
          seg_tid.push_back(kv.first);
          seg_start.push_back((uint32_t) start0);
          seg_len.push_back((uint32_t) len);
          seg_off.push_back(seg_bases.size());
        }
      }
      bk_refseq ref;
      ref.n_segs = seg_tid.size();
      ref.tid = seg_tid.data();
      ref.start = seg_start.data();
      ref.len = seg_len.data();
      ref.off = seg_off.data();
      ref.bases = seg_bases.data();
      const struct bk_junction_fit *fit = nullptr;
      if ((rc = bk_junction_fit(ctx, &ref, probes.data(), probes.size(), query.data(), (uint32_t) conslen, (uint32_t) homshift, (uint32_t) homins, HOMOLOGY_MAX_HOM, &fit)) !=
          BK_OK)
        die(rc);
      // the base at a 1-based position from the segments read above (N outside them)
      auto seg_base = [&](int32_t tid, long pos1) -> char {
        static const char tab[8] = {'T', 'C', 'A', 'G', 'N', 'N', 'N', 'N'};
        size_t lo = 0, hi = seg_tid.size();  // the segments ascend by (tid, start): the last one that starts at or before pos1
        while (lo < hi)
        {
          const size_t mid = lo + (hi - lo) / 2;
          if (seg_tid[mid] < tid || (seg_tid[mid] == tid && (long) seg_start[mid] <= pos1 - 1))
            lo = mid + 1;
          else
            hi = mid;
        }
        if (lo == 0 || seg_tid[lo - 1] != tid) return 'N';
        const long i = pos1 - 1 - (long) seg_start[lo - 1];
        if (i < 0 || i >= (long) seg_len[lo - 1]) return 'N';
        const uint8_t byte = seg_bases[seg_off[lo - 1] + (size_t) (i / 2)];
        return tab[((i & 1) ? byte : byte >> 4) & 7];
      };
      for (uint64_t call : site_call) hom[call];
      for (size_t k = 0; k < probes.size(); ++k)
      {
        if (!fit[k].placed) continue;
        const size_t x = probe_site[k];
        std::pair<HomologySide, HomologySide> &both = hom[site_call[x / 2]];
        HomologySide &side = (x & 1) ? both.second : both.first;
        side.on = true;
        side.f = fit[k];
        const long pos = probes[k].pos_own, fwd = fit[k].hom_fwd, back = fit[k].hom_back;
        const bool right = probes[k].dir_own == 1u;
        for (long p = right ? pos - fwd : pos - back + 1; p <= (right ? pos + back - 1 : pos + fwd); ++p) side.hom_seq += seg_base(probes[k].tid_own, p);
        side.ins_seq.assign((const char *) query.data() + k * (size_t) conslen, fit[k].ins);
        if (right) std::reverse(side.ins_seq.begin(), side.ins_seq.end());
      }
    }
  }
  std::ofstream out, outf, out_n, outf_n;  // (_n: the twins with the matched normal's four counts)
  std::ofstream out_s, outf_s;             // (_s: the twins with the junction consensus, -consensus)
  std::ofstream out_h, outf_h;             // (_h: the twins with the junction fit, -homology)
  std::ofstream out_g, outf_g;             // (_g: the twins with the genotype columns, -genotype)
  std::ofstream out_c, outf_c, out_r;      // (_c: the twins with the clip columns, _r: the rescued clusters, -clip)
  std::ofstream out_d, outf_d;             // (_d: the twins with the unique-support columns, -dedup)
  const bool with_normal = !normal_file.empty();  // (a tumour without calls still gets header-only twins)
  const string header_n = string(HEADER, strlen(HEADER) - 1) + NORMAL_COLUMNS;
  string header_g = string(HEADER, strlen(HEADER) - 1) + GENOTYPE_COLUMNS;
  if (with_normal) header_g += string(NORMAL_COLUMNS, strlen(NORMAL_COLUMNS) - 1) + GENOTYPE_COLUMNS_NORMAL;
  header_g += "\n";
  const string header_c = string(HEADER, strlen(HEADER) - 1) + CLIP_COLUMNS + (with_normal ? CLIP_COLUMNS_NORMAL : "") + "\n";
  const string header_d = string(HEADER, strlen(HEADER) - 1) + DEDUP_COLUMNS + "\n";
  const string header_s = string(HEADER, strlen(HEADER) - 1) + CONSENSUS_COLUMNS + "\n";
  const string header_h = string(HEADER, strlen(HEADER) - 1) + HOMOLOGY_COLUMNS + "\n";
  if (!filter)
  {
    out.open((out_file + "_fusion_all.txt").c_str());
    out << HEADER;
    if (dedup)
    {
      out_d.open((out_file + "_fusion_all_dedup.txt").c_str());
      out_d << header_d;
    }
    if (consensus)
    {
      out_s.open((out_file + "_fusion_all_consensus.txt").c_str());
      out_s << header_s;
    }
    if (homology)
    {
      out_h.open((out_file + "_fusion_all_homology.txt").c_str());
      out_h << header_h;
    }
    if (with_normal)
    {
      out_n.open((out_file + "_fusion_all_normal.txt").c_str());
      out_n << header_n;
    }
    if (genotype)
    {
      out_g.open((out_file + "_fusion_all_genotype.txt").c_str());
      out_g << header_g;
    }
    if (clip)
    {
      out_c.open((out_file + "_fusion_all_clip.txt").c_str());
      out_c << header_c;
    }
  }
  outf.open((out_file + "_fusion.txt").c_str());
  outf << HEADER;
  if (dedup)
  {
    outf_d.open((out_file + "_fusion_dedup.txt").c_str());
    outf_d << header_d;
  }
  if (consensus)
  {
    outf_s.open((out_file + "_fusion_consensus.txt").c_str());
    outf_s << header_s;
  }
  if (homology)
  {
    outf_h.open((out_file + "_fusion_homology.txt").c_str());
    outf_h << header_h;
  }
  if (with_normal)
  {
    outf_n.open((out_file + "_fusion_normal.txt").c_str());
    outf_n << header_n;
  }
  if (genotype)
  {
    outf_g.open((out_file + "_fusion_genotype.txt").c_str());
    outf_g << header_g;
  }
  if (clip)
  {
    outf_c.open((out_file + "_fusion_clip.txt").c_str());
    outf_c << header_c;
    out_r.open((out_file + "_fusion_rescued.txt").c_str());
    out_r << header_c;
    std::ofstream out_rn;  // (with -normal: the same rows with the normal's evidence at the rescued peaks)
    if (with_normal)
    {
      out_rn.open((out_file + "_fusion_rescued_normal.txt").c_str());
      out_rn << string(header_c, 0, header_c.size() - 1) << RESCUED_COLUMNS_NORMAL << "\n";
    }
    for (size_t k = 0; k < rescued.size(); ++k)
    {
      const OutRow &r = rescued[k];
      if (!rescued_written(r, !filter)) continue;
      const ClipCols cc = clip_cols(jsup[r.idx], csup[r.idx], with_normal ? &csup_normal[r.idx] : nullptr);
      write_row(out_r, r, nullptr, nullptr, nullptr, &cc);
      if (with_normal)
      {
        const RescuedCall &x = rescued_calls[k];
        std::ostringstream tail;
        tail << "\t" << x.normal_drp << "\t" << x.normal_at[0] << "\t" << x.normal_at[1] << "\t" << x.normal_depth[0] << "\t" << x.normal_depth[1];
        const string t = tail.str();
        write_row(out_rn, r, nullptr, nullptr, nullptr, &cc, &t);
      }
    }
    out_r.close();
    if (with_normal) out_rn.close();
  }
  for (auto &r : rows)
  {
    const bool all_ok = call_all_ok(r), filt_ok = call_filt_ok(r);
    if (clip)
    {
      const ClipCols cc = clip_cols(jsup[r.idx], csup[r.idx], with_normal ? &csup_normal[r.idx] : nullptr);
      if (filt_ok) write_row(outf_c, r, nullptr, nullptr, nullptr, &cc);
      if (!filter && all_ok) write_row(out_c, r, nullptr, nullptr, nullptr, &cc);
    }
    if (filt_ok) write_row(outf, r);
    if (!filter && all_ok) write_row(out, r);
    if (dedup && r.idx < usup.size())
    {
      const struct bk_unique_support &u = usup[r.idx];
      std::ostringstream tail;
      tail << "\t" << u.uniq_pairs << "\t" << u.uniq_splits << "\t" << u.top_pairs << "\t" << u.top_splits;
      const string t = tail.str();
      if (filt_ok) write_row(outf_d, r, nullptr, nullptr, nullptr, nullptr, &t);
      if (!filter && all_ok) write_row(out_d, r, nullptr, nullptr, nullptr, nullptr, &t);
    }
    if (consensus && cons.count(r.idx))
    {
      const std::pair<ConsensusSide, ConsensusSide> &both = cons.at(r.idx);
      std::ostringstream tail;
      for (const ConsensusSide *x : {&both.first, &both.second})
        tail << "\t" << x->c.n_reads << "\t" << x->c.len << "\t" << x->agree() << "\t" << (x->seq.empty() ? "." : x->seq);
      const string t = tail.str();
      if (filt_ok) write_row(outf_s, r, nullptr, nullptr, nullptr, nullptr, &t);
      if (!filter && all_ok) write_row(out_s, r, nullptr, nullptr, nullptr, nullptr, &t);
    }
    if (homology && hom.count(r.idx))
    {
      const string t = hom.at(r.idx).first.fields() + hom.at(r.idx).second.fields();
      if (filt_ok) write_row(outf_h, r, nullptr, nullptr, nullptr, nullptr, &t);
      if (!filter && all_ok) write_row(out_h, r, nullptr, nullptr, nullptr, nullptr, &t);
    }
    if (with_normal && r.idx < n_nsup)
    {
      if (filt_ok) write_row(outf_n, r, &nsup[r.idx]);
      if (!filter && all_ok) write_row(out_n, r, &nsup[r.idx]);
    }
    if (genotype && r.idx < gsup.size() && (!with_normal || (r.idx < n_nsup && r.idx < gsup_normal.size())))
    {
      const struct bk_normal_support *ns = with_normal ? &nsup[r.idx] : nullptr;
      const struct bk_ref_support *gn = with_normal ? &gsup_normal[r.idx] : nullptr;
      if (filt_ok) write_row(outf_g, r, ns, &gsup[r.idx], gn);
      if (!filter && all_ok) write_row(out_g, r, ns, &gsup[r.idx], gn);
    }
  }
  if (!filter) out.close();
  outf.close();
  if (with_normal)
  {
    if (!filter) out_n.close();
    outf_n.close();
  }
  if (genotype)
  {
    if (!filter) out_g.close();
    outf_g.close();
  }
  if (clip)
  {
    if (!filter) out_c.close();
    outf_c.close();
  }
  if (dedup)
  {
    if (!filter) out_d.close();
    outf_d.close();
  }
  if (consensus)
  {
    if (!filter) out_s.close();
    outf_s.close();
  }
  if (homology)
  {
    if (!filter) out_h.close();
    outf_h.close();
  }
  if (vcf)
  {
    VcfInput vi;
    vi.nt = nt;
    vi.names = names;
    vi.lens = lens;
    vi.nib_dir = nib_dir;
    vi.all = !filter;
    vi.jsup = &jsup;
    vi.with_normal = with_normal;
    vi.nsup = nsup;
    vi.n_nsup = n_nsup;
    vi.gsup = genotype ? &gsup : nullptr;
    vi.gsup_normal = genotype && with_normal ? &gsup_normal : nullptr;
    vi.usup = dedup ? &usup : nullptr;
    vi.cons = consensus ? &cons : nullptr;
    vi.hom = homology ? &hom : nullptr;
    if (!write_vcf(out_file + "_fusion.vcf", rows, vi))
    {
      std::cerr << "Error: cannot write " << out_file << "_fusion.vcf: the evidence tables do not cover every call" << std::endl;
      exit(1);
    }
    if (clip)
    {
      vi.gsup = vi.gsup_normal = nullptr;  // rescued calls are not genotyped
      vi.usup = nullptr;                   // ... and their files stay as they are with -dedup
      vi.cons = nullptr;                   // ... and with -consensus
      vi.hom = nullptr;                    // ... and with -homology
      vi.rescued = &rescued_calls;
      if (!write_vcf(out_file + "_fusion_rescued.vcf", rescued, vi))
      {
        std::cerr << "Error: cannot write " << out_file << "_fusion_rescued.vcf: the evidence tables do not cover every call" << std::endl;
        exit(1);
      }
    }
  }
  if (evidence)
  {
    EvidenceInput ei;
    ei.nt = nt;
    ei.names = names;
    ei.all = !filter;
    ei.rows = &ev_rows;
    ei.call_off = &ev_off;
    ei.first = dedup ? &ufirst : nullptr;
    string why;
    if (!write_evidence(out_file, inp_file, rows, ei, why))
    {
      std::cerr << "Error: cannot write " << out_file << "_evidence.txt / _evidence.bam: " << why << std::endl;
      exit(1);
    }
    if (clip && !write_evidence_rescued(out_file, inp_file, rescued, rescued_calls, ei, rescued_reads, rescued_read_off, why))
    {
      std::cerr << "Error: cannot write " << out_file << "_evidence_rescued.txt / _evidence_rescued.bam: " << why << std::endl;
      exit(1);
    }
  }
  {
    std::ofstream p((out_file + "_params.txt").c_str());  // write_enspan_params :1170-1182
    p << "ENSPAN" << std::endl;
    p << "inp_file\t" << inp_file << std::endl;
    p << "out_file\t" << out_file << std::endl;
    p << "qual\t" << (long) qual << std::endl;
    p << "w\t" << w << std::endl;
    p << "build\t" << build << std::endl;
    if (exclude) p << "exclude_file\t" << exclude_file << std::endl;
    if (!normal_file.empty()) p << "normal_file\t" << normal_file << std::endl;
    if (genotype) p << "genotype_anchor\t" << anchor << std::endl;
    if (vcf) p << "vcf\t1" << std::endl;
    if (evidence) p << "evidence\t1" << std::endl;
    if (clip) p << "clip_min_length\t" << min_clip << std::endl;
    if (clip) p << "clip_min_support\t" << clip_support << std::endl;
    if (dedup) p << "dedup\t1" << std::endl;
    if (consensus) p << "consensus_max_len\t" << conslen << std::endl;
    if (homology) p << "homology_max_shift\t" << homshift << std::endl;
    if (homology) p << "homology_max_ins\t" << homins << std::endl;
  }
  clock_t end = clock();
  std::cout << "the fusion process of file " << inp_file << "  costs time: " << (end - start) / double(CLOCKS_PER_SEC) << " seconds" << std::endl;
  {
    // :175-191.  scan_pairs_count and after_cluster_count are never updated by the reference (always 0);
    // removed_isolated_pair_count sums the groups that keep >= 2 pairs (:128); root_cluster_num is what the clustering of the
    // LAST such group returned (:131-136; the reference leaves it uninitialised when no group qualifies - 0 here)
    const bk_group_stat *gs = nullptr;
    uint32_t ngs = 0;
    if (!multi && (rc = bk_group_stats(ctx, &gs, &ngs)) != BK_OK) die(rc);
    if (multi && (rc = bk_multi_stats(ctx, nullptr, nullptr, &gs, &ngs)) != BK_OK) die(rc);  // (summed over the ranks)
    int removed_isolated_pair_count = 0, root_cluster_num = 0;
    for (uint32_t g = 0; g < ngs; ++g)
      if (gs[g].n_isolated_removed >= 2)
      {
        removed_isolated_pair_count += (int) gs[g].n_isolated_removed;
        root_cluster_num = fast ? (gs[g].cluster_id_end ? (int) gs[g].cluster_id_end - 1 : 0)
                                : (int) (gs[g].cluster_id_end + gs[g].n_isolated_removed - gs[g].n_clustered);
      }
    std::ofstream p((out_file + "_performance.txt").c_str());
    p << "scan_dist\tdiscordant pairs\tremove isolated\tafter_cluster\troot cluster\tscanning time\tcluster time\tfind breakpoint time\ttotal time" << std::endl;
    p << w << "\t" << 0 << "\t" << removed_isolated_pair_count << "\t" << 0 << "\t" << root_cluster_num << "\t" << (scan_end - scan_start) / double(CLOCKS_PER_SEC)
      << "\t" << (cluster_end - cluster_start) / double(CLOCKS_PER_SEC) << "\t" << (bp_end - bp_start) / double(CLOCKS_PER_SEC) << "\t"
      << (end - start) / double(CLOCKS_PER_SEC) << std::endl;
  }
  if (multi)
    bk_multi_free(ctx);
  else
    bk_free(ctx);
  if (normal.ctx) bk_free(normal.ctx);
  for (Sample *s : {&tumor, &normal})
  {
    if (s->bam) bk_bam_close(s->bam);
    if (s->dbam) bk_bam_dev_free(s->dbam);
  }
  return 0;
}
