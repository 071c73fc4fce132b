// BreakID command line on top of libbreakid_hip.so: same options, same output files as the reference
// (src/BreakID.cc:6-192, help text src/BreakID.h:27-36).  The hot path (BreakID.cc:98-167 minus annotation)
// runs on the MI355X through the C ABI; this file is the host side the reference keeps in main():
// argument parsing, BAM decode into the columnar table, refGene/nib annotation (BreakID.cc:492-567,
// :1528-1793, RefSeqTranscript.cc, nibtools.cc, util_bam.cc:78-122, util_bed.cc:224-261) and the writers
// (:1170-1263).  There is no CPU implementation of the hot path in here.  The options and what a command line is refused for are in
// breakid_options.h, everything that writes a file in breakid_writers.h; main() at the end of this file is the sequence of stages.
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

#include "breakid_options.h"
#include "breakid_writers.h"

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

// -known panel.bedpe: whitespace-separated fields, 0-based half-open coordinates; chrom1 start1 end1 chrom2 start2 end2, then name,
// score, strand1 and strand2 where the line has them, further columns ignored.  Blank lines and lines that start with '#', "track" or
// "browser" are skipped.  Names match the header's exactly: an interval on a contig the header lacks ('.' included) holds nothing
// (tid -1), and its line is counted; its entry stays, because the other interval can still hold a breakpoint.  Intervals are clamped to
// the contig's length, and one that lies behind it holds nothing either.  A missing or '.' name is the name "."; name ids ascend in
// order of first appearance.  The score goes through strtod, is truncated towards zero and clamped to int32; a field that strtod does
// not consume whole, or NaN, means no score.  Strand '+' is LEFT, '-' is RIGHT, anything else unstated.  Fewer than six fields, a
// coordinate that is not a number, and on a contig of the header a negative coordinate or end <= start end the run.
struct KnownPanel
{
  vector<struct bk_known_entry> entries;
  vector<string> names;  // by name id
  uint64_t unknown = 0;  // lines with a contig that the header lacks
};
static KnownPanel read_known_bedpe(const string &path, const char *const *names, const uint32_t *lens, int nt)
{
  std::ifstream in(path.c_str());
  if (!in.is_open())
  {
    std::cerr << "Error: can not open known file: " << path << std::endl;
    exit(1);
  }
  std::map<string, int> id;
  for (int i = 0; i < nt; ++i) id.emplace(names[i], i);
  std::map<string, uint32_t> name_id;
  KnownPanel p;
  string line;
  uint64_t no = 0;
  auto fail = [&](const string &why) {
    std::cerr << "Error: known file " << path << ", line " << no << ": " << why << std::endl;
    exit(1);
  };
  auto number = [&](const string &f) {
    char *e = nullptr;
    errno = 0;
    const long long v = strtoll(f.c_str(), &e, 10);
    if (f.empty() || *e || errno) fail("not a number: " + f);
    return v;
  };
  auto strand = [](const vector<string> &f, size_t k) { return k < f.size() && f[k] == "+" ? BK_STRAND_LEFT : k < f.size() && f[k] == "-" ? BK_STRAND_RIGHT : BK_STRAND_NONE; };
  while (std::getline(in, line))
  {
    ++no;
    std::istringstream ss(line);
    vector<string> f;
    for (string w; ss >> w;) f.push_back(w);
    if (f.empty() || f[0][0] == '#' || f[0] == "track" || f[0] == "browser") continue;
    if (f.size() < 6) fail("fewer than six fields (chrom1 start1 end1 chrom2 start2 end2)");
    struct bk_known_entry e = {};
    bool lacking = false;
    for (int k = 0; k < 2; ++k)
    {
      long long b = number(f[3 * k + 1]), x = number(f[3 * k + 2]);
      int32_t tid = -1;
      const auto it = id.find(f[3 * k]);
      if (it == id.end())
        lacking = true;
      else
      {
        if (b < 0) fail("negative coordinate: " + f[3 * k + 1]);
        if (x < 0) fail("negative coordinate: " + f[3 * k + 2]);
        if (x <= b) fail("end <= start");
        const long long len = lens[it->second];
        b = std::min(b, len);
        x = std::min(x, len);
        if (x > b) tid = it->second;  // (else behind the contig's end)
      }
      if (tid < 0) b = x = 0;
      (k ? e.tid2 : e.tid1) = tid;
      (k ? e.beg2 : e.beg1) = (uint32_t) b;
      (k ? e.end2 : e.end1) = (uint32_t) x;
    }
    p.unknown += lacking;
    const string name = f.size() > 6 ? f[6] : string(".");
    const auto at = name_id.find(name);
    if (at == name_id.end())
    {
      e.name = (uint32_t) p.names.size();
      name_id.emplace(name, e.name);
      p.names.push_back(name);
    }
    else
      e.name = at->second;
    e.score = BK_KNOWN_NO_SCORE;
    if (f.size() > 7)
    {
      char *end = nullptr;
      const double v = strtod(f[7].c_str(), &end);
      if (end != f[7].c_str() && !*end && v == v) e.score = v >= 2147483647.0 ? (int32_t) 2147483647 : v <= -2147483648.0 ? (int32_t) (-2147483647 - 1) : (int32_t) v;
    }
    e.strand1 = (uint8_t) strand(f, 8);
    e.strand2 = (uint8_t) strand(f, 9);
    p.entries.push_back(e);
  }
  if (p.unknown) std::cerr << "Warning: " << p.unknown << " lines of the known file " << path << " name contigs that are not in the BAM header" << std::endl;
  return p;
}

#ifndef BREAKID_INSTALLDIR
#define BREAKID_INSTALLDIR "."
#endif

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

// the voted and the rescued rows alike: contig names, gene / exon / strand on either side, the neighbour sequences and the repeat flag
static void annotate(OutRow &r, const vector<Txpt> &txpts, const string &nib_dir, const char *const *names)
{
  r.p1_chr = r.c.p1_tid < 0 ? "*" : names[r.c.p1_tid];
  r.p2_chr = r.c.p2_tid < 0 ? "*" : names[r.c.p2_tid];
  annotate_side(txpts, r.p1_chr, (long) r.c.p1_exact, r.g1, r.e1, r.s1);  // exact positions are never -1 for the rows written
  annotate_side(txpts, r.p2_chr, (long) r.c.p2_exact, r.g2, r.e2, r.s2);
  r.rpt1 = neighbour_seq(nib_dir, r.p1_chr, (int32_t) r.c.p1_exact);
  r.rpt2 = neighbour_seq(nib_dir, r.p2_chr, r.c.p2_exact);
  r.is_rpt = longest_run(r.rpt1) > 10 || longest_run(r.rpt2) > 10;
}

// ---- one input BAM: its decoded table (host or device) and, once created, its context ---------------------------------------------
struct Sample
{
  string path;
  bool is_normal = false;
  bk_bam *bam = nullptr;
  bk_bam_dev *dbam = nullptr;
  int nt = 0;
  const char *const *names = nullptr;
  const uint32_t *lens = nullptr;
  bk_soa soa{};
  int soa_where = BK_MEM_HOST;
  bk_ctx *ctx = nullptr;
  uint64_t n_excluded = 0;  // -x: records that overlapped the list
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
  void release_table()
  {
    if (dbam) bk_bam_dev_free(dbam);
    if (bam) bk_bam_close(bam);
    dbam = nullptr;
    bam = nullptr;
    soa = bk_soa{};
  }
  void host_decode();
  bool gpu_decode(const Options &o);
  int ensure_context(int device);
  void exclude(const Options &o, const bk_regions &regions);
};

// a stage of the library failed on this sample's context
static void die(const Sample &s, int rc)
{
  if (s.is_normal)
  {
    std::cerr << "Error: normal " << s.path << ": " << bk_last_error(s.ctx) << std::endl;
    exit(1);
  }
  std::cerr << (rc == BK_ERR_CIGAR ? "error cigar: " : bk_last_error(s.ctx)) << std::endl;
  exit(rc == BK_ERR_CIGAR ? -1 : 1);
}

// the host decoder (all cores, pinned columns): files whose records straddle BGZF blocks or that exceed one batch of the GPU feed
void Sample::host_decode()
{
  char err[512];
  dbam = nullptr;
  if (bk_bam_open(path.c_str(), &bam, err, sizeof err) != BK_OK)
  {
    std::cerr << "Error: can not open bam-file: " << path << std::endl;
    exit(1);
  }
  bk_bam_header(bam, &nt, &names, &lens);
  if (bk_bam_decode(bam, &soa, err, sizeof err) != BK_OK)
  {
    std::cerr << "Error: " << err << std::endl;
    exit(1);
  }
}

// One read of the file: BGZF inflate + record decode on the device (every htslib-written BAM qualifies), the stream pass of the hot path
// running on the chunks already decoded while the rest of the file is still arriving (the reference reads the BAM twice,
// BreakID.cc:1929, :1414).  With -x the table alone: context, upload and exclusion follow, the stream pass after the exclusion.
// False when the GPU feed refuses the file (or BREAKID_HOST_DECODE=1): the host decoder takes it then.
bool Sample::gpu_decode(const Options &o)
{
  char err[512];
  if (getenv("BREAKID_HOST_DECODE")) return false;
  if (o.exclude())
  {
    if (bk_bam_decode_device(path.c_str(), o.device, &dbam, &soa, &nt, &names, &lens, err, sizeof err) != BK_OK)
    {
      dbam = nullptr;
      return false;
    }
  }
  else if (bk_bam_decode_device_ctx(path.c_str(), o.device, o.qual, &dbam, &ctx, &nt, &names, &lens, err, sizeof err) != BK_OK)
    return false;
  soa_where = BK_MEM_DEVICE;
  return true;
}

// the context of a decoded table that has none yet (the GPU feed without -x has attached it and run the stream pass already);
// returns what bk_upload_records answers
int Sample::ensure_context(int device)
{
  if (ctx) return BK_OK;
  if (bk_init(device, lens, names, nt, &ctx) != BK_OK)
  {
    std::cerr << "Error: " << bk_last_error(nullptr) << std::endl;
    exit(1);
  }
  return bk_upload_records(ctx, &soa, soa_where);
}

// -x: context, upload, exclusion; then the decoded table goes (the context holds the kept records), the reference list stays as a copy
void Sample::exclude(const Options &o, const bk_regions &regions)
{
  own_header();
  if (!ctx && (ensure_context(o.device) != BK_OK || bk_exclude_regions(ctx, &regions, &n_excluded) != BK_OK))
  {
    std::cerr << "Error: " << path << ": " << bk_last_error(ctx) << std::endl;
    exit(1);
  }
  release_table();
}

// -x: the list, read against the file's reference list before anything is decoded
struct Exclusion
{
  ExcludeList list;
  bk_regions regions{};
};
static void read_exclusion(const Options &o, Exclusion &x)
{
  vector<string> names;
  vector<uint32_t> lens;
  if (!bam_header_list(o.inp_file, names, lens))
  {
    std::cerr << "Error: can not read the header of bam-file: " << o.inp_file << std::endl;
    exit(1);
  }
  x.list = read_exclude_bed(o.exclude_file, names, lens);
  x.regions.tid = x.list.tid.data();
  x.regions.beg = x.list.beg.data();
  x.regions.end = x.list.end.data();
  x.regions.n = x.list.tid.size();
}
static void say_excluded(const Options &o, const Exclusion &x, uint64_t n, const char *of_whom)
{
  std::cout << "excluded " << n << " records " << of_whom << "overlapping " << x.list.tid.size() << " intervals of " << o.exclude_file << "\n";
}

// The tumour's table.  Single context: the GPU feed first, the host decoder for what it refuses, then -x.  Sharded: nothing here (every
// rank decodes its part of the file on its own GPU, run_sharded) unless BREAKID_HOST_DECODE=1 asks for the host table.
static void decode_tumor(const Options &o, Sample &tumor, const Exclusion &x)
{
  if (!o.multi() && tumor.gpu_decode(o))
  {
    // the feed's staging buffers and slots (1-2.5 GB of device memory) go back once the last file of the process is decoded
    if (!o.with_normal()) bk_feed_release_caches();
  }
  else if (!o.multi() || getenv("BREAKID_HOST_DECODE"))
    tumor.host_decode();
  if (o.exclude() && !o.multi()) tumor.exclude(o, x.regions);
}

// ---- the hot path ----------------------------------------------------------------------------------------------------------------
// what the stages leave for the tail of main()
struct Run
{
  double w = 0;
  double mean = 0, sd = 0;  // the library's insert sizes (bk_isize_stats), kept for -fragsize
  uint64_t n_clustered = 0, n_valid = 0;
  clock_t scan_start = clock(), scan_end = scan_start, cluster_start = scan_start, cluster_end = scan_start, bp_start = scan_start, bp_end = scan_start;
};

static void need_index(const Options &o)  // findEncompassingReadsAndBreakPointInfo loads the index for every group that reaches it (:405-416)
{
  if (!index_loads(o.inp_file))
  {
    std::cerr << "Error: please index bam-file first:\t" << o.inp_file << std::endl;
    exit(1);
  }
}

// one context: the stages of include/breakid_hip.h in the reference's order, with its stdout lines
static Run run_stages(const Options &o, Sample &t, const Exclusion &x)
{
  Run run;
  int rc;
  uint64_t n_pairs = 0, n_clusters = 0;
  uint32_t n_groups = 0;
  if ((rc = t.ensure_context(o.device)) != BK_OK) die(t, rc);
  if (o.exclude()) say_excluded(o, x, t.n_excluded, "");
  double mean = 0, sd = 0;
  if ((rc = bk_isize_stats(t.ctx, &mean, &sd)) != BK_OK) die(t, rc);
  std::cout << "the insert size mean: " << mean << ", the insert size sd:" << sd << " .\n";
  run.mean = mean, run.sd = sd;
  const int times = 2;
  run.w = times * std::sqrt(times) * (mean + 3 * sd);
  std::cout << "cluster_dist = span_dist = mask_dist = scan_dist = " << run.w << " .\n";
  run.scan_start = clock();
  std::cout << "Scanning discordant read pairs ...\n";
  if ((rc = bk_discordant_pairs(t.ctx, o.qual, run.w, &n_pairs, &n_groups)) != BK_OK) die(t, rc);
  std::cout << "Scanning discordant read pairs done.\n";
  run.scan_end = clock();
  run.cluster_start = clock();
  if ((rc = bk_mask_and_cluster(t.ctx, run.w, o.fast ? 1 : 0, &run.n_clustered)) != BK_OK) die(t, rc);
  run.cluster_end = clock();
  run.bp_start = clock();
  if ((rc = bk_split_evidence(t.ctx, nullptr)) != BK_OK) die(t, rc);
  if ((rc = bk_cluster_summary(t.ctx, run.w, &n_clusters)) != BK_OK) die(t, rc);
  if (run.n_clustered) need_index(o);
  if ((rc = bk_split_breakpoints(t.ctx, run.w, &run.n_valid)) != BK_OK) die(t, rc);
  run.bp_end = clock();
  return run;
}

// -gpus N: one sample over N GPUs, record ranges per rank, RCCL (or in-process) exchange of the small tables.  The GPU feed per rank
// first (bk_bam_decode_device_part); files it cannot cut into parts (records across BGZF blocks) and anything else it refuses go
// through the host decoder and the record ranges of its table.  -x: the _ex entry points, every rank excludes on its own table before
// the record bases are counted.  n_valid is counted from the cluster table by the caller.
static Run run_sharded(const Options &o, Sample &t, const Exclusion &x)
{
  Run run;
  char err[512];
  const bool from_file = !getenv("BREAKID_HOST_DECODE");
  const int fast = o.fast ? 1 : 0;
  int rc = BK_ERR_IO;
  if (from_file)
    rc = o.exclude() ? bk_multi_run_bam_ex(o.inp_file.c_str(), &x.regions, o.n_gpus, o.transport, o.qual, fast, &run.w, &run.n_clustered, &t.ctx, &t.nt, &t.names, &t.lens, err,
                                           sizeof err)
                     : bk_multi_run_bam(o.inp_file.c_str(), o.n_gpus, o.transport, o.qual, fast, &run.w, &run.n_clustered, &t.ctx, &t.nt, &t.names, &t.lens, err, sizeof err);
  if (rc != BK_OK && (!from_file || rc == BK_ERR_IO || rc == BK_ERR_LIMIT))
  {
    t.host_decode();  // (with BREAKID_HOST_DECODE=1 a second time: decode_tumor has read the table already)
    rc = o.exclude() ? bk_multi_run_ex(&t.soa, t.lens, t.names, t.nt, &x.regions, o.n_gpus, o.transport, o.qual, fast, &run.w, &run.n_clustered, &t.ctx, err, sizeof err)
                     : bk_multi_run(&t.soa, t.lens, t.names, t.nt, o.n_gpus, o.transport, o.qual, fast, &run.w, &run.n_clustered, &t.ctx, err, sizeof err);
  }
  if (rc != BK_OK)
  {
    std::cerr << (rc == BK_ERR_CIGAR ? "error cigar: " : err) << std::endl;
    exit(rc == BK_ERR_CIGAR ? -1 : 1);
  }
  if (o.exclude())
  {
    (void) bk_multi_excluded(t.ctx, &t.n_excluded);
    say_excluded(o, x, t.n_excluded, "");
  }
  double mean = 0, sd = 0;
  (void) bk_multi_stats(t.ctx, &mean, &sd, nullptr, nullptr);
  std::cout << "the insert size mean: " << mean << ", the insert size sd:" << sd << " .\n";
  std::cout << "cluster_dist = span_dist = mask_dist = scan_dist = " << run.w << " .\n";
  std::cout << "Scanning discordant read pairs ...\n";
  std::cout << "Scanning discordant read pairs done.\n";
  if (run.n_clustered) need_index(o);
  return run;
}

// -normal: decoded now (both record tables stay resident), then only its record-level stages; the per-call search is bk_normal_support
static void run_normal(const Options &o, Sample &normal, const Sample &tumor, const Exclusion &x, double w)
{
  if (!normal.gpu_decode(o)) normal.host_decode();
  bk_feed_release_caches();
  bool same = normal.nt == tumor.nt;
  for (int i = 0; same && i < tumor.nt; ++i) same = !strcmp(normal.names[i], tumor.names[i]) && normal.lens[i] == tumor.lens[i];
  if (!same)
  {
    std::cerr << "Error: tumor and normal BAM headers differ" << std::endl;
    exit(1);
  }
  if (o.exclude())
  {
    normal.exclude(o, x.regions);
    say_excluded(o, x, normal.n_excluded, "of the normal ");
  }
  if (normal.ensure_context(o.device) != BK_OK || bk_isize_stats(normal.ctx, nullptr, nullptr) != BK_OK ||
      bk_discordant_pairs(normal.ctx, o.qual, w, nullptr, nullptr) != BK_OK || bk_split_evidence(normal.ctx, nullptr) != BK_OK)
    die(normal, 0);
}

// ---- the per-call tables -----------------------------------------------------------------------------------------------------------
// one call of the library that gives rows and their count: the rows are copied (they are the library's until its next call)
template <class T, class Call>
static void fetch_rows(const Sample &tumor, vector<T> &into, Call call)
{
  const T *rows = nullptr;
  uint64_t n = 0;
  const int rc = call(&rows, &n);
  if (rc != BK_OK) die(tumor, rc);
  into.assign(rows, rows + n);
}

static void fetch_call_tables(const Options &o, const Sample &tumor, const Sample &normal, double w, CallTables &t)
{
  bk_ctx *ctx = tumor.ctx;
  const int qual = o.qual, anchor = (int) o.anchor, min_clip = (int) o.min_clip;
  // -normal: the normal's pairs, split reads and depth at every call of the sample
  if (normal.ctx) fetch_rows(tumor, t.nsup, [&](auto rows, auto n) { return bk_normal_support(ctx, normal.ctx, w, rows, n); });
  // -genotype: reference-allele counts of every call on the sample's own records, then on the normal's (both record tables are still
  // resident: the contexts and the decoded tables are released at the end)
  if (o.genotype) fetch_rows(tumor, t.gsup, [&](auto rows, auto n) { return bk_ref_support(ctx, ctx, qual, anchor, w, rows, n); });
  if (o.genotype && normal.ctx) fetch_rows(tumor, t.gsup_normal, [&](auto rows, auto n) { return bk_ref_support(ctx, normal.ctx, qual, anchor, w, rows, n); });
  // -vcf: the junction evidence of every call (member pairs by strands, split tuples by clip side)
  if (o.vcf || o.clip || o.consensus || o.coverage || o.frame || o.known() || o.bedpe || o.context || o.link || o.fragsize) fetch_rows(tumor, t.jsup, [&](auto rows, auto n) { return bk_junctions(ctx, rows, n); });
  // -clip: the clipped reads without an SA tag at every cluster, voted or not, on the sample's records and on the normal's
  if (o.clip) fetch_rows(tumor, t.csup, [&](auto rows, auto n) { return bk_clip_support(ctx, ctx, qual, min_clip, w, rows, n); });
  if (o.clip && normal.ctx) fetch_rows(tumor, t.csup_normal, [&](auto rows, auto n) { return bk_clip_support(ctx, normal.ctx, qual, min_clip, w, rows, n); });
  const void *data = nullptr;
  const int rc = bk_fetch(ctx, BK_STAGE_CLUSTERS, &data, &t.cnt, nullptr, nullptr);
  if (rc != BK_OK) die(tumor, rc);
  t.cl = (const bk_cluster *) data;
  // -evidence: the reads behind every call (one row per member pair and per matching split tuple), listed on the device
  if (o.evidence || o.consensus)
  {
    const uint64_t *off = nullptr;
    fetch_rows(tumor, t.ev_rows, [&](auto rows, auto n) { return bk_evidence(ctx, rows, n, &off); });
    t.ev_off.assign(off, off + t.cnt + 1);
  }
  // -dedup: the different fragments among those rows, per call, and for every row the first row of its fragment
  if (o.dedup)
  {
    const uint64_t *first = nullptr;
    uint64_t n_first = 0;
    fetch_rows(tumor, t.usup, [&](auto rows, auto n) { return bk_unique_support(ctx, rows, n, &first, &n_first); });
    t.ufirst.assign(first, first + n_first);
    if (t.usup.size() != t.cnt)
    {
      std::cerr << "Error: the unique-support table does not cover every cluster" << std::endl;
      exit(1);
    }
  }
}

// ---- the rows of the files ---------------------------------------------------------------------------------------------------------
// the reference reads refGene.txt for every group that reaches findClusterBreakPointInfoSaTag and exits if it is missing
static vector<Txpt> read_transcripts(const CallTables &t, uint64_t n_clustered)
{
  vector<Txpt> txpts;
  bool have_valid = false;
  for (uint64_t i = 0; i < t.cnt; ++i) have_valid |= (t.cl[i].flags & 2u) != 0;
  if (n_clustered >= 1 || have_valid)
  {
    const char *inst = getenv("BREAKID_INSTALLDIR");
    string ref_gene = string(inst ? inst : BREAKID_INSTALLDIR) + "/ref_files/refGene.txt";
    if (!read_refgene(ref_gene, txpts))
    {
      std::cerr << "Error: cannot open \t" << ref_gene << std::endl;
      exit(1);
    }
  }
  return txpts;
}

// annotate_cluster_for_sa_tag (BreakID.cc:492-567), then write_enspan_out's std::sort with the reference's comparator (:1184-1263)
static vector<OutRow> voted_rows(const Options &o, const Sample &tumor, const CallTables &t, const vector<Txpt> &txpts)
{
  vector<OutRow> rows;
  for (uint64_t i = 0; i < t.cnt; ++i)
  {
    if (!(t.cl[i].flags & 2u)) continue;
    OutRow r;
    r.c = t.cl[i];
    r.idx = i;
    annotate(r, txpts, o.nib_dir, tumor.names);
    r.af1 = (float) (long) r.c.n_sr / (float) (double) r.c.depth1;  // :475-478
    r.af2 = (float) (long) r.c.n_sr / (float) (double) r.c.depth2;
    rows.push_back(r);
  }
  std::sort(rows.begin(), rows.end(), cmp_cluster);
  return rows;
}

// -clip: the unvoted clusters whose clipped reads pile up on both sides (bk_clip_rescue), as rows of their own: the peaks are their
// breakpoints, N_SR is 0, the depth is counted at the peaks
static vector<OutRow> rescued_rows(const Options &o, const Sample &tumor, const Sample &normal, const CallTables &t, const vector<Txpt> &txpts)
{
  if (t.csup.size() != t.cnt || t.jsup.size() != t.cnt || (normal.ctx && t.csup_normal.size() != t.cnt))
  {
    std::cerr << "Error: the clip evidence does not cover every cluster" << std::endl;
    exit(1);
  }
  vector<OutRow> rescued;
  vector<int32_t> q_tid;
  vector<uint32_t> q_pos;
  for (uint64_t i = 0; i < t.cnt; ++i)
  {
    uint32_t pos1 = 0, pos2 = 0, n1 = 0, n2 = 0;
    const int found = bk_clip_rescue(&t.cl[i], &t.jsup[i], &t.csup[i], (uint32_t) o.clip_support, &pos1, &pos2, &n1, &n2);
    if (found < 0)
    {
      std::cerr << "Error: bk_clip_rescue refused its arguments" << std::endl;
      exit(1);
    }
    if (found != 1) continue;
    OutRow r;
    r.c = t.cl[i];
    r.idx = i;
    r.c.p1_exact = pos1;
    r.c.p2_exact = (int32_t) pos2;
    r.c.n_sr = 0;
    rescued.push_back(r);
    q_tid.insert(q_tid.end(), {t.cl[i].p1_tid, t.cl[i].p2_tid});
    q_pos.insert(q_pos.end(), {pos1, pos2});
  }
  const uint32_t *depth = nullptr;
  const int rc = bk_base_depth(tumor.ctx, q_tid.data(), q_pos.data(), q_tid.size(), &depth);
  if (rc != BK_OK) die(tumor, rc);
  for (size_t k = 0; k < rescued.size(); ++k)
  {
    OutRow &r = rescued[k];
    r.c.depth1 = depth[2 * k];
    r.c.depth2 = depth[2 * k + 1];
    annotate(r, txpts, o.nib_dir, tumor.names);
    r.af1 = r.af2 = 0.0f;  // no split read: 0 of any depth, and 0 where the depth is 0
  }
  std::cout << "rescued cluster count: " << rescued.size() << std::endl;
  std::sort(rescued.begin(), rescued.end(), cmp_cluster);
  return rescued;
}

// The rescued calls (the rows _fusion_rescued.txt writes, in its order): their two sites (ps_tid, peak, d_s), for the normal's counts
// (-normal), the VCF records (-vcf) and the clipped reads themselves (-evidence)
static void describe_rescued(const Options &o, const Sample &tumor, const Sample &normal, const CallTables &t, Rescued &rescued)
{
  rescued.calls.assign(rescued.rows.size(), RescuedCall());
  if (!o.clip || !(normal.ctx || o.vcf || o.evidence)) return;
  const int min_clip = (int) o.min_clip;
  vector<struct bk_clip_site> sites;
  vector<size_t> written;
  for (size_t k = 0; k < rescued.rows.size(); ++k)
  {
    const OutRow &r = rescued.rows[k];
    RescuedCall &call = rescued.calls[k];
    uint8_t source = 0;
    bk_junction_sides(&t.jsup[r.idx], &call.right[0], &call.right[1], &source);
    for (int s = 0; s < 2; ++s) call.peak_n[s] = t.csup[r.idx].peak_n[s][call.right[s]];
    if (!rescued_written(r, o.all)) continue;
    written.push_back(k);
    sites.push_back(bk_clip_site{r.c.p1_tid, r.c.p1_exact, 0u, call.right[0]});
    sites.push_back(bk_clip_site{r.c.p2_tid, (uint32_t) r.c.p2_exact, 0u, call.right[1]});
  }
  if (o.evidence)
  {
    const uint32_t *counts = nullptr;
    const struct bk_clip_read *cr = nullptr;
    const uint64_t *off = nullptr;
    const int rc = bk_clip_reads(tumor.ctx, sites.data(), sites.size(), o.qual, min_clip, &counts, &cr, &off);
    if (rc != BK_OK) die(tumor, rc);
    rescued.read_off.assign(off, off + sites.size() + 1);
    rescued.reads.assign(cr, cr + off[sites.size()]);
  }
  if (!normal.ctx) return;
  // the +-2 bp of every other count of the normal
  vector<int32_t> q_tid;
  vector<uint32_t> q_pos;
  for (struct bk_clip_site &x : sites)
  {
    x.tol = 2;
    q_tid.push_back(x.tid);
    q_pos.push_back(x.pos);
  }
  const uint32_t *counts = nullptr, *depth = nullptr;
  if (bk_clip_reads(normal.ctx, sites.data(), sites.size(), o.qual, min_clip, &counts, nullptr, nullptr) != BK_OK) die(normal, 0);
  if (bk_base_depth(normal.ctx, q_tid.data(), q_pos.data(), q_tid.size(), &depth) != BK_OK) die(normal, 0);
  for (size_t j = 0; j < written.size(); ++j)
  {
    RescuedCall &call = rescued.calls[written[j]];
    const uint64_t idx = rescued.rows[written[j]].idx;
    call.normal_drp = idx < t.nsup.size() ? t.nsup[idx].n_drp : 0;
    for (int s = 0; s < 2; ++s)
    {
      call.normal_at[s] = counts[2 * j + s];
      call.normal_depth[s] = depth[2 * j + s];
    }
  }
}

// ---- -consensus: the clipped bases at the two breakpoints of every written call ----------------------------------------------------
// What the vote leaves: per written call its two sides, and for -homology the sites (2 per call of site_call, in its order) with the
// library's rows and bases (its own until the next bk_clip_consensus)
struct JunctionConsensus
{
  ConsensusMap sides;
  vector<struct bk_clip_site> sites;
  vector<uint64_t> site_call;
  const struct bk_consensus *rows = nullptr;
  const uint8_t *bases = nullptr;
};

// Sites: side s of a call is (ps_tid, ps_exact, 0, d_s), d_s from bk_junction_sides.  Reads: those of the call's BK_EV_SPLIT rows, and
// those bk_clip_reads lists at the sites (the reads without an SA tag), each name once.  One pass over the file brings their alignments
// back with the bases, one call piles them up.
static void junction_consensus(const Options &o, const Sample &tumor, const CallTables &t, const vector<OutRow> &rows, JunctionConsensus &jc)
{
  const int min_clip = (int) o.min_clip;
  std::set<std::pair<uint64_t, uint32_t>> seen;
  vector<bk_read_key> keys;
  auto add_key = [&](uint64_t qhash, uint32_t qcheck) {
    if (seen.emplace(qhash, qcheck).second) keys.push_back(bk_read_key{qhash, qcheck, 0});
  };
  for (const OutRow &r : rows)
  {
    if (!call_written(r, o.all)) continue;
    if (r.idx >= t.jsup.size() || r.idx + 1 >= t.ev_off.size() || t.ev_off[r.idx + 1] > t.ev_rows.size())
    {
      std::cerr << "Error: the evidence tables do not cover every call" << std::endl;
      exit(1);
    }
    uint8_t right[2] = {0, 1}, source = 0;
    bk_junction_sides(&t.jsup[r.idx], &right[0], &right[1], &source);
    jc.site_call.push_back(r.idx);
    jc.sites.push_back(bk_clip_site{r.c.p1_tid, r.c.p1_exact, 0u, right[0]});
    jc.sites.push_back(bk_clip_site{r.c.p2_tid, (uint32_t) r.c.p2_exact, 0u, right[1]});
    for (uint64_t i = t.ev_off[r.idx]; i < t.ev_off[r.idx + 1]; ++i)
      if (t.ev_rows[i].kind == BK_EV_SPLIT) add_key(t.ev_rows[i].qhash, t.ev_rows[i].qcheck);
  }
  const uint32_t *counts = nullptr;
  const struct bk_clip_read *cr = nullptr;
  const uint64_t *off = nullptr;
  int rc = bk_clip_reads(tumor.ctx, jc.sites.data(), jc.sites.size(), o.qual, min_clip, &counts, &cr, &off);
  if (rc != BK_OK) die(tumor, rc);
  for (uint64_t i = 0; i < off[jc.sites.size()]; ++i) add_key(cr[i].qhash, cr[i].qcheck);
  bk_reads reads;
  char err[512] = "";
  if (bk_bam_reads(o.inp_file.c_str(), keys.data(), keys.size(), &reads, err, sizeof err) != BK_OK)
  {
    std::cerr << "Error: cannot read the clipped reads back from " << o.inp_file << ": " << err << std::endl;
    exit(1);
  }
  rc = bk_clip_consensus(tumor.ctx, &reads, jc.sites.data(), jc.sites.size(), o.qual, min_clip, (uint32_t) o.conslen, CONSENSUS_MIN_DEPTH, &jc.rows, &jc.bases, nullptr);
  bk_reads_free(&reads);
  if (rc != BK_OK) die(tumor, rc);
  for (size_t x = 0; x < jc.sites.size(); ++x)
  {
    std::pair<ConsensusSide, ConsensusSide> &both = jc.sides[jc.site_call[x / 2]];
    ConsensusSide &side = (x & 1) ? both.second : both.first;
    side.c = jc.rows[x];
    side.seq.assign((const char *) jc.bases + x * (size_t) o.conslen, side.c.len);
    if (jc.sites[x].dir == 1u) std::reverse(side.seq.begin(), side.seq.end());
  }
}

// ---- -homology: the junction fit of the same sides ---------------------------------------------------------------------------------
// the nib files of the run, each opened once
struct NibFiles
{
  const Options &o;
  const Sample &sample;
  std::map<int32_t, std::unique_ptr<Nib>> files;
  string path(int32_t tid) const { return o.nib_dir + "/hg19_" + string(sample.names[tid]) + ".nib"; }
  Nib *of(int32_t tid)  // null without a readable file
  {
    if (tid < 0 || tid >= sample.nt) return nullptr;
    auto it = files.find(tid);
    if (it == files.end())
    {
      it = files.emplace(tid, std::unique_ptr<Nib>(new Nib)).first;
      it->second->open(path(tid));
    }
    return it->second->ok ? it->second.get() : nullptr;
  }
};

// Stretches of the reference as bk_junction_fit takes them (bk_refseq): segments ascending by (tid, start), each starting on a byte of
// its nib file, two bases per byte
struct RefWindows
{
  vector<int32_t> tid;
  vector<uint32_t> start, len;
  vector<uint64_t> off = vector<uint64_t>(1, 0);
  vector<uint8_t> bases;
  bk_refseq refseq() const
  {
    bk_refseq ref;
    ref.n_segs = tid.size();
    ref.tid = tid.data();
    ref.start = start.data();
    ref.len = len.data();
    ref.off = off.data();
    ref.bases = bases.data();
    return ref;
  }
  char base(int32_t t, long pos1) const  // the base at a 1-based position (N outside the segments)
  {
    static const char tab[8] = {'T', 'C', 'A', 'G', 'N', 'N', 'N', 'N'};
    size_t lo = 0, hi = tid.size();  // the last segment that starts at or before pos1
    while (lo < hi)
    {
      const size_t mid = lo + (hi - lo) / 2;
      if (tid[mid] < t || (tid[mid] == t && (long) start[mid] <= pos1 - 1))
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo == 0 || tid[lo - 1] != t) return 'N';
    const long i = pos1 - 1 - (long) start[lo - 1];
    if (i < 0 || i >= (long) len[lo - 1]) return 'N';
    const uint8_t byte = bases[off[lo - 1] + (size_t) (i / 2)];
    return tab[((i & 1) ? byte : byte >> 4) & 7];
  }
};

// per contig the 1-based windows [a, b]: merged where they touch, one segment per merged window, read from the contig's nib file
static RefWindows read_ref_windows(std::map<int32_t, vector<std::pair<long, long>>> &spans, NibFiles &nibs)
{
  RefWindows ref;
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
    Nib *nb = nibs.of(kv.first);
    for (const auto &w : merged)
    {
      const long start0 = (w.first - 1) & ~1l;  // a segment starts on a byte of the file
      const long len = w.second - start0;
      const size_t at = ref.bases.size(), nbytes = (size_t) ((len + 1) / 2);
      ref.bases.resize(at + nbytes);
      nb->in.clear();
      nb->in.seekg(8 + start0 / 2);
      nb->in.read((char *) ref.bases.data() + at, (std::streamsize) nbytes);
      if ((size_t) nb->in.gcount() != nbytes)
      {
        std::cerr << "Error: " << nibs.path(kv.first) << " is shorter than its header says" << std::endl;
        exit(1);
      }
      ref.tid.push_back(kv.first);
      ref.start.push_back((uint32_t) start0);
      ref.len.push_back((uint32_t) len);
      ref.off.push_back(ref.bases.size());
    }
  }
  return ref;
}

// One probe per side with a consensus, own = the side's site, mate = the other side's; the query is the side's row of the consensus
// bases as it lies.  The reference: the windows around every probe position.  One call fits every probe of the run.
static HomologyMap junction_homology(const Options &o, const Sample &tumor, const JunctionConsensus &jc)
{
  NibFiles nibs{o, tumor, {}};
  const size_t conslen = (size_t) o.conslen;
  const long radius = o.conslen + o.homshift + (long) HOMOLOGY_MAX_HOM + 1;
  vector<struct bk_junction_probe> probes;
  vector<size_t> probe_site;
  vector<uint8_t> query;
  std::map<int32_t, vector<std::pair<long, long>>> spans;
  for (size_t x = 0; x < jc.sites.size(); ++x)
  {
    const struct bk_clip_site &own = jc.sites[x], &mate = jc.sites[x ^ 1];
    if (jc.rows[x].len == 0 || !nibs.of(own.tid) || !nibs.of(mate.tid)) continue;
    probes.push_back(bk_junction_probe{own.tid, own.pos, own.dir, mate.tid, mate.pos, mate.dir, jc.rows[x].len, 0u});
    probe_site.push_back(x);
    query.insert(query.end(), jc.bases + x * conslen, jc.bases + (x + 1) * conslen);
    for (const struct bk_clip_site *e : {&own, &mate})
    {
      const long a = std::max(1l, (long) e->pos - radius), b = std::min((long) nibs.of(e->tid)->nBases, (long) e->pos + radius);
      if (a <= b) spans[e->tid].emplace_back(a, b);
    }
  }
  const RefWindows windows = read_ref_windows(spans, nibs);
  const bk_refseq ref = windows.refseq();
  const struct bk_junction_fit *fit = nullptr;
  const int rc = bk_junction_fit(tumor.ctx, &ref, probes.data(), probes.size(), query.data(), (uint32_t) o.conslen, (uint32_t) o.homshift, (uint32_t) o.homins, HOMOLOGY_MAX_HOM, &fit);
  if (rc != BK_OK) die(tumor, rc);
  HomologyMap hom;
  for (uint64_t call : jc.site_call) hom[call];
  for (size_t k = 0; k < probes.size(); ++k)
  {
    if (!fit[k].placed) continue;
    const size_t x = probe_site[k];
    std::pair<HomologySide, HomologySide> &both = hom[jc.site_call[x / 2]];
    HomologySide &side = (x & 1) ? both.second : both.first;
    side.on = true;
    side.f = fit[k];
    const long pos = probes[k].pos_own, fwd = fit[k].hom_fwd, back = fit[k].hom_back;
    const bool right = probes[k].dir_own == 1u;
    for (long p = right ? pos - fwd : pos - back + 1; p <= (right ? pos + back - 1 : pos + fwd); ++p) side.hom_seq += windows.base(probes[k].tid_own, p);
    side.ins_seq.assign((const char *) query.data() + k * conslen, fit[k].ins);
    if (right) std::reverse(side.ins_seq.begin(), side.ins_seq.end());
  }
  return hom;
}

// ---- -similar: the reference around the two breakpoints of every written call against each other -----------------------------------
// One pair per written call whose two contigs have a nib file; the reference: the windows [pos - R, pos + R] around every position,
// clamped to the contig.  One call scores every pair of the run.
static SimilarMap locus_similar(const Options &o, const Sample &tumor, const vector<OutRow> &rows)
{
  NibFiles nibs{o, tumor, {}};
  const long R = o.simflank;
  vector<struct bk_locus_pair> pairs;
  vector<uint64_t> pair_call;
  std::map<int32_t, vector<std::pair<long, long>>> spans;
  SimilarMap sim;
  for (const OutRow &r : rows)
  {
    if (!call_written(r, o.all)) continue;
    sim[r.idx];
    if (!nibs.of(r.c.p1_tid) || !nibs.of(r.c.p2_tid)) continue;
    const struct bk_locus_pair p = {r.c.p1_tid, r.c.p1_exact, r.c.p2_tid, (uint32_t) r.c.p2_exact};
    pairs.push_back(p);
    pair_call.push_back(r.idx);
    for (int e = 0; e < 2; ++e)
    {
      const int32_t tid = e ? p.tid_b : p.tid_a;
      const long pos = e ? (long) p.pos_b : (long) p.pos_a;
      const long a = std::max(1l, pos - R), b = std::min((long) nibs.of(tid)->nBases, pos + R);
      if (a <= b) spans[tid].emplace_back(a, b);
    }
  }
  const RefWindows windows = read_ref_windows(spans, nibs);
  const bk_refseq ref = windows.refseq();
  const struct bk_locus_sim *res = nullptr;
  const int rc = bk_locus_similarity(tumor.ctx, &ref, pairs.data(), pairs.size(), (uint32_t) R, &res);
  if (rc != BK_OK) die(tumor, rc);
  for (size_t k = 0; k < pairs.size(); ++k)
  {
    SimilarCall &c = sim[pair_call[k]];
    c.on = true;
    c.s = res[k];
    const long first = (long) c.s.start + c.s.diag;  // the stretch's first column of window B in the orientation it was found in
    c.pos1 = (long) pairs[k].pos_a - R + (long) c.s.start;
    c.pos2 = c.s.orient ? (long) pairs[k].pos_b + R - (first + (long) c.s.len - 1) : (long) pairs[k].pos_b - R + first;
  }
  return sim;
}

// ---- -complexity: the reference around each breakpoint of every written call described by itself ---------------------------------
// Two sites per written call, a side on a contig without a nib file left out; the reference: the windows [pos - R, pos + R] around
// every site, clamped to the contig.  One call describes every site of the run.
static ComplexityMap site_complexity(const Options &o, const Sample &tumor, const vector<OutRow> &rows)
{
  NibFiles nibs{o, tumor, {}};
  const long R = o.cplxflank;
  vector<struct bk_ref_site> sites;
  vector<std::pair<uint64_t, int>> site_side;  // the call and the side of it
  std::map<int32_t, vector<std::pair<long, long>>> spans;
  ComplexityMap cplx;
  for (const OutRow &r : rows)
  {
    if (!call_written(r, o.all)) continue;
    cplx[r.idx];
    for (int e = 0; e < 2; ++e)
    {
      const struct bk_ref_site s = {e ? r.c.p2_tid : r.c.p1_tid, e ? (uint32_t) r.c.p2_exact : r.c.p1_exact};
      if (!nibs.of(s.tid)) continue;
      sites.push_back(s);
      site_side.emplace_back(r.idx, e);
      const long a = std::max(1l, (long) s.pos - R), b = std::min((long) nibs.of(s.tid)->nBases, (long) s.pos + R);
      if (a <= b) spans[s.tid].emplace_back(a, b);
    }
  }
  const RefWindows windows = read_ref_windows(spans, nibs);
  const bk_refseq ref = windows.refseq();
  const struct bk_site_cplx *res = nullptr;
  const int rc = bk_site_complexity(tumor.ctx, &ref, sites.data(), sites.size(), (uint32_t) R, (uint32_t) o.cplxperiod, &res);
  if (rc != BK_OK) die(tumor, rc);
  const uint32_t LOG_TRACT = 12;  // only what the log line below counts: no column and no filter looks at it
  size_t n_tract = 0, n_masked = 0;
  for (size_t k = 0; k < sites.size(); ++k)
  {
    ComplexitySide &c = site_side[k].second ? cplx[site_side[k].first].second : cplx[site_side[k].first].first;
    c.on = true;
    c.c = res[k];
    const long first = (long) sites[k].pos - R;  // the position of column 0
    c.bp_pos = first + (long) c.c.bp_start;
    c.max_pos = first + (long) c.c.max_start;
    for (uint32_t j = 0; j < c.c.bp_period; ++j) c.bp_unit += windows.base(sites[k].tid, c.bp_pos + j);
    for (uint32_t j = 0; j < c.c.max_period; ++j) c.max_unit += windows.base(sites[k].tid, c.max_pos + j);
    n_tract += c.c.bp_len >= LOG_TRACT;
    n_masked += c.c.mask_run > 0;
  }
  std::cout << "complexity: " << sites.size() << " sites, " << n_tract << " with a tract of " << LOG_TRACT << " or more columns at the breakpoint, " << n_masked
            << " with the breakpoint base soft-masked" << std::endl;
  return cplx;
}

// ---- -coverage: the mean depth beside and between the breakpoints of every written call -------------------------------------------
// Five windows per written call (bk_call_windows, with the sides -vcf uses) and one per contig that carries a call; one call of
// bk_window_coverage answers them all on the sample's records, a second one on the normal's.
static CoverageMap call_coverage(const Options &o, const Sample &tumor, const Sample &normal, const CallTables &t, const vector<OutRow> &rows)
{
  CoverageMap cov;
  vector<struct bk_cov_window> windows;
  vector<uint64_t> window_call;
  std::map<int32_t, size_t> contig_at;  // the contig's window, counted from the first of them
  for (const OutRow &r : rows)
  {
    if (!call_written(r, o.all)) continue;
    if (r.idx >= t.jsup.size())
    {
      std::cerr << "Error: the evidence tables do not cover every call" << std::endl;
      exit(1);
    }
    uint8_t right[2] = {0, 1}, source = 0;
    bk_junction_sides(&t.jsup[r.idx], &right[0], &right[1], &source);
    CoverageCall &c = cov[r.idx];
    if (bk_call_windows(&r.c, right[0], right[1], (uint32_t) o.covflank, tumor.lens, c.w) != BK_OK) die(tumor, BK_ERR_ARG);
    c.cut[0] = (long long) r.c.p1_exact - right[0];
    c.cut[1] = (long long) r.c.p2_exact - right[1];
    window_call.push_back(r.idx);
    windows.insert(windows.end(), c.w, c.w + 5);
    for (int32_t tid : {r.c.p1_tid, r.c.p2_tid})
      if (tid >= 0) contig_at.emplace(tid, 0);
  }
  const size_t first_contig = windows.size();
  for (auto &at : contig_at)
  {
    at.second = windows.size() - first_contig;
    windows.push_back(bk_cov_window{at.first, 0u, tumor.lens[at.first], 0u});
  }
  auto count = [&](const Sample &sample, bool is_normal) {
    const struct bk_window_cov *res = nullptr;
    const int rc = bk_window_coverage(sample.ctx, windows.data(), windows.size(), o.qual, &res);
    if (rc != BK_OK) die(sample, rc);
    for (size_t k = 0; k < window_call.size(); ++k)
    {
      CoverageCall &c = cov[window_call[k]];
      struct bk_window_cov *into = is_normal ? c.normal : c.tumor;
      std::copy(res + 5 * k, res + 5 * k + 5, into);
      for (int s = 0; s < 2; ++s)
      {
        const int32_t tid = c.w[2 * s].tid;
        c.w[5 + s] = tid >= 0 ? windows[first_contig + contig_at.at(tid)] : bk_cov_window{tid, 0u, 0u, 0u};
        into[5 + s] = tid >= 0 ? res[first_contig + contig_at.at(tid)] : bk_window_cov{0, 0, 0};
      }
    }
  };
  count(tumor, false);
  if (normal.ctx) count(normal, true);
  return cov;
}

// ---- -frame: the 5' / 3' partners and the reading frame of every written call ------------------------------------------------------
// The model: the transcripts the run read from refGene.txt (NR_ rows are not among them), their coding parts as parse_refgene_line left
// them, on the contigs of the BAM header by exact name, sorted by (tid, txStart) with the file's order kept among equals.  One site per
// written call, with the sides -vcf prints; one call of bk_fusion_frame answers them all.
static FrameMap fusion_frames(const Options &o, const Sample &tumor, const CallTables &t, const vector<OutRow> &rows, const vector<Txpt> &txpts)
{
  std::map<string, int32_t> tid_of;
  for (int i = 0; i < tumor.nt; ++i) tid_of.emplace(tumor.names[i], i);
  vector<std::pair<int32_t, const Txpt *>> kept;
  size_t dropped = 0;
  for (const Txpt &x : txpts)
  {
    const auto at = tid_of.find(x.chrom);
    if (at == tid_of.end())
      ++dropped;
    else
      kept.emplace_back(at->second, &x);
  }
  std::stable_sort(kept.begin(), kept.end(), [](const auto &a, const auto &b) { return a.first != b.first ? a.first < b.first : a.second->txStart < b.second->txStart; });
  std::cout << "frame model: " << kept.size() << " transcripts, " << dropped << " on contigs the input lacks" << std::endl;
  vector<int32_t> tid;
  vector<uint32_t> tx_start, tx_end, ex_off{0}, ex_start, ex_end;
  vector<uint8_t> strand;
  for (const auto &k : kept)
  {
    const Txpt &x = *k.second;
    tid.push_back(k.first);
    tx_start.push_back(x.txStart);
    tx_end.push_back(x.txEnd);
    strand.push_back(x.strand == "-" ? 1 : 0);
    ex_start.insert(ex_start.end(), x.codingStarts.begin(), x.codingStarts.end());
    ex_end.insert(ex_end.end(), x.codingEnds.begin(), x.codingEnds.end());
    ex_off.push_back((uint32_t) ex_start.size());
  }
  bk_txmodel model{};
  model.n_tx = kept.size();
  model.n_parts = ex_start.size();
  model.tid = tid.data(), model.tx_start = tx_start.data(), model.tx_end = tx_end.data(), model.strand = strand.data();
  model.ex_off = ex_off.data(), model.ex_start = ex_start.data(), model.ex_end = ex_end.data();

  vector<struct bk_frame_site> sites;
  vector<uint64_t> site_call;
  for (const OutRow &r : rows)
  {
    if (!call_written(r, o.all)) continue;
    if (r.idx >= t.jsup.size())
    {
      std::cerr << "Error: the evidence tables do not cover every call" << std::endl;
      exit(1);
    }
    uint8_t right[2] = {0, 1}, source = 0;
    bk_junction_sides(&t.jsup[r.idx], &right[0], &right[1], &source);
    struct bk_frame_site s = {};
    s.tid1 = r.c.p1_tid, s.pos1 = r.c.p1_exact, s.tid2 = r.c.p2_tid, s.pos2 = (uint32_t) r.c.p2_exact;
    s.right1 = right[0], s.right2 = right[1];
    sites.push_back(s);
    site_call.push_back(r.idx);
  }
  const struct bk_frame_call *res = nullptr;
  const int rc = bk_fusion_frame(tumor.ctx, &model, sites.data(), sites.size(), &res);
  if (rc != BK_OK) die(tumor, rc);
  FrameMap frames;
  for (size_t k = 0; k < sites.size(); ++k)
  {
    FrameCall &c = frames[site_call[k]];
    c.f = res[k];
    for (int s = 0; s < 2; ++s)
      if (c.f.tx[s] >= 0 && (size_t) c.f.tx[s] < kept.size())
      {
        c.gene[s] = kept[c.f.tx[s]].second->geneName;
        c.tx[s] = kept[c.f.tx[s]].second->transcriptID;
      }
  }
  return frames;
}

// ---- -link: reciprocal partners, duplicates and events among the voted calls -----------------------------------------------------------
// One site per voted call, the calls of _fusion_all.txt, whether or not -all is given: a partner that the gene-pair filter removed is
// still evidence, and an event id then means the same in both files.  The sides are those -vcf prints; one call of bk_link_calls
// answers them all.  The sites stand in the order of their rows of BK_STAGE_CLUSTERS, so the smallest index of an event is its smallest
// row and a tie goes to the smaller row, whatever order the tables are written in.
static LinkMap link_calls(const Options &o, const Sample &tumor, const CallTables &t, const vector<OutRow> &rows)
{
  vector<const OutRow *> voted;
  for (const OutRow &r : rows)
    if (call_all_ok(r)) voted.push_back(&r);
  std::sort(voted.begin(), voted.end(), [](const OutRow *a, const OutRow *b) { return a->idx < b->idx; });
  vector<struct bk_link_site> sites;
  vector<uint64_t> site_call;
  for (const OutRow *v : voted)
  {
    const OutRow &r = *v;
    if (r.idx >= t.jsup.size())
    {
      std::cerr << "Error: the evidence tables do not cover every call" << std::endl;
      exit(1);
    }
    uint8_t right[2] = {0, 1}, source = 0;
    bk_junction_sides(&t.jsup[r.idx], &right[0], &right[1], &source);
    struct bk_link_site s = {};
    s.tid1 = r.c.p1_tid, s.pos1 = r.c.p1_exact, s.tid2 = r.c.p2_tid, s.pos2 = (uint32_t) r.c.p2_exact;
    s.right1 = right[0], s.right2 = right[1];
    sites.push_back(s);
    site_call.push_back(r.idx);
  }
  const struct bk_call_link *res = nullptr;
  const int rc = bk_link_calls(tumor.ctx, sites.data(), sites.size(), (uint32_t) o.linkdist, &res);
  if (rc != BK_OK) die(tumor, rc);
  LinkMap links;
  uint64_t events = 0, recip = 0;
  for (size_t k = 0; k < sites.size(); ++k)
  {
    LinkCall &c = links[site_call[k]];
    c.l = res[k];
    c.event_row = site_call[c.l.event];
    if (c.l.dup_of >= 0) c.dup_row = site_call[c.l.dup_of];
    if (c.l.mate >= 0) c.mate_row = site_call[c.l.mate];
    events += c.l.event == k && c.l.event_size > 1;
    recip += c.l.n_recip;
  }
  std::cout << "link: " << sites.size() << " calls, " << events << " events of more than one call, " << recip / 2 << " reciprocal pairs" << std::endl;
  return links;
}

// ---- -partners: where the discordant pairs inside the two windows of every written call point to --------------------------------------
// Two sites per written call (bk_call_partner_sites: the window of bk_normal_support.n_drp on either side, the other side's as its
// partner) and max_gap = (int) w, the run's own clustering distance; one call of bk_locus_partners answers them all on the sample's
// pairs, a second one on the normal's.
static PartnerMap locus_partners(const Options &o, const Sample &tumor, const Sample &normal, const vector<OutRow> &rows, double w)
{
  PartnerMap partners;
  vector<struct bk_partner_site> sites;
  vector<uint64_t> site_call;
  for (const OutRow &r : rows)
  {
    if (!call_written(r, o.all)) continue;
    struct bk_partner_site both[2];
    if (bk_call_partner_sites(&r.c, w, both) != BK_OK) die(tumor, BK_ERR_ARG);
    sites.insert(sites.end(), both, both + 2);
    site_call.push_back(r.idx);
  }
  const int W = (int) w;
  const uint32_t max_gap = W > 0 ? (uint32_t) W : 0u;
  auto chr = [&](int32_t tid) { return tid >= 0 && tid < tumor.nt ? string(tumor.names[tid]) : string("*"); };
  auto count = [&](const Sample &sample, bool is_normal) {
    const struct bk_locus_partners *res = nullptr;
    const int rc = bk_locus_partners(sample.ctx, sites.data(), sites.size(), max_gap, &res);
    if (rc != BK_OK) die(sample, rc);
    for (size_t k = 0; k < site_call.size(); ++k)
    {
      PartnerCall &c = partners[site_call[k]];
      for (int s = 0; s < 2; ++s)
      {
        (is_normal ? c.normal : c.tumor)[s] = res[2 * k + s];
        (is_normal ? c.normal_top_chr : c.top_chr)[s] = chr(res[2 * k + s].top_tid);
      }
    }
    return res;
  };
  const struct bk_locus_partners *res = count(tumor, false);
  uint64_t ends = 0, to_partner = 0;
  for (size_t k = 0; k < sites.size(); ++k) ends += res[k].ends, to_partner += res[k].to_partner;
  if (normal.ctx) count(normal, true);
  std::cout << "partners: " << site_call.size() << " calls, " << ends << " ends in their windows, " << to_partner << " of them to the partner" << std::endl;
  return partners;
}

// ---- -fragsize: the fragment lengths the member pairs of every written call imply across its junction ---------------------------------
// One site per BK_STAGE_CLUSTERS row, as bk_fragment_sizes wants them: a written call gets its voted positions and the sides -vcf prints,
// every other row is skipped.  The bounds are bk_fragment_bounds of the run's own insert sizes.
static FragsizeMap fragment_sizes(const Options &o, const Sample &tumor, const CallTables &t, const vector<OutRow> &rows, const Run &run)
{
  FragsizeMap frags;
  int32_t lo = 0, hi = 0;
  if (bk_fragment_bounds(run.mean, run.sd, &lo, &hi) != BK_OK) die(tumor, BK_ERR_ARG);
  vector<struct bk_frag_site> sites(t.cnt);
  for (struct bk_frag_site &s : sites)
  {
    s = bk_frag_site{};
    s.skip = 1;
  }
  vector<uint64_t> site_call;
  for (const OutRow &r : rows)
  {
    if (!call_written(r, o.all)) continue;
    if (r.idx >= t.jsup.size() || r.idx >= sites.size())
    {
      std::cerr << "Error: the evidence tables do not cover every call" << std::endl;
      exit(1);
    }
    uint8_t right[2] = {0, 1}, source = 0;
    bk_junction_sides(&t.jsup[r.idx], &right[0], &right[1], &source);
    struct bk_frag_site &s = sites[r.idx];
    s.pos1 = r.c.p1_exact, s.pos2 = (uint32_t) r.c.p2_exact;
    s.right1 = right[0], s.right2 = right[1];
    s.skip = 0;
    site_call.push_back(r.idx);
  }
  const struct bk_frag_sizes *res = nullptr;
  const int rc = bk_fragment_sizes(tumor.ctx, sites.data(), sites.size(), lo, hi, &res);
  if (rc != BK_OK) die(tumor, rc);
  uint64_t used = 0, off = 0, lost = 0;
  for (const uint64_t idx : site_call)
  {
    FragsizeCall &c = frags[idx];
    c.f = res[idx];
    c.mean = run.mean, c.sd = run.sd;
    used += c.f.n_used, off += c.f.n_off, lost += c.f.n_lost;
  }
  if (lost) std::cerr << "Warning: -fragsize found no record for " << lost << " pair rows; they are left out of the lengths" << std::endl;
  std::cout << "fragsize: " << site_call.size() << " calls, " << used << " pairs used, " << off << " off the junction's sides, library " << lo << "-" << hi << std::endl;
  return frags;
}

// ---- -known: every written call against the panel -----------------------------------------------------------------------------------------
// One site per written call, with the sides -vcf prints (a call without a side's evidence keeps LEFT, as elsewhere); one call of
// bk_known_calls answers them all.
static KnownMap known_calls(const Options &o, const Sample &tumor, const CallTables &t, const vector<OutRow> &rows, const KnownPanel &panel)
{
  vector<struct bk_known_site> sites;
  vector<uint64_t> site_call;
  for (const OutRow &r : rows)
  {
    if (!call_written(r, o.all)) continue;
    if (r.idx >= t.jsup.size())
    {
      std::cerr << "Error: the evidence tables do not cover every call" << std::endl;
      exit(1);
    }
    uint8_t right[2] = {0, 1}, source = 0;
    bk_junction_sides(&t.jsup[r.idx], &right[0], &right[1], &source);
    struct bk_known_site s = {};
    s.tid1 = r.c.p1_tid, s.pos1 = r.c.p1_exact, s.tid2 = r.c.p2_tid, s.pos2 = (uint32_t) r.c.p2_exact;
    s.right1 = source ? right[0] : 0, s.right2 = source ? right[1] : 0;
    sites.push_back(s);
    site_call.push_back(r.idx);
  }
  const struct bk_known_call *res = nullptr;
  const int rc = bk_known_calls(tumor.ctx, panel.entries.data(), panel.entries.size(), sites.data(), sites.size(), (uint32_t) o.knownslop, &res);
  if (rc != BK_OK) die(tumor, rc);
  KnownMap known;
  uint64_t with_hit = 0;
  for (size_t k = 0; k < sites.size(); ++k)
  {
    KnownCall &c = known[site_call[k]];
    c.k = res[k];
    if (c.k.best >= 0 && (size_t) c.k.best < panel.entries.size()) c.best_name = panel.names[panel.entries[c.k.best].name];
    with_hit += c.k.n_hits > 0;
  }
  std::cout << "known: " << panel.entries.size() << " entries, " << panel.unknown << " on contigs the input lacks, " << with_hit << " calls with a hit" << std::endl;
  return known;
}

// ---- -context: what the alignments that start beside the breakpoints of every written call look like -------------------------------
// The four flank windows of every written call (bk_call_windows with -ctxflank and the sides -vcf uses; the span window is left out);
// one call of bk_window_context answers them all on the sample's records, a second one on the normal's.  A side is the sum of its two
// windows' rows.
static ContextMap call_context(const Options &o, const Sample &tumor, const Sample &normal, const CallTables &t, const vector<OutRow> &rows)
{
  ContextMap ctx;
  vector<struct bk_cov_window> windows;
  vector<uint64_t> window_call;
  for (const OutRow &r : rows)
  {
    if (!call_written(r, o.all)) continue;
    if (r.idx >= t.jsup.size())
    {
      std::cerr << "Error: the evidence tables do not cover every call" << std::endl;
      exit(1);
    }
    uint8_t right[2] = {0, 1}, source = 0;
    bk_junction_sides(&t.jsup[r.idx], &right[0], &right[1], &source);
    struct bk_cov_window w[5];
    if (bk_call_windows(&r.c, right[0], right[1], (uint32_t) o.ctxflank, tumor.lens, w) != BK_OK) die(tumor, BK_ERR_ARG);
    ctx[r.idx];
    window_call.push_back(r.idx);
    windows.insert(windows.end(), w, w + 4);
  }
  auto count = [&](const Sample &sample, bool is_normal) {
    const struct bk_window_ctx *res = nullptr;
    const int rc = bk_window_context(sample.ctx, windows.data(), windows.size(), o.qual, &res);
    if (rc != BK_OK) die(sample, rc);
    for (size_t k = 0; k < window_call.size(); ++k)
    {
      ContextCall &c = ctx[window_call[k]];
      struct bk_window_ctx *into = is_normal ? c.normal : c.tumor;
      for (int j = 0; j < 4; ++j) ContextCall::add(into[j / 2], res[4 * k + j]);
    }
  };
  count(tumor, false);
  if (normal.ctx) count(normal, true);
  uint64_t reads = 0, mq0 = 0;
  for (const auto &at : ctx)
    for (int s = 0; s < 2; ++s) reads += at.second.tumor[s].reads, mq0 += at.second.tumor[s].mq0;
  std::cout << "context: " << window_call.size() << " calls, " << reads << " reads in their windows, " << mq0 << " of them with mapping quality 0" << std::endl;
  return ctx;
}

// ---- the files behind the tables ---------------------------------------------------------------------------------------------------
// -vcf: <prefix>_fusion.vcf, and with -clip <prefix>_fusion_rescued.vcf
static void write_vcf_files(const Options &o, const Sample &tumor, const CallTables &t, const vector<OutRow> &rows, const Rescued &rescued, const ConsensusMap &cons,
                            const HomologyMap &hom, const SimilarMap &sim, const CoverageMap &cov, const FrameMap &frame, const LinkMap &link,
                            const PartnerMap &partners, const FragsizeMap &frags, const KnownMap &known, const ContextMap &context,
                            const ComplexityMap &cplx)
{
  VcfInput vi;
  vi.nt = tumor.nt;
  vi.names = tumor.names;
  vi.lens = tumor.lens;
  vi.nib_dir = o.nib_dir;
  vi.all = o.all;
  vi.jsup = &t.jsup;
  vi.with_normal = o.with_normal();
  vi.nsup = t.nsup.data();
  vi.n_nsup = t.nsup.size();
  vi.gsup = o.genotype ? &t.gsup : nullptr;
  vi.gsup_normal = o.genotype && o.with_normal() ? &t.gsup_normal : nullptr;
  vi.usup = o.dedup ? &t.usup : nullptr;
  vi.cons = o.consensus ? &cons : nullptr;
  vi.hom = o.homology ? &hom : nullptr;
  vi.sim = o.similar ? &sim : nullptr;
  vi.cov = o.coverage ? &cov : nullptr;
  vi.frame = o.frame ? &frame : nullptr;
  vi.link = o.link ? &link : nullptr;
  vi.partners = o.partners ? &partners : nullptr;
  vi.frags = o.fragsize ? &frags : nullptr;
  vi.known = o.known() ? &known : nullptr;
  vi.context = o.context ? &context : nullptr;
  vi.cplx = o.complexity ? &cplx : nullptr;
  auto write = [&](const string &path, const vector<OutRow> &calls) {
    if (write_vcf(path, calls, vi)) return;
    std::cerr << "Error: cannot write " << path << ": the evidence tables do not cover every call" << std::endl;
    exit(1);
  };
  write(o.out_file + "_fusion.vcf", rows);
  if (!o.clip) return;
  vi.gsup = vi.gsup_normal = nullptr;  // rescued calls are not genotyped
  vi.usup = nullptr;                   // ... and their files stay as they are with -dedup
  vi.cons = nullptr;                   // ... and with -consensus
  vi.hom = nullptr;                    // ... and with -homology
  vi.sim = nullptr;                    // ... and with -similar
  vi.cov = nullptr;                    // ... and with -coverage
  vi.frame = nullptr;                  // ... and with -frame
  vi.link = nullptr;                   // ... and with -link
  vi.partners = nullptr;               // ... and with -partners
  vi.frags = nullptr;                  // ... and with -fragsize
  vi.known = nullptr;                  // ... and with -known
  vi.context = nullptr;                // ... and with -context
  vi.cplx = nullptr;                   // ... and with -complexity
  vi.rescued = &rescued.calls;
  write(o.out_file + "_fusion_rescued.vcf", rescued.rows);
}

// -evidence: <prefix>_evidence.txt / .bam, and with -clip <prefix>_evidence_rescued.txt / .bam
static void write_evidence_files(const Options &o, const Sample &tumor, const CallTables &t, const vector<OutRow> &rows, const Rescued &rescued)
{
  EvidenceInput ei;
  ei.nt = tumor.nt;
  ei.names = tumor.names;
  ei.all = o.all;
  ei.rows = &t.ev_rows;
  ei.call_off = &t.ev_off;
  ei.first = o.dedup ? &t.ufirst : nullptr;
  string why;
  if (!write_evidence(o.out_file, o.inp_file, rows, ei, why))
  {
    std::cerr << "Error: cannot write " << o.out_file << "_evidence.txt / _evidence.bam: " << why << std::endl;
    exit(1);
  }
  if (o.clip && !write_evidence_rescued(o.out_file, o.inp_file, rescued.rows, rescued.calls, ei, rescued.reads, rescued.read_off, why))
  {
    std::cerr << "Error: cannot write " << o.out_file << "_evidence_rescued.txt / _evidence_rescued.bam: " << why << std::endl;
    exit(1);
  }
}

// ---- -junctions: junction calls from the split reads alone --------------------------------------------------------------------------
// One call of bk_split_junctions on the sample's own tuples (-q is its mapq_min; -x applies by itself, because tuples come from kept
// records); the calls that no voted row claims get the depth at their two positions (one call of bk_base_depth) and the gene on either
// side.  It runs behind every other stage and reads what they left: no other file changes.
static void split_junction_calls(const Options &o, const Sample &tumor, const vector<Txpt> &txpts)
{
  const struct bk_split_junction *calls = nullptr;
  uint64_t n = 0, counts[6] = {};
  int rc = bk_split_junctions(tumor.ctx, o.qual, (uint32_t) o.jtol, (uint32_t) o.jsupport, &calls, &n);
  if (rc == BK_OK) rc = bk_split_junction_counts(tumor.ctx, counts);
  if (rc != BK_OK) die(tumor, rc);
  vector<SjRow> rows;
  vector<int32_t> q_tid;
  vector<uint32_t> q_pos;
  for (uint64_t i = 0; i < n; ++i)
  {
    if (calls[i].call >= 0) continue;
    SjRow r;
    r.j = calls[i];
    r.index = i;
    r.depth[0] = r.depth[1] = 0;
    rows.push_back(r);
    q_tid.insert(q_tid.end(), {calls[i].tid1, calls[i].tid2});
    q_pos.insert(q_pos.end(), {calls[i].pos1, calls[i].pos2});
  }
  const uint32_t *depth = nullptr;
  if (!rows.empty() && (rc = bk_base_depth(tumor.ctx, q_tid.data(), q_pos.data(), q_tid.size(), &depth)) != BK_OK) die(tumor, rc);
  for (size_t k = 0; k < rows.size(); ++k)
  {
    SjRow &r = rows[k];
    const uint32_t pos[2] = {r.j.pos1, r.j.pos2};
    const int32_t tid[2] = {r.j.tid1, r.j.tid2};
    for (int s = 0; s < 2; ++s)
    {
      string exon, strand;
      r.depth[s] = depth[2 * k + s];
      r.chr[s] = tumor.names[tid[s]];
      annotate_side(txpts, r.chr[s], (long) pos[s], r.gene[s], exon, strand);
    }
  }
  write_junction_files(o, rows);
  std::cout << "junctions: " << counts[1] << " tuples eligible, " << counts[2] << " exact, " << n << " calls, " << n - rows.size() << " claimed by a voted call, " << rows.size()
            << " written" << std::endl;
}

// ---- -gaps: deletions and insertions from CIGAR gaps --------------------------------------------------------------------------------
// One call of bk_cigar_gaps on the sample's own table (-q is its mapq_min; -x applies by itself, because the table holds the kept records);
// every returned call gets the depth at its start and at its right end (one call of bk_base_depth) and the gene at either.  It runs behind
// every other stage and reads the table alone: no other file changes.
static void cigar_gap_calls(const Options &o, const Sample &tumor, const vector<Txpt> &txpts)
{
  const struct bk_cigar_gap *calls = nullptr;
  uint64_t n = 0, counts[8] = {};
  int rc = bk_cigar_gaps(tumor.ctx, o.qual, (uint32_t) o.mingap, (uint32_t) o.gapanchor, (uint32_t) o.gaptol, (uint32_t) o.gapsupport, &calls, &n);
  if (rc == BK_OK) rc = bk_cigar_gap_counts(tumor.ctx, counts);
  if (rc != BK_OK) die(tumor, rc);
  vector<GapRow> rows(n);
  vector<int32_t> q_tid;
  vector<uint32_t> q_pos;
  for (uint64_t i = 0; i < n; ++i)
  {
    rows[i].g = calls[i];
    q_tid.insert(q_tid.end(), {calls[i].tid, calls[i].tid});
    q_pos.insert(q_pos.end(), {calls[i].start, gap_end(calls[i])});
  }
  const uint32_t *depth = nullptr;
  if (n && (rc = bk_base_depth(tumor.ctx, q_tid.data(), q_pos.data(), q_tid.size(), &depth)) != BK_OK) die(tumor, rc);
  for (size_t k = 0; k < rows.size(); ++k)
  {
    GapRow &r = rows[k];
    r.chr = tumor.names[r.g.tid];
    for (int s = 0; s < 2; ++s)
    {
      string exon, strand;
      r.depth[s] = depth[2 * k + s];
      annotate_side(txpts, r.chr, (long) q_pos[2 * k + s], r.gene[s], exon, strand);
    }
  }
  write_gap_files(o, rows);
  std::cout << "gaps: " << counts[1] << " records eligible, " << counts[2] << " events, " << counts[3] << " beyond a contig's end, " << counts[4] << " exact, " << counts[6]
            << " calls, " << rows.size() << " written" << std::endl;
}

// ---- -panel: the sequences a junction sequence is searched in -----------------------------------------------------------------------------
// A FASTA: a `>` line names a sequence by its first word, bases are upper-cased, every letter other than A C G T becomes N, blank lines
// are skipped.  Sequence data before a header, a duplicate name and a sequence without bases end the run with the line's number.
struct SeqLibrary
{
  vector<string> names;
  vector<uint64_t> off{0};
  string bases;
};

static SeqLibrary read_panel_fasta(const string &path)
{
  SeqLibrary lib;
  std::ifstream in(path.c_str());
  std::set<string> seen;
  auto stop = [&](long line, const string &what) {
    std::cerr << "Error: panel file " << path << " line " << line << ": " << what << std::endl;
    exit(1);
  };
  string line;
  long no = 0, header_at = 0;
  auto close_sequence = [&]() {
    if (lib.names.empty()) return;
    if (lib.bases.size() == lib.off.back()) stop(header_at, "sequence " + lib.names.back() + " has no bases");
    lib.off.push_back(lib.bases.size());
  };
  while (std::getline(in, line))
  {
    ++no;
    const size_t a = line.find_first_not_of(" \t\r\n\v\f"), b = line.find_last_not_of(" \t\r\n\v\f");
    if (a == string::npos) continue;
    line = line.substr(a, b - a + 1);
    if (line[0] == '>')
    {
      close_sequence();
      const size_t w = line.find_first_not_of(" \t", 1);
      const string name = w == string::npos ? "" : line.substr(w, line.find_first_of(" \t", w) - w);
      if (name.empty()) stop(no, "a header without a name");
      if (!seen.insert(name).second) stop(no, "duplicate sequence name " + name);
      lib.names.push_back(name);
      header_at = no;
      continue;
    }
    if (lib.names.empty()) stop(no, "sequence data before the first header");
    for (const char ch : line)
    {
      const char u = (char) toupper((unsigned char) ch);
      lib.bases.push_back(u == 'A' || u == 'C' || u == 'G' || u == 'T' ? u : 'N');
    }
  }
  close_sequence();
  return lib;
}

// ---- -lociseq: the junction sequence of every written clip locus ------------------------------------------------------------------------
// Each written row is the site (tid, pos, 0, dir); bk_clip_reads lists the reads there, one pass over the file brings their alignments
// back with the bases, bk_clip_consensus piles them up with -q, -minclip, -conslen and the vote's own minimum depth.  As with
// -consensus the reads are chosen by name and bk_clip_consensus has no SA condition, so Seq_N can differ from TopReads.  With -panel one
// call of bk_sequence_match takes the consensus as it lies, reversed = dir.
static void clip_locus_sequences(const Options &o, const Sample &tumor, const vector<ClipLocusRow> &rows, const struct bk_clip_locus *all, uint64_t n, const SeqLibrary &lib)
{
  vector<LocusSeq> seqs(rows.size());
  uint64_t with_seq = 0, with_tail = 0, with_hit = 0, pairs = 0;
  if (!rows.empty())
  {
    vector<struct bk_clip_site> sites;
    for (const ClipLocusRow &r : rows) sites.push_back(bk_clip_site{r.l.tid, r.l.pos, 0u, r.l.dir});
    const uint32_t *counts = nullptr;
    const struct bk_clip_read *cr = nullptr;
    const uint64_t *off = nullptr;
    int rc = bk_clip_reads(tumor.ctx, sites.data(), sites.size(), o.qual, (int) o.min_clip, &counts, &cr, &off);
    if (rc != BK_OK) die(tumor, rc);
    std::set<std::pair<uint64_t, uint32_t>> seen;
    vector<bk_read_key> keys;
    for (uint64_t i = 0; i < off[sites.size()]; ++i)
      if (seen.emplace(cr[i].qhash, cr[i].qcheck).second) keys.push_back(bk_read_key{cr[i].qhash, cr[i].qcheck, 0});
    bk_reads reads;
    char err[512] = "";
    if (bk_bam_reads(o.inp_file.c_str(), keys.data(), keys.size(), &reads, err, sizeof err) != BK_OK)
    {
      std::cerr << "Error: cannot read the clipped reads back from " << o.inp_file << ": " << err << std::endl;
      exit(1);
    }
    const struct bk_consensus *crow = nullptr;
    const uint8_t *cbases = nullptr;
    rc = bk_clip_consensus(tumor.ctx, &reads, sites.data(), sites.size(), o.qual, (int) o.min_clip, (uint32_t) o.conslen, CONSENSUS_MIN_DEPTH, &crow, &cbases, nullptr);
    bk_reads_free(&reads);
    if (rc != BK_OK) die(tumor, rc);
    for (size_t k = 0; k < rows.size(); ++k)
    {
      LocusSeq &x = seqs[k];
      const char *col = (const char *) cbases + k * (size_t) o.conslen;
      x.side.c = crow[k];
      x.side.seq.assign(col, x.side.c.len);
      if (x.side.c.len)
      {
        while (x.tail_len < x.side.c.len && col[x.tail_len] == col[0]) ++x.tail_len;
        x.tail = string(1, col[0]) + std::to_string(x.tail_len);
        ++with_seq;
        with_tail += x.tail_len >= 10;
      }
      if (sites[k].dir == 1u) std::reverse(x.side.seq.begin(), x.side.seq.end());
    }
    if (o.panel())
    {
      vector<struct bk_seq_probe> probes;
      for (size_t k = 0; k < rows.size(); ++k) probes.push_back(bk_seq_probe{crow[k].len, sites[k].dir});
      const bk_seq_panel panel{lib.names.size(), lib.off.data(), (const uint8_t *) lib.bases.data()};
      const struct bk_seq_hit *hits = nullptr;
      rc = bk_sequence_match(tumor.ctx, &panel, probes.data(), probes.size(), cbases, (uint32_t) o.conslen, (uint32_t) o.panelseed, &hits);
      if (rc != BK_OK) die(tumor, rc);
      std::map<uint64_t, size_t> row_of;  // by row of the returned table
      for (size_t k = 0; k < rows.size(); ++k)
      {
        seqs[k].hit = hits[k];
        with_hit += hits[k].found;
        row_of[rows[k].index] = k;
      }
      for (size_t k = 0; k < rows.size(); ++k)
      {
        const struct bk_clip_locus &l = rows[k].l;
        if (!(l.flags & 1u) || !row_of.count(l.mate)) continue;  // (a mate that is written: the Mate column names it)
        const size_t m = row_of[l.mate];
        const struct bk_seq_hit &own = seqs[k].hit, &other = seqs[m].hit;
        if (!own.found || !other.found || own.seq != other.seq || own.orient != other.orient || l.dir == rows[m].l.dir) continue;
        const struct bk_seq_hit &left = l.dir == BK_CLIP_LEFT ? own : other, &right = l.dir == BK_CLIP_LEFT ? other : own;
        const long long span = own.orient ? (long long) left.s_start + left.len - (long long) right.s_start : (long long) right.s_start + right.len - (long long) left.s_start;
        seqs[k].pair_span = std::to_string(span);
        pairs += l.dir == BK_CLIP_LEFT;
      }
    }
  }
  write_lociseq_file(o, rows, all, n, seqs, lib.names);
  std::cout << "lociseq: " << rows.size() << " loci, " << with_seq << " with a sequence, " << with_tail << " with a tail of 10 or more" << std::endl;
  if (o.panel())
    std::cout << "panel: " << lib.names.size() << " sequences, " << lib.bases.size() << " bases, " << with_hit << " loci with a hit, " << pairs << " pairs on one sequence" << std::endl;
}

// ---- -cliploci: soft-clip pile-ups over the whole table ---------------------------------------------------------------------------------
// One call of bk_clip_loci on the sample's own table with the run's voted rows as the claiming calls (-q is its mapq_min, -minclip its
// min_clip; -x applies by itself, because the table holds the kept records); the loci that no voted row claims get the depth at their
// position (one call of bk_base_depth) and the gene there.  It runs behind every other stage and reads what they left: no other file changes.
static void clip_locus_calls(const Options &o, const Sample &tumor, const vector<Txpt> &txpts, const SeqLibrary &lib)
{
  const struct bk_clip_locus *loci = nullptr;
  uint64_t n = 0, counts[8] = {};
  int rc = bk_clip_loci(tumor.ctx, tumor.ctx, o.qual, (int) o.min_clip, (uint32_t) o.locitol, (uint32_t) o.locipair, (uint32_t) o.locisupport, &loci, &n);
  if (rc == BK_OK) rc = bk_clip_locus_counts(tumor.ctx, counts);
  if (rc != BK_OK) die(tumor, rc);
  vector<ClipLocusRow> rows;
  vector<int32_t> q_tid;
  vector<uint32_t> q_pos;
  for (uint64_t i = 0; i < n; ++i)
  {
    if (loci[i].claim != 0xFFFFFFFFu) continue;
    ClipLocusRow r;
    r.l = loci[i];
    r.index = i;
    r.depth = 0;
    rows.push_back(r);
    q_tid.push_back(loci[i].tid);
    q_pos.push_back(loci[i].pos);
  }
  const uint32_t *depth = nullptr;
  if (!rows.empty() && (rc = bk_base_depth(tumor.ctx, q_tid.data(), q_pos.data(), q_tid.size(), &depth)) != BK_OK) die(tumor, rc);
  for (size_t k = 0; k < rows.size(); ++k)
  {
    ClipLocusRow &r = rows[k];
    string exon, strand;
    r.depth = depth[k];
    r.chr = tumor.names[r.l.tid];
    annotate_side(txpts, r.chr, (long) r.l.pos, r.gene, exon, strand);
  }
  write_cliploci_files(o, rows, loci, n);
  std::cout << "cliploci: " << counts[1] << " records eligible, " << counts[2] << " events, " << counts[3] << " beyond a contig's end, " << counts[4] << " exact, " << counts[5]
            << " loci, " << counts[6] << " with a mutual partner, " << n - rows.size() << " claimed by a voted call, " << rows.size() << " written" << std::endl;
  if (o.lociseq)
  {
    const vector<struct bk_clip_locus> table(loci, loci + n);  // (the library's rows are its own until the next call)
    clip_locus_sequences(o, tumor, rows, table.data(), n, lib);
  }
}

// write_enspan_params (:1170-1182); an option that changes what is called adds its line behind the reference's
static void write_params(const Options &o, double w)
{
  std::ofstream p((o.out_file + "_params.txt").c_str());
  p << "ENSPAN" << std::endl;
  p << "inp_file\t" << o.inp_file << std::endl;
  p << "out_file\t" << o.out_file << std::endl;
  p << "qual\t" << (long) o.qual << std::endl;
  p << "w\t" << w << std::endl;
  p << "build\t" << o.build << std::endl;
  if (o.exclude()) p << "exclude_file\t" << o.exclude_file << std::endl;
  if (o.with_normal()) p << "normal_file\t" << o.normal_file << std::endl;
  if (o.genotype) p << "genotype_anchor\t" << o.anchor << std::endl;
  if (o.vcf) p << "vcf\t1" << std::endl;
  if (o.evidence) p << "evidence\t1" << std::endl;
  if (o.clip) p << "clip_min_length\t" << o.min_clip << std::endl;
  if (o.clip) p << "clip_min_support\t" << o.clip_support << std::endl;
  if (o.dedup) p << "dedup\t1" << std::endl;
  if (o.consensus) p << "consensus_max_len\t" << o.conslen << std::endl;
  if (o.homology) p << "homology_max_shift\t" << o.homshift << std::endl;
  if (o.homology) p << "homology_max_ins\t" << o.homins << std::endl;
  if (o.similar) p << "similar_flank\t" << o.simflank << std::endl;
  if (o.coverage) p << "coverage_flank\t" << o.covflank << std::endl;
  if (o.frame) p << "frame" << std::endl;
  if (o.link) p << "link_max_dist\t" << o.linkdist << std::endl;
  if (o.partners) p << "partners" << std::endl;
  if (o.fragsize) p << "fragsize" << std::endl;
  if (o.known()) p << "known_file\t" << o.known_file << std::endl;
  if (o.known()) p << "known_slop\t" << o.knownslop << std::endl;
  if (o.bedpe) p << "bedpe" << std::endl;
  if (o.context) p << "context_flank\t" << o.ctxflank << std::endl;
  if (o.junctions) p << "junction_min_support\t" << o.jsupport << std::endl;
  if (o.junctions) p << "junction_tol\t" << o.jtol << std::endl;
  if (o.complexity) p << "complexity_flank\t" << o.cplxflank << std::endl;
  if (o.complexity) p << "complexity_max_period\t" << o.cplxperiod << std::endl;
  if (o.gaps) p << "gap_min_length\t" << o.mingap << std::endl;
  if (o.gaps) p << "gap_anchor\t" << o.gapanchor << std::endl;
  if (o.gaps) p << "gap_tol\t" << o.gaptol << std::endl;
  if (o.gaps) p << "gap_min_support\t" << o.gapsupport << std::endl;
  if (o.cliploci) p << "cliploci_tol\t" << o.locitol << std::endl;
  if (o.cliploci) p << "cliploci_pair\t" << o.locipair << std::endl;
  if (o.cliploci) p << "cliploci_min_support\t" << o.locisupport << std::endl;
  if (o.lociseq) p << "lociseq\t" << o.conslen << std::endl;
  if (o.panel()) p << "panel_file\t" << o.panel_file << std::endl;
  if (o.panel()) p << "panel_seed\t" << o.panelseed << std::endl;
}

// BreakID.cc:175-191.  scan_pairs_count and after_cluster_count are never updated by the reference (always 0);
// removed_isolated_pair_count sums the groups that keep >= 2 pairs (:128); root_cluster_num is what the clustering of the LAST such
// group returned (:131-136; the reference leaves it uninitialised when no group qualifies - 0 here)
static void write_performance(const Options &o, const Sample &tumor, const Run &run, clock_t start, clock_t end)
{
  const bk_group_stat *gs = nullptr;
  uint32_t ngs = 0;
  const int rc = o.multi() ? bk_multi_stats(tumor.ctx, nullptr, nullptr, &gs, &ngs) : bk_group_stats(tumor.ctx, &gs, &ngs);  // (multi: summed over the ranks)
  if (rc != BK_OK) die(tumor, rc);
  int removed_isolated_pair_count = 0, root_cluster_num = 0;
  for (uint32_t g = 0; g < ngs; ++g)
    if (gs[g].n_isolated_removed >= 2)
    {
      removed_isolated_pair_count += (int) gs[g].n_isolated_removed;
      root_cluster_num = o.fast ? (gs[g].cluster_id_end ? (int) gs[g].cluster_id_end - 1 : 0) : (int) (gs[g].cluster_id_end + gs[g].n_isolated_removed - gs[g].n_clustered);
    }
  auto seconds = [](clock_t from, clock_t to) { return (to - from) / double(CLOCKS_PER_SEC); };
  std::ofstream p((o.out_file + "_performance.txt").c_str());
  p << "scan_dist\tdiscordant pairs\tremove isolated\tafter_cluster\troot cluster\tscanning time\tcluster time\tfind breakpoint time\ttotal time" << std::endl;
  p << run.w << "\t" << 0 << "\t" << removed_isolated_pair_count << "\t" << 0 << "\t" << root_cluster_num << "\t" << seconds(run.scan_start, run.scan_end) << "\t"
    << seconds(run.cluster_start, run.cluster_end) << "\t" << seconds(run.bp_start, run.bp_end) << "\t" << seconds(start, end) << std::endl;
}

int main(int argc, char *argv[])
{
  const clock_t start = clock();
  const Options o = parse_options(argc, argv);
  std::cout << "start to stats the insert size...\n";
  Sample tumor, normal;
  tumor.path = o.inp_file;
  normal.path = o.normal_file;
  normal.is_normal = true;
  if (!opens(o.inp_file))
  {
    std::cerr << "Error: can not open bam-file: " << o.inp_file << std::endl;
    exit(1);
  }
  Exclusion exclusion;
  if (o.exclude()) read_exclusion(o, exclusion);
  decode_tumor(o, tumor, exclusion);
  KnownPanel panel;  // (read against the file's reference list before the stages run: a line that ends the run does so early)
  if (o.known()) panel = read_known_bedpe(o.known_file, tumor.names, tumor.lens, tumor.nt);
  SeqLibrary library;  // (read before the stages run: a line that ends the run does so early)
  if (o.panel()) library = read_panel_fasta(o.panel_file);
  if (!opens(o.nib_dir + "/ref_names.txt"))
  {
    std::cerr << "Error: cannot open reference names file.\n";
    exit(1);
  }
  Run run = o.multi() ? run_sharded(o, tumor, exclusion) : run_stages(o, tumor, exclusion);
  if (o.with_normal()) run_normal(o, normal, tumor, exclusion, run.w);

  CallTables tables;
  fetch_call_tables(o, tumor, normal, run.w, tables);
  if (o.multi())
  {
    run.n_valid = 0;
    for (uint64_t i = 0; i < tables.cnt; ++i) run.n_valid += (tables.cl[i].flags & 2u) != 0;
  }
  std::cout << "valid cluster count: " << run.n_valid << std::endl;

  const vector<Txpt> txpts = read_transcripts(tables, run.n_clustered);
  const vector<OutRow> rows = voted_rows(o, tumor, tables, txpts);
  Rescued rescued;
  if (o.clip) rescued.rows = rescued_rows(o, tumor, normal, tables, txpts);
  describe_rescued(o, tumor, normal, tables, rescued);

  JunctionConsensus consensus;
  HomologyMap homology;
  if (o.consensus) junction_consensus(o, tumor, tables, rows, consensus);
  if (o.homology) homology = junction_homology(o, tumor, consensus);
  SimilarMap similar;
  if (o.similar) similar = locus_similar(o, tumor, rows);
  CoverageMap coverage;
  if (o.coverage) coverage = call_coverage(o, tumor, normal, tables, rows);
  FrameMap frames;
  if (o.frame) frames = fusion_frames(o, tumor, tables, rows, txpts);
  LinkMap links;
  if (o.link) links = link_calls(o, tumor, tables, rows);
  PartnerMap partners;
  if (o.partners) partners = locus_partners(o, tumor, normal, rows, run.w);
  FragsizeMap frags;
  if (o.fragsize) frags = fragment_sizes(o, tumor, tables, rows, run);
  KnownMap known;
  if (o.known()) known = known_calls(o, tumor, tables, rows, panel);
  ContextMap context;
  if (o.context) context = call_context(o, tumor, normal, tables, rows);
  ComplexityMap complexity;
  if (o.complexity) complexity = site_complexity(o, tumor, rows);

  if (o.clip) write_rescued_tables(o, rescued, tables);
  write_fusion_tables(o, rows, fusion_twins(o, tables, consensus.sides, homology, similar, coverage, frames, links, partners, frags, known, context, complexity));
  if (o.vcf) write_vcf_files(o, tumor, tables, rows, rescued, consensus.sides, homology, similar, coverage, frames, links, partners, frags, known, context, complexity);
  if (o.evidence) write_evidence_files(o, tumor, tables, rows, rescued);
  if (o.bedpe && !write_bedpe_files(o, rows, tables.jsup))
  {
    std::cerr << "Error: cannot write " << o.out_file << "_fusion.bedpe: the evidence tables do not cover every call" << std::endl;
    exit(1);
  }
  if (o.junctions) split_junction_calls(o, tumor, txpts);
  if (o.gaps) cigar_gap_calls(o, tumor, txpts);
  if (o.cliploci) clip_locus_calls(o, tumor, txpts, library);
  write_params(o, run.w);
  const clock_t end = clock();
  std::cout << "the fusion process of file " << o.inp_file << "  costs time: " << (end - start) / double(CLOCKS_PER_SEC) << " seconds" << std::endl;
  write_performance(o, tumor, run, start, end);

  if (o.multi())
    bk_multi_free(tumor.ctx);
  else
    bk_free(tumor.ctx);
  if (normal.ctx) bk_free(normal.ctx);
  for (Sample *s : {&tumor, &normal}) s->release_table();
  return 0;
}
