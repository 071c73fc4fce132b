// BreakID command line: what it writes.  The fusion tables with their twins (write_enspan_out, BreakID.cc:1184-1263 of the reference,
// and one twin per option that adds columns), the rescued tables, the VCF breakends and the evidence listings.  Included by
// breakid_main.cc alone, behind breakid_options.h.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "breakid_options.h"

using std::string;
using std::vector;

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

// The per-call rows copied from the library (they are the library's only until its next call), each by row of BK_STAGE_CLUSTERS.  An
// option that adds a per-call output adds its rows here; fetch_call_tables() in breakid_main.cc fills them.
struct CallTables
{
  const bk_cluster *cl = nullptr;  // BK_STAGE_CLUSTERS itself (the context's, until it is freed)
  uint64_t cnt = 0;
  vector<struct bk_normal_support> nsup;             // -normal
  vector<struct bk_ref_support> gsup, gsup_normal;   // -genotype: counted on the sample's records, on the normal's
  vector<struct bk_junction> jsup;                   // -vcf, -clip, -consensus
  vector<struct bk_clip_support> csup, csup_normal;  // -clip: counted on the sample's records, on the normal's
  vector<struct bk_evidence> ev_rows;                // -evidence, -consensus: the rows of call i are ev_off[i] .. ev_off[i + 1]
  vector<uint64_t> ev_off;
  vector<struct bk_unique_support> usup;             // -dedup, and per evidence row the first row of its fragment
  vector<uint64_t> ufirst;
};

// A row of a fusion table: the 15 columns of the reference, then what the table's option adds
static void write_row(std::ostream &o, const OutRow &r, const string &tail)
{
  o << fusion_type(r.c.type_mask) << "\t";
  o << r.p1_chr << ":" << r.c.p1_exact << "\t";
  o << r.p2_chr << ":" << r.c.p2_exact << "\t";
  o << r.g1 << "\t" << r.s1 << ":" << r.e1 << "\t";
  o << r.g2 << "\t" << r.s2 << ":" << r.e2 << "\t";
  o << (long) r.c.n_drp << "\t" << (long) r.c.n_sr << "\t";
  o << (double) r.c.depth1 << "\t" << (double) r.c.depth2 << "\t";
  o << r.af1 << "\t" << r.af2 << "\t";
  o << r.rpt1 << "\t" << r.rpt2 << tail << "\n";
}

static const char *HEADER =
    "Fusion_Type\tBreakPoint1\tBreakPoint2\tGene1\tBreakPoint_Info_Pair1\tGene2\tBreakPoint_Info_Pair2\tN_DRP\tN_SR\t"
    "BreakPoint1_Depth\tBreakPoint2_Depth\tBreakPoint1_AF\tBreakPoint2_AF\tBP1_Neighbour_Seq\tBP2_Neighbour_Seq";

// -normal: the matched normal's four counts
static const char *NORMAL_COLUMNS = "\tNormal_DRP\tNormal_SR\tNormal_Depth1\tNormal_Depth2";
static string normal_columns(const struct bk_normal_support &ns)
{
  std::ostringstream o;
  o << "\t" << ns.n_drp << "\t" << ns.n_sr << "\t" << ns.depth1 << "\t" << ns.depth2;
  return o.str();
}

// the eight genotype columns of one sample: a call is genotyped on its junction reads (alt = n_sr against the mean of the two sides'
// reference reads, rounded up); the pair counts stand beside it (include/breakid_hip.h: bk_genotype_call)
static string genotype_columns(const struct bk_ref_support &rs, uint32_t n_drp, uint32_t n_sr)
{
  uint8_t gt = 255, gq = 0, gtp = 255, gqp = 0;
  float vaf = 0, vaf_pairs = 0;
  bk_genotype_call(n_sr, (uint32_t) (((uint64_t) rs.ref_reads1 + rs.ref_reads2 + 1) / 2), &gt, &gq, &vaf);
  bk_genotype_call(n_drp, (uint32_t) (((uint64_t) rs.ref_pairs1 + rs.ref_pairs2 + 1) / 2), &gtp, &gqp, &vaf_pairs);
  std::ostringstream o;
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
  return o.str();
}

// -clip: the eight clip columns of one call (the directions d_s are those of its bk_junction row), and with -normal the two of the normal
static string clip_columns(const struct bk_junction &j, const struct bk_clip_support &s, const struct bk_clip_support *normal)
{
  uint8_t d[2] = {0, 1}, source = 0;
  bk_junction_sides(&j, &d[0], &d[1], &source);
  std::ostringstream o;
  o << "\t" << s.at[0][d[0]] << "\t" << s.at[1][d[1]] << "\t" << s.peak_pos[0][d[0]] << "\t" << s.peak_n[0][d[0]] << "\t" << s.peak_pos[1][d[1]] << "\t" << s.peak_n[1][d[1]]
    << "\t" << s.events[0][d[0]] << "\t" << s.events[1][d[1]];
  if (normal) o << "\t" << normal->at[0][d[0]] << "\t" << normal->at[1][d[1]];
  return o.str();
}

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
// -similar: the twin files' columns (bk_locus_similarity of the reference around the two breakpoints of the call)
static const char *SIMILAR_COLUMNS = "\tSim_Score\tSim_Len\tSim_Mism\tSim_Run\tSim_Strand\tSim_Pos1\tSim_Pos2";

// One written call: its bk_locus_sim row (on: both contigs have a nib file, so the pair was submitted) and the lowest coordinate of
// the shared stretch on either contig
struct SimilarCall
{
  bool on = false;
  struct bk_locus_sim s = {0, 0, 0, 0, 0, 0, 0, 0};
  long pos1 = 0, pos2 = 0;
  string fields() const
  {
    if (!on) return "\t.\t.\t.\t.\t.\t.\t.";
    std::ostringstream o;
    o << "\t" << s.score << "\t" << s.len << "\t" << s.mism << "\t" << s.run;
    if (s.found)
      o << "\t" << (s.orient ? "-" : "+") << "\t" << pos1 << "\t" << pos2;
    else
      o << "\t.\t.\t.";
    return o.str();
  }
};
// -coverage: the twin files' columns (bk_window_coverage of the windows bk_call_windows gives the call, and of its contigs); with
// -normal the same eight once more, from the same windows on the normal's records
static const char *COVERAGE_NAMES[8] = {"Cov_L1", "Cov_R1", "Cov_L2", "Cov_R2", "Cov_Span", "Cov_SpanRatio", "Cov_Contig1", "Cov_Contig2"};
static string coverage_columns(const char *prefix)
{
  string s;
  for (const char *name : COVERAGE_NAMES) s += string("\t") + prefix + name;
  return s;
}

// One written call: its seven windows (the five of bk_call_windows, then the whole contig of either side), the cut of either side, and
// what the sample's records, and the normal's, have inside the windows
struct CoverageCall
{
  struct bk_cov_window w[7];
  long long cut[2] = {0, 0};
  struct bk_window_cov tumor[7], normal[7];
  bool empty(int k) const { return w[k].end <= w[k].beg; }
  double mean(const struct bk_window_cov *cov, int k) const { return (double) cov[k].bases / (double) (w[k].end - w[k].beg); }
  static string fixed(const char *format, double v)
  {
    char buf[64];
    snprintf(buf, sizeof buf, format, v);
    return buf;
  }
  string mean_text(const struct bk_window_cov *cov, int k) const { return empty(k) ? "." : fixed("%.2f", mean(cov, k)); }
  // the span's mean over the mean of the two outer flanks: the left window of the lower cut and the right window of the higher one
  string ratio_text(const struct bk_window_cov *cov) const
  {
    const int lo = cut[0] <= cut[1] ? 0 : 1, outer_l = 2 * lo, outer_r = 2 * (1 - lo) + 1;
    if (empty(4) || empty(outer_l) || empty(outer_r)) return ".";
    const double flanks = mean(cov, outer_l) + mean(cov, outer_r);
    if (flanks == 0.0) return ".";
    return fixed("%.3f", mean(cov, 4) / (flanks / 2.0));
  }
  string fields(const struct bk_window_cov *cov) const
  {
    string s;
    for (int k = 0; k < 5; ++k) s += "\t" + mean_text(cov, k);
    s += "\t" + ratio_text(cov);
    for (int k = 5; k < 7; ++k) s += "\t" + mean_text(cov, k);
    return s;
  }
};
// -frame: the twin files' columns (bk_fusion_frame on the call's two sides, against every transcript of the run's refGene)
static const char *FRAME_COLUMNS =
    "\tFr_Class\tFr_Order\tFr_Gene1\tFr_Tx1\tFr_Loc1\tFr_Exon1\tFr_Cod1\tFr_Phase1\tFr_Gene2\tFr_Tx2\tFr_Loc2\tFr_Exon2\tFr_Cod2\tFr_Phase2\tFr_Pairs\tFr_Compatible\tFr_InFrame";
static const char *FRAME_CLASS_NAMES[6] = {"none", "antisense", "truncating", "promoter", "outframe", "inframe"};  // BK_FRAME_*
static const char *FRAME_LOC_NAMES[6] = {".", "noncoding", "5UTR", "CDS", "intron", "3UTR"};                       // BK_LOC_*

// One written call: its row, and the gene and the transcript of either side of the reported pair ("" where the side has none)
struct FrameCall
{
  struct bk_frame_call f;
  string gene[2], tx[2];
  const char *cls() const { return FRAME_CLASS_NAMES[f.cls <= BK_FRAME_INFRAME ? f.cls : 0]; }
  bool phased() const { return f.cls == BK_FRAME_INFRAME || f.cls == BK_FRAME_OUTFRAME; }
  string fields() const
  {
    std::ostringstream o;
    o << "\t" << cls() << "\t" << (f.order == 1 ? "5-3" : f.order == 2 ? "3-5" : ".");
    for (int s = 0; s < 2; ++s)
    {
      if (f.tx[s] < 0)
      {
        o << "\t.\t.\t.\t.\t.\t.";
        continue;
      }
      o << "\t" << gene[s] << "\t" << tx[s] << "\t" << FRAME_LOC_NAMES[f.loc[s] <= BK_LOC_3UTR ? f.loc[s] : 0] << "\t" << f.exon[s] << "\t" << f.cod[s] << "\t";
      if (phased())
        o << f.cod[s] % 3u;
      else
        o << ".";
    }
    o << "\t" << (unsigned long long) f.n_tx[0] * f.n_tx[1] << "\t" << f.n_compatible << "\t" << f.n_inframe;
    return o.str();
  }
  // what both breakends of the call end their INFO with
  string info() const
  {
    string s;
    if (f.cls != BK_FRAME_NONE) s += string(";FRCLASS=") + cls();
    if (f.order) s += ";FR5P=" + gene[f.order == 1 ? 0 : 1] + ";FR3P=" + gene[f.order == 1 ? 1 : 0];
    return s;
  }
};
// -link: the twin files' columns (bk_link_calls over every voted call; ids are rows of BK_STAGE_CLUSTERS, as bk<row> is)
static const char *LINK_COLUMNS = "\tLk_Event\tLk_Size\tLk_Dup\tLk_Recip\tLk_Adj\tLk_DupOf\tLk_Mate\tLk_MateSide\tLk_Off1\tLk_Off2";

// One voted call: its row, and the BK_STAGE_CLUSTERS rows behind the site indices it names (dup_row / mate_row only where there is one)
struct LinkCall
{
  struct bk_call_link l;
  uint64_t event_row = 0, dup_row = 0, mate_row = 0;
  string fields() const
  {
    std::ostringstream o;
    o << "\tev" << event_row << "\t" << l.event_size << "\t" << l.n_dup << "\t" << l.n_recip << "\t" << l.n_adj << "\t";
    if (l.dup_of >= 0)
      o << "bk" << dup_row;
    else
      o << ".";
    if (l.mate >= 0)
      o << "\tbk" << mate_row << "\t" << (l.mate_crossed ? "crossed" : "straight") << "\t" << l.off[0] << "\t" << l.off[1];
    else
      o << "\t.\t.\t.\t.";
    return o.str();
  }
  // what breakend `side` (0 or 1) of the call ends its INFO with; PARID names the mate's paired breakend, and only one the file holds
  string info(int side, bool mate_in_file) const
  {
    string s;
    if (l.event_size > 1) s += ";EVENT=ev" + std::to_string(event_row);
    if (l.mate >= 0 && mate_in_file) s += ";PARID=bk" + std::to_string(mate_row) + "_" + std::to_string((l.mate_crossed ? 1 - side : side) + 1);
    return s;
  }
};
// -partners: the twin files' columns (bk_locus_partners on the two windows of the call, bk_call_partner_sites)
static const char *PARTNERS_NAMES[11] = {"Pt_Ends1", "Pt_Partner1", "Pt_Loci1", "Pt_Top1", "Pt_TopN1", "Pt_Ends2", "Pt_Partner2", "Pt_Loci2", "Pt_Top2", "Pt_TopN2", "Pt_Frac"};
static string partners_columns(const string &prefix)
{
  string s;
  for (const char *name : PARTNERS_NAMES) s += string("\t") + prefix + name;
  return s;
}

// One written call: the rows of its two sides on the sample's pairs and on the normal's, and the contig names of their top loci
struct PartnerCall
{
  struct bk_locus_partners tumor[2], normal[2];
  string top_chr[2], normal_top_chr[2];  // "*" for tid -1
  static string top_text(const struct bk_locus_partners &p, const string &chr)
  {
    if (!p.top_n) return ".";
    return chr + ":" + std::to_string(p.top_beg) + "-" + std::to_string(p.top_end);
  }
  static string fields(const struct bk_locus_partners *p, const string *chr)
  {
    std::ostringstream o;
    for (int s = 0; s < 2; ++s) o << "\t" << p[s].ends << "\t" << p[s].to_partner << "\t" << p[s].loci << "\t" << top_text(p[s], chr[s]) << "\t" << p[s].top_n;
    const uint64_t ends = (uint64_t) p[0].ends + p[1].ends, to_partner = (uint64_t) p[0].to_partner + p[1].to_partner;
    char frac[64] = ".";
    if (ends) snprintf(frac, sizeof frac, "%.3f", (double) to_partner / (double) ends);
    o << "\t" << frac;
    return o.str();
  }
  // what breakend `side` (0 or 1) of the call ends its INFO with
  string info(int side) const
  {
    return ";PTN=" + std::to_string(tumor[side].ends) + ";PTP=" + std::to_string(tumor[side].to_partner) + ";PTL=" + std::to_string(tumor[side].loci);
  }
};
// -fragsize: the twin files' columns (bk_fragment_sizes on the call's voted positions, against the library's mean and sd)
static const char *FRAGSIZE_COLUMNS = "\tFg_N\tFg_Off\tFg_Mean\tFg_Dev\tFg_Min\tFg_Max\tFg_Short\tFg_Long\tFg_Z";
struct FragsizeCall
{
  struct bk_frag_sizes f;
  double mean = 0, sd = 0;  // of the library (bk_isize_stats)
  string mean_text() const { return f.n_used ? number("%.1f", (double) f.sum / (double) f.n_used) : "."; }
  string z_text() const { return f.n_used && sd != 0 ? number("%.2f", ((double) f.sum / (double) f.n_used - mean) / sd) : "."; }
  static string number(const char *format, double v)
  {
    char buf[64];
    snprintf(buf, sizeof buf, format, v);
    return buf;
  }
  string fields() const
  {
    std::ostringstream o;
    o << "\t" << f.n_used << "\t" << f.n_off << "\t" << mean_text() << "\t" << (f.n_used ? number("%.1f", (double) f.abs_dev / (double) f.n_used) : ".") << "\t"
      << (f.n_used ? std::to_string(f.min) : ".") << "\t" << (f.n_used ? std::to_string(f.max) : ".") << "\t" << f.n_short << "\t" << f.n_long << "\t" << z_text();
    return o.str();
  }
  // what both breakends of the call end their INFO with
  string info() const
  {
    string s = ";FGN=" + std::to_string(f.n_used);
    if (mean_text() != ".") s += ";FGMEAN=" + mean_text();
    if (z_text() != ".") s += ";FGZ=" + z_text();
    return s;
  }
};
// -known: the twin files' columns (bk_known_calls of the written calls against the panel)
static const char *KNOWN_COLUMNS = "\tKn_Hits\tKn_Names\tKn_Oriented\tKn_Opposed\tKn_Best\tKn_Score\tKn_BestDist\tKn_BestMap\tKn_Side1\tKn_Side2";
struct KnownCall
{
  struct bk_known_call k;
  string best_name = ".";  // the name text of the best hit's entry
  string fields() const
  {
    std::ostringstream o;
    o << "\t" << k.n_hits << "\t" << k.n_names << "\t" << k.n_oriented << "\t" << k.n_opposed << "\t" << (k.best >= 0 ? best_name : ".") << "\t";
    if (k.best >= 0 && k.best_score != BK_KNOWN_NO_SCORE)
      o << k.best_score;
    else
      o << ".";
    o << "\t" << k.best_dist << "\t" << (k.best < 0 ? "." : k.best_crossed ? "crossed" : "straight") << "\t" << k.n_side[0] << "\t" << k.n_side[1];
    return o.str();
  }
  // what both breakends of the call end their INFO with
  string info() const;
};
// -context: the twin files' columns (bk_window_context of the four flank windows bk_call_windows gives the call); with -normal the same
// eighteen once more, from the same windows on the normal's records
static const char *CONTEXT_NAMES[9] = {"Cx_Reads", "Cx_MeanMQ", "Cx_MQ0", "Cx_LowQ", "Cx_Clip", "Cx_Improper", "Cx_Orphan", "Cx_Dup", "Cx_SecSup"};
static string context_columns(const char *prefix)
{
  string s;
  for (int side = 1; side <= 2; ++side)
    for (const char *name : CONTEXT_NAMES) s += string("\t") + prefix + name + std::to_string(side);
  return s;
}

// One written call: per side the sum of its two flank windows' rows (membership is by start, so adjacent windows add exactly), on the
// sample's records and on the normal's.  Every ratio is a quotient of two doubles made from the integers; "." where reads == 0.
struct ContextCall
{
  struct bk_window_ctx tumor[2] = {}, normal[2] = {};
  static void add(struct bk_window_ctx &into, const struct bk_window_ctx &x)
  {
    into.mapq_sum += x.mapq_sum;
    into.reads += x.reads, into.mq0 += x.mq0, into.lowq += x.lowq, into.clipped += x.clipped;
    into.improper += x.improper, into.orphan += x.orphan, into.dup += x.dup, into.secsup += x.secsup;
  }
  static string ratio(const char *format, uint64_t part, uint32_t reads) { return reads ? CoverageCall::fixed(format, (double) part / (double) reads) : string("."); }
  static string mean_mq(const struct bk_window_ctx &x) { return ratio("%.1f", x.mapq_sum, x.reads); }
  static string mq0(const struct bk_window_ctx &x) { return ratio("%.3f", x.mq0, x.reads); }
  static string fields(const struct bk_window_ctx *ctx)
  {
    std::ostringstream o;
    for (int s = 0; s < 2; ++s)
    {
      const struct bk_window_ctx &x = ctx[s];
      o << "\t" << x.reads << "\t" << mean_mq(x) << "\t" << mq0(x) << "\t" << ratio("%.3f", x.lowq, x.reads) << "\t" << ratio("%.3f", x.clipped, x.reads) << "\t"
        << ratio("%.3f", x.improper, x.reads) << "\t" << x.orphan << "\t" << x.dup << "\t" << x.secsup;
    }
    return o.str();
  }
  // what the breakend of side s ends its INFO with
  string info(int s) const
  {
    string t = ";CXN=" + std::to_string(tumor[s].reads);
    if (tumor[s].reads) t += ";MQ0F=" + mq0(tumor[s]) + ";MEANMQ=" + mean_mq(tumor[s]);
    return t;
  }
};
// -complexity: the twin files' columns (bk_site_complexity of the reference around each of the two breakpoints of the call), side 1 and
// then side 2
static const char *COMPLEXITY_NAMES[12] = {"Lc_N", "Lc_GC", "Lc_Dust", "Lc_Tri", "Lc_Mask", "Lc_MaskRun", "Lc_BpUnit", "Lc_BpLen", "Lc_BpPos", "Lc_MaxUnit", "Lc_MaxLen", "Lc_MaxPos"};
static string complexity_columns()
{
  string s;
  for (int side = 1; side <= 2; ++side)
    for (const char *name : COMPLEXITY_NAMES) s += string("\t") + name + std::to_string(side);
  return s;
}

// One side of a written call: its bk_site_cplx row (on: the contig has a nib file, so the site was submitted), the repeat units as
// the reference spells them from each tract's start, and each tract's first 1-based position.  Every ratio is a quotient of two
// doubles made from the integers.
struct ComplexitySide
{
  bool on = false;
  struct bk_site_cplx c = {};
  string bp_unit, max_unit;
  long bp_pos = 0, max_pos = 0;
  string gc_text() const { return c.valid ? CoverageCall::fixed("%.3f", (double) c.gc / (double) c.valid) : string("."); }
  string dust_text() const { return c.tri_total >= 2 ? CoverageCall::fixed("%.2f", (double) c.tri_pairs / (double) (c.tri_total - 1)) : string("."); }
  string mask_text() const { return c.covered ? CoverageCall::fixed("%.3f", (double) c.masked / (double) c.covered) : string("."); }
  string fields() const
  {
    if (!on) return "\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.";
    std::ostringstream o;
    o << "\t" << c.valid << "\t" << gc_text() << "\t" << dust_text() << "\t" << c.tri_distinct << "\t" << mask_text() << "\t" << c.mask_run;
    if (c.bp_len)
      o << "\t" << bp_unit << "\t" << c.bp_len << "\t" << bp_pos;
    else
      o << "\t.\t0\t.";
    if (c.max_len)
      o << "\t" << max_unit << "\t" << c.max_len << "\t" << max_pos;
    else
      o << "\t.\t0\t.";
    return o.str();
  }
  // what the breakend of this side ends its INFO with
  string info() const
  {
    string t;
    if (!on) return t;
    if (dust_text() != ".") t += ";LCDUST=" + dust_text();
    if (gc_text() != ".") t += ";LCGC=" + gc_text();
    if (mask_text() != ".") t += ";LCMASK=" + mask_text();
    if (c.bp_len) t += ";LCSTR=" + bp_unit + "x" + std::to_string(c.bp_len);
    return t;
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

using ConsensusMap = std::map<uint64_t, std::pair<ConsensusSide, ConsensusSide>>;  // by row of BK_STAGE_CLUSTERS: the written calls
using HomologyMap = std::map<uint64_t, std::pair<HomologySide, HomologySide>>;
using SimilarMap = std::map<uint64_t, SimilarCall>;
using CoverageMap = std::map<uint64_t, CoverageCall>;
using FrameMap = std::map<uint64_t, FrameCall>;
using LinkMap = std::map<uint64_t, LinkCall>;  // every voted call, whichever files hold it
using PartnerMap = std::map<uint64_t, PartnerCall>;
using FragsizeMap = std::map<uint64_t, FragsizeCall>;
using KnownMap = std::map<uint64_t, KnownCall>;
using ContextMap = std::map<uint64_t, ContextCall>;
using ComplexityMap = std::map<uint64_t, std::pair<ComplexitySide, ComplexitySide>>;

// -clip: the rescued clusters in the order of _fusion_rescued.txt, calls[k] to rows[k]; with -evidence the clipped reads at the peaks
// of the written ones (bk_clip_reads: the rows of sites 2 * j and 2 * j + 1 belong to the j-th written row)
struct Rescued
{
  vector<OutRow> rows;
  vector<RescuedCall> calls;
  vector<struct bk_clip_read> reads;
  vector<uint64_t> read_off;
};

// ---- the fusion tables: <prefix>_fusion<suffix>.txt and, with -all, <prefix>_fusion_all<suffix>.txt -------------------------------
struct TwinFiles
{
  std::ofstream all, filt;
  TwinFiles(const Options &o, const string &suffix, const string &columns)
  {
    if (o.all) open(all, o.out_file + "_fusion_all" + suffix + ".txt", columns);
    open(filt, o.out_file + "_fusion" + suffix + ".txt", columns);
  }
  static void open(std::ofstream &f, const string &path, const string &columns)
  {
    f.open(path.c_str());
    f << HEADER << columns << "\n";
  }
  void put(const OutRow &r, bool all_ok, bool filt_ok, const string &tail)
  {
    if (filt_ok) write_row(filt, r, tail);
    if (all.is_open() && all_ok) write_row(all, r, tail);
  }
};

// One pair of tables: its suffix, the columns it adds, and per call what stands in them (false: the twin has no row for this call)
struct Twin
{
  string suffix, columns;
  std::function<bool(const OutRow &, string &)> tail;
};

// The twins of this run, the reference's own two files first.  An option that adds columns to the calls adds its entry here.
static vector<Twin> fusion_twins(const Options &o, const CallTables &t, const ConsensusMap &cons, const HomologyMap &hom, const SimilarMap &sim,
                                 const CoverageMap &cov, const FrameMap &frame, const LinkMap &link, const PartnerMap &partners,
                                 const FragsizeMap &frags, const KnownMap &known, const ContextMap &context, const ComplexityMap &cplx)
{
  const bool with_normal = o.with_normal();  // (a tumour without calls still gets header-only twins)
  vector<Twin> twins;
  twins.push_back({"", "", [](const OutRow &, string &) { return true; }});
  if (with_normal)
    twins.push_back({"_normal", NORMAL_COLUMNS, [&t](const OutRow &r, string &tail) {
                       if (r.idx >= t.nsup.size()) return false;
                       tail = normal_columns(t.nsup[r.idx]);
                       return true;
                     }});
  if (o.genotype)
    twins.push_back({"_genotype", string(GENOTYPE_COLUMNS) + (with_normal ? string(NORMAL_COLUMNS) + GENOTYPE_COLUMNS_NORMAL : ""), [&t, with_normal](const OutRow &r, string &tail) {
                       if (r.idx >= t.gsup.size() || (with_normal && (r.idx >= t.nsup.size() || r.idx >= t.gsup_normal.size()))) return false;
                       tail = genotype_columns(t.gsup[r.idx], r.c.n_drp, r.c.n_sr);
                       if (with_normal) tail += normal_columns(t.nsup[r.idx]) + genotype_columns(t.gsup_normal[r.idx], t.nsup[r.idx].n_drp, t.nsup[r.idx].n_sr);
                       return true;
                     }});
  if (o.clip)
    twins.push_back({"_clip", string(CLIP_COLUMNS) + (with_normal ? CLIP_COLUMNS_NORMAL : ""), [&t, with_normal](const OutRow &r, string &tail) {
                       tail = clip_columns(t.jsup[r.idx], t.csup[r.idx], with_normal ? &t.csup_normal[r.idx] : nullptr);
                       return true;
                     }});
  if (o.dedup)
    twins.push_back({"_dedup", DEDUP_COLUMNS, [&t](const OutRow &r, string &tail) {
                       if (r.idx >= t.usup.size()) return false;
                       const struct bk_unique_support &u = t.usup[r.idx];
                       std::ostringstream s;
                       s << "\t" << u.uniq_pairs << "\t" << u.uniq_splits << "\t" << u.top_pairs << "\t" << u.top_splits;
                       tail = s.str();
                       return true;
                     }});
  if (o.consensus)
    twins.push_back({"_consensus", CONSENSUS_COLUMNS, [&cons](const OutRow &r, string &tail) {
                       if (!cons.count(r.idx)) return false;
                       const std::pair<ConsensusSide, ConsensusSide> &both = cons.at(r.idx);
                       std::ostringstream s;
                       for (const ConsensusSide *x : {&both.first, &both.second})
                         s << "\t" << x->c.n_reads << "\t" << x->c.len << "\t" << x->agree() << "\t" << (x->seq.empty() ? "." : x->seq);
                       tail = s.str();
                       return true;
                     }});
  if (o.homology)
    twins.push_back({"_homology", HOMOLOGY_COLUMNS, [&hom](const OutRow &r, string &tail) {
                       if (!hom.count(r.idx)) return false;
                       tail = hom.at(r.idx).first.fields() + hom.at(r.idx).second.fields();
                       return true;
                     }});
  if (o.similar)
    twins.push_back({"_similar", SIMILAR_COLUMNS, [&sim](const OutRow &r, string &tail) {
                       if (!sim.count(r.idx)) return false;
                       tail = sim.at(r.idx).fields();
                       return true;
                     }});
  if (o.coverage)
    twins.push_back({"_coverage", coverage_columns("") + (with_normal ? coverage_columns("Normal_") : ""), [&cov, with_normal](const OutRow &r, string &tail) {
                       if (!cov.count(r.idx)) return false;
                       const CoverageCall &c = cov.at(r.idx);
                       tail = c.fields(c.tumor) + (with_normal ? c.fields(c.normal) : "");
                       return true;
                     }});
  if (o.frame)
    twins.push_back({"_frame", FRAME_COLUMNS, [&frame](const OutRow &r, string &tail) {
                       if (!frame.count(r.idx)) return false;
                       tail = frame.at(r.idx).fields();
                       return true;
                     }});
  if (o.link)
    twins.push_back({"_link", LINK_COLUMNS, [&link](const OutRow &r, string &tail) {
                       if (!link.count(r.idx)) return false;
                       tail = link.at(r.idx).fields();
                       return true;
                     }});
  if (o.partners)
    twins.push_back({"_partners", partners_columns("") + (with_normal ? partners_columns("Normal_") : ""), [&partners, with_normal](const OutRow &r, string &tail) {
                       if (!partners.count(r.idx)) return false;
                       const PartnerCall &c = partners.at(r.idx);
                       tail = PartnerCall::fields(c.tumor, c.top_chr) + (with_normal ? PartnerCall::fields(c.normal, c.normal_top_chr) : "");
                       return true;
                     }});
  if (o.fragsize)
    twins.push_back({"_fragsize", FRAGSIZE_COLUMNS, [&frags](const OutRow &r, string &tail) {
                       if (!frags.count(r.idx)) return false;
                       tail = frags.at(r.idx).fields();
                       return true;
                     }});
  if (o.known())
    twins.push_back({"_known", KNOWN_COLUMNS, [&known](const OutRow &r, string &tail) {
                       if (!known.count(r.idx)) return false;
                       tail = known.at(r.idx).fields();
                       return true;
                     }});
  if (o.context)
    twins.push_back({"_context", context_columns("") + (with_normal ? context_columns("Normal_") : ""), [&context, with_normal](const OutRow &r, string &tail) {
                       if (!context.count(r.idx)) return false;
                       const ContextCall &c = context.at(r.idx);
                       tail = ContextCall::fields(c.tumor) + (with_normal ? ContextCall::fields(c.normal) : "");
                       return true;
                     }});
  if (o.complexity)
    twins.push_back({"_complexity", complexity_columns(), [&cplx](const OutRow &r, string &tail) {
                       if (!cplx.count(r.idx)) return false;
                       tail = cplx.at(r.idx).first.fields() + cplx.at(r.idx).second.fields();
                       return true;
                     }});
  return twins;
}

// write_enspan_out (BreakID.cc:1184-1263) over every twin; the files are closed when this returns
static void write_fusion_tables(const Options &o, const vector<OutRow> &rows, const vector<Twin> &twins)
{
  vector<TwinFiles> files;
  files.reserve(twins.size());
  for (const Twin &t : twins) files.emplace_back(o, t.suffix, t.columns);
  string tail;
  for (const OutRow &r : rows)
  {
    const bool all_ok = call_all_ok(r), filt_ok = call_filt_ok(r);
    for (size_t k = 0; k < twins.size(); ++k)
    {
      tail.clear();
      if (twins[k].tail(r, tail)) files[k].put(r, all_ok, filt_ok, tail);
    }
  }
}

// -bedpe: <prefix>_fusion.bedpe and, with -all, <prefix>_fusion_all.bedpe: one line per row of the fusion file in its order, no header,
// in the format -known reads.  Each breakpoint is the one-base interval [P - 1, P); the name is the prefix's base name, so that files of
// several samples put together count samples by name; the score is N_DRP + N_SR; the strands are the sides of bk_junction_sides ('+'
// keeps the bases up to the breakpoint, '-' those from it on, '.' when no evidence gives a side).  False when a call has no junction row.
static bool write_bedpe_files(const Options &o, const vector<OutRow> &rows, const vector<struct bk_junction> &jsup)
{
  const size_t slash = o.out_file.find_last_of('/');
  const string sample = slash == string::npos ? o.out_file : o.out_file.substr(slash + 1);
  std::ofstream all, filt((o.out_file + "_fusion.bedpe").c_str());
  if (o.all) all.open((o.out_file + "_fusion_all.bedpe").c_str());
  for (const OutRow &r : rows)
  {
    const bool all_ok = call_all_ok(r), filt_ok = call_filt_ok(r);
    if (!all_ok) continue;
    if (r.idx >= jsup.size()) return false;
    uint8_t right[2] = {0, 1}, source = 0;
    bk_junction_sides(&jsup[r.idx], &right[0], &right[1], &source);
    const long long p1 = r.c.p1_exact, p2 = (uint32_t) r.c.p2_exact;
    std::ostringstream l;
    l << r.p1_chr << "\t" << p1 - 1 << "\t" << p1 << "\t" << r.p2_chr << "\t" << p2 - 1 << "\t" << p2 << "\t" << (sample.empty() ? "." : sample) << "\t"
      << (uint64_t) r.c.n_drp + r.c.n_sr << "\t" << (source ? (right[0] ? "-" : "+") : ".") << "\t" << (source ? (right[1] ? "-" : "+") : ".") << "\tbk" << r.idx << "\t"
      << fusion_type(r.c.type_mask) << "\t" << (long) r.c.n_drp << "\t" << (long) r.c.n_sr << "\n";
    if (filt_ok) filt << l.str();
    if (all.is_open()) all << l.str();
  }
  return true;
}

// -junctions: <prefix>_junctions.txt, the calls of bk_split_junctions that no voted row claims (a claimed one is a row of the fusion files
// already), in the order of the call's table, and with -bedpe <prefix>_junctions.bedpe in the layout of write_bedpe_files: score = Reads,
// strands from the sides, then sj<row>, Type, 0 and Reads.  Nothing is filtered beyond -jsupport.
struct SjRow
{
  struct bk_split_junction j;
  uint64_t index;  // in the table bk_split_junctions returned
  uint32_t depth[2];
  string chr[2], gene[2];
};
static const char *JUNCTION_COLUMNS =
    "Junction\tChr1\tPos1\tSide1\tChr2\tPos2\tSide2\tType\tSize\tReads\tTuples\tExact\tTopReads\tOwn1\tOwn2\tMeanMQ1\tMeanMQ2\tSpan1\tSpan2\tDepth1\tDepth2\tGene1\tGene2";
// translocation on different contigs; on one contig with pos1 < pos2 deletion for (L, R), duplication for (R, L), inversion for equal
// sides; "." for anything else
static const char *junction_type(const struct bk_split_junction &j)
{
  if (j.tid1 != j.tid2) return "translocation";
  if (j.pos1 >= j.pos2) return ".";
  return j.right1 == j.right2 ? "inversion" : j.right1 ? "duplication" : "deletion";
}
static void write_junction_files(const Options &o, const vector<SjRow> &rows)
{
  const size_t slash = o.out_file.find_last_of('/');
  const string sample = slash == string::npos ? o.out_file : o.out_file.substr(slash + 1);
  std::ofstream table((o.out_file + "_junctions.txt").c_str()), bedpe;
  if (o.bedpe) bedpe.open((o.out_file + "_junctions.bedpe").c_str());
  table << JUNCTION_COLUMNS << "\n";
  char mq[2][32];
  for (const SjRow &r : rows)
  {
    const struct bk_split_junction &j = r.j;
    for (int k = 0; k < 2; ++k)
      if (j.n_own[k])
        snprintf(mq[k], sizeof mq[k], "%.1f", (double) j.mapq_sum[k] / (double) j.n_own[k]);
      else
        snprintf(mq[k], sizeof mq[k], ".");
    table << "sj" << r.index << "\t" << r.chr[0] << "\t" << j.pos1 << "\t" << (j.right1 ? "R" : "L") << "\t" << r.chr[1] << "\t" << j.pos2 << "\t" << (j.right2 ? "R" : "L") << "\t"
          << junction_type(j) << "\t";
    if (j.tid1 == j.tid2)
      table << (long long) j.pos2 - (long long) j.pos1;
    else
      table << ".";
    table << "\t" << j.n_reads << "\t" << j.n_tuples << "\t" << j.n_exact << "\t" << j.top_reads << "\t" << j.n_own[0] << "\t" << j.n_own[1] << "\t" << mq[0] << "\t" << mq[1] << "\t"
          << j.lo1 << "-" << j.hi1 << "\t" << j.lo2 << "-" << j.hi2 << "\t" << r.depth[0] << "\t" << r.depth[1] << "\t" << r.gene[0] << "\t" << r.gene[1] << "\n";
    if (bedpe.is_open())
      bedpe << r.chr[0] << "\t" << (long long) j.pos1 - 1 << "\t" << j.pos1 << "\t" << r.chr[1] << "\t" << (long long) j.pos2 - 1 << "\t" << j.pos2 << "\t" << (sample.empty() ? "." : sample)
            << "\t" << j.n_reads << "\t" << (j.right1 ? "-" : "+") << "\t" << (j.right2 ? "-" : "+") << "\tsj" << r.index << "\t" << junction_type(j) << "\t0\t" << j.n_reads << "\n";
  }
}

// -gaps: <prefix>_gaps.txt, the calls of bk_cigar_gaps in the order of the call's table, and with -bedpe <prefix>_gaps.bedpe in the layout of
// write_junction_files: score = Reads, then gp<row>, Type, 0 and Reads.  Start is the last reference base in front of the gap, End the
// first one behind it (Start + Len + 1 for a deletion, Start + 1 for an insertion).  Nothing is filtered beyond -gapsupport.
struct GapRow
{
  struct bk_cigar_gap g;
  uint32_t depth[2];
  string chr, gene[2];
};
static const char *GAP_COLUMNS = "Gap\tChr\tStart\tEnd\tType\tLen\tReads\tRows\tExact\tTopReads\tFwd\tRev\tMeanMQ\tStartSpan\tLenSpan\tDepth1\tDepth2\tGene1\tGene2";
static uint32_t gap_end(const struct bk_cigar_gap &g) { return g.kind == BK_GAP_DEL ? g.start + g.len + 1 : g.start + 1; }
static void write_gap_files(const Options &o, const vector<GapRow> &rows)
{
  const size_t slash = o.out_file.find_last_of('/');
  const string sample = slash == string::npos ? o.out_file : o.out_file.substr(slash + 1);
  std::ofstream table((o.out_file + "_gaps.txt").c_str()), bedpe;
  if (o.bedpe) bedpe.open((o.out_file + "_gaps.bedpe").c_str());
  table << GAP_COLUMNS << "\n";
  char mq[32];
  for (size_t i = 0; i < rows.size(); ++i)
  {
    const GapRow &r = rows[i];
    const struct bk_cigar_gap &g = r.g;
    const char *type = g.kind == BK_GAP_DEL ? "deletion" : "insertion";
    const uint32_t end = gap_end(g);
    snprintf(mq, sizeof mq, "%.1f", (double) g.mapq_sum / (double) g.n_rows);  // (a call has at least one row)
    table << "gp" << i << "\t" << r.chr << "\t" << g.start << "\t" << end << "\t" << type << "\t" << g.len << "\t" << g.n_reads << "\t" << g.n_rows << "\t" << g.n_exact << "\t"
          << g.top_reads << "\t" << g.n_fwd << "\t" << g.n_rev << "\t" << mq << "\t" << g.lo_start << "-" << g.hi_start << "\t" << g.lo_len << "-" << g.hi_len << "\t" << r.depth[0]
          << "\t" << r.depth[1] << "\t" << r.gene[0] << "\t" << r.gene[1] << "\n";
    if (bedpe.is_open())
      bedpe << r.chr << "\t" << (long long) g.start - 1 << "\t" << g.start << "\t" << r.chr << "\t" << (long long) end - 1 << "\t" << end << "\t" << (sample.empty() ? "." : sample) << "\t"
            << g.n_reads << "\t+\t-\tgp" << i << "\t" << type << "\t0\t" << g.n_reads << "\n";
  }
}

// -cliploci: <prefix>_cliploci.txt, the loci of bk_clip_loci that no voted row claims (a claimed one is a row of the fusion files
// already), in the order of the call's table and named by their row in it; a mate that is not returned or is claimed prints as ".".
// With -bedpe <prefix>_cliploci.bedpe in the layout of write_gap_files: one line per mutual pair whose two rows are both written, in the
// order of its LEFT row; score = the reads of both rows, then cl<left row>, insertion_site, 0 and the reads again.  Nothing is filtered
// beyond -locisupport.
struct ClipLocusRow
{
  struct bk_clip_locus l;
  uint64_t index;  // in the table bk_clip_loci returned
  uint32_t depth;
  string chr, gene;
};
static const char *CLIPLOCI_COLUMNS =
    "Locus\tChr\tPos\tSide\tReads\tRows\tExact\tTopReads\tFwd\tRev\tMeanMQ\tSpan\tMaxClip\tMeanClip\tOrphans\tImproper\tMate\tMatePos\tMateReads\tMateOff\tMutual\tDepth\tGene";
// the line of row r in <prefix>_cliploci.txt without its newline (all: the returned table of n rows, in which a row's mate is looked up)
static string cliploci_line(const ClipLocusRow &r, const struct bk_clip_locus *all, uint64_t n)
{
  std::ostringstream table;
  char mq[32], mc[32];
  const struct bk_clip_locus &l = r.l;
  const bool facing = l.flags & 1u, mate_written = facing && l.mate < n && all[l.mate].claim == 0xFFFFFFFFu;
  snprintf(mq, sizeof mq, "%.1f", (double) l.mapq_sum / (double) l.n_rows);  // (a locus has at least one row)
  snprintf(mc, sizeof mc, "%.1f", (double) l.clip_sum / (double) l.n_rows);
  table << "cl" << r.index << "\t" << r.chr << "\t" << l.pos << "\t" << (l.dir ? "R" : "L") << "\t" << l.n_reads << "\t" << l.n_rows << "\t" << l.n_exact << "\t" << l.top_reads << "\t"
        << l.n_fwd << "\t" << l.n_rev << "\t" << mq << "\t" << l.lo_pos << "-" << l.hi_pos << "\t" << l.max_clip << "\t" << mc << "\t" << l.n_orphan << "\t" << l.n_improper << "\t";
  if (mate_written)
    table << "cl" << l.mate;
  else
    table << ".";
  if (facing)
    table << "\t" << l.mate_pos << "\t" << l.mate_reads << "\t" << l.mate_off;
  else
    table << "\t.\t.\t.";
  table << "\t" << ((l.flags & 2u) ? 1 : 0) << "\t" << r.depth << "\t" << r.gene;
  return table.str();
}

// all: the returned table (n rows), in which a row's mate is looked up
static void write_cliploci_files(const Options &o, const vector<ClipLocusRow> &rows, const struct bk_clip_locus *all, uint64_t n)
{
  const size_t slash = o.out_file.find_last_of('/');
  const string sample = slash == string::npos ? o.out_file : o.out_file.substr(slash + 1);
  std::ofstream table((o.out_file + "_cliploci.txt").c_str()), bedpe;
  if (o.bedpe) bedpe.open((o.out_file + "_cliploci.bedpe").c_str());
  table << CLIPLOCI_COLUMNS << "\n";
  for (const ClipLocusRow &r : rows)
  {
    const struct bk_clip_locus &l = r.l;
    const bool mate_written = (l.flags & 1u) && l.mate < n && all[l.mate].claim == 0xFFFFFFFFu;
    table << cliploci_line(r, all, n) << "\n";
    if (bedpe.is_open() && l.dir == BK_CLIP_LEFT && (l.flags & 2u) && mate_written)
    {
      const struct bk_clip_locus &m = all[l.mate];
      const uint64_t reads = (uint64_t) l.n_reads + m.n_reads;
      bedpe << r.chr << "\t" << (long long) l.pos - 1 << "\t" << l.pos << "\t" << r.chr << "\t" << (long long) m.pos - 1 << "\t" << m.pos << "\t" << (sample.empty() ? "." : sample) << "\t"
            << reads << "\t+\t-\tcl" << r.index << "\tinsertion_site\t0\t" << reads << "\n";
    }
  }
}

// -lociseq: <prefix>_cliploci_seq.txt, the rows of <prefix>_cliploci.txt in its order with the junction sequence of each behind them: the
// columns of -consensus for the one side a locus has, and the base of column 0 with the number of leading columns equal to it (the
// homopolymer next to the junction; "." without a column).  With -panel the hit of bk_sequence_match behind that: the panel sequence's
// name, the strand, the segment (Pn_QStart 1-based in Seq as printed, Pn_Start .. Pn_End 1-based and inclusive on the panel
// sequence), the seeds, the runner-up, and for a row whose Mate is written and lies on the same sequence and strand the panel bases
// from the LEFT row's first to the RIGHT row's last (+; mirrored for -): what the pair implies for the inserted length.
static const char *LOCISEQ_COLUMNS = "\tSeq_N\tSeq_Len\tSeq_Agree\tSeq\tSeq_Tail";
static const char *PANEL_COLUMNS = "\tPn_Name\tPn_Strand\tPn_Score\tPn_Len\tPn_Mism\tPn_Run\tPn_QStart\tPn_Start\tPn_End\tPn_Seeds\tPn_Second\tPn_Score2\tPn_PairSpan";
struct LocusSeq
{
  ConsensusSide side;
  string tail = ".";
  uint32_t tail_len = 0;
  struct bk_seq_hit hit = {0, -1, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0};
  string pair_span = ".";
};

static void write_lociseq_file(const Options &o, const vector<ClipLocusRow> &rows, const struct bk_clip_locus *all, uint64_t n, const vector<LocusSeq> &seqs,
                               const vector<string> &panel_names)
{
  std::ofstream table((o.out_file + "_cliploci_seq.txt").c_str());
  table << CLIPLOCI_COLUMNS << LOCISEQ_COLUMNS << (o.panel() ? PANEL_COLUMNS : "") << "\n";
  for (size_t k = 0; k < rows.size(); ++k)
  {
    const LocusSeq &x = seqs[k];
    table << cliploci_line(rows[k], all, n) << "\t" << x.side.c.n_reads << "\t" << x.side.c.len << "\t" << x.side.agree() << "\t" << (x.side.seq.empty() ? "." : x.side.seq) << "\t"
          << x.tail;
    if (o.panel())
    {
      const struct bk_seq_hit &h = x.hit;
      if (h.found)
        table << "\t" << panel_names[h.seq] << "\t" << (h.orient ? "-" : "+") << "\t" << h.score << "\t" << h.len << "\t" << h.mism << "\t" << h.run << "\t" << h.q_start + 1 << "\t"
              << h.s_start + 1 << "\t" << h.s_start + h.len << "\t" << h.n_seeds << "\t" << (h.seq2 >= 0 ? panel_names[h.seq2] : string(".")) << "\t" << h.score2 << "\t" << x.pair_span;
      else
        table << "\t.\t.\t.\t.\t.\t.\t.\t.\t.\t0\t.\t.\t.";
    }
    table << "\n";
  }
}

// -clip: <prefix>_fusion_rescued.txt, a table with the clip columns, and with -normal <prefix>_fusion_rescued_normal.txt: the same rows
// with the normal's evidence at the rescued peaks behind them
static void write_rescued_tables(const Options &o, const Rescued &rescued, const CallTables &t)
{
  const bool with_normal = o.with_normal();
  const string columns = string(CLIP_COLUMNS) + (with_normal ? CLIP_COLUMNS_NORMAL : "");
  std::ofstream table, table_normal;
  TwinFiles::open(table, o.out_file + "_fusion_rescued.txt", columns);
  if (with_normal) TwinFiles::open(table_normal, o.out_file + "_fusion_rescued_normal.txt", columns + RESCUED_COLUMNS_NORMAL);
  for (size_t k = 0; k < rescued.rows.size(); ++k)
  {
    const OutRow &r = rescued.rows[k];
    if (!rescued_written(r, o.all)) continue;
    const string clip = clip_columns(t.jsup[r.idx], t.csup[r.idx], with_normal ? &t.csup_normal[r.idx] : nullptr);
    write_row(table, r, clip);
    if (!with_normal) continue;
    const RescuedCall &x = rescued.calls[k];
    std::ostringstream tail;
    tail << "\t" << x.normal_drp << "\t" << x.normal_at[0] << "\t" << x.normal_at[1] << "\t" << x.normal_depth[0] << "\t" << x.normal_depth[1];
    write_row(table_normal, r, clip + tail.str());
  }
}

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
  const ConsensusMap *cons = nullptr;
  // -homology (else null; needs cons): the same for the junction fit; HOMLEN / HOMSEQ / JINS / JAL / JMM / JSH behind CSN
  const HomologyMap *hom = nullptr;
  // -similar (else null; never for the rescued clusters): SIMSCORE / SIMLEN / SIMRUN on both breakends of a call, last in INFO
  const SimilarMap *sim = nullptr;
  // -coverage (else null; never for the rescued clusters): COVL / COVR of the breakend's own side and RDRATIO, behind everything else
  const CoverageMap *cov = nullptr;
  // -frame (else null; never for the rescued clusters): FRCLASS / FR5P / FR3P on both breakends of a call, behind everything else
  const FrameMap *frame = nullptr;
  // -link (else null; never for the rescued clusters): EVENT on both breakends of a call in an event of more than one call, PARID where
  // the mate's records are in this file, behind everything else
  const LinkMap *link = nullptr;
  // -partners (else null; never for the rescued clusters): PTN / PTP / PTL of its own side on every breakend of a call, behind everything else
  const PartnerMap *partners = nullptr;
  // -fragsize (else null; never for the rescued clusters): FGN, and FGMEAN / FGZ where the columns have a value, on both breakends, behind everything else
  const FragsizeMap *frags = nullptr;
  // -known (else null; never for the rescued clusters): KNOWN / KNAMES, and KBEST where there is a hit, on both breakends, behind everything else
  const KnownMap *known = nullptr;
  // -context (else null; never for the rescued clusters): CXN, and MQ0F / MEANMQ where the side has a read, of the breakend's own side, behind everything else
  const ContextMap *context = nullptr;
  // -complexity (else null; never for the rescued clusters): LCDUST / LCGC / LCMASK where the columns have a value and LCSTR where a tract
  // lies at the breakpoint, of the breakend's own side, behind everything else
  const ComplexityMap *cplx = nullptr;
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

string KnownCall::info() const
{
  string s = ";KNOWN=" + std::to_string(k.n_hits) + ";KNAMES=" + std::to_string(k.n_names);
  if (k.best >= 0) s += ";KBEST=" + vcf_info_text(best_name);
  return s;
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
  std::set<uint64_t> in_file;  // -link: the calls whose records this file holds (a PARID names no other)
  if (in.link && !in.rescued)
    for (const OutRow &r : rows)
      if (call_written(r, in.all)) in_file.insert(r.idx);
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
        if (in.sim && in.sim->count(r.idx) && in.sim->at(r.idx).on)
        {
          const struct bk_locus_sim &ls = in.sim->at(r.idx).s;
          o << ";SIMSCORE=" << ls.score << ";SIMLEN=" << ls.len << ";SIMRUN=" << ls.run;
        }
        if (in.cov && in.cov->count(r.idx))
        {
          const CoverageCall &cc = in.cov->at(r.idx);
          o << ";COVL=" << cc.mean_text(cc.tumor, 2 * s) << ";COVR=" << cc.mean_text(cc.tumor, 2 * s + 1);
          if (cc.ratio_text(cc.tumor) != ".") o << ";RDRATIO=" << cc.ratio_text(cc.tumor);
        }
        if (in.frame && in.frame->count(r.idx)) o << in.frame->at(r.idx).info();
        if (in.link && in.link->count(r.idx))
        {
          const LinkCall &lk = in.link->at(r.idx);
          o << lk.info(s, lk.l.mate >= 0 && in_file.count(lk.mate_row));
        }
        if (in.partners && in.partners->count(r.idx)) o << in.partners->at(r.idx).info(s);
        if (in.frags && in.frags->count(r.idx)) o << in.frags->at(r.idx).info();
        if (in.known && in.known->count(r.idx)) o << in.known->at(r.idx).info();
        if (in.context && in.context->count(r.idx)) o << in.context->at(r.idx).info(s);
        if (in.cplx && in.cplx->count(r.idx)) o << (s ? in.cplx->at(r.idx).second : in.cplx->at(r.idx).first).info();
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
  if (in.sim && !in.rescued)
    v << "##INFO=<ID=SIMSCORE,Number=1,Type=Integer,Description=\"Score (+1 a match, -2 a mismatch) of the best ungapped stretch the reference around the two breakpoints shares, on either strand\">\n"
         "##INFO=<ID=SIMLEN,Number=1,Type=Integer,Description=\"Length of that stretch\">\n"
         "##INFO=<ID=SIMRUN,Number=1,Type=Integer,Description=\"Longest exact stretch the reference around the two breakpoints shares, on either strand\">\n";
  if (in.cov && !in.rescued)
    v << "##INFO=<ID=COVL,Number=1,Type=Float,Description=\"Mean depth of the aligned bases in the window left of this breakpoint's cut\">\n"
         "##INFO=<ID=COVR,Number=1,Type=Float,Description=\"Mean depth of the aligned bases in the window right of this breakpoint's cut\">\n"
         "##INFO=<ID=RDRATIO,Number=1,Type=Float,Description=\"Mean depth between the two breakpoints over the mean depth of the two outer flanks\">\n";
  if (in.frame && !in.rescued)
    v << "##INFO=<ID=FRCLASS,Number=1,Type=String,Description=\"Best class over all pairs of transcripts at the two breakpoints: antisense, truncating, promoter, outframe or inframe\">\n"
         "##INFO=<ID=FR5P,Number=1,Type=String,Description=\"Gene of the 5' partner of the reported pair of transcripts\">\n"
         "##INFO=<ID=FR3P,Number=1,Type=String,Description=\"Gene of the 3' partner of the reported pair of transcripts\">\n";
  if (in.link && !in.rescued)
    v << "##INFO=<ID=EVENT,Number=1,Type=String,Description=\"ID of the event of calls that share a breakpoint region: ev and the smallest call of the event\">\n"
         "##INFO=<ID=PARID,Number=1,Type=String,Description=\"ID of the paired breakend of the reciprocal junction\">\n";
  if (in.partners && !in.rescued)
    v << "##INFO=<ID=PTN,Number=1,Type=Integer,Description=\"Ends of discordant pairs inside the window of this side of the call\">\n"
         "##INFO=<ID=PTP,Number=1,Type=Integer,Description=\"Those whose mate lies inside the window of the other side\">\n"
         "##INFO=<ID=PTL,Number=1,Type=Integer,Description=\"Loci elsewhere that the mates of the others fall into\">\n";
  if (in.frags && !in.rescued)
    v << "##INFO=<ID=FGN,Number=1,Type=Integer,Description=\"Discordant pairs whose implied fragment length across the junction was computed\">\n"
         "##INFO=<ID=FGMEAN,Number=1,Type=Float,Description=\"Mean fragment length those pairs imply across the junction\">\n"
         "##INFO=<ID=FGZ,Number=1,Type=Float,Description=\"That mean less the library's mean insert size, in units of the library's sd\">\n";
  if (in.known && !in.rescued)
    v << "##INFO=<ID=KNOWN,Number=1,Type=Integer,Description=\"Entries of the panel of known junctions that hold both breakpoints of the call\">\n"
         "##INFO=<ID=KNAMES,Number=1,Type=Integer,Description=\"Different names among those entries\">\n"
         "##INFO=<ID=KBEST,Number=1,Type=String,Description=\"Name of the entry with the largest score among them\">\n";
  if (in.context && !in.rescued)
    v << "##INFO=<ID=CXN,Number=1,Type=Integer,Description=\"Primary alignments, duplicates and failed reads aside, that start within the context flank of this breakpoint, before any mapping-quality filter\">\n"
         "##INFO=<ID=MQ0F,Number=1,Type=Float,Description=\"Share of those alignments with mapping quality 0\">\n"
         "##INFO=<ID=MEANMQ,Number=1,Type=Float,Description=\"Mean mapping quality of those alignments\">\n";
  if (in.cplx && !in.rescued)
    v << "##INFO=<ID=LCDUST,Number=1,Type=Float,Description=\"DUST score of the reference window around this breakpoint: pairs of equal trinucleotides over the trinucleotides less one\">\n"
         "##INFO=<ID=LCGC,Number=1,Type=Float,Description=\"Share of C and G among the bases of that window\">\n"
         "##INFO=<ID=LCMASK,Number=1,Type=Float,Description=\"Share of that window the reference files soft-mask\">\n"
         "##INFO=<ID=LCSTR,Number=1,Type=String,Description=\"Longest exact tandem repeat that holds the breakpoint base or a neighbour of it: the unit, x, the columns it covers\">\n";
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
