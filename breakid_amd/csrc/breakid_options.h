// BreakID command line: the options (help text src/BreakID.h:27-36 of the reference, and this program's own) and what a command line
// is refused for.  Included by breakid_main.cc alone.
#pragma once
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "../../include/breakid_hip.h"
#include "../../include/breakid_multi.h"

// The entry points behind the per-call options, looked up at run time (prototypes: include/breakid_hip.h, include/breakid_multi.h), so
// that this program also links against a library without them: the CPU build of the host code (oracle/Makefile), which refuses the
// option.  check_options() is the only place that tests them for null.
extern "C" {
// -normal
int bk_normal_support(bk_ctx *tumor, bk_ctx *normal, double w, const struct bk_normal_support **out, uint64_t *count) __attribute__((weak));
// -genotype
int bk_ref_support(bk_ctx *calls, bk_ctx *records, int mapq_min, int anchor, double w, const struct bk_ref_support **out, uint64_t *count) __attribute__((weak));
int bk_genotype_call(uint32_t alt, uint32_t ref, uint8_t *gt, uint8_t *gq, float *vaf) __attribute__((weak));
// -vcf (the junction evidence and the two breakend rules)
int bk_junctions(bk_ctx *ctx, const struct bk_junction **out, uint64_t *count) __attribute__((weak));
int bk_junction_sides(const struct bk_junction *j, uint8_t *right1, uint8_t *right2, uint8_t *source) __attribute__((weak));
int bk_vcf_breakend_alt(char ref_base, int own_right, const char *mate_chr, uint32_t mate_pos, int mate_right, char *buf, size_t cap) __attribute__((weak));
// -evidence (bk_bam_extract is host code and always there)
int bk_evidence(bk_ctx *ctx, const struct bk_evidence **out, uint64_t *count, const uint64_t **call_off) __attribute__((weak));
// -consensus
int bk_clip_consensus(bk_ctx *ctx, const bk_reads *reads, const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, uint32_t max_len, uint32_t min_depth,
                      const struct bk_consensus **out, const uint8_t **bases, const uint32_t **col_depth) __attribute__((weak));
// -homology
int bk_junction_fit(bk_ctx *ctx, const bk_refseq *ref, const struct bk_junction_probe *probes, uint64_t n, const uint8_t *query, uint32_t max_len, uint32_t max_shift,
                    uint32_t max_ins, uint32_t max_hom, const struct bk_junction_fit **out) __attribute__((weak));
// -similar
int bk_locus_similarity(bk_ctx *ctx, const bk_refseq *ref, const struct bk_locus_pair *pairs, uint64_t n, uint32_t flank, const struct bk_locus_sim **out) __attribute__((weak));
// -coverage (the windows of a call and the aligned bases inside them)
int bk_window_coverage(bk_ctx *records, const struct bk_cov_window *windows, uint64_t n, int mapq_min, const struct bk_window_cov **out) __attribute__((weak));
int bk_call_windows(const bk_cluster *c, int right1, int right2, uint32_t flank, const uint32_t *target_len, struct bk_cov_window out[5]) __attribute__((weak));
// -context (the record classes and the mapping quality inside the windows of a call)
int bk_window_context(bk_ctx *records, const struct bk_cov_window *windows, uint64_t n, int mapq_min, const struct bk_window_ctx **out) __attribute__((weak));
// -frame
int bk_fusion_frame(bk_ctx *ctx, const bk_txmodel *model, const struct bk_frame_site *sites, uint64_t n, const struct bk_frame_call **out) __attribute__((weak));
// -link
int bk_link_calls(bk_ctx *ctx, const struct bk_link_site *sites, uint64_t n, uint32_t max_dist, const struct bk_call_link **out) __attribute__((weak));
// -partners (where the discordant pairs inside the windows of a call point to, and the windows of a call)
int bk_locus_partners(bk_ctx *ctx, const struct bk_partner_site *sites, uint64_t n, uint32_t max_gap, const struct bk_locus_partners **out) __attribute__((weak));
int bk_call_partner_sites(const bk_cluster *c, double w, struct bk_partner_site out[2]) __attribute__((weak));
// -fragsize (the fragment lengths the member pairs imply across a junction, and the library's bounds)
int bk_fragment_sizes(bk_ctx *ctx, const struct bk_frag_site *sites, uint64_t n, int32_t lo, int32_t hi, const struct bk_frag_sizes **out) __attribute__((weak));
int bk_fragment_bounds(double mean, double sd, int32_t *lo, int32_t *hi) __attribute__((weak));
// -known
int bk_known_calls(bk_ctx *ctx, const struct bk_known_entry *entries, uint64_t n_entries, const struct bk_known_site *sites, uint64_t n, uint32_t slop,
                   const struct bk_known_call **out) __attribute__((weak));
// -junctions (junction calls from the split reads alone; bk_base_depth is listed with -clip)
int bk_split_junctions(bk_ctx *ctx, int mapq_min, uint32_t tol, uint32_t min_reads, const struct bk_split_junction **out, uint64_t *count) __attribute__((weak));
int bk_split_junction_counts(bk_ctx *ctx, uint64_t out[6]) __attribute__((weak));
// -gaps (deletions and insertions from CIGAR gaps; bk_base_depth is listed with -clip)
int bk_cigar_gaps(bk_ctx *records, int mapq_min, uint32_t min_len, uint32_t anchor, uint32_t tol, uint32_t min_reads, const struct bk_cigar_gap **out, uint64_t *count) __attribute__((weak));
int bk_cigar_gap_counts(bk_ctx *records, uint64_t out[8]) __attribute__((weak));
// -cliploci (soft-clip pile-ups over the whole table; bk_base_depth is listed with -clip)
int bk_clip_loci(bk_ctx *records, bk_ctx *calls, int mapq_min, int min_clip, uint32_t tol, uint32_t pair_dist, uint32_t min_reads, const struct bk_clip_locus **out, uint64_t *count) __attribute__((weak));
int bk_clip_locus_counts(bk_ctx *records, uint64_t out[8]) __attribute__((weak));
// -panel (the junction sequence of a clip locus searched in the sequences of a FASTA)
int bk_sequence_match(bk_ctx *ctx, const bk_seq_panel *panel, const struct bk_seq_probe *probes, uint64_t n, const uint8_t *query, uint32_t max_len, uint32_t seed,
                      const struct bk_seq_hit **out) __attribute__((weak));
// -complexity
int bk_site_complexity(bk_ctx *ctx, const bk_refseq *ref, const struct bk_ref_site *sites, uint64_t n, uint32_t flank, uint32_t max_period, const struct bk_site_cplx **out) __attribute__((weak));
// -dedup
int bk_unique_support(bk_ctx *ctx, const struct bk_unique_support **out, uint64_t *count, const uint64_t **first, uint64_t *n_rows) __attribute__((weak));
// -clip (the soft-clip evidence, the depth at the rescued positions and the rescue rule)
int bk_clip_support(bk_ctx *calls, bk_ctx *records, int mapq_min, int min_clip, double w, const struct bk_clip_support **out, uint64_t *count) __attribute__((weak));
int bk_clip_reads(bk_ctx *records, const struct bk_clip_site *sites, uint64_t n_sites, int mapq_min, int min_clip, const uint32_t **counts, const struct bk_clip_read **rows,
                  const uint64_t **site_off) __attribute__((weak));
int bk_base_depth(bk_ctx *records, const int32_t *tid, const uint32_t *pos, uint64_t n, const uint32_t **out) __attribute__((weak));
int bk_clip_rescue(const bk_cluster *c, const struct bk_junction *j, const struct bk_clip_support *s, uint32_t min_support, uint32_t *pos1, uint32_t *pos2, uint32_t *n1,
                   uint32_t *n2) __attribute__((weak));
// -x
int bk_exclude_regions(bk_ctx *ctx, const bk_regions *r, uint64_t *n_removed) __attribute__((weak));
int bk_multi_run_ex(const bk_soa *host_table, const uint32_t *target_len, const char *const *target_name, int n_targets, const bk_regions *exclude, int n_gpus, int transport,
                    int mapq_min, int fast, double *w_out, uint64_t *n_clustered_total, bk_ctx **ctx0_out, char *err, size_t errlen) __attribute__((weak));
int bk_multi_run_bam_ex(const char *path, const bk_regions *exclude, int n_gpus, int transport, int mapq_min, int fast, double *w_out, uint64_t *n_clustered_total,
                        bk_ctx **ctx0_out, int *n_targets, const char *const **names, const uint32_t **lens, char *err, size_t errlen) __attribute__((weak));
int bk_multi_excluded(bk_ctx *ctx, uint64_t *n_removed) __attribute__((weak));
}

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
     \t -homins    \t longest inserted sequence, 0 to 64 (with -homology)  [32]\n \
     \t -similar   \t score the reference around the two breakpoints of every call against each other, forward and reverse-complemented (twin files *_similar.txt; SIMSCORE / SIMLEN / SIMRUN with -vcf)  \n \
     \t -simflank  \t bases either side of a breakpoint that are compared, 1 to 255 (with -similar)  [150]\n \
     \t -coverage  \t mean depth of the aligned bases either side of both breakpoints of every call, between them and over their contigs (twin files *_coverage.txt; COVL / COVR / RDRATIO with -vcf)  \n \
     \t -covflank  \t bases either side of a breakpoint that are averaged, 1 to 1000000 (with -coverage)  [1000]\n \
     \t -frame     \t 5' / 3' partner and reading frame of every call over all pairs of transcripts at its breakpoints (twin files *_frame.txt; FRCLASS / FR5P / FR3P with -vcf)  \n \
     \t -link      \t reciprocal partner, duplicates and event of every call among all voted calls (twin files *_link.txt; EVENT / PARID with -vcf)  \n \
     \t -linkdist  \t bases up to which two breakpoints count as one region, 0 to 1000000 (with -link)  [1000]\n \
     \t -partners  \t where the discordant pairs inside the two windows of every call point to: ends, ends to the partner window, loci elsewhere and the largest of them (twin files *_partners.txt; PTN / PTP / PTL with -vcf)  \n \
     \t -fragsize  \t the fragment lengths the discordant pairs of every call imply across its junction, against the library's insert sizes (twin files *_fragsize.txt; FGN / FGMEAN / FGZ with -vcf)  \n \
     \t -known     \t match every call against a panel of known junctions (BEDPE: chrom1 start1 end1 chrom2 start2 end2 [name score strand1 strand2]; twin files *_known.txt; KNOWN / KNAMES / KBEST with -vcf)  \n \
     \t -knownslop \t bases up to which a breakpoint beside an interval of the panel still falls into it, 0 to 1000000 (with -known)  [100]\n \
     \t -bedpe     \t also write the calls as BEDPE (*_fusion.bedpe), the format -known reads  \n \
     \t -context   \t what the alignments that start beside both breakpoints of every call look like before any filter: mean mapping quality, shares of MAPQ 0, low MAPQ, soft-clipped and improper reads, unmapped mates, duplicates, secondary and supplementary alignments (twin files *_context.txt; CXN / MQ0F / MEANMQ with -vcf)  \n \
     \t -ctxflank  \t bases either side of a breakpoint in which a read must start, about one fragment length, 1 to 1000000 (with -context)  [500]\n \
     \t -junctions \t also call junctions from the split reads alone, with or without discordant pairs: deletions and duplications shorter than the library's spread, small inversions (*_junctions.txt; *_junctions.bedpe with -bedpe)  \n \
     \t -jsupport  \t distinct reads a junction needs, 1 to 1000000 (with -junctions)  [3]\n \
     \t -jtol      \t bases up to which two junctions with equal sides are one call, 0 to 100 (with -junctions)  [2]\n \
     \t -complexity \t describe the reference around both breakpoints of every call by itself: soft-masked share, DUST score, GC and the exact tandem repeat at the breakpoint (twin files *_complexity.txt; LCDUST / LCGC / LCMASK / LCSTR with -vcf)  \n \
     \t -cplxflank \t bases either side of a breakpoint that are described, 1 to 255 (with -complexity)  [32]\n \
     \t -cplxperiod \t longest repeat unit that is looked for, 1 to 64 (with -complexity)  [6]\n \
     \t -gaps      \t also call deletions and insertions that the aligner wrote inside an alignment, as a long D or I operation of the CIGAR (*_gaps.txt; *_gaps.bedpe with -bedpe)  \n \
     \t -mingap    \t shortest D or I operation that counts, 1 to 1000000 (with -gaps)  [20]\n \
     \t -gapanchor \t matched bases an alignment needs on either side of the operation, 1 to 2147483647 (with -gaps)  [10]\n \
     \t -gaptol    \t bases up to which two gaps differ in start, and then in length, and are one call, 0 to 100 (with -gaps)  [2]\n \
     \t -gapsupport \t distinct reads a gap needs, 1 to 1000000 (with -gaps)  [3]\n \
     \t -cliploci  \t also call the places where soft-clipped reads without an SA tag pile up, with or without discordant pairs: mobile-element and viral insertion sites (*_cliploci.txt; *_cliploci.bedpe with -bedpe; -minclip and -q apply)  \n \
     \t -locitol   \t bases up to which two clip positions of one side are one locus, 0 to 100 (with -cliploci)  [2]\n \
     \t -locipair  \t bases up to which a left-clipped and a right-clipped locus may lie from a blunt junction and still face each other, 0 to 100000 (with -cliploci)  [50]\n \
     \t -locisupport \t distinct reads a locus needs, 1 to 1000000 (with -cliploci)  [3]\n \
     \t -lociseq   \t vote the clipped bases of every written locus into its junction sequence, with the length of the homopolymer tail at the junction (with -cliploci; *_cliploci_seq.txt; -conslen applies)  \n \
     \t -panel     \t name the sequence of a FASTA (mobile-element consensus sequences, a viral genome) that each junction sequence continues into: strand, position, the runner-up and the insert length a facing pair implies (with -lociseq; further columns of *_cliploci_seq.txt)  \n \
     \t -panelseed \t exact bases a junction sequence must share with a panel sequence to be compared with it, 8 to 16 (with -panel)  [12]\n ";

struct Options
{
  std::string inp_file, out_file, nib_dir, normal_file, exclude_file, known_file, panel_file, build = "hg19";
  int qual = 20, device = 0, n_gpus = 0, transport = BK_TRANSPORT_AUTO;  // -gpus N: one sample over N GPUs (include/breakid_multi.h)
  bool fast = false, all = false;                                        // -all: no gene-pair and repeat filter (the _fusion_all files)
  bool genotype = false, vcf = false, evidence = false, clip = false, dedup = false, consensus = false, homology = false, similar = false, coverage = false, frame = false, link = false, partners = false, fragsize = false, bedpe = false, context = false, junctions = false, complexity = false, gaps = false, cliploci = false, lociseq = false;
  bool anchor_given = false, minclip_given = false, clipsupport_given = false, conslen_given = false, homshift_given = false, homins_given = false, simflank_given = false, covflank_given = false, linkdist_given = false, knownslop_given = false, ctxflank_given = false, jsupport_given = false, jtol_given = false, cplxflank_given = false, cplxperiod_given = false, mingap_given = false, gapanchor_given = false, gaptol_given = false, gapsupport_given = false, locitol_given = false, locipair_given = false, locisupport_given = false, panelseed_given = false;
  long anchor = 10;                      // -anchor: bases a reference read must cover on either side of the breakpoint base
  long min_clip = 10, clip_support = 3;  // -minclip: shortest clip that counts; -clipsupport: reads at one position a rescued side needs
  long conslen = 64;                     // -conslen: longest junction sequence per side
  long homshift = 32, homins = 32;       // -homshift, -homins: the largest offset and the longest insertion bk_junction_fit looks for
  long simflank = 150;                   // -simflank: the bases either side of a breakpoint that bk_locus_similarity compares
  long covflank = 1000;                  // -covflank: the bases either side of a cut that bk_call_windows gives a flank window
  long linkdist = 1000;                  // -linkdist: the distance up to which bk_link_calls takes two breakends as near
  long knownslop = 100;                  // -knownslop: the distance up to which bk_known_calls lets a breakend fall into an interval
  long ctxflank = 500;                   // -ctxflank: the bases either side of a cut in which bk_window_context counts the records that start there
  long jsupport = 3, jtol = 2;           // -jsupport, -jtol: min_reads and tol of bk_split_junctions
  long cplxflank = 32, cplxperiod = 6;   // -cplxflank, -cplxperiod: flank and max_period of bk_site_complexity
  long mingap = 20, gapanchor = 10, gaptol = 2, gapsupport = 3;  // -mingap, -gapanchor, -gaptol, -gapsupport: min_len, anchor, tol and min_reads of bk_cigar_gaps
  long locitol = 2, locipair = 50, locisupport = 3;  // -locitol, -locipair, -locisupport: tol, pair_dist and min_reads of bk_clip_loci
  long panelseed = 12;                   // -panelseed: seed of bk_sequence_match
  bool multi() const { return n_gpus >= 1; }  // the sharded run
  bool known() const { return !known_file.empty(); }
  bool panel() const { return !panel_file.empty(); }
  bool with_normal() const { return !normal_file.empty(); }
  bool exclude() const { return !exclude_file.empty(); }
};

// One thing a command line is refused for.  USAGE rules stand behind the help text, as do the GPUS refusals; `text` is the rule, the
// option's name, or what could not be opened.
struct Refusal
{
  enum Kind { USAGE, GPUS, LIBRARY, OPEN } kind;
  bool fails;
  std::string text;
};

static bool opens(const std::string &path)
{
  FILE *probe = path.empty() ? nullptr : fopen(path.c_str(), "rb");
  if (probe) fclose(probe);
  return probe != nullptr;
}

// The first refusal that applies reports and ends the run: the order of the rows is behaviour.  An option that adds a per-call output
// has one row in `Feature` form: its name, whether it is set, whether it runs sharded, whether the library has what it calls.
static void check_options(const Options &o)
{
  struct Feature
  {
    const char *name;
    bool set, gpus_ok, present;
  };
  const Feature normal{"-normal", o.with_normal(), false, bk_normal_support != nullptr};
  const Feature genotype{"-genotype", o.genotype, false, bk_ref_support && bk_genotype_call};
  const Feature vcf{"-vcf", o.vcf, false, bk_junctions && bk_junction_sides && bk_vcf_breakend_alt};
  const Feature evidence{"-evidence", o.evidence, false, bk_evidence != nullptr};
  const Feature dedup{"-dedup", o.dedup, false, bk_unique_support != nullptr};
  const Feature homology{"-homology", o.homology, false, bk_junction_fit != nullptr};
  const Feature similar{"-similar", o.similar, false, bk_locus_similarity != nullptr};
  const Feature coverage{"-coverage", o.coverage, false, bk_window_coverage && bk_call_windows && bk_junctions && bk_junction_sides};
  const Feature frame{"-frame", o.frame, false, bk_fusion_frame && bk_junctions && bk_junction_sides};
  const Feature link{"-link", o.link, false, bk_link_calls && bk_junctions && bk_junction_sides};
  const Feature partners{"-partners", o.partners, false, bk_locus_partners && bk_call_partner_sites};
  const Feature fragsize{"-fragsize", o.fragsize, false, bk_fragment_sizes && bk_fragment_bounds && bk_junctions && bk_junction_sides};
  const Feature known{"-known", o.known(), false, bk_known_calls && bk_junctions && bk_junction_sides};
  const Feature bedpe{"-bedpe", o.bedpe, false, bk_junctions && bk_junction_sides};
  const Feature context{"-context", o.context, false, bk_window_context && bk_call_windows && bk_junctions && bk_junction_sides};
  const Feature junctions{"-junctions", o.junctions, false, bk_split_junctions && bk_split_junction_counts && bk_base_depth};
  const Feature complexity{"-complexity", o.complexity, false, bk_site_complexity != nullptr};
  const Feature gaps{"-gaps", o.gaps, false, bk_cigar_gaps && bk_cigar_gap_counts && bk_base_depth};
  const Feature cliploci{"-cliploci", o.cliploci, false, bk_clip_loci && bk_clip_locus_counts && bk_base_depth};
  const Feature lociseq{"-lociseq", o.lociseq, false, bk_clip_consensus && bk_clip_reads};
  const Feature panel{"-panel", o.panel(), false, bk_sequence_match != nullptr};
  const Feature consensus{"-consensus", o.consensus, false, bk_clip_consensus && bk_clip_reads && bk_evidence && bk_junctions && bk_junction_sides};
  const Feature clip{"-clip", o.clip, false, bk_clip_support && bk_clip_reads && bk_base_depth && bk_clip_rescue && bk_junctions && bk_junction_sides};
  const Feature exclude{"-x", o.exclude(), true, bk_exclude_regions && bk_multi_run_ex && bk_multi_run_bam_ex && bk_multi_excluded};
  auto rule = [](bool broken, const char *text) { return Refusal{Refusal::USAGE, broken, text}; };
  auto gpus = [&](const Feature &f) { return Refusal{Refusal::GPUS, f.set && !f.gpus_ok && o.multi(), f.name}; };
  auto library = [](const Feature &f) { return Refusal{Refusal::LIBRARY, f.set && !f.present, f.name}; };
  auto in_range = [](long v, long lo, long hi) { return v >= lo && v <= hi; };
  const long int_max = 0x7FFFFFFFl;
  const Refusal refusals[] = {
      rule(o.inp_file.empty() || o.out_file.empty(), "input- and output file is required."),
      rule(o.nib_dir.empty(), "nib file's root dir is required."),
      gpus(normal), library(normal), {Refusal::OPEN, normal.set && !opens(o.normal_file), "normal bam-file: " + o.normal_file},
      rule(o.anchor_given && !o.genotype, "-anchor needs -genotype."),
      gpus(genotype), rule(o.genotype && !in_range(o.anchor, 0, int_max), "-anchor must be a number from 0 to 2147483647."), library(genotype),
      gpus(vcf), library(vcf),
      gpus(evidence), library(evidence),
      gpus(dedup), library(dedup),
      rule((o.homshift_given || o.homins_given) && !o.homology, "-homshift and -homins need -homology."),
      rule(o.homology && !o.consensus, "-homology needs -consensus."), gpus(homology), library(homology),
      rule(o.homology && !(in_range(o.homshift, 0, 64) && in_range(o.homins, 0, 64)), "-homshift and -homins must be numbers from 0 to 64."),
      rule(o.conslen_given && !o.consensus && !o.lociseq, "-conslen needs -consensus."),
      gpus(consensus), library(consensus), rule(o.consensus && !in_range(o.conslen, 1, 256), "-conslen must be a number from 1 to 256."),
      rule(o.consensus && !in_range(o.min_clip, 1, int_max), "-minclip must be a number from 1 to 2147483647."),
      rule((o.minclip_given && !o.clip && !o.consensus && !o.cliploci) || (o.clipsupport_given && !o.clip), "-minclip and -clipsupport need -clip."),
      library(clip), gpus(clip),  // (the one option that looks for the library first)
      rule(o.clip && !(in_range(o.min_clip, 1, int_max) && in_range(o.clip_support, 1, int_max)), "-minclip and -clipsupport must be numbers from 1 to 2147483647."),
      gpus(exclude), library(exclude), {Refusal::OPEN, exclude.set && !opens(o.exclude_file), "exclude file: " + o.exclude_file},
      // (behind every older row: no command line without these options changes its answer)
      rule(o.simflank_given && !o.similar, "-simflank needs -similar."), gpus(similar), library(similar),
      rule(o.similar && !in_range(o.simflank, 1, 255), "-simflank must be a number from 1 to 255."),
      rule(o.covflank_given && !o.coverage, "-covflank needs -coverage."), gpus(coverage), library(coverage),
      rule(o.coverage && !in_range(o.covflank, 1, 1000000), "-covflank must be a number from 1 to 1000000."),
      gpus(frame), library(frame),
      rule(o.linkdist_given && !o.link, "-linkdist needs -link."), gpus(link),
      rule(o.link && !in_range(o.linkdist, 0, 1000000), "-linkdist must be a number from 0 to 1000000."), library(link),
      gpus(partners), library(partners),
      gpus(fragsize), library(fragsize),
      rule(o.knownslop_given && !o.known(), "-knownslop needs -known."), gpus(known),
      rule(o.known() && !in_range(o.knownslop, 0, 1000000), "-knownslop must be a number from 0 to 1000000."), library(known),
      {Refusal::OPEN, known.set && !opens(o.known_file), "known file: " + o.known_file},
      gpus(bedpe), library(bedpe),
      rule(o.ctxflank_given && !o.context, "-ctxflank needs -context."), gpus(context), library(context),
      rule(o.context && !in_range(o.ctxflank, 1, 1000000), "-ctxflank must be a number from 1 to 1000000."),
      rule((o.jsupport_given || o.jtol_given) && !o.junctions, "-jsupport and -jtol need -junctions."), gpus(junctions),
      rule(o.junctions && !in_range(o.jsupport, 1, 1000000), "-jsupport must be a number from 1 to 1000000."),
      rule(o.junctions && !in_range(o.jtol, 0, 100), "-jtol must be a number from 0 to 100."), library(junctions),
      rule(o.cplxflank_given && !o.complexity, "-cplxflank needs -complexity."), rule(o.cplxperiod_given && !o.complexity, "-cplxperiod needs -complexity."),
      gpus(complexity), library(complexity),
      rule(o.complexity && !in_range(o.cplxflank, 1, 255), "-cplxflank must be a number from 1 to 255."),
      rule(o.complexity && !in_range(o.cplxperiod, 1, 64), "-cplxperiod must be a number from 1 to 64."),
      rule((o.mingap_given || o.gapanchor_given || o.gaptol_given || o.gapsupport_given) && !o.gaps, "-mingap, -gapanchor, -gaptol and -gapsupport need -gaps."), gpus(gaps),
      rule(o.gaps && !in_range(o.mingap, 1, 1000000), "-mingap must be a number from 1 to 1000000."),
      rule(o.gaps && !in_range(o.gapanchor, 1, int_max), "-gapanchor must be a number from 1 to 2147483647."),
      rule(o.gaps && !in_range(o.gaptol, 0, 100), "-gaptol must be a number from 0 to 100."),
      rule(o.gaps && !in_range(o.gapsupport, 1, 1000000), "-gapsupport must be a number from 1 to 1000000."), library(gaps),
      rule((o.locitol_given || o.locipair_given || o.locisupport_given) && !o.cliploci, "-locitol, -locipair and -locisupport need -cliploci."), gpus(cliploci),
      rule(o.cliploci && !in_range(o.min_clip, 1, int_max), "-minclip must be a number from 1 to 2147483647."),
      rule(o.cliploci && !in_range(o.locitol, 0, 100), "-locitol must be a number from 0 to 100."),
      rule(o.cliploci && !in_range(o.locipair, 0, 100000), "-locipair must be a number from 0 to 100000."),
      rule(o.cliploci && !in_range(o.locisupport, 1, 1000000), "-locisupport must be a number from 1 to 1000000."), library(cliploci),
      rule(o.lociseq && !o.cliploci, "-lociseq needs -cliploci."), gpus(lociseq), library(lociseq),
      rule(o.lociseq && !in_range(o.conslen, 1, 256), "-conslen must be a number from 1 to 256."),
      rule((o.panel() || o.panelseed_given) && !o.lociseq, "-panel and -panelseed need -lociseq."), rule(o.panelseed_given && !o.panel(), "-panelseed needs -panel."), gpus(panel),
      rule(o.panel() && !in_range(o.panelseed, 8, 16), "-panelseed must be a number from 8 to 16."), library(panel),
      {Refusal::OPEN, panel.set && !opens(o.panel_file), "panel file: " + o.panel_file},
  };
  for (const Refusal &r : refusals)
  {
    if (!r.fails) continue;
    switch (r.kind)
    {
    case Refusal::USAGE: std::cerr << HELP << "Error: " << r.text << "\n"; break;
    case Refusal::GPUS: std::cerr << HELP << "Error: " << r.text << " cannot be combined with -gpus.\n"; break;
    case Refusal::LIBRARY: std::cerr << "Error: " << r.text << " needs the GPU library" << std::endl; break;
    case Refusal::OPEN: std::cerr << "Error: can not open " << r.text << std::endl; break;
    }
    exit(1);
  }
}

static Options parse_options(int argc, char *argv[])
{
  static struct option longopts[] = {{"help", 0, 0, 'h'}, {"i", 1, 0, 1}, {"o", 1, 0, 2}, {"q", 1, 0, 3}, {"n", 1, 0, 4},
                                     {"fast", 0, 0, 5},   {"t", 0, 0, 6}, {"all", 0, 0, 7}, {"gpu", 1, 0, 8}, {"gpus", 1, 0, 9},
                                     {"comm", 1, 0, 10},  {"normal", 1, 0, 11}, {"x", 1, 0, 12}, {"genotype", 0, 0, 13},
                                     {"anchor", 1, 0, 14}, {"vcf", 0, 0, 15}, {"evidence", 0, 0, 16}, {"clip", 0, 0, 17},
                                     {"minclip", 1, 0, 18}, {"clipsupport", 1, 0, 19}, {"dedup", 0, 0, 20}, {"consensus", 0, 0, 21},
                                     {"conslen", 1, 0, 22}, {"homology", 0, 0, 23}, {"homshift", 1, 0, 24}, {"homins", 1, 0, 25},
                                     {"similar", 0, 0, 26}, {"simflank", 1, 0, 27}, {"coverage", 0, 0, 28}, {"covflank", 1, 0, 29}, {"frame", 0, 0, 30},
                                     {"link", 0, 0, 31}, {"linkdist", 1, 0, 32}, {"partners", 0, 0, 33}, {"fragsize", 0, 0, 34},
                                     {"known", 1, 0, 35}, {"knownslop", 1, 0, 36}, {"bedpe", 0, 0, 37},
                                     {"context", 0, 0, 38}, {"ctxflank", 1, 0, 39},
                                     {"junctions", 0, 0, 40}, {"jsupport", 1, 0, 41}, {"jtol", 1, 0, 42},
                                     {"complexity", 0, 0, 43}, {"cplxflank", 1, 0, 44}, {"cplxperiod", 1, 0, 45},
                                     {"gaps", 0, 0, 46}, {"mingap", 1, 0, 47}, {"gapanchor", 1, 0, 48}, {"gaptol", 1, 0, 49}, {"gapsupport", 1, 0, 50},
                                     {"cliploci", 0, 0, 51}, {"locitol", 1, 0, 52}, {"locipair", 1, 0, 53}, {"locisupport", 1, 0, 54},
                                     {"lociseq", 0, 0, 55}, {"panel", 1, 0, 56}, {"panelseed", 1, 0, 57},
                                     {"f", 0, 0, 5},  // (-f used to complete to -fast alone; it still means it beside -frame)
                                     {0, 0, 0, 0}};
  Options o;
  auto number = [](long &value, bool &given) {
    value = atol(optarg);
    given = true;
  };
  int opt, li;
  optind = 0;
  while ((opt = getopt_long_only(argc, argv, "h?", longopts, &li)) != -1)
  {
    switch (opt)
    {
    case 'h': case '?': std::cerr << HELP; exit(1);
    case 1: o.inp_file = optarg; break;
    case 2: o.out_file = optarg; break;
    case 3: o.qual = (int) std::labs(atol(optarg)); break;
    case 4: o.nib_dir = optarg; break;
    case 5: o.fast = true; break;
    case 6: break;  // the reference dereferences a NULL optarg here (has_arg = 0); `times` is effectively always 2
    case 7: o.all = true; break;
    case 8: o.device = atoi(optarg); break;
    case 9: o.n_gpus = atoi(optarg); break;
    case 10: o.transport = !strcmp(optarg, "rccl") ? BK_TRANSPORT_RCCL : !strcmp(optarg, "local") ? BK_TRANSPORT_LOCAL : BK_TRANSPORT_AUTO; break;
    case 11: o.normal_file = optarg; break;
    case 12: o.exclude_file = optarg; break;
    case 13: o.genotype = true; break;
    case 14: number(o.anchor, o.anchor_given); break;
    case 15: o.vcf = true; break;
    case 16: o.evidence = true; break;
    case 17: o.clip = true; break;
    case 18: number(o.min_clip, o.minclip_given); break;
    case 19: number(o.clip_support, o.clipsupport_given); break;
    case 20: o.dedup = true; break;
    case 21: o.consensus = true; break;
    case 22: number(o.conslen, o.conslen_given); break;
    case 23: o.homology = true; break;
    case 24: number(o.homshift, o.homshift_given); break;
    case 25: number(o.homins, o.homins_given); break;
    case 26: o.similar = true; break;
    case 27: number(o.simflank, o.simflank_given); break;
    case 28: o.coverage = true; break;
    case 29: number(o.covflank, o.covflank_given); break;
    case 30: o.frame = true; break;
    case 31: o.link = true; break;
    case 32: number(o.linkdist, o.linkdist_given); break;
    case 33: o.partners = true; break;
    case 34: o.fragsize = true; break;
    case 35: o.known_file = optarg; break;
    case 36: number(o.knownslop, o.knownslop_given); break;
    case 37: o.bedpe = true; break;
    case 38: o.context = true; break;
    case 39: number(o.ctxflank, o.ctxflank_given); break;
    case 40: o.junctions = true; break;
    case 41: number(o.jsupport, o.jsupport_given); break;
    case 42: number(o.jtol, o.jtol_given); break;
    case 43: o.complexity = true; break;
    case 44: number(o.cplxflank, o.cplxflank_given); break;
    case 45: number(o.cplxperiod, o.cplxperiod_given); break;
    case 46: o.gaps = true; break;
    case 47: number(o.mingap, o.mingap_given); break;
    case 48: number(o.gapanchor, o.gapanchor_given); break;
    case 49: number(o.gaptol, o.gaptol_given); break;
    case 50: number(o.gapsupport, o.gapsupport_given); break;
    case 51: o.cliploci = true; break;
    case 52: number(o.locitol, o.locitol_given); break;
    case 53: number(o.locipair, o.locipair_given); break;
    case 54: number(o.locisupport, o.locisupport_given); break;
    case 55: o.lociseq = true; break;
    case 56: o.panel_file = optarg; break;
    case 57: number(o.panelseed, o.panelseed_given); break;
    default: std::cerr << "Error: cannot parse arguments.\n"; exit(1);
    }
  }
  check_options(o);
  return o;
}
