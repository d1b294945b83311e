/* C ABI of libdl4vc_cand.so: candidate generation from a BAM (the first stage of call_variants.sh; reference
 * tools/candidate_generator.py).  Host threads inflate and frame the records of each subregion; the per-read work (CIGAR + MD
 * walk, allele keys, coverage) and the per-locus counting (radix sort + run-length encode of the keys, depth by a scan of
 * coverage difference events, the allele-frequency filter in double precision) run on the GPU.  Bindings:
 * dl4vc_amd/candgen.py.
 *
 * Every call returns 0 on success and a negative code on failure; cg_last_error() then says why.  No call aborts the process
 * on bad input: a corrupt BAM is an error code. */
#ifndef DL4VC_CANDGEN_H
#define DL4VC_CANDGEN_H

#include <stdint.h>

#include "dl4vc_loader.h"   /* dl4vc_read_stats */

#ifdef __cplusplus
extern "C" {
#endif

/* The longest REF or ALT an allele key holds (bases, anchor included): --max_len_indel_allele may not exceed it. */
#define CG_MAX_ALLELE_LEN 63

typedef struct cg_handle cg_handle_t;

typedef struct {
    int32_t threads;               /* host threads that inflate and frame records (<= 0: 1) */
    int32_t max_len_indel_allele;  /* indels whose REF or ALT is longer are dropped (reference CLI default 60) */
    double snp_min_freq;           /* a SNP is kept when min(count, depth) / depth > snp_min_freq */
    double indel_min_freq;         /* the same for an insertion or deletion */
    int32_t device;                /* HIP device ordinal */
} cg_options;

/* One subregion: reads are fetched over [start, end) (htslib's overlap rule), alleles counted at start <= pos <= end. */
typedef struct {
    int32_t tid;
    int32_t start;
    int32_t end;
} cg_region;

/* One surviving allele of one subregion.  ref / alt are NUL-terminated upper-case bases. */
typedef struct {
    int32_t region;                /* index into the cg_run regions array */
    int32_t tid;
    int32_t pos0;                  /* 0-based position (the anchor base of an indel) */
    int32_t depth;                 /* reads whose M/=/X operations cover pos0, in this subregion's fetch */
    int32_t count;                 /* reads of this subregion carrying the allele */
    char ref[CG_MAX_ALLELE_LEN + 1];
    char alt[CG_MAX_ALLELE_LEN + 1];
} cg_candidate;

typedef struct {
    int64_t reads;                 /* records fetched, summed over subregions (a read in two subregions counts twice) */
    int64_t reads_no_md;           /* coverage counted, no alleles (the reference's "MD tag not present") */
    int64_t reads_no_pairs;        /* no CIGAR or no reference-consuming operation: no alleles */
    int64_t reads_unsupported;     /* N or P CIGAR operation, or SEQ '*': coverage counted, alleles skipped */
    int64_t reads_malformed;       /* MD inconsistent with CIGAR / SEQ, or a letter outside the BAM alphabet: alleles skipped */
    int64_t reads_deletions_dropped; /* a deletion anchored on an inserted base: the read's deletions dropped */
    int64_t allele_events;         /* alleles emitted by reads, before counting */
    int64_t alleles;               /* distinct (subregion, allele) after counting */
    int64_t candidates;            /* survivors of the frequency filter */
    int64_t batches;
    double host_frame_ms;          /* inflate + frame (wall time of the host threads) */
    double upload_ms;              /* host -> device copy of the framed records */
    double device_ms;              /* count, scan, emit, sort, encode, depth, filter (device events) */
    double total_ms;
} cg_stats;

/* What the device inflate path did in the last cg_run (all zero when it is off). */
typedef struct {
    int64_t blocks;                /* BGZF blocks inflated (a block two ranges touch counts for each) */
    int64_t compressed_bytes;      /* read from the file and uploaded as they are */
    int64_t inflated_bytes;
    int64_t records;               /* BAM records walked and framed on the device */
    double read_ms;                /* host: index ranges, file to pinned memory, header / trailer checks */
    double inflate_ms;             /* device events around the inflate kernel */
    double walk_frame_ms;          /* device events around the walk, frame, scan and emit passes */
} cg_inflate_stats;

/* What the reference source did (all zero when it is off).  reads is of the last cg_run; the rest describe the contigs that are
 * resident now and the one-time cost of loading them, summed since cg_set_reference. */
typedef struct {
    int64_t reads;                 /* reads without MD taken against the FASTA (a read in two subregions counts twice) */
    int64_t contigs;               /* contigs resident on the device */
    int64_t bases;                 /* their bases = their bytes on the device */
    int64_t other_bytes;           /* bytes outside "=ACMGRSVTWYHKDBN" (either case) at base positions: read as N */
    double read_ms;                /* host: the contigs' raw byte ranges read from the FASTA */
    double upload_convert_ms;      /* host -> device copy of the raw bytes and the kernel that makes codes of them */
} cg_reference_stats;

int cg_open(const char* bam_path, const char* bai_path /* NULL or "": linear scan */, const cg_options* opt,
            cg_handle_t** out);
/* Runs every region (internally in batches).  On success *out points at n_out candidates owned by the handle, valid until the
 * next cg_run or cg_close; their order is unspecified. */
int cg_run(cg_handle_t* h, const cg_region* regions, int64_t n_regions, const cg_candidate** out, int64_t* n_out,
           cg_stats* stats);
/* on != 0: the BGZF blocks of each batch go to the device compressed, and inflate, record walk and framing run there
 * (dl4vc_bgzf.h has the decoder's statuses); the host reads the file and the index and does no per-record work.  Needs the BAI
 * (its bins give the byte ranges): fails with a message on a handle opened without one.  Limits: ISIZE <= 65536 per block (the
 * format's), one inflated buffer per batch sized from the block trailers.  Off by default; cg_stats.host_frame_ms keeps its
 * meaning (host wall time in front of the device work). */
int cg_set_inflate_device(cg_handle_t* h, int on);
int cg_get_inflate_stats(const cg_handle_t* h, cg_inflate_stats* out);
/* Read subsampling by name hash, the rule of `samtools view --subsample fraction --subsample-seed seed` (csrc/bam_frame.h:
 * keep iff (wang(X31(read name) ^ seed) & 0xffffff) < ceil(fraction * 2^24)).  A record is framed and checked as without the
 * option and then dropped where a record outside the subregion is dropped, on the host or in the device's frame kernel: every
 * count behind that point (depth, alleles, cg_stats.reads) sees the kept reads alone, and a damaged record gives the same error
 * at the same offset.  Mates share a name and so an answer; a read in two subregions gets one answer.  fraction 0 turns it off
 * again, 1 keeps every read; a fraction outside [0, 1] or NaN is refused.  Unpinned against samtools itself. */
int cg_set_subsample(cg_handle_t* h, double fraction, uint32_t seed);
/* Of the last cg_run: records that passed the region test (a read in two subregions counts twice, as in cg_stats.reads) and
 * those of them the rule kept (= cg_stats.reads).  Equal with the option off. */
typedef struct {
    int64_t records_seen;
    int64_t records_kept;
} cg_subsample_stats;
int cg_get_subsample_stats(const cg_handle_t* h, cg_subsample_stats* out);
/* Read filter by flags and mapping quality (the rule of `samtools view -F exclude -f require -q min_mapq`, one definition in
 * csrc/bam_frame.h; pe_set_read_filter in dl4vc_loader.h states it).  A record is framed and checked as without the option, then
 * dropped where a record outside the subregion is dropped, in front of the sample rule, on the host or in the device's frame
 * kernel: depth, alleles and cg_stats.reads see the kept reads alone, and cg_subsample_stats.records_seen counts what passed
 * region and filter.  All zero: off.  Refused: a mask outside [0, 0xFFFF], min_mapq outside [0, 255], a bit in both masks.
 * cg_set_read_stats(h, 1): the read census (dl4vc_read_stats, dl4vc_loader.h) of a cg_run is collected without a filter too; a
 * read in two subregions counts twice, as in cg_stats.reads.  With neither, the frame kernel runs as without the option. */
int cg_set_read_filter(cg_handle_t* h, int32_t exclude, int32_t require, int32_t min_mapq);
int cg_set_read_stats(cg_handle_t* h, int on);
int cg_get_read_stats(const cg_handle_t* h, dl4vc_read_stats* out);
/* fasta_path: a read WITHOUT an MD tag is walked against the bases of its contig in this FASTA (indexed by fasta_path.fai when
 * that file exists, else scanned once), in the same kernels; a read WITH an MD tag is walked by its MD as before, whatever the
 * FASTA says.  NULL or "": off again (such reads count in cg_stats.reads_no_md and give no alleles), and the resident contigs
 * are freed.  A contig is read, uploaded and converted to one byte per base the first time a cg_run touches it and stays on the
 * device for the handle's life: 1 byte per base, whole contigs, no eviction.  Fails here when the FASTA cannot be opened; cg_run
 * fails, naming the contig, when the FASTA lacks a contig it needs, when its length there differs from the BAM header's (both
 * lengths are given), or when the index does not describe the file (a line end or '>' at a base position). */
int cg_set_reference(cg_handle_t* h, const char* fasta_path);
int cg_get_reference_stats(const cg_handle_t* h, cg_reference_stats* out);
/* For tests: the conversion cg_set_reference applies, on raw[0, raw_len) = the contig's bytes from its first base on, line
 * breaks included: out[p] = the BAM nibble code of base p for p < length, *n_other = the bytes read as N for being outside the
 * alphabet.  cg_reference_codes_host runs the rule on the CPU, cg_reference_codes the kernel on `device`.  -3 when a base
 * position holds a line end or '>' or lies past raw_len (out is then unspecified). */
int cg_reference_codes_host(const uint8_t* raw, uint64_t raw_len, int64_t linebases, int64_t linewidth, int64_t length,
                            uint8_t* out, int64_t* n_other);
int cg_reference_codes(const uint8_t* raw, uint64_t raw_len, int64_t linebases, int64_t linewidth, int64_t length, uint8_t* out,
                       int64_t* n_other, int device);
/* Left-alignment of insertions and deletions (csrc/cand_left_align.h has the rule).  on != 0: before an indel observation is
 * counted, the kernels move it to its left-most placement on the reference bases of its contig, so that the placements of one
 * event inside a homopolymer or tandem repeat give one allele key, one count and one record.  The shift stops at the read's own
 * POS (the read covers its shifted anchor, so the subregion of the new position fetches it) and at a reference base outside
 * ACGT.  Not shifted, and counted as before: an indel anchored on a deleted or inserted position or on the stand-in anchor of a
 * leading deletion, one with a base outside ACGT, and one whose anchor or deleted bases differ from the FASTA (an MD tag that
 * disagrees with it).  The length limit, the deletion-drop rule and the coverage are those of the option off; the position
 * tests and the depth are taken at the shifted position.  Needs cg_set_reference: refused with the reason on a handle without
 * one (the handle stays usable), and while it is on cg_set_reference(h, NULL) is refused.  A consequence of needing the
 * reference: reads without MD are walked against the FASTA too.  Off by default. */
int cg_set_left_align(cg_handle_t* h, int on);
/* Of the last cg_run, over the indel observations that were counted as alleles (all zero with the option off): exact integer
 * sums, independent of the order the reads ran in. */
typedef struct {
    int64_t observations;          /* = the indel share of cg_stats.allele_events */
    int64_t shifted;               /* moved by at least one base */
    int64_t bases_shifted;         /* the sum of their shifts */
    int64_t clamped;               /* stopped at the read's POS where the reference would have let them go on */
    int64_t not_eligible;          /* left as they were */
} cg_left_align_stats;
int cg_get_left_align_stats(const cg_handle_t* h, cg_left_align_stats* out);
/* For tests and the sanitizer program: the rule for one observation, on the CPU.  codes[0, length): the contig as BAM nibble
 * codes; kind 1 = insertion, 2 = deletion; anchor_aligned: the anchor is an aligned pair of the read; bases[0, n_bases): the
 * inserted or deleted bases as codes; floor: the read's POS.  *pos_out = the placement's anchor position, bases_out[0] its
 * anchor code and bases_out[1 .. n_bases] its bases (n_bases + 1 bytes), *flags = 1 (eligible) | 2 (clamped).  An observation
 * that is not eligible, n_bases > 63 included, comes back as it went in with *flags = 0.  Reads nothing outside codes[0, length). */
int cg_left_align_host(const uint8_t* codes, int64_t length, int32_t kind, int32_t anchor_aligned, int64_t anchor_pos,
                       int32_t anchor_code, const uint8_t* bases, int32_t n_bases, int64_t floor, int64_t* pos_out,
                       uint8_t* bases_out, int32_t* flags);
/* For tests: the byte ranges and walk boundaries the device path would use for one region, as BGZF virtual offsets.
 * ranges: n_ranges pairs [begin, end), merged and sorted; bounds: every walk boundary (range ends included), sorted.  At most
 * cap_* entries are written; the counts are always the full ones.  Reads the index only. */
int cg_debug_ranges(const cg_handle_t* h, int32_t tid, int32_t start, int32_t end, uint64_t* ranges, int64_t cap_ranges,
                    int64_t* n_ranges, uint64_t* bounds, int64_t cap_bounds, int64_t* n_bounds);
/* Reference names and lengths of the BAM header. */
int32_t cg_n_refs(const cg_handle_t* h);
const char* cg_ref_name(const cg_handle_t* h, int32_t tid);
int64_t cg_ref_length(const cg_handle_t* h, int32_t tid);
const char* cg_last_error(void);
void cg_close(cg_handle_t* h);

#ifdef __cplusplus
}
#endif
#endif
