/*
 * dl4vc_loader.h -- C ABI of the native batched candidate loader (libdl4vc_loader.so).
 *
 * Replaces, for the inference path, the reference's per-item data pipeline:
 *   DataLoader(ContextDatasetFromNumpy(test_file), batch_size, shuffle=False, num_workers=5)   main.py:86-94
 *   ContextDatasetFromNumpy.__getitem__ / _get_generator                                      dl4vc/dataset.py:494-680
 *   sample_single_reads (row subset)                                                           dl4vc/dataset.py:256-287
 *   get_read_mask_vectors (allele masks) + the blacklist fallback                              dl4vc/dataset.py:112-250, 644-663
 * It reads the HDF5 file the converter writes (dataset "data", packed compound records,
 * tools/convert_bam_single_reads.py:659,694-698) and delivers batches of the six uint8 planes that
 * dan_forward() consumes, in record order.  Host-only C++; libhdf5 is dlopen'ed at run time.
 * Every function returns 0 / a count on success and a negative value on error (text: dl_last_error / pe_last_error):
 * -1 a refused argument or file, -2 a piece of dl_next that failed, -4 an exception caught at the entry (dl_open, dl_next,
 * dl_select_rows, dl_select_rows_downsample, dl_allele_masks, pe_open, pe_encode), its text "<entry>: <what()>".  No entry lets an exception out.
 */
#ifndef DL4VC_LOADER_H
#define DL4VC_LOADER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dl_loader dl_loader_t;

/* Open `hdf_path` for records [lo, hi) (hi < 0 = to the end).  `reads` = R rows per site (max_reads of the
 * dataset class, dl4vc/dataset.py:409); `batch_sites` = sites per dl_next() call.  Pileups that store more than R
 * reads get a sorted random subset drawn like numpy's legacy RandomState seeded with (seed + absolute record
 * index) -- exactly np.random.seed(s); np.random.random(); np.random.choice(...) of the reference (dataset.py:274-281,
 * 531); with use_seed = 0 such a record is an error instead of an unpinned draw.  `threads` worker threads inflate
 * and assemble 128-site pieces; at most `prefetch` batches are prepared ahead.  `libhdf5_path` may be NULL/"".
 * Refused (-1) with "<path>: unexpected record layout": a record type in which single_reads, q-scores or strand (each
 * stored rows x 201 bytes), ref_bases (201), vcfrec (128) or num_reads (4) does not end inside the record, or whose planes are
 * not laid out as the converter packs them.  When it fails nothing stays open and no thread stays behind. */
int dl_open(const char* hdf_path, const char* libhdf5_path, int32_t reads, int64_t lo, int64_t hi, int32_t batch_sites,
            uint64_t seed, int32_t use_seed, int32_t threads, int32_t prefetch, dl_loader_t** out);
int64_t dl_num_records(const dl_loader_t* l);          /* len(dataset), dl4vc/dataset.py:489-491 */
int64_t dl_num_sites(const dl_loader_t* l);            /* hi - lo */
int32_t dl_window(const dl_loader_t* l);               /* columns per read (201) */
/* Next batch in record order into caller buffers (any may be NULL): reads/qual/strand [n][R][L], ref/ref_mask/
 * var_mask [n][L], vcfrec [n][129] NUL-terminated, num_reads [n], blacklist [n].  Returns n (0 at the end), -2 when a piece
 * failed: a record the loader refuses (named), "zlib inflate failed", "chunk <c> holds <have> bytes[ once inflated], the piece
 * needs <need> of it" (no length in the file is trusted: a chunk that inflates short, or is stored short without the filter,
 * is never served from a buffer another chunk left), "native loader: <what()>" for what a worker thread threw; -4 (as
 * int64_t) for an exception in the call itself. */
int64_t dl_next(dl_loader_t* l, uint8_t* reads, uint8_t* qual, uint8_t* strand, uint8_t* ref, uint8_t* ref_mask,
                uint8_t* var_mask, char* vcfrec, int32_t* num_reads, uint8_t* blacklist);
void dl_close(dl_loader_t* l);                         /* stops and joins the workers, closes the file; NULL is allowed */
const char* dl_last_error(const dl_loader_t* l);       /* l may be NULL: error of the last failed dl_open */

/* Exposed for parity tests: the subset draw and the allele masks on their own.
 * dl_select_rows: rows_out gets the chosen stored rows, returns their count.
 * dl_allele_masks: 0 = ok, 1 = blacklisted (the reference's AssertionError cases: zero masks), 2 = fatal (the
 * reference dies with a non-assert exception). */
int dl_select_rows(uint32_t seed, int32_t num_reads, int32_t stored_rows, int32_t max_reads, int32_t* rows_out);
/* dl_select_rows with the reference's dynamic read down-sampling (dl4vc/dataset.py:17-22, 256-281, 531), draw for draw after
 * np.random.seed(seed): the coin u = random(); if u < prob, d = clip(normal(rate, max(0.001, rate / 2)), 0, 0.8) (the legacy
 * polar Box-Muller) and sampled = int((1 - d) * num_reads) reads are kept, else all.  If no read is dropped the rows are
 * dl_select_rows's.  Otherwise min(R', sampled) sorted rows of the first min(stored_rows, num_reads), R' = min(max_reads,
 * stored_rows), filled up to R' with stored row stored_rows - 1; where rows were filled, zero_reads_out[r] = 1 for every row r
 * that names stored row stored_rows - 1 (the reference zeroes that row's reads plane, not its quality or strand), else 0.
 * rows_out, zero_reads_out: max(max_reads, stored_rows) entries; sampled_out (may be NULL) gets sampled.  Returns the count of
 * rows, -1 for a bad argument (a rate outside [0, 1), a prob outside [0, 1], a negative size). */
int dl_select_rows_downsample(uint32_t seed, int32_t num_reads, int32_t stored_rows, int32_t max_reads, double rate, double prob,
                              int32_t* rows_out, uint8_t* zero_reads_out, int32_t* sampled_out);
int dl_allele_masks(const char* vcfrec, const uint8_t* window /*[201]*/, uint8_t* ref_mask, uint8_t* var_mask);

/* ---- native pileup encoder -------------------------------------------------------------
 * Replaces the per-location work of the reference's converter, which it spreads over 80 pysam processes:
 *   process_location                      tools/convert_bam_single_reads.py:846-1118   (pileup columns -> three image planes)
 *   process_locations_chunk, image part   tools/convert_bam_single_reads.py:720-838    (crop / trim / centre / pad -> record)
 *   samfile.pileup(...) / fetch           tools/convert_bam_single_reads.py:873-874    (BGZF, BAM records, BAI, CIGAR walk)
 * pe_encode fills, for each location (contig name, 1-based VCF POS), the image fields of the converter's record
 * (:694-698): single_reads / q-scores / strand [max_reads][2 w + 1], ref_bases [2 w + 1], num_reads; name / label / vcfrec are
 * text the caller already has.  status: 1 = planes written, 0 = the location yields no record (no read over the candidate's
 * column; the reference counts an error), 2 = the location needs the column-by-column form (reads sharing a name:sequence
 * key, a reference skip, a base outside the token table, > 1000 columns, > 8000 reads, min_base_quality > 0): the Python
 * module encodes those, so results are identical to dl4vc_amd/pileup_encoder.py for every location.  Also 2, because the
 * specification has no answer: a read inside the window whose alignment has no reference position (0M 5I) or whose SEQ
 * is shorter than its CIGAR's query length (SEQ '*'); the Python module raises ValueError there.  `threads` workers take
 * contiguous runs of locations (locations sorted by position keep every alignment parsed once per run).
 * A BAM record is framed by the core every BAM path shares (csrc/bam_frame.h); one it refuses fails pe_encode (-1) with the
 * core's text, e.g. "corrupt BAM record (l_read_name)" for a name length of 0, "... (l_seq exceeds the record)". */
typedef struct pe_encoder pe_encoder_t;
typedef struct pe_options {
    int32_t window_size;                 /* --window-size (100) */
    int32_t max_reads;                   /* --max-reads (call_variants.sh: 200) */
    int32_t max_insert_length;           /* --max-insert-length (10) */
    int32_t max_insert_length_variant;   /* --max-insert-length-variant (50) */
    int32_t min_base_quality;            /* --min-base-quality (0) */
} pe_options;
int pe_open(const char* bam_path, const char* bai_path /* NULL: <bam>.bai, <stem>.bai, else a linear scan */, const char* fasta_path,
            const pe_options* opt, pe_encoder_t** out);
int pe_encode(pe_encoder_t* e, const char* const* contigs, const int32_t* positions, int64_t n, uint8_t* reads_out, uint8_t* qual_out,
              uint8_t* strand_out, uint8_t* ref_out, int32_t* num_reads_out, int8_t* status_out, int32_t threads);
/* Read subsampling by name hash, the rule of `samtools view --subsample fraction --subsample-seed seed` (csrc/bam_frame.h): a
 * record the rule drops overlaps no window.  fraction 0: off; outside [0, 1] or NaN: refused (-1, pe_last_error(e)). */
int pe_set_subsample(pe_encoder_t* e, double fraction, uint32_t seed);
/* The rule alone, for tests: 1 if a record whose read name field is name[0, l_read_name) (the bytes as they lie in the record,
 * NUL included; 1 <= l_read_name <= 255) is kept at `fraction` in (0, 1] and `seed`, 0 if dropped, -1 for a refused argument. */
int pe_subsample_keeps(const uint8_t* name, int32_t l_read_name, double fraction, uint32_t seed);
/* Read filter by flags and mapping quality, the rule of `samtools view -F exclude -f require -q min_mapq` (csrc/bam_frame.h): a
 * read is kept iff (flag & exclude) == 0 && (flag & require) == require && MAPQ >= min_mapq.  A record is framed and checked as
 * without the option and then dropped where a record outside the window is dropped, in front of the sample rule; the encoder's own
 * fixed mask (0x704) stays behind it.  All zero: off.  exclude or require outside [0, 0xFFFF], min_mapq outside [0, 255] or a bit
 * in both masks (nothing could pass): refused (-1, pe_last_error(e)). */
int pe_set_read_filter(pe_encoder_t* e, int32_t exclude, int32_t require, int32_t min_mapq);
/* The read census, one struct for the three BAM consumers (pe_, pg_ and cg_get_read_stats): the records that passed the region
 * test, counted in front of the filter and the sample rule, once per region they belong to (pe_: per location window, pg_: per run
 * of locations, cg_: per subregion).  dropped_flags is tested before dropped_mapq, so a record counts in one; kept is what is left
 * behind the sample rule as well.  Collected with a filter on or after *_set_read_stats(h, 1); all zero otherwise. */
typedef struct dl4vc_read_stats {
    uint64_t mapq_hist[256];   /* records by MAPQ */
    uint64_t flag_bits[16];    /* records with flag bit k set */
    uint64_t seen;
    uint64_t dropped_flags;
    uint64_t dropped_mapq;
    uint64_t kept;
} dl4vc_read_stats;
int pe_set_read_stats(pe_encoder_t* e, int on);
int pe_get_read_stats(const pe_encoder_t* e, dl4vc_read_stats* out);     /* of the last pe_encode */
/* The rule alone, for tests: 1 if a record with these flags and MAPQ is kept, 0 if dropped, -1 for a refused argument. */
int pe_read_filter_passes(int32_t flag, int32_t mapq, int32_t exclude, int32_t require, int32_t min_mapq);
void pe_close(pe_encoder_t* e);
const char* pe_last_error(const pe_encoder_t* e);      /* e may be NULL: error of the last failed pe_open */

#ifdef __cplusplus
}
#endif
#endif /* DL4VC_LOADER_H */
