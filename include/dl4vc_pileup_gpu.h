/* C ABI of libdl4vc_pileup.so: the pileup encoder of include/dl4vc_loader.h (pe_*) with the image built on the GPU.
 * Bindings: dl4vc_amd/pileup_gpu.py.
 *
 * Host threads fetch the records of each run of locations once (BAI linear index, else a linear scan), frame and validate
 * them (bam_native.h) into one pinned buffer and read the reference slices (fasta_native.h).  On the device one kernel
 * resolves every record's CIGAR (per reference position: query position, deletion, merged indel length) and hashes its
 * name:sequence key; a second kernel, one workgroup per location, picks the tracks, builds coverage, the capped insertion
 * widths and the column map in LDS, and writes the cropped, trimmed, centred and padded planes.
 *
 * The contract with pe_encode, location by location:
 *   status 1: reads / qual / strand / ref / num_reads are byte-identical to what pe_encode writes;
 *   status 0: no record -- only where pe_encode also gives 0;
 *   status 2: declined -- the caller hands the location to pe_encode (and what that declines to the Python encoder).
 * Declined: two tracks with the same name:sequence hash, a reference skip or an '=' base in a track, a track whose SEQ
 * holds fewer bases than its CIGAR's query length (SEQ '*'), a zero-length alignment inside the window (a read such as
 * 0M 5I: a reference-consuming operation, no reference position; pe_encode declines it too, and the Python builder raises
 * ValueError), a base of the reference outside the token table, more than PG_MAX_TRACKS tracks,
 * window_size > PG_MAX_WINDOW, min_base_quality > 0, a contig missing from the FASTA, a position below 1, a BAM that is not
 * coordinate-sorted within a run.  A record whose CIGAR spans more than 2^29 reference bases is a corrupt-BAM error.
 *
 * Every call returns 0 on success and a negative code on failure; pg_last_error() then says why.  No call aborts the process
 * on bad input: a corrupt BAM is an error code. */
#ifndef DL4VC_PILEUP_GPU_H
#define DL4VC_PILEUP_GPU_H

#include <stdint.h>

#include "dl4vc_loader.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_MAX_TRACKS 1024   /* tracks one location may hold on the GPU */
#define PG_MAX_WINDOW 100    /* largest window_size the GPU plan holds */

typedef struct pg_encoder pg_encoder_t;

int pg_open(const char* bam_path, const char* bai_path /* NULL: <bam>.bai, <stem>.bai, else a linear scan */,
            const char* fasta_path, const pe_options* opt, int32_t device, pg_encoder_t** out);
/* Host outputs, laid out as pe_encode's: reads / qual / strand [n][max_reads][2 w + 1], ref [n][2 w + 1]. */
int pg_encode(pg_encoder_t* h, const char* const* contigs, const int32_t* positions, int64_t n, uint8_t* reads_out,
              uint8_t* qual_out, uint8_t* strand_out, uint8_t* ref_out, int32_t* num_reads_out, int8_t* status_out);
/* The same, except that reads / qual / strand are DEVICE pointers ([n][max_reads][2 w + 1] each, on the encoder's device).
 * They are written after the work already enqueued on `stream` (a hipStream_t, NULL = the default stream), and the call
 * returns once they are written.  Every slot is written: zeros where the status is not 1. */
int pg_encode_device(pg_encoder_t* h, const char* const* contigs, const int32_t* positions, int64_t n, uint8_t* reads_dev,
                     uint8_t* qual_dev, uint8_t* strand_dev, uint8_t* ref_out, int32_t* num_reads_out, int8_t* status_out,
                     void* stream);
/* Site assembly on the device: the stored planes pg_encode_device wrote -> the six planes dan_forward_device reads
 * (include/dl4vc_dan.h), compacted over the m locations that gave a record.
 *   reads_src / qual_src / strand_src: DEVICE, [n_slots][stored_rows][window] (stored_rows = the encoder's max_reads);
 *   slots [m]: HOST, the location slot each output site comes from;
 *   rows [m][reads]: HOST int16, the stored rows of each output site in output order (NULL: every site takes rows
 *     0..reads-1); first_rows [m]: HOST, may be NULL; != 0 marks a site that takes rows 0..reads-1 (its rows are not read);
 *   ref / ref_mask / var_mask [m][window]: HOST;
 *   outputs: DEVICE, reads_out / qual_out / strand_out [m][reads][window], ref_out / ref_mask_out / var_mask_out [m][window];
 *     qual_out / strand_out are zero-filled when use_q / use_strand is 0.
 * Slots and rows are range-checked on the host before anything is enqueued.  The host arrays are free again on return; the
 * copies and the kernel are enqueued on `stream` (a hipStream_t, NULL = the default stream) behind the work already there, and
 * the call returns without waiting for them: the caller synchronises, or enqueues dan_forward_device on the same stream. */
int pg_assemble_device(pg_encoder_t* h, const uint8_t* reads_src, const uint8_t* qual_src, const uint8_t* strand_src,
                       int64_t n_slots, int32_t stored_rows, int32_t window, const int32_t* slots, const int16_t* rows,
                       const uint8_t* first_rows, int64_t m, int32_t reads, const uint8_t* ref, const uint8_t* ref_mask,
                       const uint8_t* var_mask, int32_t use_q, int32_t use_strand, uint8_t* reads_out, uint8_t* qual_out,
                       uint8_t* strand_out, uint8_t* ref_out, uint8_t* ref_mask_out, uint8_t* var_mask_out, void* stream);
void pg_close(pg_encoder_t* h);
const char* pg_last_error(const pg_encoder_t* h);      /* h may be NULL: error of the last failed pg_open */

#ifdef __cplusplus
}
#endif
#endif
