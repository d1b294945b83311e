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
/* The record census: for n locations exactly the statuses pg_encode_device would return (0 no record, 1 record, 2 declined),
 * by the same status rule (csrc/pileup_kernels.hip::location_status, which both kernels call) over the same fetched and framed
 * records, with pg_set_inflate_device off or on.  No plane, reference line or read count is written anywhere: status_out
 * [n] is the only output (HOST).  The rule's last step needs every record's resolved CIGAR, so the resolve kernel runs as in
 * an encode call.  `stream` as above.  pg_get_stats then gives the call's stages, with census_ms in place of encode_ms. */
int pg_census(pg_encoder_t* h, const char* const* contigs, const int32_t* positions, int64_t n, int8_t* status_out, void* stream);
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
/* ---- records inflated and framed on the device ------------------------------------------------------------------------------
 * With pg_set_inflate_device(h, 1, budget) the host threads above do no per-record work.  Each call builds the same runs of
 * locations, takes every run's byte ranges from the BAI bins, reads the BGZF blocks they touch as they are into pinned memory
 * and uploads them; the device inflates them (a group of runs at a time, at most `max_inflated_bytes` of inflated data per
 * group, 0 = 256 MB; one run larger than that is a group of its own), walks the record chain, frames every record with the
 * checks of the host path, lists it once for each run it belongs to (run-major, file order within a run) and finds every
 * location's records.  The encode kernels then read the records where they lie in the inflated buffer.  The host still reads
 * the index, the file and the reference tokens.  Outputs are byte-identical to the encoder with the option off.
 * Refused (an error, pg_last_error(h) says why): an encoder without the bins of a .bai (opened without one: the scan builds
 * only the linear index), and, at encode time, a BGZF block with ISIZE > 65536.  A block that two byte ranges touch is
 * inflated once for each.  A damaged block is "BGZF block fails its CRC / size check (<status>, block at file offset N)"; a
 * refused record is the host path's text with "(record at virtual offset N)".  on = 0 restores the host path. */
int pg_set_inflate_device(pg_encoder_t* h, int on, uint64_t max_inflated_bytes /* 0: default */);

/* Stages of the last pg_encode / pg_encode_device / pg_census call, times in ms.  With the option off only host_frame_ms, upload_ms,
 * encode_ms, copy_back_ms, host_records and records are filled.  upload_ms, inflate_ms, frame_ms and encode_ms are device time
 * between events on the encoder's stream, on both paths; host_frame_ms, read_ms and copy_back_ms are host wall clock (copy_back_ms
 * around blocking copies). */
typedef struct {
    double host_frame_ms;     /* wall time of the fetch threads, plus the gather */
    double read_ms;           /* index ranges, pread into pinned memory, header and trailer checks */
    double upload_ms;         /* host -> device copies (records or blocks, locations, reference tokens) */
    double inflate_ms;        /* device events around the inflate kernel */
    double frame_ms;          /* walk, frame, scans, emit and location search */
    double encode_ms;         /* resolve_records and encode_locations */
    double copy_back_ms;      /* planes back to the host (pg_encode only) */
    double census_ms;         /* pg_census only: resolve_records and census_locations (device events; encode_ms stays 0) */
    int64_t host_records;     /* records framed on the host; 0 on the device path */
    int64_t blocks, compressed_bytes, inflated_bytes;
    int64_t records;          /* records listed for the runs (a record shared by two runs counts twice) */
    int64_t groups;
    /* the last pg_compress_records_device call (device time between events on the caller's stream; an encode call clears them) */
    double pack_ms;           /* blob and slot upload, hdf_pack_kernel */
    double deflate_ms;        /* zd_deflate_kernel or zd_deflate_dyn_kernel */
    double gather_ms;         /* stream sizes, their scan, zd_gather_kernel */
    double compress_copy_back_ms;   /* the chunks' bytes and their table to the host */
    int64_t chunks, raw_bytes, chunk_bytes_out, stored_chunks;
    /* segments of those chunks by what they were written as; counted with pg_set_compress_codes(h, 1) only (0 otherwise) */
    int64_t fixed_segments, dynamic_segments, stored_segments;
} pg_stats;
int pg_get_stats(const pg_encoder_t* h, pg_stats* out);

/* Read subsampling by name hash (the rule of cg_set_subsample in dl4vc_candgen.h, one definition in csrc/bam_frame.h).  A record
 * is framed and checked as without the option and then dropped where a record outside its run is dropped: by the host framing
 * threads, or in the device's frame kernel with pg_set_inflate_device.  Everything behind sees the kept reads alone: coverage,
 * track selection, duplicate keys, the track limit, the stored rows.  Holds for pg_encode, pg_encode_device and pg_census.
 * fraction 0: off; outside [0, 1] or NaN: refused. */
int pg_set_subsample(pg_encoder_t* h, double fraction, uint32_t seed);
/* Of the last encode / census call: records that passed the run's region test (once per run they belong to) and those kept. */
typedef struct {
    int64_t records_seen;
    int64_t records_kept;
} pg_subsample_stats;
int pg_get_subsample_stats(const pg_encoder_t* h, pg_subsample_stats* out);
/* Read filter by flags and mapping quality (the rule of `samtools view -F exclude -f require -q min_mapq`, one definition in
 * csrc/bam_frame.h; pe_set_read_filter in dl4vc_loader.h states it).  A record is framed and checked as without the option, then
 * dropped where a record outside its run is dropped, in front of the sample rule, by the host framing threads or in the device's
 * frame kernel.  Everything behind sees the kept reads alone; the encoder's fixed mask 0x704 stays where it is.  Holds for
 * pg_encode, pg_encode_device and pg_census; pg_subsample_stats.records_seen then counts what passed region and filter.
 * pg_set_read_stats(h, 1): the read census (dl4vc_read_stats) of a call is collected without a filter too, once per run a record
 * belongs to; on the device a workgroup counts in LDS and adds to one small array with integer atomics. */
int pg_set_read_filter(pg_encoder_t* h, int32_t exclude, int32_t require, int32_t min_mapq);
int pg_set_read_stats(pg_encoder_t* h, int on);
int pg_get_read_stats(const pg_encoder_t* h, dl4vc_read_stats* out);

/* ---- candidate HDF5 chunks compressed on the device ---------------------------------------------------------------------------
 * The zlib compressor (csrc/zdeflate.h): an RFC 1950 stream of DEFLATE blocks (fixed codes, or with ZD_DYNAMIC the smaller of a
 * fixed and a dynamic block per segment), the input cut into segments of `segment` bytes (ZD_MIN_SEGMENT..ZD_MAX_SEGMENT) that are
 * compressed on their own and joined byte-aligned, so the bytes depend on the input, the segment size and the mode alone.  zlib's inflate (and so HDF5's deflate filter) reads it.  A stream that is not smaller
 * than its input is flagged "store": it is still a valid stream within zd_bound, and the writer of an HDF5 chunk passes the raw
 * bytes with filter mask 1 instead.  Errors: the text pg_last_error(NULL) returns. */
#define ZD_MIN_SEGMENT 1024
#define ZD_MAX_SEGMENT 32768
#define ZD_DEFAULT_SEGMENT 16384
#define ZD_REVERSED 1        /* zd_deflate: the kernel takes the segments in the opposite launch order (same bytes) */
#define ZD_RAW_ON_STORE 2    /* zd_deflate: a "store" chunk's output is its raw bytes (size = chunk_bytes), not its stream */
#define ZD_DYNAMIC 4         /* dynamic codes: a segment is parsed twice, first to count its symbols; it is written as a dynamic
                              * block where that is smaller than the fixed one, so no stream is larger than without the flag */
int zd_bound(uint64_t n, uint32_t segment, uint64_t* bound);      /* n <= 2^31; no stream of n bytes is longer */
/* CPU twin: the same text, the segments one after the other.  out_cap >= zd_bound. */
int zd_deflate_host(const uint8_t* in, uint64_t n, uint32_t segment, uint8_t* out, uint64_t out_cap, uint64_t* size, uint32_t* adler,
                    int32_t* store);
/* The same with flags: 0 (zd_deflate_host's bytes) or ZD_DYNAMIC. */
int zd_deflate_host_flags(const uint8_t* in, uint64_t n, uint32_t segment, int32_t flags, uint8_t* out, uint64_t out_cap, uint64_t* size,
                          uint32_t* adler, int32_t* store);
/* The compressor's code construction on its own (a test entry): counts freq[n] (n 2..286, their sum <= 65535) -> code lengths
 * lens[n] of at most `limit` bits (1..15, 2^limit >= n): optimal where the Huffman code's depth fits the limit, Kraft sum 1; two
 * codes of length 1 where fewer than two symbols occur. */
int zd_code_lengths_host(const uint32_t* freq, int32_t n, int32_t limit, uint8_t* lens);
/* n_chunks (1..65535) streams, one per chunk of chunk_bytes of in_dev (DEVICE), written one behind the other into out_dev (DEVICE,
 * out_cap >= n_chunks * zd_bound; nothing but the streams' own bytes is written).  offsets / sizes / adlers / store [n_chunks]: HOST.
 * Runs on `stream` (a hipStream_t, NULL = the default stream) and returns when the streams are written. */
int zd_deflate(const uint8_t* in_dev, uint64_t chunk_bytes, int64_t n_chunks, uint32_t segment, int32_t flags, uint8_t* out_dev,
               uint64_t out_cap, uint64_t* offsets, uint64_t* sizes, uint32_t* adlers, uint8_t* store, void* stream);
/* n_records candidate records -> the chunks of the HDF5 dataset, compressed.  Record i is packed on the device in the layout of
 * dl4vc_amd/hdf5_schema.py (packed compound, window = the encoder's 2 w + 1, max_reads stored rows) from
 *   the stored planes at slot slots[i] (HOST int32, each in [0, n_slots)) of reads_dev / qual_dev / strand_dev
 *     (DEVICE [n_slots][max_reads][window], what pg_encode_device wrote), and
 *   blob[i] (HOST, blob_bytes = 149 + 16 * window each): the record's other members as the schema lays them out, the three
 *     planes left out -- name, ref, reads | ref_bases, num_reads, label, vcfrec.
 * Chunk c holds records [c * records_per_chunk, ...); the last chunk is padded with zero bytes to the full records_per_chunk
 * (HDF5 stores edge chunks at full size).  Every chunk is compressed with ZD_DEFAULT_SEGMENT; *out (HOST, pinned, the encoder's
 * own: valid until the next call or pg_close) holds chunk c's bytes at offsets[c], sizes[c] of them: its zlib stream, or, where
 * store[c] != 0, its raw bytes (H5Dwrite_chunk with filter mask 1).  offsets / sizes / adlers / store: HOST
 * [ceil(n_records / records_per_chunk)].  Runs behind the work already enqueued on `stream` (a hipStream_t, NULL = the default
 * stream), on it, and returns when the bytes are on the host. */
int pg_compress_records_device(pg_encoder_t* h, const uint8_t* reads_dev, const uint8_t* qual_dev, const uint8_t* strand_dev,
                               int64_t n_slots, const int32_t* slots, const uint8_t* blob, int64_t n_records,
                               int32_t records_per_chunk, const uint8_t** out, uint64_t* offsets, uint64_t* sizes, uint32_t* adlers,
                               uint8_t* store, void* stream);

/* The codes pg_compress_records_device compresses with: 0 = fixed (the default), 1 = dynamic (ZD_DYNAMIC).  No chunk is larger
 * with 1 than with 0. */
int pg_set_compress_codes(pg_encoder_t* h, int mode);

/* Test hook, no device call: the framed records of the run [s0, stop) of contig `tid`, by the host path (path 0) or by the
 * CPU twin of the device path (path 1: index ranges, the host form of the inflate, the shared frame core, serially; path 2:
 * the same, with the run's blocks taken from the plan of a larger call).
 * Every field of a record but its hash; bytes_hash stands for `off`: FNV-1a 64 of the bytes it points at (up to the end of
 * the qualities).  *n = records of the run (the first `cap` are written).  Errors: pg_last_error(NULL). */
typedef struct {
    int32_t pos, end, res, l_seq;
    uint32_t cigar_off, seq_off, qual_off, n_cig, l_name, bits;
    uint64_t bytes_hash;
} pg_rec_view;
int pg_debug_run_records(const char* bam, const char* bai, int32_t tid, int64_t s0, int64_t stop,
                         int path /* 0: fetch_run, 1: index ranges + bz_inflate_host + the shared frame core, serially;
                                     2: as 1, inside a call that also asks for [0, 64) of the contig: the blocks are read for
                                     the call's plan and the run takes its own from it, as a group of runs does */,
                         pg_rec_view* out, int64_t cap, int64_t* n, int64_t* max_nref, int32_t* sorted);

void pg_close(pg_encoder_t* h);
const char* pg_last_error(const pg_encoder_t* h);      /* h may be NULL: error of the last failed pg_open */

#ifdef __cplusplus
}
#endif
#endif
