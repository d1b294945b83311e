/* zlib stream inflate of libdl4vc_pileup.so: whole zlib streams (RFC 1950: a 2-byte header, a raw DEFLATE body, a big-endian
 * Adler-32) of any length up to ZI_MAX_OUTPUT, as the deflate filter of HDF5 writes one per chunk -- on the GPU (one workgroup
 * per stream) or on the host with the same text (dl4vc_amd/csrc/zinflate.h over the decode core of bgzf_inflate.h).  The output
 * passes through a 64 KiB ring, so a stream is not bound to the 65 536 bytes of a BGZF block.  Bindings: dl4vc_amd/zinflate.py.
 *
 * A damaged stream is a status, never an abort: no input makes the decoder read outside [stream, stream + len), write outside the
 * stream's slot out[out_off, out_off + out_len), or loop without consuming input or producing output.  Unlike bz_inflate, a
 * stream that fails has already written the halves of the ring it completed: a failed slot's content is unspecified (but no byte
 * outside it is touched). */
#ifndef DL4VC_CHUNKS_H
#define DL4VC_CHUNKS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-stream status.  0..12 are the BZ_* codes of dl4vc_bgzf.h with the same numbers and causes (ISIZE = the expected length). */
#define ZI_OK 0
#define ZI_BAD_BLOCK_TYPE 1
#define ZI_BAD_STORED_LEN 2
#define ZI_BAD_CODE_LENGTHS 3
#define ZI_BAD_SYMBOL 4
#define ZI_DISTANCE_BEFORE_START 5
#define ZI_OUTPUT_EXCEEDS_LENGTH 6  /* the stream holds more than out_len bytes */
#define ZI_OUTPUT_SHORT_OF_LENGTH 7 /* the stream ends before out_len bytes */
#define ZI_INPUT_EXHAUSTED 8
#define ZI_TRAILING_INPUT 9         /* the final DEFLATE block ends before the body does */
#define ZI_BAD_SLOT 12              /* out_off + out_len exceeds out_cap, or out_len > ZI_MAX_OUTPUT */
#define ZI_BAD_ZLIB_HEADER 13       /* CM != 8, CINFO > 7, FCHECK wrong, or a preset dictionary (FDICT) */
#define ZI_ADLER_MISMATCH 14
#define ZI_RAW_SIZE_MISMATCH 15     /* a raw (not deflated) chunk whose length is not out_len */
#define ZI_BAD_RANGE 16             /* off + len exceeds nbytes, or len >= 2^32 */

#define ZI_MAX_OUTPUT 1073741824    /* bytes of one stream's output (2^30) */

/* Inflates n streams: stream i is streams[off[i], off[i] + len[i]) and must hold exactly out_len[i] bytes, which go to
 * out + out_off[i]; status[i] says how it ended.  Where raw[i] is non-zero (raw may be NULL: none is) the bytes are not a zlib
 * stream but the chunk itself -- what an HDF5 filter mask that skips the deflate filter means -- and are copied.  All pointers
 * are host pointers.  Bytes of out outside the slots are left as they were; the slots must not overlap.  Returns 0 when the call
 * itself ran (look at status[]), a negative code otherwise (zi_last_error()). */
int zi_inflate(const uint8_t* streams, uint64_t nbytes, const uint64_t* off, const uint64_t* len, int64_t n, uint8_t* out,
               uint64_t out_cap, const uint64_t* out_off, const uint64_t* out_len, const uint8_t* raw, int32_t* status, int device);
/* The same on the CPU: one thread runs the text of the kernel, ring included. */
int zi_inflate_host(const uint8_t* streams, uint64_t nbytes, const uint64_t* off, const uint64_t* len, int64_t n, uint8_t* out,
                    uint64_t out_cap, const uint64_t* out_off, const uint64_t* out_len, const uint8_t* raw, int32_t* status);
const char* zi_status_text(int status);
const char* zi_last_error(void);

/* ---- the candidate file's chunks inflated and its sites assembled on the device -------------------------------------------------
 * A loader handle owns a device buffer of inflated records [record][record_bytes] (the packed compound of
 * dl4vc_amd/hdf5_schema.py: the members in front of the reads plane, the reads plane, the members between it and the quality
 * plane, the quality plane, the strand plane -- cl_open refuses any other arrangement) and the pinned host copies of what the
 * host needs of them.  The caller reads the file's raw chunks (H5Dread_chunk), the handle does the rest; the planes never reach
 * the host. */
typedef struct cl_loader cl_loader_t;

/* max_records: the most records one cl_inflate_chunks_device call covers (whole chunks: a range that is not chunk-aligned takes
 * one chunk more, which cl_open allows for).  plane_off: byte offsets of the reads, quality and strand planes in a record. */
int cl_open(int64_t record_bytes, int32_t chunk_records, int32_t window, int32_t stored_rows, const int64_t* plane_off,
            int64_t max_records, int32_t device, cl_loader_t** out);
void cl_close(cl_loader_t* h);
const char* cl_last_error(const cl_loader_t* h);   /* h == NULL: the error of a failed cl_open */

/* Chunk c is comp[off[c], off[c] + len[c]) (host memory, best pinned): a zlib stream of chunk_records * record_bytes bytes, or
 * with raw[c] those bytes themselves.  Uploads them, inflates them into the handle's record buffer (record c * chunk_records + k
 * is record k of chunk c), copies every record's non-plane members back -- blob_bytes = record_bytes - 3 * stored_rows * window
 * per record, in the record's order -- and the per-chunk status (ZI_*) into status[].  *blob points at the handle's pinned copy,
 * valid until the next call.  Everything is enqueued on `stream` (a hipStream_t, NULL = the default stream) and waited for.
 * Returns 0 when the call ran (look at status[]), a negative code otherwise. */
int cl_inflate_chunks_device(cl_loader_t* h, const uint8_t* comp, uint64_t nbytes, const uint64_t* off, const uint64_t* len,
                             const uint8_t* raw, int64_t n_chunks, void* stream, const uint8_t** blob, int32_t* status);

/* pg_assemble_device's contract (dl4vc_pileup_gpu.h) with the records of the last cl_inflate_chunks_device call as the slots:
 * site i takes rows[i] (or the first `reads` rows) of record slots[i].  Slots and rows are range-checked before anything is
 * enqueued.  The six outputs are device pointers; asynchronous on `stream`. */
int cl_assemble_device(cl_loader_t* h, const int32_t* slots, const int16_t* rows, const uint8_t* first_rows, int64_t m, int32_t reads,
                       const uint8_t* ref, const uint8_t* ref_mask, const uint8_t* var_mask, int32_t use_q, int32_t use_strand,
                       uint8_t* reads_out, uint8_t* qual_out, uint8_t* strand_out, uint8_t* ref_out, uint8_t* ref_mask_out,
                       uint8_t* var_mask_out, void* stream);

/* The read tokens at the two columns the training targets count ((window - 1) / 2 and the column after it: 100 and 101 of the
 * 201-column window) in an assembled reads plane reads[m][rows][window], a device pointer -- cl_assemble_device's reads_out:
 * counts[i][k][t] (int32 [m][2][16], a device pointer) = rows of site i whose byte at column (window - 1) / 2 + k is t.  Bytes above 15
 * are not counted.  One wave per site, no global atomics; every element of counts[m][2][16] is written once and nothing else is.
 * Asynchronous on `stream`. */
int cl_center_counts_device(cl_loader_t* h, const uint8_t* reads, int64_t m, int32_t rows, int32_t window, int32_t* counts, void* stream);
/* Its definition on the CPU, same arguments with host pointers: h may be NULL (it only receives the error text), stream is ignored. */
int cl_center_counts_host(cl_loader_t* h, const uint8_t* reads, int64_t m, int32_t rows, int32_t window, int32_t* counts, void* stream);

/* The last cl_inflate_chunks_device call and the last cl_assemble_device call since: device time between events on the caller's
 * stream, in ms.  (cl_get_stats waits for that assembly.) */
typedef struct {
    double upload_ms;            /* chunk bytes and their table, host -> device */
    double inflate_ms;           /* zi_inflate_kernel */
    double blob_copy_back_ms;    /* the non-plane members and the statuses, device -> host */
    double assemble_ms;          /* assemble_planes and the copies of its tables */
    int64_t chunks, compressed_bytes, inflated_bytes, raw_chunks;
} cl_stats;
int cl_get_stats(cl_loader_t* h, cl_stats* out);

#ifdef __cplusplus
}
#endif
#endif
