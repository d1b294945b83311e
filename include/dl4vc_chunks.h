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

/* ---- the record store: a file's records inflated once and kept in device memory ---------------------------------------------------
 * A stored record is its three planes trimmed of their trailing all-zero rows: reads[kept][window] | qual[kept][window] |
 * strand[kept][window] and zero bytes up to the next multiple of 16, where kept = 1 + the last stored row that holds a non-zero
 * byte in ANY of the three planes (0: none does).  The trimming is by the bytes, not by num_reads: rows >= kept are all-zero by
 * definition and the assembly writes them as zeros, so what is assembled from the store equals what cl_assemble_device makes of
 * the inflated records, byte for byte, for any file.  Records lie in the order they are appended, each at a 16-byte boundary of
 * a slab; a record that does not fit what is left of the last slab opens the next (none straddles two), a record without rows
 * takes no byte (slab 0, offset 0).  A slab holds slab_bytes, or what capacity_bytes leaves when that is less.  capacity_bytes
 * bounds the sum of the stored records' bytes, NOT the allocations: a slab is allocated whole, so the device memory a store takes
 * exceeds its records' bytes by the unused part of its slabs (less than one slab when the records are many; 272 bytes of guard and
 * pad per slab besides).  One thread at a time uses a handle.
 *
 * The compact format (cl_store_set_format(h, 1), windows of at most 255 columns) stores the same record in fewer bytes and
 * assembles the same planes byte for byte.  For stored row r < kept, [c0_r, c0_r + n_r) is the smallest column range that contains
 * every non-zero byte of the three planes in that row (n_r = 0, c0_r = 0 for an all-zero row below kept).  A compact record is
 *   rowtab[kept + 1]  little-endian uint32: bits 0-23 off_r = the cells of rows < r, bits 24-31 c0_r (0 in the last entry, whose
 *                     off is the record's cells)
 *   ts[cells]         token | strand << 4 of every cell, row by row
 *   q[cells]          the quality byte of every cell
 * and zeros up to the next multiple of 16: pad16(4 (kept + 1) + 2 cells) bytes, none for kept = 0.  A record with any byte >= 16
 * in its reads or strand plane is stored in the rows layout above inside the same store; cl_store_record_span names the format
 * of a record.  dl4vc_amd/csrc/store_host.h holds the definition the kernels are tested against. */
typedef struct cl_store cl_store_t;

/* n_records: the records the store may come to hold (the table's size).  slab_bytes: a multiple of 16.  device < 0: the slabs lie
 * in host memory and the store takes cl_store_pack_host / cl_store_assemble_host (the CPU definitions) instead of the device
 * entries. */
int cl_store_open(int32_t window, int32_t stored_rows, int64_t n_records, uint64_t capacity_bytes, uint64_t slab_bytes, int32_t device,
                  cl_store_t** out);
void cl_store_close(cl_store_t* h);
const char* cl_store_last_error(const cl_store_t* h);   /* h == NULL: the error of a failed cl_store_open or of cl_store_extent_host */
/* The format records appended from now on are stored in: 0 = rows (the default), 1 = compact.  Refused (-1, with the reason) once
 * the store holds a record, for any other value, and for the compact format on a store whose window exceeds 255 columns. */
int cl_store_set_format(cl_store_t* h, int32_t format);

/* Record slots[i] of the loader's last cl_inflate_chunks_device call becomes record records[i] of the store (not in it yet, named
 * once): the extents are measured on the device (kept_out[i], host memory), the records laid out on the host and packed on the
 * device.  Enqueued on `stream` and waited for: the loader's record buffer is free again when the call returns.  Returns -3,
 * with kept_out filled and the store unchanged, when capacity_bytes would be exceeded; any other failure leaves it unchanged too. */
int cl_store_append_device(cl_store_t* h, cl_loader_t* loader, const int32_t* slots, const int32_t* records, int64_t n, void* stream,
                           int32_t* kept_out);

/* cl_store_append_device with the pileup encoder's output as the source (pg_encode_device's status-1 planes, or any planes of that
 * layout): three device arrays [n_slots][stored_rows][window], read only, not necessarily aligned; slot slots[i] (range-checked
 * against n_slots before anything is enqueued) becomes record records[i].  Same kernels, same contract: extents on the device,
 * layout on the host, packed on the device, waited for; -3 with the store unchanged when capacity_bytes would be exceeded.
 * cl_store_get_stats counts 3 * stored_rows * window inflated bytes per record.  n_records of cl_store_open is an upper bound:
 * a caller that stores only the locations that gave a record opens the store for the number of locations. */
int cl_store_append_planes_device(cl_store_t* h, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots,
                                  const int32_t* slots, const int32_t* records, int64_t n, void* stream, int32_t* kept_out);

/* cl_assemble_device's contract with the store's records as the source: site i takes rows[i] (or the first `reads` rows) of record
 * records[i]; a row >= kept is zeros.  Records and rows are range-checked before anything is enqueued.  The six outputs are
 * device pointers; asynchronous on `stream`. */
int cl_store_assemble_device(cl_store_t* h, const int32_t* records, const int16_t* rows, const uint8_t* first_rows, int64_t m, int32_t reads,
                             const uint8_t* ref, const uint8_t* ref_mask, const uint8_t* var_mask, int32_t use_q, int32_t use_strand,
                             uint8_t* reads_out, uint8_t* qual_out, uint8_t* strand_out, uint8_t* ref_out, uint8_t* ref_mask_out,
                             uint8_t* var_mask_out, void* stream);
/* cl_center_counts_device (same kernel, same contract) for a caller that holds a store and no loader any more: the resident loader
 * closes its cl_loader after the fill, and cl_center_counts_device needs one. */
int cl_store_center_counts_device(cl_store_t* h, const uint8_t* reads, int64_t m, int32_t rows, int32_t window, int32_t* counts, void* stream);

/* The CPU definitions, all pointers host pointers.  inflated: records of record_bytes, inflated_bytes of them in all (slots are
 * checked against it), the planes [stored_rows][window] at plane_off[0..2] of each.  cl_store_extent_host: kept_out[i] = the
 * extent of record slots[i].  cl_store_pack_host: cl_store_append_device on a host store.  cl_store_assemble_host:
 * cl_store_assemble_device on a host store, same arguments (stream is ignored). */
int cl_store_extent_host(const uint8_t* inflated, uint64_t inflated_bytes, int64_t record_bytes, const int64_t* plane_off, int32_t stored_rows,
                         int32_t window, const int32_t* slots, int64_t n, int32_t* kept_out);
int cl_store_pack_host(cl_store_t* h, const uint8_t* inflated, uint64_t inflated_bytes, int64_t record_bytes, const int64_t* plane_off,
                       const int32_t* slots, const int32_t* records, int64_t n, int32_t* kept_out);
/* cl_store_extent_host / cl_store_pack_host for three host arrays [n_slots][stored_rows][window]: the CPU definitions of
 * cl_store_append_planes_device. */
int cl_store_extent_planes_host(const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots, int32_t stored_rows,
                                int32_t window, const int32_t* slots, int64_t n, int32_t* kept_out);
int cl_store_pack_planes_host(cl_store_t* h, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots,
                              const int32_t* slots, const int32_t* records, int64_t n, int32_t* kept_out);
int cl_store_assemble_host(cl_store_t* h, const int32_t* records, const int16_t* rows, const uint8_t* first_rows, int64_t m, int32_t reads,
                           const uint8_t* ref, const uint8_t* ref_mask, const uint8_t* var_mask, int32_t use_q, int32_t use_strand,
                           uint8_t* reads_out, uint8_t* qual_out, uint8_t* strand_out, uint8_t* ref_out, uint8_t* ref_mask_out,
                           uint8_t* var_mask_out, void* stream);
/* The CPU definition of the compact format's spans (window <= 255), for inflated records and for three host arrays as above:
 * kept_out[i], cells_out[i] (the sum of the rows' n), mergeable_out[i] (1: no byte >= 16 in the reads or strand plane) and
 * rowspans_out[i * stored_rows + r] = c0_r | n_r << 8 for every stored row r of record slots[i]. */
int cl_store_spans_host(const uint8_t* inflated, uint64_t inflated_bytes, int64_t record_bytes, const int64_t* plane_off, int32_t stored_rows,
                        int32_t window, const int32_t* slots, int64_t n, int32_t* kept_out, int32_t* cells_out, int32_t* mergeable_out,
                        uint16_t* rowspans_out);
int cl_store_spans_planes_host(const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots, int32_t stored_rows,
                               int32_t window, const int32_t* slots, int64_t n, int32_t* kept_out, int32_t* cells_out, int32_t* mergeable_out,
                               uint16_t* rowspans_out);

/* ---- test and debug entries: what the tests need to see of a store; no loader or command-line path calls them ------------------- */
/* Where a record lies: for a device store read from the table in device memory that the kernels follow. */
int cl_store_record(cl_store_t* h, int64_t record, int32_t* slab, int64_t* offset, int32_t* kept);
/* The format a record is stored in (0 rows, 1 compact; for a device store as the table in device memory has it) and the bytes it
 * takes in its slab. */
int cl_store_record_span(cl_store_t* h, int64_t record, int32_t* format, int64_t* bytes);
/* A slab's sizes, and with dst != NULL a copy of its whole allocation (host memory): the slab's `capacity` bytes begin data_off
 * bytes in (a device slab has 256 bytes that are never written in front of them and 16 behind, so that a 16-byte load at a
 * record's last bytes stays inside the allocation), the first `used` of them hold records. */
int cl_store_slab(cl_store_t* h, int32_t slab, uint8_t* dst, uint64_t dst_bytes, int64_t* data_off, int64_t* used, int64_t* capacity);
/* Debug only (it adds a fill to every slab allocation): every slab allocated from now on is filled with `value` (0..255; -1: not
 * filled, the default) before records are packed into it: what a test needs to see that no byte outside the records is written. */
int cl_store_debug_fill(cl_store_t* h, int32_t value);

typedef struct {
    int64_t records;             /* in the store */
    int64_t stored_bytes;        /* the sum of their bytes in the slabs */
    int64_t inflated_bytes;      /* the bytes of the inflated records they replace */
    int64_t slabs;
    int64_t refused_fit_records; /* of the last append the capacity refused (-3): how many of its records would have fit, */
    int64_t refused_fit_bytes;   /* and the bytes the store would hold with them (0 / 0: no append was refused) */
    double extent_ms, pack_ms;   /* record_extent / store_pack of all appends, device time */
    double assemble_ms;          /* the last cl_store_assemble_device (cl_store_get_stats waits for it) */
} cl_store_stats;
int cl_store_get_stats(cl_store_t* h, cl_store_stats* out);

typedef struct {
    int64_t format;              /* what cl_store_set_format chose */
    int64_t rows_records;        /* records stored in the rows layout (all of a rows store; of a compact store, those that fell back) */
    int64_t rows_bytes;          /* and the sum of their bytes in the slabs */
    int64_t compact_records;     /* records stored in the compact format */
    int64_t compact_bytes;
    double spans_ms;             /* record_spans of all appends of a compact store, device time (its extent_ms stays 0) */
} cl_store_format_stats;
int cl_store_get_format_stats(cl_store_t* h, cl_store_format_stats* out);

#ifdef __cplusplus
}
#endif
#endif
