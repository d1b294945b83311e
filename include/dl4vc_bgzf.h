/* BGZF block inflate of libdl4vc_cand.so: raw DEFLATE (RFC 1951) of whole BGZF blocks, on the GPU (one workgroup per
 * block) or on the host with the same decode core (dl4vc_amd/csrc/bgzf_inflate.h).  Bindings: dl4vc_amd/candgen.py::inflate_blocks.
 *
 * A damaged block is a status, never an abort: no input makes the decoder read outside the block's body, write outside the
 * block's slot out[out_off, out_off + ISIZE), or loop without consuming input or producing output. */
#ifndef DL4VC_BGZF_H
#define DL4VC_BGZF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-block status. */
#define BZ_OK 0
#define BZ_BAD_BLOCK_TYPE 1      /* BTYPE 3 */
#define BZ_BAD_STORED_LEN 2      /* LEN / NLEN mismatch of a stored block */
#define BZ_BAD_CODE_LENGTHS 3    /* over-subscribed or unusable code lengths (an incomplete set only for a single code of length 1) */
#define BZ_BAD_SYMBOL 4          /* literal/length symbol 286 / 287, distance symbol 30 / 31, or a code outside an incomplete set */
#define BZ_DISTANCE_BEFORE_START 5 /* a match reaches before the start of the block's output */
#define BZ_OUTPUT_EXCEEDS_ISIZE 6
#define BZ_OUTPUT_SHORT_OF_ISIZE 7
#define BZ_INPUT_EXHAUSTED 8
#define BZ_TRAILING_INPUT 9      /* the final DEFLATE block ends before the body does */
#define BZ_CRC_MISMATCH 10
#define BZ_BAD_HEADER 11         /* not a BGZF block: magic, BC field, body < 8 bytes, ISIZE > 65536, or it runs past the input */
#define BZ_BAD_SLOT 12           /* out_off + ISIZE exceeds out_cap */

/* Inflates n_blocks whole BGZF blocks (18-byte header and 8-byte trailer included) that start at blocks + block_off[i]; block i's
 * bytes go to out + out_off[i] and status[i] says how it ended.  All pointers are host pointers.  Bytes of out outside the
 * slots are left as they were; a failed block's slot is left untouched by the device path and holds what was decoded before the
 * fault on the host path.  Returns 0 when the call itself ran (look at status[]), a negative code otherwise (bz_last_error()). */
int bz_inflate(const uint8_t* blocks, uint64_t nbytes, const uint64_t* block_off, int64_t n_blocks, uint8_t* out,
               uint64_t out_cap, const uint64_t* out_off, int32_t* status, int device);
/* The same on the CPU. */
int bz_inflate_host(const uint8_t* blocks, uint64_t nbytes, const uint64_t* block_off, int64_t n_blocks, uint8_t* out,
                    uint64_t out_cap, const uint64_t* out_off, int32_t* status);
const char* bz_status_text(int status);
const char* bz_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
