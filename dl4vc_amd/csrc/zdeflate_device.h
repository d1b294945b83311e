// Shared between the host side (zdeflate_capi.cpp, pileup_capi.cpp) and the kernels (zdeflate_kernels.hip) of the device
// compressor of libdl4vc_pileup.so; the encode core itself is zdeflate.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "zdeflate.h"

namespace zd {

constexpr int DEFLATE_BLOCK = 64;            // one wave64: one lane per segment, the lanes' hash tables interleaved in LDS
constexpr int COPY_BLOCK = 256;

// hdf_pack_kernel: the raw chunk image [n_chunks][rpc][itemsize] of n_records records (the rest of the last chunk: zeros).
// A record, in hdf5_schema.record_dtype's packed layout:  head | reads plane | mid | qual plane | strand plane, where
// head | mid is the record's blob (name, ref, reads | ref_bases, num_reads, label, vcfrec) and the planes are the encoder's
// stored ones, [slot][plane] each.
struct PackArgs {
    const uint8_t* planes[3];   // device: reads, qual, strand
    const uint8_t* blob;        // device [n_records][head + mid]
    const int32_t* slots;       // device [n_records], range-checked on the host
    int64_t n_records;
    uint32_t plane, head, mid;  // bytes; itemsize = head + mid + 3 * plane
};
hipError_t launch_pack(const PackArgs& a, uint64_t image_bytes /* multiple of 8 */, uint8_t* image, hipStream_t s);

// Device buffers of the passes, grown on demand and kept.
struct Ctx;
Ctx* ctx_create();
void ctx_destroy(Ctx* c);

// What run() leaves on the device, one entry per chunk: where the chunk's bytes lie in `out`, how many, the stream's Adler-32, and
// whether it is "store".
struct Streams {
    const uint64_t* offs;
    const uint64_t* sizes;
    const uint32_t* adlers;
    const uint8_t* store;
    const uint8_t* seg_kind;    // dynamic mode: KIND_* of each of the n_segs segments, chunk-major; else null
    uint64_t n_segs;
};
// n_chunks streams, one per chunk of chunk_bytes (<= MAX_STREAM) of `in` (device), placed one behind the other in `out` (device,
// n_chunks * bound(chunk_bytes, seg) bytes at least; only the streams' own bytes are written).  reversed: the deflate kernel takes
// the segments in the opposite launch order (same bytes).  dynamic: zd_deflate_dyn_kernel in place of zd_deflate_kernel (ZD_DYNAMIC).
// raw_on_store: a "store" chunk's bytes in `out` are its chunk_bytes raw
// bytes instead of its stream.  `mid` (may be null) is recorded behind the deflate kernel.  Enqueues on s and does not wait.
// 0, or -2 with msg.
int run(Ctx* c, const uint8_t* in, uint64_t chunk_bytes, int64_t n_chunks, uint32_t seg, bool reversed, bool raw_on_store, bool dynamic,
        uint8_t* out, hipStream_t s, hipEvent_t mid, Streams* res, const char** msg);

}  // namespace zd
