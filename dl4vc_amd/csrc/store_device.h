// Device side of the record store (store_kernels.hip): what its kernels take and the functions that launch them.  The host side
// (store_capi.cpp) checks every index these follow before anything is enqueued.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pileup_device.h"
#include "store_host.h"

namespace st {

constexpr int STORE_BLOCK = 256;             // threads per workgroup of the store's kernels (four waves)

// what the extent, spans and pack kernels read: slot i's plane p, [S][W], at plane[p] + i * stride (st::HostSource's rule).
// Inflated records of record_bytes: plane[p] = records + plane_off[p], stride = record_bytes.  The pileup encoder's three arrays
// [n_slots][S][W]: plane[p] = the array, stride = S * W.
struct Source {
    const uint8_t* plane[3];
    int64_t stride;
    int32_t S, W;
};

// one entry of the record table: where a stored record lies (0 where kept == 0), how many rows it kept and its format
// (st::FORMAT_ROWS / st::FORMAT_COMPACT)
struct DevRec {
    uint64_t addr;
    int32_t kept;
    int32_t format;
};

// one record of a pack launch
struct PackItem {
    uint64_t dst;          // device address of the stored record (a 16-byte boundary)
    int32_t slot;          // record of the inflated buffer
    int32_t kept;
    int32_t record;        // entry of the record table
    int32_t entry;         // store_pack_compact: the entry of the append whose spans record_spans wrote (rowspans + entry * S)
    int32_t cells;         // store_pack_compact: the sum of those spans
    int32_t bytes;         // store_pack_compact: the bytes of the stored record; nothing outside [dst, dst + bytes) is written
};

struct AssembleArgs {
    const DevRec* table;
    uint8_t* dst[3];             // assembled reads / qual / strand [m][R][L]
    const pg::SiteSrc* sites;    // [m], device: slot = the record
    const int16_t* rows;         // [m][R], device; read only where first_rows == 0
    int32_t R, L;
    int32_t use[3];              // 0: the plane is zero-filled
};

// kept[i] = the extent of record slots[i] of src (one workgroup per record); the caller has checked every slot
hipError_t launch_extent(const Source& src, const int32_t* slots, int64_t n, int32_t* kept, hipStream_t s);
// items[i].kept rows of the three planes of record items[i].slot to items[i].dst, and table[items[i].record] = {dst, kept}
hipError_t launch_pack(const Source& src, const PackItem* items, int64_t n, DevRec* table, hipStream_t s);
// sums[i] and rowspans[i * S + r] = the spans of record slots[i] of src (one workgroup per record; src.W <= COMPACT_MAX_WINDOW)
hipError_t launch_spans(const Source& src, const int32_t* slots, int64_t n, SpanSums* sums, uint16_t* rowspans, hipStream_t s);
// the compact record of every item from the spans launch_spans wrote, and its table entry (one workgroup per record)
hipError_t launch_pack_compact(const Source& src, const PackItem* items, int64_t n, const uint16_t* rowspans, DevRec* table, hipStream_t s);
// any_compact == false: the kernel of a store that holds records in the rows layout only
hipError_t launch_store_assemble(const AssembleArgs& a, int32_t m, bool any_compact, hipStream_t s);

}  // namespace st
