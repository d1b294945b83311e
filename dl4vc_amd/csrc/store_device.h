// Device side of the record store (store_kernels.hip): what its kernels take and the functions that launch them.  The host side
// (store_capi.cpp) checks every index these follow before anything is enqueued.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pileup_device.h"

namespace st {

constexpr int STORE_BLOCK = 256;             // threads per workgroup of the three kernels (four waves)

// what the extent and pack kernels read: slot i's plane p, [S][W], at plane[p] + i * stride (st::HostSource's rule).  Inflated
// records of record_bytes: plane[p] = records + plane_off[p], stride = record_bytes.  The pileup encoder's three arrays
// [n_slots][S][W]: plane[p] = the array, stride = S * W.
struct Source {
    const uint8_t* plane[3];
    int64_t stride;
    int32_t S, W;
};

// one entry of the record table: where a stored record lies (0 where kept == 0) and how many rows it kept
struct DevRec {
    uint64_t addr;
    int32_t kept;
    int32_t pad;
};

// one record of a pack launch
struct PackItem {
    uint64_t dst;          // device address of the stored record (a 16-byte boundary)
    int32_t slot;          // record of the inflated buffer
    int32_t kept;
    int32_t record;        // entry of the record table
    int32_t pad;
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
hipError_t launch_store_assemble(const AssembleArgs& a, int32_t m, hipStream_t s);

}  // namespace st
