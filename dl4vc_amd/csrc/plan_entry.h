// An entry of the host plan rows [m][R] (int16) that the three site gathers follow: pg_assemble_device / cl_assemble_device
// (assemble_kernels.hip), cl_store_assemble_device (store_kernels.hip) and its CPU twin cl_store_assemble_host (store_host.h).
// Bits 0-13 name the stored row.  Bit 14 (ZERO_READS) set: quality and strand come from that row, the reads plane of the output
// row is zeros -- the row dynamic read down-sampling fills a site up with (dl4vc_amd/dataset.py::plan_rows).  The stored rows of a
// plan therefore number at most MAX_STORED (the layouts in use store 200).
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PLAN_ENTRY_FN __host__ __device__ __forceinline__
#else
#define PLAN_ENTRY_FN inline
#endif

namespace plan_entry {

constexpr int ZERO_READS = 0x4000;
constexpr int MAX_STORED = ZERO_READS;
constexpr int NO_ROW = INT16_MAX;           // >= every stored row count and every kept extent: "this row is zeros"

// the stored row an entry names, whatever its flag; a negative entry stays negative (the host checks refuse it)
PLAN_ENTRY_FN int stored_row(int entry) { return entry < 0 ? entry : entry & (ZERO_READS - 1); }

// the stored row plane `plane` (0 reads, 1 quality, 2 strand) of an output row takes, NO_ROW where it is zeros
PLAN_ENTRY_FN int source_row(int entry, int plane) {
    return (entry & ZERO_READS) ? (plane == 0 ? NO_ROW : entry & (ZERO_READS - 1)) : entry;
}

}  // namespace plan_entry
