// What the record store (store_capi.cpp) reads of a cl_loader handle (chunk_capi.cpp): where the records of its last
// cl_inflate_chunks_device call lie in device memory.  The view holds until the loader's next call.
#pragma once

#include <cstdint>

struct cl_loader;

namespace clh {

struct RecordsView {
    const uint8_t* records;      // device: record i at records + i * record_bytes
    int64_t record_bytes, n_records;
    int64_t plane_off[3];
    int32_t window, stored_rows, device;
};

RecordsView records_view(const cl_loader* h);

}  // namespace clh
