// Device side of the zlib stream inflate (zinflate_kernels.hip) as its host sees it (zinflate_capi.cpp).
#pragma once

#include "zinflate.h"

namespace zi {

// Inflates (or, where desc.raw, copies) n streams of comp (device) into their slots of out (device); status[i] per stream.
// Streams whose desc.status is set are skipped: their status is passed on.
hipError_t launch_inflate(const uint8_t* comp, const StreamDesc* tab, int64_t n, uint8_t* out, int32_t* status, hipStream_t stream);

}  // namespace zi
