// Structure rules of the network, once: which layers pool and carry a residual, a layer's extents, a segment's reach, the
// feature width and the padded strides.  Shared by the inference handle (dan_capi.cpp), its weight packing (dan_pack.h) and
// the trainer (dan_train_capi.cpp).  Host only: no HIP runtime call.
#pragma once

#include "../../include/dl4vc_dan.h"
#include "dan_kernels.h"

namespace dan {

inline bool pool_after(const dan_config& c, int l1) { return (c.pool_layers_mask >> l1) & 1u; }   // 1-based layer

inline bool is_residual(const dan_config& c, int l1) {
    return c.residual_start > 0 && l1 >= c.residual_start && !(l1 == c.layers && c.c_init != c.c_final);
}

inline void layer_dims(const dan_config& c, int l1, int* cin, int* cout, int* dil) {
    const int in0 = 2 * EMBED + (c.use_q ? 1 : 0) + (c.use_strand ? 1 : 0) + (c.use_mask ? 3 : 0);
    if (l1 == 1) { *cin = in0; *cout = c.c_init; *dil = 1; }
    else if (l1 < c.layers) { *cin = c.c_init; *cout = c.c_init; *dil = c.dil_mid; }
    else { *cin = c.c_init; *cout = c.c_final; *dil = c.dil_final; }
}

// receptive-field radius of layers [l_begin, l_end) (0-based): the sum of their dilations (3 taps each; model.py:214-231)
inline int segment_halo(const dan_config& c, int l_begin, int l_end) {
    int halo = 0;
    for (int l = l_begin; l < l_end; ++l) halo += (l == 0) ? 1 : (l + 1 < c.layers ? c.dil_mid : c.dil_final);
    return halo;
}

// the feature row of a site: max and mean pool of the last layer, then every layer's highway outputs (model.py:824-859)
inline int feature_width(const dan_config& c) { return 2 * c.c_final * c.length + c.layers * c.bottleneck * c.reads; }

// row strides of the FC operands: a multiple of 16 (K of launch_fc)
inline int64_t pad16(int64_t n) { return (n + 15) / 16 * 16; }

}  // namespace dan
