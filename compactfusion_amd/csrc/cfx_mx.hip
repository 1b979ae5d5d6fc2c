// libcfx.so - the MXFP4 block-scaled residual codec (CFX_CODEC_MXFP4, include/cfx.h "MXFP4"): 32 consecutive elements share one E8M0
// power-of-two scale, every element is an FP4 E2M1 value.  A block's scale is a function of the block alone, so - as for top-k - there is
// nothing global to wait for: compress / decompress kernels and the layer launch (k_mx_layer) are cfx_local.h's skeleton around this codec.
// Shared device code: cfx_device.h; the launch skeleton of the block-local codecs: cfx_local.h; the C-ABI and the dispatch: cfx_api.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "cfx.h"
#include "cfx_internal.h"
#include "cfx_device.h"
#include "cfx_host.h"
#include "cfx_local.h"
#include "cfx_mx.h"


// stand-alone compress / decompress and the layer in ONE launch: cfx_local.h's bodies
__global__ __launch_bounds__(256) void k_mx_compress(BatchC batch, size_t E, int flags) { local_compress<MxCodec>(batch, E, flags); }
__global__ __launch_bounds__(256) void k_mx_layer(BatchC batch, BatchD gated, LocalLayerArgs a) { LOCAL_LAYER(batch, gated, a, MxCodec); }
__global__ __launch_bounds__(256) void k_mx_decompress(BatchD batch, size_t E, unsigned* pre, unsigned pre_val) {
    local_decompress<MxCodec>(batch, E, pre, pre_val);
}

// ---------------------------------------------------------------------------------------------------
// host side: this family's launches (validated and dispatched by cfx_api.hip)
// ---------------------------------------------------------------------------------------------------
LOCAL_FAMILY_HOST(mx, "mxfp4", MX_LAUNCH)
