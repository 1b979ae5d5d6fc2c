// libcfx.so - the MXINT8 block-scaled residual codec (CFX_CODEC_MXINT8, include/cfx.h "MXINT8"): 32 consecutive elements share one E8M0
// power-of-two scale, every element is an int8 with an implied 2^-6 (OCP Microscaling v1.0).  A block's scale is a function of the block
// alone, so there is nothing global to wait for and no workspace: compress / decompress kernels and the layer launch (k_mxi8_layer) are
// cfx_local.h's skeleton around this codec, for fp16 and bf16 activations.
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
#include "cfx_mxint8.h"


// stand-alone compress / decompress and the layer in ONE launch: cfx_local.h's bodies
template <class El>
__global__ __launch_bounds__(256) void k_mxi8_compress(BatchC batch, size_t E, int flags) { local_compress<MxI8Codec<El>>(batch, E, flags); }
template <class El>
__global__ __launch_bounds__(256) void k_mxi8_layer(BatchC batch, BatchD gated, LocalLayerArgs a) { LOCAL_LAYER(batch, gated, a, MxI8Codec<El>); }
template <class El>
__global__ __launch_bounds__(256) void k_mxi8_decompress(BatchD batch, size_t E, unsigned* pre, unsigned pre_val) {
    local_decompress<MxI8Codec<El>>(batch, E, pre, pre_val);
}

// ---------------------------------------------------------------------------------------------------
// host side: this family's launches (validated and dispatched by cfx_api.hip)
// ---------------------------------------------------------------------------------------------------

LOCAL_FAMILY_HOST(mxi8, "mxint8", MXI8_LAUNCH)
