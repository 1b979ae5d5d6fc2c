// libcfx.so - the block-scaled 1-bit residual codec (CFX_CODEC_BINARY_BLOCK, include/cfx.h "BINARY_BLOCK"): sign bits plus one fp16
// abs-mean per B consecutive elements of a row, B = param in {32, 64, 128}.  A block's scale is a function of the block alone, so - as for
// MXFP4 - there is nothing global to wait for: compress / decompress kernels and the layer launch (k_bb_layer) are cfx_local.h's skeleton around
// this codec, for fp16 and bf16 activations.  Shared device code: cfx_device.h; the C-ABI and the dispatch: cfx_api.hip.
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
#include "cfx_bscale.h"
#include "cfx_bblock.h"


// stand-alone compress / decompress and the layer in ONE launch: cfx_local.h's bodies
template <class El, int B>
__global__ __launch_bounds__(256) void k_bb_compress(BatchC batch, size_t E, int flags) { local_compress<BbCodec<El, B>>(batch, E, flags); }
template <class El, int B>
__global__ __launch_bounds__(256) void k_bb_layer(BatchC batch, BatchD gated, LocalLayerArgs a) { LOCAL_LAYER(batch, gated, a, BbCodec<El, B>); }
template <class El, int B>
__global__ __launch_bounds__(256) void k_bb_decompress(BatchD batch, size_t E, unsigned* pre, unsigned pre_val) {
    local_decompress<BbCodec<El, B>>(batch, E, pre, pre_val);
}

// ---------------------------------------------------------------------------------------------------
// host side: this family's launches (validated and dispatched by cfx_api.hip)
// ---------------------------------------------------------------------------------------------------
LOCAL_FAMILY_HOST(bb, "binary-block", BB_LAUNCH)
