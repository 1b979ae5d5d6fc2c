// libcfx.so - the block-scaled 2-bit residual codec (CFX_CODEC_INT2_BLOCK, include/cfx.h "INT2_BLOCK"): INT2's sign / magnitude codes and
// levels around BINARY_BLOCK's scale, one fp16 abs-mean per B consecutive elements of a row, B = param in {32, 64, 128}.  A block's packet
// words are a function of the block alone: compress / decompress kernels and the layer launch (k_i2b_layer) are cfx_local.h's skeleton around
// this codec, for fp16 and bf16 activations.  The exact block sum and the launch macro: cfx_bscale.h, shared with cfx_bblock.hip.
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
#include "cfx_i2block.h"


template <class El, int B>
__global__ __launch_bounds__(256) void k_i2b_compress(BatchC batch, size_t E, int flags) { local_compress<I2bCodec<El, B>>(batch, E, flags); }
template <class El, int B>
__global__ __launch_bounds__(256) void k_i2b_layer(BatchC batch, BatchD gated, LocalLayerArgs a) { LOCAL_LAYER(batch, gated, a, I2bCodec<El, B>); }
template <class El, int B>
__global__ __launch_bounds__(256) void k_i2b_decompress(BatchD batch, size_t E, unsigned* pre, unsigned pre_val) {
    local_decompress<I2bCodec<El, B>>(batch, E, pre, pre_val);
}

// ---------------------------------------------------------------------------------------------------
// host side: this family's launches (validated and dispatched by cfx_api.hip)
// ---------------------------------------------------------------------------------------------------
LOCAL_FAMILY_HOST(i2b, "int2-block", BB_LAUNCH)
