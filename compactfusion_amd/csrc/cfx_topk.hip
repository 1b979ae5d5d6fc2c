// libcfx.so - the 1:m top-1 sparsifier (compress_topk.py:11-163): compress / decompress kernels and the layer launch (k_topk_layer).
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
#include "cfx_topk.h"


// stand-alone compress / decompress and the layer in ONE launch: cfx_local.h's bodies
template <int M>
__global__ __launch_bounds__(256) void k_topk_compress(BatchC batch, size_t E, int flags) { local_compress<TopkCodec<M>>(batch, E, flags); }
template <int M>
__global__ __launch_bounds__(256) void k_topk_layer(BatchC batch, BatchD gated, LocalLayerArgs a) { LOCAL_LAYER(batch, gated, a, TopkCodec<M>); }
template <int M>
__global__ __launch_bounds__(256) void k_topk_decompress(BatchD batch, size_t E, unsigned* pre, unsigned pre_val) {
    local_decompress<TopkCodec<M>>(batch, E, pre, pre_val);
}

// ---------------------------------------------------------------------------------------------------
// host side: this family's launches (validated and dispatched by cfx_api.hip)
// ---------------------------------------------------------------------------------------------------

LOCAL_FAMILY_HOST(topk, "topk", TOPK_LAUNCH)
