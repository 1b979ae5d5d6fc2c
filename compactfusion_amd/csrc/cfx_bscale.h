// What the block-scaled codecs whose scale is a block's abs-mean share - BINARY_BLOCK (cfx_bblock.hip) and INT2_BLOCK (cfx_i2block.hip): the
// exact sum of |d| over the lanes of a block, and the choice among the six instantiations (element type x block size) of a kernel template.
// One lane owns 8 consecutive flat elements; a block is B / 8 = 4, 8 or 16 neighbouring lanes - a DPP quad, half row or row.
#ifndef CFX_BSCALE_H
#define CFX_BSCALE_H
#include "cfx_device.h"

// The sum of a u64 over the B / 8 lanes of a block, in every lane of the block.  A lane's 8 elements are below 2^43 units: the low 24
// bits and the bits above travel as two 32-bit DPP sums (16 lanes: below 2^28 and 2^23), with no carry between them until the end.
template <int B>
__device__ __forceinline__ u64 bb_block_sum(u64 v) {
    unsigned lo = (unsigned)v & 0xFFFFFFu, hi = (unsigned)(v >> 24);
    lo += __builtin_amdgcn_update_dpp(0u, lo, 0xB1, 0xf, 0xf, true);     // quad_perm [1,0,3,2]
    hi += __builtin_amdgcn_update_dpp(0u, hi, 0xB1, 0xf, 0xf, true);
    lo += __builtin_amdgcn_update_dpp(0u, lo, 0x4E, 0xf, 0xf, true);     // quad_perm [2,3,0,1]
    hi += __builtin_amdgcn_update_dpp(0u, hi, 0x4E, 0xf, 0xf, true);
    if constexpr (B >= 64) {
        lo += __builtin_amdgcn_update_dpp(0u, lo, 0x141, 0xf, 0xf, true);    // row_half_mirror: the other quad of the 8 lanes
        hi += __builtin_amdgcn_update_dpp(0u, hi, 0x141, 0xf, 0xf, true);
    }
    if constexpr (B >= 128) {
        lo += __builtin_amdgcn_update_dpp(0u, lo, 0x140, 0xf, 0xf, true);    // row_mirror: the other half of the 16 lanes
        hi += __builtin_amdgcn_update_dpp(0u, hi, 0x140, 0xf, 0xf, true);
    }
    return ((u64)hi << 24) + lo;
}

// one of the six instantiations of a kernel template: the element type x the block size (validated: 32, 64 or 128); cfx_host.h's LAUNCH
// with the caller's `ctx` and stream `s`
#define BB_LAUNCH(bf16, B, kid, kern, grid, ...) \
    do { \
        if (bf16) { \
            if ((B) == 32) LAUNCH(ctx, kid, s, (kern<ElemBF16, 32>), grid, dim3(256), 0, s, __VA_ARGS__); \
            else if ((B) == 64) LAUNCH(ctx, kid, s, (kern<ElemBF16, 64>), grid, dim3(256), 0, s, __VA_ARGS__); \
            else LAUNCH(ctx, kid, s, (kern<ElemBF16, 128>), grid, dim3(256), 0, s, __VA_ARGS__); \
        } else { \
            if ((B) == 32) LAUNCH(ctx, kid, s, (kern<ElemF16, 32>), grid, dim3(256), 0, s, __VA_ARGS__); \
            else if ((B) == 64) LAUNCH(ctx, kid, s, (kern<ElemF16, 64>), grid, dim3(256), 0, s, __VA_ARGS__); \
            else LAUNCH(ctx, kid, s, (kern<ElemF16, 128>), grid, dim3(256), 0, s, __VA_ARGS__); \
        } \
    } while (0)
#endif
