// libcfx.so - cfx_attn_merge_many (include/cfx.h): ALL of a layer's attention blocks merged in ONE launch.  The chain
// (cfx_attn_merge_ex, once per block) reads and rewrites the running fp32 out / lse for every block; this kernel reads each block's
// output once and writes the result once, forming the softmax-weighted combination directly.  Per row (b, s, h), in fp32, every
// operation rounded on its own (the library is compiled with -ffp-contract=off: no fma):
//     m     = max_i lse_i
//     x_i   = lse_i - m                            one subtraction; exactly 0 for the maximum
//     e_i   = __expf(x_i)                          exactly 1 for the maximum
//     Z     = ((e_0 + e_1) + e_2) + ...            index order
//     a_d   = ((e_0 o_0d + e_1 o_1d) + ...)        each product rounded, sums in index order
//     out_d = a_d / Z                              ONE correctly rounded division (no reciprocal)
//     lse   = m + logf(Z)
// n = 1: e = 1, Z = 1, logf(1) = 0 - the block's own values and its lse, exactly.
// Thread shape: the chain kernel's (cfx_api.hip, attn_merge_body) - one thread owns 8 consecutive d of one row, a row takes the power of
// two >= D/8 lanes, idle lanes return.  A thread reads the row's n lse values first (the same addresses across its group: a broadcast),
// then issues the blocks' 16-byte non-temporal loads, up to 8 in flight before the first is consumed.  The outputs never alias the inputs.
// The two pointer tables travel BY VALUE in the kernel arguments: no device-side table, nothing a captured graph bakes in besides the
// pointers themselves.  Every loop over blocks is fully unrolled with a wave-uniform guard, so the tables are read with constant
// offsets from the kernel-argument segment and the per-block values stay in registers (no scratch).
// A translation unit of its own, compiled into libcfx.so beside build.py's SRC and CAPTURE_SRC: their kernels stay exactly what they were.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include "cfx.h"
#include "cfx_internal.h"
#include "cfx_device.h"

struct MergeTabs {
    const u16* bo[CFX_MERGE_MAX_BLOCKS];
    const float* bl[CFX_MERGE_MAX_BLOCKS];
};

template <class E, bool F32OUT>
__global__ __launch_bounds__(256) void k_attn_merge_many(MergeTabs t, int n, void* __restrict__ out, float* __restrict__ lse,
                                                         int B, int S, int H, int D, size_t bo_sb, size_t bo_ss, size_t bo_sh, int lg) {
    constexpr int NB = CFX_MERGE_MAX_BLOCKS, FLIGHT = 8;
    const int D8 = D >> 3;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t rows = (size_t)B * S * H;
    const int d8 = (int)(i & ((1u << lg) - 1));
    size_t r = i >> lg;
    if (r >= rows || d8 >= D8) return;
    const int h = (int)(r % H); r /= H;
    const int s_ = (int)(r % S);
    const int b = (int)(r / S);
    const size_t o_idx = (((size_t)b * S + s_) * H + h) * D + (size_t)d8 * 8;
    const size_t l_idx = ((size_t)b * S + s_) * H + h;
    const size_t bl_idx = ((size_t)b * H + h) * S + s_;
    const size_t bo_idx = (size_t)b * bo_sb + (size_t)s_ * bo_ss + (size_t)h * bo_sh + (size_t)d8 * 8;
    // the row's lse values, their maximum, the weights and their sum
    float e[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k)
        if (k < n) e[k] = t.bl[k][bl_idx];
    float m = e[0];
#pragma unroll
    for (int k = 1; k < NB; ++k)
        if (k < n) m = fmaxf(m, e[k]);
    float Z = 0.0f;
#pragma unroll
    for (int k = 0; k < NB; ++k)
        if (k < n) {
            e[k] = __expf(e[k] - m);
            Z = k ? Z + e[k] : e[k];
        }
    // the blocks, FLIGHT loads at a time
    float a[8];
#pragma unroll
    for (int k0 = 0; k0 < NB; k0 += FLIGHT) {
        if (k0 < n) {
            h16x8 w[FLIGHT];
#pragma unroll
            for (int j = 0; j < FLIGHT; ++j)
                if (k0 + j < n) w[j] = ld8nt(reinterpret_cast<const h16*>(t.bo[k0 + j]) + bo_idx);      // (the 16-bit words as they are: E says what they hold)
#pragma unroll
            for (int j = 0; j < FLIGHT; ++j)
                if (k0 + j < n) {
                    float o[8];
                    el_widen8<E>(w[j], o);
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const float p = e[k0 + j] * o[c];
                        a[c] = (k0 + j) ? a[c] + p : p;
                    }
                }
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) a[c] = a[c] / Z;
    if constexpr (F32OUT) {
        float4* op = reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + o_idx);
        op[0] = make_float4(a[0], a[1], a[2], a[3]);
        op[1] = make_float4(a[4], a[5], a[6], a[7]);
    } else {
        st8(reinterpret_cast<h16*>(out) + o_idx, el_round8<E>(a));
    }
    if (d8 == 0) lse[l_idx] = m + logf(Z);
}

extern "C" {

int cfx_attn_merge_many(cfx_ctx* ctx, int n, const void* const* block_outs, const void* const* block_lses, int B, int S, int H, int D,
                        int flags, void* out, void* lse, void* stream) {
    if (!ctx || !block_outs || !block_lses || !out || !lse) return fail(ctx, CFX_ERR_NULL, "attn_merge_many: null pointer");
    const int nt = n < 0 ? 0 : (n > CFX_MERGE_MAX_BLOCKS ? CFX_MERGE_MAX_BLOCKS : n);
    for (int k = 0; k < nt; ++k)
        if (!block_outs[k] || !block_lses[k]) return fail(ctx, CFX_ERR_NULL, "attn_merge_many: null pointer in a block table");
    if (flags & ~(CFX_MERGE_BSHD | CFX_ELEM_BF16 | CFX_MERGE_OUT_F32)) return fail(ctx, CFX_ERR_CODEC, "attn_merge_many: unknown flag bit (CFX_MERGE_FIRST is not accepted here)");
    if (n < 1 || n > CFX_MERGE_MAX_BLOCKS) return fail(ctx, CFX_ERR_SHAPE, "attn_merge_many: 1 to 16 blocks");
    if (B <= 0 || S <= 0 || H <= 0 || D <= 0 || (D & 7) || D > 512) return fail(ctx, CFX_ERR_SHAPE, "attn_merge_many: head dim must be a positive multiple of 8, at most 512");
    int lg = 0;
    while ((1 << lg) < D / 8) ++lg;          // a row's D/8 threads in 2^lg lanes of one wave
    const size_t total = ((size_t)B * S * H) << lg;
    if ((total + 255) / 256 > 0x7fffffffu) return fail(ctx, CFX_ERR_SHAPE, "attn_merge_many: too many rows for one launch");
    if (!AL16(out)) return fail(ctx, CFX_ERR_ALIGN, "attn_merge_many: pointers must be 16-byte aligned");
    for (int k = 0; k < n; ++k)
        if (!AL16(block_outs[k])) return fail(ctx, CFX_ERR_ALIGN, "attn_merge_many: pointers must be 16-byte aligned");
    if (ctx->gate_err && *(volatile unsigned*)ctx->gate_err) return fail(ctx, CFX_ERR_GATE, "attn_merge_many: an earlier flag / gate wait on this context timed out (cfx_gate_errors)");
    hipStream_t s = (hipStream_t)stream;
    const int bshd = flags & CFX_MERGE_BSHD;
    MergeTabs t;
    for (int k = 0; k < CFX_MERGE_MAX_BLOCKS; ++k) {         // (unused entries repeat block 0: never read, never garbage)
        t.bo[k] = (const u16*)block_outs[k < n ? k : 0];
        t.bl[k] = (const float*)block_lses[k < n ? k : 0];
    }
#define MERGE_MANY(E, F32) \
    LAUNCH(ctx, KID_ATTN_MERGE, s, (k_attn_merge_many<E, F32>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, t, n, out, (float*)lse, \
           B, S, H, D, (size_t)S * H * D, bshd ? (size_t)H * D : (size_t)D, bshd ? (size_t)D : (size_t)S * D, lg)
    if (flags & CFX_ELEM_BF16) {
        if (flags & CFX_MERGE_OUT_F32) MERGE_MANY(ElemBF16, true); else MERGE_MANY(ElemBF16, false);
    } else {
        if (flags & CFX_MERGE_OUT_F32) MERGE_MANY(ElemF16, true); else MERGE_MANY(ElemF16, false);
    }
#undef MERGE_MANY
    return check_launch(ctx, "attn_merge_many launch");
}

}  // extern "C"
