// libcfx.so - the block-scaled 1-bit residual codec (CFX_CODEC_BINARY_BLOCK, include/cfx.h "BINARY_BLOCK"): sign bits plus one fp16
// abs-mean per B consecutive elements of a row, B = param in {32, 64, 128}.  A block's scale is a function of the block alone, so - as for
// MXFP4 - there is nothing global to wait for: compress / decompress kernels and the layer launch (k_bb_layer), the shape of cfx_mx.hip,
// for fp16 and bf16 activations.  Shared device code: cfx_device.h; the C-ABI and the dispatch: cfx_api.hip.
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

// ---------------------------------------------------------------------------------------------------
// One lane owns 8 consecutive flat elements (one 16-byte load of x, one of base, one byte of sign bits); a block is B / 8 = 4, 8 or 16
// neighbouring lanes - a DPP quad, half row or row (E % B == 0 and a workgroup starts at a multiple of 2048: blocks never straddle rows
// of lanes).  The block's scale is the exact integer sum of |d| in units of 2^-24 (habs_units), rounded once to fp32 and once to fp16
// (mean16): order-independent, so the lanes may add in any order.
// ---------------------------------------------------------------------------------------------------
#define BB_PUT(ptr, v) do { if (WT) st_wt(ptr, v); else *(ptr) = (v); } while (0)

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

// 8 sign bits (bit i: element i >= 0) + the block's scale (fp16 bits, never negative) -> what a receiver adds: +s or -s
__device__ __forceinline__ h16x8 bb_recv(unsigned bits, unsigned sbits) {
    u16x8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (u16)(sbits | (((bits >> i) & 1u) ? 0u : 0x8000u));
    return __builtin_bit_cast(h16x8, r);
}

// The 8 elements at flat offset e of one tensor.  EVERY lane of a wave calls it - the block sum, the sign bytes and the scales travel
// between lanes - a lane past the tensor's end (live == false: the last wave of E % 2048 != 0) with the clamped loads of its caller, and
// stores nothing.  WT: the packet goes out write-through - workgroups of the same launch read it (k_bb_layer).
template <class El, int B, bool WT>
__device__ __forceinline__ void bb_compress_unit(const cfx_comp_item& it, size_t e, size_t E, bool live, int flags, h16x8 xv, h16x8 bv) {
    const bool has_base = it.base != nullptr;
    h16* nb = (h16*)it.new_base;
    unsigned* bitw = (unsigned*)it.packet;
    u16* scale = (u16*)((unsigned char*)it.packet + E / 8);
    const bool upd = (flags & CFX_FLAG_UPDATE_CACHE) && nb;
    const bool ef = !(flags & CFX_FLAG_NO_EF);
    h16x8 d;
    if constexpr (El::bf16) d = el_diff<El>(xv, has_base ? bv : (h16x8)(h16)0);
    else d = has_base ? (xv - bv) : xv;
    const u16x8 db = __builtin_bit_cast(u16x8, d);
    u64 units = 0;
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        units += habs_units(db[i]);
        bits |= (unsigned)(d[i] >= (h16)0) << i;
    }
    const unsigned sbits = hbits(mean16(bb_block_sum<B>(units), B));
    // the sign bytes of a quad (32 elements) in one 32-bit store
    unsigned w = (unsigned)__builtin_amdgcn_update_dpp(0, (int)bits, 0x00, 0xf, 0xf, true);          // quad_perm [0,0,0,0]
    w |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)bits, 0x55, 0xf, 0xf, true) << 8;             // quad_perm [1,1,1,1]
    w |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)bits, 0xAA, 0xf, 0xf, true) << 16;            // quad_perm [2,2,2,2]
    w |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)bits, 0xFF, 0xf, 0xf, true) << 24;            // quad_perm [3,3,3,3]
    // the scales of 2 neighbouring blocks (B / 4 lanes) in one 32-bit store; a tensor's last block where their number is odd: a 16-bit one
    const unsigned sw = sbits | ((unsigned)__shfl_down((int)sbits, B / 8, 64) << 16);
    if (!live) return;
    if ((threadIdx.x & 3) == 0) BB_PUT(&bitw[e / 32], w);
    if ((threadIdx.x & (B / 4 - 1)) == 0) {
        if (e + 2 * B <= E) BB_PUT((unsigned*)(scale + e / B), sw);
        else BB_PUT(scale + e / B, (u16)sbits);
    }
    if (upd) st8nt(nb + e, ef ? el_state<El>(has_base, bv, bb_recv(bits, sbits)) : xv);
}

template <class El, int B>
__global__ __launch_bounds__(256) void k_bb_compress(BatchC batch, size_t E, int flags) {
    const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    const bool live = e < E;
    const size_t ec = live ? e : 0;                       // (no lane leaves before the cross-lane steps: clamped loads, no stores)
    const cfx_comp_item it = batch.it[blockIdx.y];
    const h16x8 xv = ld8nt((const h16*)it.x + ec);
    h16x8 bv = (h16x8)(h16)0;
    if (it.base) bv = ld8nt((const h16*)it.base + ec);
    bb_compress_unit<El, B, false>(it, e, E, live, flags, xv, bv);
}

// What a receiver needs for the 8 elements at flat offset e: their sign byte and the block's scale, from a packet read with plain loads
// (MODE 0), with L2-bypassing loads (1: another workgroup of this launch wrote it) or with system-scope loads (2: another GPU did).
// Load and use are apart so that a caller can put several units' loads in flight.
struct BbRecv { unsigned char bits; u16 sbits; };
template <int B, int MODE>
__device__ __forceinline__ void bb_recv_load(BbRecv& r, const unsigned char* bits, const u16* scale, size_t e) {
    r.bits = MODE == 0 ? bits[e / 8] : (MODE == 1 ? ld_wt(bits + e / 8) : ld_sys(bits + e / 8));
    r.sbits = MODE == 0 ? scale[e / B] : (MODE == 1 ? ld_wt(scale + e / B) : ld_sys(scale + e / B));
}

// ---- the layer in ONE launch (cfx_compress_batch_gated / the exchange-layer ops), k_mx_layer's structure: group S compresses the own
// tensors and counts itself on the gate; group D - launched with it - holds the peers' state rows in registers until the gate (or the
// external gate: the packets of the other ranks) opens, then reads sign bytes + scales and stores.
#define BBL_SU 4                // units (8 elements a thread) of an S workgroup: 8192 elements, their loads in flight together
#define BBL_DU 8                // ... of a D workgroup: 16384 elements, 128 bytes of state a thread held across the wait
struct BbLayerArgs {
    size_t E;
    int n_sw, n_st;             // S workgroups per own tensor / in all
    int n_dw;                   // D workgroups per reconstruction item
    int flags;
    unsigned* gate; unsigned gate_expect;
    unsigned* xgate; unsigned xexpect;
    unsigned* err;
    long long timeout;
    int remote;
    P2PInline p2p;
};
template <class El, int B>
__global__ __launch_bounds__(256) void k_bb_layer(BatchC batch, BatchD gated, BbLayerArgs a) {
    int b = blockIdx.x;
    if (b < a.n_st) {
        const int z = b / a.n_sw, sw = b - z * a.n_sw;
        const cfx_comp_item it = batch.it[z];
        h16x8 xv[BBL_SU], xb[BBL_SU];
#pragma unroll
        for (int u = 0; u < BBL_SU; ++u) {                  // every unit's loads first (clamped offset: unconditional)
            const size_t e = (((size_t)sw * BBL_SU + u) * 256 + threadIdx.x) * 8, ec = e < a.E ? e : 0;
            xv[u] = ld8nt((const h16*)it.x + ec);
            xb[u] = it.base ? ld8nt((const h16*)it.base + ec) : (h16x8)(h16)0;
        }
#pragma unroll
        for (int u = 0; u < BBL_SU; ++u) {
            const size_t e = (((size_t)sw * BBL_SU + u) * 256 + threadIdx.x) * 8;
            bb_compress_unit<El, B, true>(it, e, a.E, e < a.E, a.flags, xv[u], xb[u]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) gate_arrive(a.gate, 1u, a.gate_expect);
        // (packets complete = the word the gate's last arriver writes for XCD 0)
        if (b == 0 && a.p2p.own) p2p_exchange_inline(a.gate + GATE_LINE, a.gate_expect, 1, a.p2p, a.xgate, a.xexpect, a.err);
        return;
    }
    b -= a.n_st;
    const int item = b / a.n_dw, dw = b - item * a.n_dw;
    const cfx_decomp_item it = gated.it[item];
    const h16* base = (const h16*)it.base;
    h16* out = (h16*)it.recon;
    h16x8 bv[BBL_DU];
#pragma unroll
    for (int u = 0; u < BBL_DU; ++u) {
        const size_t e = (((size_t)dw * BBL_DU + u) * 256 + threadIdx.x) * 8;
        bv[u] = (base && e < a.E) ? ld8nt(base + e) : (h16x8)(h16)0;
    }
    if (!(a.xgate ? gate_wait<true>(a.xgate, a.xexpect, a.err, a.timeout) : gate_wait<false>(a.gate, a.gate_expect, a.err, a.timeout))) return;
    const unsigned char* bits = (const unsigned char*)it.packet;
    const u16* scale = (const u16*)(bits + a.E / 8);
    BbRecv rr[BBL_DU];                                      // every unit's packet words in flight at once, then the stores
#pragma unroll
    for (int u = 0; u < BBL_DU; ++u) {
        const size_t e = (((size_t)dw * BBL_DU + u) * 256 + threadIdx.x) * 8, ec = e < a.E ? e : 0;
        if (a.remote) bb_recv_load<B, 2>(rr[u], bits, scale, ec);
        else bb_recv_load<B, 1>(rr[u], bits, scale, ec);
    }
#pragma unroll
    for (int u = 0; u < BBL_DU; ++u) {
        const size_t e = (((size_t)dw * BBL_DU + u) * 256 + threadIdx.x) * 8;
        if (e < a.E) st8nt(out + e, el_state<El>(base != nullptr, bv[u], bb_recv(rr[u].bits, rr[u].sbits)));
    }
}

template <class El, int B>
__global__ __launch_bounds__(256) void k_bb_decompress(BatchD batch, size_t E, unsigned* pre, unsigned pre_val) {
    // lane: publish `pre` first - the launch in front of this one in the stream (the previous peer's reconstruction) has finished
    if (pre && (blockIdx.x | blockIdx.y | blockIdx.z | threadIdx.x) == 0) st_wt(pre, pre_val);
    const cfx_decomp_item it = batch.it[blockIdx.y];
    const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (e >= E) return;                                      // (nothing travels between lanes here)
    const h16* base = (const h16*)it.base;
    h16* out = (h16*)it.recon;
    const unsigned char* bits = (const unsigned char*)it.packet;
    BbRecv rr;
    bb_recv_load<B, 0>(rr, bits, (const u16*)(bits + E / 8), e);
    h16x8 bv = (h16x8)(h16)0;
    if (base) bv = ld8nt(base + e);
    st8nt(out + e, el_state<El>(base != nullptr, bv, bb_recv(rr.bits, rr.sbits)));
}

// ---------------------------------------------------------------------------------------------------
// host side: this family's launches (validated and dispatched by cfx_api.hip)
// ---------------------------------------------------------------------------------------------------
// one of the six instantiations of a kernel template: the element type x the block size (validated: 32, 64 or 128)
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

int cfx_i_bb_compress(CompressCall& cc) {
    cfx_ctx* ctx = cc.ctx;
    const int N = cc.N, C = cc.C, B = cc.param, flags = cc.flags, batch = cc.batch, n_gated = cc.n_gated;
    const cfx_comp_item* items = cc.items;
    const cfx_decomp_item* gated = cc.gated;
    void* stream = cc.stream;
    hipStream_t s = (hipStream_t)stream;
    CfxXGate* xg = cc.xg;
    const size_t E = (size_t)N * C;
    // ---- the layer in ONE launch (k_bb_layer): the reconstruction group launched with the compress group, gated on the packets ----
    const int stream_cus = n_gated ? stream_cu_count(ctx, stream) : 0;
    bool layer = n_gated && ctx->gated_on && !ctx->dev_probe && stream_cus >= 128 && !cc.capturing;
    if (layer && !xg) {
        // loop-back: every reconstruction item reads one of this launch's packets
        for (int g_ = 0; g_ < n_gated && layer; ++g_) {
            bool mine = false;
            for (int i = 0; i < batch; ++i) mine = mine || gated[g_].packet == items[i].packet;
            layer = mine;
        }
    }
    if (layer && !ctx->tick && cfx_prepare(ctx) != CFX_OK) return CFX_ERR_LAUNCH;
    if (layer) {
        if (ctx->gate_err && *(volatile unsigned*)ctx->gate_err)
            return fail(ctx, CFX_ERR_GATE, "compress: an earlier gate / flag wait on this context timed out (cfx_gate_errors reads and clears the count)");
        const unsigned slot = ticket_slot(ctx, stream);
        BbLayerArgs a;
        memset(&a, 0, sizeof(a));
        a.E = E;
        a.n_sw = (int)((E / 8 + 256 * BBL_SU - 1) / (256 * BBL_SU));
        a.n_st = a.n_sw * batch;
        a.n_dw = (int)((E / 8 + 256 * BBL_DU - 1) / (256 * BBL_DU));
        a.flags = flags;
        a.gate = ctx->gate + (size_t)slot * GATE_STRIDE;
        ctx->gate_expect[3 * slot] += (unsigned)a.n_st;
        a.gate_expect = ctx->gate_expect[3 * slot];
        a.err = ctx->gate_err;
        a.timeout = ctx->gate_timeout;
        if (xg) {
            a.xgate = a.gate + GATE_BLOCK;
            a.xexpect = ++ctx->gate_expect[3 * slot + 1];
            a.remote = xg->remote;
            fill_p2p(ctx, xg, a.p2p);
            xg->taken = 1;
            xg->p_gate = a.gate + GATE_LINE; xg->p_expect = a.gate_expect;      // the word the gate's last arriver writes for XCD 0
            xg->f_gate = a.xgate; xg->f_expect = a.xexpect;
        }
        const dim3 g((unsigned)(a.n_st + a.n_dw * n_gated));
        BB_LAUNCH(cc.bf16, B, KID_ABSMEAN_COMPRESS_GATED, k_bb_layer, g, cc.b, cc.gd, a);
        return check_launch(ctx, "binary-block layer launch");
    }
    const dim3 g((unsigned)((E / 8 + 255) / 256), batch);
    BB_LAUNCH(cc.bf16, B, KID_TOPK_COMPRESS, k_bb_compress, g, cc.b, E, flags);
    const int rc = check_launch(ctx, "binary-block compress launch");
    // no layer form here: an exchange-layer op runs its exchange and the reconstruction behind this call; a plain gated call gets the
    // reconstruction in stream order
    if (rc != CFX_OK || xg || !n_gated) return rc;
    return cfx_i_decompress_impl(ctx, cc.codec | (cc.bf16 ? CFX_ELEM_BF16 : 0), N, C, B, n_gated, gated, stream, nullptr, 0u);
}

int cfx_i_bb_decompress(cfx_ctx* ctx, bool bf16, int N, int C, int B, int batch, const BatchD& b, void* stream, unsigned* pre, unsigned pre_val) {
    hipStream_t s = (hipStream_t)stream;
    const size_t E = (size_t)N * C;
    const dim3 g((unsigned)((E / 8 + 255) / 256), batch);
    BB_LAUNCH(bf16, B, KID_TOPK_DECOMPRESS, k_bb_decompress, g, b, E, pre, pre_val);
    return check_launch(ctx, "decompress launch");
}
