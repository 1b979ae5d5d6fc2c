// libcfx.so - the MXFP4 block-scaled residual codec (CFX_CODEC_MXFP4, include/cfx.h "MXFP4"): 32 consecutive elements share one E8M0
// power-of-two scale, every element is an FP4 E2M1 value.  A block's scale is a function of the block alone, so - as for top-k - there is
// nothing global to wait for: compress / decompress kernels and the layer launch (k_mx_layer), the shape of cfx_topk.hip.
// Shared device code: cfx_device.h; the C-ABI and the dispatch: cfx_api.hip.
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
// One lane owns 8 consecutive flat elements (one 16-byte load of x, one of base, one 32-bit word of codes); a block is the 4 lanes of a
// DPP quad (E % 32 == 0 and a workgroup starts at a multiple of 2048: quads never straddle blocks).  The conversions are written in plain
// integer / exact fp32 arithmetic, not with v_cvt_scalef32_pk_fp4_f16 / _pk_f16_fp4: the contract fixes the sign of a zero code, the NaN
// block and the exponent clamp bit for bit, and those cases were never measured against the hardware conversions.
// ---------------------------------------------------------------------------------------------------
#define MX_PUT(ptr, v) do { if (WT) st_wt(ptr, v); else *(ptr) = (v); } while (0)
#define MX_NAN ((u16)0x7e00)

// The scale byte of the block whose largest magnitude (fp16 bits without the sign) is `a`: 0xFF for a block with a NaN or an inf, else
// X + 127 with X = max(floor(log2 |d|max), -21) - 2.
__device__ __forceinline__ unsigned mx_scale_byte(unsigned a) {
    if (a >= 0x7c00u) return 0xFFu;
    // normal: the exponent field; subnormal a * 2^-24: from the leading bit (a == 0: below the clamp)
    int e = a >= 0x400u ? (int)(a >> 10) - 15 : (31 - __builtin_clz(a | 1u)) - 24;
    e = e < -21 ? -21 : e;
    return (unsigned)(e - 2 + 127);
}

// 8 deltas -> 8 codes (sign << 3 | index of the nearest grid point of |d| / 2^X, ties to the even index, y > 6 saturates), element i at
// bits 4i.  y is exact in fp32: an 11-bit significand times a power of two, 2^-37 <= y < 8.
__device__ __forceinline__ unsigned mx_codes(h16x8 d, unsigned sbyte) {
    if (sbyte == 0xFFu) return 0u;
    const float inv = __builtin_bit_cast(float, (254u - sbyte) << 23);      // 2^-X
    const u16x8 db = __builtin_bit_cast(u16x8, d);
    unsigned codes = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float y = (float)hfrom((u16)(db[i] & 0x7fffu)) * inv;
        const unsigned mag = (unsigned)(y > 0.25f) + (unsigned)(y >= 0.75f) + (unsigned)(y > 1.25f) + (unsigned)(y >= 1.75f) +
                             (unsigned)(y > 2.5f) + (unsigned)(y >= 3.5f) + (unsigned)(y > 5.0f);
        codes |= ((((unsigned)db[i] >> 15) << 3) | mag) << (4 * i);
    }
    return codes;
}

// 8 codes + the block's scale byte -> what a receiver adds: (+-) grid[mag] * 2^X, exact in fp16 (twice the grid as an integer times
// 2^(X-1) in fp32, one exact conversion; the sign bit is or-ed in, so that code 8 is -0); a 0xFF block is NaN.
__device__ __forceinline__ h16x8 mx_recv(unsigned codes, unsigned sbyte) {
    u16x8 r;
    if (sbyte == 0xFFu) {
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = MX_NAN;
        return __builtin_bit_cast(h16x8, r);
    }
    const float half_scale = __builtin_bit_cast(float, (sbyte - 1u) << 23);      // 2^(X-1)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned c = (codes >> (4 * i)) & 15u;
        const unsigned g2 = (0xC8643210u >> (4 * (c & 7u))) & 15u;              // 2 * {0, 0.5, 1, 1.5, 2, 3, 4, 6}
        const h16 v = (h16)((float)(int)g2 * half_scale);
        r[i] = (u16)(hbits(v) | ((c & 8u) << 12));
    }
    return __builtin_bit_cast(h16x8, r);
}

// The 8 elements at flat offset e of one tensor.  EVERY lane of a wave calls it - the block maximum and the scale bytes travel between
// lanes - a lane past the tensor's end (live == false: the last wave of E % 2048 != 0) with the clamped loads of its caller, and stores nothing.
// WT: the packet goes out write-through - workgroups of the same launch read it (k_mx_layer).
template <bool WT>
__device__ __forceinline__ void mx_compress_unit(const cfx_comp_item& it, size_t e, size_t E, bool live, int flags, h16x8 xv, h16x8 bv) {
    const h16* base = (const h16*)it.base;
    h16* nb = (h16*)it.new_base;
    unsigned* code = (unsigned*)it.packet;
    unsigned char* scale = (unsigned char*)it.packet + E / 2;
    const bool upd = (flags & CFX_FLAG_UPDATE_CACHE) && nb;
    const bool ef = !(flags & CFX_FLAG_NO_EF);
    const h16x8 d = base ? (xv - bv) : xv;
    u16x8 m = __builtin_bit_cast(u16x8, d);
    m &= (u16)0x7fff;
    unsigned a = m[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) a = a > (unsigned)m[i] ? a : (unsigned)m[i];
    // the block's maximum: an integer max over the quad's 4 lanes
    unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)a, 0xB1, 0xf, 0xf, true);     // quad_perm [1,0,3,2]
    a = a > o ? a : o;
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)a, 0x4E, 0xf, 0xf, true);              // quad_perm [2,3,0,1]
    a = a > o ? a : o;
    const unsigned sbyte = mx_scale_byte(a);
    const unsigned codes = mx_codes(d, sbyte);
    // the scale bytes of 4 neighbouring blocks (16 lanes, 128 elements) in one 32-bit store; the tensor's last 64 elements: 2 in a 16-bit one
    unsigned w = sbyte;
    w |= (unsigned)__shfl_down((int)sbyte, 4, 64) << 8;
    w |= (unsigned)__shfl_down((int)sbyte, 8, 64) << 16;
    w |= (unsigned)__shfl_down((int)sbyte, 12, 64) << 24;
    if (!live) return;
    MX_PUT(&code[e / 8], codes);
    if ((threadIdx.x & 15) == 0) {
        if (e + 128 <= E) MX_PUT((unsigned*)(scale + e / 32), w);
        else MX_PUT((u16*)(scale + e / 32), (u16)w);
    }
    if (upd) {
        h16x8 out;
        if (ef) {
            const h16x8 recv = mx_recv(codes, sbyte);
            out = base ? (bv + recv) : recv;
        } else out = xv;
        st8nt(nb + e, out);
    }
}

__global__ __launch_bounds__(256) void k_mx_compress(BatchC batch, size_t E, int flags) {
    const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    const bool live = e < E;
    const size_t ec = live ? e : 0;                       // (no lane leaves before the cross-lane steps: clamped loads, no stores)
    const cfx_comp_item it = batch.it[blockIdx.y];
    const h16x8 xv = ld8nt((const h16*)it.x + ec);
    h16x8 bv = (h16x8)(h16)0;
    if (it.base) bv = ld8nt((const h16*)it.base + ec);
    mx_compress_unit<false>(it, e, E, live, flags, xv, bv);
}

// What a receiver needs for the 8 elements at flat offset e: one code word and the block's scale byte, from a packet read with plain
// loads (MODE 0), with L2-bypassing loads (1: another workgroup of this launch wrote it) or with system-scope loads (2: another GPU did).
// Load and use are apart so that a caller can put several units' loads in flight.
struct MxRecv { unsigned codes; unsigned char sbyte; };
template <int MODE>
__device__ __forceinline__ void mx_recv_load(MxRecv& r, const unsigned* code, const unsigned char* scale, size_t e) {
    r.codes = MODE == 0 ? code[e / 8] : (MODE == 1 ? ld_wt(code + e / 8) : ld_sys(code + e / 8));
    r.sbyte = MODE == 0 ? scale[e / 32] : (MODE == 1 ? ld_wt(scale + e / 32) : ld_sys(scale + e / 32));
}

// ---- the MXFP4 layer in ONE launch (cfx_compress_batch_gated / the exchange-layer ops), k_topk_layer's structure: group S compresses the
// own tensors and counts itself on the gate; group D - launched with it - holds the peers' state rows in registers until the gate (or the
// external gate: the packets of the other ranks) opens, then reads code words + scale bytes and stores.
#define MXL_SU 4                // units (8 elements a thread) of an S workgroup: 8192 elements, their loads in flight together
#define MXL_DU 8                // ... of a D workgroup: 16384 elements, 128 bytes of state a thread held across the wait
struct MxLayerArgs {
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
__global__ __launch_bounds__(256) void k_mx_layer(BatchC batch, BatchD gated, MxLayerArgs a) {
    int b = blockIdx.x;
    if (b < a.n_st) {
        const int z = b / a.n_sw, sw = b - z * a.n_sw;
        const cfx_comp_item it = batch.it[z];
        h16x8 xv[MXL_SU], xb[MXL_SU];
#pragma unroll
        for (int u = 0; u < MXL_SU; ++u) {                  // every unit's loads first (clamped offset: unconditional)
            const size_t e = (((size_t)sw * MXL_SU + u) * 256 + threadIdx.x) * 8, ec = e < a.E ? e : 0;
            xv[u] = ld8nt((const h16*)it.x + ec);
            xb[u] = it.base ? ld8nt((const h16*)it.base + ec) : (h16x8)(h16)0;
        }
#pragma unroll
        for (int u = 0; u < MXL_SU; ++u) {
            const size_t e = (((size_t)sw * MXL_SU + u) * 256 + threadIdx.x) * 8;
            mx_compress_unit<true>(it, e, a.E, e < a.E, a.flags, xv[u], xb[u]);
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
    h16x8 bv[MXL_DU];
#pragma unroll
    for (int u = 0; u < MXL_DU; ++u) {
        const size_t e = (((size_t)dw * MXL_DU + u) * 256 + threadIdx.x) * 8;
        bv[u] = (base && e < a.E) ? ld8nt(base + e) : (h16x8)(h16)0;
    }
    if (!(a.xgate ? gate_wait<true>(a.xgate, a.xexpect, a.err, a.timeout) : gate_wait<false>(a.gate, a.gate_expect, a.err, a.timeout))) return;
    const unsigned* code = (const unsigned*)it.packet;
    const unsigned char* scale = (const unsigned char*)it.packet + a.E / 2;
    MxRecv rr[MXL_DU];                                      // every unit's packet words in flight at once, then the stores
#pragma unroll
    for (int u = 0; u < MXL_DU; ++u) {
        const size_t e = (((size_t)dw * MXL_DU + u) * 256 + threadIdx.x) * 8, ec = e < a.E ? e : 0;
        if (a.remote) mx_recv_load<2>(rr[u], code, scale, ec);
        else mx_recv_load<1>(rr[u], code, scale, ec);
    }
#pragma unroll
    for (int u = 0; u < MXL_DU; ++u) {
        const size_t e = (((size_t)dw * MXL_DU + u) * 256 + threadIdx.x) * 8;
        if (e < a.E) {
            const h16x8 rv = mx_recv(rr[u].codes, rr[u].sbyte);
            st8nt(out + e, base ? (bv[u] + rv) : rv);
        }
    }
}

__global__ __launch_bounds__(256) void k_mx_decompress(BatchD batch, size_t E, unsigned* pre, unsigned pre_val) {
    // lane: publish `pre` first - the launch in front of this one in the stream (the previous peer's reconstruction) has finished
    if (pre && (blockIdx.x | blockIdx.y | blockIdx.z | threadIdx.x) == 0) st_wt(pre, pre_val);
    const cfx_decomp_item it = batch.it[blockIdx.y];
    const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (e >= E) return;                                      // (nothing travels between lanes here)
    const h16* base = (const h16*)it.base;
    h16* out = (h16*)it.recon;
    MxRecv rr;
    mx_recv_load<0>(rr, (const unsigned*)it.packet, (const unsigned char*)it.packet + E / 2, e);
    h16x8 bv = (h16x8)(h16)0;
    if (base) bv = ld8nt(base + e);
    const h16x8 recv = mx_recv(rr.codes, rr.sbyte);
    st8nt(out + e, base ? (bv + recv) : recv);
}

// ---------------------------------------------------------------------------------------------------
// host side: this family's launches (validated and dispatched by cfx_api.hip)
// ---------------------------------------------------------------------------------------------------
int cfx_i_mx_compress(CompressCall& cc) {
    cfx_ctx* ctx = cc.ctx;
    const int N = cc.N, C = cc.C, flags = cc.flags, batch = cc.batch, n_gated = cc.n_gated;
    const cfx_comp_item* items = cc.items;
    const cfx_decomp_item* gated = cc.gated;
    void* stream = cc.stream;
    hipStream_t s = (hipStream_t)stream;
    CfxXGate* xg = cc.xg;
    const size_t E = (size_t)N * C;
    // ---- the layer in ONE launch (k_mx_layer): the reconstruction group launched with the compress group, gated on the packets ----
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
        MxLayerArgs a;
        memset(&a, 0, sizeof(a));
        a.E = E;
        a.n_sw = (int)((E / 8 + 256 * MXL_SU - 1) / (256 * MXL_SU));
        a.n_st = a.n_sw * batch;
        a.n_dw = (int)((E / 8 + 256 * MXL_DU - 1) / (256 * MXL_DU));
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
        LAUNCH(ctx, KID_ABSMEAN_COMPRESS_GATED, s, k_mx_layer, g, dim3(256), 0, s, cc.b, cc.gd, a);
        return check_launch(ctx, "mxfp4 layer launch");
    }
    const dim3 g((unsigned)((E / 8 + 255) / 256), batch);
    LAUNCH(ctx, KID_TOPK_COMPRESS, s, k_mx_compress, g, dim3(256), 0, s, cc.b, E, flags);
    const int rc = check_launch(ctx, "mxfp4 compress launch");
    // no layer form here: an exchange-layer op runs its exchange and the reconstruction behind this call; a plain gated call gets the
    // reconstruction in stream order
    if (rc != CFX_OK || xg || !n_gated) return rc;
    return cfx_i_decompress_impl(ctx, cc.codec, N, C, cc.param, n_gated, gated, stream, nullptr, 0u);
}

int cfx_i_mx_decompress(cfx_ctx* ctx, int N, int C, int batch, const BatchD& b, void* stream, unsigned* pre, unsigned pre_val) {
    hipStream_t s = (hipStream_t)stream;
    const size_t E = (size_t)N * C;
    const dim3 g((unsigned)((E / 8 + 255) / 256), batch);
    LAUNCH(ctx, KID_TOPK_DECOMPRESS, s, k_mx_decompress, g, dim3(256), 0, s, b, E, pre, pre_val);
    return check_launch(ctx, "decompress launch");
}
