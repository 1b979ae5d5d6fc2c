// libcfx.so - the MXFP4 codec's device code and policy type (MxCodec) and the launch of its one instantiation: what cfx_mx.hip (the family's kernels and launches) and
// cfx_capture.hip (the capturable instantiations of the layer launch) both compile: one policy type, so the same bits in both.
#ifndef CFX_MX_H
#define CFX_MX_H
#include "cfx_device.h"
#include "cfx_host.h"
#include "cfx_local.h"

// ---------------------------------------------------------------------------------------------------
// One lane owns 8 consecutive flat elements (one 16-byte load of x, one of base, one 32-bit word of codes); a block is the 4 lanes of a
// DPP quad (E % 32 == 0 and a workgroup starts at a multiple of 2048: quads never straddle blocks).  The conversions are written in plain
// integer / exact fp32 arithmetic, not with v_cvt_scalef32_pk_fp4_f16 / _pk_f16_fp4: the contract fixes the sign of a zero code, the NaN
// block and the exponent clamp bit for bit, and those cases were never measured against the hardware conversions.
// ---------------------------------------------------------------------------------------------------
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
    st_put<WT>(&code[e / 8], codes);
    if ((threadIdx.x & 15) == 0) {
        if (e + 128 <= E) st_put<WT>((unsigned*)(scale + e / 32), w);
        else st_put<WT>((u16*)(scale + e / 32), (u16)w);
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

// The codec as cfx_local.h's skeleton sees it.  What a receiver needs for the 8 elements at flat offset e: one code word and the block's
// scale byte, from a packet read with plain loads (MODE 0), with L2-bypassing loads (1: another workgroup of this launch wrote it) or with
// system-scope loads (2: another GPU did).  Load and use are apart so that a caller can put several units' loads in flight.
struct MxCodec {
    using El = ElemF16;
    static constexpr bool ALL_LANES = true;
    static constexpr bool MAKE_FIRST = false;
    static constexpr int IN_FLIGHT = LOCAL_DU;            // every unit's packet words in flight at once, then the stores
    struct Recv { unsigned codes; unsigned char sbyte; };
    template <bool WT>
    static __device__ __forceinline__ void compress_unit(const cfx_comp_item& it, size_t e, size_t E, bool live, int flags, h16x8 xv, h16x8 bv) {
        mx_compress_unit<WT>(it, e, E, live, flags, xv, bv);
    }
    template <int MODE>
    static __device__ __forceinline__ void recv_load(Recv& r, const void* packet, size_t E, size_t e) {
        const unsigned* code = (const unsigned*)packet;
        const unsigned char* scale = (const unsigned char*)packet + E / 2;
        r.codes = MODE == 0 ? code[e / 8] : (MODE == 1 ? ld_wt(code + e / 8) : ld_sys(code + e / 8));
        r.sbyte = MODE == 0 ? scale[e / 32] : (MODE == 1 ? ld_wt(scale + e / 32) : ld_sys(scale + e / 32));
    }
    static __device__ __forceinline__ h16x8 recv_make(const Recv& r, size_t) { return mx_recv(r.codes, r.sbyte); }
};

// the one instantiation of a kernel: cfx_internal.h's LAUNCH with the caller's `ctx` and stream `s`
#define MX_LAUNCH(bf16, param, kid, kern, grid, ...) LAUNCH(ctx, kid, s, kern, grid, dim3(256), 0, s, __VA_ARGS__)
#endif
