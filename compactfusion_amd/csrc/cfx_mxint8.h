// libcfx.so - the MXINT8 codec's device code and policy type (MxI8Codec) and the choice among its instantiations: what cfx_mxint8.hip (the family's kernels and launches) and
// cfx_capture.hip (the capturable instantiations of the layer launch) both compile: one policy type, so the same bits in both.
#ifndef CFX_MXINT8_H
#define CFX_MXINT8_H
#include "cfx_device.h"
#include "cfx_host.h"
#include "cfx_local.h"

// ---------------------------------------------------------------------------------------------------
// MXFP4's lanes (cfx_mx.hip): one lane owns 8 consecutive flat elements - one 16-byte load of x, one of base, one 64-bit word of codes -
// and a block is the 4 lanes of a DPP quad (E % 32 == 0 and a workgroup starts at a multiple of 2048: quads never straddle blocks).  As
// there, the conversions are plain integer / exact fp32 arithmetic, not v_cvt_scalef32_*: the contract fixes the zero code, the NaN block
// and both clamps bit for bit, and those cases were never measured against the hardware conversions.
// ---------------------------------------------------------------------------------------------------
#define MXI8_NAN ((u16)0x7e00)

// The scale byte of the block whose largest magnitude (fp16 bits without the sign) is `a`: 0xFF for a block with a NaN or an inf, else
// X + 127 with X = max(floor(log2 |d|max), -18): 109 ... 142.
__device__ __forceinline__ unsigned mxi8_scale_byte(unsigned a) {
    if (a >= 0x7c00u) return 0xFFu;
    // normal: the exponent field; subnormal a * 2^-24: from the leading bit (a == 0: below the clamp)
    int e = a >= 0x400u ? (int)(a >> 10) - 15 : (31 - __builtin_clz(a | 1u)) - 24;
    e = e < -18 ? -18 : e;
    return (unsigned)(e + 127);
}

// 8 deltas -> 8 two's-complement code bytes, element i at bits 8i: q = clamp(rne(d * 2^(6-X)), -127, 127).  y is exact in fp32 (an 11-bit
// significand times a power of two, |y| < 128); a zero of either sign and a delta that rounds to zero give the byte 0.
__device__ __forceinline__ u64 mxi8_codes(h16x8 d, unsigned sbyte) {
    if (sbyte == 0xFFu) return 0ull;
    const float inv = __builtin_bit_cast(float, (260u - sbyte) << 23);      // 2^(6-X)
    unsigned w[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float r = __builtin_rintf((float)d[i] * inv);
        const int q = (int)__builtin_fminf(__builtin_fmaxf(r, -127.0f), 127.0f);
        w[i >> 2] |= ((unsigned)q & 0xFFu) << (8 * (i & 3));
    }
    return (u64)w[0] | ((u64)w[1] << 32);
}

// 8 code bytes + the block's scale byte -> what a receiver adds: q * 2^(X-6), exact in fp16 (|q| <= 127 times a power of two >= 2^-24:
// one fp32 product, one exact conversion; q == 0 gives +0); the byte 0x80 reads as -127; a 0xFF block is NaN.
__device__ __forceinline__ h16x8 mxi8_recv(u64 codes, unsigned sbyte) {
    u16x8 r;
    if (sbyte == 0xFFu) {
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = MXI8_NAN;
        return __builtin_bit_cast(h16x8, r);
    }
    const float scale = __builtin_bit_cast(float, (sbyte - 6u) << 23);      // 2^(X-6)
    const unsigned w[2] = {(unsigned)codes, (unsigned)(codes >> 32)};
    h16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int q = (int)(signed char)(w[i >> 2] >> (8 * (i & 3)));
        q = q < -127 ? -127 : q;
        v[i] = (h16)((float)q * scale);
    }
    return v;
}

// mx_compress_unit's contract: EVERY lane of a wave calls it - the block maximum and the scale bytes travel between lanes - a lane past
// the tensor's end (live == false) with the clamped loads of its caller, and stores nothing.  WT: the packet goes out write-through.
template <class El, bool WT>
__device__ __forceinline__ void mxi8_compress_unit(const cfx_comp_item& it, size_t e, size_t E, bool live, int flags, h16x8 xv, h16x8 bv) {
    const bool has_base = it.base != nullptr;
    h16* nb = (h16*)it.new_base;
    u64* code = (u64*)it.packet;
    unsigned char* scale = (unsigned char*)it.packet + E;
    const bool upd = (flags & CFX_FLAG_UPDATE_CACHE) && nb;
    const bool ef = !(flags & CFX_FLAG_NO_EF);
    h16x8 d;
    if constexpr (El::bf16) d = el_diff<El>(xv, has_base ? bv : (h16x8)(h16)0);
    else d = has_base ? (xv - bv) : xv;
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
    const unsigned sbyte = mxi8_scale_byte(a);
    const u64 codes = mxi8_codes(d, sbyte);
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
    if (upd) st8nt(nb + e, ef ? el_state<El>(has_base, bv, mxi8_recv(codes, sbyte)) : xv);
}

// The codec as cfx_local.h's skeleton sees it: a receiver's 8 elements are one 64-bit code word and the block's scale byte
template <class E_> struct MxI8Codec {
    using El = E_;
    static constexpr bool ALL_LANES = true;
    static constexpr bool MAKE_FIRST = false;
    static constexpr int IN_FLIGHT = LOCAL_DU;            // eight three-word records: 79 / 80 VGPRs (fp16 / bf16), 6 waves a SIMD; four: 63 / 64, 8 waves,
                                                          // and the layer launch 0.3 - 0.4 us slower (profiles/mxint8_config_rows.json, in_flight_ab)
    struct Recv { u64 codes; unsigned char sbyte; };
    template <bool WT>
    static __device__ __forceinline__ void compress_unit(const cfx_comp_item& it, size_t e, size_t E, bool live, int flags, h16x8 xv, h16x8 bv) {
        mxi8_compress_unit<El, WT>(it, e, E, live, flags, xv, bv);
    }
    template <int MODE>
    static __device__ __forceinline__ void recv_load(Recv& r, const void* packet, size_t E, size_t e) {
        const u64* code = (const u64*)packet;
        const unsigned char* scale = (const unsigned char*)packet + E;
        r.codes = MODE == 0 ? code[e / 8] : (MODE == 1 ? ld_wt(code + e / 8) : ld_sys(code + e / 8));
        r.sbyte = MODE == 0 ? scale[e / 32] : (MODE == 1 ? ld_wt(scale + e / 32) : ld_sys(scale + e / 32));
    }
    static __device__ __forceinline__ h16x8 recv_make(const Recv& r, size_t) { return mxi8_recv(r.codes, r.sbyte); }
};

// one of the two instantiations of a kernel template: the element type; cfx_host.h's LAUNCH with the caller's `ctx` and stream `s`
#define MXI8_LAUNCH(bf16, param, kid, kern, grid, ...) \
    do { \
        if (bf16) LAUNCH(ctx, kid, s, (kern<ElemBF16>), grid, dim3(256), 0, s, __VA_ARGS__); \
        else LAUNCH(ctx, kid, s, (kern<ElemF16>), grid, dim3(256), 0, s, __VA_ARGS__); \
    } while (0)
#endif
