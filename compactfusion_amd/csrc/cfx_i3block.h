// libcfx.so - the INT3_BLOCK codec's device code and policy type (I3bCodec): what cfx_i3block.hip (the family's kernels and launches) and
// cfx_capture.hip (the capturable instantiations of the layer launch) both compile: one policy type, so the same bits in both.
#ifndef CFX_I3BLOCK_H
#define CFX_I3BLOCK_H
#include "cfx_device.h"
#include "cfx_host.h"
#include "cfx_local.h"
#include "cfx_bscale.h"

// ---------------------------------------------------------------------------------------------------
// BINARY_BLOCK's lanes, exact block sum and scale (cfx_bscale.h: E % B == 0 and a workgroup starts at a multiple of 2048, so blocks never
// straddle rows of lanes).  A lane's 8 elements are 16 hi bits - sign << 1 | mag >> 1, element i of the lane at bits 2i (INT2's layout) -
// and 8 lo bits - mag & 1, element i at bit i (BINARY's layout); mag = 0..3 counts the thresholds 0.75 s, 1.5 s, 2.625 s that |d| exceeds.
// Two neighbouring lanes make one 32-bit hi word, a quad one 32-bit lo word (E % 64 == 0: all live or none).  A receiver adds
// +-{0.375, 1.125, 1.875, 3.375} s, each held to 65504.
// ---------------------------------------------------------------------------------------------------
// fp16( min( fp32(s) * k, 65504 ) ) as bits: the products are exact in fp32 (k has at most 5 significant bits, s 11), the one rounding is
// the conversion to fp16 - to nearest even, subnormals included; never inf
__device__ __forceinline__ unsigned i3b_scaled(float s, float k) { return hbits((h16)fminf(s * k, 65504.0f)); }

// 16 hi bits + 8 lo bits + the block's scale (fp16 bits, never negative, never above 65504) -> what a receiver adds.  The four levels once
// per unit.
__device__ __forceinline__ h16x8 i3b_recv(unsigned hi, unsigned lo, unsigned sbits) {
    const float s = (float)hfrom((u16)sbits);
    const unsigned l0 = i3b_scaled(s, 0.375f), l1 = i3b_scaled(s, 1.125f), l2 = i3b_scaled(s, 1.875f), l3 = i3b_scaled(s, 3.375f);
    u16x8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned c = hi >> (2 * i);
        const bool b0 = (lo >> i) & 1u;
        const unsigned l = (c & 1u) ? (b0 ? l3 : l2) : (b0 ? l1 : l0);
        r[i] = (u16)(l | ((c & 2u) ? 0u : 0x8000u));
    }
    return __builtin_bit_cast(h16x8, r);
}

// bb_compress_unit's contract (every lane of a wave calls it, live or not) for the 3-bit codes
template <class El, int B, bool WT>
__device__ __forceinline__ void i3b_compress_unit(const cfx_comp_item& it, size_t e, size_t E, bool live, int flags, h16x8 xv, h16x8 bv) {
    const bool has_base = it.base != nullptr;
    h16* nb = (h16*)it.new_base;
    unsigned* hiw = (unsigned*)it.packet;
    unsigned* low = (unsigned*)((unsigned char*)it.packet + E / 4);
    u16* scale = (u16*)((unsigned char*)it.packet + E / 4 + E / 8);
    const bool upd = (flags & CFX_FLAG_UPDATE_CACHE) && nb;
    const bool ef = !(flags & CFX_FLAG_NO_EF);
    h16x8 d;
    if constexpr (El::bf16) d = el_diff<El>(xv, has_base ? bv : (h16x8)(h16)0);
    else d = has_base ? (xv - bv) : xv;
    const u16x8 db = __builtin_bit_cast(u16x8, d);
    u64 units = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) units += habs_units(db[i]);
    const unsigned sbits = hbits(mean16(bb_block_sum<B>(units), B));
    // the three thresholds once per unit; |d| > t on the magnitude bits: both are finite and not negative, so fp16 order is integer order
    const float s = (float)hfrom((u16)sbits);
    const unsigned t0 = i3b_scaled(s, 0.75f), t1 = i3b_scaled(s, 1.5f), t2 = i3b_scaled(s, 2.625f);
    unsigned hi = 0, lo = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned a = db[i] & 0x7FFFu;
        const unsigned mag = (unsigned)(a > t0) + (unsigned)(a > t1) + (unsigned)(a > t2);
        hi |= (((unsigned)(d[i] >= (h16)0) << 1) | (mag >> 1)) << (2 * i);
        lo |= (mag & 1u) << i;
    }
    // the hi bits of two neighbouring lanes (16 elements) in one 32-bit store
    unsigned hw = (unsigned)__builtin_amdgcn_update_dpp(0, (int)hi, 0xA0, 0xf, 0xf, true);           // quad_perm [0,0,2,2]
    hw |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)hi, 0xF5, 0xf, 0xf, true) << 16;             // quad_perm [1,1,3,3]
    // the lo bytes of a quad (32 elements) in one 32-bit store
    unsigned lw = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0x00, 0xf, 0xf, true);           // quad_perm [0,0,0,0]
    lw |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0x55, 0xf, 0xf, true) << 8;              // quad_perm [1,1,1,1]
    lw |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0xAA, 0xf, 0xf, true) << 16;             // quad_perm [2,2,2,2]
    lw |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0xFF, 0xf, 0xf, true) << 24;             // quad_perm [3,3,3,3]
    // the scales of 2 neighbouring blocks (B / 4 lanes) in one 32-bit store; a tensor's last block where their number is odd: a 16-bit one
    const unsigned sw = sbits | ((unsigned)__shfl_down((int)sbits, B / 8, 64) << 16);
    if (!live) return;
    if ((threadIdx.x & 1) == 0) st_put<WT>(&hiw[e / 16], hw);
    if ((threadIdx.x & 3) == 0) st_put<WT>(&low[e / 32], lw);
    if ((threadIdx.x & (B / 4 - 1)) == 0) {
        if (e + 2 * B <= E) st_put<WT>((unsigned*)(scale + e / B), sw);
        else st_put<WT>(scale + e / B, (u16)sbits);
    }
    if (upd) st8nt(nb + e, ef ? el_state<El>(has_base, bv, i3b_recv(hi, lo, sbits)) : xv);
}

// The 3-bit codec as cfx_local.h's skeleton sees it: a receiver's 8 elements are one 16-bit hi word, one lo byte and the block's scale
template <class E_, int B> struct I3bCodec {
    using El = E_;
    static constexpr bool ALL_LANES = true;
    static constexpr bool MAKE_FIRST = false;
    static constexpr int IN_FLIGHT = 4;                   // eight three-word records: 85 / 89 VGPRs (fp16 / bf16), 5 waves a SIMD; four: 69, 7 waves
    struct Recv { u16 hi; unsigned char lo; u16 sbits; };
    template <bool WT>
    static __device__ __forceinline__ void compress_unit(const cfx_comp_item& it, size_t e, size_t E, bool live, int flags, h16x8 xv, h16x8 bv) {
        i3b_compress_unit<El, B, WT>(it, e, E, live, flags, xv, bv);
    }
    template <int MODE>
    static __device__ __forceinline__ void recv_load(Recv& r, const void* packet, size_t E, size_t e) {
        const u16* hi = (const u16*)packet;
        const unsigned char* lo = (const unsigned char*)packet + E / 4;
        const u16* scale = (const u16*)(lo + E / 8);
        r.hi = MODE == 0 ? hi[e / 8] : (MODE == 1 ? ld_wt(hi + e / 8) : ld_sys(hi + e / 8));
        r.lo = MODE == 0 ? lo[e / 8] : (MODE == 1 ? ld_wt(lo + e / 8) : ld_sys(lo + e / 8));
        r.sbits = MODE == 0 ? scale[e / B] : (MODE == 1 ? ld_wt(scale + e / B) : ld_sys(scale + e / B));
    }
    static __device__ __forceinline__ h16x8 recv_make(const Recv& r, size_t) { return i3b_recv(r.hi, r.lo, r.sbits); }
};
#endif
