// libcfx.so - the INT2_BLOCK codec's device code and policy type (I2bCodec): what cfx_i2block.hip (the family's kernels and launches) and
// cfx_capture.hip (the capturable instantiations of the layer launch) both compile: one policy type, so the same bits in both.
#ifndef CFX_I2BLOCK_H
#define CFX_I2BLOCK_H
#include "cfx_device.h"
#include "cfx_host.h"
#include "cfx_local.h"
#include "cfx_bscale.h"

// ---------------------------------------------------------------------------------------------------
// BINARY_BLOCK's lanes, exact block sum and scale (cfx_bscale.h: E % B == 0 and a workgroup starts at a multiple of 2048, so blocks never
// straddle rows of lanes).  A lane's 8 elements are 16 code bits - code = sign << 1 | (|d| > s), element i of the lane at bits 2i (INT2's
// layout: element j of a row at bits 2 (j % 4) of byte j / 4) - and two neighbouring lanes make one 32-bit code word (E % 64 == 0: both
// live or neither).  A receiver adds +-0.5 s or +-min(2 s, 65504).
// ---------------------------------------------------------------------------------------------------
// 16 code bits + the block's scale (fp16 bits, never negative, never above 65504) -> what a receiver adds.  The two levels once per unit:
// 0.5 s is one fp16 product (round to nearest even where s is subnormal or below 2^-13: 2^-24 gives 0), 2 s goes through fp32 and is held
// to 65504 before its - then exact - rounding to fp16: a block whose mean is past 32752 never sends inf into a state.
__device__ __forceinline__ h16x8 i2b_recv(unsigned codes, unsigned sbits) {
    const h16 s = hfrom((u16)sbits);
    const unsigned small = hbits(s * (h16)0.5f);
    const unsigned large = hbits((h16)fminf(2.0f * (float)s, 65504.0f));
    u16x8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned c = codes >> (2 * i);
        r[i] = (u16)(((c & 1u) ? large : small) | ((c & 2u) ? 0u : 0x8000u));
    }
    return __builtin_bit_cast(h16x8, r);
}

// bb_compress_unit's contract (every lane of a wave calls it, live or not) for the 2-bit codes
template <class El, int B, bool WT>
__device__ __forceinline__ void i2b_compress_unit(const cfx_comp_item& it, size_t e, size_t E, bool live, int flags, h16x8 xv, h16x8 bv) {
    const bool has_base = it.base != nullptr;
    h16* nb = (h16*)it.new_base;
    unsigned* codew = (unsigned*)it.packet;
    u16* scale = (u16*)((unsigned char*)it.packet + E / 4);
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
    // |d| > s on the magnitude bits: both are finite and not negative, so fp16 order is integer order
    unsigned codes = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        codes |= (((unsigned)(d[i] >= (h16)0) << 1) | (unsigned)((db[i] & 0x7FFFu) > sbits)) << (2 * i);
    // the codes of two neighbouring lanes (16 elements) in one 32-bit store
    unsigned w = (unsigned)__builtin_amdgcn_update_dpp(0, (int)codes, 0xA0, 0xf, 0xf, true);         // quad_perm [0,0,2,2]
    w |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)codes, 0xF5, 0xf, 0xf, true) << 16;           // quad_perm [1,1,3,3]
    // the scales of 2 neighbouring blocks (B / 4 lanes) in one 32-bit store; a tensor's last block where their number is odd: a 16-bit one
    const unsigned sw = sbits | ((unsigned)__shfl_down((int)sbits, B / 8, 64) << 16);
    if (!live) return;
    if ((threadIdx.x & 1) == 0) st_put<WT>(&codew[e / 16], w);
    if ((threadIdx.x & (B / 4 - 1)) == 0) {
        if (e + 2 * B <= E) st_put<WT>((unsigned*)(scale + e / B), sw);
        else st_put<WT>(scale + e / B, (u16)sbits);
    }
    if (upd) st8nt(nb + e, ef ? el_state<El>(has_base, bv, i2b_recv(codes, sbits)) : xv);
}

// The 2-bit codec as cfx_local.h's skeleton sees it: a receiver's 8 elements are one 16-bit code word and the block's scale
template <class E_, int B> struct I2bCodec {
    using El = E_;
    static constexpr bool ALL_LANES = true;
    static constexpr bool MAKE_FIRST = false;
    static constexpr int IN_FLIGHT = LOCAL_DU;
    struct Recv { u16 codes; u16 sbits; };
    template <bool WT>
    static __device__ __forceinline__ void compress_unit(const cfx_comp_item& it, size_t e, size_t E, bool live, int flags, h16x8 xv, h16x8 bv) {
        i2b_compress_unit<El, B, WT>(it, e, E, live, flags, xv, bv);
    }
    template <int MODE>
    static __device__ __forceinline__ void recv_load(Recv& r, const void* packet, size_t E, size_t e) {
        const u16* codes = (const u16*)packet;
        const u16* scale = (const u16*)((const unsigned char*)packet + E / 4);
        r.codes = MODE == 0 ? codes[e / 8] : (MODE == 1 ? ld_wt(codes + e / 8) : ld_sys(codes + e / 8));
        r.sbits = MODE == 0 ? scale[e / B] : (MODE == 1 ? ld_wt(scale + e / B) : ld_sys(scale + e / B));
    }
    static __device__ __forceinline__ h16x8 recv_make(const Recv& r, size_t) { return i2b_recv(r.codes, r.sbits); }
};
#endif
