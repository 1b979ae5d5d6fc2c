// libcfx.so - the BINARY_BLOCK codec's device code and policy type (BbCodec): what cfx_bblock.hip (the family's kernels and launches) and
// cfx_capture.hip (the capturable instantiations of the layer launch) both compile: one policy type, so the same bits in both.
#ifndef CFX_BBLOCK_H
#define CFX_BBLOCK_H
#include "cfx_device.h"
#include "cfx_host.h"
#include "cfx_local.h"
#include "cfx_bscale.h"

// ---------------------------------------------------------------------------------------------------
// One lane owns 8 consecutive flat elements (one 16-byte load of x, one of base, one byte of sign bits); a block is B / 8 = 4, 8 or 16
// neighbouring lanes - a DPP quad, half row or row (E % B == 0 and a workgroup starts at a multiple of 2048: blocks never straddle rows
// of lanes).  The block's scale is the exact integer sum of |d| in units of 2^-24 (habs_units), rounded once to fp32 and once to fp16
// (mean16): order-independent, so the lanes may add in any order.
// ---------------------------------------------------------------------------------------------------

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
    if ((threadIdx.x & 3) == 0) st_put<WT>(&bitw[e / 32], w);
    if ((threadIdx.x & (B / 4 - 1)) == 0) {
        if (e + 2 * B <= E) st_put<WT>((unsigned*)(scale + e / B), sw);
        else st_put<WT>(scale + e / B, (u16)sbits);
    }
    if (upd) st8nt(nb + e, ef ? el_state<El>(has_base, bv, bb_recv(bits, sbits)) : xv);
}

// The codec as cfx_local.h's skeleton sees it.  What a receiver needs for the 8 elements at flat offset e: their sign byte and the block's
// scale, from a packet read with plain loads (MODE 0), with L2-bypassing loads (1: another workgroup of this launch wrote it) or with
// system-scope loads (2: another GPU did).  Load and use are apart so that a caller can put several units' loads in flight.
template <class E_, int B> struct BbCodec {
    using El = E_;
    static constexpr bool ALL_LANES = true;
    static constexpr bool MAKE_FIRST = false;
    static constexpr int IN_FLIGHT = LOCAL_DU;            // every unit's packet words in flight at once, then the stores
    struct Recv { unsigned char bits; u16 sbits; };
    template <bool WT>
    static __device__ __forceinline__ void compress_unit(const cfx_comp_item& it, size_t e, size_t E, bool live, int flags, h16x8 xv, h16x8 bv) {
        bb_compress_unit<El, B, WT>(it, e, E, live, flags, xv, bv);
    }
    template <int MODE>
    static __device__ __forceinline__ void recv_load(Recv& r, const void* packet, size_t E, size_t e) {
        const unsigned char* bits = (const unsigned char*)packet;
        const u16* scale = (const u16*)(bits + E / 8);
        r.bits = MODE == 0 ? bits[e / 8] : (MODE == 1 ? ld_wt(bits + e / 8) : ld_sys(bits + e / 8));
        r.sbits = MODE == 0 ? scale[e / B] : (MODE == 1 ? ld_wt(scale + e / B) : ld_sys(scale + e / B));
    }
    static __device__ __forceinline__ h16x8 recv_make(const Recv& r, size_t) { return bb_recv(r.bits, r.sbits); }
};
#endif
