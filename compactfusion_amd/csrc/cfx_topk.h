// libcfx.so - the 1:m top-1 sparsifier's device code and policy type (TopkCodec) and the choice among its instantiations: what cfx_topk.hip (the family's kernels and launches) and
// cfx_capture.hip (the capturable instantiations of the layer launch) both compile: one policy type, so the same bits in both.
#ifndef CFX_TOPK_H
#define CFX_TOPK_H
#include "cfx_device.h"
#include "cfx_host.h"
#include "cfx_local.h"

// ---------------------------------------------------------------------------------------------------
// 1:m block top-1 sparsifier on the flat (-1, 1024) view       compress_topk.py:44-105, :128-163
// One lane owns 8 consecutive flat elements.  Half-blocks of m <= 8 live inside a lane; m = 16 spans two lanes.
// ---------------------------------------------------------------------------------------------------
// The 8 elements at flat offset e of one tensor (whole waves call it together: the 16-wide blocks talk to their neighbour lanes).
// WT: the packet goes out write-through - workgroups of the same launch read it (k_topk_layer).
// Magnitude v beats the best so far b in tl.argmax's order (compress_topk.py:82-83): larger, or a NaN against a number - NaN is above
// everything, +inf included, and a later NaN does not replace an earlier one (the first maximum / the first NaN wins).
__device__ __forceinline__ bool topk_beats(h16 v, h16 b) { return v > b || (v != v && b == b); }
template <int M, bool WT>
__device__ __forceinline__ void topk_compress_unit(const cfx_comp_item& it, size_t e, size_t E, int flags, h16x8 xv, h16x8 bv) {
    const h16* x = (const h16*)it.x;
    const h16* base = (const h16*)it.base;
    h16* nb = (h16*)it.new_base;
    u16* val = (u16*)it.packet;
    unsigned char* idx = (unsigned char*)(val + E / M);
    const bool upd = (flags & CFX_FLAG_UPDATE_CACHE) && nb;
    const bool ef = !(flags & CFX_FLAG_NO_EF);
    const h16x8 d = xv - bv;                          // (x and base loaded by the caller: several units' loads in flight at once)
    const h16x8 a = habs8(d);
    unsigned keep = 0;   // bit i set = element i survives
    if constexpr (M <= 8) {
        constexpr int HB = 8 / M;   // half-blocks per lane
        unsigned sel[HB];
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            int best = 0;
            h16 bestv = a[hb * M];
#pragma unroll
            for (int i = 1; i < M; ++i) {
                const h16 v = a[hb * M + i];
                if (topk_beats(v, bestv)) { bestv = v; best = i; }     // strict: first maximum wins (tl.argmax)
            }
            sel[hb] = best;
            keep |= 1u << (hb * M + best);
            st_put<WT>(&val[e / M + hb], hbits(d[hb * M + best]));
        }
        if constexpr (M == 8) {
            const unsigned other = __shfl_xor(sel[0], 1, 64);
            if ((threadIdx.x & 1) == 0) st_put<WT>(&idx[e / 16], (unsigned char)((sel[0] << 4) | other));
        } else {
#pragma unroll
            for (int bk = 0; bk < HB / 2; ++bk) st_put<WT>(&idx[e / (2 * M) + bk], (unsigned char)((sel[2 * bk] << 4) | sel[2 * bk + 1]));
        }
    } else {   // M == 16: half-block = lanes (2k, 2k+1); block = 4 lanes
        int best = 0;
        h16 bestv = a[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) if (topk_beats(a[i], bestv)) { bestv = a[i]; best = i; }
        const int odd = threadIdx.x & 1;
        const unsigned pb = hbits(bestv);
        const unsigned ob = __shfl_xor(pb, 1, 64);
        const int oi = __shfl_xor(best, 1, 64);
        // lower lane wins ties (its elements come first)
        const bool mine = odd ? topk_beats(hfrom((u16)pb), hfrom((u16)ob)) : !topk_beats(hfrom((u16)ob), hfrom((u16)pb));
        const int selidx = mine ? (best + 8 * odd) : (oi + 8 * (1 - odd));   // index within the 16-wide half-block
        if (mine) { keep |= 1u << best; st_put<WT>(&val[e / 16], hbits(d[best])); }
        const int other = __shfl_xor(selidx, 2, 64);
        if ((threadIdx.x & 3) == 0) st_put<WT>(&idx[e / 32], (unsigned char)((selidx << 4) | other));
    }
    if (upd) {
        h16x8 o;
        if (ef) {
            h16x8 recv;
#pragma unroll
            for (int i = 0; i < 8; ++i) recv[i] = ((keep >> i) & 1u) ? d[i] : (h16)0;
            o = base ? (bv + recv) : recv;
        } else o = xv;
        st8nt(nb + e, o);
    }
}

// The codec as cfx_local.h's skeleton sees it.  What a receiver adds for the 8 elements at flat offset e comes from a packet read with plain
// loads (MODE 0), with L2-bypassing loads (1: another workgroup of this launch wrote it) or with system-scope loads (2: another GPU did).
// Every value / index byte the lane needs is loaded once; load and use are apart so that a caller can put several units' loads in flight
// (the compiler keeps atomic loads in program order: a use between two of them is a round trip each).
template <int M> struct TopkCodec {
    using El = ElemF16;
    static constexpr bool ALL_LANES = false;              // E % 1024 == 0: whole waves leave, the 16-wide blocks' neighbour lanes with them
    static constexpr bool MAKE_FIRST = true;
    static constexpr int HB = M <= 8 ? 8 / M : 1;         // half-blocks the lane's 8 elements touch
    static constexpr int NB = HB >= 2 ? HB / 2 : 1;       // index bytes (two half-blocks a byte)
    struct Recv { u16 v[HB]; unsigned char by[NB]; };
    // the packet words of as many units in flight at once as 16 small registers hold
    static constexpr int IN_FLIGHT = HB + NB <= 2 ? LOCAL_DU : (HB + NB <= 4 ? 4 : (HB + NB <= 8 ? 2 : 1));
    template <bool WT>
    static __device__ __forceinline__ void compress_unit(const cfx_comp_item& it, size_t e, size_t E, bool, int flags, h16x8 xv, h16x8 bv) {
        topk_compress_unit<M, WT>(it, e, E, flags, xv, bv);
    }
    template <int MODE>
    static __device__ __forceinline__ void recv_load(Recv& r, const void* packet, size_t E, size_t e) {
        const u16* val = (const u16*)packet;
        const unsigned char* idx = (const unsigned char*)(val + E / M);
        const size_t hb0 = e / M;
#pragma unroll
        for (int k = 0; k < HB; ++k) r.v[k] = MODE == 0 ? val[hb0 + k] : (MODE == 1 ? ld_wt(val + hb0 + k) : ld_sys(val + hb0 + k));
#pragma unroll
        for (int k = 0; k < NB; ++k)
            r.by[k] = MODE == 0 ? idx[(hb0 >> 1) + k] : (MODE == 1 ? ld_wt(idx + (hb0 >> 1) + k) : ld_sys(idx + (hb0 >> 1) + k));
    }
    static __device__ __forceinline__ h16x8 recv_make(const Recv& r, size_t e) {
        const size_t hb0 = e / M;
        h16x8 recv;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = M <= 8 ? i / M : 0;
            const size_t hb = hb0 + k;
            const unsigned b = r.by[HB >= 2 ? k / 2 : 0];
            const unsigned sel = (hb & 1) ? (b & 15u) : (b >> 4);
            recv[i] = ((unsigned)((e + i) % M) == sel) ? hfrom(r.v[k]) : (h16)0;
        }
        return recv;
    }
};

// one of the five instantiations of a kernel template (param validated: 1, 2, 4, 8 or 16)
#define TOPK_LAUNCH(bf16, m, kid, kern, grid, ...) \
    do { \
        switch (m) { \
            case 1: LAUNCH(ctx, kid, s, kern<1>, grid, dim3(256), 0, s, __VA_ARGS__); break; \
            case 2: LAUNCH(ctx, kid, s, kern<2>, grid, dim3(256), 0, s, __VA_ARGS__); break; \
            case 4: LAUNCH(ctx, kid, s, kern<4>, grid, dim3(256), 0, s, __VA_ARGS__); break; \
            case 8: LAUNCH(ctx, kid, s, kern<8>, grid, dim3(256), 0, s, __VA_ARGS__); break; \
            default: LAUNCH(ctx, kid, s, kern<16>, grid, dim3(256), 0, s, __VA_ARGS__); break; \
        } \
    } while (0)
#endif
