// libcfx.so - cfx_attn_fwd_blocks_hd (include/cfx.h): cfx_attn_fwd_blocks_var for the head dims BETWEEN 64 and 128 - D = 72, 80, 88, 96,
// 104, 112, 120 (PixArt / Latte's 72, HunyuanDiT's 88) - the attention of a rank's queries over all of a layer's K,V blocks in ONE launch.
//
// The walk is that of k_attn_fwd_blocks_var (csrc/cfx_attn_var.hip; csrc/cfx_attn.hip's head comment describes the MFMA operand layout,
// the LDS swizzle and the double buffer), operation for operation, at D = 128 with everything past the true D an EXACT ZERO that is never
// loaded: the scores take KS = ceil(D / 16) k-steps, O^T DB = ceil(D / 32) accumulator blocks.  A zero product adds nothing to an fp32
// sum and rounds nothing, so the result is, bit for bit, what cfx_attn_fwd_blocks_var returns on the same tensors zero-padded to D = 128
// with the same scale (tests/test_gpu_attn_hd.py holds it to that).  What differs from the 64 / 128 forms, and where each can go wrong:
//   - Q fragment: the 8 elements at column 16 ks + 8 hh >= D ARE zero, not loaded (for the last head of the last row they lie past q)
//   - staging: a tile is 64 D / 8 chunks of 16 bytes, not a whole number per thread (576 for 256 threads at D = 72): the last pass is
//     guarded, and a guarded-off thread neither loads nor writes
//   - LDS image: the D = 128 one unchanged - 256-byte pitch, tile_off<128>'s swizzle, 4 x 16 KiB (conflict-free by the bank rule as it
//     stands; at one wave a SIMD the LDS size does not set occupancy).  The chunks from D / 8 on that the MFMAs read (K: up to chunk
//     2 KS - 1; V, transposed: up to chunk 4 DB - 1) are never written by staging: they are zeroed ONCE in all four buffers, before the
//     first tile's barrier (LDS garbage may be NaN, and 0 x NaN is NaN)
//   - output: D / 8 chunks a row; accumulator rows d >= D (products of V's zero columns) are never staged or stored
// A translation unit and a source list (build.py's ATTN_HD_SRC) of its own: cfx_attn.hip and cfx_attn_var.hip stay byte for byte what
// they were, their kernels pinned register by register (tests/test_attn_fwd_f64.py, tests/test_attn_var_f64.py).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "cfx.h"
#include "cfx_internal.h"
#include "cfx_device.h"

struct AttnHdTabs {
    const u16* k[CFX_ATTN_MAX_BLOCKS];
    const u16* v[CFX_ATTN_MAX_BLOCKS];
    int sk[CFX_ATTN_MAX_BLOCKS];                          // keys of block i
};

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

#define LDS_PTR(T, p) ((__attribute__((address_space(3))) T*)(p))

constexpr int PITCH = 256, NCH = 16, TILEB = 64 * PITCH;              // the D = 128 image: 16 chunks a row, 16 KiB a tile

// byte offset of 16-byte chunk `ch` (0 .. 15) of row `row` in a [64][128] 16-bit tile image: csrc/cfx_attn.hip's XOR swizzle for D = 128
__device__ __forceinline__ int tile_off(int row, int ch) {
    return PITCH * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

template <class E>
__device__ __forceinline__ f32x16 mfma16(u32x4 a, u32x4 b, f32x16 c) {
    if constexpr (E::bf16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
}

// two fp32 -> one word of two elements, round to nearest even (the packed converts)
template <class E>
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    const f32x2 p = {lo, hi};
    if constexpr (E::bf16) return f32_bf2(p);
    else return __builtin_bit_cast(unsigned, __builtin_convertvector(p, h16x2));
}

}  // namespace

// T: the key tiles of all blocks, sum_i ceil(t.sk[i] / 64) (the host's sum: every workgroup would form the same one)
template <class E, int D, int NW>
__global__ __launch_bounds__(NW * 64) void k_attn_fwd_blocks_hd(AttnHdTabs t, int T, const u16* __restrict__ q, u16* __restrict__ out,
                                                                float* __restrict__ lse, int Sq, int H, int nqt, float scale) {
    constexpr int NT = NW * 64, CH = D / 8, NC = 64 * CH, PER = (NC + NT - 1) / NT, KS = (D + 15) / 16, DB = (D + 31) / 32;
    constexpr int PADC = (2 * KS > 4 * DB ? 2 * KS : 4 * DB) - CH, OPER = (32 * CH + 63) / 64;     // PADC: chunks read but never staged
    static_assert(D % 8 == 0 && D > 64 && D < 128, "head dims 72 .. 120 in steps of 8: a row is whole 16-byte chunks");
    static_assert(PER >= 1 && (PER - 1) * NT < NC && NC <= PER * NT, "every pass but the last is whole; the last is guarded");
    static_assert(2 * KS <= NCH && 4 * DB <= NCH && CH <= 2 * KS && CH <= 4 * DB, "the MFMAs read chunks of the image only, all of D among them");
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TILEB];     // K tile x 2, V tile x 2; at the end the O rows of the workgroup
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    unsigned bid = blockIdx.x;
    const int qt = (int)(bid % (unsigned)nqt);
    bid /= (unsigned)nqt;
    const int h = (int)(bid % (unsigned)H), b = (int)(bid / (unsigned)H);
    const int q0 = qt * (32 * NW) + wave * 32;            // this wave's first query row
    const bool wave_on = q0 < Sq;                         // (wave-uniform) a wave wholly in the query tail only helps staging
    const size_t kv_row = (size_t)H * D;                  // elements between two keys of a block (and between two query rows)

    // this lane's query row as the B operand of S^T = K Q^T: element j of k-step ks is Q[q0 + r][16 ks + 8 hh + j] - and zero from
    // column D on: never loaded (the address of a masked fragment is that of the row's first one)
    u32x4 qf[KS];
    {
        const bool ok = q0 + r < Sq;
        const u16* qp = q + ((size_t)b * Sq + (size_t)(ok ? q0 + r : 0)) * kv_row + (size_t)h * D;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bool in = ok && 16 * ks + 8 * hh < D;
            qf[ks] = in ? *reinterpret_cast<const u32x4*>(qp + (in ? 16 * ks + 8 * hh : 0)) : (u32x4)(0u);
        }
    }

    u32x4 sk_[PER], sv_[PER];                             // the tile in flight, global -> registers -> LDS
    // tile kt of block blk, whose length is len: the batch stride and the row mask are that block's own
    auto stage_load = [&](int blk, int kt, int len) {
        const size_t kv_base = (size_t)b * (size_t)len * kv_row + (size_t)h * D;
        const u16* kp = t.k[blk] + kv_base;
        const u16* vp = t.v[blk] + kv_base;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = i * NT + tid, row = c / CH, ch = c % CH, key = kt * 64 + row;
            const bool ok = c < NC && key < len;          // (c < NC: the guarded last pass; true at compile time on the others)
            const size_t o = (size_t)(ok ? key : 0) * kv_row + (size_t)ch * 8;
            sk_[i] = ok ? *reinterpret_cast<const u32x4*>(kp + o) : (u32x4)(0u);
            sv_[i] = ok ? *reinterpret_cast<const u32x4*>(vp + o) : (u32x4)(0u);
        }
    };
    auto stage_write = [&](int buf) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = i * NT + tid, row = c / CH, ch = c % CH;
            if (c < NC) {                                 // (row < 64: inside the tile image)
                const int o = tile_off(row, ch);
                *reinterpret_cast<u32x4*>(smem + buf * TILEB + o) = sk_[i];
                *reinterpret_cast<u32x4*>(smem + (2 + buf) * TILEB + o) = sv_[i];
            }
        }
    };

    // chunks CH .. CH + PADC - 1 of every row of the four tile images - what the MFMAs read past D (K up to chunk 2 KS - 1, V up to
    // 4 DB - 1; none at D = 96): zero, once - staging never writes them.  Disjoint from what stage_write(0) writes; both are complete at
    // the first barrier, before any read.
    if constexpr (PADC > 0) {
        for (int c = tid; c < 4 * 64 * PADC; c += NT) {
            const int img = c / (64 * PADC), rc = c % (64 * PADC), row = rc / PADC, ch = CH + rc % PADC;
            *reinterpret_cast<u32x4*>(smem + img * TILEB + tile_off(row, ch)) = (u32x4)(0u);
        }
    }

    f32x16 o_[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) o_[db] = (f32x16)(0.0f);
    float m = -INFINITY, l = 0.0f;                        // l: this lane's HALF of the row's sum (its 16 keys of every half tile)

    // transposed-read lane geometry: lane 4 qq + pp of the 16-lane group g supplies row qq, columns 4 pp .. 4 pp + 3 of the group's block
    const int g = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;

    int cur = 0, blk = 0, kt = 0;
    int len = t.sk[0];                                    // keys of the block being scored (wave-uniform, as blk and kt are)
    stage_load(0, 0, len);
    stage_write(0);
    __syncthreads();
    // Every load so far - the Q fragments, tile 0 - has landed before the loop: stage_write's guarded pass waits for its loads INSIDE a
    // branch, which leaves them pending on the path around it as far as the compiler's wait insertion can tell, and with that state at
    // the loop's head the first MFMA of EVERY tile waited for vmcnt(0) - for the next tile's loads, just issued.  One wait here, outside
    // the loop, and the loads of the tile in flight overlap the tile being scored again.
    __builtin_amdgcn_s_waitcnt(0);
    for (int it = 0; it < T; ++it) {
        int nblk = blk, nkt = kt + 1, nlen = len;
        const bool more = it + 1 < T;
        if (nkt * 64 >= len) {                            // the block's last tile was this one
            nkt = 0;
            ++nblk;
            if (more) nlen = t.sk[nblk];                  // (not past the table: after the last tile there is no next block)
        }
        if (more) stage_load(nblk, nkt, nlen);            // masked against the length of the block it reads: the NEXT tile's
        if (wave_on) {
            const unsigned char* kb = smem + cur * TILEB;
            const unsigned char* vb = smem + (2 + cur) * TILEB;
            f32x16 s_[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                s_[u] = (f32x16)(0.0f);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const u32x4 kf = *reinterpret_cast<const u32x4*>(kb + tile_off(32 * u + r, 2 * ks + hh));
                    s_[u] = mfma16<E>(kf, qf[ks], s_[u]);
                }
            }
            // scores: the fp32 sums times the scale, one rounding; keys past the END OF THIS BLOCK are -inf (their K, V rows were staged as zeros)
            const int kleft = len - kt * 64;              // valid keys of this tile, >= 1
            float mx = -INFINITY;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float x = s_[u][i] * scale;
                    if (kleft < 64 && 32 * u + (i & 3) + 8 * (i >> 2) + 4 * hh >= kleft) x = -INFINITY;
                    s_[u][i] = x;
                    mx = fmaxf(mx, x);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m, mx);
            const float mu = mn == -INFINITY ? 0.0f : mn;                 // (an all-masked row so far: exp(-inf - 0) = 0, never -inf - -inf)
            const float alpha = __expf(m - mu);                           // 0 at the first tile (m = -inf), 1 when the maximum stands
            m = mn;
            float ts = 0.0f;
            unsigned pw[2][8];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int i = 0; i < 16; i += 2) {
                    const float p0 = __expf(s_[u][i] - mu), p1 = __expf(s_[u][i + 1] - mu);
                    ts = (ts + p0) + p1;                                  // l from the UNROUNDED p, fp32 adds in register order
                    pw[u][i >> 1] = pack2<E>(p0, p1);
                }
            l = l * alpha + ts;
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {         // (a product by 1 changes nothing: skipped for the whole wave)
#pragma unroll
                for (int db = 0; db < DB; ++db) o_[db] *= alpha;
            }
            // O^T += V^T P^T: k-step kk = keys 16 kk .. 16 kk + 15 of the tile, P's accumulator rows 8 (kk & 1) .. + 7 of half tile kk >> 1
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int ch = 4 * db + 2 * (g & 1) + (pp >> 1);
                    const int row0 = 16 * kk + 4 * hh + qq;
                    const i16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(i16x4, vb + tile_off(row0, ch) + 8 * (pp & 1)));
                    const i16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(i16x4, vb + tile_off(row0 + 8, ch) + 8 * (pp & 1)));
                    const u32x2 w0 = __builtin_bit_cast(u32x2, a0), w1 = __builtin_bit_cast(u32x2, a1);
                    const u32x4 vf = {w0[0], w0[1], w1[0], w1[1]};
                    const int u = kk >> 1, s4 = 4 * (kk & 1);
                    const u32x4 pf = {pw[u][s4], pw[u][s4 + 1], pw[u][s4 + 2], pw[u][s4 + 3]};
                    o_[db] = mfma16<E>(vf, pf, o_[db]);
                }
        }
        if (more) stage_write(cur ^ 1);
        __syncthreads();
        cur ^= 1;
        blk = nblk;
        kt = nkt;
        len = nlen;
    }

    // out = O / l (one division, one rounding to the element type), staged as this wave's 32 rows of 256 bytes; lse = m + log l
    const float lt = l + __shfl_xor(l, 32, 64);
    unsigned char* ob = smem + wave * 32 * PITCH;
    if (wave_on) {
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            // accumulator rows 4 g4 .. 4 g4 + 3 are d = 32 db + 8 g4 + 4 hh + (0 .. 3): 8 bytes of row r's chunk 4 db + g4 - a chunk at or
            // past D / 8 holds rows d >= D only: not staged
            if (4 * db + g4 < CH) {
                const u32x2 w = {pack2<E>(o_[db][4 * g4] / lt, o_[db][4 * g4 + 1] / lt), pack2<E>(o_[db][4 * g4 + 2] / lt, o_[db][4 * g4 + 3] / lt)};
                *reinterpret_cast<u32x2*>(ob + r * PITCH + 16 * ((4 * db + g4) ^ (r & (NCH - 1))) + 8 * hh) = w;
            }
        }
    }
    __syncthreads();
    if (wave_on) {
#pragma unroll
        for (int i = 0; i < OPER; ++i) {
            const int c = i * 64 + lane, row = c / CH, ch = c % CH;
            if (c < 32 * CH && q0 + row < Sq)             // (c < 32 CH: the guarded last pass)
                *reinterpret_cast<u32x4*>(out + ((size_t)b * Sq + (size_t)(q0 + row)) * kv_row + (size_t)h * D + (size_t)ch * 8) =
                    *reinterpret_cast<const u32x4*>(ob + row * PITCH + 16 * (ch ^ (row & (NCH - 1))));
        }
        if (hh == 0 && q0 + r < Sq) lse[((size_t)b * Sq + (size_t)(q0 + r)) * H + h] = m + logf(lt);
    }
}

extern "C" {

int cfx_attn_fwd_blocks_hd(cfx_ctx* ctx, int n, const void* q, const void* const* ks, const void* const* vs, const int* sks,
                           int B, int Sq, int H, int D, float softmax_scale, unsigned flags, void* out, void* lse, void* stream) {
    if (!ctx || !q || !ks || !vs || !sks || !out || !lse) return fail(ctx, CFX_ERR_NULL, "attn_fwd_blocks_hd: null pointer");
    const int nt = n < 0 ? 0 : (n > CFX_ATTN_MAX_BLOCKS ? CFX_ATTN_MAX_BLOCKS : n);
    for (int i = 0; i < nt; ++i)
        if (!ks[i] || !vs[i]) return fail(ctx, CFX_ERR_NULL, "attn_fwd_blocks_hd: null pointer in a block table");
    if (flags & ~(unsigned)CFX_ELEM_BF16) return fail(ctx, CFX_ERR_CODEC, "attn_fwd_blocks_hd: unknown flag bit (CFX_ELEM_BF16 only)");
    if (n < 1 || n > CFX_ATTN_MAX_BLOCKS) return fail(ctx, CFX_ERR_SHAPE, "attn_fwd_blocks_hd: 1 to 16 blocks");
    if (B <= 0 || Sq <= 0 || H <= 0 || D < 72 || D > 120 || (D & 7))
        return fail(ctx, CFX_ERR_SHAPE, "attn_fwd_blocks_hd: positive sizes, head dim 72, 80, 88, 96, 104, 112 or 120 (64 and 128: cfx_attn_fwd_blocks_var)");
    int T = 0;                                                        // at most 16 x 2^25 tiles
    for (int i = 0; i < n; ++i) {
        if (sks[i] <= 0) return fail(ctx, CFX_ERR_SHAPE, "attn_fwd_blocks_hd: every block needs at least one key");
        T += (int)(((long long)sks[i] + 63) >> 6);
    }
    const int qtile = ctx->attn_qtile ? ctx->attn_qtile : 128;        // query rows per workgroup, as cfx_attn_fwd_blocks: cfx_set_attn_qtile
    const size_t nqt = ((size_t)Sq + qtile - 1) / qtile;
    if (nqt * (size_t)H * (size_t)B > 0x7fffffffu) return fail(ctx, CFX_ERR_SHAPE, "attn_fwd_blocks_hd: too many workgroups for one launch");
    if (!isfinite(softmax_scale) || !(softmax_scale > 0.0f)) return fail(ctx, CFX_ERR_SHAPE, "attn_fwd_blocks_hd: the scale must be finite and positive");
    if (!AL16(q) || !AL16(out) || !AL16(lse)) return fail(ctx, CFX_ERR_ALIGN, "attn_fwd_blocks_hd: pointers must be 16-byte aligned");
    for (int i = 0; i < n; ++i)
        if (!AL16(ks[i]) || !AL16(vs[i])) return fail(ctx, CFX_ERR_ALIGN, "attn_fwd_blocks_hd: pointers must be 16-byte aligned");
    if (ctx->gate_err && *(volatile unsigned*)ctx->gate_err) return fail(ctx, CFX_ERR_GATE, "attn_fwd_blocks_hd: an earlier flag / gate wait on this context timed out (cfx_gate_errors)");
    hipStream_t s = (hipStream_t)stream;
    AttnHdTabs t;
    for (int i = 0; i < CFX_ATTN_MAX_BLOCKS; ++i) {          // (unused entries repeat block 0: never read, never garbage)
        t.k[i] = (const u16*)ks[i < n ? i : 0];
        t.v[i] = (const u16*)vs[i < n ? i : 0];
        t.sk[i] = sks[i < n ? i : 0];
    }
    const dim3 grid((unsigned)(nqt * (size_t)H * (size_t)B));
#define ATTN_HD(E, DD, NW) \
    hipLaunchKernelGGL((k_attn_fwd_blocks_hd<E, DD, NW>), grid, dim3(NW * 64), 0, s, t, T, (const u16*)q, (u16*)out, (float*)lse, Sq, H, (int)nqt, softmax_scale)
#define ATTN_HD_D(E, NW) do { switch (D) { \
        case 72: ATTN_HD(E, 72, NW); break; case 80: ATTN_HD(E, 80, NW); break; case 88: ATTN_HD(E, 88, NW); break; \
        case 96: ATTN_HD(E, 96, NW); break; case 104: ATTN_HD(E, 104, NW); break; case 112: ATTN_HD(E, 112, NW); break; \
        default: ATTN_HD(E, 120, NW); break; } } while (0)
#define ATTN_HD_E(NW) do { if (flags & CFX_ELEM_BF16) ATTN_HD_D(ElemBF16, NW); else ATTN_HD_D(ElemF16, NW); } while (0)
    if (qtile == 64) ATTN_HD_E(2);
    else if (qtile == 256) ATTN_HD_E(8);
    else ATTN_HD_E(4);
#undef ATTN_HD_E
#undef ATTN_HD_D
#undef ATTN_HD
    const int rc = check_launch(ctx, "attn_fwd_blocks_hd launch");
    if (rc == CFX_OK) ++ctx->attn_launches;
    return rc;
}

}  // extern "C"
