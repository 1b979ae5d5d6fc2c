// libcfx.so - the block-local codecs' layer launch in ONE launch UNDER hipGraph CAPTURE (include/cfx.h "Stream capture",
// cfx_set_captured_layer): capturable instantiations of cfx_local.h's layer body, one per k_{topk,mx,bb,i2b,i3b,mxi8}_layer instantiation,
// with the same policy types (the families' headers) - the same compress_unit / recv_load / recv_make, so the same bits - and the pool of
// private gate slots they run on.  What differs from the eager body is where the numbers come from: the eager launch is TOLD the value its
// gate opens at (a launch argument the host advances with every launch - a replayed graph node would wait for numbers that have gone by);
// this one derives its launch number on the device from counters that only ever grow (cfx_capture_gate.h: the protocol and its arithmetic).
// A translation unit of its own, compiled into libcfx.so beside build.py's SRC: the kernels of SRC stay exactly what they were.
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
#include "cfx_local.h"
#include "cfx_capture_gate.h"
#include "cfx_topk.h"
#include "cfx_mx.h"
#include "cfx_bblock.h"
#include "cfx_i2block.h"
#include "cfx_i3block.h"
#include "cfx_mxint8.h"

static_assert(CFX_CAP_LINE == GATE_LINE && CFX_CAP_GATE_WORDS == GATE_BLOCK, "a slot's gate blocks are gate_wait's");
static_assert(CFX_CAP_MAX_ITEMS == CFX_MAX_BATCH, "one ticket line per reconstruction item");

struct CapturedLayerArgs {
    size_t E;
    int n_sw, n_st;             // S workgroups per own tensor / in all
    int n_dw;                   // D workgroups per reconstruction item
    int flags;
    unsigned* slot;             // the launch's private gate slot (cfx_capture_gate.h)
    int xgate;                  // exchange-layer op: group D waits for the slot's external gate (the in-launch exchange opens it)
    unsigned* err;
    long long timeout;
    int remote;
    P2PInline p2p;
};

__device__ __forceinline__ cfx_cap_u64 cap_draw(unsigned* counter) {
    return __hip_atomic_fetch_add((cfx_cap_u64*)counter, (cfx_cap_u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The body of k_*_layer_cap(BatchC batch, BatchD gated, CapturedLayerArgs a) for the codec `...`: cfx_local.h's LOCAL_LAYER (a macro for the
// reason given there) with the arrival and the wait of cfx_capture_gate.h.  Group S: lane 0's arrival returns `old`; the launch's last arriver
// opens the gate at cfx_cap_expect(r); workgroup 0's in-launch exchange takes both of its numbers from its own arrival.  Group D: lane 0
// draws its item's entry ticket BEFORE the state preload and looks at it only at the wait - the round trip sits under loads the workgroup
// issues anyway - and a wait that gives up has drawn it all the same.
#define CAPTURED_LAYER(batch, gated, a, ...) \
    using P = __VA_ARGS__; \
    int b = blockIdx.x; \
    if (b < a.n_st) { \
        const int z = b / a.n_sw, sw = b - z * a.n_sw; \
        const cfx_comp_item it = batch.it[z]; \
        h16x8 xv[LOCAL_SU], xb[LOCAL_SU]; \
        _Pragma("unroll") for (int u = 0; u < LOCAL_SU; ++u) { \
            const size_t e = (((size_t)sw * LOCAL_SU + u) * 256 + threadIdx.x) * 8, ec = e < a.E ? e : 0; \
            xv[u] = ld8nt((const h16*)it.x + ec); \
            xb[u] = it.base ? ld8nt((const h16*)it.base + ec) : (h16x8)(h16)0; \
        } \
        _Pragma("unroll") for (int u = 0; u < LOCAL_SU; ++u) { \
            const size_t e = (((size_t)sw * LOCAL_SU + u) * 256 + threadIdx.x) * 8; \
            if (P::ALL_LANES || e < a.E) P::template compress_unit<true>(it, e, a.E, e < a.E, a.flags, xv[u], xb[u]); \
        } \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
        __syncthreads(); \
        cfx_cap_u64 old = 0; \
        if (threadIdx.x == 0) { \
            old = cap_draw(a.slot); \
            if (cfx_cap_last(old, (unsigned)a.n_st)) { \
                const unsigned open_at = cfx_cap_expect(cfx_cap_launch(old, (unsigned)a.n_st)); \
                _Pragma("unroll") for (int x = 0; x < 8; ++x) st_wt(a.slot + (1 + x) * GATE_LINE, open_at); \
            } \
        } \
        if (b == 0 && a.p2p.own && (threadIdx.x >> 6) == 0) { \
            const cfx_cap_u64 mine = ((cfx_cap_u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(old >> 32)) << 32) | \
                                     (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)old); \
            const unsigned open_at = cfx_cap_expect(cfx_cap_launch(mine, (unsigned)a.n_st)); \
            p2p_exchange_inline(a.slot + GATE_LINE, open_at, 1, a.p2p, a.slot + CFX_CAP_GATE_WORDS, open_at, a.err); \
        } \
        return; \
    } \
    b -= a.n_st; \
    const int item = b / a.n_dw, dw = b - item * a.n_dw; \
    cfx_cap_u64 ticket = 0; \
    if (threadIdx.x == 0) ticket = cap_draw(a.slot + CFX_CAP_TICKET_OFF + item * CFX_CAP_LINE); \
    const cfx_decomp_item it = gated.it[item]; \
    const h16* base = (const h16*)it.base; \
    h16* out = (h16*)it.recon; \
    h16x8 bv[LOCAL_DU]; \
    _Pragma("unroll") for (int u = 0; u < LOCAL_DU; ++u) { \
        const size_t e = (((size_t)dw * LOCAL_DU + u) * 256 + threadIdx.x) * 8; \
        bv[u] = (base && e < a.E) ? ld8nt(base + e) : (h16x8)(h16)0; \
    } \
    const unsigned expect = cfx_cap_expect(cfx_cap_launch(ticket, (unsigned)a.n_dw));      /* (lane 0's is the one the wait reads) */ \
    if (!(a.xgate ? gate_wait<true>(a.slot + CFX_CAP_GATE_WORDS, expect, a.err, a.timeout) : gate_wait<false>(a.slot, expect, a.err, a.timeout))) return; \
    constexpr int G = P::IN_FLIGHT; \
    _Pragma("unroll") for (int u0 = 0; u0 < LOCAL_DU; u0 += G) { \
        typename P::Recv rr[G]; \
        _Pragma("unroll") for (int g = 0; g < G; ++g) { \
            const size_t e = (((size_t)dw * LOCAL_DU + u0 + g) * 256 + threadIdx.x) * 8, ec = e < a.E ? e : 0; \
            if (a.remote) P::template recv_load<2>(rr[g], it.packet, a.E, ec); \
            else P::template recv_load<1>(rr[g], it.packet, a.E, ec); \
        } \
        _Pragma("unroll") for (int g = 0; g < G; ++g) { \
            const size_t e = (((size_t)dw * LOCAL_DU + u0 + g) * 256 + threadIdx.x) * 8; \
            if (e < a.E) { \
                const h16x8 rv = P::recv_make(rr[g], e); \
                st8nt(out + e, el_state<typename P::El>(base != nullptr, bv[u0 + g], rv)); \
            } \
        } \
    }

// one capturable twin per instantiation of the families' k_*_layer
template <int M>
__global__ __launch_bounds__(256) void k_topk_layer_cap(BatchC batch, BatchD gated, CapturedLayerArgs a) { CAPTURED_LAYER(batch, gated, a, TopkCodec<M>); }
__global__ __launch_bounds__(256) void k_mx_layer_cap(BatchC batch, BatchD gated, CapturedLayerArgs a) { CAPTURED_LAYER(batch, gated, a, MxCodec); }
template <class El, int B>
__global__ __launch_bounds__(256) void k_bb_layer_cap(BatchC batch, BatchD gated, CapturedLayerArgs a) { CAPTURED_LAYER(batch, gated, a, BbCodec<El, B>); }
template <class El, int B>
__global__ __launch_bounds__(256) void k_i2b_layer_cap(BatchC batch, BatchD gated, CapturedLayerArgs a) { CAPTURED_LAYER(batch, gated, a, I2bCodec<El, B>); }
template <class El, int B>
__global__ __launch_bounds__(256) void k_i3b_layer_cap(BatchC batch, BatchD gated, CapturedLayerArgs a) { CAPTURED_LAYER(batch, gated, a, I3bCodec<El, B>); }
template <class El>
__global__ __launch_bounds__(256) void k_mxi8_layer_cap(BatchC batch, BatchD gated, CapturedLayerArgs a) { CAPTURED_LAYER(batch, gated, a, MxI8Codec<El>); }

// ---------------------------------------------------------------------------------------------------
// host side: the decision and the launch (called by the families' cfx_i_*_compress, cfx_local.h LOCAL_FAMILY_HOST), the pool (C-ABI)
// ---------------------------------------------------------------------------------------------------
// A validated compress call of a block-local family on a CAPTURING stream.  1: the capturable layer kernel is enqueued on a slot of the
// pool (an exchange-layer op: xg->taken / inline_done say so); 0: not this form - the caller enqueues the capturable sequence -; < 0: an
// error code.
int cfx_i_captured_layer(CompressCall& cc) {
    cfx_ctx* ctx = cc.ctx;
    CfxXGate* xg = cc.xg;
    if (!cc.capturing || !ctx->cap_n || !cc.n_gated || !ctx->gated_on || ctx->dev_probe) return 0;
    // an exchange-layer op: only the peer-to-peer form, whose exchange runs inside the launch (any other is a second stream's kernel that
    // would have to be told this launch's number)
    if (xg && !xg->p2p_own) return 0;
    if (stream_cu_count(ctx, cc.stream) < 128) return 0;
    if (!xg) {
        // loop-back: every reconstruction item reads one of this launch's packets
        for (int g_ = 0; g_ < cc.n_gated; ++g_) {
            bool mine = false;
            for (int i = 0; i < cc.batch; ++i) mine = mine || cc.gated[g_].packet == cc.items[i].packet;
            if (!mine) return 0;
        }
    }
    if (ctx->cap_used >= ctx->cap_n) return 0;
    if (ctx->gate_err && *(volatile unsigned*)ctx->gate_err)
        return fail(ctx, CFX_ERR_GATE, "compress: an earlier gate / flag wait on this context timed out (cfx_gate_errors reads and clears the count)");
    const size_t E = (size_t)cc.N * cc.C;
    CapturedLayerArgs a;
    memset(&a, 0, sizeof(a));
    a.E = E;
    a.n_sw = (int)((E / 8 + 256 * LOCAL_SU - 1) / (256 * LOCAL_SU));
    a.n_st = a.n_sw * cc.batch;
    a.n_dw = (int)((E / 8 + 256 * LOCAL_DU - 1) / (256 * LOCAL_DU));
    a.flags = cc.flags;
    a.slot = ctx->cap_pool + (size_t)ctx->cap_used * CFX_CAP_SLOT_WORDS;
    a.err = ctx->gate_err;
    a.timeout = ctx->gate_timeout;
    if (xg) {
        a.xgate = 1;
        a.remote = xg->remote;
        fill_p2p(ctx, xg, a.p2p);
        xg->taken = 1;
    }
    hipStream_t s = (hipStream_t)cc.stream;
    const dim3 grid((unsigned)(a.n_st + a.n_dw * cc.n_gated));
    switch (cc.codec) {
        case CFX_CODEC_TOPK: TOPK_LAUNCH(cc.bf16, cc.param, KID_ABSMEAN_COMPRESS_GATED, k_topk_layer_cap, grid, cc.b, cc.gd, a); break;
        case CFX_CODEC_MXFP4: MX_LAUNCH(cc.bf16, cc.param, KID_ABSMEAN_COMPRESS_GATED, k_mx_layer_cap, grid, cc.b, cc.gd, a); break;
        case CFX_CODEC_BINARY_BLOCK: BB_LAUNCH(cc.bf16, cc.param, KID_ABSMEAN_COMPRESS_GATED, k_bb_layer_cap, grid, cc.b, cc.gd, a); break;
        case CFX_CODEC_INT2_BLOCK: BB_LAUNCH(cc.bf16, cc.param, KID_ABSMEAN_COMPRESS_GATED, k_i2b_layer_cap, grid, cc.b, cc.gd, a); break;
        case CFX_CODEC_INT3_BLOCK: BB_LAUNCH(cc.bf16, cc.param, KID_ABSMEAN_COMPRESS_GATED, k_i3b_layer_cap, grid, cc.b, cc.gd, a); break;
        case CFX_CODEC_MXINT8: MXI8_LAUNCH(cc.bf16, cc.param, KID_ABSMEAN_COMPRESS_GATED, k_mxi8_layer_cap, grid, cc.b, cc.gd, a); break;
        default: if (xg) xg->taken = xg->inline_done = 0; return 0;
    }
    const int rc = check_launch(ctx, "captured layer launch");
    if (rc != CFX_OK) return rc;
    ++ctx->cap_used;            // the slot is this graph node's for good (cfx_captured_layer_release)
    ++ctx->cap_one;
    return 1;
}

static int cap_zero(cfx_ctx* ctx) {
    if (!ctx->cap_pool) return CFX_OK;
    if (hipMemset(ctx->cap_pool, 0, (size_t)ctx->cap_n * CFX_CAP_SLOT_WORDS * sizeof(unsigned)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        return CFX_ERR_LAUNCH;
    }
    return CFX_OK;
}
// cfx_gate_recover (the device is drained): all-zero is "before launch 0", so the graphs that hold the slots stay valid
int cfx_i_cap_recover(cfx_ctx* ctx) { return cap_zero(ctx); }
void cfx_i_cap_destroy(cfx_ctx* ctx) {
    if (ctx->cap_pool) (void)hipFree(ctx->cap_pool);
    ctx->cap_pool = nullptr;
    ctx->cap_n = ctx->cap_used = 0;
}

extern "C" {

int cfx_set_captured_layer(cfx_ctx* ctx, int slots) {
    if (!ctx) return CFX_ERR_NULL;
    if (slots < 0 || slots > CFX_CAP_MAX_SLOTS) return fail(ctx, CFX_ERR_SHAPE, "captured layer: the pool is 0 .. 4096 slots");
    if (slots == ctx->cap_n) return CFX_OK;
    if (ctx->cap_used) return fail(ctx, CFX_ERR_SHAPE, "captured layer: slots are handed out (cfx_captured_layer_release first)");
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (cur != ctx->device && hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, CFX_ERR_LAUNCH, "captured layer: hipSetDevice failed");
    int rc = CFX_OK;
    if (ctx->cap_pool) (void)hipDeviceSynchronize();
    cfx_i_cap_destroy(ctx);
    if (slots) {
        // (the error word the waits report to, the ticket blocks of the sequence's compress launches: nothing may be allocated during capture)
        void* p = nullptr;
        if (cfx_prepare(ctx) != CFX_OK) rc = CFX_ERR_LAUNCH;
        else if (hipMalloc(&p, (size_t)slots * CFX_CAP_SLOT_WORDS * sizeof(unsigned)) != hipSuccess) {
            (void)hipGetLastError();
            rc = fail(ctx, CFX_ERR_LAUNCH, "captured layer: cannot allocate the slots");
        } else {
            ctx->cap_pool = (unsigned*)p;
            ctx->cap_n = slots;
            if (cap_zero(ctx) != CFX_OK) {
                cfx_i_cap_destroy(ctx);
                rc = fail(ctx, CFX_ERR_LAUNCH, "captured layer: cannot zero the slots");
            }
        }
    }
    if (cur >= 0 && cur != ctx->device) (void)hipSetDevice(cur);
    return rc;
}

int cfx_captured_layer_stats(cfx_ctx* ctx, int* one_launch, int* sequence, int* slots_free) {
    if (!ctx) return CFX_ERR_NULL;
    if (one_launch) *one_launch = ctx->cap_one;
    if (sequence) *sequence = ctx->cap_seq;
    if (slots_free) *slots_free = ctx->cap_n - ctx->cap_used;
    return CFX_OK;
}

int cfx_captured_layer_release(cfx_ctx* ctx) {
    if (!ctx) return CFX_ERR_NULL;
    if (!ctx->cap_pool) return CFX_OK;
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (cur != ctx->device && hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, CFX_ERR_LAUNCH, "captured layer: hipSetDevice failed");
    int rc = CFX_OK;
    if (hipDeviceSynchronize() != hipSuccess || cap_zero(ctx) != CFX_OK) {
        (void)hipGetLastError();
        rc = fail(ctx, CFX_ERR_LAUNCH, "captured layer: cannot reset the slots");
    } else ctx->cap_used = 0;
    if (cur >= 0 && cur != ctx->device) (void)hipSetDevice(cur);
    return rc;
}

}  // extern "C"
