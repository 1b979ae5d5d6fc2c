// The launch skeleton of libcfx.so's BLOCK-LOCAL wire codecs (the family files of compactfusion_amd/build.py SRC that include this header): a
// block's packet words are a function of the block alone, so nothing global is waited for.  Held once here: the bodies of the stand-alone
// compress / decompress kernels and of the one-launch layer (LOCAL_LAYER), and the host code of the layer form (decision, gate bookkeeping,
// hand-over to an exchange-layer op).  A family file keeps its codec - a policy type P - and its __global__ kernels, one-line wrappers of these bodies:
//   P::IN_FLIGHT   units whose packet words the layer's reconstruction group has in flight at once (divides LOCAL_DU)
//   P::ALL_LANES   lanes past the tensor's end take part in the compress unit (cross-lane steps and E % 2048 != 0 allowed: clamped loads,
//                  live == false, nothing stored); false: E % 1024 == 0, whole waves leave
//   P::MAKE_FIRST  the stand-alone decompress expands the record before it loads the state (false: behind that load) - each family's order
//                  from before the bodies were shared: either order for all costs one of them registers (tests pin the kernels' rows)
//   P::El          element type of the tensors (el_state<El>)
//   P::Recv        what a receiver loads for 8 elements
//   P::compress_unit<WT>(it, e, E, live, flags, xv, bv)    the 8 elements at flat offset e; WT: the packet goes out write-through
//   P::recv_load<MODE>(rec, packet, E, e)                  plain (0), L2-bypassing (1) or system-scope (2) loads
//   P::recv_make(rec, e) -> h16x8                          what the receiver adds
#ifndef CFX_LOCAL_H
#define CFX_LOCAL_H
#include "cfx_host.h"

#define LOCAL_SU 4              // units (8 elements a thread) of an S workgroup: 8192 elements, their loads in flight together
#define LOCAL_DU 8              // ... of a D workgroup: 16384 elements, 128 bytes of state a thread held across the wait
struct LocalLayerArgs {
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

template <class P>
__device__ __forceinline__ void local_compress(const BatchC& batch, size_t E, int flags) {
    const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    const bool live = e < E;
    if (!P::ALL_LANES && !live) return;                   // whole waves exit together
    const size_t ec = live ? e : 0;                       // (ALL_LANES: no lane leaves before the cross-lane steps: clamped loads, no stores)
    const cfx_comp_item it = batch.it[blockIdx.y];
    const h16x8 xv = ld8nt((const h16*)it.x + ec);
    h16x8 bv = (h16x8)(h16)0;
    if (it.base) bv = ld8nt((const h16*)it.base + ec);
    P::template compress_unit<false>(it, e, E, live, flags, xv, bv);
}

template <class P>
__device__ __forceinline__ void local_decompress(const BatchD& batch, size_t E, unsigned* pre, unsigned pre_val) {
    // lane: publish `pre` first - the launch in front of this one in the stream (the previous peer's reconstruction) has finished
    if (pre && (blockIdx.x | blockIdx.y | blockIdx.z | threadIdx.x) == 0) st_wt(pre, pre_val);
    const cfx_decomp_item it = batch.it[blockIdx.y];
    const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (e >= E) return;                                      // (nothing travels between lanes here)
    const h16* base = (const h16*)it.base;
    typename P::Recv rr;
    P::template recv_load<0>(rr, it.packet, E, e);
    h16x8 recv;
    if (P::MAKE_FIRST) recv = P::recv_make(rr, e);
    h16x8 bv = (h16x8)(h16)0;
    if (base) bv = ld8nt(base + e);
    if (!P::MAKE_FIRST) recv = P::recv_make(rr, e);
    st8nt((h16*)it.recon + e, el_state<typename P::El>(base != nullptr, bv, recv));
}

// ---- the layer in ONE launch (cfx_compress_batch_gated / the exchange-layer ops): group S compresses the own tensors (nothing global to
// wait for: every unit's loads first, at a clamped offset so that they are unconditional) and counts itself on the gate (packets complete =
// the word the gate's last arriver writes for XCD 0); group D - launched with it - holds the peers' state rows in registers until the gate
// (or the external gate: the packets of the other ranks) opens, then reads the packet words of P::IN_FLIGHT units at once and stores.
// The body of k_*_layer(BatchC batch, BatchD gated, LocalLayerArgs a) for the codec `...`.  A macro, not a function like the two above: the
// kernels' registers are pinned by the tests, and this body inlined from a function compiles to another allocation (k_topk_layer<16>: 61 ->
// 74 VGPRs, 8 -> 6 waves a SIMD); expanded in the kernel it compiles as it did when every family had its own copy.
#define LOCAL_LAYER(batch, gated, a, ...) \
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
        if (threadIdx.x == 0) gate_arrive(a.gate, 1u, a.gate_expect); \
        if (b == 0 && a.p2p.own) p2p_exchange_inline(a.gate + GATE_LINE, a.gate_expect, 1, a.p2p, a.xgate, a.xexpect, a.err); \
        return; \
    } \
    b -= a.n_st; \
    const int item = b / a.n_dw, dw = b - item * a.n_dw; \
    const cfx_decomp_item it = gated.it[item]; \
    const h16* base = (const h16*)it.base; \
    h16* out = (h16*)it.recon; \
    h16x8 bv[LOCAL_DU]; \
    _Pragma("unroll") for (int u = 0; u < LOCAL_DU; ++u) { \
        const size_t e = (((size_t)dw * LOCAL_DU + u) * 256 + threadIdx.x) * 8; \
        bv[u] = (base && e < a.E) ? ld8nt(base + e) : (h16x8)(h16)0; \
    } \
    if (!(a.xgate ? gate_wait<true>(a.xgate, a.xexpect, a.err, a.timeout) : gate_wait<false>(a.gate, a.gate_expect, a.err, a.timeout))) return; \
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

// ---------------------------------------------------------------------------------------------------
// host side (declared in cfx_host.h): what a family's cfx_i_*_compress / _decompress does around picking its kernel
// ---------------------------------------------------------------------------------------------------
// grid of the stand-alone kernels: one thread per 8 elements, one row of workgroups per tensor
inline dim3 cfx_i_local_grid(int N, int C, int batch) { return dim3((unsigned)(((size_t)N * C / 8 + 255) / 256), batch); }

// The layer form of a validated compress call.  > 0: the layer in ONE launch - `a` is filled, the gate bookkeeping is done, the exchange-layer
// op (cc.xg) has its words; the value is the grid of k_*_layer.  0: no layer form (stand-alone compress).  < 0: an error code.
inline int cfx_i_local_layer(CompressCall& cc, LocalLayerArgs& a) {
    cfx_ctx* ctx = cc.ctx;
    CfxXGate* xg = cc.xg;
    const size_t E = (size_t)cc.N * cc.C;
    const int stream_cus = cc.n_gated ? stream_cu_count(ctx, cc.stream) : 0;
    bool layer = cc.n_gated && ctx->gated_on && !ctx->dev_probe && stream_cus >= 128 && !cc.capturing;
    if (layer && !xg) {
        // loop-back: every reconstruction item reads one of this launch's packets
        for (int g_ = 0; g_ < cc.n_gated && layer; ++g_) {
            bool mine = false;
            for (int i = 0; i < cc.batch; ++i) mine = mine || cc.gated[g_].packet == cc.items[i].packet;
            layer = mine;
        }
    }
    if (!layer) return 0;
    if (!ctx->tick && cfx_prepare(ctx) != CFX_OK) return CFX_ERR_LAUNCH;
    if (ctx->gate_err && *(volatile unsigned*)ctx->gate_err)
        return fail(ctx, CFX_ERR_GATE, "compress: an earlier gate / flag wait on this context timed out (cfx_gate_errors reads and clears the count)");
    const unsigned slot = ticket_slot(ctx, cc.stream);
    memset(&a, 0, sizeof(a));
    a.E = E;
    a.n_sw = (int)((E / 8 + 256 * LOCAL_SU - 1) / (256 * LOCAL_SU));
    a.n_st = a.n_sw * cc.batch;
    a.n_dw = (int)((E / 8 + 256 * LOCAL_DU - 1) / (256 * LOCAL_DU));
    a.flags = cc.flags;
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
    return a.n_st + a.n_dw * cc.n_gated;
}

// Behind the stand-alone compress launch (`what`: its name for check_launch).  No layer form here: an exchange-layer op runs its exchange
// and the reconstruction behind this call; a plain gated call gets the reconstruction in stream order.
inline int cfx_i_local_tail(CompressCall& cc, const char* what) {
    const int rc = check_launch(cc.ctx, what);
    if (rc != CFX_OK || cc.xg || !cc.n_gated) return rc;
    return cfx_i_decompress_impl(cc.ctx, cc.codec | (cc.bf16 ? CFX_ELEM_BF16 : 0), cc.N, cc.C, cc.param, cc.n_gated, cc.gated, cc.stream, nullptr, 0u);
}

// A family's two launchers (cfx_host.h CFX_FAMILY; the last line of a family file), for its kernels k_<name>_compress / _layer / _decompress.
// `label`: the family's name in check_launch's messages.  PICK(bf16, param, kid, kern, grid, ...): launches the instantiation of the template
// `kern` that the call's element type and param select, with the caller's `ctx` and stream `s`; a family ignores what it has no template
// argument for.
#define LOCAL_FAMILY_HOST(name, label, PICK) \
    int cfx_i_##name##_compress(CompressCall& cc) { \
        cfx_ctx* ctx = cc.ctx; \
        hipStream_t s = (hipStream_t)cc.stream; \
        LocalLayerArgs a; \
        if (cc.capturing) {                 /* a pool of private gate slots (cfx_set_captured_layer): ONE capturable launch, cfx_capture.hip */ \
            const int cl = cfx_i_captured_layer(cc); \
            if (cl) return cl < 0 ? cl : CFX_OK; \
        } \
        const int lg = cfx_i_local_layer(cc, a); \
        if (lg < 0) return lg; \
        if (lg) { \
            PICK(cc.bf16, cc.param, KID_ABSMEAN_COMPRESS_GATED, k_##name##_layer, dim3((unsigned)lg), cc.b, cc.gd, a); \
            return check_launch(ctx, label " layer launch"); \
        } \
        PICK(cc.bf16, cc.param, KID_TOPK_COMPRESS, k_##name##_compress, cfx_i_local_grid(cc.N, cc.C, cc.batch), cc.b, (size_t)cc.N * cc.C, cc.flags); \
        return cfx_i_local_tail(cc, label " compress launch"); \
    } \
    int cfx_i_##name##_decompress(const DecompressCall& dc) { \
        cfx_ctx* ctx = dc.ctx; \
        hipStream_t s = (hipStream_t)dc.stream; \
        PICK(dc.bf16, dc.param, KID_TOPK_DECOMPRESS, k_##name##_decompress, cfx_i_local_grid(dc.N, dc.C, dc.batch), dc.b, (size_t)dc.N * dc.C, dc.pre, dc.pre_val); \
        return check_launch(ctx, "decompress launch"); \
    }
#endif
