// Host-side internals shared by the translation units of libcfx.so's streaming codecs (compactfusion_amd/build.py SRC: cfx_api.hip - context,
// C-ABI, the codec table and its dispatch - and one file per codec family, with the family's kernels AND the code that launches them).
// Not part of the ABI.
#ifndef CFX_HOST_H
#define CFX_HOST_H
#include <algorithm>
#include "cfx_device.h"

// One compress call after validation: what cfx_api.hip's compress_impl has checked and packed, handed to the family that launches it.
struct CompressCall {
    cfx_ctx* ctx;
    int codec, N, C, param, flags, batch;
    const cfx_comp_item* items;
    int n_ride, n_gated;
    const cfx_decomp_item* gated;
    void* stream;
    CfxXGate* xg;                    // exchange-layer op: the gated items wait on an external gate (see compress_impl)
    BatchC b;
    BatchD rd, gd;
    u64* ws;
    size_t wstride;
    int CB;
    bool bf16;                       // the call's tensors (x, base, new_base, recon) are bf16: CFX_ELEM_BF16 on the codec argument
    bool upd, capturing;             // capturing: the stream is under hipGraph capture - no eager one-launch layer form (include/cfx.h; the
                                     // block-local families: the capturable one on a private gate slot, cfx_capture.hip, where a pool has one)
    // the tile geometry of the abs-mean and min/max families' compress launches (compress_impl, before the dispatch)
    bool fused;
    unsigned* tick;
    unsigned slot;
    int stream_cus, R, P;
    const cfx_second_item* second;   // != NULL: second-order states of the items (cfx_compress_batch_res2; 1-bit / 2-bit, fp16) and their decay
    float decay;
};
// One reconstruction call after validation (cfx_api.hip's cfx_i_decompress_checked).  `pre` / `pre_val`: an optional flag word the launch publishes
struct DecompressCall {
    cfx_ctx* ctx;
    int codec, N, C, param, batch;
    bool bf16;
    BatchD b;
    int R;                           // rows of a tile (the abs-mean and min/max families)
    void* stream;
    unsigned* pre;
    unsigned pre_val;
};
extern "C" {
// a family's two launchers, as the rows of cfx_api.hip's codec_table name them
#define CFX_FAMILY(name) \
    CFX_HIDDEN int cfx_i_##name##_compress(CompressCall& cc); \
    CFX_HIDDEN int cfx_i_##name##_decompress(const DecompressCall& dc);
CFX_FAMILY(absmean) CFX_FAMILY(minmax) CFX_FAMILY(topk) CFX_FAMILY(mx) CFX_FAMILY(bb) CFX_FAMILY(i2b) CFX_FAMILY(i3b) CFX_FAMILY(mxi8)
#undef CFX_FAMILY
// second order: the abs-mean family's reconstruction with a batch type of its own
CFX_HIDDEN int cfx_i_absmean_decompress2(cfx_ctx* ctx, int codec, int N, int C, int batch, const BatchD2& b, int R, void* stream, unsigned* pre, unsigned pre_val);
// cfx_api.hip
CFX_HIDDEN int cfx_i_auto_rows(const cfx_ctx* ctx, int N, int C, int batch, bool stats);
CFX_HIDDEN int cfx_i_fused_rows(const cfx_ctx* ctx, int N, int C, int batch, int cus);
CFX_HIDDEN unsigned cfx_i_ticket_slot(cfx_ctx* ctx, void* stream);
CFX_HIDDEN void cfx_i_fill_p2p(cfx_ctx* ctx, CfxXGate* xg, P2PInline& p);
CFX_HIDDEN int cfx_i_decompress_checked(cfx_ctx* ctx, int codec, int N, int C, int param, int batch, const cfx_decomp_item* items, void* stream,
                                        unsigned* pre, unsigned pre_val);
CFX_HIDDEN int cfx_i_decompress2_checked(cfx_ctx* ctx, int codec, int N, int C, int param, int batch, const cfx_decomp_item* items,
                                         const cfx_second_item* second, float decay, void* stream, unsigned* pre, unsigned pre_val);
}  // extern "C"
// cfx_local.h (inline: the block-local families' files include it): the stand-alone kernels' grid, the layer form of a compress call
// (> 0: `a` filled and the gates booked, the grid of k_*_layer; 0: none; < 0: an error code), the tail behind a stand-alone compress launch
struct LocalLayerArgs;
CFX_HIDDEN dim3 cfx_i_local_grid(int N, int C, int batch);
CFX_HIDDEN int cfx_i_local_layer(CompressCall& cc, LocalLayerArgs& a);
CFX_HIDDEN int cfx_i_local_tail(CompressCall& cc, const char* what);
// A ring's arena of TAGGED words (the min/max and the abs-mean layer launches: `arena` / `bytes` are the family's fields of the context for
// this ring), at least `need` bytes for a launch on `stream`.  Context-owned because a stale word must never carry a tag a later launch
// expects: it starts zeroed and only ever takes this context's tags.  Returns the arena, NULL when it cannot be allocated.
static inline u64* ring_arena_reserve(cfx_ctx* ctx, unsigned ring, void* stream, u64** arena, size_t* bytes, size_t need, size_t min_cap) {
    if (!ctx->mml_arena_owned[ring] || ctx->mml_arena_owner[ring] != stream) {
        // the ring - and with it its arenas - changed hands (more than CFX_RING_STREAMS streams issue compress launches): whatever its
        // previous owner still has in flight reads them.  Rare by construction; wait for it
        if (ctx->mml_arena_owned[ring]) (void)hipDeviceSynchronize();
        ctx->mml_arena_owner[ring] = stream;
        ctx->mml_arena_owned[ring] = true;
    }
    if (*bytes < need) {
        if (*arena) (void)hipFree(*arena);      // (synchronises the device: no launch still reads it)
        *arena = nullptr;
        *bytes = 0;
        const size_t cap = (std::max(need, min_cap) + 4095) & ~(size_t)4095;
        void* m = nullptr;
        // (zeroed IN the launch stream: a plain hipMemset runs on the NULL stream, which a non-blocking stream does not wait for)
        if (hipMalloc(&m, cap) != hipSuccess || hipMemsetAsync(m, 0, cap, (hipStream_t)stream) != hipSuccess) {
            (void)hipGetLastError();
            if (m) (void)hipFree(m);
            return nullptr;
        }
        *arena = (u64*)m;
        *bytes = cap;
    }
    return *arena;
}
// (short names the family files were written with)
#define auto_rows cfx_i_auto_rows
#define fused_rows cfx_i_fused_rows
#define ticket_slot cfx_i_ticket_slot
#define fill_p2p cfx_i_fill_p2p
#define stream_cu_count cfx_i_stream_cus
#define decompress_impl cfx_i_decompress_checked
#ifndef CFX_API_TU
#define shape_ok cfx_i_shape_ok
#define ws_words cfx_i_ws_words
#endif
#endif
