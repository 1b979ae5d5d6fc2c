/* cfx_dev.h - developer entry points of libcfx_dev.so (the same sources as libcfx.so compiled with -DCFX_DEV_PROBES:
 * `python -m compactfusion_amd.build --dev-probes`).  NOT part of the product ABI: libcfx.so exports none of these symbols, its kernels carry
 * no probe argument and no probe branch (csrc/cfx_internal.h: `Probe` is an empty type there), and compactfusion_amd/_lib.py does not bind
 * them.  Users: tools/*_stamps.py, tools/fused_probe.py (timelines of the layer launches and of the slab-resident low-rank chain) and
 * tests/tagwrap_child.py (walks a context across the wrap of its launch tags), tests/lr_q4_child.py (the low-rank factor quantiser alone). */
#ifndef CFX_DEV_H
#define CFX_DEV_H
#include "cfx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* When `buf` is non-NULL every workgroup of a layer launch / compress launch / k_lrs launch writes 16 u64 words at buf + 16 * workgroup:
 * phase times on the 100 MHz wall clock (word 7 of the layer kernels: the workgroup's role).  NULL switches it off. */
int cfx_dev_stamps(cfx_ctx* ctx, void* buf);
/* The layer launches tag what they hand over with numbers a context gives out in sequence (24 bits for the 1-bit / 2-bit layer, 31 for the
 * int4 / int8 layer); where a sequence wraps - 16.7 million, 2.1 billion launches in - the tagged arenas are zeroed and the numbers start
 * over.  This sets the two counters (after a device synchronisation) so that a test can walk a context across the wrap. */
int cfx_dev_set_launch_tags(cfx_ctx* ctx, unsigned abs_seq, unsigned mml_seq);
/* Early exits of the one-launch compress kernel (tools/fused_probe.py): 1 = stop after publishing, 2 = after the tickets, 3 = empty grid,
 * 4 = loads only; 0 = off.
 * CFX_DEV_SCALE_SPLIT + s, s in {0, 1, 2, 4}: leaves the probe mode alone and makes the 1-bit / 2-bit layer launches split a column block's
 * channel-scale job over s workgroups where the shape allows it (csrc/cfx_absmean.hip scale_jobs_split), instead of the split the library
 * chooses; s = 0 gives the choice back.  For the sweep behind profiles/scale_jobs_split_sweep.md - the split is no product knob. */
#define CFX_DEV_SCALE_SPLIT 0x100
int cfx_dev_set_probe(cfx_ctx* ctx, int mode);
/* k_lr_q4 alone on given fp16 factors: U (N, r), Vt (C, r) -> the two packet sections and, want_dq, the dequantised factors
 * (LOW_RANK_Q shapes: N, C even, rank % 8 == 0; every pointer 16-byte aligned; the launch geometry of cfx_lr_compress_batch).  The chains
 * hand the quantiser their factors in the workspace; this is how tests/lr_q4_child.py hands it a matrix. */
int cfx_dev_lr_q4(cfx_ctx* ctx, int N, int C, int rank, int want_dq, int batch, const void* const* U, const void* const* Vt,
                  void* const* packet, void* const* Uq, void* const* Vtq, void* stream);

#ifdef __cplusplus
}
#endif
#endif
