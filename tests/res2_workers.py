"""Worker body of the two-process second-order test (tests/test_gpu_res2_plugin.py; run through tests/_dist_workers.run)."""
import os

import numpy as np
import torch
import torch.distributed as dist

import _dist_workers as W

L, STEPS, SHAPE = 3, 6, (1, 64, 8, 64)


def w_res2_ring(rank, world, codec_name, gens):
    """compact_fwd (ring gather schedule), residual 2, WARMUP at steps 0 and 1, over `gens` generations with compact_reset in between:
    every rank's base and delta_base of every key after every step."""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd import _lib, codecs
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig, xlayer
    from compactfusion_amd.compact import ring as ring_mod
    os.environ["CFX_LANE"] = "off"
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s < 2 else T[codec_name], residual=2, ef=True,
                                  fastpath=False, comp_rank=-1, delta_decay_factor=0.5))
    res = {}
    for gen in range(gens):
        if gen:
            cm.compact_reset()
        qs = [W.drift(1000 * gen + 7 + 10 * l + rank, SHAPE, STEPS) for l in range(L)]
        ks = [W.drift(1000 * gen + 17 + 10 * l + rank, SHAPE, STEPS) for l in range(L)]
        vs = [W.drift(1000 * gen + 27 + 10 * l + rank, SHAPE, STEPS) for l in range(L)]
        for step in range(STEPS):
            cm.compact_set_step(step)
            for l in range(L):
                out, _, _ = ring_mod.compact_fwd(W.TD(qs[l][step]), W.TD(ks[l][step]), W.TD(vs[l][step]), causal=False, group=None, mod_idx=l,
                                                 current_iter=step)
                assert out.shape == SHAPE
            torch.cuda.synchronize()
            cache = cm.compact_cache()
            for l in range(L):
                for r in range(world):
                    for n in ("k", "v"):
                        key = f"{l}-{r}-{n}"
                        res[f"g{gen}/s{step}/l{l}/{n}{r}"] = W.bits(cache.get_base(key)).copy()
                        d = cache.get_delta_base(key)
                        if d is not None:
                            res[f"g{gen}/s{step}/l{l}/d{n}{r}"] = W.bits(d).copy()
    ops = [e.xop for e in ring_mod._xbuf.values() if e.xop is not None]
    res["n_ops"] = np.array([len(ops)])
    res["p2p"] = np.array([sum(1 for o in ops if o.transport == "p2p")])
    res["second"] = np.array([sum(1 for o in ops if o.own2 is not None)])
    res["fell_back"] = np.array([sum(1 for o in ops if o.fallback_reason is not None)])
    res["validated"] = np.array([min([o.region.validated for o in ops if o.region is not None] or [-1])])
    res["gate_errors"] = np.array([int(_lib.load().cfx_gate_errors(codecs.context(torch.cuda.current_device())))])
    dist.barrier()
    xlayer.release()
    return res
