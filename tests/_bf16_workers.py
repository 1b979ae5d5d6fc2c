"""Worker bodies of the world_size-2 gloo tests with bf16 activations (spawned processes, CPU tensors; the kernels replaced by the bf16
stand-in of tests/_bf16_backend.py).  Run through tests/_dist_workers.run."""
import numpy as np
import torch

import _dist_workers as W


def _drift_bf16(seed, shape, T):
    return [x.bfloat16() for x in W.drift(seed, shape, T)]


def w_all_gather_bf16(rank, world, codec_name, ef):
    import _bf16_backend as BB
    BB.install_plain()
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    N, C = 32, 256
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=1, ef=ef, fastpath=ef, comp_rank=-1))
    res = {}
    for t, x in enumerate(_drift_bf16(100 + rank, (N, C), 5)):
        typ = T.WARMUP if t == 0 else T[codec_name]
        outs = cm.compact_all_gather("3-k", x.view(1, N, C), typ)
        assert len(outs) == world and all(o.shape == (1, N, C) and o.dtype == torch.bfloat16 for o in outs)
        for i, o in enumerate(outs):
            res[f"t{t}/out{i}"] = W.bits(o).reshape(N, C).copy()
            res[f"t{t}/state{i}"] = W.bits(cm.compact_cache().get_base(f"3-k-{i}")).reshape(N, C).copy()
        res[f"t{t}/x"] = W.bits(x)
    return res


def w_all_gather_kv_bf16(rank, world, codec_name):
    import _bf16_backend as BB
    BB.install_plain()
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    N, C = 32, 256
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=1, ef=True, fastpath=True, comp_rank=-1))
    res = {}
    ks, vs = _drift_bf16(200 + rank, (N, C), 5), _drift_bf16(300 + rank, (N, C), 5)
    for t, (k, v) in enumerate(zip(ks, vs)):
        typ = T.WARMUP if t == 0 else T[codec_name]
        ko, vo = cm.compact_all_gather_kv("4-k", "4-v", k.view(1, N, C), v.view(1, N, C), typ)
        assert all(o.dtype == torch.bfloat16 for o in ko + vo)
        for i in range(world):
            res[f"t{t}/k{i}"] = W.bits(ko[i]).reshape(N, C).copy()
            res[f"t{t}/v{i}"] = W.bits(vo[i]).reshape(N, C).copy()
        res[f"t{t}/xk"], res[f"t{t}/xv"] = W.bits(k), W.bits(v)
    return res
