"""patch_gather_fwd's raw synchronous gather and its DistriFusion gather under configure(attention="native") on the GPU (-m gpu), two
rank processes (gloo) on one GPU: the two gather modes that had reached the one launch only through CPU stand-ins
(tests/test_attn_hd_f64.py) and run on a GPU only under SDPA (tests/_dist_workers.py, w_patch).  The compressed gather is
tests/test_gpu_attn_hd.py's.

Per configuration - gather mode x head dim 72 / 64 x joint tensors none / front / rear, one with softmax_scale = 0.3 passed in, one in
bf16 - 4 steps under "sdpa", then the same 4 under "native".  Every native call: ONE counted launch, no torch.cat from fwd.py, the blocks
handed to the launch bit for bit the tensors the mode must attend to (recomputed here from tests/_dist_workers.py's seeded `drift`),
the scale handed on the one the caller passed, out / lse within tests/_attn_var_f64.py's bound over exactly those blocks at that
scale, and out the sdpa run's to rtol = atol = 2e-3.  Every sdpa call: no launch, two or more cats.  A causal call under "native"
keeps cat + SDPA."""
import os
import socket

import numpy as np
import pytest
import torch

import _attn_var_f64 as VW
import bf16_contract as BC

pytestmark = pytest.mark.gpu
PSTEPS, WORLD = 4, 2
HEADS, SHARD, JOINT = 4, 64, 16              # shards (1, 64, 4, D), joint tensors (1, 16, 4, D)
# The bf16 configuration's shards: 256 keys a rank.  Two correct bf16 results may differ by one ulp where their unrounded values straddle
# a rounding boundary; an ulp is 2^-8 = 3.9e-3 for |x| in [0.5, 1) - MORE than 2e-3 + 2e-3 |x| below 0.95 - and 2^-9 = 1.95e-3 in
# [0.25, 0.5), less than the 2.5e-3 the tolerance is there.  So rtol = atol = 2e-3 against the sdpa run can hold in bf16 only where
# |out| < 0.5.  out is a softmax-weighted mean of unit Gaussian values over K keys with unit Gaussian scores: about K / e keys count,
# sigma = (e / K)^0.5 - 0.15 at K = 128 (0.5 is 3.4 sigma: some of 18432 elements pass it), 0.073 at K = 512 (6.9 sigma: none does).
SHARD_BF16 = 256
MODES = {"sync": (False, False, 0), "df": (False, True, 1)}          # PatchConfig's arguments: the raw synchronous gather, DistriFusion
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
bits = BC.torch_bits
# (mode, D, joint, element type, softmax_scale passed - None: the default, D ** -0.5 -, keys of a rank's shard)
PCONFIGS = [(mode, D, joint, "fp16", None, SHARD) for mode in MODES for D, joint in ((72, "none"), (72, "front"), (72, "rear"), (64, "none"), (64, "front"))]
PCONFIGS += [("df", 72, "front", "fp16", 0.3, SHARD), ("sync", 72, "rear", "bf16", None, SHARD_BF16)]


def _cid(cfg):
    mode, D, joint, dname, scale, shard = cfg
    return f"{mode}-d{D}-{joint}-{dname}-k{shard}" + ("" if scale is None else f"-s{scale}")


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _TorchSpy:
    """stands in for compact/patchpara/fwd.py's `torch`: counts torch.cat, passes everything through"""

    def __init__(self):
        self.cats = 0

    def cat(self, *a, **kw):
        self.cats += 1
        return torch.cat(*a, **kw)

    def __getattr__(self, name):
        return getattr(torch, name)


def _inputs(rank, D, dname, shard=SHARD):
    """the seeded sequences of tests/_dist_workers.py (`drift`: q 7 + rank, K 17 + rank, V 27 + rank; the joint tensors 37 and 47 on
    every rank), in the element type: per tensor a list over the steps"""
    import _dist_workers as DW
    shape, jshape = (1, shard, HEADS, D), (1, JOINT, HEADS, D)
    to = lambda seq: [t.to(TDT[dname]) for t in seq]             # noqa: E731
    return (to(DW.drift(7 + rank, shape, PSTEPS)), to(DW.drift(17 + rank, shape, PSTEPS)), to(DW.drift(27 + rank, shape, PSTEPS)),
            to(DW.drift(37, jshape, PSTEPS)), to(DW.drift(47, jshape, PSTEPS)))


def _patch_worker(rank, world, port, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import tempfile
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import compactfusion_amd
    from compactfusion_amd.collector import collector
    collector.init(collector.Collector(tempfile.mkdtemp(), enabled=False))
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import CompactConfig, PatchConfig
    from compactfusion_amd.compact import attention as A
    from compactfusion_amd.compact.patchpara import fwd as F
    from compactfusion_amd.compact.ring import compact_fwd
    spy = _TorchSpy()
    F.torch = spy
    seen = []

    def record(fn):
        def wrap(q, lk, lv, scale, *a, **kw):
            seen.append(([bits(t).copy() for t in lk], [bits(t).copy() for t in lv], float(scale)))
            return fn(q, lk, lv, scale, *a, **kw)
        return wrap
    F._attn_fwd_native, F._attn_fwd_native_var = record(F._attn_fwd_native), record(F._attn_fwd_native_var)
    res = {}

    def call(pre, q, k, v, step, **kw):
        torch.cuda.synchronize()
        del seen[:]
        spy.cats = 0
        n0 = A.attn_fwd_launches(0)
        out_, lse, _ = compact_fwd(q, k, v, group=None, mod_idx=3, current_iter=step, **kw)
        torch.cuda.synchronize()
        res[pre + "launches"] = np.array([A.attn_fwd_launches(0) - n0])
        res[pre + "cats"] = np.array([spy.cats])
        res[pre + "calls"] = np.array([len(seen)])
        res[pre + "out"] = out_.float().cpu().numpy()
        res[pre + "lse"] = lse.transpose(1, 2).float().cpu().numpy()                  # (B, Sq, H)
        if seen:
            res[pre + "scale"] = np.array([seen[0][2]])
            for i, (kk, vv) in enumerate(zip(seen[0][0], seen[0][1])):
                res[pre + f"k{i}"], res[pre + f"v{i}"] = kk, vv

    for cfg in PCONFIGS:
        mode, D, joint, dname, scale, shard = cfg
        qs, ks, vs, jks, jvs = _inputs(rank, D, dname, shard)
        for attention in ("sdpa", "native"):
            compactfusion_amd.configure(attention=attention)
            F._buffers.clear()
            cm.compact_init(CompactConfig(enabled=True, override_with_patch_gather_fwd=True, patch_gather_fwd_config=PatchConfig(*MODES[mode]),
                                          compress_func=None, residual=0, ef=False, fastpath=False, comp_rank=-1))
            for step in range(PSTEPS):
                cm.compact_set_step(step)
                kw = dict(joint_tensor_key=jks[step].cuda(), joint_tensor_value=jvs[step].cuda(), joint_strategy=joint) if joint != "none" else {}
                if scale is not None:
                    kw["softmax_scale"] = scale
                call(f"{_cid(cfg)}/{attention}/s{step}/", qs[step].cuda(), ks[step].cuda(), vs[step].cuda(), step, causal=False, **kw)
            if mode == "df":                                         # the last step's gather is in flight: nobody will consume it
                cm.allgather_cache().get("3-kv")[0].wait()
            dist.barrier()
    # a call the launch does not take, under "native": cat + SDPA, no launch
    compactfusion_amd.configure(attention="native")
    F._buffers.clear()
    cm.compact_init(CompactConfig(enabled=True, override_with_patch_gather_fwd=True, patch_gather_fwd_config=PatchConfig(*MODES["sync"]),
                                  compress_func=None, residual=0, ef=False, fastpath=False, comp_rank=-1))
    cm.compact_set_step(0)
    qs, ks, vs, _, _ = _inputs(rank, 72, "fp16")
    call("causal/", qs[0].cuda(), ks[0].cuda(), vs[0].cuda(), 0, causal=True)
    compactfusion_amd.configure(attention="sdpa")
    dist.barrier()
    np.savez(out + f".r{rank}.npz", **res)
    dist.destroy_process_group()


def _patch_runs(tmp_path):
    """ONE pair of rank processes runs every configuration of PCONFIGS under both settings (a fresh child per rank)"""
    import torch.multiprocessing as mp
    out = str(tmp_path / "patch")
    mp.start_processes(_patch_worker, args=(WORLD, _port(), out), nprocs=WORLD, join=True, start_method="spawn")
    return [dict(np.load(out + f".r{r}.npz")) for r in range(WORLD)]


def _floats(b, dname):
    """uint16 bit patterns -> the values, as float32"""
    if dname == "fp16":
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def _expected_blocks(cfg, rank, step, inputs):
    """the K and the V blocks the launch of `rank` must be handed at `step`, as 16-bit patterns.  Raw synchronous: every rank's step-s
    shard.  DistriFusion: the same at step 0 (the warm-up step gathers synchronously); from step 1 on the PEERS' shards of step s - 1
    and the rank's own of step s.  Joint tensors in front or at the rear."""
    mode, D, joint, dname, _, _ = cfg
    lk, lv = [], []
    for r in range(WORLD):
        s = step - 1 if (mode == "df" and step >= 1 and r != rank) else step
        lk.append(inputs[r][1][s])
        lv.append(inputs[r][2][s])
    jk, jv = inputs[rank][3][step], inputs[rank][4][step]
    if joint == "front":
        lk, lv = [jk] + lk, [jv] + lv
    elif joint == "rear":
        lk, lv = lk + [jk], lv + [jv]
    return [bits(t) for t in lk], [bits(t) for t in lv]


def _check_config(patch_runs, cfg):
    """Both ranks, every step.  sdpa: no launch, no call of a launch wrapper, two or more cats.  native: ONE counted launch through ONE
    wrapper call, no cat; the scale handed on is fp32 of the caller's (D ** -0.5 by default); the K and V blocks are `_expected_blocks`
    bit for bit - so a DistriFusion step that attended to the peers' FRESH shards, or to its own stale one, fails here whatever the
    tolerance -; out / lse within the float64 bound over those blocks at that scale; out within rtol = atol = 2e-3 of the sdpa run.
    Measured on an MI355X: at most 0.23 of the bound at the default scale, 0.34 at 0.3, 0.15 in bf16; at most 0.25 of the sdpa
    tolerance in fp16, 0.78 in bf16 (one bf16 ulp below 0.5)."""
    mode, D, joint, dname, scale, shard = cfg
    nb = WORLD + (joint != "none")
    inputs = [_inputs(r, D, dname, shard) for r in range(WORLD)]
    want_scale = float(np.float32(D ** -0.5 if scale is None else scale))
    worst = 0.0
    for rank in range(WORLD):
        top = _cid(cfg) + "/"
        g = {k[len(top):]: v for k, v in patch_runs[rank].items() if k.startswith(top)}
        for s in range(PSTEPS):
            a, b = f"sdpa/s{s}/", f"native/s{s}/"
            assert int(g[a + "launches"][0]) == 0 and int(g[a + "calls"][0]) == 0 and int(g[a + "cats"][0]) >= 2, (_cid(cfg), rank, a, g[a + "launches"], g[a + "cats"])
            assert int(g[b + "launches"][0]) == 1 and int(g[b + "calls"][0]) == 1 and int(g[b + "cats"][0]) == 0, (_cid(cfg), rank, b, g[b + "launches"], g[b + "cats"])
            assert float(np.float32(g[b + "scale"][0])) == want_scale, (_cid(cfg), rank, b, g[b + "scale"])
            wk, wv = _expected_blocks(cfg, rank, s, inputs)
            assert [k.shape[1] for k in wk] == [JOINT] * (joint == "front") + [shard] * WORLD + [JOINT] * (joint == "rear") and f"{b}k{nb}" not in g
            for i in range(nb):
                assert g[b + f"k{i}"].shape == wk[i].shape and np.array_equal(g[b + f"k{i}"], wk[i]), f"{_cid(cfg)} rank {rank} step {s}: K block {i} is not the expected tensor"
                assert g[b + f"v{i}"].shape == wv[i].shape and np.array_equal(g[b + f"v{i}"], wv[i]), f"{_cid(cfg)} rank {rank} step {s}: V block {i} is not the expected tensor"
            q = inputs[rank][0][s].float().numpy()
            ref = VW.reference_and_bound(q, [_floats(k, dname) for k in wk], [_floats(v, dname) for v in wv], want_scale, dname)
            fo, fl = VW.check(g[b + "out"], g[b + "lse"], ref, f"patch_gather_fwd native, {_cid(cfg)} rank {rank} step {s}")
            worst = max(worst, fo, fl)
            d = np.abs(g[b + "out"] - g[a + "out"]) / (2e-3 + 2e-3 * np.abs(g[a + "out"]))
            print(f"{_cid(cfg)} rank {rank} step {s}: {fo:.3f} / {fl:.3f} of the bound; against sdpa {d.max():.3f} of rtol = atol = 2e-3")
            np.testing.assert_allclose(g[b + "out"], g[a + "out"], rtol=2e-3, atol=2e-3)
    print(f"{_cid(cfg)}: largest fraction of the bound {worst:.3f}")


def test_raw_and_distrifusion_gather_are_one_launch_on_the_right_blocks(tmp_path):
    """every configuration of PCONFIGS (`_check_config`; a miss names its configuration, rank and step), and the causal call under
    "native": cat + SDPA, no launch"""
    patch_runs = _patch_runs(tmp_path)
    for cfg in PCONFIGS:
        _check_config(patch_runs, cfg)
    for rank in range(WORLD):
        g = patch_runs[rank]
        assert int(g["causal/launches"][0]) == 0 and int(g["causal/calls"][0]) == 0 and int(g["causal/cats"][0]) >= 2, (rank, g["causal/launches"], g["causal/cats"])
        assert np.isfinite(g["causal/out"]).all()
