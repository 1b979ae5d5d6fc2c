"""MXINT8 (codec id 16) on the CPU: the C-ABI's sizes, error order and refusals on the real library, and the host logic - state machine
with residual 0 / 1 / 2 in fp16 and 0 / 1 in bf16, the bf16 refusals, simulate mode, the stand-alone quantiser triple, the preset, the gloo
all-gather - with the kernels replaced by the numpy contract through the TEST-ONLY stand-in tests/_mxint8_backend.py.  The GPU tests
(tests/test_gpu_mxint8.py) hold the kernels to the same contract."""
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _dist_workers as W
import _mxint8_backend as KB
import mxint8_contract as M
import test_distributed_gloo as DG
from oracle import ref_np as R

F16 = np.float16
BF = M.ELEM_BF16
CID, CID_BF = 16, 0x110
bits = M.BC.torch_bits
NOT_CODECS = (15, 17, 0x10F, 0x111, 0x210, 0x1110, 0x310)


@pytest.fixture(autouse=True)
def _collector(tmp_path):
    from compactfusion_amd import config
    from compactfusion_amd.collector import collector
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    yield
    config.reset()


@pytest.fixture
def cpu_kernels(monkeypatch):
    KB.install(monkeypatch)
    import compactfusion_amd.compact.main as cm
    yield
    cm._packets.clear()


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_sizes_and_shape_rule():
    from compactfusion_amd import _lib, codecs
    lib = _lib.load()
    assert int(codecs.Codec.MXINT8) == CID and CID | BF == CID_BF and lib.cfx_abi_version() == 2
    for N, C in ((1, 64), (1, 128), (3, 192), (5, 320), (4, 2112), (129, 128), (129, 3072), (544, 3072), (4448, 3072)):
        want = N * C + N * C // 32
        for cid in (CID, CID_BF):
            assert lib.cfx_packet_bytes(cid, N, C, 0) == want == 2 * M.packet_halves(N, C), (hex(cid), N, C)
            for batch in (1, 16):
                assert lib.cfx_workspace_bytes(cid, N, C, 0, batch) == 0                      # as top-k and MXFP4: callers pass NULL / 0
    for N, C in ((4, 32), (4, 96), (4, 160), (4, 8), (0, 128), (544, 3080)):
        assert lib.cfx_packet_bytes(CID, N, C, 0) == 0 and lib.cfx_packet_bytes(CID_BF, N, C, 0) == 0
    for param in (1, 8, 32, 64, 128, -1):
        assert lib.cfx_packet_bytes(CID, 544, 3072, param) == 0 and lib.cfx_packet_bytes(CID_BF, 544, 3072, param) == 0
    for bad in NOT_CODECS:
        assert lib.cfx_packet_bytes(bad, 544, 3072, 0) == 0 and lib.cfx_workspace_bytes(bad, 544, 3072, 0, 2) == 0, hex(bad)


@pytest.mark.parametrize("cid", [CID, CID_BF])
def test_abi_argument_errors_in_order(cid):
    """null, batch, shape, alignment in the documented order - and no workspace is required"""
    from compactfusion_amd import _lib
    lib = _lib.load()
    ctx = lib.cfx_create(0)
    assert ctx
    items = (_lib.CompItem * 1)()
    d = (_lib.DecompItem * 1)()
    assert lib.cfx_compress_batch(ctx, cid, 8, 64, 0, 0, 1, None, None, 0, None) == -1             # null items
    assert lib.cfx_compress_batch(ctx, cid, 8, 96, 0, 0, 1, items, None, 0, None) == -2            # C % 64 != 0: CFX_ERR_SHAPE before the item checks
    assert lib.cfx_compress_batch(ctx, cid, 8, 64, 32, 0, 1, items, None, 0, None) == -2           # param is not 0
    assert lib.cfx_decompress_batch(ctx, cid, 8, 96, 0, 1, d, None) == -2
    assert lib.cfx_decompress_batch(ctx, cid, 8, 128, 1, 1, d, None) == -2
    assert lib.cfx_compress_batch(ctx, cid, 8, 64, 0, 0, 0, items, None, 0, None) == -5
    assert lib.cfx_compress_batch(ctx, cid, 8, 96, 0, 0, 17, items, None, 0, None) == -5           # batch before shape
    assert lib.cfx_decompress_batch(ctx, cid, 8, 96, 0, 17, d, None) == -5
    assert lib.cfx_compress_batch(ctx, cid, 8, 64, 0, 0, 1, items, None, 0, None) == -1            # null x
    items[0] = _lib.CompItem(0x1002, None, None, 0x2000)
    assert lib.cfx_compress_batch(ctx, cid, 8, 64, 0, 0, 1, items, None, 0, None) == -3
    items[0] = _lib.CompItem(0x1000, None, None, 0x2008)                                          # the packet too: its code words are 64-bit stores
    assert lib.cfx_compress_batch(ctx, cid, 8, 64, 0, 0, 1, items, None, 0, None) == -3
    items[0] = _lib.CompItem(0x1000, None, None, 0x2000)
    assert lib.cfx_compress_batch(ctx, cid, 8, 64, 0, 1, 1, items, None, 0, None) == -1            # UPDATE_CACHE without new_base
    assert lib.cfx_decompress_batch(ctx, cid, 8, 64, 0, 1, d, None) == -1
    d[0] = _lib.DecompItem(0x2000, 0x3008, 0x3000)
    assert lib.cfx_decompress_batch(ctx, cid, 8, 64, 0, 1, d, None) == -3
    d[0] = _lib.DecompItem(0x2008, 0x3000, 0x3000)
    assert lib.cfx_decompress_batch(ctx, cid, 8, 64, 0, 1, d, None) == -3
    lib.cfx_destroy(ctx)


def test_abi_refusals():
    """any other high bit, ride-along items, the second-order entry points: CFX_ERR_CODEC before any launch"""
    from compactfusion_amd import _lib
    lib = _lib.load()
    ctx = lib.cfx_create(0)
    items = (_lib.CompItem * 1)()
    d = (_lib.DecompItem * 1)()
    for bad in NOT_CODECS:
        assert lib.cfx_compress_batch(ctx, bad, 8, 64, 0, 0, 1, items, None, 0, None) == -4, hex(bad)
        assert lib.cfx_decompress_batch(ctx, bad, 8, 64, 0, 1, d, None) == -4, hex(bad)
    items[0] = _lib.CompItem(0x1000, None, None, 0x2000)
    ride = (_lib.DecompItem * 1)(_lib.DecompItem(0x2000, 0x3000, 0x3000))
    c = (_lib.CompItem * 2)(_lib.CompItem(0x1000, 0x2000, 0x2000, 0x3000), _lib.CompItem(0x4000, 0x5000, 0x5000, 0x6000))
    s2 = (_lib.SecondItem * 2)(_lib.SecondItem(0xa000, 0xa000), _lib.SecondItem(0xb000, 0xb000))
    d2 = (_lib.DecompItem * 2)(_lib.DecompItem(0x7000, 0x8000, 0x8000), _lib.DecompItem(0x7000, 0x8000, 0x8000))
    for cid in (CID, CID_BF):
        assert lib.cfx_compress_batch_ex(ctx, cid, 8, 64, 0, 0, 1, items, 1, ride, None, 0, None) == -4
        assert lib.cfx_compress_batch_res2(ctx, cid, 544, 3072, 0, 1, 2, c, s2, 0.5, None, 0, None) == -4
        assert lib.cfx_decompress_batch_res2(ctx, cid, 544, 3072, 0, 2, d2, s2, 0.5, None) == -4
    lib.cfx_destroy(ctx)


def test_abi_plan_ops_added_and_copied():
    """plan ops keep the bf16 bit: an op added with 0x110 is copied as it is, and refuses what 16 refuses"""
    from compactfusion_amd import _lib
    lib = _lib.load()
    ctx = lib.cfx_create(0)
    plan = lib.cfx_plan_create(ctx)
    c = (_lib.CompItem * 2)(_lib.CompItem(0x1000, 0x2000, 0x2000, 0x3000), _lib.CompItem(0x4000, 0x5000, 0x5000, 0x6000))
    dd = (_lib.DecompItem * 14)(*[_lib.DecompItem(0x7000, 0x8000, 0x8000)] * 14)
    assert lib.cfx_plan_add_compress(plan, CID, 544, 3072, 0, 1, 2, c, None, 0) == 0
    assert lib.cfx_plan_add_decompress(plan, CID, 544, 3072, 0, 14, dd) == 1
    assert lib.cfx_plan_add_compress_gated(plan, CID_BF, 544, 3072, 0, 1, 2, c, 0, None, 14, dd, None, 0) == 2
    assert lib.cfx_plan_add_decompress(plan, CID_BF, 544, 3072, 0, 14, dd) == 3
    assert lib.cfx_plan_add_compress(plan, CID, 544, 3080, 0, 1, 2, c, None, 0) == -2
    assert lib.cfx_plan_add_compress(plan, CID, 544, 3072, 32, 1, 2, c, None, 0) == -2
    assert lib.cfx_plan_add_compress(plan, 0x210, 544, 3072, 0, 1, 2, c, None, 0) == -4
    assert lib.cfx_plan_add_decompress(plan, 0x210, 544, 3072, 0, 14, dd) == -4
    ride = (_lib.DecompItem * 1)(_lib.DecompItem(0x7000, 0x8000, 0x8000))
    assert lib.cfx_plan_add_compress_ex(plan, CID, 544, 3072, 0, 1, 2, c, 1, ride, None, 0) == -4
    assert lib.cfx_plan_add_exchange_layer(plan, 0x210, 544, 3072, 0, 1, 2, c, 14, dd, None, None, None, 0, None, 0) == -4
    assert lib.cfx_plan_add_exchange_layer(plan, 17, 544, 3072, 0, 1, 2, c, 14, dd, None, None, None, 0, None, 0) == -4
    other = lib.cfx_plan_create(ctx)
    assert [lib.cfx_plan_copy_op(other, plan, i) for i in range(4)] == [0, 1, 2, 3]
    s2 = (_lib.SecondItem * 2)(_lib.SecondItem(0xa000, 0xa000), _lib.SecondItem(0xb000, 0xb000))
    assert lib.cfx_plan_set_second_order(plan, 0, 2, s2, 0, None, 0.5) == -4
    assert lib.cfx_plan_set_second_order(plan, 2, 2, s2, 0, None, 0.5) == -4
    assert lib.cfx_plan_set_second_order(other, 2, 2, s2, 0, None, 0.5) == -4
    # the peer-to-peer exchange layer refuses 15, 17 and 0x210 and takes 16 / 0x110 (past the codec check it allocates a device word: needs a GPU)
    for bad in (15, 17, 0x210):
        assert lib.cfx_plan_add_exchange_layer_p2p(plan, bad, 544, 3072, 0, 1, 2, c, 14, dd, 0xc000, 0, None, None, 0) == -4
    for cid in (CID, CID_BF):
        rc = lib.cfx_plan_add_exchange_layer_p2p(plan, cid, 544, 3072, 0, 1, 2, c, 14, dd, 0xc000, 0, None, None, 0)
        assert rc >= 4 or rc == -6, rc
    lib.cfx_plan_destroy(other)
    lib.cfx_plan_destroy(plan)
    lib.cfx_destroy(ctx)


def test_kernels_exist_without_scratch():
    """the three kernel templates in the built library, each for both element types: no scratch, no LDS beyond the gate wait's barrier
    word, and the layer leaves a collective kernel room (at most 104 registers, as the other layer launches)"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import resource_usage
    rows = {k["demangled"].split("(")[0]: k for k in resource_usage.collect() if k["demangled"].startswith("k_mxi8_")}
    want = {f"{n}<{e}>" for n in ("k_mxi8_compress", "k_mxi8_decompress", "k_mxi8_layer") for e in ("ElemF16", "ElemBF16")}
    assert set(rows) == want, sorted(rows)
    for k in rows.values():
        assert k.get("scratch", 0) == 0 and k["vgpr"] + k.get("agpr", 0) <= 104 and k["lds"] <= 256, k


# ---- the mappings ----------------------------------------------------------------------------------------------------------------------
def test_mappings_and_preset():
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, presets, xlayer
    assert T.MXINT8.value == "mxint8" and cm._native(T.MXINT8) == (CID, 0)
    c = presets.get_config("Flux", "mxint8")
    assert c.enabled and c.compress_residual == 1 and c.error_feedback and not c.fastpath and not c.simulate_compress
    assert [c.compress_func(0, s) for s in range(3)] == [T.WARMUP, T.MXINT8, T.MXINT8]
    assert [presets.get_config("CogVideoX", "mxint8").compress_func(3, s) for s in range(3)] == [T.WARMUP, T.WARMUP, T.MXINT8]
    assert "mxint8" in presets.METHODS
    # the layer op takes id 16; 15 and 17 are no codecs
    assert xlayer.usable(CID, 2, True) and xlayer.usable(CID, 8, True) and not xlayer.usable(CID, 2, False)
    assert not xlayer.usable(15, 2, True) and not xlayer.usable(17, 2, True)


# ---- the host state machine against the contract -------------------------------------------------------------------------------------
MODES = [("res1_ef", dict(residual=1, ef=True)), ("res1_noef", dict(residual=1, ef=False)), ("res0", dict(residual=0, ef=False))]


@pytest.mark.parametrize("bf", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("mode,kw", MODES, ids=[m[0] for m in MODES])
def test_state_machine_equals_the_contract(cpu_kernels, mode, kw, bf):
    """Warm-up, then 6 compressed steps: packets, the sender's state and the receiver's state follow the contract bit for bit; with error
    feedback both states are the same bits."""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    N, C = 64, 1024
    dt = torch.bfloat16 if bf else torch.float16
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, **kw))
    res, ef = kw["residual"], kw["ef"]
    skey, rkey = "0-0-k", "0-1-k"
    s_state = r_state = None
    for t, x in enumerate(W.drift(11, (N, C), 7)):
        x = x.to(dt)
        x4 = x.view(1, N, 8, C // 8)
        xb = bits(x).reshape(N, C)
        warm = res == 1 and t == 0
        typ = T.WARMUP if warm else T.MXINT8
        pkt = cm.compact_compress(skey, x4, typ, update_cache=True)
        if warm:
            assert pkt.dtype == dt and np.array_equal(bits(pkt).reshape(N, C), xb)
            rec = cm.compact_decompress(rkey, pkt.clone(), typ, x4.shape, update_cache=True)
            assert rec.dtype == dt and np.array_equal(bits(rec).reshape(N, C), xb)
            s_state, r_state = xb.copy(), xb.copy()
            continue
        want_pkt, nb = M.step(xb, s_state if res else None, bf, ef)
        assert pkt.dtype == torch.float16 and pkt.numel() == M.packet_halves(N, C)
        assert np.array_equal(bits(pkt).reshape(-1), want_pkt), f"{mode} step {t}: packet"
        want_rec = M.recon(want_pkt, r_state if res else None, N, C, bf)
        if res == 0:
            rec = cm._decompress(rkey, pkt.clone(), typ, x4.shape, True, dt)
            assert rec.dtype == dt and rec.shape == x4.shape and np.array_equal(bits(rec).reshape(N, C), want_rec)
            assert cm.compact_cache().get_base(skey) is None and cm.compact_cache().get_base(rkey) is None
            continue
        rec = cm.compact_decompress(rkey, pkt.clone(), typ, x4.shape, update_cache=True)
        assert rec.dtype == dt and rec.shape == x4.shape
        assert np.array_equal(bits(rec).reshape(N, C), want_rec), f"{mode} step {t}: reconstruction"
        s_state, r_state = nb, want_rec
        assert cm.compact_cache().get_base(skey).dtype == dt and cm.compact_cache().get_base(rkey).dtype == dt
        assert np.array_equal(bits(cm.compact_cache().get_base(skey)).reshape(N, C), s_state), f"{mode} step {t}: sender state"
        assert np.array_equal(bits(cm.compact_cache().get_base(rkey)).reshape(N, C), r_state), f"{mode} step {t}: receiver state"
        if ef:
            assert np.array_equal(s_state, r_state), f"{mode} step {t}: sender and receiver states differ"
        else:
            assert np.array_equal(s_state, xb)


class _Oracle(R.OracleCompact):
    """R.OracleCompact with the contract of tests/mxint8_contract.py as its codec 'mxint8'"""

    def _comp(self, codec, d):
        return M.encode(d) if codec == M.NAME else super()._comp(codec, d)

    def _decomp(self, codec, pkt, N, C):
        return M.decode(pkt, N, C) if codec == M.NAME else super()._decomp(codec, pkt, N, C)


def test_residual_2_composes_around_the_codec(cpu_kernels):
    """fp16, residual 2: cfx_residual2_delta ; codec (base NULL) ; cfx_residual2_update around id 16 (codecs.res2_fused is false for it) -
    packets and both states of both sides follow R.OracleCompact over the contract bit for bit"""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd import codecs
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    N, C = 64, 1024
    assert not codecs.res2_fused(CID, torch.zeros(4, 64).half())
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=2, ef=True, delta_decay_factor=0.5))
    orc_s, orc_r = (_Oracle(residual=2, ef=True, decay=0.5) for _ in range(2))
    skey, rkey = "0-0-k", "0-1-k"
    for t, x in enumerate(W.drift(11, (N, C), 6)):
        x4 = x.contiguous().view(1, N, 8, C // 8)
        warm = t < 2
        typ, name = (T.WARMUP, "warmup") if warm else (T.MXINT8, M.NAME)
        pkt = cm.compact_compress(skey, x4, typ, update_cache=True)
        want = orc_s.compress(skey, bits(x4).reshape(1, N, 8, C // 8), name, True)
        assert np.array_equal(bits(pkt).reshape(-1), want), f"step {t}: packet"
        rec = cm.compact_decompress(rkey, pkt.clone(), typ, x4.shape, update_cache=True)
        wrec = orc_r.decompress(rkey, want, name, x4.shape, True)
        assert np.array_equal(bits(rec).reshape(-1), R.bits(wrec).reshape(-1)), f"step {t}: reconstruction"
        assert np.array_equal(bits(cm.compact_cache().get_base(skey)), R.bits(orc_s.base[skey])), f"step {t}: sender state"
        assert np.array_equal(bits(cm.compact_cache().get_base(rkey)), R.bits(orc_r.base[rkey])), f"step {t}: receiver state"
        assert np.array_equal(bits(cm.compact_cache().get_base(skey)), bits(cm.compact_cache().get_base(rkey)))
        if t >= 1:
            assert np.array_equal(bits(cm.compact_cache().get_delta_base(skey)), R.bits(orc_s.dbase[skey])), f"step {t}: delta state"


def test_bf16_with_residual_2_raises_before_any_state_moves(cpu_kernels):
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig, slowpath as S
    N, C = 64, 1024
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=2, ef=True, delta_decay_factor=0.5))
    cache = cm.compact_cache()
    x16 = W.drift(5, (N, C), 1)[0]
    cm.compact_compress("0-0-k", x16, T.WARMUP, update_cache=True)
    cm.compact_decompress("0-1-k", x16.clone(), T.WARMUP, (N, C), update_cache=True)
    before = {k: (v.dtype, bits(v).copy()) for k, v in cache.base.items()}
    version = cache.version
    with pytest.raises(NotImplementedError, match="compress_residual 2"):
        cm.compact_compress("0-0-k", x16.bfloat16(), T.MXINT8, update_cache=True)
    with pytest.raises(NotImplementedError):
        cm._decompress("0-1-k", torch.zeros(M.packet_halves(N, C)).half(), T.MXINT8, (N, C), True, torch.bfloat16)
    assert cache.version == version and {k for k in cache.base} == set(before)
    for k, v in cache.base.items():
        assert v.dtype == before[k][0] and np.array_equal(bits(v), before[k][1])
    # simulation with bf16 stays refused too; fp16 simulation is compress ; decompress with base NULL
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=0, ef=False, simulate=True))
    with pytest.raises(NotImplementedError):
        cm.compact_compress("0-0-k", x16.bfloat16(), T.MXINT8, update_cache=True)
    want = R.bits(M.compress(bits(x16).reshape(N, C).view(F16), None)[1])
    out = cm.compact_compress("0-0-k", x16, T.MXINT8, update_cache=True)
    assert out.shape == x16.shape and np.array_equal(bits(out).reshape(N, C), want)
    assert np.array_equal(bits(S.sim_compress(x16, T.MXINT8)), want)
    # the wire codec through the slowpath mirror
    pkt = S.slowpath_compress(x16, T.MXINT8)
    assert pkt.numel() == M.packet_halves(N, C) and np.array_equal(bits(S.slowpath_decompress(pkt, (N, C), T.MXINT8)), want)


_BF16_REFUSALS = [("simulate_res1", dict(residual=1, ef=True, simulate=True), False, "simulate_compress"),
                  ("simulate_res0", dict(residual=0, ef=False, simulate=True), False, "simulate_compress"),
                  ("quantized_cache", dict(residual=1, ef=True, quantized_cache=True), True, "quantized_cache")]


@pytest.mark.parametrize("label,kw,deprecated,word", _BF16_REFUSALS, ids=[r[0] for r in _BF16_REFUSALS])
def test_bf16_with_simulation_or_quantized_cache_raises_before_any_state_moves(cpu_kernels, monkeypatch, label, kw, deprecated, word):
    """bf16 activations with MXINT8 under simulation (residual 1 and 0) and under a quantized cache: NotImplementedError from the compress
    and from the decompress side, the warm-up step included where no bf16 state may ever be stored, and the cache - version, keys, element
    types, bits - exactly as it was"""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig, utils as U
    if deprecated:
        monkeypatch.setattr(U, "ALLOW_DEPRECATED", True)
    N, C = 64, 1024
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, **kw))
    cache = cm.compact_cache()
    assert cache.quantize == bool(kw.get("quantized_cache"))
    x16 = W.drift(5, (N, C), 1)[0]
    if label == "simulate_res1":
        # fp16 states that must stay exactly as they are
        cm.compact_compress("0-0-k", x16, T.WARMUP, update_cache=True)
        cm.compact_decompress("0-1-k", x16.clone(), T.WARMUP, (N, C), update_cache=True)
        assert len(cache.base) == 2
    before = {k: (v.dtype, bits(v).copy()) for k, v in cache.base.items()}
    version = cache.version

    def untouched():
        assert cache.version == version and set(cache.base) == set(before), label
        for k, (dt, b) in before.items():
            assert cache.base[k].dtype == dt and np.array_equal(bits(cache.base[k]), b), (label, k)
    with pytest.raises(NotImplementedError, match="bfloat16") as e:
        cm.compact_compress("0-0-k", x16.bfloat16(), T.MXINT8, update_cache=True)
    assert "not supported with" in str(e.value) and word in str(e.value) and "MXINT8" in str(e.value), (label, str(e.value))
    untouched()
    with pytest.raises(NotImplementedError, match="bfloat16"):
        cm._decompress("0-1-k", torch.zeros(M.packet_halves(N, C)).half(), T.MXINT8, (N, C), True, torch.bfloat16)
    untouched()
    if label == "quantized_cache":
        with pytest.raises(NotImplementedError, match="bfloat16"):
            cm.compact_compress("0-0-k", x16.bfloat16(), T.WARMUP, update_cache=True)      # (not even the warm-up step)
        untouched()
    # never a silent cast: the same type with fp16 or bf16 activations alone is not refused by the bf16 rule
    assert cm._check_bf16(torch.float16, T.MXINT8) is None


def test_fastpath_still_asserts_binary_or_int2(cpu_kernels):
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    cm.compact_init(CompactConfig(enabled=True, residual=1, ef=True, fastpath=True, comp_rank=-1))
    x = torch.randn(1, 8, 64).half()
    cm.compact_compress("0-0-k", x, T.WARMUP, update_cache=True)
    with pytest.raises(AssertionError):
        cm.compact_compress("0-0-k", x, T.MXINT8, update_cache=True)


def test_quantize_dequantize_triple_round_trip(cpu_kernels):
    from compactfusion_amd.compact import compress_quantize as Q
    N, C = 64, 256
    torch.manual_seed(42)
    d = torch.randn(N, C).half()
    codes, scales = Q.quantize_mxint8(d)
    assert codes.shape == (N, C) and codes.dtype == torch.int8 and scales.shape == (N, C // 32) and scales.dtype == torch.uint8
    want_pkt, want_recv = M.compress(bits(d).view(F16), None)
    wq, ws = M.split(want_pkt, N, C)
    assert np.array_equal(codes.numpy(), wq) and np.array_equal(scales.numpy(), ws)
    assert np.array_equal(bits(Q.dequantize_mxint8(codes, scales)), R.bits(want_recv))
    assert np.array_equal(bits(Q.sim_mxint8(d)), R.bits(want_recv))
    with pytest.raises(AssertionError):
        Q.quantize_mxint8(d[:, :96].contiguous())
    with pytest.raises(AssertionError):
        Q.dequantize_mxint8(codes.view(torch.uint8), scales)


# ---- compact_all_gather over two gloo ranks --------------------------------------------------------------------------------------------
def _entry(rank, world, port, out):
    W.run(KB.w_all_gather_mxint8, rank, world, port, out)


def test_compact_all_gather_2rank(tmp_path):
    out = str(tmp_path / "res")
    for attempt in range(3):
        try:
            mp.start_processes(_entry, args=(2, DG._port(), out), nprocs=2, join=True, start_method="spawn")
            break
        except Exception as e:  # noqa: BLE001
            if "EADDRINUSE" not in str(e) or attempt == 2:
                raise
    res = [dict(np.load(out + f".r{r}.npz")) for r in range(2)]
    N, C = 32, 256
    state = [None, None]
    for t in range(4):
        for i in range(2):
            assert np.array_equal(res[0][f"t{t}/out{i}"], res[1][f"t{t}/out{i}"]), (t, i)
            x = res[i][f"t{t}/x"].reshape(N, C)
            if t == 0:
                assert np.array_equal(res[0][f"t0/out{i}"], x)
                state[i] = x.copy()
            else:
                _, nb = M.step(x, state[i], False)
                state[i] = nb.reshape(N, C)
                assert np.array_equal(res[0][f"t{t}/out{i}"], state[i]), f"step {t} shard {i}: not the contract's state"
    for r in range(2):
        assert int(res[r]["passed_count"][0]) == 1
