"""MXFP4 (codec id 8) on the CPU: the C-ABI's sizes and refusals on the real library, and the host logic - state machine, residual 0 / 1 / 2,
simulate mode, the gloo all-gather, the stand-alone quantiser pair, the bf16 refusal - with the kernels replaced by the numpy contract
through the TEST-ONLY stand-in tests/_mxfp4_backend.py (tests/_oracle_backend.py plus id 8).  The GPU tests (tests/test_gpu_mxfp4.py) hold
the kernels to the same contract."""
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _dist_workers as W
import _mxfp4_backend as MB
import mxfp4_contract as M
import test_distributed_gloo as DG
from oracle import ref_np as R

F16 = np.float16


@pytest.fixture(autouse=True)
def _collector(tmp_path):
    from compactfusion_amd.collector import collector
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    yield


@pytest.fixture
def cpu_kernels(monkeypatch):
    MB.install(monkeypatch)


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_sizes_and_shape_rule():
    from compactfusion_amd import _lib, codecs
    lib = _lib.load()
    assert int(codecs.Codec.MXFP4) == 8 and lib.cfx_abi_version() == 2
    for N, C in ((1, 64), (3, 64), (5, 320), (544, 3072), (4448, 3072), (17, 576)):
        assert lib.cfx_packet_bytes(8, N, C, 0) == N * C // 2 + N * C // 32 == 2 * M.packet_halves(N, C)
        for batch in (1, 16):
            assert lib.cfx_workspace_bytes(8, N, C, 0, batch) == 0                                   # as top-k: callers pass NULL / 0
    for N, C in ((4, 32), (4, 96), (544, 3080), (4, 8), (0, 64)):
        assert lib.cfx_packet_bytes(8, N, C, 0) == 0 and lib.cfx_workspace_bytes(8, N, C, 0, 1) == 0
    for param in (1, 8, 32, -1):
        assert lib.cfx_packet_bytes(8, 544, 3072, param) == 0
    assert lib.cfx_packet_bytes(0x108, 544, 3072, 0) == 0 and lib.cfx_workspace_bytes(0x108, 544, 3072, 0, 2) == 0
    assert lib.cfx_packet_bytes(7, 544, 3072, 0) == 0 and lib.cfx_packet_bytes(9, 544, 3072, 0) == 0


def test_abi_argument_errors_in_order():
    """null, shape, batch, alignment - and no workspace is required"""
    from compactfusion_amd import _lib
    lib = _lib.load()
    ctx = lib.cfx_create(0)
    assert ctx
    items = (_lib.CompItem * 1)()
    d = (_lib.DecompItem * 1)()
    assert lib.cfx_compress_batch(ctx, 8, 8, 64, 0, 0, 1, None, None, 0, None) == -1             # null items
    assert lib.cfx_compress_batch(ctx, 8, 8, 96, 0, 0, 1, items, None, 0, None) == -2            # C % 64 != 0: CFX_ERR_SHAPE before the item checks
    assert lib.cfx_compress_batch(ctx, 8, 8, 64, 1, 0, 1, items, None, 0, None) == -2            # param != 0
    assert lib.cfx_decompress_batch(ctx, 8, 8, 96, 0, 1, d, None) == -2
    assert lib.cfx_decompress_batch(ctx, 8, 8, 64, 4, 1, d, None) == -2
    assert lib.cfx_compress_batch(ctx, 8, 8, 64, 0, 0, 0, items, None, 0, None) == -5
    assert lib.cfx_compress_batch(ctx, 8, 8, 96, 0, 0, 17, items, None, 0, None) == -5           # batch before shape
    assert lib.cfx_compress_batch(ctx, 8, 8, 64, 0, 0, 1, items, None, 0, None) == -1            # null x
    items[0] = _lib.CompItem(0x1002, None, None, 0x2000)
    assert lib.cfx_compress_batch(ctx, 8, 8, 64, 0, 0, 1, items, None, 0, None) == -3
    items[0] = _lib.CompItem(0x1000, None, None, 0x2000)
    assert lib.cfx_compress_batch(ctx, 8, 8, 64, 0, 1, 1, items, None, 0, None) == -1            # UPDATE_CACHE without new_base
    assert lib.cfx_decompress_batch(ctx, 8, 8, 64, 0, 1, d, None) == -1
    d[0] = _lib.DecompItem(0x2000, 0x3008, 0x3000)
    assert lib.cfx_decompress_batch(ctx, 8, 8, 64, 0, 1, d, None) == -3
    items = (_lib.CompItem * 1)()
    for bad in (0x108, 7, 0x208):
        assert lib.cfx_compress_batch(ctx, bad, 8, 64, 0, 0, 1, items, None, 0, None) == -4, hex(bad)     # CFX_ERR_CODEC
        assert lib.cfx_decompress_batch(ctx, bad, 8, 64, 0, 1, d, None) == -4, hex(bad)
    # ride-along reconstruction items stay the 1-bit codec's
    items[0] = _lib.CompItem(0x1000, None, None, 0x2000)
    ride = (_lib.DecompItem * 1)(_lib.DecompItem(0x2000, 0x3000, 0x3000))
    assert lib.cfx_compress_batch_ex(ctx, 8, 8, 64, 0, 0, 1, items, 1, ride, None, 0, None) == -4
    lib.cfx_destroy(ctx)


def test_abi_plan_ops_and_second_order_refusals():
    from compactfusion_amd import _lib
    lib = _lib.load()
    ctx = lib.cfx_create(0)
    plan = lib.cfx_plan_create(ctx)
    c = (_lib.CompItem * 2)(_lib.CompItem(0x1000, 0x2000, 0x2000, 0x3000), _lib.CompItem(0x4000, 0x5000, 0x5000, 0x6000))
    dd = (_lib.DecompItem * 14)(*[_lib.DecompItem(0x7000, 0x8000, 0x8000)] * 14)
    assert lib.cfx_plan_add_compress(plan, 8, 544, 3072, 0, 1, 2, c, None, 0) == 0
    assert lib.cfx_plan_add_decompress(plan, 8, 544, 3072, 0, 14, dd) == 1
    assert lib.cfx_plan_add_compress_gated(plan, 8, 544, 3072, 0, 1, 2, c, 0, None, 14, dd, None, 0) == 2
    assert lib.cfx_plan_add_compress(plan, 8, 544, 3080, 0, 1, 2, c, None, 0) == -2
    assert lib.cfx_plan_add_compress(plan, 8, 544, 3072, 2, 1, 2, c, None, 0) == -2
    assert lib.cfx_plan_add_compress(plan, 0x108, 544, 3072, 0, 1, 2, c, None, 0) == -4
    assert lib.cfx_plan_add_decompress(plan, 0x108, 544, 3072, 0, 14, dd) == -4
    ride = (_lib.DecompItem * 1)(_lib.DecompItem(0x7000, 0x8000, 0x8000))
    assert lib.cfx_plan_add_compress_ex(plan, 8, 544, 3072, 0, 1, 2, c, 1, ride, None, 0) == -4
    assert lib.cfx_plan_add_exchange_layer(plan, 0x108, 544, 3072, 0, 1, 2, c, 14, dd, None, None, None, 0, None, 0) == -4
    assert lib.cfx_plan_add_exchange_layer(plan, 7, 544, 3072, 0, 1, 2, c, 14, dd, None, None, None, 0, None, 0) == -4
    other = lib.cfx_plan_create(ctx)
    assert [lib.cfx_plan_copy_op(other, plan, i) for i in range(3)] == [0, 1, 2]
    # second-order states: refused as for INT4 (residual 2 composes cfx_residual2_delta / _update around the codec)
    s2 = (_lib.SecondItem * 2)(_lib.SecondItem(0xa000, 0xa000), _lib.SecondItem(0xb000, 0xb000))
    assert lib.cfx_compress_batch_res2(ctx, 8, 544, 3072, 0, 1, 2, c, s2, 0.5, None, 0, None) == -4
    d2 = (_lib.DecompItem * 2)(_lib.DecompItem(0x7000, 0x8000, 0x8000), _lib.DecompItem(0x7000, 0x8000, 0x8000))
    assert lib.cfx_decompress_batch_res2(ctx, 8, 544, 3072, 0, 2, d2, s2, 0.5, None) == -4
    assert lib.cfx_plan_set_second_order(plan, 0, 2, s2, 0, None, 0.5) == -4
    # the peer-to-peer exchange layer refuses 7 and 0x108 and takes 8 (past the codec check it allocates a device word, which needs a GPU)
    for bad in (7, 0x108):
        assert lib.cfx_plan_add_exchange_layer_p2p(plan, bad, 544, 3072, 0, 1, 2, c, 14, dd, 0xc000, 0, None, None, 0) == -4
    rc = lib.cfx_plan_add_exchange_layer_p2p(plan, 8, 544, 3072, 0, 1, 2, c, 14, dd, 0xc000, 0, None, None, 0)
    assert rc == 3 or rc == -6, rc
    lib.cfx_plan_destroy(other)
    lib.cfx_plan_destroy(plan)
    lib.cfx_destroy(ctx)


def test_kernels_exist_without_scratch():
    """k_mx_compress, k_mx_decompress and k_mx_layer in the built library: no scratch, and the layer leaves a collective kernel room
    (at most 104 registers, as the other layer launches)"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import resource_usage
    rows = {k["demangled"].split("(")[0]: k for k in resource_usage.collect() if k["demangled"].startswith("k_mx_")}
    assert set(rows) == {"k_mx_compress", "k_mx_decompress", "k_mx_layer"}, sorted(rows)
    for k in rows.values():
        assert k.get("scratch", 0) == 0 and k["vgpr"] + k.get("agpr", 0) <= 104, k


# ---- the host state machine against the contract -------------------------------------------------------------------------------------
class _Oracle(R.OracleCompact):
    """R.OracleCompact with the contract of tests/mxfp4_contract.py as its codec 'mxfp4'"""

    def _comp(self, codec, d):
        return M.compress(d, None) if codec == "mxfp4" else super()._comp(codec, d)

    def _decomp(self, codec, pkt, N, C):
        return M.decompress(pkt, N, C) if codec == "mxfp4" else super()._decomp(codec, pkt, N, C)


MODES = [("res1_ef", dict(residual=1, ef=True), 1), ("res1_noef", dict(residual=1, ef=False), 1), ("res0", dict(residual=0, ef=False), 0),
         ("res2", dict(residual=2, ef=True, delta_decay_factor=0.5), 2)]


@pytest.mark.parametrize("mode,kw,nwarm", MODES, ids=[m[0] for m in MODES])
def test_state_machine_equals_the_contract(cpu_kernels, mode, kw, nwarm):
    """WARMUP, then compressed steps: packets, the sender's and the receiver's states (residual 2: the second-order states too) follow
    R.OracleCompact over the contract bit for bit; residual 2 runs the composition around the codec (codecs.res2_fused is false for id 8)."""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd import codecs
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    N, C = 64, 1024
    assert not codecs.res2_fused(8, torch.zeros(4, 64).half())
    assert cm._native(T.MXFP4) == (8, 0) and T.MXFP4.value == "mxfp4"
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, **kw))
    mk = lambda: _Oracle(residual=kw["residual"], ef=kw["ef"], decay=kw.get("delta_decay_factor"))      # noqa: E731
    orc_s, orc_r = mk(), mk()
    skey, rkey = "0-0-k", "0-1-k"
    g = torch.Generator().manual_seed(11)
    cur = torch.randn(N, C, generator=g).half()
    for t in range(6):
        x4 = cur.contiguous().view(1, N, 8, C // 8)
        warm = t < nwarm
        typ, name = (T.WARMUP, "warmup") if warm else (T.MXFP4, "mxfp4")
        pkt = cm.compact_compress(skey, x4, typ, update_cache=True)
        want = orc_s.compress(skey, bits(x4).reshape(1, N, 8, C // 8), name, True)
        assert np.array_equal(bits(pkt).reshape(-1), want), f"{mode} step {t}: packet"
        if not warm:
            assert pkt.numel() == M.packet_halves(N, C)
        rec = cm.compact_decompress(rkey, pkt.clone(), typ, x4.shape, update_cache=True)
        wrec = orc_r.decompress(rkey, want, name, x4.shape, True)
        assert rec.shape == x4.shape and np.array_equal(bits(rec).reshape(-1), R.bits(wrec).reshape(-1)), f"{mode} step {t}: reconstruction"
        if kw["residual"]:
            assert np.array_equal(bits(cm.compact_cache().get_base(skey)), R.bits(orc_s.base[skey])), f"{mode} step {t}: sender state"
            assert np.array_equal(bits(cm.compact_cache().get_base(rkey)), R.bits(orc_r.base[rkey])), f"{mode} step {t}: receiver state"
            if kw["ef"]:
                assert np.array_equal(bits(cm.compact_cache().get_base(skey)), bits(cm.compact_cache().get_base(rkey)))
        else:
            assert cm.compact_cache().get_base(skey) is None
        if kw["residual"] == 2 and t >= 1:
            assert np.array_equal(bits(cm.compact_cache().get_delta_base(skey)), R.bits(orc_s.dbase[skey]))
        cur = (cur.float() + 0.1 * torch.randn(N, C, generator=g)).half()


def test_simulate_mode_is_compress_then_decompress(cpu_kernels):
    """simulate_compress=True ships decode(encode(d)) at full size: the existing _sim path, compress ; decompress with base NULL"""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from compactfusion_amd.compact import slowpath as S
    N, C = 16, 128
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, C, generator=g).half()
    want = R.bits(M.compress(bits(x), None)[1])
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=0, ef=False, simulate=True))
    out = cm.compact_compress("0-0-k", x, T.MXFP4, update_cache=True)
    assert out.shape == x.shape and np.array_equal(bits(out).reshape(N, C), want)
    assert np.array_equal(bits(S.sim_compress(x, T.MXFP4)), want)
    # residual 1, simulated: recv = sim(x - base), the state takes base + recv
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=1, ef=True, simulate=True))
    cm.compact_compress("0-0-k", x, T.WARMUP, update_cache=True)
    x2 = (x.float() + 0.1 * torch.randn(N, C, generator=g)).half()
    recv = cm.compact_compress("0-0-k", x2, T.MXFP4, update_cache=True)
    d = (bits(x2).view(F16) - bits(x).view(F16)).astype(F16)
    wrecv = M.compress(d, None)[1]
    assert np.array_equal(bits(recv).reshape(N, C), R.bits(wrecv))
    assert np.array_equal(bits(cm.compact_cache().get_base("0-0-k")), R.bits((bits(x).view(F16) + wrecv).astype(F16)))
    # the wire codec through the slowpath mirror
    pkt = S.slowpath_compress(x, T.MXFP4)
    assert pkt.numel() == M.packet_halves(N, C) and np.array_equal(bits(S.slowpath_decompress(pkt, (N, C), T.MXFP4)), want)


def test_quantize_dequantize_pair_round_trip(cpu_kernels):
    from compactfusion_amd.compact import compress_quantize as Q
    N, C = 64, 256
    torch.manual_seed(42)
    d = torch.randn(N, C).half()
    codes, scales = Q.quantize_mxfp4(d)
    assert codes.shape == (N, C // 2) and codes.dtype == torch.uint8 and scales.shape == (N, C // 32) and scales.dtype == torch.uint8
    want_pkt, want_recv = M.compress(bits(d), None)
    by = want_pkt.view(np.uint8)
    assert np.array_equal(codes.numpy().reshape(-1), by[:N * C // 2]) and np.array_equal(scales.numpy().reshape(-1), by[N * C // 2:])
    rec = Q.dequantize_mxfp4(codes, scales)
    assert np.array_equal(bits(rec), R.bits(want_recv))
    assert np.array_equal(bits(Q.sim_mxfp4(d)), R.bits(want_recv))
    with pytest.raises(AssertionError):
        Q.quantize_mxfp4(d[:, :96])


def test_bf16_raises_before_any_state_changes(cpu_kernels):
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    N, C = 64, 1024
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=1, ef=True))
    cache = cm.compact_cache()
    x16 = W.drift(5, (N, C), 1)[0]
    cm.compact_compress("0-0-k", x16, T.WARMUP, update_cache=True)
    cm.compact_decompress("0-1-k", x16.clone(), T.WARMUP, (N, C), update_cache=True)
    before = {k: (v.dtype, bits(v).copy()) for k, v in cache.base.items()}
    version = cache.version
    with pytest.raises(NotImplementedError, match="MXFP4"):
        cm.compact_compress("0-0-k", x16.bfloat16(), T.MXFP4, update_cache=True)
    with pytest.raises(NotImplementedError):
        cm._decompress("0-1-k", torch.zeros(M.packet_halves(N, C)).half(), T.MXFP4, (N, C), True, torch.bfloat16)
    assert cache.version == version and {k: (v.dtype, bits(v).copy()) for k, v in cache.base.items()}.keys() == before.keys()
    for k, v in cache.base.items():
        assert v.dtype == before[k][0] and np.array_equal(bits(v), before[k][1])


def test_fastpath_still_asserts_binary_or_int2_and_the_layer_op_takes_id_8(cpu_kernels):
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from compactfusion_amd.compact import xlayer
    cm.compact_init(CompactConfig(enabled=True, residual=1, ef=True, fastpath=True, comp_rank=-1))
    x = torch.randn(1, 8, 64).half()
    cm.compact_compress("0-0-k", x, T.WARMUP, update_cache=True)
    with pytest.raises(AssertionError):
        cm.compact_compress("0-0-k", x, T.MXFP4, update_cache=True)
    assert xlayer.usable(8, 2, True) and xlayer.usable(8, 8, True) and not xlayer.usable(8, 2, False)
    assert not xlayer.usable(7, 2, True) and not xlayer.usable(9, 2, True) and all(xlayer.usable(c, 2, True) for c in range(1, 7))


# ---- compact_all_gather over two gloo ranks --------------------------------------------------------------------------------------------
def _entry(rank, world, port, out):
    W.run(MB.w_all_gather_mxfp4, rank, world, port, out)


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
                _, nb = M.residual_compress(x, state[i].view(F16))
                state[i] = R.bits(nb)
                assert np.array_equal(res[0][f"t{t}/out{i}"], state[i]), f"step {t} shard {i}: not the contract's state"
    for r in range(2):
        assert int(res[r]["passed_count"][0]) == 1
