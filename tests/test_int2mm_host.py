"""INT2_MINMAX (codec id 6) on the CPU: the C-ABI's sizes and refusals, and the host logic - state machine, residual 0 / 1 / 2, the gloo
all-gather, the stand-alone quantiser pair, the bf16 refusal - with the kernels replaced by the numpy contract through the TEST-ONLY
stand-in tests/_int2mm_backend.py (tests/_oracle_backend.py plus id 6).  The GPU tests (tests/test_gpu_int2mm.py) hold the kernels to the
same contract."""
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _dist_workers as W
import _int2mm_backend as IB
import int2mm_contract as I
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
    IB.install(monkeypatch)


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_sizes_and_shape_rule():
    from compactfusion_amd import _lib, codecs
    lib = _lib.load()
    assert int(codecs.Codec.INT2_MINMAX) == 6
    for N, C in ((4, 8), (4, 72), (544, 3072), (4448, 3072), (1028, 16)):
        assert lib.cfx_packet_bytes(6, N, C, 0) == N * C // 4 + 4 * C == 2 * I.packet_halves(N, C)
        for batch in (1, 16):
            assert lib.cfx_workspace_bytes(6, N, C, 0, batch) == lib.cfx_workspace_bytes(3, N, C, 0, batch) != 0      # INT4's workspace
    for N, C in ((2, 8), (6, 72), (543, 3072), (4, 12), (0, 8)):
        assert lib.cfx_packet_bytes(6, N, C, 0) == 0 and lib.cfx_workspace_bytes(6, N, C, 0, 1) == 0
    assert lib.cfx_packet_bytes(0x106, 544, 3072, 0) == 0 and lib.cfx_workspace_bytes(0x106, 544, 3072, 0, 2) == 0
    assert lib.cfx_packet_bytes(7, 544, 3072, 0) == 0


def test_abi_argument_errors():
    from compactfusion_amd import _lib
    lib = _lib.load()
    ctx = lib.cfx_create(0)
    assert ctx
    items = (_lib.CompItem * 1)()
    d = (_lib.DecompItem * 1)()
    assert lib.cfx_compress_batch(ctx, 6, 8, 64, 0, 0, 1, items, None, 0, None) == -1            # null x
    for N in (2, 6, 9):
        assert lib.cfx_compress_batch(ctx, 6, N, 64, 0, 0, 1, items, None, 0, None) == -2        # N % 4 != 0: CFX_ERR_SHAPE
        assert lib.cfx_decompress_batch(ctx, 6, N, 64, 0, 1, d, None) == -2
    assert lib.cfx_compress_batch(ctx, 6, 8, 20, 0, 0, 1, items, None, 0, None) == -2
    assert lib.cfx_compress_batch(ctx, 6, 8, 64, 0, 0, 0, items, None, 0, None) == -5
    items[0] = _lib.CompItem(0x1002, None, None, 0x2000)
    assert lib.cfx_compress_batch(ctx, 6, 8, 64, 0, 0, 1, items, None, 0, None) == -3
    items[0] = _lib.CompItem(0x1000, None, None, 0x2000)
    assert lib.cfx_compress_batch(ctx, 6, 8, 64, 0, 0, 1, items, None, 0, None) == -7            # workspace missing
    assert lib.cfx_decompress_batch(ctx, 6, 8, 64, 0, 1, d, None) == -1
    items = (_lib.CompItem * 1)()
    for bad in (0x106, 7):
        assert lib.cfx_compress_batch(ctx, bad, 8, 64, 0, 0, 1, items, None, 0, None) == -4, hex(bad)     # CFX_ERR_CODEC
        assert lib.cfx_decompress_batch(ctx, bad, 8, 64, 0, 1, d, None) == -4, hex(bad)
    # ride-along reconstruction items stay the 1-bit codec's
    items[0] = _lib.CompItem(0x1000, None, None, 0x2000)
    ride = (_lib.DecompItem * 1)(_lib.DecompItem(0x2000, 0x3000, 0x3000))
    assert lib.cfx_compress_batch_ex(ctx, 6, 8, 64, 0, 0, 1, items, 1, ride, 0x9000, 1 << 20, None) == -4
    lib.cfx_destroy(ctx)


def test_abi_plan_ops_and_second_order_refusals():
    from compactfusion_amd import _lib
    lib = _lib.load()
    ctx = lib.cfx_create(0)
    plan = lib.cfx_plan_create(ctx)
    c = (_lib.CompItem * 2)(_lib.CompItem(0x1000, 0x2000, 0x2000, 0x3000), _lib.CompItem(0x4000, 0x5000, 0x5000, 0x6000))
    dd = (_lib.DecompItem * 14)(*[_lib.DecompItem(0x7000, 0x8000, 0x8000)] * 14)
    assert lib.cfx_plan_add_compress(plan, 6, 544, 3072, 0, 1, 2, c, 0x9000, 1 << 22) == 0
    assert lib.cfx_plan_add_decompress(plan, 6, 544, 3072, 0, 14, dd) == 1
    assert lib.cfx_plan_add_compress(plan, 6, 542, 3072, 0, 1, 2, c, 0x9000, 1 << 22) == -2
    assert lib.cfx_plan_add_compress(plan, 0x106, 544, 3072, 0, 1, 2, c, 0x9000, 1 << 22) == -4
    assert lib.cfx_plan_add_decompress(plan, 0x106, 544, 3072, 0, 14, dd) == -4
    # the exchange-layer op takes the codec (peer-to-peer form: no exchange stream to create)
    assert lib.cfx_plan_add_exchange_layer(plan, 0x106, 544, 3072, 0, 1, 2, c, 14, dd, None, None, None, 0, 0x9000, 1 << 22) == -4
    assert lib.cfx_plan_add_exchange_layer(plan, 7, 544, 3072, 0, 1, 2, c, 14, dd, None, None, None, 0, 0x9000, 1 << 22) == -4
    other = lib.cfx_plan_create(ctx)
    assert lib.cfx_plan_copy_op(other, plan, 0) == 0 and lib.cfx_plan_copy_op(other, plan, 1) == 1
    # second-order states: refused as for codecs 3 - 5 (residual 2 composes cfx_residual2_delta / _update around the codec)
    s2 = (_lib.SecondItem * 2)(_lib.SecondItem(0xa000, 0xa000), _lib.SecondItem(0xb000, 0xb000))
    assert lib.cfx_compress_batch_res2(ctx, 6, 544, 3072, 0, 1, 2, c, s2, 0.5, 0x9000, 1 << 22, None) == -4
    d2 = (_lib.DecompItem * 2)(_lib.DecompItem(0x7000, 0x8000, 0x8000), _lib.DecompItem(0x7000, 0x8000, 0x8000))
    assert lib.cfx_decompress_batch_res2(ctx, 6, 544, 3072, 0, 2, d2, s2, 0.5, None) == -4
    assert lib.cfx_plan_set_second_order(plan, 0, 2, s2, 0, None, 0.5) == -4
    # ... and takes id 6 (peer-to-peer form: no exchange stream to create; past the codec check it allocates a device word, which needs a GPU)
    rc = lib.cfx_plan_add_exchange_layer_p2p(plan, 7, 544, 3072, 0, 1, 2, c, 14, dd, 0xc000, 0, None, 0x9000, 1 << 22)
    assert rc == -4
    rc = lib.cfx_plan_add_exchange_layer_p2p(plan, 6, 544, 3072, 0, 1, 2, c, 14, dd, 0xc000, 0, None, 0x9000, 1 << 22)
    assert rc == 2 or rc == -6, rc
    lib.cfx_plan_destroy(other)
    lib.cfx_plan_destroy(plan)
    lib.cfx_destroy(ctx)


# ---- the host state machine against the contract -------------------------------------------------------------------------------------
class _Oracle(R.OracleCompact):
    """R.OracleCompact with the contract of tests/int2mm_contract.py as its codec 'int2mm'"""

    def _comp(self, codec, d):
        return I.compress(d, None) if codec == "int2mm" else super()._comp(codec, d)

    def _decomp(self, codec, pkt, N, C):
        return I.decompress(pkt, N, C) if codec == "int2mm" else super()._decomp(codec, pkt, N, C)


MODES = [("res1_ef", dict(residual=1, ef=True), 1), ("res1_noef", dict(residual=1, ef=False), 1), ("res0", dict(residual=0, ef=False), 0),
         ("res2", dict(residual=2, ef=True, delta_decay_factor=0.5), 2)]


@pytest.mark.parametrize("mode,kw,nwarm", MODES, ids=[m[0] for m in MODES])
def test_state_machine_equals_the_contract(cpu_kernels, mode, kw, nwarm):
    """WARMUP, then compressed steps: packets, the sender's and the receiver's states (residual 2: the second-order states too) follow
    R.OracleCompact over the contract bit for bit; residual 2 runs the composition around the codec (codecs.res2_fused is false for id 6)."""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd import codecs
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    N, C = 64, 1024
    assert not codecs.res2_fused(6, torch.zeros(4, 8).half())
    assert cm._native(T.INT2_MINMAX) == (6, 0)
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, **kw))
    mk = lambda: _Oracle(residual=kw["residual"], ef=kw["ef"], decay=kw.get("delta_decay_factor"))      # noqa: E731
    orc_s, orc_r = mk(), mk()
    skey, rkey = "0-0-k", "0-1-k"
    g = torch.Generator().manual_seed(11)
    cur = torch.randn(N, C, generator=g).half()
    for t in range(6):
        x4 = cur.contiguous().view(1, N, 8, C // 8)
        warm = t < nwarm
        typ, name = (T.WARMUP, "warmup") if warm else (T.INT2_MINMAX, "int2mm")
        pkt = cm.compact_compress(skey, x4, typ, update_cache=True)
        want = orc_s.compress(skey, bits(x4).reshape(1, N, 8, C // 8), name, True)
        assert np.array_equal(bits(pkt).reshape(-1), want), f"{mode} step {t}: packet"
        if not warm:
            assert pkt.numel() == I.packet_halves(N, C)
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


def test_simulate_mode_keeps_the_simulation_function(cpu_kernels):
    """simulate_compress=True still returns sim_int2_minmax(d) - NaN on a constant channel, where the wire codec reconstructs min"""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from compactfusion_amd.compact import slowpath as S
    N, C = 16, 64
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, C, generator=g).half()
    x[:, 5] = 0.25
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=0, ef=False, simulate=True))
    out = cm.compact_compress("0-0-k", x, T.INT2_MINMAX, update_cache=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = R.bits(R.sim_int2_minmax(bits(x)))
    got = bits(out).reshape(N, C)
    nan = lambda a: (a & 0x7FFF) > 0x7C00          # noqa: E731
    assert nan(want[:, 5]).all() and nan(got[:, 5]).all() and np.array_equal(got[~nan(want)], want[~nan(want)])
    sim = bits(S.sim_compress(x, T.INT2_MINMAX))
    assert nan(sim[:, 5]).all() and np.array_equal(sim[~nan(want)], want[~nan(want)])
    # the wire codec through the slowpath mirror: code 0, min
    pkt = S.slowpath_compress(x, T.INT2_MINMAX)
    assert pkt.numel() == I.packet_halves(N, C)
    rec = bits(S.slowpath_decompress(pkt, (N, C), T.INT2_MINMAX))
    assert np.array_equal(rec[:, 5], bits(x)[:, 5])
    assert np.array_equal(rec[~nan(want)], want[~nan(want)])


def test_quantize_dequantize_pair_round_trip(cpu_kernels):
    from compactfusion_amd.compact import compress_quantize as Q
    N, C = 64, 256
    torch.manual_seed(42)
    d = torch.randn(N, C).half()
    packed, scale, mn = Q.quantize_int2_minmax(d)
    assert packed.shape == (N // 4, C) and packed.dtype == torch.uint8 and scale.shape == (1, C) and mn.shape == (1, C)
    want_pkt, want_recv = I.compress(bits(d), None)
    qn = N * C // 8
    assert np.array_equal(packed.numpy().reshape(-1), want_pkt[:qn].view(np.uint8))
    assert np.array_equal(bits(scale).reshape(-1), want_pkt[qn:qn + C]) and np.array_equal(bits(mn).reshape(-1), want_pkt[qn + C:])
    rec = Q.dequantize_int2_minmax(packed, scale, mn)
    assert np.array_equal(bits(rec), R.bits(want_recv)) and np.array_equal(bits(rec), R.bits(R.sim_int2_minmax(bits(d))))
    assert np.array_equal(bits(Q.sim_int2_minmax(d)), bits(rec))           # (no constant channel here: the simulation equals the wire codec)
    with pytest.raises(AssertionError):
        Q.quantize_int2_minmax(d[:62])


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
    with pytest.raises(NotImplementedError, match="INT2_MINMAX"):
        cm.compact_compress("0-0-k", x16.bfloat16(), T.INT2_MINMAX, update_cache=True)
    with pytest.raises(NotImplementedError):
        cm._decompress("0-1-k", torch.zeros(I.packet_halves(N, C)).half(), T.INT2_MINMAX, (N, C), True, torch.bfloat16)
    assert cache.version == version and {k: (v.dtype, bits(v).copy()) for k, v in cache.base.items()}.keys() == before.keys()
    for k, v in cache.base.items():
        assert v.dtype == before[k][0] and np.array_equal(bits(v), before[k][1])


def test_fastpath_still_asserts_binary_or_int2(cpu_kernels):
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from compactfusion_amd.compact import xlayer
    cm.compact_init(CompactConfig(enabled=True, residual=1, ef=True, fastpath=True, comp_rank=-1))
    x = torch.randn(1, 8, 64).half()
    cm.compact_compress("0-0-k", x, T.WARMUP, update_cache=True)
    with pytest.raises(AssertionError):
        cm.compact_compress("0-0-k", x, T.INT2_MINMAX, update_cache=True)
    assert xlayer.usable(6, 2, True) and not xlayer.usable(6, 2, False) and not xlayer.usable(7, 2, True)


# ---- compact_all_gather over two gloo ranks --------------------------------------------------------------------------------------------
def _entry(rank, world, port, out):
    W.run(IB.w_all_gather_int2mm, rank, world, port, out)


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
                _, nb = I.residual_compress(x, state[i].view(F16))
                state[i] = R.bits(nb)
                assert np.array_equal(res[0][f"t{t}/out{i}"], state[i]), f"step {t} shard {i}: not the contract's state"
    for r in range(2):
        assert int(res[r]["passed_count"][0]) == 1
