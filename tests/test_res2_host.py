"""Second-order residual inside the 1-bit and 2-bit codec launches - everything that can be checked without a GPU: the contract
(tests/res2_contract.py) against the pinned oracle's state machine, the three C-ABI entry points and their argument errors, the
compiled kernels' resource rows, and the host state machine's calls (one fused call per tensor where the predicate holds, today's
composition where it does not).  Every comparison is of bits."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _dist_workers as W
import _oracle_backend as OB
import res2_contract as RC
from oracle import ref_np as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODECS = [("binary", 1, "BINARY"), ("int2", 2, "INT2")]
DECAYS = (0.0, 0.3, 0.5, 1.0)


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


@pytest.fixture(autouse=True)
def _collector(tmp_path):
    from compactfusion_amd.collector import collector
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    yield


# ---- 1. the contract is the oracle's residual-2 state machine --------------------------------------------------------------------------
@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("name,cid,tname", CODECS)
def test_contract_equals_the_oracle_state_machine(name, cid, tname, decay):
    N, C = 34, 72
    xs = [bits(x).reshape(N, C) for x in W.drift(23, (N, C), 5)]
    snd, rcv = R.OracleCompact(residual=2, decay=decay), R.OracleCompact(residual=2, decay=decay)
    for t, x in enumerate(xs):
        if t < 2:
            pkt = snd.compress("k", x.view(np.float16), "warmup", True)
            rcv.decompress("k", pkt, "warmup", (N, C), True)
            continue
        b0, d0 = R.bits(snd.base["k"]).copy(), R.bits(snd.dbase["k"]).copy()
        rb0, rd0 = R.bits(rcv.base["k"]).copy(), R.bits(rcv.dbase["k"]).copy()
        dd = R.residual2_delta(x.view(np.float16), b0.view(np.float16), d0.view(np.float16))
        assert np.isfinite(dd).all() and np.abs(dd.astype(np.float32)).max() < 1.0
        want_pkt = snd.compress("k", x.view(np.float16), name, True)
        want_rec = rcv.decompress("k", want_pkt, name, (N, C), True)
        pkt, nb, nd = RC.compress(name, x, b0, d0, decay)
        assert np.array_equal(pkt, np.asarray(want_pkt).view(np.uint16).reshape(-1)), f"step {t}: packet"
        assert np.array_equal(nb, R.bits(snd.base["k"])), f"step {t}: sender base"
        assert np.array_equal(nd, R.bits(snd.dbase["k"])), f"step {t}: sender delta_base"
        rec, rnd = RC.decompress(name, pkt, rb0, rd0, decay, N, C)
        assert np.array_equal(rec, R.bits(want_rec)) and np.array_equal(rec, R.bits(rcv.base["k"])), f"step {t}: reconstruction"
        assert np.array_equal(rnd, R.bits(rcv.dbase["k"])), f"step {t}: receiver delta_base"
        assert np.isfinite(nb.view(np.float16)).all() and np.isfinite(nd.view(np.float16)).all()
        if decay == 0.0:
            assert not (nd & 0x7fff).any()              # (+-0: the predictor falls back to first order)


# ---- 2. C-ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_argument_errors_without_a_gpu():
    from compactfusion_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "cfx.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for sym in ("cfx_compress_batch_res2", "cfx_decompress_batch_res2", "cfx_plan_set_second_order"):
        assert sym + "(" in hdr and hasattr(lib, sym) and sym in bound, sym
    assert "Second-order residual" in hdr and lib.cfx_abi_version() == 2
    ctx = lib.cfx_create(0)
    assert ctx
    N, C = 8, 64
    ok_c = _lib.CompItem(0x1000, 0x2000, 0x2000, 0x3000)
    ok_s = _lib.SecondItem(0x4000, 0x4000)

    def comp(codec=1, flags=1, batch=1, item=ok_c, sec=ok_s, ws=None, wsn=0, second=True):
        items = (_lib.CompItem * 1)(item)
        s2 = (_lib.SecondItem * 1)(sec) if second else None
        return lib.cfx_compress_batch_res2(ctx, codec, N, C, 0, flags, batch, items, s2, 0.5, ws, wsn, None)

    def dec(codec=1, batch=1, item=_lib.DecompItem(0x3000, 0x2000, 0x2000), sec=ok_s, second=True):
        items = (_lib.DecompItem * 1)(item)
        s2 = (_lib.SecondItem * 1)(sec) if second else None
        return lib.cfx_decompress_batch_res2(ctx, codec, N, C, 0, batch, items, s2, 0.5, None)
    for cid in (1, 2):
        assert comp(cid, second=False) == -1                                                          # no second-order states
        assert comp(cid, sec=_lib.SecondItem(None, 0x4000)) == -1                                      # null delta_base
        assert comp(cid, item=_lib.CompItem(0x1000, None, 0x2000, 0x3000)) == -1                       # null base
        assert comp(cid, sec=_lib.SecondItem(0x4000, None)) == -1                                      # UPDATE_CACHE without new_delta_base
        assert comp(cid, sec=_lib.SecondItem(0x4002, 0x4000)) == -3                                    # misaligned delta_base
        assert comp(cid, sec=_lib.SecondItem(0x4000, 0x4008)) == -3                                    # misaligned new_delta_base
        assert comp(cid, item=_lib.CompItem(0x1002, 0x2000, 0x2000, 0x3000)) == -3                     # misaligned x
        assert comp(cid, flags=1 | _lib.FLAG_NO_EF) == -4                                              # error feedback cannot be off
        assert comp(cid | _lib.ELEM_BF16) == -4                                                        # bf16
        assert comp(cid, batch=17) == -5 and comp(cid, batch=0) == -5
        assert comp(cid) == -7 and b"workspace" in lib.cfx_last_error_string(ctx)                      # everything else in order: no workspace
        assert comp(cid, flags=0, sec=_lib.SecondItem(0x4000, None)) == -7                             # (no update: new_delta_base not needed)
        assert dec(cid, second=False) == -1
        assert dec(cid, sec=_lib.SecondItem(None, None)) == -1                                         # null delta_base
        assert dec(cid, item=_lib.DecompItem(0x3000, None, 0x2000)) == -1                              # null base
        assert dec(cid, item=_lib.DecompItem(None, 0x2000, 0x2000)) == -1
        assert dec(cid, sec=_lib.SecondItem(0x4002, None)) == -3
        assert dec(cid, item=_lib.DecompItem(0x3000, 0x2004, 0x2000)) == -3
        assert dec(cid | _lib.ELEM_BF16) == -4
        assert dec(cid, batch=17) == -5
    for cid in (3, 4, 9):
        assert comp(cid) == -4 and dec(cid) == -4, cid
    lib2 = lib.cfx_compress_batch_res2
    items = (_lib.CompItem * 1)(ok_c)
    s2 = (_lib.SecondItem * 1)(ok_s)
    ditems = (_lib.DecompItem * 1)(_lib.DecompItem(0x3000, 0x2000, 0x2000))
    assert lib2(ctx, 5, 16, 64, 8, 1, 1, items, s2, 0.5, None, 0, None) == -4                         # top-k (a shape it accepts)
    assert lib.cfx_decompress_batch_res2(ctx, 5, 16, 64, 8, 1, ditems, s2, 0.5, None) == -4
    assert lib2(ctx, 1, 8, 20, 0, 1, 1, items, s2, 0.5, None, 0, None) == -2                          # bad shape
    assert lib2(None, 1, 8, 64, 0, 1, 1, items, s2, 0.5, None, 0, None) == -1

    # cfx_plan_set_second_order
    plan = lib.cfx_plan_create(ctx)
    c = (_lib.CompItem * 2)(_lib.CompItem(0x1000, 0x2000, 0x2000, 0x3000), _lib.CompItem(0x4000, 0x5000, 0x5000, 0x6000))
    d = (_lib.DecompItem * 14)(*[_lib.DecompItem(0x3000, 0x7000 + 0x1000 * i, 0x7000 + 0x1000 * i) for i in range(14)])
    c2 = (_lib.SecondItem * 2)(_lib.SecondItem(0x20000, 0x20000), _lib.SecondItem(0x21000, 0x21000))
    r2 = (_lib.SecondItem * 14)(*[_lib.SecondItem(0x30000 + 0x1000 * i, 0x30000 + 0x1000 * i) for i in range(14)])
    so = lib.cfx_plan_set_second_order
    assert lib.cfx_plan_add_compress(plan, 1, 544, 3072, 0, 1, 2, c, 0x9000, 1 << 22) == 0
    assert lib.cfx_plan_add_decompress(plan, 2, 544, 3072, 0, 14, d) == 1
    assert so(plan, 0, 2, c2, 0, None, 0.5) == 0
    assert so(plan, 1, 0, None, 14, r2, 0.5) == 0
    assert so(plan, 2, 2, c2, 0, None, 0.5) == -5 and so(plan, -1, 2, c2, 0, None, 0.5) == -5         # op index out of range
    assert so(plan, 0, 1, c2, 0, None, 0.5) == -5 and so(plan, 0, 2, c2, 1, r2, 0.5) == -5            # wrong counts
    assert so(plan, 1, 0, None, 13, r2, 0.5) == -5 and so(plan, 1, 2, c2, 14, r2, 0.5) == -5
    assert so(plan, 0, 2, None, 0, None, 0.5) == -1
    bad = (_lib.SecondItem * 2)(_lib.SecondItem(0x20000, 0x20000), _lib.SecondItem(None, 0x21000))
    assert so(plan, 0, 2, bad, 0, None, 0.5) == -1
    bad = (_lib.SecondItem * 2)(_lib.SecondItem(0x20000, 0x20000), _lib.SecondItem(0x21004, 0x21000))
    assert so(plan, 0, 2, bad, 0, None, 0.5) == -3
    # codecs and flags without a second-order form; a flag op; an op with ride-along items
    assert lib.cfx_plan_add_compress(plan, 3, 544, 3072, 0, 1, 2, c, 0x9000, 1 << 22) == 2
    assert so(plan, 2, 2, c2, 0, None, 0.5) == -4
    assert lib.cfx_plan_add_compress(plan, 0x101, 544, 3072, 0, 1, 2, c, 0x9000, 1 << 22) == 3
    assert so(plan, 3, 2, c2, 0, None, 0.5) == -4
    assert lib.cfx_plan_add_compress(plan, 1, 544, 3072, 0, 1 | _lib.FLAG_NO_EF, 2, c, 0x9000, 1 << 22) == 4
    assert so(plan, 4, 2, c2, 0, None, 0.5) == -4
    assert lib.cfx_plan_add_compress_ex(plan, 1, 544, 3072, 0, 0, 2, c, 14, d, 0x9000, 1 << 22) == 5
    assert so(plan, 5, 2, c2, 0, None, 0.5) == -4
    q0 = (ctypes.c_void_p * 2)(0xa000, 0xb000)
    assert lib.cfx_plan_add_lr_compress(plan, 0, 544, 3072, 8, 1, 2, c, q0, 0x9000, 1 << 20) == 6
    assert so(plan, 6, 2, c2, 0, None, 0.5) == -5                                                     # not a codec op of the streaming family
    # the states travel with a copied op; activations are re-pointed as before
    other = lib.cfx_plan_create(ctx)
    assert lib.cfx_plan_copy_op(other, plan, 0) == 0 and lib.cfx_plan_copy_op(other, plan, 1) == 1
    assert lib.cfx_plan_set_input(plan, 0, 1, 0xc000) == 0 and lib.cfx_plan_set_input(other, 0, 0, 0xc000) == 0
    # exchange layers: one state per compress item and one per reconstruction item
    xl = lib.cfx_plan_create(ctx)
    assert lib.cfx_plan_use_exchange_stream(xl, 0x5678) == 0
    assert lib.cfx_plan_add_exchange_layer(xl, 1, 544, 3072, 0, 1, 2, c, 14, d, None, None, None, 0, 0x9000, 1 << 22) == 0
    assert so(xl, 0, 2, c2, 14, r2, 0.5) == 0
    assert so(xl, 0, 2, c2, 0, None, 0.5) == -5 and so(xl, 0, 0, None, 14, r2, 0.5) == -5
    for p in (xl, other, plan):
        lib.cfx_plan_destroy(p)
    lib.cfx_destroy(ctx)


def test_predicate_and_cpu_tensors():
    from compactfusion_amd import codecs as K
    from compactfusion_amd._lib import CfxError
    t = torch.zeros(8, 64, dtype=torch.float16)
    assert not K.res2_fused(1, t, t) and not K.res2_fused(2, t) and not K.res2_fused(1)        # CPU tensors: the composition
    for cid in (3, 4, 5, 101):
        assert not K.res2_fused(cid, t)
    with pytest.raises(CfxError):
        K.compress_batch_res2(1, [t], [t], [t], [t], [t], [torch.zeros(128, dtype=torch.float16)], 8, 64, 0.5)
    with pytest.raises(CfxError):
        K.decompress_batch_res2(1, [torch.zeros(128, dtype=torch.float16)], [t], [t], [t], [t], 8, 64, 0.5)


# ---- 3. the compiled kernels ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_usage
    return {k["demangled"]: k for k in resource_usage.collect() if k["file"] == "cfx_absmean.hip"}


def test_second_order_kernels_exist_without_scratch(rows):
    """Every launch cfx_i_absmean_compress / _decompress dispatch without gated items has its second-order twin, under a name of its own
    (the first-order kernels keep their names and rows: tests/test_bf16_host.py), none with scratch.
    Registers over the fp16 twin: the reconstruction and quantise kernels carry one more operand per row in flight (4 registers a row,
    plus addresses); the statistics tile loops gain ONE load per row in flight - 4 rows: 16 registers of data and its address, observed
    +18 for all four 4-row forms (k_absmean_stats2<true> 86 vs 68, <false> 81 vs 63, k_absmean_compress2<true, 4> 88 vs 70,
    <false, 4> 83 vs 65) and +4 / +0 for the 2-row forms (64 vs 60, 60 vs 60).  Bound: 4 registers per row in flight + 4."""
    twins = {"k_absmean_compress2<true, 4>": ("k_absmean_compress<true, 4, false, false, ElemF16>", 4),
             "k_absmean_compress2<true, 2>": ("k_absmean_compress<true, 2, false, false, ElemF16>", 2),
             "k_absmean_compress2<false, 4>": ("k_absmean_compress<false, 4, false, false, ElemF16>", 4),
             "k_absmean_compress2<false, 2>": ("k_absmean_compress<false, 2, false, false, ElemF16>", 2),
             "k_absmean_stats2<true>": ("k_absmean_stats<true, ElemF16>", 4),
             "k_absmean_stats2<false>": ("k_absmean_stats<false, ElemF16>", 4),
             "k_int2_quant2": ("k_int2_quant<ElemF16>", 2),
             "k_int2_dequant2": ("k_int2_dequant<ElemF16>", 2),
             "k_binary_dequant2<2>": ("k_binary_dequant<2, ElemF16>", 2),
             "k_binary_dequant2<4>": ("k_binary_dequant<4, ElemF16>", 4)}
    for name, (twin, rows_in_flight) in twins.items():
        assert name in rows, name
        assert twin in rows, twin
        k, t = rows[name], rows[twin]
        assert k.get("scratch", 0) == 0, k
        assert "ElemF16" not in name and "ElemBF16" not in name
        over = k["vgpr"] + k.get("agpr", 0) - t["vgpr"] - t.get("agpr", 0)
        print(f"{name}: {k['vgpr']} VGPRs, {over:+d} over {twin}")
        if "stats2" in name or "compress2" in name:
            assert over <= 4 * rows_in_flight + 4, (name, over)
            assert k["lds"] == t["lds"], (name, k["lds"], t["lds"])
        if "k_absmean_compress" in name:
            assert k["vgpr"] + k.get("agpr", 0) <= 128 and k["lds"] <= 80 * 1024, k


# ---- 4. the host state machine -------------------------------------------------------------------------------------------------------
@pytest.fixture
def spy(monkeypatch):
    """the oracle stand-in for today's calls, the contract stand-in for the fused ones, and a log of which were made"""
    from compactfusion_amd import codecs
    OB.install(monkeypatch)
    log = []
    for fn in ("compress_batch", "decompress_batch", "residual2_delta", "residual2_update"):
        def wrap(*a, _f=getattr(codecs, fn), _n=fn, **kw):
            log.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(codecs, fn, wrap)
    for fn in ("compress_batch_res2", "decompress_batch_res2"):
        def wrap2(*a, _f=getattr(RC, fn), _n=fn, **kw):
            log.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(codecs, fn, wrap2)
    import compactfusion_amd.compact.main as cm
    yield log
    cm._packets.clear()


@pytest.mark.parametrize("upd", [True, False], ids=["update_cache", "no_update"])
@pytest.mark.parametrize("name,cid,tname", CODECS)
def test_state_machine_makes_one_fused_call(spy, monkeypatch, name, cid, tname, upd):
    """2 WARMUP + 4 steps.  update_cache: sender and receiver base / delta_base follow the OracleCompact replay bit for bit.  Without it
    (the states stay where the second WARMUP left them) packet and reconstruction follow it, and nothing is stored."""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd import codecs
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    monkeypatch.setattr(codecs, "res2_fused", lambda codec, *ts: int(codec) in (1, 2))
    N, C = 34, 72
    decay = 0.5
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=2, ef=True, comp_rank=-1, delta_decay_factor=decay))
    snd, rcv = R.OracleCompact(residual=2, decay=decay), R.OracleCompact(residual=2, decay=decay)
    skey, rkey = "0-0-k", "0-1-k"
    cache = cm.compact_cache
    for t, x in enumerate(W.drift(31, (N, C), 6)):
        x4 = x.view(1, N, 8, C // 8)
        warm = t < 2
        del spy[:]
        pkt = cm.compact_compress(skey, x4, T.WARMUP if warm else T[tname], update_cache=warm or upd)
        want = snd.compress(skey, bits(x4).view(np.float16).reshape(1, N, 8, C // 8), "warmup" if warm else name, warm or upd)
        assert np.array_equal(bits(pkt).reshape(-1), np.asarray(want).view(np.uint16).reshape(-1)), f"step {t}: packet"
        rec = cm.compact_decompress(rkey, pkt.clone(), T.WARMUP if warm else T[tname], x4.shape, update_cache=warm or upd)
        wrec = rcv.decompress(rkey, want, "warmup" if warm else name, x4.shape, warm or upd)
        assert rec.shape == x4.shape and np.array_equal(bits(rec).reshape(-1), R.bits(wrec).reshape(-1)), f"step {t}: reconstruction"
        if not warm:
            assert spy == ["compress_batch_res2", "decompress_batch_res2"], spy
        else:
            assert spy == []
        for key, orc in ((skey, snd), (rkey, rcv)):
            assert np.array_equal(bits(cache().get_base(key)).reshape(-1), R.bits(orc.base[key]).reshape(-1)), f"step {t}: base {key}"
            if t >= 1:
                assert np.array_equal(bits(cache().get_delta_base(key)).reshape(-1), R.bits(orc.dbase[key]).reshape(-1)), f"step {t}: delta_base {key}"
    assert not [k for k in cm._packets if k[1] in ("dd", "recv", "ndb")], "the fused path allocates no scratch tensors"


@pytest.mark.parametrize("tname,want_fused", [("BINARY", False), ("INT2", False), ("INT4", False)])
def test_predicate_off_keeps_todays_calls(spy, tname, want_fused):
    """CPU tensors (the real predicate says no), and a codec without a fused form: delta ; codec ; decode ; update, as before"""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    N, C = 34, 72
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=2, ef=True, comp_rank=-1, delta_decay_factor=0.5))
    for t, x in enumerate(W.drift(31, (N, C), 4)):
        del spy[:]
        typ = T.WARMUP if t < 2 else T[tname]
        pkt = cm.compact_compress("0-0-k", x, typ, update_cache=True)
        if t >= 2:
            assert spy == ["residual2_delta", "compress_batch", "decompress_batch", "residual2_update"], spy
        del spy[:]
        cm.compact_decompress("0-1-k", pkt.clone(), typ, x.shape, update_cache=(t != 3))
        if t >= 2:
            assert spy == ["decompress_batch", "residual2_update"], spy
    assert [k for k in cm._packets if k[1] in ("dd", "recv")]


def test_forced_predicate_leaves_other_codecs_and_stats_logging_alone(spy, monkeypatch):
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd import codecs
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    monkeypatch.setattr(codecs, "res2_fused", lambda codec, *ts: int(codec) in (1, 2))
    N, C = 34, 72
    xs = W.drift(31, (N, C), 3)
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=2, ef=True, comp_rank=-1, delta_decay_factor=0.5))
    for x in xs[:2]:
        cm.compact_compress("0-0-k", x, T.WARMUP, update_cache=True)
    del spy[:]
    cm.compact_compress("0-0-k", xs[2], T.INT8, update_cache=True)
    assert spy == ["residual2_delta", "compress_batch", "decompress_batch", "residual2_update"], spy
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=2, ef=True, comp_rank=-1, delta_decay_factor=0.5,
                                  log_stats=True))
    for x in xs[:2]:
        cm.compact_compress("0-0-k", x, T.WARMUP, update_cache=True)
    del spy[:]
    cm.compact_compress("0-0-k", xs[2], T.BINARY, update_cache=True)
    assert spy == ["residual2_delta", "compress_batch", "decompress_batch", "residual2_update"], spy
