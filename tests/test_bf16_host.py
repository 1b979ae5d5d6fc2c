"""bf16 activations in the 1-bit and 2-bit exchange - everything that can be checked without a GPU: the C-ABI's sizes and argument errors
with CFX_ELEM_BF16, the host state machine on the bf16 stand-in (tests/_bf16_backend.py) against the contract (tests/bf16_contract.py),
the refused combinations, the gloo all-gathers, the quality of the contract itself, and the compiled kernels' resource rows."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _bf16_backend as BB
import _bf16_workers as BW
import _dist_workers as W
import bf16_contract as BC
from oracle import ref_np as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = BC.ELEM_BF16
bits = BC.torch_bits


@pytest.fixture
def cpu_kernels(monkeypatch, tmp_path):
    BB.install(monkeypatch)
    from compactfusion_amd.collector import collector
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    import compactfusion_amd.compact.main as cm
    yield
    cm._packets.clear()


def _drift(seed, N, C, T):
    return [x.bfloat16() for x in W.drift(seed, (N, C), T)]


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_sizes_with_the_element_bit():
    from compactfusion_amd import _lib
    lib = _lib.load()
    assert _lib.ELEM_BF16 == BF == 0x100
    for N, C in ((544, 3072), (3, 8), (129, 1168)):
        for cid in (1, 2):
            if not lib.cfx_packet_bytes(cid, N, C, 0):
                continue
            assert lib.cfx_packet_bytes(cid | BF, N, C, 0) == lib.cfx_packet_bytes(cid, N, C, 0) != 0
            assert lib.cfx_workspace_bytes(cid | BF, N, C, 0, 2) == lib.cfx_workspace_bytes(cid, N, C, 0, 2) != 0
    assert lib.cfx_packet_bytes(0x101, 544, 3072, 0) == 544 * 3072 // 8 + 2 * (544 + 3072)
    assert lib.cfx_packet_bytes(0x102, 544, 3072, 0) == 544 * 3072 // 4 + 2 * (544 + 3072)
    for bad in (0x103, 0x104, 0x105, 0x201, 0x109, 0x100, 0x1101):
        assert lib.cfx_packet_bytes(bad, 544, 3072, 8 if bad == 0x105 else 0) == 0, hex(bad)
        assert lib.cfx_workspace_bytes(bad, 544, 3072, 0, 2) == 0, hex(bad)
    assert lib.cfx_abi_version() == 2


def test_abi_argument_errors_with_the_element_bit_come_in_todays_order():
    from compactfusion_amd import _lib
    lib = _lib.load()
    ctx = lib.cfx_create(0)
    assert ctx
    for cid in (0x101, 0x102):
        items = (_lib.CompItem * 1)()
        assert lib.cfx_compress_batch(ctx, cid, 8, 64, 0, 0, 1, items, None, 0, None) == -1          # null x
        assert lib.cfx_compress_batch(ctx, cid, 8, 20, 0, 0, 1, items, None, 0, None) == -2          # bad shape
        assert lib.cfx_compress_batch(ctx, cid, 8, 64, 0, 0, 0, items, None, 0, None) == -5          # bad batch
        items[0] = _lib.CompItem(0x1002, None, None, 0x2000)
        assert lib.cfx_compress_batch(ctx, cid, 8, 64, 0, 0, 1, items, None, 0, None) == -3          # misaligned x
        items[0] = _lib.CompItem(0x1000, None, None, 0x2000)
        assert lib.cfx_compress_batch(ctx, cid, 8, 64, 0, 0, 1, items, None, 0, None) == -7          # workspace missing
        d = (_lib.DecompItem * 1)()
        assert lib.cfx_decompress_batch(ctx, cid, 8, 64, 0, 1, d, None) == -1
        assert lib.cfx_decompress_batch(ctx, cid, 8, 20, 0, 1, d, None) == -2
        d[0] = _lib.DecompItem(0x2000, 0x1002, 0x3000)
        assert lib.cfx_decompress_batch(ctx, cid, 8, 64, 0, 1, d, None) == -3
    items = (_lib.CompItem * 1)()
    d = (_lib.DecompItem * 1)()
    for bad in (0x109, 0x103, 0x104, 0x105, 0x201):
        assert lib.cfx_compress_batch(ctx, bad, 8, 64, 0, 0, 1, items, None, 0, None) == -4, hex(bad)
        assert lib.cfx_decompress_batch(ctx, bad, 8, 64, 0, 1, d, None) == -4, hex(bad)
    # plans: the bit is kept with the op; a codec without a bf16 form is refused when the op is added
    plan = lib.cfx_plan_create(ctx)
    c = (_lib.CompItem * 2)(_lib.CompItem(0x1000, 0x2000, 0x2000, 0x3000), _lib.CompItem(0x4000, 0x5000, 0x5000, 0x6000))
    dd = (_lib.DecompItem * 14)(*[_lib.DecompItem(0x7000, 0x8000, 0x8000)] * 14)
    assert lib.cfx_plan_add_compress(plan, 0x101, 544, 3072, 0, 1, 2, c, 0x9000, 1 << 22) == 0
    assert lib.cfx_plan_add_decompress(plan, 0x102, 544, 3072, 0, 14, dd) == 1
    assert lib.cfx_plan_add_compress(plan, 0x103, 544, 3072, 0, 1, 2, c, 0x9000, 1 << 22) == -4
    assert lib.cfx_plan_add_decompress(plan, 0x201, 544, 3072, 0, 14, dd) == -4
    assert lib.cfx_plan_add_compress(plan, 0x101, 544, 3077, 0, 1, 2, c, 0x9000, 1 << 22) == -2
    assert lib.cfx_plan_add_exchange_layer(plan, 0x104, 544, 3072, 0, 1, 2, c, 14, dd, None, None, None, 0, 0x9000, 1 << 22) == -4
    other = lib.cfx_plan_create(ctx)
    assert lib.cfx_plan_copy_op(other, plan, 0) == 0 and lib.cfx_plan_copy_op(other, plan, 1) == 1
    lib.cfx_plan_destroy(other)
    lib.cfx_plan_destroy(plan)
    lib.cfx_destroy(ctx)


# ---- the host state machine against the contract -------------------------------------------------------------------------------------
MODES = [("res1_ef", dict(residual=1, ef=True, fastpath=True, comp_rank=-1)), ("res1_noef", dict(residual=1, ef=False, comp_rank=-1)),
         ("res0", dict(residual=0, ef=False, comp_rank=-1))]


@pytest.mark.parametrize("tname,name", [("BINARY", "binary"), ("INT2", "int2")])
@pytest.mark.parametrize("mode,kw", MODES, ids=[m[0] for m in MODES])
def test_state_machine_equals_the_contract(cpu_kernels, mode, kw, tname, name):
    """Warm-up, then 6 compressed steps: packets, the sender's state and the receiver's state follow the contract bit for bit; with error
    feedback both states are the same bits."""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    N, C = 64, 1024
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, **kw))
    res, ef = kw["residual"], kw["ef"]
    skey, rkey = "0-0-k", "0-1-k"
    s_state = r_state = None
    for t, x in enumerate(_drift(11, N, C, 7)):
        x4 = x.view(1, N, 8, C // 8)
        xb = bits(x).reshape(N, C)
        warm = res == 1 and t == 0
        typ = T.WARMUP if warm else T[tname]
        pkt = cm.compact_compress(skey, x4, typ, update_cache=True)
        if warm:
            assert pkt.dtype == torch.bfloat16 and np.array_equal(bits(pkt).reshape(N, C), xb)
            rec = cm.compact_decompress(rkey, pkt.clone(), typ, x4.shape, update_cache=True)
            assert rec.dtype == torch.bfloat16 and np.array_equal(bits(rec).reshape(N, C), xb)
            s_state, r_state = xb.copy(), xb.copy()
            continue
        want_pkt, nb = BC.compress(name, xb, s_state if res else None, 0, ef)
        assert pkt.dtype == torch.float16 and np.array_equal(bits(pkt).reshape(-1), want_pkt), f"{mode} step {t}: packet"
        want_rec = BC.decompress(name, want_pkt, r_state if res else None, N, C)
        if res == 0:
            # no state says what the sender's activations were: the public call returns fp16 (= the plain fp16 reconstruction), the
            # gather / forward entry points pass the activation type down
            pub = cm.compact_decompress(rkey, pkt.clone(), typ, x4.shape, update_cache=True)
            assert pub.dtype == torch.float16 and np.array_equal(bits(pub).reshape(-1), R.bits(R.decompress(name, want_pkt, N, C)).reshape(-1))
            rec = cm._decompress(rkey, pkt.clone(), typ, x4.shape, True, torch.bfloat16)
            assert rec.dtype == torch.bfloat16 and rec.shape == x4.shape and np.array_equal(bits(rec).reshape(N, C), want_rec)
            assert cm.compact_cache().get_base(skey) is None and cm.compact_cache().get_base(rkey) is None
            continue
        rec = cm.compact_decompress(rkey, pkt.clone(), typ, x4.shape, update_cache=True)
        assert rec.dtype == torch.bfloat16 and rec.shape == x4.shape
        assert np.array_equal(bits(rec).reshape(N, C), want_rec), f"{mode} step {t}: reconstruction"
        s_state, r_state = nb, want_rec
        assert cm.compact_cache().get_base(skey).dtype == torch.bfloat16 and cm.compact_cache().get_base(rkey).dtype == torch.bfloat16
        assert np.array_equal(bits(cm.compact_cache().get_base(skey)).reshape(N, C), s_state), f"{mode} step {t}: sender state"
        assert np.array_equal(bits(cm.compact_cache().get_base(rkey)).reshape(N, C), r_state), f"{mode} step {t}: receiver state"
        if ef:
            assert np.array_equal(s_state, r_state), f"{mode} step {t}: sender and receiver states differ"
        else:
            assert np.array_equal(s_state, xb)


def _refusals():
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T
    return [
        ("int4", dict(residual=1, ef=True), T.INT4, False),
        ("int8", dict(residual=1, ef=True), T.INT8, False),
        ("sparse", dict(residual=1, ef=True, sparse_ratio=8), T.SPARSE, False),
        ("low_rank", dict(residual=1, ef=True, comp_rank=8), T.LOW_RANK, False),
        ("low_rank_q", dict(residual=1, ef=True, comp_rank=32), T.LOW_RANK_Q, False),
        ("binary_rank4", dict(residual=1, ef=True, comp_rank=4), T.BINARY, False),
        ("simulate_binary", dict(residual=1, ef=True, simulate=True, comp_rank=-1), T.BINARY, False),
        ("simulate_int2_res0", dict(residual=0, ef=False, simulate=True, comp_rank=-1), T.INT2, False),
        ("residual2", dict(residual=2, ef=True, comp_rank=-1, delta_decay_factor=0.5), T.BINARY, False),
        ("quantized_cache", dict(residual=1, ef=True, comp_rank=-1, quantized_cache=True), T.BINARY, True),
    ]


@pytest.mark.parametrize("case", range(10))
def test_refused_combinations_raise_before_any_state_changes(cpu_kernels, monkeypatch, case):
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig, utils as U
    label, kw, typ, deprecated = _refusals()[case]
    if deprecated:
        monkeypatch.setattr(U, "ALLOW_DEPRECATED", True)
    N, C = 64, 1024
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, **kw))
    cache = cm.compact_cache()
    x16 = W.drift(5, (N, C), 1)[0]
    if kw["residual"] and not deprecated and kw["residual"] != 2:
        # an fp16 state that must stay exactly as it is
        cm.compact_compress("0-0-k", x16, T.WARMUP, update_cache=True)
        cm.compact_decompress("0-1-k", x16.clone(), T.WARMUP, (N, C), update_cache=True)
    before = {k: (v.dtype, bits(v).copy()) for k, v in cache.base.items()}
    version = cache.version
    x = x16.bfloat16()
    pkt16 = torch.zeros(8, dtype=torch.float16)

    def untouched():
        assert cache.version == version and set(cache.base) == set(before), label
        for k, (dt, b) in before.items():
            assert cache.base[k].dtype == dt and np.array_equal(bits(cache.base[k]), b), (label, k)
    with pytest.raises(NotImplementedError, match="bfloat16") as e:
        cm.compact_compress("0-0-k", x, typ, update_cache=True)
    assert "not supported with" in str(e.value), label
    untouched()
    with pytest.raises(NotImplementedError, match="bfloat16"):
        cm._decompress("0-1-k", pkt16, typ, (N, C), True, torch.bfloat16)
    untouched()
    if label == "quantized_cache" or kw["residual"] == 2:
        with pytest.raises(NotImplementedError, match="bfloat16"):
            cm.compact_compress("0-0-k", x, T.WARMUP, update_cache=True)       # (not even the warm-up step: no bf16 state is ever stored)
        untouched()
    # never a silent cast: the same calls in fp16 are not refused by the bf16 rule
    assert cm._check_bf16(torch.float16, typ) is None


def test_mixed_element_types_raise_value_error(cpu_kernels):
    from compactfusion_amd import codecs
    from compactfusion_amd.compact import fastpath
    N, C = 16, 256
    x = torch.zeros(N, C, dtype=torch.bfloat16)
    b = torch.zeros(N, C, dtype=torch.float16)
    pkt = torch.zeros(codecs.packet_halves(1, N, C), dtype=torch.float16)
    with pytest.raises(ValueError, match="mixed element types"):
        codecs.compress_batch(1, [x], [b], [None], [pkt], N, C)
    with pytest.raises(ValueError, match="mixed element types"):
        codecs.decompress_batch(1, [pkt], [b], [x], N, C)
    with pytest.raises(ValueError, match="mixed element types"):
        codecs.elem_dtype(x, None, b)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        codecs.elem_dtype(x.float())
    assert codecs.elem_dtype(None, None) == torch.float16 and codecs.elem_dtype(x, None, x) == torch.bfloat16
    assert codecs.codec_arg(2, torch.bfloat16) == 0x102 and codecs.codec_arg(2, torch.float16) == 2
    with pytest.raises(ValueError, match="mixed element types"):
        fastpath.binary_quant_fastpath(x, b, -1, True)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        fastpath.binary_quant_fastpath(x, x, 4, True)


# ---- gloo, world size 2 --------------------------------------------------------------------------------------------------------------
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _entry(rank, fn_name, world, port, out, args):
    W.run(getattr(BW, fn_name), rank, world, port, out, *args)


def _spawn(fn, world, tmp_path, *args):
    out = str(tmp_path / "res")
    for attempt in range(3):
        try:
            mp.start_processes(_entry, args=(fn.__name__, world, _port(), out, args), nprocs=world, join=True, start_method="spawn")
            break
        except Exception as e:  # noqa: BLE001  (the free port was taken again before rank 0 bound it)
            if "EADDRINUSE" not in str(e) or attempt == 2:
                raise
    return [dict(np.load(out + f".r{r}.npz")) for r in range(world)]


@pytest.mark.parametrize("codec,name,ef", [("BINARY", "binary", True), ("INT2", "int2", True), ("BINARY", "binary", False)])
def test_compact_all_gather_2rank_bf16(tmp_path, codec, name, ef):
    res = _spawn(BW.w_all_gather_bf16, 2, tmp_path, codec, ef)
    N, C = 32, 256
    state = [None, None]
    for t in range(5):
        for i in range(2):
            assert np.array_equal(res[0][f"t{t}/out{i}"], res[1][f"t{t}/out{i}"]), (t, i)          # every rank: the same bf16 states
            assert np.array_equal(res[0][f"t{t}/state{i}"], res[1][f"t{t}/state{i}"]), (t, i)
            x = res[i][f"t{t}/x"].reshape(N, C)
            if t == 0:
                state[i] = x.copy()
            else:
                pkt, _ = BC.compress(name, x, state[i], 0, ef)
                state[i] = BC.decompress(name, pkt, state[i], N, C)
            assert np.array_equal(res[0][f"t{t}/out{i}"], state[i]), (t, i)                       # ... and the contract's
            assert np.array_equal(res[1 - i][f"t{t}/state{i}"], state[i]), (t, i)


@pytest.mark.parametrize("codec,name", [("BINARY", "binary"), ("INT2", "int2")])
def test_compact_all_gather_kv_2rank_bf16(tmp_path, codec, name):
    res = _spawn(BW.w_all_gather_kv_bf16, 2, tmp_path, codec)
    N, C = 32, 256
    state = {}
    for t in range(5):
        for i in range(2):
            for kv in "kv":
                assert np.array_equal(res[0][f"t{t}/{kv}{i}"], res[1][f"t{t}/{kv}{i}"]), (t, i, kv)
                x = res[i][f"t{t}/x{kv}"].reshape(N, C)
                if t == 0:
                    state[i, kv] = x.copy()
                else:
                    pkt, _ = BC.compress(name, x, state[i, kv], 0, True)
                    state[i, kv] = BC.decompress(name, pkt, state[i, kv], N, C)
                assert np.array_equal(res[0][f"t{t}/{kv}{i}"], state[i, kv]), (t, i, kv)


# ---- quality of the contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["binary", "int2"])
def test_bf16_contract_tracks_the_drift_as_well_as_fp16(name):
    """Golden G12's drift (tests/golden/make_golden_quality.py: (128, 3072), 28 steps, x_t = fp16(x_{t-1} + 0.1 N(0, 1))), one warm-up step,
    residual 1 with error feedback.  The inputs x_t are exact fp16 values: the fp16 oracle runs on them as they are, the bf16 contract on
    bf16(x_t).  At every step
        || state_bf16 - x_t || / || x_t ||   <=   || state_fp16 - x_t || / || x_t ||   +   || bf16(x_t) - x_t || / || x_t ||
    - the right side is computed from the inputs and the pinned oracle alone: what the fp16 path loses on the same drift, plus what the
    rounding of that step's input to bf16 loses before the codec sees it (a relative 0.0017)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_quality", os.path.join(REPO, "tests", "golden", "make_golden_quality.py"))
    mq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mq)
    N, C = mq.N, mq.C
    assert (N, C) == (128, 3072)
    xs = mq.drift(mq.SEED_X, 28)
    s16 = sbf = None
    worst = 0.0
    for t, x in enumerate(xs):
        x32 = x.float().numpy()
        xbf = bits(x.bfloat16()).reshape(N, C)
        if t == 0:
            s16, sbf = R.bits(x.numpy()).reshape(N, C).copy(), xbf.copy()
        else:
            _, s16n = R.residual_compress(name, s16 * 0 + R.bits(x.numpy()).reshape(N, C), s16, 0, True)
            s16 = R.bits(s16n).reshape(N, C).copy()
            _, sbf = BC.compress(name, xbf, sbf, 0, True)
        nx = np.linalg.norm(x32)
        e16 = np.linalg.norm(s16.view(np.float16).astype(np.float32) - x32) / nx
        ebf = np.linalg.norm(BC.bf16_to_f32(sbf) - x32) / nx
        allow = np.linalg.norm(BC.bf16_to_f32(xbf) - x32) / nx
        print(f"{name} step {t:2d}: bf16 {ebf:.5f}  fp16 {e16:.5f}  input rounding {allow:.5f}")
        assert 0.0010 < allow < 0.0020
        assert ebf <= e16 + allow, (name, t, ebf, e16, allow)
        worst = max(worst, ebf - e16)
    print(f"{name}: bf16 error exceeds fp16 error by at most {worst:.5f}")


# ---- the compiled kernels ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_usage
    return resource_usage.collect()


def test_bf16_kernels_exist_without_scratch(rows):
    for want in ("k_absmean_compress<", "k_int2_compress_gated<", "k_binary_dequant<", "k_int2_dequant<", "k_int2_quant<", "k_absmean_stats<"):
        ks = [k for k in rows if k["demangled"].startswith(want) and k["demangled"].endswith("ElemBF16>")]
        assert ks, want
        for k in ks:
            assert k.get("scratch", 0) == 0, k
    # every form the fp16 path dispatches has its bf16 twin
    f16 = sorted(k["demangled"].replace("ElemF16", "ElemBF16") for k in rows if "ElemF16" in k["demangled"])
    b16 = sorted(k["demangled"] for k in rows if "ElemBF16" in k["demangled"])
    assert f16 == b16 and len(b16) >= 12


def test_bf16_layer_forms_keep_two_workgroups_a_cu_and_room_for_a_collective(rows):
    layer = [k for k in rows if "ElemBF16" in k["demangled"] and any(n in k["demangled"] for n in ("k_absmean_compress", "k_int2_compress_gated"))]
    assert len(layer) >= 6
    for k in layer:
        assert k["vgpr"] + k.get("agpr", 0) <= 128 and k["lds"] <= 80 * 1024, k
    one = [k for k in rows if k["demangled"].startswith("k_absmean_compress<true, 4, true") and k["demangled"].endswith("ElemBF16>")]
    assert one
    for k in one:
        assert k["vgpr"] + k.get("agpr", 0) <= 104, k       # as the fp16 form: 512 - 2 x 104 registers a SIMD stay free for a collective kernel


def test_every_kernel_of_the_parent_commit_compiles_to_the_same_resources(rows):
    """tests/golden/resource_rows_parent.json: the rows of every kernel at the commit before bf16 (same collector).  The element type is a
    trailing template argument; the fp16 instantiation of a kernel is the parent's kernel of the same name without it.  The min/max
    family's kernels have since become templates on RPC, the rows per code row (1 int8, 2 int4): the layer kernel kept its body and is held
    to the parent's row under its new name; the four stand-alone kernels were rewritten as two templates and are held to no more
    registers than the parent's, the same LDS and no scratch (their SGPR counts moved; 41 at most, far from bounding their occupancy)."""
    parent = json.load(open(os.path.join(REPO, "tests", "golden", "resource_rows_parent.json")))
    assert len(parent) >= 90
    minmax = {"k_minmax_layer<1, 4>": "k_minmax_layer<false, 4>", "k_minmax_layer<1, 8>": "k_minmax_layer<false, 8>",
              "k_minmax_layer<2, 4>": "k_minmax_layer<true, 4>", "k_minmax_layer<2, 8>": "k_minmax_layer<true, 8>",
              "k_minmax_quant<1>": "k_int8_quant", "k_minmax_quant<2>": "k_int4_quant",
              "k_minmax_dequant<1>": "k_int8_dequant", "k_minmax_dequant<2>": "k_int4_dequant"}
    rewritten = {"k_int8_quant", "k_int4_quant", "k_int8_dequant", "k_int4_dequant"}

    def parent_name(n):
        return minmax.get(n, n).replace(", ElemF16>", ">").replace("<ElemF16>", "")
    cur = {}
    for k in rows:
        if "ElemBF16" not in k["demangled"]:
            assert (k["file"], parent_name(k["demangled"])) not in cur, k
            cur[k["file"], parent_name(k["demangled"])] = k
    for p in parent:
        k = cur.get((p["file"], p["demangled"]))
        assert k is not None, ("kernel of the parent commit is gone", p)
        if p["demangled"] in rewritten:
            assert k["vgpr"] + k.get("agpr", 0) <= p["vgpr"] + p["agpr"] and k.get("lds", 0) == p["lds"] and k.get("scratch", 0) == 0, (p, k)
            continue
        got = {f: k.get(f, 0) for f in ("vgpr", "agpr", "sgpr", "lds", "scratch")}
        assert got == {f: p[f] for f in got}, (p, got)
    assert any(p["sgpr"] for p in parent)
