"""Second-order residuals (CompactConfig(residual=2)) through the PRODUCT path of the gather schedules on the GPU (-m gpu): `compact_fwd`
(ring gather schedule) and `compact_all_gather_kv` (what `patch_gather_fwd` calls) hand a BINARY / INT2 layer to ONE native op per layer
(compact/xlayer.py with second-order states, cfx_plan_set_second_order) instead of one Python call per tensor: no cfx_residual2_delta /
_update launch (kernel ids 25 / 26), one reconstruction launch per layer, every rank's base AND delta_base of every key equal to the
oracle's replay bit for bit.  8 logical ranks looped back in one process (the arrangement of tests/test_gpu_plugin_path.py, re-stated
here), and two rank processes on one GPU over two generations."""
import ctypes

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _dist_workers as W
import res2_workers as RW
from oracle import ref_np as R
from test_gpu_schedules import ONAME, _port

pytestmark = pytest.mark.gpu
WL = 8
DECAY = 0.5


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


@pytest.fixture
def loop8(monkeypatch):
    """An 8-rank group whose peers are all this rank; torch.distributed is not initialised."""
    from compactfusion_amd.compact import ring, main as cm, xlayer
    from compactfusion_amd.collector import collector
    from compactfusion_amd.prof import Profiler
    monkeypatch.setenv("CFX_RING_SCHEDULE", "gather")
    monkeypatch.setenv("CFX_LANE", "off")
    monkeypatch.delenv("CFX_RING_EXCHANGE_STREAM", raising=False)
    monkeypatch.delenv("CFX_RING_EXCHANGE", raising=False)
    monkeypatch.setattr(ring.dist, "get_rank", lambda g=None: 0)
    monkeypatch.setattr(ring.dist, "get_world_size", lambda g=None: WL)
    monkeypatch.setattr(ring.dist, "all_gather_into_tensor",            # WARMUP steps gather raw fp16 through torch.distributed
                        lambda recv, send, group=None: recv.view(WL, -1).copy_(send.view(1, -1).expand(WL, -1)))
    xlayer.set_p2p_loopback(True)
    Profiler.instance().disable()
    collector.init(collector.Collector("/tmp/none", enabled=False))
    ring._xbuf.clear()
    ring._steady.clear()
    yield ring, cm, xlayer
    cm._drop_kv_exchanges()
    for e in ring._xbuf.values():
        e.close()
    ring._xbuf.clear()
    ring._steady.clear()
    xlayer.set_p2p_loopback(False)


def replay(codec, seq, N, C, warm=2, decay=DECAY):
    """(base bits, delta_base bits | None) after every step of WARMUP x warm, codec, codec, ... (R.OracleCompact, residual 2)"""
    name, param = ONAME[codec]
    orc = R.OracleCompact(residual=2, ef=True, param=param, decay=decay)
    out = []
    for t, x in enumerate(seq):
        orc.compress("k", x.numpy().reshape(N, C), "warmup" if t < warm else name, True)
        d = orc.dbase["k"]
        out.append((R.bits(orc.base["k"]).copy(), None if d is None else R.bits(d).copy()))
    return out


def _kernel_ids(lib, ctx):
    ids = (ctypes.c_int * 8192)()
    ms = (ctypes.c_float * 8192)()
    n = lib.cfx_profile_read(ctx, ids, ms, 8192)
    return [ids[i] for i in range(n)]


@pytest.mark.parametrize("codec", ["BINARY", "INT2", "INT4"])
@pytest.mark.parametrize("api", ["ring", "gather"])
def test_plugin_call_residual2_one_native_op(loop8, api, codec):
    ring, cm, xlayer = loop8
    from compactfusion_amd import _lib, codecs as K
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig, PatchConfig
    lib, ctx = _lib.load(), K.context(0)
    L, STEPS = 3, 6
    shape, N, C = (1, 64, 8, 64), 64, 512
    kw = dict(enabled=True, compress_func=lambda l, s: T.WARMUP if s < 2 else T[codec], comp_rank=-1, residual=2, ef=True, fastpath=False,
              delta_decay_factor=DECAY)
    if api == "gather":
        kw.update(override_with_patch_gather_fwd=True, patch_gather_fwd_config=PatchConfig(True, False, 1))
    cm.compact_init(CompactConfig(**kw))
    qs = [W.drift(7 + l, shape, STEPS) for l in range(L)]
    ks = [W.drift(17 + l, shape, STEPS) for l in range(L)]
    vs = [W.drift(27 + l, shape, STEPS) for l in range(L)]
    want = {(l, n): replay(codec, seq[l], N, C) for l in range(L) for n, seq in (("k", ks), ("v", vs))}
    dev = torch.device("cuda:0")
    fused = codec in ("BINARY", "INT2")
    rec_id = {"BINARY": 4, "INT2": 6, "INT4": 12}[codec]
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        for s in range(STEPS):
            cm.compact_set_step(s)
            torch.cuda.synchronize()
            assert lib.cfx_profile_enable(ctx, 8192, 0xffffffff, 1) == 0
            for l in range(L):
                ring.compact_fwd(qs[l][s].to(dev), ks[l][s].to(dev), vs[l][s].to(dev), causal=False, mod_idx=l, current_iter=s)
            torch.cuda.synchronize()
            got = _kernel_ids(lib, ctx)
            lib.cfx_profile_enable(ctx, 0, 0, 1)
            if s >= 3 and fused:
                assert got.count(25) == 0 and got.count(26) == 0 and got.count(31) == 0, (api, codec, s, got)
                assert got.count(rec_id) == L, (api, codec, s, got)              # ONE reconstruction launch per layer
            if s >= 3 and not fused:
                assert got.count(25) > 0 and got.count(26) > 0, (api, codec, s, got)    # the composition is untouched
            cache = cm.compact_cache()
            for l in range(L):
                for n in ("k", "v"):
                    wb, wd = want[(l, n)][s]
                    for r in range(WL):
                        key = f"{l}-{r}-{n}" if api == "ring" else f"{l}-{n}-{r}"
                        assert np.array_equal(bits(cache.get_base(key)).reshape(N, C), wb.reshape(N, C)), (api, codec, s, l, n, r, "base")
                        if wd is not None:
                            assert np.array_equal(bits(cache.get_delta_base(key)).reshape(N, C), wd.reshape(N, C)), (api, codec, s, l, n, r, "delta_base")
    ops = [e.xop for e in ring._xbuf.values() if e.xop is not None] + [e.xop for e in cm._kv_exchanges.values() if e.xop is not None]
    if fused:
        assert len(ops) == L and all(o.transport == "p2p" and o.own2 is not None for o in ops), "the layer op / the IPC arena was not used"
    else:
        assert not ops
    assert lib.cfx_gate_errors(ctx) == 0


def _entry(rank, fn_name, world, port, out, args):
    W.run(getattr(RW, fn_name), rank, world, port, out, *args, device="cuda")


def _spawn(fn, world, tmp_path, *args):
    """test_gpu_schedules._spawn for a worker of tests/res2_workers.py"""
    out = str(tmp_path / "res")
    for attempt in range(3):
        try:
            mp.start_processes(_entry, args=(fn.__name__, world, _port(), out, args), nprocs=world, join=True, start_method="spawn")
            break
        except Exception as e:  # noqa: BLE001
            if "EADDRINUSE" not in str(e) or attempt == 2:
                raise
    return [dict(np.load(out + f".r{r}.npz")) for r in range(world)]


def test_two_processes_two_generations_residual2(tmp_path):
    """Two rank processes on one GPU, ring mode, BINARY, residual 2, packets read in place through IPC mappings; compact_reset between
    two generations.  Both states bit-equal across the ranks and to the oracle; the peer-to-peer layer op was taken and validated."""
    L, STEPS, shape, N, C = RW.L, RW.STEPS, RW.SHAPE, 64, 512
    res = _spawn(RW.w_res2_ring, 2, tmp_path, "BINARY", 2)
    for r in range(2):
        assert int(res[r]["n_ops"][0]) == L and int(res[r]["p2p"][0]) == L and int(res[r]["second"][0]) == L and int(res[r]["fell_back"][0]) == 0
        assert int(res[r]["validated"][0]) == min(4, STEPS - 2) and int(res[r]["gate_errors"][0]) == 0
    for gen in range(2):
        for l in range(L):
            want = {("k", q): replay("BINARY", W.drift(1000 * gen + 17 + 10 * l + q, shape, STEPS), N, C) for q in range(2)}
            want.update({("v", q): replay("BINARY", W.drift(1000 * gen + 27 + 10 * l + q, shape, STEPS), N, C) for q in range(2)})
            for s in range(STEPS):
                for q in range(2):
                    for n in ("k", "v"):
                        wb, wd = want[(n, q)][s]
                        for r in range(2):
                            assert np.array_equal(res[r][f"g{gen}/s{s}/l{l}/{n}{q}"].reshape(-1), wb.reshape(-1)), (gen, l, s, q, n, r, "base")
                            if wd is not None:
                                assert np.array_equal(res[r][f"g{gen}/s{s}/l{l}/d{n}{q}"].reshape(-1), wd.reshape(-1)), (gen, l, s, q, n, r, "delta_base")
