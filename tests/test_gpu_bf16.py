"""bf16 activations in the 1-bit and 2-bit exchange on the GPU (-m gpu): every result bit-exact against the contract
(tests/bf16_contract.py: d = fp16(fp32(x) - fp32(base)); the fp16 path between d and recv; state = bf16(fp32(base) + fp32(recv))),
packets compared as whole byte strings.  These tests fail on a library without CFX_ELEM_BF16 (sizes 0, ValueError)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _domain_cases as D
import bf16_contract as BC
from oracle import ref_np as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BF = BC.ELEM_BF16
NAME = {1: "binary", 2: "int2"}
UPD, NO_EF = 1, 2
bits = BC.torch_bits


@pytest.fixture(autouse=True)
def _collector(tmp_path):
    from compactfusion_amd.collector import collector
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    yield


def _lib_ctx():
    from compactfusion_amd import _lib, codecs as K
    return _lib, _lib.load(), K.context(0)


def bf_bits(rng, N, C, scale=0.5, near=None):
    """bf16 bit patterns (N, C) of a random tensor (near: a drift step away from that tensor)"""
    a = rng.standard_normal((N, C)).astype(np.float32) * scale
    if near is not None:
        a = BC.bf16_to_f32(near) + 0.2 * a
    return bits(torch.from_numpy(a).bfloat16()).reshape(N, C).copy()


def dev(u16, dtype=torch.bfloat16):
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16).copy()).view(dtype).cuda()


def pkt_bytes(t, n):
    return t.cpu().numpy().view(np.uint8).reshape(-1)[:n]


# ---- stand-alone compress / decompress through the C-ABI -----------------------------------------------------------------------------
SHAPES = [(N, C) for N, C, _ in D.SHAPES] + [(544, 3072)]
STAND_ALONE = [(cid, N, C) for cid in (1, 2) for N, C in SHAPES if D.legal(NAME[cid], N, C)]       # every shape the codec accepts


@pytest.mark.parametrize("cid,N,C", STAND_ALONE, ids=[f"{NAME[c]}-{n}x{k}" for c, n, k in STAND_ALONE])
def test_stand_alone_calls_equal_the_contract(cid, N, C):
    name = NAME[cid]
    _lib, lib, ctx = _lib_ctx()
    rng = np.random.default_rng(1000 * cid + N + C)
    nb_ = lib.cfx_packet_bytes(cid | BF, N, C, 0)
    assert nb_ == lib.cfx_packet_bytes(cid, N, C, 0) != 0
    slot = (nb_ + 255) // 256 * 256
    bb = [bf_bits(rng, N, C) for _ in range(2)]
    xb = [bf_bits(rng, N, C, near=b) for b in bb]
    with_base = [BC.compress(name, xb[i], bb[i]) for i in range(2)]            # (packet, new_base)
    no_base = [BC.compress(name, xb[i], None) for i in range(2)]
    rec_base = [BC.decompress(name, with_base[i][0], bb[i], N, C) for i in range(2)]
    rec_none = [BC.decompress(name, no_base[i][0], None, N, C) for i in range(2)]
    for i in range(2):
        assert np.array_equal(rec_base[i], with_base[i][1])                    # (the sender's update IS the receiver's reconstruction)
    for batch in (1, D.MAX_BATCH):
        wsb = lib.cfx_workspace_bytes(cid | BF, N, C, 0, batch)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
        x = [dev(xb[i % 2]) for i in range(batch)]

        def compress(flags, base, new_base):
            pk = torch.zeros(batch, slot, dtype=torch.uint8, device="cuda")
            items = (_lib.CompItem * batch)(*[_lib.CompItem(x[i].data_ptr(), None if base is None else base[i].data_ptr(),
                                                            None if new_base is None else new_base[i].data_ptr(), pk[i].data_ptr()) for i in range(batch)])
            rc = lib.cfx_compress_batch(ctx, cid | BF, N, C, 0, flags, batch, items, ws.data_ptr(), wsb, None)
            assert rc == 0, lib.cfx_last_error_string(ctx)
            torch.cuda.synchronize()
            return pk

        def decompress(pk, base, recon):
            items = (_lib.DecompItem * batch)(*[_lib.DecompItem(pk[i].data_ptr(), None if base is None else base[i].data_ptr(), recon[i].data_ptr())
                                                for i in range(batch)])
            rc = lib.cfx_decompress_batch(ctx, cid | BF, N, C, 0, batch, items, None)
            assert rc == 0, lib.cfx_last_error_string(ctx)
            torch.cuda.synchronize()
        tag = f"{name} ({N}, {C}) batch {batch}"
        # base given, new_base a tensor of its own
        base = [dev(bb[i % 2]) for i in range(batch)]
        nb = [torch.zeros(N, C, dtype=torch.bfloat16, device="cuda") for _ in range(batch)]
        pk = compress(UPD, base, nb)
        for i in range(batch):
            assert pkt_bytes(pk[i], nb_).tobytes() == with_base[i % 2][0].view(np.uint8).tobytes(), f"{tag}: packet {i}"
            assert np.array_equal(bits(nb[i]), with_base[i % 2][1]), f"{tag}: new_base {i}"
            assert np.array_equal(bits(base[i]), bb[i % 2]), f"{tag}: base {i} was written"
        # reconstruction: recon a tensor of its own, then aliasing base
        rec = [torch.zeros(N, C, dtype=torch.bfloat16, device="cuda") for _ in range(batch)]
        decompress(pk, base, rec)
        for i in range(batch):
            assert np.array_equal(bits(rec[i]), rec_base[i % 2]), f"{tag}: recon {i}"
        decompress(pk, base, base)
        for i in range(batch):
            assert np.array_equal(bits(base[i]), rec_base[i % 2]), f"{tag}: recon aliasing base {i}"
        # new_base aliasing base
        base = [dev(bb[i % 2]) for i in range(batch)]
        pk = compress(UPD, base, base)
        for i in range(batch):
            assert pkt_bytes(pk[i], nb_).tobytes() == with_base[i % 2][0].view(np.uint8).tobytes(), f"{tag}: packet {i} (in place)"
            assert np.array_equal(bits(base[i]), with_base[i % 2][1]), f"{tag}: new_base aliasing base {i}"
        # error feedback off: the state is the activation, bit for bit
        base = [dev(bb[i % 2]) for i in range(batch)]
        nb = [torch.zeros(N, C, dtype=torch.bfloat16, device="cuda") for _ in range(batch)]
        pk = compress(UPD | NO_EF, base, nb)
        for i in range(batch):
            assert pkt_bytes(pk[i], nb_).tobytes() == with_base[i % 2][0].view(np.uint8).tobytes(), f"{tag}: packet {i} (no EF)"
            assert np.array_equal(bits(nb[i]), xb[i % 2]), f"{tag}: CFX_FLAG_NO_EF new_base {i}"
        # base NULL
        nb = [torch.zeros(N, C, dtype=torch.bfloat16, device="cuda") for _ in range(batch)]
        pk = compress(UPD, None, nb)
        for i in range(batch):
            assert pkt_bytes(pk[i], nb_).tobytes() == no_base[i % 2][0].view(np.uint8).tobytes(), f"{tag}: packet {i} (no base)"
            assert np.array_equal(bits(nb[i]), no_base[i % 2][1]), f"{tag}: new_base {i} (no base)"
        decompress(pk, None, rec)
        for i in range(batch):
            assert np.array_equal(bits(rec[i]), rec_none[i % 2]), f"{tag}: recon {i} (no base)"
    assert lib.cfx_gate_errors(ctx) == 0


def test_int2_quantize_alone_takes_the_element_flag():
    """cfx_int2_quantize has no codec argument: CFX_FLAG_ELEM_BF16 in `flags`.  With the contract's own scales planted in the packet
    tail the codes and the state are the contract's."""
    _lib, lib, ctx = _lib_ctx()
    N, C = 129, 384
    rng = np.random.default_rng(5)
    bb = bf_bits(rng, N, C)
    xb = bf_bits(rng, N, C, near=bb)
    want_pkt, want_nb = BC.compress("int2", xb, bb)
    nbytes = lib.cfx_packet_bytes(2, N, C, 0)
    pk = torch.from_numpy(want_pkt.view(np.uint8).copy()).cuda()
    pk[:N * C // 4] = 0
    x, base, nb = dev(xb), dev(bb), torch.zeros(N, C, dtype=torch.bfloat16, device="cuda")
    items = (_lib.CompItem * 1)(_lib.CompItem(x.data_ptr(), base.data_ptr(), nb.data_ptr(), pk.data_ptr()))
    assert lib.cfx_int2_quantize(ctx, N, C, UPD | _lib.FLAG_ELEM_BF16, 1, items, None) == 0, lib.cfx_last_error_string(ctx)
    torch.cuda.synchronize()
    assert pkt_bytes(pk, nbytes).tobytes() == want_pkt.view(np.uint8).tobytes()
    assert np.array_equal(bits(nb), want_nb)


# ---- the layer call --------------------------------------------------------------------------------------------------------------------
class Layer:
    """One layer call: B own tensors compressed (error feedback in place), NP looped-back peer states reconstructed from those packets."""

    def __init__(self, cid, N, C, dtype, seed, B=2, NP=14):
        _lib, lib, ctx = _lib_ctx()
        self._lib, self.lib, self.ctx = _lib, lib, ctx
        self.cid, self.N, self.C, self.B, self.NP, self.dtype = cid, N, C, B, NP, dtype
        self.bf = dtype == torch.bfloat16
        self.cabi = cid | (BF if self.bf else 0)
        self.rng = np.random.default_rng(seed)
        self.nbytes = lib.cfx_packet_bytes(self.cabi, N, C, 0)
        assert self.nbytes
        slot = (self.nbytes + 255) // 256 * 256
        first = [self.draw() for _ in range(B)]
        self.want = [f.copy() for f in first]
        self.xin = [dev(f, dtype) for f in first]
        self.own = [dev(f, dtype) for f in first]
        self.peer = [dev(first[g % B], dtype) for g in range(NP)]
        self.pk = torch.zeros(B, slot, dtype=torch.uint8, device="cuda")
        self.wsb = lib.cfx_workspace_bytes(self.cabi, N, C, 0, B)
        self.ws = torch.empty(max(self.wsb, 16), dtype=torch.uint8, device="cuda")
        self.comp = (_lib.CompItem * B)(*[_lib.CompItem(self.xin[i].data_ptr(), self.own[i].data_ptr(), self.own[i].data_ptr(), self.pk[i].data_ptr())
                                          for i in range(B)])
        self.gated = (_lib.DecompItem * NP)(*[_lib.DecompItem(self.pk[g % B].data_ptr(), self.peer[g].data_ptr(), self.peer[g].data_ptr())
                                              for g in range(NP)])
        self.want_pkt = [None] * B

    def draw(self, near=None):
        if self.bf:
            return bf_bits(self.rng, self.N, self.C, near=near)
        a = self.rng.standard_normal((self.N, self.C)).astype(np.float32) * 0.5
        if near is not None:
            a = near.view(np.float16).astype(np.float32) + 0.2 * a
        return a.astype(np.float16).view(np.uint16)

    def advance(self):
        """fresh activations into the static input buffers; the contract's (fp16: the oracle's) packets and states"""
        for i in range(self.B):
            x = self.draw(near=self.want[i])
            self.xin[i].copy_(dev(x, self.dtype))
            if self.bf:
                self.want_pkt[i], self.want[i] = BC.compress(NAME[self.cid], x, self.want[i])
            else:
                p, nb = R.residual_compress(NAME[self.cid], x, self.want[i], 0)
                self.want_pkt[i], self.want[i] = p, R.bits(nb).reshape(self.N, self.C).copy()
        torch.cuda.synchronize()

    def call(self, sh):
        rc = self.lib.cfx_compress_batch_gated(self.ctx, self.cabi, self.N, self.C, 0, UPD, self.B, self.comp, 0, None, self.NP, self.gated,
                                               self.ws.data_ptr(), self.wsb, sh)
        assert rc == 0, self.lib.cfx_last_error_string(self.ctx)

    def check(self, what):
        torch.cuda.synchronize()
        assert self.lib.cfx_gate_errors(self.ctx) == 0, what
        for i in range(self.B):
            assert pkt_bytes(self.pk[i], self.nbytes).tobytes() == self.want_pkt[i].view(np.uint8).tobytes(), f"{what}: packet {i}"
            assert np.array_equal(bits(self.own[i]).reshape(self.N, self.C), self.want[i]), f"{what}: own state {i}"
        for g in range(self.NP):
            assert np.array_equal(bits(self.peer[g]).reshape(self.N, self.C), self.want[g % self.B]), f"{what}: peer state {g}"


def _kernels_of(lib, ctx, fn):
    assert lib.cfx_profile_enable(ctx, 64, 0xffffffff, 1) == 0
    fn()
    torch.cuda.synchronize()
    ids, ms = (ctypes.c_int * 64)(), (ctypes.c_float * 64)()
    n = lib.cfx_profile_read(ctx, ids, ms, 64)
    lib.cfx_profile_enable(ctx, 0, 0, 1)
    return [ids[i] for i in range(n)]


@pytest.mark.parametrize("cid", [1, 2])
@pytest.mark.parametrize("N,C,one", [(544, 3072, True), (544, 576, False)], ids=["544x3072", "544x576-fallback"])
def test_layer_call_equals_compress_then_decompress_and_the_contract(cid, N, C, one):
    """cfx_compress_batch_gated with 2 compress items, 14 gated items and the own error-feedback update: the contract's packets and
    states, the same bits as compress ; cfx_decompress_batch - as ONE kernel for both codecs where the shape qualifies, as the
    documented sequence where it does not (C % 128 != 0) - and under four replays of a captured graph between eager launches."""
    ly = Layer(cid, N, C, torch.bfloat16, 31 + cid)
    lib, ctx, _lib = ly.lib, ly.ctx, ly._lib
    side = torch.cuda.Stream()
    ly.advance()
    start = [bits(t).copy() for t in ly.own] + [bits(t).copy() for t in ly.peer]
    x_now = [bits(t).copy() for t in ly.xin]
    with torch.cuda.stream(side):
        ids = _kernels_of(lib, ctx, lambda: ly.call(side.cuda_stream))
    ly.check("layer call")
    if one:
        # (2-bit: 6 column blocks x 17 row tiles x 2 tensors = 204 workgroups, within the co-residency rule of a full stream)
        assert ids == [31], f"the {cid}-bit bf16 layer call must be one kernel (the gated layer launch), got kernel ids {ids}"
    if not one:
        assert len(ids) >= 2 and 31 not in ids, f"C % 128 != 0 has no one-launch form, got kernel ids {ids}"
    # the same step as compress ; cfx_decompress_batch on copies of the starting states
    own2 = [dev(s.reshape(N, C)) for s in start[:ly.B]]
    peer2 = [dev(s.reshape(N, C)) for s in start[ly.B:]]
    x2 = [dev(x.reshape(N, C)) for x in x_now]
    pk2 = torch.zeros_like(ly.pk)
    c2 = (_lib.CompItem * ly.B)(*[_lib.CompItem(x2[i].data_ptr(), own2[i].data_ptr(), own2[i].data_ptr(), pk2[i].data_ptr()) for i in range(ly.B)])
    d2 = (_lib.DecompItem * ly.NP)(*[_lib.DecompItem(pk2[g % ly.B].data_ptr(), peer2[g].data_ptr(), peer2[g].data_ptr()) for g in range(ly.NP)])
    assert lib.cfx_compress_batch(ctx, ly.cabi, N, C, 0, UPD, ly.B, c2, ly.ws.data_ptr(), ly.wsb, None) == 0
    assert lib.cfx_decompress_batch(ctx, ly.cabi, N, C, 0, ly.NP, d2, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(pk2, ly.pk)
    for a, b in zip(own2 + peer2, ly.own + ly.peer):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    # captured: four replays with fresh activations, eager launches of the same context before and between them
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ly.call(side.cuda_stream)
    torch.cuda.synchronize()
    ly.check("capture must not execute")
    for rep in range(4):
        ly.advance()
        graph.replay()
        ly.check(f"replay {rep}")
        if rep == 1:
            ly.advance()
            with torch.cuda.stream(side):
                ly.call(side.cuda_stream)
            ly.check("eager launch between replays")


@pytest.mark.parametrize("cid", [1, 2])
def test_fp16_and_bf16_layer_calls_alternate_on_one_context_and_stream(cid):
    """One context, one stream: the tag arena, the ticket ring and the gates are shared by launches of both element types."""
    N, C = 544, 3072
    h = Layer(cid, N, C, torch.float16, 7)
    b = Layer(cid, N, C, torch.bfloat16, 8)
    side = torch.cuda.Stream()
    for step in range(3):
        h.advance(); b.advance()
        with torch.cuda.stream(side):
            h.call(side.cuda_stream)
            b.call(side.cuda_stream)            # (back to back: the bf16 launch follows the fp16 one in the stream without a host wait)
        h.check(f"fp16 step {step}")
        b.check(f"bf16 step {step}")
    # a bf16 sender's packet is a valid fp16-path packet: an fp16 receiver reconstructs it with the plain codec id
    _lib, lib, ctx = b._lib, b.lib, b.ctx
    base16 = h.draw()
    st = dev(base16, torch.float16)
    d = (_lib.DecompItem * 1)(_lib.DecompItem(b.pk[0].data_ptr(), st.data_ptr(), st.data_ptr()))
    assert lib.cfx_decompress_batch(ctx, cid, N, C, 0, 1, d, None) == 0
    torch.cuda.synchronize()
    want = R.residual_decompress(NAME[cid], b.want_pkt[0], base16, N, C, 0)
    assert np.array_equal(bits(st).reshape(N, C), R.bits(want).reshape(N, C))


# ---- the peer-to-peer exchange layer op, two rank processes on one GPU ------------------------------------------------------------------
@pytest.mark.parametrize("cid", [1, 2])
def test_p2p_exchange_layer_two_processes_one_gpu(tmp_path, cid):
    """cfx_plan_add_exchange_layer_p2p with CFX_ELEM_BF16: each rank's packets in memory the other has opened, the exchange inside the
    layer launch.  Four steps (both packet parities twice): every rank's reconstruction of the other's shard is that rank's own bf16
    state, and both are the contract's.  Each rank process runs under its own time limit, once."""
    W, N, C, steps = 2, 544, 3072, 4
    env = dict(os.environ)
    env.setdefault("GPU_MAX_HW_QUEUES", "8")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "bf16_p2p_rank.py"), str(r), str(W), str(tmp_path), str(cid), str(N), str(C), str(steps)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=REPO, env=env) for r in range(W)]
    outs, failed = [], False
    for p in procs:
        try:
            o, _ = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            failed = True
            for q in procs:
                q.kill()
            o, _ = p.communicate()
        outs.append(o)
    assert not failed and all(p.returncode == 0 for p in procs), "\n".join(o[-2000:] for o in outs)
    name = NAME[cid]
    for r in range(W):
        own = np.load(tmp_path / f"own{r}.npy")
        x0 = np.load(tmp_path / f"x0_{r}.npy")
        assert not np.array_equal(own, x0)
        got = np.load(tmp_path / f"peer{1 - r}_{r}.npy")
        assert np.array_equal(got, own), f"rank {1 - r}: reconstruction of rank {r}'s shard differs from rank {r}'s own state"
        xs = [np.load(tmp_path / f"xs{s}_{r}.npy") for s in range(2)]
        st = x0.copy()
        for l in range(st.shape[0]):
            for b in range(2):
                s_ = st[l, b].reshape(N, C)
                for i in range(steps):
                    _, s_ = BC.compress(name, xs[i & 1][l, b].reshape(N, C), s_)
                st[l, b] = s_.reshape(st[l, b].shape)
        assert np.array_equal(own, st), f"rank {r}: bf16 states differ from the contract's replay"


# ---- compact_fwd --------------------------------------------------------------------------------------------------------------------
WL = 4


def _fake_path():
    sys.path.insert(0, os.path.join(HERE, "fake_rccl"))
    try:
        import build as fake_build
        return fake_build.build()
    finally:
        sys.path.pop(0)
        sys.modules.pop("build", None)


@pytest.mark.parametrize("codec,cid", [("BINARY", 1), ("INT2", 2)])
@pytest.mark.parametrize("lane", ["off", "auto"])
def test_compact_fwd_with_bf16_activations(monkeypatch, lane, codec, cid):
    """compact_fwd (gather schedule) with bf16 q, k, v and 4 logical ranks looped back - the lane off (ONE native op per layer on the
    caller's stream, the exchange inside the launch) and auto (the layer's chain on the exchange lane).  The K,V states are the contract's;
    the output is the eager ring formula (block_attention per block, update_out_and_lse) in bf16 on the K,V the rank holds, within the
    tolerance tests/test_gpu_schedules.py uses for its fp16 comparison (rtol = atol = 2e-3)."""
    from compactfusion_amd import _lib, codecs as K, exchange
    from compactfusion_amd.collector import collector
    from compactfusion_amd.compact import ring, main as cm, xlayer
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from compactfusion_amd.compact.attention import block_attention, update_out_and_lse
    from compactfusion_amd.prof import Profiler
    lib = _lib.load()
    monkeypatch.setenv("CFX_RING_SCHEDULE", "gather")
    monkeypatch.setenv("CFX_LANE", lane)
    monkeypatch.delenv("CFX_RING_EXCHANGE_STREAM", raising=False)
    monkeypatch.setattr(ring.dist, "get_rank", lambda g=None: 0)
    monkeypatch.setattr(ring.dist, "get_world_size", lambda g=None: WL)
    monkeypatch.setattr(ring.dist, "all_gather_into_tensor",            # WARMUP steps gather the raw shards through torch.distributed
                        lambda recv, send, group=None: recv.view(WL, -1).copy_(send.view(1, -1).expand(WL, -1)))
    if lane == "auto":
        monkeypatch.setenv("CFX_FAKE_RCCL_MODE", "loopback")
        monkeypatch.setenv("CFX_RING_EXCHANGE", "native")
        fake = _fake_path()

        class LoopComm:
            def __init__(self, group, device):
                ctx = K.context(device)
                assert lib.cfx_rccl_load(fake.encode()) == 0
                uid = ctypes.create_string_buffer(128)
                assert lib.cfx_comm_unique_id(ctx, uid) == 0
                self.handle = lib.cfx_comm_create(ctx, uid, WL, 0)
                assert self.handle
        exchange.set_comm_factory(LoopComm)
    else:
        monkeypatch.delenv("CFX_RING_EXCHANGE", raising=False)
        xlayer.set_p2p_loopback(True)
    Profiler.instance().disable()
    collector.init(collector.Collector("/tmp/none", enabled=False))
    ring._xbuf.clear(); ring._steady.clear(); ring._lane_ok.clear()
    try:
        L, STEPS = 2, 5
        shape = (1, 64, 8, 64)
        N, C = 64, 512
        cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T[codec], comp_rank=-1,
                                      residual=1, ef=True, fastpath=True))
        g = torch.Generator().manual_seed(3)

        def drift():
            cur = torch.randn(*shape, generator=g)
            out = []
            for _ in range(STEPS):
                out.append(cur.bfloat16().contiguous())
                cur = cur + 0.1 * torch.randn(*shape, generator=g)
            return out
        qs, ks, vs = [drift() for _ in range(L)], [drift() for _ in range(L)], [drift() for _ in range(L)]
        want = {}
        for l in range(L):
            for nm, seq in (("k", ks[l]), ("v", vs[l])):
                st = bits(seq[0]).reshape(N, C).copy()
                want[l, nm] = [st]
                for x in seq[1:]:
                    _, st = BC.compress(NAME[cid], bits(x).reshape(N, C), st)
                    want[l, nm].append(st)
        for s in range(STEPS):
            cm.compact_set_step(s)
            for l in range(L):
                q, k, v = qs[l][s].cuda(), ks[l][s].cuda(), vs[l][s].cuda()
                out, lse, _ = ring.compact_fwd(q, k, v, causal=False, mod_idx=l, current_iter=s)
                torch.cuda.synchronize()
                assert out.dtype == torch.bfloat16 and out.shape == shape
                cache = cm.compact_cache()
                for nm in ("k", "v"):
                    for r in range(WL):
                        stt = cache.get_base(f"{l}-{r}-{nm}")
                        assert stt.dtype == torch.bfloat16
                        assert np.array_equal(bits(stt).reshape(N, C), want[l, nm][s]), (lane, s, l, r, nm)
                ro = rl = None
                for t in range(WL):
                    kk = k if t == 0 else cache.get_base(f"{l}-{(0 - t) % WL}-k").view(shape)
                    vv = v if t == 0 else cache.get_base(f"{l}-{(0 - t) % WL}-v").view(shape)
                    bo, bl = block_attention(q, kk, vv, 0.0, shape[-1] ** -0.5, causal=False)
                    ro, rl = update_out_and_lse(ro, rl, bo, bl)
                torch.testing.assert_close(out.float(), ro.to(torch.bfloat16).float(), rtol=2e-3, atol=2e-3)
        assert lib.cfx_gate_errors(K.context(0)) == 0
        exs = [e for e in ring._xbuf.values() if e.sig is not None]
        assert exs, "no layer was bound to a native exchange"
        if lane == "off":
            assert all(e.xop is not None and e.xop.dtype == torch.bfloat16 for e in exs), "the one-op layer exchange was not taken"
        else:
            assert all(e.plan is not None for e in exs), "the native lane plan was not used"
    finally:
        exchange.set_comm_factory(None)
        cm._drop_kv_exchanges()
        for e in ring._xbuf.values():
            e.close()
        ring._xbuf.clear(); ring._steady.clear(); ring._lane_ok.clear()
        xlayer.set_p2p_loopback(False)


def test_gather_entry_points_with_bf16_on_the_gpu(monkeypatch):
    """compact_all_gather_kv (the one-op LayerOp over the looped-back peer-to-peer arena) and compact_compress / compact_decompress with
    bf16 K,V: states are the contract's."""
    from compactfusion_amd.compact import main as cm, xlayer
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    monkeypatch.setenv("CFX_LANE", "off")
    monkeypatch.setattr(cm.dist, "get_rank", lambda g=None: 0)
    monkeypatch.setattr(cm.dist, "get_world_size", lambda g=None: WL)
    monkeypatch.setattr(cm.dist, "all_gather_into_tensor",
                        lambda recv, send, group=None: recv.view(WL, -1).copy_(send.view(1, -1).expand(WL, -1)))
    xlayer.set_p2p_loopback(True)
    try:
        N, C = 128, 1024
        rng = np.random.default_rng(9)
        for codec, cid in (("BINARY", 1), ("INT2", 2)):
            cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=1, ef=True, fastpath=True, comp_rank=-1))
            stk = stv = None
            for t in range(5):
                kb = bf_bits(rng, N, C, near=stk)
                vb = bf_bits(rng, N, C, near=stv)
                typ = T.WARMUP if t == 0 else T[codec]
                ko, vo = cm.compact_all_gather_kv("7-k", "7-v", dev(kb).view(1, N, C), dev(vb).view(1, N, C), typ)
                torch.cuda.synchronize()
                if t == 0:
                    stk, stv = kb, vb
                else:
                    _, stk = BC.compress(NAME[cid], kb, stk)
                    _, stv = BC.compress(NAME[cid], vb, stv)
                for r in range(WL):
                    assert ko[r].dtype == torch.bfloat16 and np.array_equal(bits(ko[r]).reshape(N, C), stk), (codec, t, r)
                    assert np.array_equal(bits(vo[r]).reshape(N, C), stv), (codec, t, r)
            ops = [e.xop for e in cm._kv_exchanges.values() if e.xop is not None]
            assert ops and all(o.dtype == torch.bfloat16 for o in ops), "the one-op layer exchange was not taken"
            # the plain pair on the same codec
            xb = bf_bits(rng, N, C)
            cm.compact_compress("9-0-k", dev(xb), T.WARMUP, update_cache=True)
            cm.compact_decompress("9-1-k", dev(xb), T.WARMUP, (N, C), update_cache=True)
            x2 = bf_bits(rng, N, C, near=xb)
            pkt = cm.compact_compress("9-0-k", dev(x2), T[codec], update_cache=True)
            rec = cm.compact_decompress("9-1-k", pkt.clone(), T[codec], (N, C), update_cache=True)
            torch.cuda.synchronize()
            wp, wn = BC.compress(NAME[cid], x2, xb)
            assert bits(pkt).tobytes() == wp.tobytes() and rec.dtype == torch.bfloat16
            assert np.array_equal(bits(rec).reshape(N, C), wn) and np.array_equal(bits(cm.compact_cache().get_base("9-0-k")).reshape(N, C), wn)
    finally:
        cm._drop_kv_exchanges()
        xlayer.set_p2p_loopback(False)


def test_mixed_element_types_raise_value_error_on_the_gpu():
    from compactfusion_amd import codecs as K
    N, C = 64, 512
    x = torch.zeros(N, C, dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(N, C, dtype=torch.float16, device="cuda")
    pkt = torch.zeros(K.packet_halves(1, N, C), dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="mixed element types"):
        K.compress_batch(1, [x], [b], [b], [pkt], N, C)
    with pytest.raises(ValueError, match="mixed element types"):
        K.decompress_batch(2, [pkt], [x], [b], N, C)
    with pytest.raises(ValueError, match="mixed element types"):
        K.compress(1, x, b, N, C)
    with pytest.raises(ValueError):                                   # bf16 with a codec that has no bf16 form: CFX_ERR_CODEC
        K.compress_batch(3, [x], [x], [x], [torch.zeros(K.packet_halves(3, N, C), dtype=torch.float16, device="cuda")], N, C)
    run = K.prepare_compress(1, [x], [x], [pkt], N, C)
    with pytest.raises(ValueError):
        run([b])
    torch.cuda.synchronize()
