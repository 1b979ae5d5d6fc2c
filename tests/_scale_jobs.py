"""The layer launches' scale jobs (csrc/cfx_absmean.hip absmean_tagged_jobs: a column block's V job split over workgroups, the U job's one
round, the 16-byte scale stores) through cfx_compress_batch_gated, against the oracle bit for bit.  Shared by tests/test_gpu_scale_jobs.py
(the product library: the split the library chooses) and tests/scale_jobs_child.py (the developer library: every split forced)."""
import ctypes

import numpy as np
import torch

import _bf16_cases as V
import bf16_contract as BC
from oracle import ref_np as R

F16 = np.float16
NAME = {1: "binary", 2: "int2"}
KID_LAYER = 31
UPD = 1

# the shapes are the smallest at which each path of the jobs is taken (32-row statistics tiles: P = ceil(N / 32))
P_AROUND_THE_SPLIT = [(n, 512) for n in (2, 33, 64, 96, 130, 160)]                 # P = 1 .. 5: U behind V, the split clamped, U on its own tile
RAGGED_BLOCKS = [(96, 1152), (64, 640), (64, 128)]                                 # a last column block of 128 channels: sub-jobs without a channel
MANY_BLOCKS = [(34, 8192)]
U_ROUNDS = [(n, 512) for n in (511, 512, 513, 544, 1024, 1025, 1100)]              # one row a thread, two, a ragged second, a third pass
ALIGNMENT = [(n, 512) for n in (2, 130, 132, 544)]
ALL_SHAPES = list(dict.fromkeys(P_AROUND_THE_SPLIT + RAGGED_BLOCKS + MANY_BLOCKS + U_ROUNDS + ALIGNMENT))
SMALL_SHAPES = list(dict.fromkeys(P_AROUND_THE_SPLIT + RAGGED_BLOCKS + MANY_BLOCKS + ALIGNMENT + [(513, 512), (1100, 512)]))


def scale_store_paths(cid, N, C):
    """(V packed, rows of U stored per element) from the packet layout: sign bits / codes, then U (N fp16), then V (C fp16); a 16-byte
    store needs its 8 scales 16-byte aligned in a 16-byte aligned packet"""
    bits_bytes = N * C // (8 if cid == 1 else 4)
    assert bits_bytes % 16 == 0
    return (bits_bytes + 2 * N) % 16 == 0, N % 8


def to_dev(u16):
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16).copy()).cuda()


def host_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def same_bits(a, b, what):
    a = np.asarray(a).view(np.uint16).reshape(-1)
    b = np.asarray(b).view(np.uint16).reshape(-1)
    assert a.size == b.size, f"{what}: {a.size} words against {b.size}"
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())}/{a.size} differ (first at {int(np.argmax(bad))})"


def inputs(seed, N, C, bf16, drift=0.1):
    """(x, state) as 16-bit words"""
    rng = np.random.default_rng(seed)
    if bf16:
        base = V.bf16_bits(0.5 * rng.standard_normal((N, C)))
        x = V.bf16_bits(V.bf16_f32(base) + 2 * drift * rng.standard_normal((N, C)).astype(np.float32))
        return x, base
    base = rng.standard_normal((N, C)).astype(F16)
    x = (base.astype(np.float32) + drift * rng.standard_normal((N, C)).astype(np.float32)).astype(F16)
    return x.view(np.uint16), base.view(np.uint16)


def reference(cid, bf16, x, state):
    """one step of the codec with error feedback: (packet words, new state words)"""
    if bf16:
        return BC.compress(NAME[cid], x, state)
    p, nb = R.residual_compress(NAME[cid], x.view(F16), state.view(F16), 0)
    return np.asarray(p).view(np.uint16), R.bits(nb).copy()


def layer_ran(lib, ctx, fn):
    torch.cuda.synchronize()
    assert lib.cfx_profile_enable(ctx, 64, 0xffffffff, 1) == 0
    try:
        fn()
        torch.cuda.synchronize()
        ids, ms = (ctypes.c_int * 64)(), (ctypes.c_float * 64)()
        n = lib.cfx_profile_read(ctx, ids, ms, 64)
    finally:
        lib.cfx_profile_enable(ctx, 0, 0, 1)
    return KID_LAYER in [ids[i] for i in range(n)]


def layer_case(cid, bf16, N, C, B, drift=0.1, NP=3, launches=3, seed=0):
    """`launches` back-to-back layer launches (gate and tag reuse; every launch's scales feed the next one's residual) of B own tensors - error
    feedback in place, by CFX_FLAG_UPDATE_CACHE - and NP looped-back peer states: the last packets (bits / codes and fp16 scales) and every
    state equal the reference stepped as often."""
    from compactfusion_amd import _lib, codecs as K
    lib = _lib.load()
    ctx = K.context(0)
    pairs = [inputs(seed + 31 * N + C + i, N, C, bf16, drift) for i in range(B)]
    xs = [x for x, _ in pairs]
    state = [np.array(b, copy=True) for _, b in pairs]
    xd = [to_dev(x) for x in xs]
    own = [to_dev(b) for b in state]
    src = [g % B for g in range(NP)]
    peer = [to_dev(state[s]) for s in src]
    pk = [torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda") for _ in range(B)]
    assert all(p.data_ptr() % 16 == 0 for p in pk)
    code = cid | (BC.ELEM_BF16 if bf16 else 0)
    wsb = lib.cfx_workspace_bytes(code, N, C, 0, B)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    comp = (_lib.CompItem * B)(*[_lib.CompItem(xd[i].data_ptr(), own[i].data_ptr(), own[i].data_ptr(), pk[i].data_ptr()) for i in range(B)])
    gated = (_lib.DecompItem * NP)(*[_lib.DecompItem(pk[src[g]].data_ptr(), peer[g].data_ptr(), peer[g].data_ptr()) for g in range(NP)])
    sh = torch.cuda.current_stream().cuda_stream

    def call():
        rc = lib.cfx_compress_batch_gated(ctx, code, N, C, 0, UPD, B, comp, 0, None, NP, gated, ws.data_ptr(), wsb, sh)
        assert rc == 0, lib.cfx_last_error_string(ctx)

    what = f"{NAME[cid]} {'bf16' if bf16 else 'fp16'} ({N}, {C}) x {B}"
    assert layer_ran(lib, ctx, lambda: [call() for _ in range(launches)]), f"{what}: not the one-launch layer form"
    assert lib.cfx_gate_errors(ctx) == 0, what
    last = [None] * B
    for t in range(launches):
        for i in range(B):
            last[i], state[i] = reference(cid, bf16, xs[i], state[i])
    for i in range(B):
        same_bits(host_bits(pk[i]), last[i], f"{what}: packet {i} of launch {launches - 1}")
        same_bits(host_bits(own[i]), state[i], f"{what}: own state {i} after {launches} launches")
    for g in range(NP):
        same_bits(host_bits(peer[g]), state[src[g]], f"{what}: peer state {g} after {launches} launches")
