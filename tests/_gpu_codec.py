"""What tests/test_gpu_codec_domain.py (the shape domain) and tests/test_gpu_value_domain.py (the value domain) share: tensors to and from
the device, the oracle of one residual compress, the kernel ids a call launched, and the gated layer call with looped-back peers.
Plain module (GPU box only: imported by tests marked gpu)."""
import ctypes

import numpy as np
import torch

import _f64_check as F
import _nonfinite as NF
import _zero_min as Z
from oracle import c_oracle as CO
from oracle import ref_np as R

F16 = np.float16
BIG = 4 << 20                     # elements: above, the C oracle (OpenMP) instead of numpy
KID_LAYER = 31                    # csrc/cfx_internal.h KID_ABSMEAN_COMPRESS_GATED: every codec's layer launch
same_bits = NF.same_bits


def dev(a16):
    return torch.from_numpy(np.ascontiguousarray(a16).view(np.int16)).view(torch.float16).cuda()


def host(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def inputs(seed, N, C):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((N, C)).astype(F16)
    x = (base.astype(np.float32) + 0.1 * rng.standard_normal((N, C)).astype(np.float32)).astype(F16)
    return x, base


def oracle(name, x, base, param, N, C, ef=True):
    """(packet words, new state) of one residual compress"""
    if N * C > BIG:
        CO.set_num_threads(16)
        pkt, nb = CO.compress(name, x, base, N, C, param, update=True, ef=ef)
        return np.asarray(pkt).view(np.uint16).reshape(-1), np.asarray(nb).view(np.uint16).reshape(N, C)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pkt, nb = R.residual_compress(name, x, base, param, ef=ef) if base is not None else R.compress(name, x, None, param)
    return np.asarray(pkt).view(np.uint16), R.bits(nb)


def same_packet(name, got, want, x, base, what, allowed=None):
    """a packet against the oracle's, bit for bit - but for the int4 `min` half of a channel whose zero minimum occurs with both signs
    (tests/_zero_min.py).  allowed None: no such channel may occur (random inputs have none); a set: the channels the rule was used on
    are added to it, for the caller to hold against what its input planted."""
    used = Z.same_packet(name, got, want, x, base, what)
    if allowed is None:
        assert not used, f"{what}: int4 min differs by the sign of a zero on channel(s) {sorted(used)[:8]} of an input that plants none"
    else:
        allowed |= used


def _profile(ctx, lib, fn):
    """kernel ids of what fn launched"""
    torch.cuda.synchronize()
    assert lib.cfx_profile_enable(ctx, 64, 0xffffffff, 1) == 0
    try:
        fn()
        torch.cuda.synchronize()
        ids, ms = (ctypes.c_int * 64)(), (ctypes.c_float * 64)()
        n = lib.cfx_profile_read(ctx, ids, ms, 64)
    finally:
        lib.cfx_profile_enable(ctx, 0, 0, 1)
    return [ids[i] for i in range(n)]


# ---- the gated layer call: own error feedback + looped-back peers, over rounds ----
def _gated_layer(name, cid, param, N, C, B, NP, rounds, seed, check=True, ins=None, allowed=None, f64=False):
    """cfx_compress_batch_gated as test_gated_int2_layer_in_one_launch drives it; returns the kernel ids of the first round.
    ins: the B (x, state) pairs instead of the random ones of `seed`; allowed: see same_packet; f64: every round's packet and own state
    against the float64 definition as well (tests/_f64_check.py)."""
    from compactfusion_amd import _lib, codecs as K
    lib = _lib.load()
    ctx = K.context(0)
    if ins is None:
        ins = [inputs(seed + i, N, C) for i in range(B)]
    xs = [x for x, _ in ins]
    xd = [dev(x) for x in xs]
    own = [dev(b) for _, b in ins]
    src = [i % B for i in range(NP)]
    peer = [dev(ins[src[g]][1]) for g in range(NP)]
    pk = [torch.zeros(K.packet_halves(cid, N, C, param), dtype=torch.float16, device="cuda") for _ in range(B)]
    ws = K.workspace(cid, N, C, param, B, 0)
    wsp, wsn = (None, 0) if ws is None else (ws.data_ptr(), ws.numel())
    sh = torch.cuda.current_stream().cuda_stream
    comp = (_lib.CompItem * B)(*[_lib.CompItem(xd[i].data_ptr(), own[i].data_ptr(), own[i].data_ptr(), pk[i].data_ptr()) for i in range(B)])
    gated = (_lib.DecompItem * NP)(*[_lib.DecompItem(pk[src[g]].data_ptr(), peer[g].data_ptr(), peer[g].data_ptr()) for g in range(NP)])

    def go():
        assert lib.cfx_compress_batch_gated(ctx, cid, N, C, param, _lib.FLAG_UPDATE_CACHE, B, comp, 0, None, NP, gated, wsp, wsn, sh) == 0
    ostate = [np.ascontiguousarray(b).view(np.uint16).copy() for _, b in ins]
    ids = None
    for t in range(rounds):
        if ids is None:
            ids = _profile(ctx, lib, go)
        else:
            go()
        if not check:
            continue
        opk, before = [], [s for s in ostate]
        for i in range(B):
            p, nb = oracle(name, xs[i], ostate[i].view(F16), param, N, C)
            opk.append(p)
            ostate[i] = nb.copy()
        torch.cuda.synchronize()
        assert lib.cfx_gate_errors(ctx) == 0
        for i in range(B):
            same_packet(name, host(pk[i]), opk[i], xs[i], before[i].view(F16), f"packet round {t} item {i}", allowed)
            same_bits(host(own[i]), ostate[i], f"own state round {t} item {i}")
            if f64:
                F.check(name, param, xs[i], before[i].view(F16), host(pk[i]), host(own[i]).reshape(N, C))
        for g in range(NP):
            same_bits(host(peer[g]), ostate[src[g]], f"peer state round {t} peer {g}")
    torch.cuda.synchronize()
    return ids
