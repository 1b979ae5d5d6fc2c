"""TEST-ONLY stand-in for the HIP kernels with the MXINT8 codec (id 16): tests/_bf16_backend.py (tests/_oracle_backend.py plus the bf16
forms of the 1-bit and 2-bit codecs) for every other codec, the numpy contract of tests/mxint8_contract.py for id 16 - fp16 or bf16, chosen
from the tensors of the call as `compactfusion_amd.codecs` does; param is 0.  Installed by monkeypatching inside tests, never shipped."""
import torch

import _bf16_backend as BB
import mxint8_contract as I

CID = I.CID
_u16 = BB._u16


def _shape(what, N, C, param):
    if not I.shape_ok(N, C) or param != 0:
        raise ValueError(f"{what}: CFX_ERR_SHAPE: N={N} C={C} param={param}")


def compress_batch(codec, xs, bases, new_bases, packets, N, C, param=0, update_cache=True, ef=True, stream=None, ws=None):
    if int(codec) != CID:
        return BB.compress_batch(codec, xs, bases, new_bases, packets, N, C, param, update_cache, ef, stream, ws)
    bf = BB._elem(*xs, *bases, *new_bases) == torch.bfloat16
    _shape("cfx_compress_batch", N, C, param)
    for x, b, nb, p in zip(xs, bases, new_bases, packets):
        pkt, newb = I.step(_u16(x).reshape(N, C), None if b is None else _u16(b).reshape(N, C).copy(), bf, ef)
        _u16(p).reshape(-1)[:pkt.size] = pkt
        if update_cache and nb is not None:
            _u16(nb).reshape(N, C)[:] = newb


def decompress_batch(codec, packets, bases, recons, N, C, param=0, stream=None):
    if int(codec) != CID:
        return BB.decompress_batch(codec, packets, bases, recons, N, C, param, stream)
    bf = BB._elem(*recons, *bases) == torch.bfloat16
    _shape("cfx_decompress_batch", N, C, param)
    n_half = I.packet_halves(N, C)
    for p, b, r in zip(packets, bases, recons):
        rec = I.recon(_u16(p).reshape(-1)[:n_half].copy(), None if b is None else _u16(b).reshape(N, C).copy(), N, C, bf)
        _u16(r).reshape(N, C)[:] = rec


def prepare_compress(codec, bases, new_bases, packets, N, C, param=0, update_cache=True, ef=True, dtype=None):
    def run(xs, stream_handle=None):
        compress_batch(codec, xs, bases, new_bases, packets, N, C, param, update_cache, ef)
    return run


def prepare_decompress(codec, packets, bases, recons, N, C, param=0):
    def run(stream_handle=None):
        decompress_batch(codec, packets, bases, recons, N, C, param)
    return run


_OURS = dict(compress_batch=compress_batch, decompress_batch=decompress_batch, prepare_compress=prepare_compress,
             prepare_decompress=prepare_decompress)


def install(monkeypatch):
    from compactfusion_amd import codecs
    BB.install(monkeypatch)
    for k, v in _OURS.items():
        monkeypatch.setattr(codecs, k, v)


def install_plain():
    """For spawned worker processes (no pytest monkeypatch there)."""
    from compactfusion_amd import codecs
    BB.install_plain()
    for k, v in _OURS.items():
        setattr(codecs, k, v)


# ---- worker body for the world_size-2 gloo test (spawned by tests/test_mxint8_host.py through _dist_workers.run) ----
def w_all_gather_mxint8(rank, world):
    import _dist_workers as W
    install_plain()
    return W.w_all_gather(rank, world, "MXINT8")
