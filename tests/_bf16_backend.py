"""TEST-ONLY stand-in for the HIP kernels that also takes bf16 tensors: tests/_oracle_backend.py for fp16, the bf16 contract
(tests/bf16_contract.py) for bf16, chosen from the tensors of the call as `compactfusion_amd.codecs` does - a mix raises ValueError,
bf16 with a codec that has no bf16 form too.  Installed by monkeypatching inside tests; never shipped."""
import numpy as np
import torch

import _oracle_backend as OB
import bf16_contract as BC
from compactfusion_amd import codecs as _codecs

_elem = _codecs.elem_dtype       # (the product's own rule for a call's element type)


def _u16(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def compress_batch(codec, xs, bases, new_bases, packets, N, C, param=0, update_cache=True, ef=True, stream=None, ws=None):
    if _elem(*xs, *bases, *new_bases) != torch.bfloat16:
        return OB.compress_batch(codec, xs, bases, new_bases, packets, N, C, param, update_cache, ef)
    if int(codec) not in BC.NAMES:
        raise ValueError(f"cfx_compress_batch: CFX_ERR_CODEC: no bf16 form of codec {int(codec)}")
    for x, b, nb, p in zip(xs, bases, new_bases, packets):
        pkt, newb = BC.compress(BC.NAMES[int(codec)], _u16(x).reshape(N, C), None if b is None else _u16(b).reshape(N, C).copy(), param, ef)
        _u16(p).reshape(-1)[:pkt.size] = pkt
        if update_cache and nb is not None:
            _u16(nb).reshape(N, C)[:] = newb


def decompress_batch(codec, packets, bases, recons, N, C, param=0, stream=None):
    if _elem(*recons, *bases) != torch.bfloat16:
        return OB.decompress_batch(codec, packets, bases, recons, N, C, param)
    if int(codec) not in BC.NAMES:
        raise ValueError(f"cfx_decompress_batch: CFX_ERR_CODEC: no bf16 form of codec {int(codec)}")
    name = BC.NAMES[int(codec)]
    n_half = BC.R.packet_halves(name, N, C, param)
    for p, b, r in zip(packets, bases, recons):
        rec = BC.decompress(name, _u16(p).reshape(-1)[:n_half].copy(), None if b is None else _u16(b).reshape(N, C).copy(), N, C, param)
        _u16(r).reshape(N, C)[:] = rec


def prepare_compress(codec, bases, new_bases, packets, N, C, param=0, update_cache=True, ef=True, dtype=None):
    def run(xs, stream_handle=None):
        compress_batch(codec, xs, bases, new_bases, packets, N, C, param, update_cache, ef)
    return run


def prepare_decompress(codec, packets, bases, recons, N, C, param=0):
    def run(stream_handle=None):
        decompress_batch(codec, packets, bases, recons, N, C, param)
    return run


_PATCHED = dict(compress_batch=compress_batch, decompress_batch=decompress_batch, prepare_compress=prepare_compress,
                prepare_decompress=prepare_decompress)


def install(monkeypatch):
    OB.install(monkeypatch)
    for k, f in _PATCHED.items():
        monkeypatch.setattr(_codecs, k, f)


def install_plain():
    OB.install_plain()
    for k, f in _PATCHED.items():
        setattr(_codecs, k, f)
