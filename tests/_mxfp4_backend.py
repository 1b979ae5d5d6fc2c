"""TEST-ONLY stand-in for the HIP kernels with the MXFP4 codec (id 8): tests/_oracle_backend.py for every other codec, the numpy
contract of tests/mxfp4_contract.py for id 8.  Installed by monkeypatching inside tests, never shipped."""
import numpy as np
import torch

import _oracle_backend as OB
import mxfp4_contract as I

CID = I.CID


def compress_batch(codec, xs, bases, new_bases, packets, N, C, param=0, update_cache=True, ef=True, stream=None, ws=None):
    if int(codec) != CID:
        return OB.compress_batch(codec, xs, bases, new_bases, packets, N, C, param, update_cache, ef, stream, ws)
    for x, b, nb, p in zip(xs, bases, new_bases, packets):
        bb = None if b is None else OB._np16(b).reshape(N, C).copy()
        pkt, newb = I.residual_compress(OB._np16(x).reshape(N, C), bb, ef)
        p.view(torch.int16).numpy().view(np.uint16).reshape(-1)[:pkt.size] = pkt
        if update_cache and nb is not None:
            nb.view(torch.int16).numpy().view(np.uint16).reshape(N, C)[:] = I.R.bits(newb)


def decompress_batch(codec, packets, bases, recons, N, C, param=0, stream=None):
    if int(codec) != CID:
        return OB.decompress_batch(codec, packets, bases, recons, N, C, param, stream)
    n_half = I.packet_halves(N, C)
    for p, b, r in zip(packets, bases, recons):
        bb = None if b is None else OB._np16(b).reshape(N, C).copy()
        rec = I.residual_decompress(OB._np16(p).reshape(-1)[:n_half].copy(), bb, N, C)
        r.view(torch.int16).numpy().view(np.uint16).reshape(N, C)[:] = I.R.bits(rec)


def prepare_compress(codec, bases, new_bases, packets, N, C, param=0, update_cache=True, ef=True):
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
    OB.install(monkeypatch)
    for k, v in _OURS.items():
        monkeypatch.setattr(codecs, k, v)


def install_plain():
    """For spawned worker processes (no pytest monkeypatch there)."""
    from compactfusion_amd import codecs
    OB.install_plain()
    for k, v in _OURS.items():
        setattr(codecs, k, v)


# ---- worker body for the world_size-2 gloo test (spawned by tests/test_mxfp4_host.py through _dist_workers.run) ----
def w_all_gather_mxfp4(rank, world):
    import _dist_workers as W
    install_plain()
    return W.w_all_gather(rank, world, "MXFP4")
