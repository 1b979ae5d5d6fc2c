"""The contract of the second-order residual inside the 1-bit and 2-bit codec launches (include/cfx.h, "Second-order residual"), as a
composition of the pinned oracle (oracle/ref_np.py) - plain module, shared by tests/test_res2_host.py (CPU) and the GPU tests:

    dd        = R.residual2_delta(x, base, delta_base)                    fp16( fp16(x - base) - delta_base )
    pkt, recv = R.residual_compress(name, dd, None, param)                the fp16 codec unchanged, as if base were NULL
    new_base, new_delta = R.residual2_update(base, delta_base, recv, decay)

tests/test_res2_host.py holds it equal to R.OracleCompact(residual=2).  The second half of the module is a TEST-ONLY stand-in for
`codecs.compress_batch_res2` / `codecs.decompress_batch_res2` on CPU tensors (the product has no CPU path), for the host-logic tests."""
import numpy as np
import torch

from oracle import ref_np as R

F16 = np.float16
NAMES = {1: "binary", 2: "int2"}


def _f16(a, N, C):
    return np.ascontiguousarray(a).view(np.uint16).view(F16).reshape(N, C)


def compress(name, x, base, dbase, decay, param=0):
    """(packet words, new_base bits, new_delta bits) of one second-order compress; x / base / dbase: (N, C) fp16 values or their bits"""
    N, C = np.asarray(x).shape
    x, base, dbase = _f16(x, N, C), _f16(base, N, C), _f16(dbase, N, C)
    with np.errstate(invalid="ignore", over="ignore"):
        dd = R.residual2_delta(x, base, dbase)
        pkt, recv = R.residual_compress(name, dd, None, param)
        nb, nd = R.residual2_update(base, dbase, recv, decay)
    return np.asarray(pkt).view(np.uint16).reshape(-1), R.bits(nb).reshape(N, C), R.bits(nd).reshape(N, C)


def decompress(name, pkt, base, dbase, decay, N, C, param=0):
    """(recon bits, new_delta bits) of one second-order reconstruction"""
    base, dbase = _f16(base, N, C), _f16(dbase, N, C)
    with np.errstate(invalid="ignore", over="ignore"):
        recv = R.residual_decompress(name, np.asarray(pkt).view(np.uint16).reshape(-1), None, N, C, param)
        nb, nd = R.residual2_update(base, dbase, recv, decay)
    return R.bits(nb).reshape(N, C), R.bits(nd).reshape(N, C)


# ---- TEST-ONLY stand-in for the two fused codecs functions, on CPU tensors ------------------------------------------------------------
def _np16(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def _put(t, words):
    t.view(torch.int16).numpy().view(np.uint16).reshape(-1)[:] = np.asarray(words).reshape(-1)


calls = []          # ("compress" | "decompress", codec, batch, update) per stand-in call


def compress_batch_res2(codec, xs, bases, delta_bases, new_bases, new_delta_bases, packets, N, C, decay, param=0, update_cache=True,
                        stream=None, ws=None):
    calls.append(("compress", int(codec), len(xs), bool(update_cache)))
    for x, b, d, nb, nd, p in zip(xs, bases, delta_bases, new_bases, new_delta_bases, packets):
        pkt, wb, wd = compress(NAMES[int(codec)], _np16(x).reshape(N, C), _np16(b).reshape(N, C).copy(), _np16(d).reshape(N, C).copy(), decay, param)
        p.view(torch.int16).numpy().view(np.uint16).reshape(-1)[:pkt.size] = pkt
        if update_cache:
            _put(nb, wb)
            _put(nd, wd)


def decompress_batch_res2(codec, packets, bases, delta_bases, recons, new_delta_bases, N, C, decay, param=0, stream=None):
    calls.append(("decompress", int(codec), len(packets), all(nd is not None for nd in new_delta_bases)))
    n_half = R.packet_halves(NAMES[int(codec)], N, C, param)
    for p, b, d, r, nd in zip(packets, bases, delta_bases, recons, new_delta_bases):
        wb, wd = decompress(NAMES[int(codec)], _np16(p).reshape(-1)[:n_half].copy(), _np16(b).reshape(N, C).copy(), _np16(d).reshape(N, C).copy(),
                            decay, N, C, param)
        _put(r, wb)
        if nd is not None:
            _put(nd, wd)
