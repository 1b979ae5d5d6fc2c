"""The contract of the 1-bit codec with rank-K scales (include/cfx.h "1-bit codec with rank-K scales"; k_binary_rank, csrc/cfx_absmean.hip)
in plain numpy - written from the header and the comment above the kernel, independent of oracle/ref_np.py (tests/test_brank_host.py
holds the two against each other).  The arithmetic is fully specified, so the witness is BIT FOR BIT: no tolerance anywhere.

    d          = fp16(x - base), one rounding                       base None: d = x
    bit e of byte (n, c / 8) = d[n, c + e] >= 0                     -0 and +0 give 1, NaN gives 0
    scale[n,c] = fp16( sum_k fp32( fp16(U[n,k] * V[c,k]) ) )        the product rounded ONCE to fp16 (subnormals kept), the adds in fp32 in
                                                                    index order from +0, one final rounding
    recv       = bit ? scale : -scale
    out        = fp16(base + recv)                                  base None: recv
    sender: NO_EF: new_base = x;  no UPDATE_CACHE: new_base is not written
    packet     = [ bits N*C/8 | U (N,K) fp16 | V (C,K) fp16 ]       the factor sections are the factors' bits

The products are formed in float64 (two fp16 factors: 22 bits, exact) and rounded once; that is what "fp16 product, one rounding" means
and also what an exact fp32 product rounded to fp16 gives.  A NaN has no contractual payload: same() takes any NaN for any NaN and
every other value by its bits (the `large` case keeps the products of one sum of one sign, so no inf - inf arises in a sum).

scale(.., fault=...) plants the errors a kernel could make (FAULTS); tests/test_brank_host.py shows each is caught."""
import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64

FAULTS = ("chunk dropped",        # the factors k >= 8 never reach the sum
          "no k guard",           # chunks of 8 without `k0 + k < K`: the next row's factors (flat index) join the sum
          "product not rounded",  # the exact product goes into the fp32 sum
          "fp16 sum",             # the adds run in fp16
          "V as (K, C)")          # V's section indexed transposed


def f16(a):
    return np.ascontiguousarray(a, dtype=F16)


def residual(x, base):
    x = f16(x)
    if base is None:
        return x
    with np.errstate(invalid="ignore", over="ignore"):
        return (x.astype(F64) - f16(base).astype(F64)).astype(F16)              # exact difference, one rounding


def sign_bits(x, base):
    """(N, C / 8) bytes"""
    d = residual(x, base)
    N, C = d.shape
    with np.errstate(invalid="ignore"):
        b = (d >= 0).reshape(N, C // 8, 8)
    return (b * (1 << np.arange(8))).sum(2).astype(np.uint8)


def unpack(bits, C):
    return ((bits[:, :, None] >> np.arange(8, dtype=np.uint8)) & 1).reshape(bits.shape[0], C).astype(bool)


def _flat_next(M, K, KP):
    """(rows, KP): element [i, k] is M.flat[i * K + k], 0 past the end - what a read without the k guard sees"""
    rows = M.shape[0]
    flat = np.concatenate([M.reshape(-1), np.zeros(KP, dtype=M.dtype)])
    idx = np.arange(rows)[:, None] * K + np.arange(KP)[None, :]
    return flat[idx]


def scale(U, V, fault=None):
    """(N, C) fp16 from U (N, K), V (C, K)"""
    U, V = f16(U), f16(V)
    K = U.shape[1]
    assert V.shape[1] == K and fault in (None,) + FAULTS
    if fault == "V as (K, C)":
        V = np.ascontiguousarray(V.reshape(K, V.shape[0]).T)
    if fault == "no k guard":
        KP = -(-K // 8) * 8
        U, V, K = _flat_next(U, K, KP), _flat_next(V, K, KP), KP
    if fault == "chunk dropped":
        K = min(K, 8)
    acc = np.zeros((U.shape[0], V.shape[0]), dtype=F16 if fault == "fp16 sum" else F32)           # +0
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(K):
            p = U[:, k].astype(F64)[:, None] * V[:, k].astype(F64)[None, :]                      # exact
            p = p.astype(F32) if fault == "product not rounded" else p.astype(F16)
            acc = acc + p.astype(acc.dtype)
        return acc.astype(F16)


def apply(bits, U, V, base, fault=None):
    """the receiver's reconstruction / the sender's error-feedback state"""
    sc = scale(U, V, fault)
    recv = np.where(unpack(bits, sc.shape[1]), sc, -sc)
    if base is None:
        return recv
    with np.errstate(invalid="ignore", over="ignore"):
        return (f16(base).astype(F64) + recv.astype(F64)).astype(F16)                            # exact sum, one rounding


def packet(bits, U, V):
    """the wire bytes"""
    return np.concatenate([np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1), f16(U).reshape(-1).view(np.uint8),
                           f16(V).reshape(-1).view(np.uint8)])


def packet_bytes(N, C, K):
    """cfx_binary_rank_packet_bytes, 0 where the shape is refused"""
    if N < 1 or C < 1 or C % 8 or not 1 <= K <= 32 or (N * (C // 8)) % 2:
        return 0
    return N * C // 8 + 2 * (N + C) * K


def split(pk, N, C, K):
    """-> bits (N, C / 8) uint8, U (N, K), V (C, K) fp16"""
    pk = np.ascontiguousarray(pk).reshape(-1).view(np.uint8)
    assert pk.size == packet_bytes(N, C, K) != 0
    nb = N * C // 8
    return pk[:nb].reshape(N, C // 8), pk[nb:nb + 2 * N * K].view(F16).reshape(N, K), pk[nb + 2 * N * K:].view(F16).reshape(C, K)


def sender(x, base, U, V, ef=True):
    """what cfx_binary_rank_compress_batch leaves GIVEN the factors its chain produced: (packet bytes, new_base)"""
    bits = sign_bits(x, base)
    return packet(bits, U, V), (apply(bits, U, V, base) if ef else f16(x).copy())


def same(a, b):
    """bit for bit; a NaN for a NaN"""
    a, b = f16(a), f16(b)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint16) == b.view(np.uint16)) | (np.isnan(a) & np.isnan(b))).all())


def differing(a, b):
    a, b = f16(a), f16(b)
    return int((~((a.view(np.uint16) == b.view(np.uint16)) | (np.isnan(a) & np.isnan(b)))).sum())
