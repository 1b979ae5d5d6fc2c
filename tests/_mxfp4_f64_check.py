"""An independent float64 witness of the MXFP4 codec (include/cfx.h, "MXFP4"): it shares no code with tests/mxfp4_contract.py, takes the
shared exponent from np.frexp of the block maximum (not from fp16 bits) and judges every element code by DISTANCE to the grid (not by
thresholds):

  * scale byte = max(floor(log2 max|d|), -21) - 2 + 127; a block with a non-finite delta: 0xFF, codes 0
  * every reconstructed magnitude is a grid point nearest to y = |d| / 2^X; where two grid points are equally near, the even index;
    y > 6 has 6 as its nearest grid point, so saturation needs no rule of its own - and happens only there
  * the sign bit of the code is the sign bit of the delta (a zero magnitude included)
  * decode is exact in fp16; with error feedback the state is fp16(base + recv)

Hence |recv - d| <= 2^X (half the widest grid step, 2) and, where y > 6, < 2 * 2^X: derived from the grid, not measured."""
import numpy as np

F16, F64 = np.float16, np.float64
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def check(x, base, pkt, state=None, ef=True):
    x = np.asarray(x).view(F16) if np.asarray(x).dtype == np.uint16 else np.asarray(x)
    N, C = x.shape
    if base is None:
        d16 = x.copy()
    else:
        base = np.asarray(base).view(F16) if np.asarray(base).dtype == np.uint16 else np.asarray(base)
        with np.errstate(invalid="ignore", over="ignore"):
            d16 = (x.astype(F64) - base.astype(F64)).astype(F16)         # the correctly rounded difference
    d = d16.astype(F64)
    by = np.ascontiguousarray(np.asarray(pkt).view(np.uint16).reshape(-1)).view(np.uint8)
    assert by.size == N * C // 2 + N * C // 32, "packet length"
    cb, sb = by[:N * C // 2].reshape(N, C // 2), by[N * C // 2:].reshape(N, C // 32).astype(np.int64)
    code = np.empty((N, C), dtype=np.int64)
    code[:, 0::2], code[:, 1::2] = cb & 15, cb >> 4
    dblk = d.reshape(N, C // 32, 32)
    finite = np.isfinite(dblk).all(axis=2)
    # ---- blocks with a NaN or an inf
    assert (sb[~finite] == 0xFF).all(), "a non-finite block without the 0xFF scale byte"
    assert (sb[finite] != 0xFF).all(), "a finite block with the 0xFF scale byte"
    assert (code.reshape(N, C // 32, 32)[~finite] == 0).all(), "a non-finite block with non-zero codes"
    # ---- the shared exponent
    amax = np.where(finite, np.abs(np.where(np.isfinite(dblk), dblk, 0)).max(axis=2), 1.0)
    _, ex = np.frexp(amax)                                               # amax = m * 2^ex, 0.5 <= m < 1: floor(log2 amax) = ex - 1
    e = np.where(amax == 0, -21, np.maximum(ex - 1, -21))
    X = e - 2
    bad = finite & (sb != X + 127)
    assert not bad.any(), f"scale byte: {int(bad.sum())} blocks differ from floor(log2 max) - 2 + 127 (first: got {sb[bad][:1]}, want {(X + 127)[bad][:1]})"
    # ---- the element codes by distance
    fin = np.repeat(finite, 32, axis=1)
    Xe = np.repeat(X, 32, axis=1)
    y = np.where(fin, np.abs(np.where(fin, d, 0)) / np.ldexp(1.0, Xe), 0.0)
    assert (y < 8).all()
    mag, sign = code & 7, code >> 3
    dist = np.abs(GRID[None, None, :] - y[:, :, None])
    best = dist.min(axis=2)
    mine = np.take_along_axis(dist, mag[:, :, None], axis=2)[:, :, 0]
    bad = fin & (mine != best)
    assert not bad.any(), f"{int(bad.sum())} codes are not a nearest grid point"
    tie = fin & ((dist == best[:, :, None]).sum(axis=2) > 1)
    assert not (tie & (mag % 2 == 1)).any(), "a tie went to the odd index"
    assert not (fin & (mag == 7) & (y <= 5)).any() and not (fin & (y > 6) & (mag != 7)).any(), "saturation"
    assert not (fin & (sign != np.signbit(d))).any(), "sign bit"
    # ---- decode: exact in fp16, within the derived bounds
    recv = np.where(sign == 1, -1.0, 1.0) * GRID[mag] * np.ldexp(1.0, Xe)
    r16 = recv.astype(F16)
    assert np.array_equal(r16.astype(F64)[fin], recv[fin]), "decode is not exact in fp16"
    assert (np.abs(recv)[fin] <= 49152).all()
    err = np.abs(recv - np.where(fin, d, 0))
    bound = np.where(y > 6, 2.0, 1.0) * np.ldexp(1.0, Xe)
    assert not (fin & (err > bound)).any(), "reconstruction further from the delta than the grid allows"
    if state is not None:
        st = np.asarray(state).view(np.uint16).reshape(N, C) if np.asarray(state).dtype != np.uint16 else np.asarray(state).reshape(N, C)
        if not ef:
            want = np.ascontiguousarray(x).view(np.uint16)
            assert np.array_equal(st, want), "state without error feedback is not x"
            return
        if base is None:
            want = np.ascontiguousarray(r16).view(np.uint16)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                want = np.ascontiguousarray((base.astype(F64) + recv).astype(F16)).view(np.uint16)
        assert np.array_equal(st[fin], want[fin]), "state != fp16(base + decode(packet))"
        assert ((st[~fin] & 0x7FFF) > 0x7C00).all(), "a non-finite block's state is not NaN"
