"""The contract of the low-rank SENDER's factor chains (csrc/cfx_lrslab.hip, csrc/cfx_lrgram.hip, csrc/cfx_lowrank.hip) in float64
numpy - independent of compactfusion_amd/compact/compress_lowrank.py, whose float32 port it MEASURES.

It works on A = fp16(x - base) (one rounding, as the kernels form it), the start matrix Q0 and the fp16 factors U16 (N, r), V16 (r, C)
of the packet.  Every bound is either derived from the number formats or computed from the reference alone, per case:

    floor   what the float64 replay's OWN factors lose when rounded to fp16 (no chain can send better factors than that)
    port    how far the float32 port of the reference iteration is from the float64 replay on the same case

 b. projection     rel(U16 V16, P_ref) <= 2 floor + 8 port, globally and as the worst row and the worst column (norm of that row / column of
                   the difference over the RMS row / column norm of P_ref); P_ref = U (U^T A) of the replay: Householder QR, two
                   iterations from Q0, U = qr(A Q), V = U^T A.
                   2 floor: the kernels' U is the replay's up to column signs, its rounding is another draw of the same size, and the worst
                   row is the maximum of such draws.  8 port = 4 x 2: the kernels keep 22 bits of an operand (fp16 hi + lo, or tagged
                   words) where float32 keeps 24, and sum in an order of their own.
 c. orthonormality max |U16^T U16 - diag(d)| <= 2^-10 + 8 port: |sum_n u_nk du_nj| <= 2^-11 sum |u_nk| |u_nj| <= 2^-11 by Cauchy-Schwarz,
                   twice (du on either side); never above the 5e-3 tests/test_gpu_lowrank_slab.py has always asked
 d. coefficients   ||V16[k] - U16[:, k]^T A|| <= ||half ulp(V16[k])|| + 2^-11 || |U16[:, k]|^T |A| || + 8 port: the chain's V is u^T A of
                   the UNROUNDED u, so the two roundings are all that separates them (flat cases)
 e. deficient      rank(A) < r: U16 V16 = A within (b) (P_ref is A itself), a dropped direction is an all-zero column of U and row of V

`graded` cases keep the fixed 3e-3 / 5e-3 of tests/test_gpu_lowrank_slab.py, no lower: on a decaying spectrum the small directions are
resolved to fewer bits by any single-precision chain, and what tests/test_gpu_lowrank_slab.py asks of them stays what it is."""
import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
GRADED_TOL, ORTH_CAP = 3e-3, 5e-3
FLOOR_X, PORT_X = 2.0, 8.0


def replay(A, Q0, iters=2, fault=None):
    """the reference iteration in float64 (numpy's QR is LAPACK's Householder).  `fault(name, M, ctx)` may replace any product:
    names Y0, Z0, Y1, Z1, .. (Y_i = A Q_i, Z_i = A^T Y_i), Ylast, U, V; ctx holds what the product was made from."""
    A = np.asarray(A, dtype=F64)
    Q = np.asarray(Q0, dtype=F64)
    f = fault or (lambda name, M, ctx: M)
    Yprev = Qprev = None
    for i in range(iters):
        Y = f(f"Y{i}", A @ Q, dict(A=A, Q=Q, Qprev=Qprev))
        Z = f(f"Z{i}", A.T @ Y, dict(A=A, Y=Y, Yprev=Yprev))
        Yprev, Qprev = Y, Q
        Q = np.linalg.qr(Z)[0]
    Y = f("Ylast", A @ Q, dict(A=A, Q=Q))
    U = f("U", np.linalg.qr(Y)[0], {})
    V = f("V", U.T @ A, {})
    return U, V


def _port(A, Q0, rank):
    """the float32 port (library GEMM / QR through PyTorch on the CPU), two iterations from the same start"""
    import torch
    from compactfusion_amd.compact.compress_lowrank import subspace_iter
    U, V, _ = subspace_iter(torch.from_numpy(np.array(A, dtype=F32)), rank, num_iters=2,
                            init_q=torch.from_numpy(np.array(Q0[:, :rank], dtype=F32)))
    return U.numpy().astype(F64), V.numpy().astype(F64)


def dist(P, Pref):
    """(global, worst row, worst column) distance of P from Pref"""
    E = P - Pref
    n = max(float(np.linalg.norm(Pref)), 1e-300)
    rms_r = max(float(np.sqrt((Pref ** 2).sum(1).mean())), 1e-300)
    rms_c = max(float(np.sqrt((Pref ** 2).sum(0).mean())), 1e-300)
    return np.array([np.linalg.norm(E) / n, np.sqrt((E ** 2).sum(1)).max() / rms_r, np.sqrt((E ** 2).sum(0)).max() / rms_c])


def r16(M):
    return np.asarray(M, dtype=F64).astype(F16).astype(F64)


def orth_err(U, d=None):
    G = U.T @ U
    return float(np.abs(G - np.diag(np.ones(U.shape[1]) if d is None else d)).max())


def coef_err(U, V, A):
    """(r,) ||V[k] - U[:, k]^T A|| over ||A||_F / sqrt(r)"""
    return np.linalg.norm(V - U.T @ A, axis=1) / (np.linalg.norm(A) / np.sqrt(U.shape[1]))


class Ref:
    """everything the contract needs of one case, from the reference alone"""

    def __init__(self, A16, Q0, rank, kind):
        assert kind in ("flat", "graded", "deficient")
        self.kind, self.rank = kind, rank
        self.A = A = np.asarray(A16, dtype=F16).astype(F64)
        N, C = A.shape
        if kind == "deficient":
            # rank(A) < r: the iterated subspace holds all of A's range, the projection is A.  Factors of the same kind from an SVD:
            # in float64 for the floor, in float32 for what single precision costs
            self.P = A
            k = int(np.linalg.matrix_rank(A))
            assert k < rank, (k, rank)
            self.rankA = k
            if k == 0:
                self.floor, self.port, self.port_orth, self.port_coef = np.zeros(3), np.zeros(3), 0.0, 0.0
                return
            Us = np.linalg.svd(A, full_matrices=False)[0][:, :k]
            U32 = np.linalg.svd(A.astype(F32), full_matrices=False)[0][:, :k]
            Up, Vp = U32.astype(F64), (U32.T @ A.astype(F32)).astype(F64)
            Ur, Vr = Us, Us.T @ A
        else:
            Ur, Vr = replay(A, Q0[:, :rank])
            self.P = Ur @ Vr
            Up, Vp = _port(A, Q0, rank)
        self.Ur, self.Vr = Ur, Vr
        self.floor = dist(r16(Ur) @ r16(Vr), self.P)
        self.port = dist(Up @ Vp, self.P)
        self.port_orth = orth_err(Up)
        self.port_coef = float(coef_err(Up, Vp, A).max())

    def proj_bound(self):
        """(global, row, column)"""
        if self.kind == "graded":
            return np.array([GRADED_TOL, np.inf, np.inf])
        return FLOOR_X * self.floor + PORT_X * self.port

    def orth_bound(self):
        return ORTH_CAP if self.kind == "graded" else min(2.0 ** -10 + PORT_X * self.port_orth, ORTH_CAP)


def half_ulp16(V16):
    return np.spacing(np.abs(np.asarray(V16, dtype=F16))).astype(F64) / 2


def measure(ref, U16, V16):
    """the figures of the contract and their bounds: {item: (value, bound)}; `finite` and `dropped` are booleans against True"""
    U16, V16 = np.asarray(U16, dtype=F16), np.asarray(V16, dtype=F16)
    r = ref.rank
    assert U16.shape == (ref.A.shape[0], r) and V16.shape == (r, ref.A.shape[1])
    out = {"finite": (bool(np.isfinite(U16).all() and np.isfinite(V16).all()), True)}
    if not out["finite"][0]:
        return out
    U, V = U16.astype(F64), V16.astype(F64)
    d = np.ones(r)
    if ref.kind == "deficient":
        # a direction is either kept (a unit column) or dropped (an all-zero column of U AND row of V): nothing in between
        zu, zv = ~U16.astype(bool).any(0), ~V16.astype(bool).any(1)
        d = (~zu).astype(F64)
        out["dropped"] = (bool(np.array_equal(zu, zv) and int(d.sum()) >= ref.rankA), True)
    g, row, col = dist(U @ V, ref.P)
    bg, br, bc = ref.proj_bound()
    out["proj"], out["proj_row"], out["proj_col"] = (g, bg), (row, br), (col, bc)
    out["orth"] = (orth_err(U, d), ref.orth_bound())
    if ref.kind == "flat":
        scale = np.linalg.norm(ref.A) / np.sqrt(r)
        e = np.linalg.norm(V - U.T @ ref.A, axis=1)
        b = np.linalg.norm(half_ulp16(V16), axis=1) + 2.0 ** -11 * np.linalg.norm(np.abs(U).T @ np.abs(ref.A), axis=1) \
            + PORT_X * ref.port_coef * scale
        k = int(np.argmax(e / b))
        out["coef"] = (float(e[k] / scale), float(b[k] / scale))
    return out


def ratios(m):
    return {k: (v / b if b else (0.0 if v == 0 else np.inf)) for k, (v, b) in m.items() if not isinstance(v, bool)}


def failures(m):
    bad = []
    for k, (v, b) in m.items():
        if isinstance(v, bool):
            if v is not b:
                bad.append(f"{k}: {v}")
        elif not v <= b:
            bad.append(f"{k}: {v:.3e} > {b:.3e}")
    return bad


def check(ref, U16, V16, what=""):
    m = measure(ref, U16, V16)
    bad = failures(m)
    assert not bad, f"{what}: " + "; ".join(bad)
    return m


def split(packet16, N, C, r):
    p = np.asarray(packet16).reshape(-1)
    p = p.view(F16) if p.dtype == np.uint16 else p
    assert p.size == (N + C) * r
    return p[:N * r].reshape(N, r), p[N * r:].reshape(r, C)


# ---- planted faults: one product of the float64 replay goes wrong the way a kernel's branch could ---------------------------------------
def fault_rows(N, C):
    """rows the last row split of k_lr_aty owns (one split: N / 32 rows, at least one)"""
    import _lr_sender_cases as SC
    ns, rps, nz = SC.aty_splits(N, C)
    return N - rps * (nz - 1) if nz > 1 else max(1, N // 32)


def fault_cols(C):
    """columns of the last partial 32-column tile (a whole number of tiles: the last 8, the width of one lane's load)"""
    return C % 32 or 8


def planted(name, N, C, r):
    """-> (fault for replay(), post(U, V) on the factors) or None where the shape has no such branch"""
    ident = lambda U, V: (U, V)
    if name == "last row split dropped":                                   # Z1 = A^T Y1 without its last rows
        n0 = N - fault_rows(N, C)
        if n0 <= 0:
            return None
        return (lambda nm, M, c: c["A"][:n0].T @ c["Y"][:n0] if nm == "Z1" else M), ident
    if name == "last partial column tile dropped":                         # Y1 = A Q1 without its last columns
        c0 = C - fault_cols(C)
        if c0 <= 0:
            return None
        return (lambda nm, M, c: c["A"][:, :c0] @ c["Q"][:c0] if nm == "Y1" else M), ident
    if name == "a column group's chunk skipped":                           # Y1 = A Q1 without its last 256-column chunk
        c0 = (C - 1) // 256 * 256
        if c0 == 0:
            return None
        return (lambda nm, M, c: c["A"][:, :c0] @ c["Q"][:c0] if nm == "Y1" else M), ident
    if name == "stale partial":                                            # the last row split's partial of Z1 is the one Z0 left: made of Y0
        import _lr_sender_cases as SC
        n0, c0 = N - fault_rows(N, C), (C - 1) // 256 * 256
        if SC.aty_splits(N, C)[2] > 1:
            return (lambda nm, M, c: c["A"][:n0].T @ c["Y"][:n0] + c["A"][n0:].T @ c["Yprev"][n0:] if nm == "Z1" else M), ident
        if c0 == 0:                                                        # one row split and one column chunk: no sum is made of partials
            return None
        # ... or the last 256-column chunk's share of Y1 is the one Y0 left: made of Q0
        return (lambda nm, M, c: c["A"][:, :c0] @ c["Q"][:c0] + c["A"][:, c0:] @ c["Qprev"][c0:] if nm == "Y1" else M), ident
    if name == "stale product":                                            # Z1 = A^T Y0 altogether: an iteration lost (see LOST_ITERATION)
        return (lambda nm, M, c: c["A"].T @ c["Yprev"] if nm == "Z1" else M), ident
    if name == "a row of V scaled by 1 + 2^-8":
        def post(U, V):
            V = V.copy()
            V[r - 1] *= 1 + 2.0 ** -8
            return U, V
        return (lambda nm, M, c: M), post
    if name == "two columns of U exchanged":
        def post(U, V):
            U = U.copy()
            U[:, [0, r - 1]] = U[:, [r - 1, 0]]
            return U, V
        return (lambda nm, M, c: M), post
    raise KeyError(name)


PRODUCT_FAULTS = ("last row split dropped", "last partial column tile dropped", "a column group's chunk skipped", "stale partial")
LOST_ITERATION = "stale product"      # not among the planted faults: on a flat spectrum A^T A is a multiple of the identity on the residual's
#                                       directions, one iteration more or less spans the same subspace - the graded cases are there for it
FACTOR_FAULTS = ("a row of V scaled by 1 + 2^-8", "two columns of U exchanged")


def faulty_factors(ref, Q0, name):
    """the fp16 factors a chain with the planted fault would send, or None"""
    N, C = ref.A.shape
    p = planted(name, N, C, ref.rank)
    if p is None:
        return None
    U, V = replay(ref.A, Q0[:, :ref.rank], fault=p[0])
    U, V = p[1](U, V)
    return U.astype(F16), V.astype(F16)


# ---- one reference per case, shared by every test that needs it (computed once, never written to) -----------------------------------------
_refs = {}


def case(kind, N, C, rank, key=0, **kw):
    """-> (x, base, q0, Ref) of flat(N, C, rank, rep = key), graded_np(N, C, rank, seed = key) or deficient(form = key, N, C, rank)"""
    import _lr_sender_cases as SC
    k = (kind, N, C, rank, key, tuple(sorted(kw.items())))
    if k not in _refs:
        if kind == "flat":
            x, base, q0 = SC.flat(N, C, rank, key)
        elif kind == "graded":
            x, base, q0 = SC.graded_np(N, C, rank, key, **kw)
        else:
            x, base, q0 = SC.deficient(key, N, C, rank)
        for a in (x, base, q0):
            a.setflags(write=False)
        _refs[k] = (x, base, q0, Ref(SC.residual(x, base), q0, rank, kind))
    return _refs[k]
