"""Child process of tests/test_gpu_lr_receiver.py::test_factor_quantiser_against_the_int4_contract: loads libcfx_dev.so (use_dev_library()
before the first load) and runs k_lr_q4 ALONE on given matrices through cfx_dev_lr_q4 (include/cfx_dev.h).

Inputs: the int4 VALUE cases of tests/_value_cases.py as rows x r matrices, r in 8 / 16 / 24 / 32, through the U slot (rows 2, 66, 1022,
1024, 4100: one, one, one, two and eight row shares with uneven p0 .. p1 splits) and through the V^T slot (always six shares; a V^T has
C rows and C % 8 == 0, so the rows there are 8 - shares left empty -, 72, 1016, 1024, 4104).  Expected: oracle/ref_np.py
compress("int4", M, None), the pinned oracle tests/test_value_domain_f64.py holds to float64 - codes, scale and min of both sections bit
for bit (the one allowance of the int4 contract: which zero a both-signed zero minimum keeps, tests/_zero_min.py, on the channels the case
plants one in), the dequantised factors (want_dq) bit for bit, left untouched without want_dq.  Then q4 -> dq4 -> decode is closed: the
sections go through lr_decompress_batch(True, ...) against the witness, wherever U V stays finite."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

ROWS = [(2, 8), (66, 72), (1022, 1016), (1024, 1024), (4100, 4104)]       # (N: the U slot, C: the V^T slot)
RANKS = (8, 16, 24, 32)
NAMES = ("extremes-placed", "constant-channels", "signed-zero-extremes", "offset", "tiny", "wide", "range-overflow", "rint-ties")
FINITE_PRODUCT = ("extremes-placed", "constant-channels", "signed-zero-extremes", "tiny", "rint-ties")     # |U| |V| < 65504: decode's domain
DECODE_UP_TO = 1022
CANARY = 0x7E00


def main():
    import numpy as np
    import torch

    from compactfusion_amd import _lib
    _lib.use_dev_library()
    from compactfusion_amd import codecs as K
    import _gpu_codec as GC
    import _lr_f64_check as W
    import _nonfinite as NF
    import _value_cases as VC
    import _zero_min as Z
    from oracle import ref_np as R

    lib = _lib.load()
    assert hasattr(lib, "cfx_dev_lr_q4"), "the developer library was not loaded"
    ctx = K.context(0)
    sh = torch.cuda.current_stream().cuda_stream
    B = len(NAMES)
    arr = lambda ts: (ctypes.c_void_p * B)(*[t.data_ptr() for t in ts])      # noqa: E731
    n_dec = 0
    for r in RANKS:
        for N, C in ROWS:
            # (the value cases plant columns up to index 8: an 8-column matrix is the first 8 columns of the 16-column one - every case's
            # properties, and signed_zero_channels, are per column)
            mat = lambda n, rows, rep: np.ascontiguousarray(VC.build(n, "int4", rows, max(r, 16), rep=rep, nobase=True)[0][:, :r])      # noqa: E731
            Ms = [(mat(n, N, 0), mat(n, C, 1)) for n in NAMES]
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                want = [(R.compress("int4", mu, None), R.compress("int4", mv, None)) for mu, mv in Ms]
            ud, vd = [GC.dev(mu) for mu, _ in Ms], [GC.dev(mv) for _, mv in Ms]
            nu, nv = N * r // 4 + 2 * r, C * r // 4 + 2 * r                  # halves of the two sections
            assert 2 * (nu + nv) == lib.cfx_lr_packet_bytes(1, N, C, r)
            for want_dq in (1, 0):
                pk = [torch.full((nu + nv + 16,), CANARY, dtype=torch.int16, device="cuda") for _ in range(B)]
                uq = [torch.full((N + 2, r), CANARY, dtype=torch.int16, device="cuda") for _ in range(B)]
                vq = [torch.full((C + 2, r), CANARY, dtype=torch.int16, device="cuda") for _ in range(B)]
                ids = GC._profile(ctx, lib, lambda: K._check(ctx, lib.cfx_dev_lr_q4(ctx, N, C, r, want_dq, B, arr(ud), arr(vd), arr(pk), arr(uq), arr(vq), sh),
                                                             "cfx_dev_lr_q4"))
                assert ids == [11], ids                                       # one launch, the int4 quantiser's id
                assert lib.cfx_gate_errors(ctx) == 0
                for i, name in enumerate(NAMES):
                    what = f"{name} r={r} N={N} C={C} want_dq={want_dq}"
                    got = pk[i].cpu().numpy().view(np.uint16)
                    assert (got[nu + nv:] == CANARY).all(), what + ": wrote behind the packet"
                    for sec, (pw, recv), M, rows, tag in ((got[:nu], want[i][0], Ms[i][0], N, "U"), (got[nu:nu + nv], want[i][1], Ms[i][1], C, "V^T")):
                        used = Z.same_packet("int4", sec, pw, M, None, f"{what} section {tag}")
                        assert used <= VC.signed_zero_channels(name, rows, r), (what, tag, sorted(used))
                    for t, M, (pw, recv), rows in ((uq[i], Ms[i][0], want[i][0], N), (vq[i], Ms[i][1], want[i][1], C)):
                        g = t.cpu().numpy().view(np.uint16)
                        assert (g[rows:] == CANARY).all(), what + ": wrote behind a dequantised factor"
                        if want_dq:
                            NF.same_bits(g[:rows], R.bits(recv), what + ": dequantised factor")
                        else:
                            assert (g == CANARY).all(), what + ": dequantised factors written without want_dq"
                    same_in = np.array_equal(GC.host(ud[i]), Ms[i][0].view(np.uint16)) and np.array_equal(GC.host(vd[i]), Ms[i][1].view(np.uint16))
                    assert same_in, what + ": the input factors changed"
                if not want_dq or N > DECODE_UP_TO:
                    continue
                # q4 -> dq4 -> decode: the kernel's own sections through the receiver, against the witness
                sel = [i for i, n in enumerate(NAMES) if n in FINITE_PRODUCT]
                pks = [pk[i][:nu + nv].clone().view(torch.float16) for i in sel]
                recs = [torch.full((N, C), CANARY, dtype=torch.int16, device="cuda").view(torch.float16) for _ in sel]
                K.lr_decompress_batch(True, pks, [None] * len(sel), recs, N, C, r)
                torch.cuda.synchronize()
                for j, i in enumerate(sel):
                    W.check_q(GC.host(pks[j]), N, C, r, None, GC.host(recs[j]).reshape(N, C), f"{NAMES[i]} r={r} N={N} C={C}: q4 -> dq4 -> decode")
                    n_dec += 1
    assert n_dec == len(RANKS) * 3 * len(FINITE_PRODUCT)
    print("ok")


if __name__ == "__main__":
    main()
