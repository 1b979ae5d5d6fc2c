"""One rank PROCESS of the MXINT8 codec's peer-to-peer exchange-layer test (tests/test_gpu_mxint8.py starts two of them on one
GPU, each under its own time limit): the rank's packets live in cfx_ipc_alloc memory the other rank has opened,
cfx_plan_add_exchange_layer_p2p with codec 16 (0x110 for bf16 tensors) exchanges inside the layer launch (k_mxi8_layer reads the peer's code
words and scales with system-scope loads).
usage: mxint8_p2p_rank.py RANK WORLD TMPDIR N C STEPS BF16"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main(r, W, tmp, N, C, steps, bf):
    from compactfusion_amd import _lib, codecs as K
    torch.cuda.set_device(0)
    lib = _lib.load()
    ctx = lib.cfx_create(0)
    assert lib.cfx_prepare(ctx) == 0 and lib.cfx_set_gate_timeout_ms(ctx, 4000) == 0
    L = 2
    dt = torch.bfloat16 if bf else torch.float16
    cabi = K.codec_arg(K.Codec.MXINT8, dt)
    slot = (K.packet_bytes(cabi, N, C, 0) + 255) // 256 * 256
    flags_off = L * 2 * slot
    ptr, handle = ctypes.c_void_p(), ctypes.create_string_buffer(64)
    assert lib.cfx_ipc_alloc(ctx, flags_off + 2 * L * 64, ctypes.byref(ptr), handle) == 0, lib.cfx_last_error_string(ctx)
    with open(os.path.join(tmp, f"h{r}.tmp"), "wb") as f:
        f.write(handle.raw)
    os.replace(os.path.join(tmp, f"h{r}.tmp"), os.path.join(tmp, f"h{r}.bin"))
    peers = {}
    for q in range(W):
        if q == r:
            continue
        fn = os.path.join(tmp, f"h{q}.bin")
        t0 = time.time()
        while not os.path.exists(fn):
            assert time.time() - t0 < 60, "peer never published its handle"
            time.sleep(0.01)
        pp = ctypes.c_void_p()
        assert lib.cfx_ipc_open(ctx, open(fn, "rb").read(), ctypes.byref(pp)) == 0, lib.cfx_last_error_string(ctx)
        peers[q] = pp.value
    g = torch.Generator(device="cuda").manual_seed(77)
    x0 = torch.randn(W, L, 2, N, C, generator=g, device="cuda").to(dt)              # the same in every process
    xs = [(x0.float() + 0.1 * (s + 1) * torch.randn(W, L, 2, N, C, generator=g, device="cuda")).to(dt) for s in range(2)]
    own = x0[r].clone()
    peer = {q: x0[q].clone() for q in peers}
    assert lib.cfx_workspace_bytes(cabi, N, C, 0, 2) == 0              # no workspace: NULL / 0
    h = ctypes.c_void_p()
    assert lib.cfx_stream_create_masked(ctx, (256 // W) * r, 256 // W, ctypes.byref(h)) == 0      # each rank its share of the CUs
    run = h.value
    torch.cuda.synchronize()
    plans = []
    for s in range(2):
        plan = lib.cfx_plan_create(ctx)
        for l in range(L):
            c = (_lib.CompItem * 2)(*[_lib.CompItem(xs[s][r, l, b].data_ptr(), own[l, b].data_ptr(), own[l, b].data_ptr(), ptr.value + (l * 2 + b) * slot)
                                      for b in range(2)])
            items = [_lib.DecompItem(peers[q] + (l * 2 + b) * slot, peer[q][l, b].data_ptr(), peer[q][l, b].data_ptr()) for q in peers for b in range(2)]
            d = (_lib.DecompItem * len(items))(*items)
            pf = (ctypes.c_void_p * len(peers))(*[peers[q] + flags_off + (s * L + l) * 64 for q in peers])
            rc = lib.cfx_plan_add_exchange_layer_p2p(plan, cabi, N, C, 0, _lib.FLAG_UPDATE_CACHE, 2, c, len(items), d,
                                                     ptr.value + flags_off + (s * L + l) * 64, len(peers), pf, None, 0)
            assert rc >= 0, (rc, lib.cfx_last_error_string(ctx))
        plans.append(plan)
    for i in range(steps):
        rc = lib.cfx_plan_run(plans[i & 1], 0, L, run)
        assert rc == 0, (rc, lib.cfx_last_error_string(ctx))
    torch.cuda.synchronize()
    assert lib.cfx_gate_errors(ctx) == 0, "an in-launch wait timed out"

    def u16(t):
        return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    np.save(os.path.join(tmp, f"own{r}.npy"), u16(own))
    for q in peer:
        np.save(os.path.join(tmp, f"peer{r}_{q}.npy"), u16(peer[q]))
    np.save(os.path.join(tmp, f"x0_{r}.npy"), u16(x0[r]))
    for s in range(2):
        np.save(os.path.join(tmp, f"xs{s}_{r}.npy"), u16(xs[s][r]))
    # the peer reads this rank's packets in place: do not free them before it has finished
    open(os.path.join(tmp, f"done{r}"), "w").close()
    t0 = time.time()
    while not all(os.path.exists(os.path.join(tmp, f"done{q}")) for q in peers):
        assert time.time() - t0 < 60, "peer never finished"
        time.sleep(0.01)
    for p in plans:
        lib.cfx_plan_destroy(p)
    for q in peers:
        lib.cfx_ipc_close(ctx, ctypes.c_void_p(peers[q]))
    lib.cfx_ipc_free(ctx, ptr)
    lib.cfx_stream_destroy(ctx, ctypes.c_void_p(run))


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]), int(a[1]), a[2], int(a[3]), int(a[4]), int(a[5]), int(a[6]) != 0)
